"""The anti-aliased downscale and the folder scorer without a GPU: the NumPy restatement (tests/_postprocess_aa_ref.py) against
the fixtures recorded from scipy (tools/gen_postprocess_aa_golden.py), ``postprocess.gaussian_weights`` against scipy's own
tables, the argument checks of the two new entry points of the C ABI, which precede any launch, ``evaluate.pair_files`` on trees
of empty files, and the table ``evaluate.write_csv`` writes.

Bars.  Weights and the Gaussian stage: exact (scipy's float32 result, bit for bit).  float64 zoom: |d| <= 1e-12, float32: one
float32 step below 2, the bars of test_postprocess_host.py: the spline that follows the Gaussian is the same one."""
import csv
import os

import numpy as np
import pytest
import torch

from diff_sal_amd import _lib, evaluate
from diff_sal_amd import eval_metrics as em
from diff_sal_amd import postprocess as pp
from tests import _postprocess_aa_ref as ref

CASES = ref.load_cases()
F64_BAR = 1e-12


def _map(name):
    return ref.big_input() if name in ref.BIG else CASES[name]["map"]


def test_fixture_cases_are_the_ones_the_checks_need():
    shapes = {n: (tuple(_map(n).shape), c["size"]) for n, c in CASES.items()}
    assert shapes == {"a8x12": ((2, 8, 12), (7, 9)), "a16x24": ((1, 16, 24), (7, 24)), "a12x20": ((2, 12, 20), (15, 11)),
                      "a6x7": ((1, 6, 7), (1, 2)), "a5x200": ((1, 5, 200), (5, 20)), "a70x33": ((1, 70, 33), (20, 33)),
                      "a33x70": ((3, 33, 70), (16, 35)), "edge12x20": ((1, 12, 20), (8, 13)),
                      "big_strong": ((2, 224, 384), (100, 120)), "big_mild": ((2, 224, 384), (180, 320))}
    radii = {n: tuple(0 if c[k] is None else len(c[k]) - 1 for k in ("wy", "wx")) for n, c in CASES.items()}
    assert radii == {"a8x12": (0, 1), "a16x24": (3, 0), "a12x20": (0, 2), "a6x7": (10, 5), "a5x200": (0, 18), "a70x33": (5, 0),
                     "a33x70": (2, 2), "edge12x20": (1, 1), "big_strong": (2, 4), "big_mild": (0, 0)}
    assert CASES["a16x24"]["wx"] is None and CASES["a12x20"]["wy"] is None                 # an axis that does not shrink: no table
    assert CASES["a8x12"]["wy"] is not None and np.array_equal(CASES["a8x12"]["wy"], [1.0])      # sigma > 0, radius 0: the identity
    flat = CASES["a33x70"]["map"][1]
    assert flat.min() == flat.max()                                                        # a flat image among non-flat neighbours
    e = CASES["edge12x20"]
    assert e["filtered"].max() < e["map"].max() == 1.0                                     # the Gaussian lowers the maximum ...
    assert e["zoom3_f64"].max() > 1.0 > e["filtered"].max() and e["zoom3_f64"].min() < 0.0      # ... and the cubic overshoots both ends
    assert e["clip3_f64"].max() == 1.0 and e["clip3_f64"].min() == 0.0                     # clipped to the UNFILTERED range


@pytest.mark.parametrize("name", sorted(CASES))
def test_gaussian_weights_equal_the_recorded_tables(name):
    c = CASES[name]
    (h, w), (H, W) = _map(name).shape[1:], c["size"]
    for got, mine, want in ((pp.gaussian_weights(h, H), ref.gaussian_weights(h, H), c["wy"]),
                            (pp.gaussian_weights(w, W), ref.gaussian_weights(w, W), c["wx"])):
        if want is None:
            assert got is None and mine is None
        else:
            assert got.dtype == np.float64 and np.array_equal(got, want) and np.array_equal(mine, want)


def test_gaussian_weights_limits():
    assert pp.gaussian_weights(10, 10) is None and pp.gaussian_weights(10, 25) is None
    assert len(pp.gaussian_weights(330, 10)) == 65                       # factor 33: sigma 16, radius 64: the largest taken
    with pytest.raises(ValueError, match="radius 65"):
        pp.gaussian_weights(3325, 100)                                   # factor 33.25: sigma 16.125, radius 65
    with pytest.raises(ValueError, match="at least 1"):
        pp.gaussian_weights(10, 0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_scipy_fixtures(name):
    c = CASES[name]
    m = _map(name)
    worst = 0.0
    for b in range(m.shape[0]):
        f = ref.gauss(m[b], c["wy"], c["wx"])
        assert f.dtype == np.float32 and np.array_equal(f[c["frows"]][:, c["fcols"]], c["filtered"][b]), (name, b)      # exact
        for order in ref.ORDERS:
            for clip, key in ((False, "zoom"), (True, "clip")):
                got = ref.resize_aa(m[b], c["size"], order=order, clip=clip)[c["rows"]][:, c["cols"]]
                d = float(np.abs(got - c[f"{key}{order}_f64"][b]).max())
                worst = max(worst, d)
                assert d <= F64_BAR, (name, order, b, key, d)
                d32 = np.abs(got.astype(np.float32).astype(np.float64) - c[f"{key}{order}_f32"][b].astype(np.float64)).max()
                assert d32 <= 2.0 ** -23, (name, order, b, key, d32)
    print(f"{name}: worst float64 |d| = {worst:.2e}")


def test_restatement_equals_scipy_directly():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    for (h, w), (H, W) in (((9, 14), (4, 5)), ((40, 64), (9, 13)), ((2, 2), (1, 1)), ((12, 20), (15, 11))):
        x = rng.random((h, w), dtype=np.float32)
        sigma = (max(0.0, (h / H - 1) / 2), max(0.0, (w / W - 1) / 2))
        want = ndimage.gaussian_filter(x, sigma, mode="mirror")
        got = ref.gauss(x, ref.gaussian_weights(h, H), ref.gaussian_weights(w, W))
        assert np.array_equal(got, want), ((h, w), (H, W), int((got != want).sum()))
        for order in ref.ORDERS:
            z = ndimage.zoom(want.astype(np.float64), (H / h, W / w), order=order, mode="mirror", grid_mode=True)
            d = float(np.abs(ref.resize_aa(x, (H, W), order=order, clip=False) - z).max())
            print(f"{h} x {w} -> {H} x {W} order {order}: |d| = {d:.2e}")
            assert d <= F64_BAR


def test_argument_errors_are_reported_without_a_gpu():
    import ctypes as C

    lib = _lib.load()
    P = 256      # never dereferenced: every check precedes the first launch
    g = (C.c_double * 66)(*([1.0] + [0.0] * 65))
    BIG = 1 << 30

    def aa(h=8, w=8, H=5, W=9, order=3, B=1, clip=1, f64=0, wy=g, ry=1, wx=None, rx=0, inp=P, out=P, ws=P, nws=BIG):
        return lib.diffsal_map_resize_aa(inp, B, h, w, H, W, order, clip, f64, wy, ry, wx, rx, out, ws, nws, None)

    def gauss(h=8, w=8, B=1, wy=g, ry=1, wx=g, rx=1, inp=P, out=512, ws=P, nws=BIG):
        return lib.diffsal_map_gauss(inp, B, h, w, wy, ry, wx, rx, out, ws, nws, None)

    assert aa(inp=None) == -4 and aa(out=None) == -4 and aa(ws=None) == -4                              # null pointers
    assert aa(wy=None) == -4 and b"without its weights" in lib.diffsal_last_error()                     # a radius without its table
    assert aa(wx=None, rx=2) == -4 and aa(ry=-1) == -4
    assert aa(ry=65) == -1 and b"factor below 33" in lib.diffsal_last_error()                           # radius 65
    assert aa(wx=g, rx=65) == -1 and b"above 64" in lib.diffsal_last_error()
    assert aa(H=0) == -1 and aa(W=0) == -1 and aa(H=-3) == -1 and b"target" in lib.diffsal_last_error()     # H = 0
    assert aa(H=40000) == -1 and aa(h=40000) == -1
    assert aa(h=1) == -1 and b"at least 2 samples" in lib.diffsal_last_error()
    assert aa(B=0) == -1 and aa(B=65536) == -1
    for order in (0, 2, 4):
        assert aa(order=order) == -4 and b"order" in lib.diffsal_last_error()
    assert aa(clip=2) == -4 and aa(f64=7) == -4
    assert aa(nws=16) == -4 and b"workspace" in lib.diffsal_last_error()                                # a workspace too small
    assert aa(ws=P + 4) == -4 and b"misaligned" in lib.diffsal_last_error()
    assert gauss(inp=None) == -4 and gauss(out=None) == -4 and gauss(ws=None) == -4 and gauss(out=P) == -4
    assert gauss(wy=None) == -4 and gauss(wx=None) == -4
    assert gauss(ry=65) == -1 and gauss(rx=65) == -1 and b"factor below 33" in lib.diffsal_last_error()
    assert gauss(h=1) == -1 and gauss(w=1) == -1 and gauss(B=0) == -1 and gauss(h=40000) == -1
    assert gauss(nws=16) == -4 and b"workspace" in lib.diffsal_last_error()
    # the upscale-only entry point still refuses a downscale
    assert lib.diffsal_map_resize(P, 1, 8, 8, 5, 9, 3, 1, 0, P, P, BIG, None) == -1 and b"shrinks an axis" in lib.diffsal_last_error()
    assert lib.diffsal_map_resize(P, 1, 8, 8, 9, 7, 1, 1, 0, P, P, BIG, None) == -1 and b"shrinks an axis" in lib.diffsal_last_error()
    # workspace sizes: the upscale's layout plus two [B][h][w] float32 arrays; host arithmetic only
    n, B = 224 * 384, 64
    for order in (1, 3):
        for clip in (0, 1):
            assert lib.diffsal_map_resize_aa_ws_bytes(B, 224, 384, order, clip) == lib.diffsal_map_resize_ws_bytes(B, 224, 384, order, clip) + 2 * B * n * 4
    assert lib.diffsal_map_resize_aa_ws_bytes(3, 33, 70, 1, 0) == 2 * ((3 * 33 * 70 * 4 + 15) // 16 * 16)      # each array on 16 bytes
    assert lib.diffsal_map_resize_aa_ws_bytes(B, 224, 384, 2, 0) == 0 and lib.diffsal_map_resize_aa_ws_bytes(0, 224, 384, 3, 0) == 0
    assert lib.diffsal_map_gauss_ws_bytes(B, 224, 384) == B * n * 4 and lib.diffsal_map_gauss_ws_bytes(B, 0, 384) == 0


def test_python_argument_errors_without_a_gpu():
    x = torch.zeros(1, 8, 8)
    for call in (lambda: pp.resize(x, (5, 9), anti_aliasing=True), lambda: pp.antialias(x, (5, 9))):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()


def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "wb").close()


def test_pair_files_dhf1k(tmp_path):
    pred, maps = tmp_path / "pred" / "task" / "601", tmp_path / "gt" / "annotation" / "0601" / "maps"
    for k in (1, 2, 10, 100):
        _touch(str(pred / f"{k}.png"))
        _touch(str(maps / f"{k:04d}.png"))
    _touch(str(pred / "notes.txt"))
    got = evaluate.pair_files(str(pred), str(maps) + "/", "dhf1k", 601)
    fix = tmp_path / "gt" / "annotation" / "0601" / "fixation"
    assert got == [(str(pred / f"{k}.png"), str(maps / f"{k:04d}.png"), str(fix / f"{k:04d}.png")) for k in (1, 10, 100, 2)]      # sorted as strings


def test_pair_files_ucf(tmp_path):
    vid = "Diving-Side-001"
    pred, maps = tmp_path / "pred" / "task" / vid, tmp_path / "ucf" / vid / "maps"
    for k in (1, 2, 12):
        _touch(str(pred / f"{k}.png"))
    got = evaluate.pair_files(str(pred), str(maps), "ucf", vid)
    fix = tmp_path / "ucf" / vid / "fixation"
    assert got == [(str(pred / f"{k}.png"), str(maps / f"Diving-Side_001_{k:03d}.png"), str(fix / f"Diving-Side_001_{k:03d}.png"))
                   for k in (1, 12, 2)]


def test_pair_files_holly(tmp_path):
    vid = "actioncliptest00003"
    pred, maps = tmp_path / "pred" / "task" / vid, tmp_path / "holly" / vid / "maps"
    names = [f"{vid}_{k:05d}" for k in (1, 2, 3)]
    for n in names:
        _touch(str(maps / f"{n}.png"))
    for k in (1, 3):
        _touch(str(pred / f"{k}.png"))
    fix = tmp_path / "holly" / vid / "fixation"
    got = evaluate.pair_files(str(pred), str(maps), "holly", vid)
    assert got == [(str(pred / f"{k}.png"), str(maps / f"{names[k - 1]}.png"), str(fix / f"{names[k - 1]}.png")) for k in (1, 3)]
    _touch(str(pred / "4.png"))      # beyond the annotation list: the reference reuses the previous frame's name
    with pytest.raises(ValueError, match=r"4\.png is prediction 4 of a video with 3 annotated frames"):
        evaluate.pair_files(str(pred), str(maps), "holly", vid)
    with pytest.raises(ValueError, match="data_type"):
        evaluate.pair_files(str(pred), str(maps), "avad", vid)


def test_csv_header_and_rounding(tmp_path):
    meter = em.VideoMeter()      # CPU tensors: the meter's arithmetic is the device path's
    meter.update("a", {"auc_judd": torch.tensor([0.91234, 0.91244], dtype=torch.float64), "cc": torch.tensor([0.5, 0.25], dtype=torch.float64),
                       "nss": torch.tensor([2.00005, 2.00005], dtype=torch.float64), "sim": torch.tensor([0.33333, 0.33334], dtype=torch.float64)})
    meter.update("b", {"auc_judd": torch.tensor([0.8], dtype=torch.float64), "cc": torch.tensor([0.125], dtype=torch.float64),
                       "nss": torch.tensor([1.0], dtype=torch.float64), "sim": torch.tensor([0.5], dtype=torch.float64)})
    row = meter.compute()
    want = {k: float(np.around(np.mean([np.mean(a), np.mean(b)]), 4)) for k, a, b in (
        ("auc_judd", [0.91234, 0.91244], [0.8]), ("cc", [0.5, 0.25], [0.125]), ("nss", [2.00005, 2.00005], [1.0]), ("sim", [0.33333, 0.33334], [0.5]))}
    assert row == want
    path = str(tmp_path / "pred_metrics.csv")
    evaluate.write_csv(path, {"task_a": row, "task_b": dict(row, auc_borji=0.7512)})
    with open(path, newline="") as f:
        lines = f.read().splitlines()
    assert lines[0] == "Task,AUC_J ,AUC_S ,CC ,NSS ,Sim"      # the reference's header, trailing blanks included
    rows = list(csv.reader(lines[1:]))
    assert [r[0] for r in rows] == ["task_a", "task_b"]
    assert [float(v) for v in rows[0][1:]] == [want["auc_judd"], 0.0, want["cc"], want["nss"], want["sim"]]      # AUC_S: 0.0 as the reference writes it
    assert [float(v) for v in rows[1][1:]] == [want["auc_judd"], 0.7512, want["cc"], want["nss"], want["sim"]]
    assert all(len(v.split(".")[-1]) <= 4 for r in rows for v in r[1:])      # four places at the most
