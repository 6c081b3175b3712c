"""The anti-aliased downscale and the folder scorer on the GPU (csrc/postprocess.hip through diff_sal_amd.postprocess and
diff_sal_amd.evaluate) against the fixtures recorded from scipy (tools/gen_postprocess_aa_golden.py) and against the NumPy
restatement (tests/_postprocess_aa_ref.py) on every pixel.

Bars.  The Gaussian stage: exact -- the float32 map scipy.ndimage.gaussian_filter returns, bit for bit (every float64 operation
of a sample is rounded on its own, in scipy's order, and the sample is rounded once).  Resize with float64 output: |d| <= 1e-12,
the bar of test_gpu_postprocess.py::test_resize_against_scipy: the spline behind the Gaussian is the same code on a map of the
same range.  Resize in float32: |d| <= 2^-23, one float32 step below 2; how many pixels differ from scipy's float32 at all is
printed, not asserted.  Metric rows: 1e-12 for the AUCs, 1e-9 for CC, NSS, SIM against the restatement applied to the DEVICE's
resized maps, as in test_gpu_postprocess.py.  The folder scorer against its own composition: exact."""
import csv
import math
import os

import numpy as np
import pytest
import torch

from diff_sal_amd import eval_metrics as em
from diff_sal_amd import evaluate, ops, png
from diff_sal_amd import postprocess as pp
from tests import _eval_metrics_ref as mref
from tests import _postprocess_aa_ref as ref
from tests import _postprocess_ref as upref

pytestmark = pytest.mark.gpu

F64_BAR, F32_BAR, AUC_BAR, MOMENT_BAR = 1e-12, 2.0 ** -23, 1e-12, 1e-9
DEV = "cuda"
CASES = ref.load_cases()
_MAPS, _FILTERED, _ZOOM = {}, {}, {}      # the restatement's results, computed once per case


def _map(name):
    if name not in _MAPS:
        _MAPS[name] = ref.big_input() if name in ref.BIG else CASES[name]["map"]
    return _MAPS[name]


def _filtered(name):
    if name not in _FILTERED:
        c = CASES[name]
        _FILTERED[name] = np.stack([ref.gauss(p, c["wy"], c["wx"]) for p in _map(name)])
    return _FILTERED[name]


def _zoom(name, order):
    if (name, order) not in _ZOOM:
        _ZOOM[name, order] = np.stack([ref.zoom(f, CASES[name]["size"], order) for f in _filtered(name)])
    return _ZOOM[name, order]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pick(a, rows, cols):
    return a[:, rows][:, :, cols]


@pytest.mark.parametrize("name", sorted(CASES))
def test_gaussian_stage_is_bit_equal_to_scipy(name):
    c = CASES[name]
    x = _t(_map(name))
    got = pp.antialias(x, c["size"])
    assert got.dtype == torch.float32 and got.shape == x.shape
    assert torch.equal(_pick(got, _t(c["frows"]), _t(c["fcols"])), _t(c["filtered"]))      # scipy's float32 map, at the recorded points
    assert torch.equal(got, _t(_filtered(name)))                                            # the restatement: every pixel
    assert torch.equal(got, ops.map_gauss(x, c["wy"], c["wx"]))                             # the recorded tables, passed as they are
    if name == "a33x70":
        assert torch.equal(got[1], x[1]) and float(x[1].min()) == float(x[1].max())          # the flat image stays flat
    if c["wy"] is None and c["wx"] is None or name == "big_mild":
        assert torch.equal(got, x)                                                          # no radius: a copy


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("order", ref.ORDERS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_resize_aa_against_scipy(name, order, clip):
    c = CASES[name]
    m = _map(name)
    key = f"{'clip' if clip else 'zoom'}{order}"
    x = _t(m)
    got64 = pp.resize(x, c["size"], order=order, clip=clip, dtype=torch.float64, anti_aliasing=True)
    got32 = pp.resize(x, c["size"], order=order, clip=clip, anti_aliasing=True)
    assert got64.dtype == torch.float64 and got32.dtype == torch.float32 and got64.shape == got32.shape == (m.shape[0],) + c["size"]
    got64, got32 = got64.cpu().numpy(), got32.cpu().numpy()
    full = _zoom(name, order)
    if clip:
        full = np.clip(full, m.reshape(len(m), -1).min(1).astype(np.float64)[:, None, None], m.reshape(len(m), -1).max(1).astype(np.float64)[:, None, None])
    pick = lambda a: _pick(a, c["rows"], c["cols"])      # noqa: E731
    d_fix = float(np.abs(pick(got64) - c[key + "_f64"]).max())
    d_all = float(np.abs(got64 - full).max())
    d32 = float(np.abs(pick(got32).astype(np.float64) - c[key + "_f32"].astype(np.float64)).max())
    d32_all = float(np.abs(got32.astype(np.float64) - full).max())
    n_diff = int((pick(got32) != c[key + "_f32"]).sum())
    print(f"{name} order {order} clip {clip}: f64 |d| fixture {d_fix:.2e} restatement {d_all:.2e}; f32 |d| fixture {d32:.2e}, "
          f"{n_diff} of {c[key + '_f32'].size} recorded pixels differ from scipy's float32 at all")
    assert np.array_equal(got32, got64.astype(np.float32))      # the float32 path is the float64 one rounded once
    assert d_fix <= F64_BAR and d_all <= F64_BAR
    assert d32 <= F32_BAR and d32_all <= F32_BAR


def test_an_upscale_with_the_keyword_is_the_default_call():
    c = upref.load_cases()["s7x12"]
    assert c["pred"].shape[1:] == (7, 12) and c["size"] == (11, 20)
    x = _t(np.stack([upref.from_uint8(upref.to_uint8(p)) for p in c["pred"]]))
    for size in ((11, 20), (7, 12), (7, 13)):      # both axes up, equal, one equal
        assert pp.gaussian_weights(7, size[0]) is None and pp.gaussian_weights(12, size[1]) is None
        for order in ref.ORDERS:
            for clip in (False, True):
                for dtype in (torch.float32, torch.float64):
                    want = pp.resize(x, size, order=order, clip=clip, dtype=dtype)
                    assert torch.equal(pp.resize(x, size, order=order, clip=clip, dtype=dtype, anti_aliasing=True), want)
                    # the new entry point fed no weights is the old one's arithmetic
                    assert torch.equal(ops.map_resize_aa(x, size[0], size[1], None, None, order=order, clip=clip, out_f64=dtype == torch.float64), want)


def test_a_mild_downscale_has_no_radius_and_is_the_plain_zoom():
    c = CASES["big_mild"]
    assert c["size"] == (180, 320)
    x = _t(_map("big_mild"))
    for g in (pp.gaussian_weights(224, 180), pp.gaussian_weights(384, 320)):
        assert g is not None and np.array_equal(g, [1.0])      # sigma 0.12 and 0.1: radius 0
    for order in ref.ORDERS:
        for dtype in (torch.float32, torch.float64):
            got = pp.resize(x, c["size"], order=order, dtype=dtype, anti_aliasing=True)
            assert torch.equal(got, ops.map_resize_aa(x, 180, 320, None, None, order=order, clip=True, out_f64=dtype == torch.float64))


def test_the_clip_uses_the_range_of_the_unfiltered_map():
    c = CASES["edge12x20"]
    m = c["map"].copy()
    m = np.concatenate([m, m * np.float32(0.5) + np.float32(0.25)])      # a second range: the clip is per image
    x = _t(m)
    filtered = pp.antialias(x, c["size"]).cpu().numpy()
    raw = pp.resize(x, c["size"], order=3, clip=False, anti_aliasing=True).cpu().numpy()
    out = pp.resize(x, c["size"], order=3, clip=True, anti_aliasing=True).cpu().numpy()
    for b in range(2):
        lo, hi = m[b].min(), m[b].max()
        print(f"image {b}: input [{lo}, {hi}] filtered [{filtered[b].min()}, {filtered[b].max()}] raw [{raw[b].min()}, {raw[b].max()}] "
              f"clipped [{out[b].min()}, {out[b].max()}]")
        assert filtered[b].max() < hi and filtered[b].min() == lo      # the Gaussian lowers the maximum
        assert raw[b].min() < lo and raw[b].max() > hi                 # the cubic overshoots both ends of the unfiltered range
        assert out[b].min() == lo and out[b].max() == hi               # clipped there, not at the filtered maximum below it
        assert np.array_equal(out[b], np.clip(raw[b], lo, hi))


def _annotations(B, H, W, seed=77):
    rng = np.random.default_rng(seed)
    fix = np.zeros((B, H * W), dtype=np.uint8)
    other = np.zeros((B, H * W), dtype=np.uint8)
    for b in range(B):
        fix[b, rng.choice(H * W, max(5, H * W // 40), replace=False)] = 1
        other[b, rng.choice(H * W, H * W // 4, replace=False)] = 1
    gt = (rng.integers(0, 16, size=(B, H, W)) / 15.0).astype(np.float32) ** 2
    return fix.reshape(B, H, W), gt, other.reshape(B, H, W)


def _same(tag, got, want, bar):
    print(f"{tag}: {got!r} want {want!r}")
    if math.isnan(want):
        assert math.isnan(got), tag
    else:
        assert abs(got - want) <= bar, (tag, got, want)


def _equal_with_nans(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def test_protocol_metrics_with_the_keyword_is_its_composition_and_matches_the_restatement():
    c = CASES["a33x70"]
    size = c["size"]
    fix, gt, other = _annotations(3, *size)
    p, f, g, o = _t(c["map"]).unsqueeze(1), _t(fix), _t(gt), _t(other)
    seed, ids, n_rep = 0x5EED, [11, (1 << 33) + 5, 13], 5
    kw = dict(n_rep=n_rep, seed=seed, image_ids=ids)
    with pytest.raises(ValueError, match="shrinks an axis"):
        pp.protocol_metrics(p, f, g, o, **kw)                      # without the keyword the refusal stays
    out = pp.protocol_metrics(p, f, g, o, anti_aliasing=True, **kw)
    assert list(out) == list(em.METRICS) and all(v.dtype == torch.float64 and v.shape == (3,) for v in out.values())
    m = pp.from_uint8(pp.to_uint8(p))
    m3, m1 = pp.resize(m, size, order=3, anti_aliasing=True), pp.resize(m, size, order=1, anti_aliasing=True)
    rest = tuple(k for k in em.METRICS if k != "nss")
    comp = em.benchmark_metrics(m3, f, g, o, metrics=rest, **kw)
    comp.update(em.benchmark_metrics(m1, f, metrics=("nss",)))
    for k in em.METRICS:
        assert _equal_with_nans(out[k], comp[k]), k
    h3, h1 = m3.cpu().numpy(), m1.cpu().numpy()      # the device's own maps
    with np.errstate(all="ignore"):
        for b in range(3):
            flat = not h3[b].max() > h3[b].min()
            want = {"auc_judd": mref.auc_judd(h3[b], fix[b]),
                    "auc_borji": mref.auc_borji(h3[b], fix[b], mref.borji_locations(fix[b], seed, ids[b], n_rep)),
                    "auc_shuffled": mref.auc_shuffled(h3[b], fix[b], other[b], mref.shuffled_locations(fix[b], other[b], seed, ids[b], n_rep)),
                    "cc": float("nan") if flat else mref.cc(h3[b], gt[b]), "nss": mref.nss(h1[b], fix[b]),
                    "sim": float("nan") if flat else mref.sim(h3[b], gt[b])}
            assert flat == (b == 1)
            for k in em.METRICS:
                _same(f"[{b}] {k}", out[k][b].item(), want[k], AUC_BAR if k.startswith("auc") else MOMENT_BAR)
    # the audio-visual sets' protocol takes the keyword too
    jp = pp.protocol_metrics(p, f, g, quantize="jpeg", anti_aliasing=True, metrics=("cc", "nss"))
    from diff_sal_amd import jpeg
    mj = pp.from_uint8(jpeg.roundtrip(pp.to_uint8(p)))
    assert _equal_with_nans(jp["cc"], em.cc(pp.resize(mj, size, order=3, anti_aliasing=True), g))
    assert _equal_with_nans(jp["nss"], em.nss(pp.resize(mj, size, order=1, anti_aliasing=True), f))


def test_without_the_keyword_a_downscale_still_raises():
    x = torch.rand(2, 8, 12, device=DEV)
    for size in ((7, 12), (8, 11), (9, 5)):
        with pytest.raises(ValueError, match="shrinks an axis"):
            pp.resize(x, size)
        with pytest.raises(ValueError, match="shrinks an axis"):
            pp.resize(x, size, anti_aliasing=False)
        assert pp.resize(x, size, anti_aliasing=True).shape == (2,) + size
    with pytest.raises(RuntimeError, match="shrinks an axis"):
        ops.map_resize(x, 7, 12)
    with pytest.raises(ValueError, match="anti_aliasing"):
        pp.resize(x, (7, 12), anti_aliasing="yes")
    with pytest.raises(ValueError, match="at least 1 x 1"):
        pp.resize(x, (0, 12), anti_aliasing=True)
    with pytest.raises(ValueError, match="radius"):
        pp.resize(torch.rand(1, 400, 8, device=DEV), (10, 8), anti_aliasing=True)      # a factor of 40
    with pytest.raises(RuntimeError, match="order"):
        pp.resize(x, (7, 12), order=2, anti_aliasing=True)


def test_two_calls_give_the_same_bits_and_a_batch_is_its_images():
    c = CASES["a33x70"]
    x = _t(c["map"])
    a = pp.antialias(x, c["size"])
    assert torch.equal(a, pp.antialias(x, c["size"]))
    assert torch.equal(a, torch.cat([pp.antialias(x[b:b + 1], c["size"]) for b in range(3)]))
    for order in ref.ORDERS:
        for dtype in (torch.float32, torch.float64):
            r = pp.resize(x, c["size"], order=order, dtype=dtype, anti_aliasing=True)
            assert torch.equal(r, pp.resize(x, c["size"], order=order, dtype=dtype, anti_aliasing=True)), (order, dtype)
            one = torch.cat([pp.resize(x[b:b + 1], c["size"], order=order, dtype=dtype, anti_aliasing=True) for b in range(3)])
            assert torch.equal(r, one), (order, dtype)


def test_graph_capture_and_replay_on_new_data():
    c = CASES["a33x70"]
    fix, gt, other = _annotations(3, *c["size"])
    first, second = [0, 2], [2, 1]      # the replay sees other maps, the flat one among them
    static = [_t(a[first]).clone() for a in (c["map"], fix, gt, other)]
    fresh = [_t(a[second]) for a in (c["map"] * np.float32(0.5) + np.float32(0.125), fix, gt, other)]
    ids = torch.tensor([21, 22], dtype=torch.int64, device=DEV)
    seed = torch.tensor([5], dtype=torch.int64, device=DEV)
    kw = dict(n_rep=4, seed=seed, image_ids=ids, anti_aliasing=True)
    eager = pp.protocol_metrics(*fresh, **kw)
    pp.protocol_metrics(*static, **kw)      # warm-up outside the capture: library load, allocator
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            captured = pp.protocol_metrics(*static, **kw)
    for s, f in zip(static, fresh):
        s.copy_(f)
    graph.replay()
    torch.cuda.synchronize()
    for k in em.METRICS:
        print(k, captured[k].cpu().numpy(), eager[k].cpu().numpy())
        assert _equal_with_nans(captured[k], eager[k]), k
    assert not torch.isnan(captured["cc"][0]) and torch.isnan(captured["cc"][1])


def _write_pngs(u8, paths):
    data, lengths = png.encode(u8)
    data, lengths = data.cpu().numpy(), lengths.cpu().numpy()
    for b, path in enumerate(paths):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(data[b, :lengths[b]].tobytes())


@pytest.mark.parametrize("data_type", ["dhf1k", "holly"])
def test_score_directory_is_the_meter_over_per_video_protocol_metrics(tmp_path, data_type):
    g = torch.Generator(device=DEV).manual_seed(3)
    videos = [601, 602] if data_type == "dhf1k" else ["clipA", "clipB"]
    shapes = {videos[0]: (12, 20), videos[1]: (20, 30)}      # annotations below the 16 x 24 predictions on both axes, and above
    pred_path, gt_root = str(tmp_path / "preds"), str(tmp_path / "gt")
    names, annotations = {}, {}
    for vid in videos:      # the dataset: maps and fixation files per video
        H, W = shapes[vid]
        vdir = os.path.join(gt_root, "annotation", f"{vid:04d}") if data_type == "dhf1k" else os.path.join(gt_root, vid)
        names[vid] = [f"{k:04d}.png" if data_type == "dhf1k" else f"{vid}_{k:05d}.png" for k in (1, 2, 3)]
        gt_u8 = torch.randint(0, 256, (3, H, W), device=DEV, dtype=torch.uint8, generator=g)
        fix_u8 = (torch.rand((3, H, W), device=DEV, generator=g) < 0.05).to(torch.uint8) * 255
        count = fix_u8.reshape(3, -1).count_nonzero(1)
        assert 0 < int(count.min()) and int(count.max()) < H * W
        _write_pngs(gt_u8, [os.path.join(vdir, "maps", n) for n in names[vid]])
        _write_pngs(fix_u8, [os.path.join(vdir, "fixation", n) for n in names[vid]])
        annotations[vid] = (gt_u8, fix_u8)
    want = {}
    for task in ("run_a", "run_b"):      # two tasks: a folder of predictions per video each
        meter = em.VideoMeter()
        for vid in videos:
            gt_u8, fix_u8 = annotations[vid]
            pred = torch.rand((3, 1, 16, 24), device=DEV, generator=g)
            png.save_predictions(pred, [str(vid)] * 3, [1, 2, 3], os.path.join(pred_path, task))
            p = pp.from_uint8(pp.to_uint8(pred))      # what the files hold, as plt.imread returns it
            meter.update(vid, pp.protocol_metrics(p, pp.from_uint8(fix_u8) > 0.5, pp.from_uint8(gt_u8), quantize=False,
                                                  anti_aliasing=True, metrics=("auc_judd", "cc", "nss", "sim")))
        want[task] = meter.compute()
    os.makedirs(os.path.join(pred_path, "run_a", "9999"))      # a prediction folder of a video that is not asked for
    asked = videos + ([603] if data_type == "dhf1k" else ["clipC"])      # the last has no prediction folder: skipped
    got = evaluate.score_directory(pred_path, gt_root, data_type, asked)
    print(got)
    assert got == want and list(got) == ["run_a", "run_b"] and all(list(r) == ["auc_judd", "cc", "nss", "sim"] for r in got.values())
    assert all(math.isfinite(v) for r in got.values() for v in r.values()) and got["run_a"] != got["run_b"]
    with open(pred_path + "_metrics.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["Task", "AUC_J ", "AUC_S ", "CC ", "NSS ", "Sim"]
    assert [row[0] for row in rows[1:]] == ["run_a", "run_b"]
    for row in rows[1:]:
        r = want[row[0]]
        assert [float(v) for v in row[1:]] == [r["auc_judd"], 0.0, r["cc"], r["nss"], r["sim"]]      # the same four-place numbers
    # a video's frames in chunks of two: a frame's scores do not depend on the call it is in
    vid = videos[0]
    maps_dir = os.path.join(gt_root, "annotation", f"{vid:04d}", "maps") if data_type == "dhf1k" else os.path.join(gt_root, vid, "maps")
    pairs = evaluate.pair_files(os.path.join(pred_path, "run_a", str(vid)), maps_dir, data_type, vid)
    assert [os.path.basename(m) for _, m, _ in pairs] == names[vid] and all(os.path.exists(q) for t in pairs for q in t)
    whole, chunked = evaluate.score_video(pairs), evaluate.score_video(pairs, batch=2)
    assert list(whole) == ["auc_judd", "cc", "nss", "sim"] and all(v.shape == (3,) and v.dtype == torch.float64 and v.is_cuda for v in whole.values())
    assert all(torch.equal(whole[k], chunked[k]) for k in whole)
