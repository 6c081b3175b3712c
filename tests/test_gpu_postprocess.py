"""Benchmark post-processing on the GPU (csrc/postprocess.hip through diff_sal_amd.postprocess): the 8-bit export and the spline
resize against the fixtures recorded from numpy, PIL, matplotlib and scipy (tools/gen_postprocess_golden.py) and against the NumPy
restatement on every pixel, the clip, determinism, batch independence, protocol_metrics against its explicit composition and
against tests/_eval_metrics_ref.py, graph capture, the PNG files, argument errors.

Bars.  Bytes and byte / 255: exact.  Resize with float64 output: |d| <= 1e-12 (fp64 epsilon 1.1e-16 x an l1 gain of 3 of the
coefficient filter per axis x 16 taps is about 1e-14; two decimal digits are left for the order of summation).  Resize in float32:
|d| <= 2^-23, one float32 step at the top of [0, 1] and below 2: with the float64 bar met, the single final rounding can differ from
scipy's by at most that; how many pixels differ at all is printed, not asserted.  Metric rows: the bars of
test_gpu_eval_metrics.py (1e-12 for the AUCs, 1e-9 for CC, NSS, SIM) against the restatement applied to the DEVICE's resized map,
copied back: a last-bit difference in one pixel may legitimately move an integer rank count, and the resize has its own bar."""
import math
import os

import numpy as np
import pytest
import torch

from diff_sal_amd import eval_metrics as em
from diff_sal_amd import postprocess as pp
from tests import _eval_metrics_ref as mref
from tests import _postprocess_ref as ref

pytestmark = pytest.mark.gpu

F64_BAR, F32_BAR, AUC_BAR, MOMENT_BAR = 1e-12, 2.0 ** -23, 1e-12, 1e-9
DEV = "cuda"
CASES = ref.load_cases()
_IMREAD = {}      # case -> the full float map the resize tests start from (restatement; equal to the fixture where recorded)


def _pred(name):
    return ref.big_input() if name == "big" else CASES[name]["pred"]


def _imread(name):
    if name not in _IMREAD:
        _IMREAD[name] = np.stack([ref.from_uint8(ref.to_uint8(p)) for p in _pred(name)])
    return _IMREAD[name]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pick(a, c):
    return a[:, c["rows"]][:, :, c["cols"]]


@pytest.mark.parametrize("name", sorted(CASES))
def test_bytes_and_png_floats_are_bit_equal_to_the_fixtures(name):
    c = CASES[name]
    pred = _pred(name)
    q = pp.to_uint8(_t(pred).unsqueeze(1))
    f = pp.from_uint8(q)
    assert q.dtype == torch.uint8 and f.dtype == torch.float32 and q.shape == f.shape == pred.shape
    q, f = q.cpu().numpy(), f.cpu().numpy()
    sub = (slice(None), slice(None, None, 7), slice(None, None, 5)) if name == "big" else (slice(None),) * 3
    assert np.array_equal(q[sub], c["u8"]) and np.array_equal(f[sub], c["imread"])
    assert np.array_equal(q, np.stack([ref.to_uint8(p) for p in pred])) and np.array_equal(f, _imread(name))      # every pixel
    if name == "s33x70":      # the flat image among non-flat neighbours: zeros by definition
        assert not q[1].any() and q[0].max() == 255 and q[2].max() == 255 and q[0].min() == 0


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("order", ref.ORDERS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_resize_against_scipy(name, order, clip):
    c = CASES[name]
    m = _imread(name)
    key = f"{'clip' if clip else 'zoom'}{order}"
    x = _t(m)
    got64 = pp.resize(x, c["size"], order=order, clip=clip, dtype=torch.float64)
    got32 = pp.resize(x, c["size"], order=order, clip=clip)
    assert got64.dtype == torch.float64 and got32.dtype == torch.float32 and got64.shape == got32.shape == (m.shape[0],) + c["size"]
    got64, got32 = got64.cpu().numpy(), got32.cpu().numpy()
    full = np.stack([ref.resize(p, c["size"], order=order, clip=clip) for p in m])      # every pixel, float64
    d_fix = float(np.abs(_pick(got64, c) - c[key + "_f64"]).max())
    d_all = float(np.abs(got64 - full).max())
    d32 = float(np.abs(_pick(got32, c).astype(np.float64) - c[key + "_f32"].astype(np.float64)).max())
    d32_all = float(np.abs(got32.astype(np.float64) - full).max())
    n_diff = int((_pick(got32, c) != c[key + "_f32"]).sum())
    print(f"{name} order {order} clip {clip}: f64 |d| fixture {d_fix:.2e} restatement {d_all:.2e}; f32 |d| fixture {d32:.2e}, "
          f"{n_diff} of {c[key + '_f32'].size} recorded pixels differ from scipy's float32 at all")
    assert np.array_equal(got32, got64.astype(np.float32))      # the float32 path is the float64 one rounded once
    assert d_fix <= F64_BAR and d_all <= F64_BAR
    assert d32 <= F32_BAR and d32_all <= F32_BAR


def test_clip_holds_each_image_to_its_own_input_range():
    c = CASES["s7x12"]
    z = c["zoom3_f64"].reshape(2, -1)      # the fixture: every image overshoots on both sides without the clip
    assert (z.min(1) < -0.01).all() and (z.max(1) > 1.01).all()
    m = _imread("s7x12").copy()
    m[1] = m[1] * np.float32(0.5) + np.float32(0.25)      # a second range: the clip is per image
    x = _t(m)
    raw = pp.resize(x, c["size"], order=3, clip=False).cpu().numpy()
    out = pp.resize(x, c["size"], order=3, clip=True).cpu().numpy()
    for b in range(2):
        lo, hi = m[b].min(), m[b].max()
        print(f"image {b}: input [{lo}, {hi}] raw [{raw[b].min()}, {raw[b].max()}] clipped [{out[b].min()}, {out[b].max()}]")
        assert raw[b].min() < lo and raw[b].max() > hi
        assert out[b].min() == lo and out[b].max() == hi
        assert np.array_equal(out[b], np.clip(raw[b], lo, hi))
    lin = pp.resize(x, c["size"], order=1, clip=True).cpu().numpy()
    assert all(lin[b].min() >= m[b].min() and lin[b].max() <= m[b].max() for b in range(2))


def test_two_calls_give_the_same_bits_and_a_batch_is_its_images():
    pred = _t(CASES["s33x70"]["pred"])
    size = CASES["s33x70"]["size"]
    q = pp.to_uint8(pred)
    assert torch.equal(q, pp.to_uint8(pred))
    assert torch.equal(q, torch.cat([pp.to_uint8(pred[b:b + 1]) for b in range(3)]))
    m = pp.from_uint8(q)
    for order in ref.ORDERS:
        for dtype in (torch.float32, torch.float64):
            a = pp.resize(m, size, order=order, dtype=dtype)
            assert torch.equal(a, pp.resize(m, size, order=order, dtype=dtype)), (order, dtype)
            one = torch.cat([pp.resize(m[b:b + 1], size, order=order, dtype=dtype) for b in range(3)])
            assert torch.equal(a, one), (order, dtype)


def _annotations(name="s33x70"):
    c = CASES[name]
    B = c["pred"].shape[0]
    H, W = c["size"]
    rng = np.random.default_rng(77)
    other = np.zeros((B, H * W), dtype=np.uint8)
    for b in range(B):
        other[b, rng.choice(H * W, 400, replace=False)] = 1
    return c, c["fix"], c["gt"], other.reshape(B, H, W)


def _same(tag, got, want, bar):
    print(f"{tag}: {got!r} want {want!r}")
    if math.isnan(want):
        assert math.isnan(got), tag
    else:
        assert abs(got - want) <= bar, (tag, got, want)


def test_protocol_metrics_is_its_composition_and_matches_the_restatement():
    c, fix, gt, other = _annotations()
    size = c["size"]
    p, f, g, o = _t(c["pred"]).unsqueeze(1), _t(fix), _t(gt), _t(other)
    seed, ids, n_rep = 0x5EED, [11, (1 << 33) + 5, 13], 5
    kw = dict(n_rep=n_rep, seed=seed, image_ids=ids)
    out = pp.protocol_metrics(p, f, g, o, **kw)
    assert list(out) == list(em.METRICS) and all(v.dtype == torch.float64 and v.shape == (3,) for v in out.values())
    m = pp.from_uint8(pp.to_uint8(p))
    m3, m1 = pp.resize(m, size, order=3), pp.resize(m, size, order=1)
    rest = tuple(k for k in em.METRICS if k != "nss")
    comp = em.benchmark_metrics(m3, f, g, o, metrics=rest, **kw)
    comp.update(em.benchmark_metrics(m1, f, metrics=("nss",)))
    for k in em.METRICS:
        assert torch.equal(out[k], comp[k]) or (torch.isnan(out[k]) == torch.isnan(comp[k])).all() and torch.equal(
            torch.nan_to_num(out[k]), torch.nan_to_num(comp[k])), k
    only = pp.protocol_metrics(p, f, g, metrics=("cc", "nss"))
    assert list(only) == ["cc", "nss"] and all(torch.equal(torch.nan_to_num(only[k]), torch.nan_to_num(out[k])) for k in only)
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


def test_protocol_metrics_without_quantisation_at_matching_shapes_is_benchmark_metrics():
    c = mref.CASES["small"]
    p, f, g, o = (_t(c[k]) for k in ("pred", "fix", "gt", "other"))
    kw = dict(n_rep=4, seed=3, image_ids=[1, 2, 3])
    a = pp.protocol_metrics(p, f, g, o, quantize=False, **kw)
    b = em.benchmark_metrics(p, f, g, o, **kw)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) and not torch.isnan(a[k]).any() for k in b)
    q = pp.protocol_metrics(p, f, g, o, **kw)      # quantised, same shapes: no resize, the 8-bit map's scores
    want = em.benchmark_metrics(pp.from_uint8(pp.to_uint8(p)), f, g, o, **kw)
    assert all(torch.equal(q[k], want[k]) for k in want) and not torch.equal(q["cc"], b["cc"])


def test_benchmark_metrics_still_raises_on_a_shape_mismatch():
    c, fix, gt, _ = _annotations()
    with pytest.raises(ValueError, match="does not match") as e:
        em.benchmark_metrics(_t(c["pred"]), _t(fix), _t(gt))
    assert "protocol_metrics" in str(e.value)


def test_graph_capture_and_replay_on_new_data():
    c, fix, gt, other = _annotations()
    first, second = [0, 2], [2, 1]      # the replay sees other maps, the flat one among them
    static = [_t(a[first]).clone() for a in (c["pred"], fix, gt, other)]
    fresh = [_t(a[second]) for a in (c["pred"] * np.float32(0.5) + np.float32(0.125), fix, gt, other)]
    ids = torch.tensor([21, 22], dtype=torch.int64, device=DEV)
    seed = torch.tensor([5], dtype=torch.int64, device=DEV)
    kw = dict(n_rep=4, seed=seed, image_ids=ids)
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
        assert torch.equal(torch.isnan(captured[k]), torch.isnan(eager[k])), k
        assert torch.equal(torch.nan_to_num(captured[k]), torch.nan_to_num(eager[k])), k
    assert not torch.isnan(captured["cc"][0]) and torch.isnan(captured["cc"][1])


def test_save_predictions_writes_the_reference_layout(tmp_path):
    from PIL import Image

    pred = _t(CASES["s33x70"]["pred"]).unsqueeze(1)
    vids, frames = ["601", "601", "0612"], torch.tensor([[7], [8], [120]])
    paths = pp.save_predictions(pred, vids, frames, str(tmp_path))
    want = pp.to_uint8(pred).cpu().numpy()
    assert [os.path.relpath(p, str(tmp_path)) for p in paths] == [os.path.join("601", "7.png"), os.path.join("601", "8.png"),
                                                                   os.path.join("0612", "120.png")]
    for b, p in enumerate(paths):
        img = Image.open(p)
        assert img.mode == "L" and np.array_equal(np.asarray(img), want[b])
    with pytest.raises(ValueError, match="lossy"):
        pp.save_predictions(pred, vids, frames, str(tmp_path), fmt="jpg")


def test_argument_errors_on_gpu_tensors():
    p = torch.rand(2, 1, 8, 12, device=DEV)
    f = torch.zeros(2, 16, 24, dtype=torch.uint8, device=DEV)
    for call in (lambda: pp.to_uint8(p.cpu()), lambda: pp.from_uint8(pp.to_uint8(p).cpu()), lambda: pp.resize(p.cpu(), (16, 24)),
                 lambda: pp.protocol_metrics(p.cpu(), f), lambda: pp.protocol_metrics(p, f.cpu()),
                 lambda: pp.save_predictions(p.cpu(), ["a", "b"], [1, 2], "unused")):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    with pytest.raises(ValueError, match="floating"):
        pp.to_uint8((p * 255).to(torch.int32))
    with pytest.raises(ValueError, match="floating"):
        pp.protocol_metrics((p * 255).to(torch.uint8), f)
    with pytest.raises(ValueError, match="uint8"):
        pp.from_uint8(p)
    with pytest.raises(ValueError, match="shrinks an axis"):
        pp.resize(p, (7, 12))
    with pytest.raises(ValueError, match="shrinks an axis"):
        pp.protocol_metrics(p, f[:, :4, :6])
    with pytest.raises(RuntimeError, match="order"):
        pp.resize(p, (16, 24), order=2)
    with pytest.raises(RuntimeError, match="at least 2 samples"):
        pp.resize(p[:, :, :1], (16, 24))
    with pytest.raises(ValueError, match="share the resolution"):
        pp.protocol_metrics(p, f, torch.rand(2, 16, 25, device=DEV))
    with pytest.raises(ValueError, match="unknown metric"):
        pp.protocol_metrics(p, f, metrics=("auc",))
