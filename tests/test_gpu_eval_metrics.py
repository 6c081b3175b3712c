"""Benchmark metrics on the GPU (csrc/eval_metrics.hip through diff_sal_amd.eval_metrics): parity with the values recorded from the
reference, degenerate images, the device generator against the NumPy restatement, determinism, graph capture, VideoMeter.

Bars.  AUC-Judd, AUC-Borji, sAUC: |d| <= 1e-12 -- the counts are integers and exact, only the order of at most n_fix + 2 fp64
trapezoid terms of magnitude <= 1 differs (n_fix <= 4000 in the fixtures).  CC, NSS, SIM: |d| <= 1e-9 against the float64
reference values -- fp64 accumulation over <= 15 360 well-conditioned pixels is ~1e-12, the margin is for the variance
cancellation."""
import math

import numpy as np
import pytest
import torch

from diff_sal_amd import eval_metrics as em
from tests import _eval_metrics_ref as ref
from tests._eval_metrics_ref import CASES

pytestmark = pytest.mark.gpu

AUC_BAR, MOMENT_BAR = 1e-12, 1e-9
DEV = "cuda"


def _dev(c, k, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV)
    return t if dtype is None else t.to(dtype)


def _check(tag, got, want, bar):
    got = got.cpu().numpy()
    for b, (g, w) in enumerate(zip(got, want)):
        d = abs(g - w)
        print(f"{tag}[{b}]: {g:.15f} want {w:.15f} |d| = {d:.2e}")
        assert d <= bar, (tag, b, g, w)


@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_with_the_reference_fixtures(name):
    c = CASES[name]
    pred, fix, gt, other = _dev(c, "pred"), _dev(c, "fix"), _dev(c, "gt"), _dev(c, "other")
    rb, rs = _dev(c, "rand_borji"), _dev(c, "rand_shuffled")
    out = em.benchmark_metrics(pred.unsqueeze(1), fix, gt, other, n_rep=c["n_rep"], rand_index=rb, rand_index_shuffled=rs)
    assert list(out) == list(em.METRICS) and all(v.dtype == torch.float64 and v.shape == (pred.shape[0],) for v in out.values())
    for k in em.METRICS:
        _check(f"{name} {k}", out[k], c["expected"][k], AUC_BAR if k.startswith("auc") else MOMENT_BAR)
    # the single-metric entry points are the same numbers; fixation maps as bool and as float
    assert torch.equal(em.auc_judd(pred, fix.bool()), out["auc_judd"])
    assert torch.equal(em.auc_borji(pred, fix.float(), n_rep=c["n_rep"], rand_index=rb), out["auc_borji"])
    assert torch.equal(em.auc_shuffled(pred, fix, other, n_rep=c["n_rep"], rand_index=rs), out["auc_shuffled"])
    assert torch.equal(em.cc(pred, gt), out["cc"]) and torch.equal(em.sim(pred, gt), out["sim"])
    assert torch.equal(em.nss(pred, fix), out["nss"])
    assert list(em.benchmark_metrics(pred, fix, rand_index=rb, n_rep=c["n_rep"])) == ["auc_judd", "auc_borji", "nss"]


def test_degenerate_images_are_nan_and_leave_their_neighbours_alone():
    c = CASES["small"]
    H, W = 24, 40
    p, f, g, o = (c[k][1] for k in ("pred", "fix", "gt", "other"))
    pred = np.stack([p, p, p, np.full_like(p, 0.25), p])
    fix = np.stack([f, np.zeros_like(f), np.ones_like(f), f, f])
    gt = np.stack([g] * 5)
    other = np.stack([o, o, o, o, np.zeros_like(o)])
    n_rep = c["n_rep"]
    rb = np.stack([c["rand_borji"][1]] * 5)
    rs = np.stack([c["rand_shuffled"][1]] * 5)
    t = lambda a: torch.from_numpy(a).to(DEV)      # noqa: E731
    out = em.benchmark_metrics(t(pred), t(fix), t(gt), t(other), n_rep=n_rep, rand_index=t(rb), rand_index_shuffled=t(rs))
    one = em.benchmark_metrics(t(pred[:1]), t(fix[:1]), t(gt[:1]), t(other[:1]), n_rep=n_rep, rand_index=t(rb[:1]),
                               rand_index_shuffled=t(rs[:1]))
    for k in em.METRICS:
        v = out[k].cpu().numpy()
        print(k, v)
        assert v[0] == one[k].item() and not math.isnan(v[0])                  # bit for bit
        if k in ("auc_judd", "auc_borji", "auc_shuffled", "nss"):
            assert np.isnan(v[1:4]).all(), (k, v)                              # no fixation, all fixated, flat map
        else:
            assert not np.isnan(v[1:3]).any() and math.isnan(v[3]), (k, v)     # cc / sim: only the flat map
    v = out["auc_shuffled"].cpu().numpy()
    assert math.isnan(v[4])                                                     # `other` without fixations
    for k in ("auc_judd", "auc_borji", "cc", "nss", "sim"):
        assert out[k][4].item() == one[k].item()


def _gen_case():
    c = CASES["odd"]
    return c["pred"], c["fix"], c["other"]


def test_device_generator_equals_the_restatement():
    pred, fix, other = _gen_case()
    seed, ids, n_rep = 0x1234567890ABCDEF, [(1 << 32) + 17, 5], 8              # an id above 2^32
    p, f, o = (torch.from_numpy(a).to(DEV) for a in (pred, fix, other))
    got_b = em.auc_borji(p, f, n_rep=n_rep, seed=seed, image_ids=ids)
    got_s = em.auc_shuffled(p, f, o, n_rep=n_rep, seed=seed, image_ids=ids)
    got_j = em.auc_judd(p, f, jitter=True, seed=seed, image_ids=ids)
    want_b = [ref.auc_borji(pred[b], fix[b], ref.borji_locations(fix[b], seed, ids[b], n_rep)) for b in range(2)]
    want_s = [ref.auc_shuffled(pred[b], fix[b], other[b], ref.shuffled_locations(fix[b], other[b], seed, ids[b], n_rep)) for b in range(2)]
    want_j = [ref.auc_judd(ref.jittered(pred[b], seed, ids[b]), fix[b]) for b in range(2)]
    _check("generator borji", got_b, want_b, AUC_BAR)
    _check("generator sauc", got_s, want_s, AUC_BAR)
    _check("generator judd+jitter", got_j, want_j, AUC_BAR)
    assert not torch.equal(got_b, em.auc_borji(p, f, n_rep=n_rep, seed=seed + 1, image_ids=ids))


def test_device_generator_jitter_breaks_ties():
    c = CASES["ties"]
    pred, fix = c["pred"], c["fix"]
    p, f = torch.from_numpy(pred).to(DEV), torch.from_numpy(fix).to(DEV)
    ids = [3, 4]
    got = em.auc_judd(p, f, jitter=True, seed=9, image_ids=ids)
    want = [ref.auc_judd(ref.jittered(pred[b], 9, ids[b]), fix[b]) for b in range(2)]
    _check("ties judd+jitter", got, want, AUC_BAR)
    assert not torch.equal(got, em.auc_judd(p, f))


def test_device_generator_is_keyed_by_image_not_by_batch_position():
    c = CASES["small"]
    p, f, o, g = (_dev(c, k) for k in ("pred", "fix", "other", "gt"))
    ids = torch.tensor([7, (1 << 40) + 1, 9], dtype=torch.int64, device=DEV)
    kw = dict(n_rep=6, seed=11)
    full = em.benchmark_metrics(p, f, g, o, image_ids=ids, **kw)
    perm = torch.tensor([2, 0, 1], device=DEV)
    shuffled = em.benchmark_metrics(p[perm], f[perm], g[perm], o[perm], image_ids=ids[perm], **kw)
    a = em.benchmark_metrics(p[:1], f[:1], g[:1], o[:1], image_ids=ids[:1], **kw)
    b = em.benchmark_metrics(p[1:], f[1:], g[1:], o[1:], image_ids=ids[1:], **kw)
    for k in em.METRICS:
        assert torch.equal(shuffled[k], full[k][perm]), k
        assert torch.equal(torch.cat([a[k], b[k]]), full[k]), k
    jit = em.auc_judd(p, f, jitter=True, seed=11, image_ids=ids)
    assert torch.equal(em.auc_judd(p[perm], f[perm], jitter=True, seed=11, image_ids=ids[perm]), jit[perm])


def test_two_calls_give_the_same_bits():
    c = CASES["tiles"]
    p, f, o, g = (_dev(c, k) for k in ("pred", "fix", "other", "gt"))
    x = em.benchmark_metrics(p, f, g, o, n_rep=4, seed=3, image_ids=[12])
    y = em.benchmark_metrics(p, f, g, o, n_rep=4, seed=3, image_ids=[12])
    for k in em.METRICS:
        assert torch.equal(x[k], y[k]) and not torch.isnan(x[k]).any(), k


def test_graph_capture_and_replay_on_new_data():
    small, ties = CASES["small"], CASES["ties"]
    # static inputs hold the first two images of `small` at capture and are overwritten with `ties` before the replay
    names = ("pred", "fix", "gt", "other")
    static = [_dev(small, k)[:2].clone() for k in names]
    fresh = [_dev(ties, k) for k in names]
    ids = torch.tensor([21, 22], dtype=torch.int64, device=DEV)
    seed = torch.tensor([5], dtype=torch.int64, device=DEV)
    kw = dict(n_rep=5, seed=seed, image_ids=ids)
    eager = em.benchmark_metrics(*fresh, **kw)
    em.benchmark_metrics(*static, **kw)      # warm-up outside the capture: library load, allocator
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            captured = em.benchmark_metrics(*static, **kw)
    for s, f in zip(static, fresh):
        s.copy_(f)
    graph.replay()
    torch.cuda.synchronize()
    for k in em.METRICS:
        print(k, captured[k].cpu().numpy(), eager[k].cpu().numpy())
        assert torch.equal(captured[k], eager[k]), k


def test_argument_errors_on_gpu_tensors():
    p = torch.rand(2, 1, 8, 8, device=DEV)
    f = torch.zeros(2, 8, 8, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="does not match"):
        em.auc_judd(p, torch.zeros(2, 16, 16, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="does not match"):
        em.cc(p, torch.rand(2, 1, 8, 9, device=DEV))
    with pytest.raises(ValueError, match="image_ids"):
        em.auc_borji(p, f)
    with pytest.raises(ValueError, match="image_ids"):
        em.auc_judd(p, f, jitter=True)
    with pytest.raises(ValueError, match="image_ids"):
        em.auc_shuffled(p, f, f)
    with pytest.raises(ValueError, match="image_ids"):
        em.auc_borji(p, f, image_ids=[1, 2, 3])
    with pytest.raises(ValueError):
        em.auc_borji(p, f, image_ids=[1, -2])
    with pytest.raises(ValueError, match="rand_index"):
        em.auc_borji(p, f, n_rep=4, rand_index=torch.zeros(2, 3, 5, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="bool, uint8 or floating"):
        em.nss(p, f.to(torch.int32))
    with pytest.raises(ValueError, match="unknown metric"):
        em.benchmark_metrics(p, f, metrics=("auc",))
    with pytest.raises(RuntimeError, match="GPU only"):
        em.auc_judd(p, f.cpu())


def test_video_meter_on_device_tensors():
    c = CASES["small"]
    p, f, g = (_dev(c, k) for k in ("pred", "fix", "gt"))
    out = em.benchmark_metrics(p, f, g, metrics=("auc_judd", "cc", "nss", "sim"))
    meter = em.VideoMeter()
    meter.update("v1", {k: v[:2] for k, v in out.items()})
    meter.update("v2", {k: v[2:] for k, v in out.items()})
    assert all(s.is_cuda for per in meter._sums.values() for s, _ in per.values())
    got = meter.compute()
    for k, v in out.items():
        h = v.cpu().numpy()
        assert got[k] == float(np.around(np.mean([np.mean(h[:2]), np.mean(h[2:])]), 4)), k
