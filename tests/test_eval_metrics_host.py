"""Benchmark metrics without a GPU: the NumPy restatement against the values recorded from the reference
(tests/golden/eval_metrics.npz, written by tools/gen_eval_metrics_golden.py), VideoMeter's aggregation, argument errors."""
import math
import os

import numpy as np
import pytest
import torch

from diff_sal_amd import _lib, eval_metrics as em
from tests import _eval_metrics_ref as ref

GOLDEN, CASES = ref.GOLDEN, ref.CASES


def test_fixture_covers_the_cases_the_kernels_can_go_wrong_on():
    assert os.path.getsize(GOLDEN) < 300 * 1024
    assert sorted(CASES) == ["odd", "small", "ties", "tiles"]
    small = CASES["small"]
    assert small["pred"].shape == (3, 24, 40) and small["fix"].reshape(3, -1).sum(1).tolist() == [1, 37, 24 * 40 - 1]
    assert CASES["odd"]["pred"].shape[1:] == (23, 37)
    assert CASES["tiles"]["pred"].shape[1:] == (96, 160) and CASES["tiles"]["fix"].sum() == 700
    assert len(np.unique(CASES["ties"]["pred"])) == 8
    for c in CASES.values():
        assert c["pred"].dtype == np.float32 and c["fix"].sum(axis=(1, 2)).max() <= 4000
        assert all(np.isfinite(v).all() for v in c["expected"].values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_numpy_restatement_reproduces_the_reference(name):
    c = CASES[name]
    for b in range(c["pred"].shape[0]):
        p, g, f, o = c["pred"][b], c["gt"][b], c["fix"][b], c["other"][b]
        got = {
            "auc_judd": ref.auc_judd(p, f),
            "auc_borji": ref.auc_borji(p, f, c["rand_borji"][b]),
            "auc_shuffled": ref.auc_shuffled(p, f, o, c["rand_shuffled"][b]),
            "cc": ref.cc(p, g), "nss": ref.nss(p, f), "sim": ref.sim(p, g),
        }
        for k, v in got.items():
            d = abs(v - c["expected"][k][b])
            print(f"{name}[{b}] {k}: {v:.15f} |d| = {d:.2e}")
            assert d <= 1e-12, (name, b, k, v, c["expected"][k][b])


def test_restatement_degenerate_images_are_nan():
    rng = np.random.default_rng(0)
    p = rng.random((8, 8), dtype=np.float32)
    some = np.zeros((8, 8), np.uint8)
    some[2, 3] = some[5, 1] = 1
    loc = [np.array([3, 9])]
    for pm, fm in ((p, np.zeros_like(some)), (p, np.ones_like(some)), (np.full_like(p, 0.25), some)):
        assert math.isnan(ref.auc_judd(pm, fm)) and math.isnan(ref.auc_borji(pm, fm, loc)) and math.isnan(ref.nss(pm, fm))
    assert math.isnan(ref.auc_shuffled(p, some, np.zeros_like(some), loc))
    assert 0.0 <= ref.auc_judd(p, some) <= 1.0


def test_generator_layouts_of_the_restatement():
    rng = np.random.default_rng(1)
    fix = (rng.random((6, 10)) < 0.2).astype(np.uint8)
    other = (rng.random((6, 10)) < 0.1).astype(np.uint8)
    locs = ref.borji_locations(fix, 7, (1 << 33) + 5, 4)
    assert len(locs) == 4 and all(len(l) == fix.sum() and l.min() >= 0 and l.max() < 60 for l in locs)
    sel = ref.shuffled_locations(fix, other, 7, 3, 4)
    m = min(fix.sum(), other.sum())
    assert all(len(s) == m and len(set(s.tolist())) == m and other.ravel()[s].all() for s in sel)
    assert any(not np.array_equal(sel[0], s) for s in sel[1:])
    j = ref.jittered(np.zeros(60, np.float32), 7, 3)
    assert j.dtype == np.float32 and (j >= 0).all() and (j < 1.0001e-7).all() and len(np.unique(j)) > 50


def test_video_meter_aggregates_frames_then_videos():
    m = em.VideoMeter()
    m.update("a", {"cc": torch.tensor([0.2, 0.4], dtype=torch.float64), "nss": torch.tensor([1.0, 3.0])})
    m.update("a", {"cc": torch.tensor([0.9], dtype=torch.float64), "nss": torch.tensor([2.0])})
    m.update("b", {"cc": torch.tensor([0.123456, 0.1], dtype=torch.float64), "nss": torch.tensor(5.0)})
    want_cc = np.around(np.mean([np.mean([0.2, 0.4, 0.9]), np.mean([0.123456, 0.1])]), 4)
    assert m.compute() == {"cc": float(want_cc), "nss": 3.5}


def test_video_meter_nan_policy():
    nan = float("nan")
    frames = {"a": [0.5, nan, 0.7], "b": [0.2], "c": [nan]}
    prop, omit = em.VideoMeter(), em.VideoMeter(nan_policy="omit")
    for k, v in frames.items():
        prop.update(k, {"auc_judd": torch.tensor(v, dtype=torch.float64)})
        omit.update(k, {"auc_judd": torch.tensor(v, dtype=torch.float64)})
    assert math.isnan(prop.compute()["auc_judd"])
    assert omit.compute() == {"auc_judd": round((0.6 + 0.2) / 2, 4)}      # the NaN frame and the all-NaN video are left out
    with pytest.raises(ValueError):
        em.VideoMeter(nan_policy="zero")


def test_cpu_tensors_and_bad_arguments_raise():
    p, f = torch.rand(2, 1, 8, 8), torch.zeros(2, 8, 8, dtype=torch.uint8)
    for call in (lambda: em.auc_judd(p, f), lambda: em.auc_borji(p, f, image_ids=[0, 1]), lambda: em.cc(p, p),
                 lambda: em.nss(p, f), lambda: em.sim(p, p), lambda: em.benchmark_metrics(p, f),
                 lambda: em.auc_shuffled(p, f, f, image_ids=[0, 1])):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()


def test_library_argument_errors_are_reported_before_any_launch():
    lib = _lib.load()
    J, B, S, CC, JIT = 1, 2, 4, 8, 64
    # device pointers are plain integers here: non-null, never dereferenced by the checks

    def call(terms, pred=16, fix=16, gt=16, other=16, Bn=(2, 64), n_rep=4, step=0.1, rb=None, rs=None, cap=0, ids=None, seed=None,
             ws=16, ws_bytes=1 << 30, out=16):
        return lib.diffsal_eval_metrics(pred, fix, gt, other, Bn[0], Bn[1], terms, n_rep, step, rb, rs, cap, ids, seed, ws, ws_bytes, out, None)

    assert call(J, pred=None) == -4 and b"null" in lib.diffsal_last_error()
    assert call(0) == -4 and b"no metric" in lib.diffsal_last_error()
    assert call(JIT, ids=16, seed=16) == -4
    assert call(J, fix=None) == -4 and b"fixation" in lib.diffsal_last_error()
    assert call(CC, gt=None) == -4 and b"ground-truth" in lib.diffsal_last_error()
    assert call(S, other=None, rs=16, cap=4) == -4 and b"other" in lib.diffsal_last_error()
    assert call(B) == -4 and b"image ids" in lib.diffsal_last_error()              # device generator without ids / seed
    assert call(J | JIT) == -4 and b"image ids" in lib.diffsal_last_error()
    assert call(J | B | JIT, ids=16, seed=16) == -4 and b"jitter" in lib.diffsal_last_error()
    assert call(B, rb=16, cap=4, step=0.0) == -4 and b"step" in lib.diffsal_last_error()
    assert call(B, rb=16, cap=4, step=1e-4) == -4
    assert call(B, rb=16, cap=4, n_rep=0) != 0 and b"n_rep" in lib.diffsal_last_error()
    assert call(B, rb=16, cap=0) != 0 and b"cap" in lib.diffsal_last_error()
    assert call(J, Bn=(0, 64)) != 0 and call(J, Bn=(2, 1)) != 0 and call(J, Bn=(2, 1 << 31)) != 0
    need = lib.diffsal_eval_metrics_ws_bytes(2, 64, B, 4)
    assert need > 0 and need % 16 == 0
    assert lib.diffsal_eval_metrics_ws_bytes(0, 64, B, 4) == 0
    # the [B][n] arrays are sized by the terms: none for CC / NSS / SIM, six of them for the three AUCs together
    small, full = lib.diffsal_eval_metrics_ws_bytes(64, 230400, CC | 16 | 32, 0), lib.diffsal_eval_metrics_ws_bytes(64, 230400, J | B | S, 100)
    assert small < 1 << 20 and 6 * 64 * 230400 * 4 <= full < 6 * 64 * 230400 * 4 + (1 << 20)
    assert call(B, rb=16, cap=4, ws_bytes=need - 16) == -4 and b"workspace" in lib.diffsal_last_error()
    assert call(J, ws=8) == -4 and b"misaligned" in lib.diffsal_last_error()
