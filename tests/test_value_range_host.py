"""The cases of tests/test_gpu_value_range.py are valid and their bounds attainable (no GPU): for every case of parts A, B and D
the fp32 torch reference is finite and stays well inside the fp64 one, and a float32 restatement of each activation passes the
bounds of part C over the whole sweep."""
import math

import numpy as np
import pytest
import torch

from tests import _value_range_ref as vr

CASES = vr.all_cases()


def test_case_ids_are_unique_and_every_family_has_cases():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    assert {c.family for c in CASES} == set(vr.FAMILIES)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_reference_is_finite_and_fp32_stays_inside_the_cap(case):
    """ref32 finite, 8 max|ref32 - ref64| <= 1e-2 max|ref64| for every output: inputs on which the reference itself falls apart
    are not valid cases."""
    _, ref64, ref32 = vr.evaluate(case)
    for k, (m64, d32) in vr.reference_spread(ref64, ref32).items():
        assert torch.isfinite(ref32[k]).all() and torch.isfinite(ref64[k]).all(), (case.id, k)
        if k in vr.outside_the_rule(case):
            continue
        print(f"{case.id} {k}: max|ref64| {m64:.3e} max|ref32-ref64| {d32:.3e}")
        assert 8.0 * d32 <= vr.REF_CAP * m64, (case.id, k, d32, m64)


@pytest.mark.parametrize("fill", vr.FILLS)
def test_constant_rows_normalise_to_beta(fill):
    """part D: the reference of a constant row is beta (or swish(beta)) exactly"""
    case = next(c for c in CASES if c.family == "ln" and c.p["R"] == fill and c.p["dname"] == "fp32")
    t, ref64, _ = vr.evaluate(case)
    assert torch.equal(ref64["y"], t["b"].double().expand_as(ref64["y"]))
    case = next(c for c in CASES if c.family == "gn" and c.p["R"] == fill and c.p["swish"] and c.p["dname"] == "fp32")
    t, ref64, _ = vr.evaluate(case)
    b = t["b"].double()
    assert torch.allclose(ref64["y"], (b * torch.sigmoid(b)).expand_as(ref64["y"]), rtol=1e-14, atol=0)


def test_block_front_reference_is_the_fold_tests_own_in_fp64():
    from tests.test_gpu_block_front_fold import _reference64

    for cid in ("block_front-R64", "block_front-a16"):
        t, ref64, _ = vr.evaluate(next(c for c in CASES if c.id == cid))
        assert torch.equal(ref64["y"], _reference64(t["x"], t["kp"], t["vp"], t["prm"], t["w"], t["b"]))


def test_offset_inputs_alternate_as_stated():
    x = vr.offset_input("t.g", (1, 2, 2, 96), 512, "group")
    m = x.reshape(4, 32, 3).mean((0, 2))
    assert (m[0::2] > 500).all() and (m[1::2] < -500).all()
    x = vr.offset_input("t.r", (6, 32), 64, "row")
    assert (x.mean(1)[0::2] > 60).all() and (x.mean(1)[1::2] < -60).all()
    x = vr.offset_input("t.c", (50, 8), 8, "channel")
    assert (x.mean(0)[0::2] > 7).all() and (x.mean(0)[1::2] < -7).all()
    x16 = vr.offset_input("t.g", (1, 2, 2, 96), 8, "group", "bf16")
    assert torch.equal(x16, x16.to(torch.bfloat16).float())


def test_softmax_modes_reach_the_stated_logits():
    case = next(c for c in CASES if c.id == "attention-fp32-96.200.18-a128")
    t, _, _ = vr.evaluate(case)
    d = 48
    s = (t["q"][..., :d] @ t["k"][..., :d].transpose(-1, -2)) * 96 ** -0.5
    assert s.abs().max().item() > 300.0            # exp overflows in fp32 without the maximum subtracted (88.7)
    case = next(c for c in CASES if c.id == "attention-fp32-96.200.18-flat")
    t, ref64, _ = vr.evaluate(case)
    assert torch.allclose(ref64["o"], t["v"].double().mean(1, keepdim=True).expand_as(ref64["o"]), rtol=0, atol=1e-13)
    case = next(c for c in CASES if c.id == "attention-fp32-96.200.18-onehot")
    t, ref64, _ = vr.evaluate(case)
    assert torch.allclose(ref64["o"][:, 0], t["v"][:, 0].double(), rtol=0, atol=1e-9)     # query 0 sees key 0 alone


def test_sweep_is_the_stated_one():
    x = vr.sweep()
    assert tuple(x.shape) == (688, 96) and x.numel() == 66048
    flat = x.reshape(-1)
    for v in vr.SPLICED:
        for s in (1.0, -1.0):
            w = torch.tensor(s * v, dtype=torch.float32)
            hit = (flat == w) & (torch.signbit(flat) == torch.signbit(w))
            assert hit.any(), s * v
    assert (flat == 1e-40).any() and 0 < 1e-40 < torch.finfo(torch.float32).tiny         # a subnormal
    grid = flat[(flat.abs() <= 40) & (flat.abs() > 1e-20)]
    assert grid.numel() > 66000 and grid.min().item() == -40.0 and grid.max().item() == 40.0
    for dname in ("bf16", "fp16"):
        assert torch.isfinite(vr.sweep(dname)).all()


@pytest.mark.parametrize("form,act", [("sigmoid", "sigmoid"), ("swish", "swish"), ("gelu", "gelu"), ("gelu_poly", "gelu"),
                                      ("gelu_grad_poly", "gelu_grad")])
def test_activation_bounds_are_attainable_in_float32(form, act):
    """A float32 numpy restatement of the libm forms (and of the kernels' polynomial) passes the bounds of part C on the sweep."""
    x = vr.sweep()
    vr.act_check(torch.from_numpy(vr.f32_forms(x, form)), x, act, "float32 restatement " + form)


def test_plain_swish_form_misses_the_bound_where_its_exponential_overflows():
    """x / (1 + exp(-x)) returns 0 at x = -88.8, where x sigmoid(x) = -2.4e-37 is a normal float: what swishf was before this test"""
    x = vr.sweep()
    with pytest.raises(AssertionError):
        vr.act_check(torch.from_numpy(vr.f32_forms(x, "swish_plain")), x, "swish", "plain swish form")


def test_changed_polynomial_coefficient_misses_the_bound():
    """the bound bites: erf_as's last coefficient changed in the fourth digit fails"""
    x = vr.sweep()
    f = np.float32
    ax = np.abs(x.numpy() * f(0.70710678118654752440))
    t = f(1.0) / (f(0.3275911) * ax + f(1.0))
    p = f(1.061405429) * t + f(-1.453152027)
    for c in (1.421413741, -0.284496736, 0.254929592):               # 0.254829592 in csrc/common.h
        p = p * t + f(c)
    with np.errstate(over="ignore", under="ignore"):
        erf = np.copysign(f(1.0) - p * t * np.exp(-ax * ax), x.numpy())
    with pytest.raises(AssertionError):
        vr.act_check(torch.from_numpy(f(0.5) * x.numpy() * (f(1.0) + erf)), x, "gelu", "changed coefficient")


def test_specials_have_ordinary_neighbours():
    x = vr.specials_tensor()
    bad = ~torch.isfinite(x)
    assert int(bad.sum()) == 5 and int(torch.isnan(x).sum()) == 2
    assert (bad.reshape(-1, 4).sum(1) <= 1).all()                     # at most one per 16-byte access
    assert vr.same_values(x, x.clone()) and not vr.same_values(x, torch.nan_to_num(x, nan=1.5))
    assert math.isnan(vr.SPECIALS[2])
