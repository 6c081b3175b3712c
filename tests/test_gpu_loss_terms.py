"""CC / SIM / NSS / KL and their fused backward (csrc/metrics.hip) against the fp64 restatement of tests/_train_nodes_ref.py, one term
at a time and element by element: n below, at and off the 64 chunks, B = 1, a binary ground truth, a minimum attained many times,
exact zeros, a nearly flat prediction, images 100 x apart in scale.

The kernels compute in fp64 and round once to fp32, so the bound is rel = 2^-22 per element plus floor * max|ref| with
floor = max(1e-9, (mean(pred)^2 / var(pred)) 2^-48): the second argument is the cancellation of the one-pass variance
sum s^2 - n mu^2 (about 1e-8 on the flat family).  The bound is derived, not measured; every test prints the worst ratio it saw.
tests/test_train_nodes_host.py ties the restatement to the reference's recorded numbers and shows that each of these checks fails
for a gradient without the arg-min spike, with the spike on the last minimum, with a biased NSS, or with one term left out."""
import types

import pytest
import torch

from tests import _train_nodes_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = list(dict.fromkeys(R.LOSS_CASES))


@pytest.fixture(scope="module")
def sl():
    from diff_sal_amd import sal_losses

    return sal_losses


def maps(t):
    """[B, n] -> [B, 1, h, w] on the device."""
    h, w = R.hw_of(t.shape[1])
    return t.reshape(t.shape[0], 1, h, w).to(DEV)


def w4_tensor(w4):
    return torch.tensor(w4, dtype=torch.float32)


@pytest.mark.parametrize("case", CASES + R.FORWARD_ONLY_CASES, ids=R.case_id)
def test_saliency_metrics_per_image_and_means(sl, case):
    pred, gt = R.loss_inputs(*case)
    ref = R.loss_terms64(pred, gt)
    floor = R.loss_floor(pred)
    m = sl.saliency_metrics(maps(pred), maps(gt))
    assert m["per_image"].shape == (case[1], 4)
    worst = R.check_elementwise(m["per_image"], ref, R.LOSS_REL, floor, "per_image")
    means = torch.stack([m[k] for k in R.TERMS])
    worst = max(worst, R.check_elementwise(means, ref.mean(0), R.LOSS_REL, floor, "means"))
    print(f"{R.case_id(case)}: metrics, worst ratio to the bound {worst:.3f} (floor {floor:.1e})")
    if case[0] == "identical":                                               # image 1: pred == gt
        cc, sim, _, kl = (float(v) for v in m["per_image"][1])
        assert abs(cc - 1.0) <= 2.0 ** -22 and abs(sim - 1.0) <= 2.0 ** -22 and abs(kl) <= 1e-9, (cc, sim, kl)


@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_gradient_of_each_term_alone_and_of_a_mix(sl, case):
    """saliency_terms under autograd with w4 = each unit vector, each times an upstream factor of -300, and one mixed w4.  Pixels
    that are not a minimum of pred are compared one by one, the minima by their sum and one by one (the spike sits on the first)."""
    pred, gt = R.loss_inputs(*case)
    floor = R.loss_floor(pred)
    pd, gd = maps(pred), maps(gt)
    worst = {}
    for w4 in R.UNIT_W4 + [R.MIXED_W4]:
        p = pd.clone().requires_grad_(True)
        terms = sl.saliency_terms(p, gd)
        assert terms.shape == (4,)
        (terms * w4_tensor(w4).to(DEV)).sum().backward()
        assert p.grad.shape == p.shape
        ref = R.loss_grad64(pred, gt, w4_tensor(w4))
        worst[w4] = R.check_loss_grad(p.grad.reshape(pred.shape), ref, pred, R.LOSS_REL, floor, f"w4={w4}")
    print(f"{R.case_id(case)}: gradients, worst ratio to the bound {max(worst.values()):.3f} at w4={max(worst, key=worst.get)} (floor {floor:.1e})")


def test_upstream_factor_reaches_the_kernel_as_the_weight(sl):
    """(-300 * terms[k]).backward(): the chain rule's factor arrives in w4 -- the same bits as w4 = -300 e_k."""
    pred, gt = R.loss_inputs("uniform", 2, 1000)
    pd, gd = maps(pred), maps(gt)
    for k in range(4):
        p = pd.clone().requires_grad_(True)
        (R.UPSTREAM * sl.saliency_terms(p, gd)[k]).backward()
        ref = R.loss_grad64(pred, gt, w4_tensor([R.UPSTREAM * (i == k) for i in range(4)]))
        R.check_loss_grad(p.grad.reshape(pred.shape), ref, pred, R.LOSS_REL, R.loss_floor(pred), R.TERMS[k])


def test_get_lossv2_with_all_four_terms(sl):
    pred, gt = R.loss_inputs("uniform", 2, 1000)
    cc_w, sim_w, nss_w, kl_w = R.MIXED_W4
    lc = dict(loss_kl=True, loss_ce=False, loss_mse=False, loss_cc=True, loss_sim=True, loss_nss=True, kl_weight=kl_w, cc_weight=cc_w,
              sim_weight=sim_w, nss_weight=nss_w, mse_weight=1.0, ce_weight=1.0)
    cfg = types.SimpleNamespace(loss=types.SimpleNamespace(**lc))
    p = maps(pred).requires_grad_(True)
    out = sl.get_lossv2(cfg, p, maps(gt))
    out["total"].backward()
    ref = R.loss_terms64(pred, gt).mean(0)
    w = w4_tensor(R.MIXED_W4).double()
    parts = {"cc": w[0] * ref[0], "sim": w[1] * ref[1], "nss": w[2] * ref[2], "main": w[3] * ref[3]}
    got = {k: v.item() for k, v in out.items()}
    for k, v in parts.items():                                               # the term's rounding and the product's: 2 * 2^-24 < 2^-22
        assert abs(got[k] - float(v)) <= 2.0 ** -22 * abs(float(v)) + 1e-9 * float(ref.abs().max()), (k, got[k], float(v))
    mag = sum(abs(float(v)) for v in parts.values())
    assert abs(got["total"] - sum(float(v) for v in parts.values())) <= 2.0 ** -21 * mag      # three more fp32 additions
    worst = R.check_loss_grad(p.grad.reshape(pred.shape), R.loss_grad64(pred, gt, w4_tensor(R.MIXED_W4)), pred, R.LOSS_REL,
                              R.loss_floor(pred), "get_lossv2")
    print(f"get_lossv2: gradient, worst ratio to the bound {worst:.3f}")


def test_a_transposed_view_gives_what_its_contiguous_copy_gives(sl):
    pred, gt = R.loss_inputs("uniform", 2, 1000)
    h, w = R.hw_of(1000)
    base = pred.reshape(2, 1, h, w).transpose(2, 3).contiguous().to(DEV)     # [2, 1, w, h]
    view = base.transpose(2, 3)                                              # [2, 1, h, w], strides (.., 1, h)
    assert not view.is_contiguous() and torch.equal(view.contiguous(), maps(pred))
    gd = maps(gt)
    a, b = sl.saliency_metrics(view, gd), sl.saliency_metrics(maps(pred), gd)
    assert all(torch.equal(a[k], b[k]) for k in R.TERMS + ("per_image",))
    grads = []
    for leaf in (view.detach().requires_grad_(True), maps(pred).requires_grad_(True)):
        (sl.saliency_terms(leaf, gd) * w4_tensor(R.MIXED_W4).to(DEV)).sum().backward()
        grads.append(leaf.grad)
    assert grads[0].shape == grads[1].shape and torch.equal(grads[0], grads[1])
