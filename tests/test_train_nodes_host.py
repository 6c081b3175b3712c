"""tests/_train_nodes_ref.py on the host (no GPU): the fp64 restatement of the loss terms against the reference's recorded numbers,
the closed forms of metric_bwd_kernel against its autograd, the conditions every case of the GPU files relies on, and the power of
every comparison those files make: a reference made wrong on purpose has to fail the same check on the same inputs."""
import numpy as np
import pytest
import torch

from tests import _train_nodes_ref as R


# ---- the restatement is the reference's function ---------------------------------------------------------------------------------------
def test_loss_terms64_reproduces_the_recorded_values(golden_dir):
    m = np.load(f"{golden_dir}/sal_metrics.npz")
    terms = R.loss_terms64(torch.from_numpy(m["pred"]), torch.from_numpy(m["gt"])).mean(0)
    for k, name in enumerate(R.TERMS):
        ref = float(m[name])
        assert abs(float(terms[k]) - ref) < 1e-4 * max(1.0, abs(ref)), (name, float(terms[k]), ref)


@pytest.mark.parametrize("name", ["all", "mse"])
def test_loss_grad64_reproduces_the_recorded_gradients(golden_dir, name):
    """'all' = KL + CC + SIM + NSS; 'mse' = weighted MSE + CC + NSS: the MSE part 2 w (pred - gt) / B is taken off by hand."""
    m = np.load(f"{golden_dir}/sal_metrics.npz")
    g = np.load(f"{golden_dir}/sal_loss_grads.npz")
    pred, gt = torch.from_numpy(m["pred"]), torch.from_numpy(m["gt"])
    kl_w, cc_w, sim_w, nss_w, mse_w = (float(v) for v in g[f"{name}.cfg"])
    gref = torch.from_numpy(g[f"{name}.grad"]).double()
    if name == "mse":
        w4 = (cc_w, 0.0, nss_w, 0.0)
        gref = gref - 2.0 * mse_w / pred.shape[0] * (pred.double() - gt.double())
    else:
        w4 = (cc_w, sim_w, nss_w, kl_w)
    got = R.loss_grad64(pred, gt, w4)
    err = (got - gref).abs().max().item() / gref.abs().max().item()
    print(f"loss_grad64 vs the recorded gradient [{name}]: {err:.2e}")
    assert err < 1e-4


@pytest.mark.parametrize("case", R.LOSS_CASES, ids=R.case_id)
def test_closed_forms_of_the_backward_kernel_agree_with_autograd(case):
    """Two fp64 evaluations of the same gradient: sums of n <= 16385 terms (n 2^-53 = 1.8e-12) through quotients whose conditioning is
    at most mean^2 / var of the flat family (3e6 if a one-pass variance were used; the centred sums here stay near 1e-12).  1e-9
    relative, plus 1e-14 of the largest entry where a gradient passes through zero."""
    pred, gt = R.loss_inputs(*case)
    worst = 0.0
    for w4 in R.UNIT_W4[::2] + [R.MIXED_W4]:
        worst = max(worst, R.check_elementwise(R.loss_grad_closed64(pred, gt, w4), R.loss_grad64(pred, gt, w4), 1e-9, 1e-14,
                                               f"{case} w4={w4}"))
    print(f"{R.case_id(case)}: closed form vs autograd, worst ratio to the bound {worst:.2e}")


def test_the_spike_of_the_reference_sits_on_the_first_minimum():
    assert R.first_min_is_where_torch_puts_it()
    pred, gt = R.loss_inputs("eighths", 2, 300)
    mins = R.minima_mask(pred)
    first = mins.int().argmax(1)
    d = R.loss_grad64(pred, gt, (0, 1.0, 0, 0))
    for b in range(2):
        others = d[b][mins[b]]
        assert d[b, first[b]].abs() > 10 * others[1:].abs().max()            # the one spike, on the first of the 1/8 pixels


# ---- conditions ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.LOSS_CASES + R.FORWARD_ONLY_CASES, ids=R.case_id)
def test_loss_inputs_meet_their_conditions(case):
    family, B, n = case
    pred, gt = R.loss_inputs(*case)
    assert pred.dtype == gt.dtype == torch.float32 and pred.shape == gt.shape == (B, n)
    h, w = R.hw_of(n)
    assert h * w == n
    assert float(pred.max()) <= 1.0 and float(gt.min()) >= 0.0 and float(gt.sum(1).min()) > 0.0
    assert float(pred.min()) > 0.0 or family == "zeros"
    n_min = R.minima_mask(pred).sum(1)
    if family in R.DUPLICATED_MIN:
        assert int(n_min.min()) > 1                                          # and not at the start only: the LAST minimum is another pixel
    else:
        assert int(n_min.max()) == 1, "this case needs a unique minimum of pred"
    assert float((pred.max(1)[0] - pred.min(1)[0]).min()) > 0 and float((gt.max(1)[0] - gt.min(1)[0]).min()) > 0
    if family == "binary":
        assert set(gt.unique().tolist()) == {0.0, 1.0}
    if family == "zeros":
        assert float(pred.min()) == 0.0 and bool((gt[pred == 0] == 0).all()) and float(gt.min()) == 0.0
    if family == "flat":
        assert 5e-9 < R.loss_floor(pred) < 3e-8                              # the cancellation term of the bound decides here
    else:
        assert R.loss_floor(pred) == 1e-9
    if family == "scale100":
        assert 50 < float(pred[0].mean() / pred[1].mean()) < 200 and 50 < float(gt[1].mean() / gt[0].mean()) < 200
    if family == "identical":
        assert torch.equal(pred[1], gt[1]) and not torch.equal(pred[0], gt[0])
        t = R.loss_terms64(pred, gt)[1]
        assert abs(float(t[0]) - 1) < 1e-12 and abs(float(t[1]) - 1) < 1e-12 and abs(float(t[3])) < 1e-9      # log(eps + x / (x + eps)) ~ -eps / x per pixel


def test_loss_shapes_cross_the_chunk_count_and_the_weights_are_fp32_numbers():
    ns = [n for _, n in R.LOSS_SHAPES]
    assert min(ns) < 64 and 64 in ns and 65 in ns and any(n % 64 for n in ns if n > 64) and any(B == 1 for B, _ in R.LOSS_SHAPES)
    assert all(n != 2 for n in ns)                                           # CC's gradient is identically zero at n = 2
    assert len(R.UNIT_W4) == 8 and all(sum(v != 0 for v in w) == 1 for w in R.UNIT_W4)


@pytest.mark.parametrize("case", R.RELPOS_CASES, ids=R.case_id)
def test_relpos_cases_stay_exact_in_fp32(case):
    q_size, k_size, E, BH, D = case
    assert R.relpos_sum_bound(case) < R.LIMIT
    t0, h0, w0 = R.slot_offsets(E)
    assert k_size[0] <= h0 - t0 and k_size[1] <= w0 - h0 and k_size[2] <= E - w0
    q, Rs, dE, acc = R.relpos_operands(case)
    ex = R.relpos_extra64(q, Rs, q_size, k_size, E)
    outs = (ex,) + R.relpos_bwd64(q, Rs, dE, q_size, k_size, E, dq_accum=acc)
    for t in outs:
        assert float(t.abs().max()) < R.LIMIT and torch.equal(t, t.round())
    assert float(ex[:, :, 0].abs().max()) == 0.0                             # class-token row
    used = torch.zeros(E, dtype=torch.bool)
    for o, k in zip((t0, h0, w0), k_size):
        used[o:o + k] = True
    assert float(ex[..., ~used].abs().max() if (~used).any() else 0.0) == 0.0
    assert torch.equal(outs[1][:, :, 0], acc[:, :, 0])                       # dq's class-token row: unchanged under accumulate


def test_relpos_table_reaches_what_it_names():
    full32 = [c for c in R.RELPOS_CASES if c[2] == 32 and c[1][0] == 8] + [c for c in R.RELPOS_CASES if c[2] == 32 and c[1][1:] == (8, 16)]
    assert len(full32) >= 2 and any(c[2] == 48 and c[1][1:] == (16, 24) for c in R.RELPOS_CASES)
    assert any(k % 4 for c in R.RELPOS_CASES for k in c[1])                  # key counts that are no multiple of 4
    assert any(c[3] * c[0][0] * c[0][1] * c[0][2] < 32 for c in R.RELPOS_CASES)      # fewer queries than chunks
    assert {c[4] for c in R.RELPOS_CASES} >= {64, 96, 512}
    two_pass = [c for c in R.RELPOS_CASES if max((k + 3) // 4 for k in c[1]) * (c[4] // 4) > 256]
    assert two_pass and all(c[4] % 4 == 0 and c[4] <= 1024 for c in R.RELPOS_CASES)


@pytest.mark.parametrize("case", R.MAXPOOL_CASES, ids=R.case_id)
def test_maxpool_cases_tie_and_the_walk_is_torchs_rule(case):
    for C in R.MAXPOOL_CS:
        for negative in (False, True):
            x, dy = R.maxpool_operands(case, C, negative)
            share = R.maxpool_tie_share(x, case)
            assert share >= 0.5, share
            out, idx = R.maxpool_ref(x, case)
            t_out, t_idx, t_dx = R.maxpool_torch(x, case, dy)
            R.check_exact(out, t_out, "first-position walk vs F.max_pool3d")
            R.check_exact(idx, t_idx, "first-position walk vs return_indices")
            dx = R.maxpool_bwd_from_idx(dy, t_idx, x.shape[1])
            R.check_exact(dx, t_dx, "scatter by index vs autograd")
            assert float(dx.abs().max()) < R.LIMIT
            assert float(x.max()) < 0 or not negative
    print(f"{R.case_id(case)}: tie share {share:.2f}")


def test_rel_plans_have_two_tap_rows_and_identity_rows():
    kinds = set()
    for geom in R.REL_GEOMS + list(R.REL_MIXED):
        pl = R.rel_plan(*geom)
        kinds.add(bool((pl["w2"][:, 1] != 0).any()))
        assert int(pl["csr_ptr"][-1]) == pl["csr_col"].numel() and pl["idx2"].shape == (geom[1] * geom[2], 2)
    assert kinds == {False, True}                                            # tables of the grid's own length and resampled ones
    assert len(set(R.REL_MIXED)) == 3 and all(2 * max(q, k) - 1 == n for n, q, k in R.REL_GEOMS)


def test_copy_plan_has_gaps_and_both_alignments():
    for count in R.COPY_COUNTS:
        plan, offs, total = R.copy_plan(count)
        assert len(plan) == count and all(o % 64 == 0 for o in offs)
        ends = [o + n for o, (n, _) in zip(offs, plan)]
        assert all(e < o2 for e, o2 in zip(ends, offs[1:])) and ends[-1] < total and offs[0] > 0
    plan, _, _ = R.copy_plan(100)
    assert {(n, m) for n, m in plan} == {(n, m) for n in R.COPY_SIZES for m in (False, True)}
    assert 48 in R.COPY_COUNTS and 49 in R.COPY_COUNTS


# ---- power: a wrong reference fails the same check on the same inputs ---------------------------------------------------------------------
SIM, NSS = (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0)


def fails(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


@pytest.mark.parametrize("case", R.LOSS_CASES, ids=R.case_id)
def test_power_of_the_loss_gradient_check(case):
    pred, gt = R.loss_inputs(*case)
    floor = R.loss_floor(pred)

    def chk(got, w4):
        return R.check_loss_grad(got, R.loss_grad64(pred, gt, w4), pred, R.LOSS_REL, floor, R.case_id(case))

    for w4 in (SIM, NSS, R.MIXED_W4):
        chk(R.loss_grad_closed64(pred, gt, w4).float(), w4)                  # the right answer, rounded once to fp32, passes
    for w4 in (SIM, tuple(R.UPSTREAM * v for v in SIM), R.MIXED_W4):
        fails(chk, R.loss_grad_closed64(pred, gt, w4, spike=False).float(), w4)
    if case[0] in R.DUPLICATED_MIN:
        fails(chk, R.loss_grad_closed64(pred, gt, SIM, last_min=True).float(), SIM)
        fails(chk, R.loss_grad_closed64(pred, gt, R.MIXED_W4, last_min=True).float(), R.MIXED_W4)
    fails(chk, R.loss_grad_closed64(pred, gt, NSS, biased_std=True).float(), NSS)
    for k in range(4):                                                       # one term's weight dropped from the mix
        w = tuple(0.0 if i == k else v for i, v in enumerate(R.MIXED_W4))
        fails(chk, R.loss_grad_closed64(pred, gt, w).float(), R.MIXED_W4)


@pytest.mark.parametrize("case", R.LOSS_CASES + R.FORWARD_ONLY_CASES, ids=R.case_id)
def test_power_of_the_loss_value_check(case):
    """per_image [B, 4]: NSS with the biased standard deviation (a factor sqrt(n / (n - 1))) and a SIM that skips the min-max step."""
    pred, gt = R.loss_inputs(*case)
    ref = R.loss_terms64(pred, gt)
    floor = R.loss_floor(pred)
    R.check_elementwise(ref.float(), ref, R.LOSS_REL, floor)
    n = case[2]
    wrong = ref.clone()
    wrong[:, 2] *= (n / (n - 1)) ** 0.5
    fails(R.check_elementwise, wrong.float(), ref, R.LOSS_REL, floor)
    s, g = pred.double(), gt.double()
    wrong = ref.clone()
    wrong[:, 1] = torch.minimum(s / s.sum(1, keepdim=True), g / g.sum(1, keepdim=True)).sum(1)
    if case[0] != "zeros":                                                   # min pred = 0 there: the min-max step is the identity
        fails(R.check_elementwise, wrong.float(), ref, R.LOSS_REL, floor)


@pytest.mark.parametrize("case", R.RELPOS_CASES, ids=R.case_id)
def test_power_of_the_relpos_checks(case):
    q_size, k_size, E, BH, D = case
    q, Rs, dE, acc = R.relpos_operands(case)
    ex = R.relpos_extra64(q, Rs, q_size, k_size, E)
    R.check_exact(ex.float(), ex)
    fails(R.check_exact, R.relpos_extra64(q, Rs, q_size, k_size, E, swap_hw=True).float(), ex, "slots swapped")
    ref = R.relpos_bwd64(q, Rs, dE, q_size, k_size, E, dq_accum=acc)
    fails(R.check_exact, R.relpos_bwd64(q, Rs, dE, q_size, k_size, E, dq_accum=acc, overwrite=True)[0].float(), ref[0], "overwrite")
    wrong = R.relpos_bwd64(q, Rs, dE, q_size, k_size, E, swap_hw=True)
    fails(R.check_exact, wrong[0].float(), R.relpos_bwd64(q, Rs, dE, q_size, k_size, E)[0], "dq with the slots swapped")
    if k_size[1] > 1 or k_size[2] > 1:                                       # one key per axis: the swapped slots hold dE values of the same law
        assert any(not torch.equal(a, b) for a, b in zip(wrong[2:], ref[2:]))


@pytest.mark.parametrize("case", R.MAXPOOL_CASES, ids=R.case_id)
def test_power_of_the_maxpool_checks(case):
    x, dy = R.maxpool_operands(case, 4)
    out, idx = R.maxpool_ref(x, case)
    out_l, idx_l = R.maxpool_ref(x, case, last=True)
    R.check_exact(out_l, out)                                                # the values cannot tell the two rules apart ...
    fails(R.check_exact, idx_l, idx, "tie to the last position")             # ... the index and the gradient do
    fails(R.check_exact, R.maxpool_bwd_from_idx(dy, idx_l, x.shape[1]), R.maxpool_bwd_from_idx(dy, idx, x.shape[1]), "dx")
    xn, _ = R.maxpool_operands(case, 4, negative=True)
    zero_start = torch.maximum(R.maxpool_ref(xn, case)[0], torch.zeros(()))
    zero_start[:, 0] = xn[:, 0]
    fails(R.check_exact, zero_start, R.maxpool_ref(xn, case)[0], "maximum started at zero")


@pytest.mark.parametrize("block", R.REL_BLOCKS, ids=R.case_id)
def test_power_of_the_rel_table_checks(block):
    g = R.generator(9)
    for geom in set(block):
        pl = R.rel_plan(*geom)
        for D in R.REL_DS:
            rel = torch.randn(geom[0], D, generator=g)
            ref, tol = R.rel_table64(rel, pl)
            R.check_bound(ref.float(), ref, tol)
            other = dict(pl, w2=pl["w2"].flip(1))                            # the two taps' weights exchanged
            if bool((pl["w2"][:, 1] != 0).any()):
                fails(R.check_bound, R.rel_table64(rel, other)[0].float(), ref, tol, "weights exchanged")
            fails(R.check_bound, R.rel_table64(rel.roll(1, 0), pl)[0].float(), ref, tol, "rows off by one")
            dout = R.ints(g, (geom[1], geom[2], D))
            dref, dtol = R.rel_table_bwd64(dout, pl)
            R.check_bound(dref.float(), dref, dtol)
            row = int((pl["csr_ptr"][1:] - pl["csr_ptr"][:-1]).argmax())
            fails(R.check_bound, R.rel_table_bwd64(dout, pl, drop_row=row)[0].float(), dref, dtol, "one CSR row missing")


def test_power_of_the_transpose_checks():
    for L, C, off in R.TRANSPOSE_CASES:
        x, dy = R.transpose_operands(L, C, off)
        ref = R.channels_first_ref(x, off)
        assert ref.shape == (2, C, L)
        R.check_exact(x[:, off:].permute(0, 2, 1), ref)
        if off:
            fails(R.check_exact, R.channels_first_ref(x, off, ignore_off=True), ref, "off ignored")
            back = R.channels_first_bwd_ref(dy, off)
            assert back.shape == x.shape and float(back[:, 0].abs().max()) == 0.0
            fails(R.check_exact, R.channels_first_bwd_ref(dy, 0)[:, :L], back[:, :L], "gradient rows not shifted")


def test_power_of_the_one_addition_criterion():
    """|a - b| <= 2^-23 (|a| + |b|): passes for the two roundings of one sum, fails for a sum that lost a term of relative size 1e-6."""
    g = R.generator(3)
    a, b = torch.randn(4096, generator=g), torch.randn(4096, generator=g) * 0.3
    s = a + b
    s_up = torch.nextafter(s, torch.full_like(s, float("inf")))
    R.check_bound(s_up, s, 2.0 ** -23 * (s.abs() + s_up.abs()).double())
    lost = (a.double() + b.double() * (1 - 1e-5)).float()
    fails(R.check_bound, lost, s, 2.0 ** -23 * (s.abs() + lost.abs()).double())
