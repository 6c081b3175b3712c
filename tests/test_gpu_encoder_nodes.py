"""The encoder's tape nodes one by one (csrc/mvit.hip, csrc/mvit_pool.hip, diff_sal_amd/encoder_autograd.py) against the fp64
references of tests/_train_nodes_ref.py.  Wherever the arithmetic is sums of products the operands are integers in [-4, 4]: every
fp32 partial sum is exact in any order, and the assertion is bit-equality with the fp64 result (tests/test_train_nodes_host.py checks
the 2^24 bound, the tie share of the max-pool inputs, and that each comparison here fails for a reference made wrong on purpose)."""
import pytest
import torch

from tests import _train_nodes_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from diff_sal_amd import encoder_autograd, ops

    return ops, encoder_autograd


def to_dev(t):
    """The upload of every case body here; tests/test_gpu_guard_bands.py passes tests/_guard.py's ``put`` in its place."""
    return t.to(DEV)


def dev32(t, up=to_dev):
    return up(t.float())


# ---- relative-position projection ------------------------------------------------------------------------------------------------------
def case_relpos_project_forward_and_backward_are_exact(lib, case, up=to_dev):
    ops, eg = lib
    q_size, k_size, E, BH, D = case
    q, Rs, dE, acc = R.relpos_operands(case)
    qd, Rd, dEd = dev32(q, up), [dev32(r, up) for r in Rs], dev32(dE, up)
    ref = R.relpos_extra64(q, Rs, q_size, k_size, E)
    ex = ops.relpos_project(qd, *Rd, q_size, k_size, E)
    R.check_exact(ex, ref, "extra")
    used = torch.zeros(E, dtype=torch.bool)
    for o, k in zip(R.slot_offsets(E), k_size):
        used[o:o + k] = True
    assert int(ex[..., ~used.to(DEV)].count_nonzero()) == 0 and int(ex[:, :, 0].count_nonzero()) == 0
    # the upstream gradient is non-zero in the unused slots and in the class-token row: none of it may arrive anywhere
    names = ("dq", "dRt", "dRh", "dRw")
    refs = R.relpos_bwd64(q, Rs, dE, q_size, k_size, E)
    got = ops.relpos_project_bwd(dEd, qd, *Rd, q_size, k_size)
    for n, a, b in zip(names, got, refs):
        R.check_exact(a, b, n)
    assert int(got[0][:, :, 0].count_nonzero()) == 0
    # accumulate: the tensor passed in is the one returned, and it holds its old value plus the projection's gradient
    accd = dev32(acc, up)
    refs_acc = R.relpos_bwd64(q, Rs, dE, q_size, k_size, E, dq_accum=acc)
    got_acc = ops.relpos_project_bwd(dEd, qd, *Rd, q_size, k_size, dq_accum=accd)
    assert got_acc[0] is accd
    for n, a, b in zip(names, got_acc, refs_acc):
        R.check_exact(a, b, n + " (accumulate)")
    R.check_exact(accd[:, :, 0], acc[:, :, 0], "class-token row under accumulate")
    # the autograd node
    ql, Rl = qd.clone().requires_grad_(True), [r.clone().requires_grad_(True) for r in Rd]
    out = eg.relpos_project(ql, *Rl, q_size, k_size, E)
    R.check_exact(out, ref, "RelposProjectFn forward")
    (out * dEd).sum().backward()
    for n, a, b in zip(names, [ql.grad] + [r.grad for r in Rl], refs):
        R.check_exact(a, b, n + " (RelposProjectFn)")


@pytest.mark.parametrize("case", R.RELPOS_CASES, ids=R.case_id)
def test_relpos_project_forward_and_backward_are_exact(lib, case):
    case_relpos_project_forward_and_backward_are_exact(lib, case)


@pytest.mark.parametrize("case", R.ATTENTION_CASES, ids=R.case_id)
def test_relpos_attention_node_against_the_two_nodes_and_fp64(lib, case, monkeypatch):
    """RelposAttentionFn (the projection's query gradient accumulates into the attention's dq) against relpos_project +
    attention_general as two nodes (the tape adds the two dq): forward, dk, dv and the table gradients come from the same kernels on
    the same operands -- bit-equal; dq differs by the order of one fp32 addition per element.  Both against fp64 autograd of the dense
    formula with the figure test_attention_general_backward uses for the same quantities (5e-5), here per element."""
    from diff_sal_amd import autograd_ops as ag

    ops, eg = lib
    B, H, q_size, k_size = case
    D, E = 96, ops.relpos_columns(k_size)
    Lq, Lk = 1 + q_size[0] * q_size[1] * q_size[2], 1 + k_size[0] * k_size[1] * k_size[2]
    g = R.generator(41 + Lq)
    q, k, v = (torch.randn(B, H, L, D, generator=g) for L in (Lq, Lk, Lk))
    Rs = [0.2 * torch.randn(a, b, D, generator=g) for a, b in zip(q_size, k_size)]
    G = torch.randn(B, Lq, H * D, generator=g)
    # fp64: softmax(scale q k^T + bias) v, + q on every row but the class token's
    leaves = [t.double().requires_grad_(True) for t in (q, k, v, *Rs)]
    q64, k64, v64 = leaves[:3]
    extra = R.relpos_extra64(q64, leaves[3:], q_size, k_size, E)
    s = (q64 * D ** -0.5) @ k64.transpose(-1, -2) + extra @ ops.relpos_onehot(k_size, E, "cpu").double().t()
    o = s.softmax(-1) @ v64
    o = torch.cat([o[:, :, :1], o[:, :, 1:] + q64[:, :, 1:]], 2).transpose(1, 2).reshape(B, Lq, H * D)
    (o * G.double()).sum().backward()
    onehot = ops.relpos_onehot(k_size, E, DEV)

    def run(fused):
        monkeypatch.setattr(ag, "FUSE_RELPOS", fused)
        lv = [t.to(DEV).requires_grad_(True) for t in (q, k, v, *Rs)]
        out = eg.relpos_attention(*lv, onehot, scale=D ** -0.5, q_size=q_size, k_size=k_size, E=E)
        assert ("RelposAttentionFn" in type(out.grad_fn).__name__) == fused
        (out * G.to(DEV)).sum().backward()
        return out.detach(), [t.grad for t in lv]

    out_f, g_f = run(True)
    out_s, g_s = run(False)
    names = ("dq", "dk", "dv", "dRt", "dRh", "dRw")
    assert torch.equal(out_f, out_s)
    for n, a, b in zip(names[1:], g_f[1:], g_s[1:]):
        assert torch.equal(a, b), n
    w = R.check_bound(g_f[0], g_s[0], 2.0 ** -23 * (g_f[0].abs() + g_s[0].abs()).double(), "dq: fused vs two nodes")
    print(f"{R.case_id(case)}: dq fused vs two nodes, worst ratio to one addition's rounding {w:.3f}")
    for form, out, grads in (("fused", out_f, g_f), ("two nodes", out_s, g_s)):
        worst = R.check_elementwise(out, o, 5e-5, 5e-5, f"out ({form})")
        for n, a, b in zip(names, grads, leaves):
            worst = max(worst, R.check_elementwise(a, b.grad, 5e-5, 5e-5, f"{n} ({form})"))
        print(f"{R.case_id(case)}: {form} vs fp64, worst ratio to the bound {worst:.3f}")


# ---- relative-position tables ----------------------------------------------------------------------------------------------------------
def case_rel_tables_forward_backward_and_an_unused_table(lib, block, D, up=to_dev):
    ops, eg = lib
    plans = tuple({k: up(v) if torch.is_tensor(v) else v for k, v in R.rel_plan(*geom, DEV).items()} for geom in block)
    g = R.generator(77 + D)
    rels = [torch.randn(geom[0], D, generator=g) for geom in block]
    douts = [R.ints(g, (geom[1], geom[2], D)).float() for geom in block]
    outs = ops.rel_tables([up(r) for r in rels], plans)
    worst_f = worst_b = 0.0
    for rel, pl, out in zip(rels, plans, outs):
        ref, tol = R.rel_table64(rel, pl)
        worst_f = max(worst_f, R.check_bound(out, ref, tol, "rel_tables"))
    grads = ops.rel_tables_bwd([up(d) for d in douts], plans)
    for dout, pl, got in zip(douts, plans, grads):
        ref, tol = R.rel_table_bwd64(dout, pl)
        worst_b = max(worst_b, R.check_bound(got, ref, tol, "rel_tables_bwd"))
    print(f"{R.case_id(block)} D={D}: worst ratio to the bound: forward {worst_f:.3f}, backward {worst_b:.3f}")
    # the autograd node; a table whose gathered form nobody uses gets an exactly zero gradient
    for unused in (None, 0, 1, 2):
        leaves = [up(r).requires_grad_(True) for r in rels]
        tabs = eg.rel_tables(*leaves, plans)
        sum((t * up(d)).sum() for i, (t, d) in enumerate(zip(tabs, douts)) if i != unused).backward()
        for i, (leaf, dout, pl) in enumerate(zip(leaves, douts, plans)):
            assert leaf.grad is not None and leaf.grad.shape == leaf.shape
            if i == unused:
                assert int(leaf.grad.count_nonzero()) == 0
            else:
                R.check_bound(leaf.grad, *R.rel_table_bwd64(dout, pl), "RelTablesFn")


@pytest.mark.parametrize("D", R.REL_DS)
@pytest.mark.parametrize("block", R.REL_BLOCKS, ids=R.case_id)
def test_rel_tables_forward_backward_and_an_unused_table(lib, block, D):
    case_rel_tables_forward_backward_and_an_unused_table(lib, block, D)


# ---- max-pool with arg-max -------------------------------------------------------------------------------------------------------------
def case_maxpool_ties_go_to_the_first_window_position(lib, case, C, up=to_dev):
    ops, eg = lib
    for negative in (False, True):
        x, dy = R.maxpool_operands(case, C, negative)
        t_out, t_idx, t_dx = R.maxpool_torch(x, case, dy)
        xd, dyd = up(x), up(dy)
        out, idx = ops.maxpool_tokens_idx(xd, *case)
        R.check_exact(out, t_out, "out")
        R.check_exact(idx, t_idx, "idx")
        R.check_exact(ops.maxpool_tokens_bwd(dyd, idx, *case), t_dx, "dx")
        R.check_exact(ops.maxpool_tokens(xd, *case), t_out, "out (the kernel without the index)")
        xl = xd.clone().requires_grad_(True)
        o = eg.maxpool_tokens(xl, *case)
        o.backward(dyd)
        R.check_exact(o, t_out, "MaxPoolTokensFn forward")
        R.check_exact(xl.grad, t_dx, "MaxPoolTokensFn backward")


@pytest.mark.parametrize("C", R.MAXPOOL_CS)
@pytest.mark.parametrize("case", R.MAXPOOL_CASES, ids=R.case_id)
def test_maxpool_ties_go_to_the_first_window_position(lib, case, C):
    """Inputs from {0, 1, 2}: more than half of the windows tie.  Output, recorded index and input gradient against F.max_pool3d on
    the CPU (first position in (t, y, x) order wins); an all-negative input tells the -3e38 start value from a zero start."""
    case_maxpool_ties_go_to_the_first_window_position(lib, case, C)


# ---- token transposes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", (0, 1))
def test_token_transposes_at_ragged_tiles(lib, off):
    ops, eg = lib
    for L, C, o in R.TRANSPOSE_CASES:
        if o != off:
            continue
        x, dy = R.transpose_operands(L, C, off)
        xd, dyd = x.to(DEV), dy.to(DEV)
        what = f"L={L} C={C} off={off}"
        ref = R.channels_first_ref(x, off)
        R.check_exact(ops.tokens_to_channels_first(xd, off), ref, what)
        xl = xd.clone().requires_grad_(True)
        out = eg.tokens_to_channels_first(xl, off)
        R.check_exact(out, ref, what + " (TokensToChannelsFirstFn)")
        out.backward(dyd)
        R.check_exact(xl.grad, R.channels_first_bwd_ref(dy, off), what + " (TokensToChannelsFirstFn backward)")
        if off:
            assert int(xl.grad[:, :off].count_nonzero()) == 0
        else:                                   # PackTokensFn: [B, C, 1, 1, L] -> [B, L, C], backward = tokens_to_channels_first
            zl = dyd.view(2, C, 1, 1, L).clone().requires_grad_(True)
            tok = eg.pack_tokens(zl)
            R.check_exact(tok, dy.transpose(1, 2), what + " (PackTokensFn)")
            tok.backward(xd)
            R.check_exact(zl.grad, x.transpose(1, 2).reshape(2, C, 1, 1, L), what + " (PackTokensFn backward)")


# ---- pooling convolutions outside the fused path ---------------------------------------------------------------------------------------
def case_qkv_pool_per_tensor_route(lib, param_layout, up=to_dev):
    ops, eg = lib
    c = R.QKVPOOL_CASE
    B, heads, D, size = c["B"], c["heads"], c["D"], c["size"]
    strides = (c["stride_q"], c["stride_kv"], c["stride_kv"])
    g = R.generator(91)
    N = 1 + size[0] * size[1] * size[2]
    qkv = torch.randn(B, N, 3, heads, D, generator=g)
    ws = [0.2 * torch.randn(D, 1, 3, 3, 3, generator=g) for _ in range(3)]
    q64, w64 = qkv.double().requires_grad_(True), [w.double().requires_grad_(True) for w in ws]
    refs = R.qkv_pool64(q64, w64, size, strides)
    Gs = [torch.randn(*r.shape, generator=g) for r in refs]
    sum((r * G.double()).sum() for r, G in zip(refs, Gs)).backward()

    def rel(got, ref):
        ref = ref.detach().double().cpu()
        return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())

    qd = up(qkv).requires_grad_(True)
    wd = [up(w.reshape(D, 27) if param_layout else w.reshape(D, 27).t().contiguous()).requires_grad_(True) for w in ws]
    outs = eg.qkv_pool(qd, *wd, size, strides[0], strides[1])
    sum((o * up(G)).sum() for o, G in zip(outs, Gs)).backward()
    for o, r in zip(outs, refs):
        assert o.shape == r.shape and rel(o, r) < 2e-5
    assert rel(qd.grad, q64.grad) < 5e-5
    for i in range(3):
        ref_dw = w64[i].grad.reshape(D, 27)
        assert rel(wd[i].grad, ref_dw if param_layout else ref_dw.t()) < 5e-5, i


@pytest.mark.parametrize("param_layout", (False, True), ids=("tap-major", "parameter-layout"))
def test_qkv_pool_per_tensor_route(lib, param_layout):
    """D = 64: QKVPoolFn takes the per-tensor pool3d kernels (the one-launch form is D = 96 only); filters tap-major [27, D] or in
    the parameter's own [D, 27] layout.  Against fp64 conv3d autograd, with the figures test_pool_maxpool_relpos_backward uses."""
    case_qkv_pool_per_tensor_route(lib, param_layout)
