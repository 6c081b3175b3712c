"""Every lane-group instantiation of the row, attention and pooling kernels at op level (tables: tests/_instantiation_cases.py,
their coverage: tests/test_instantiation_cases_host.py).  References are the same formulas in float64 torch on the CPU; the error
measure is max |got - ref| / max |ref| with the bounds of the neighbouring op tests.  Before each op a NaN-filled block of every
output's size is allocated and freed, so the wrapper's torch.empty gets it back and an element the kernel never writes shows as
NaN; the last float4 piece of the width (of each head's slice) is measured on its own so a wrong ragged tail is named."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import mvit_oracle as mo
from oracle import salunet_oracle as orc
from tests import _instantiation_cases as ic
from tests.test_gpu_lowp import DTYPES, OP_RTOL, q as q16

pytestmark = pytest.mark.gpu
DEV = "cuda"


def to_dev(t):
    """The upload of every case body here; tests/test_gpu_guard_bands.py passes tests/_guard.py's ``put`` in its place."""
    return t.to(DEV)

FWD_TOL = 2e-5          # fp32 forward (test_gpu_ops.py)
ATTN_BWD_TOL = 5e-5     # attention backward (test_gpu_train_ops.py)
LN_BWD_TOL = 2e-5       # LayerNorm-family backward (test_gpu_train_ops.py)
# pooling backward: dx is at most 27 fp32 fmas per element (27 * 2^-24 = 1.6e-6 of the largest term); the filter gradient adds at
# most B * heads * To * Ho * Wo = 420 fp32 terms per lane before the fp64 partial sums (random-walk growth: ~20 * 6e-8 = 1.2e-6).
# Both sit under the fp32 forward bound, which is what is asserted.
POOL_BWD_TOL = 2e-5

WORST = {}              # family -> (largest measured error, case)


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for fam in sorted(WORST):
        print(f"\n[instantiations] {fam}: largest error {WORST[fam][0]:.3e} at {WORST[fam][1]}", end="")
    print()


@pytest.fixture(scope="module")
def ops():
    from diff_sal_amd import ops as o

    assert torch.cuda.is_available()
    return o


def rnd(name, *shape, scale=1.0):
    return orc.synth_tensor(name, shape, scale)


def poison(*like):
    """NaN blocks of the outputs' sizes, freed at once: the caching allocator hands them to the next torch.empty of that size.
    like: tensors, or (numel, dtype)."""
    blocks = [torch.full((t.numel(),) if torch.is_tensor(t) else (t[0],), float("nan"), device=DEV,
                         dtype=t.dtype if torch.is_tensor(t) else t[1]) for t in like]
    del blocks


@pytest.mark.parametrize("numel", [1000, 1 << 20])
def test_poison_reaches_the_next_allocation(numel):
    """What the never-written check rests on: the freed NaN block is what the next torch.empty of that size gets."""
    poison((numel, torch.float32))
    assert torch.isnan(torch.empty(numel, device=DEV)).all()


def check(got, ref, tol, family, case, tail=4, heads=1):
    """got against the float64 reference: no NaN, the last float4 piece of every head's slice, then the whole tensor."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (family, case, got.shape, ref.shape)
    assert not torch.isnan(got).any(), f"{family} {case}: {int(torch.isnan(got).sum())} output elements were never written"
    den = ref.abs().max().item() + 1e-300
    d = got.shape[-1] // heads
    cut = lambda t: t.reshape(*t.shape[:-1], heads, d)[..., d - tail:]      # noqa: E731
    e_tail = (cut(got) - cut(ref)).abs().max().item() / den
    e = (got - ref).abs().max().item() / den
    if e > WORST.get(family, (-1.0, None))[0]:
        WORST[family] = (e, case)
    assert e_tail < tol, f"{family} {case}: last float4 piece of the width off by {e_tail:.3e} (bound {tol:g})"
    assert e < tol, f"{family} {case}: error {e:.3e} (bound {tol:g})"
    return e


# ---- a. attention forward ------------------------------------------------------------------------------------------------------

def attention_ref(qq, k, v, heads, scale):
    n, Lq, C = qq.shape
    d = C // heads
    qh, kh, vh = (t.reshape(n, -1, heads, d).transpose(1, 2) for t in (qq, k, v))
    return (F.softmax(qh @ kh.transpose(-1, -2) * scale, -1) @ vh).transpose(1, 2).reshape(n, Lq, C)


@functools.lru_cache(maxsize=None)
def attention_inputs(C, heads, Lk, dname):
    """(q, k, v) as the kernel sees them (rounded to the storage type) and the float64 result; N = 2 checks the image stride."""
    Lq = ic.attention_lq(C // heads)
    qkv = [rnd(f"ia{nm}", 2, L, C) for nm, L in (("q", Lq), ("k", Lk), ("v", Lk))]
    if dname != "fp32":
        qkv = [q16(t, DTYPES[dname]) for t in qkv]
    return qkv, attention_ref(*(t.double() for t in qkv), heads, C ** -0.5)


def run_attention_forward(ops, case, dname, family, up=to_dev):
    C, heads, Lk, _ = case
    (qq, k, v), ref = attention_inputs(C, heads, Lk, dname)
    dt = torch.float32 if dname == "fp32" else DTYPES[dname]
    qd, kd, vd = (up(t.to(dt)) for t in (qq, k, v))
    poison(qd)
    got = ops.attention(qd, kd, vd, heads, C ** -0.5)
    check(got, ref, FWD_TOL if dname == "fp32" else OP_RTOL[dname], family, ic.attention_id(case), heads=heads)


@pytest.mark.parametrize("case", ic.ATTN_FWD_CASES, ids=ic.attention_id)
def test_attention_forward_fp32(ops, case):
    """The exact-160-KiB case (id ...-lds160KiB) is the largest K | V tile diffsal_attention accepts."""
    run_attention_forward(ops, case, "fp32", "attention fwd fp32")


@pytest.mark.parametrize("generic", [True, False], ids=["generic", "planned"])
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("case", ic.ATTN_FWD_CASES, ids=ic.attention_id)
def test_attention_forward_16bit(ops, tuning, case, dname, generic):
    """generic: DIFFSAL_NO_STREAM16 = 1, so attention_kernel<LK, G, T> runs; planned: the switch unset, where a shape that falls off
    the 16-byte and matrix-core forms must still land on a correct kernel.  Same reference for both."""
    if generic:
        tuning.set("DIFFSAL_NO_STREAM16", 1)
    run_attention_forward(ops, case, dname, f"attention fwd {dname} {'generic' if generic else 'planned'}")


# ---- b. attention backward -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def attention_bwd_reference(C, heads, Lk):
    Lq = ic.attention_lq(C // heads)
    qq, k, v = (rnd(f"ib{nm}", 2, L, C).double().requires_grad_(True) for nm, L in (("q", Lq), ("k", Lk), ("v", Lk)))
    go = rnd("ibgo", 2, Lq, C)
    attention_ref(qq, k, v, heads, C ** -0.5).backward(go.double())
    return tuple(t.detach().float() for t in (qq, k, v)) + (go,), (qq.grad, k.grad, v.grad)


def case_attention_backward(ops, case, up=to_dev):
    C, heads, Lk, _ = case
    (qq, k, v, go), grads = attention_bwd_reference(C, heads, Lk)
    qd, kd, vd, god = (up(t) for t in (qq, k, v, go))
    ld = (heads * Lk + 3) // 4 * 4
    poison(qd, (qd.shape[0] * qd.shape[1] * ld, torch.float32), (qd.shape[0] * qd.shape[1] * ld, torch.float32),
           (2 * ld * C, torch.float32), (2 * ld * C, torch.float32))
    got = ops.attention_bwd(qd, kd, vd, god, heads, C ** -0.5)
    for name, g_, r_ in zip(("dq", "dk", "dv"), got, grads):
        check(g_, r_, ATTN_BWD_TOL, f"attention bwd {name}", ic.attention_id(case), heads=heads)


@pytest.mark.parametrize("case", ic.ATTN_BWD_CASES, ids=ic.attention_id)
def test_attention_backward(ops, case):
    case_attention_backward(ops, case)


@pytest.mark.parametrize("C,heads,Lk", ic.ATTN_AUTOGRAD)
def test_attention_autograd_end_to_end(C, heads, Lk):
    from diff_sal_amd import autograd_ops

    (qq, k, v, go), grads = attention_bwd_reference(C, heads, Lk)
    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (qq, k, v))
    out = autograd_ops.attention(qd, kd, vd, heads, C ** -0.5)
    check(out, attention_ref(qq.double(), k.double(), v.double(), heads, C ** -0.5), FWD_TOL, "attention autograd fwd", (C, heads, Lk), heads=heads)
    out.backward(go.to(DEV))
    for name, t, r_ in zip(("dq", "dk", "dv"), (qd, kd, vd), grads):
        check(t.grad, r_, ATTN_BWD_TOL, f"attention autograd {name}", (C, heads, Lk), heads=heads)


def test_attention_backward_refuses_a_bad_width_before_any_launch(ops, monkeypatch):
    """C % 32 != 0 (what the pass-2 GEMM needs) is an argument error: no library entry may have been called when it is raised."""
    def launched(*a, **k):
        raise AssertionError("attention_bwd called into the library before it refused the width")

    monkeypatch.setattr(ops._lib, "check", launched)
    z = torch.zeros(1, 8, 48, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ops.attention_bwd(z, z[:, :2], z[:, :2], z, 2, 48 ** -0.5)


# ---- c. row family ---------------------------------------------------------------------------------------------------------------

def ln_params(C, tag=""):
    return rnd(f"ig{tag}", C, scale=0.2) + 1.0, rnd(f"ib{tag}", C, scale=0.2)


def ln_ref(x, g, b, eps=1e-5):
    return F.layer_norm(x.double(), (x.shape[-1],), g.double(), b.double(), eps)


@functools.lru_cache(maxsize=None)
def ln_inputs(C, M, dname):
    x = rnd(f"ilx{C}", M, C) * 1.5 + 0.3
    if dname != "fp32":
        x = q16(x, DTYPES[dname])
    g, b = ln_params(C)
    return x, g, b, ln_ref(x, g, b)


def run_layernorm(ops, C, dname, family, up=to_dev):
    dt = torch.float32 if dname == "fp32" else DTYPES[dname]
    for M in ic.row_counts(C):
        x, g, b, ref = ln_inputs(C, M, dname)
        xd = up(x.to(dt))
        poison(xd)
        got = ops.layernorm(xd, up(g), up(b), 1e-5)
        check(got, ref, FWD_TOL if dname == "fp32" else OP_RTOL[dname], family, f"C={C} M={M}", tail=min(4, C))


@pytest.mark.parametrize("C", ic.ROW_WIDTHS)
def test_layernorm_fp32(ops, C):
    run_layernorm(ops, C, "fp32", "layernorm fp32")


@pytest.mark.parametrize("generic", [True, False], ids=["generic", "planned"])
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("C", ic.ROW_WIDTHS)
def test_layernorm_16bit(ops, tuning, C, dname, generic):
    if generic:
        tuning.set("DIFFSAL_NO_STREAM16", 1)
    run_layernorm(ops, C, dname, f"layernorm {dname} {'generic' if generic else 'planned'}")


def multi_rows(C, n):
    many = ic.row_counts(C)[0]
    return ([many], [many, 1], [7, many, 1])[n - 1]


def case_layernorm_multi(ops, C, up=to_dev):
    for n in (1, 2, 3):
        xs = [rnd(f"imx{C}_{t}", M, C) * 1.5 + 0.3 for t, M in enumerate(multi_rows(C, n))]
        gb = [ln_params(C, str(t)) for t in range(n)]
        eps = [1e-5, 1e-6, 1e-5][:n]
        xd = [up(x) for x in xs]
        gd, bd = [up(g) for g, _ in gb], [up(b) for _, b in gb]
        poison(*xd)
        got = ops.layernorm_multi(xd, gd, bd, eps)
        for t in range(n):
            check(got[t], ln_ref(xs[t], *gb[t], eps[t]), FWD_TOL, "layernorm_multi", f"C={C} n={n} tensor {t}", tail=min(4, C))
            assert torch.equal(got[t], ops.layernorm(xd[t], gd[t], bd[t], eps[t])), (C, n, t)


@pytest.mark.parametrize("C", ic.ROW_WIDTHS)
def test_layernorm_multi(ops, C):
    """Up to three tensors of one width in one launch: bit-equal to a launch per tensor, and within the bound of float64."""
    case_layernorm_multi(ops, C)


@functools.lru_cache(maxsize=None)
def ln_bwd_reference(C, M, tag=""):
    x = (rnd(f"ibx{C}{tag}", M, C) * 1.7 + 0.2)
    g, b = ln_params(C, tag)
    dy, add = rnd(f"ibdy{tag}", M, C), rnd(f"ibadd{tag}", M, C)
    xr, gr, br = (t.double().requires_grad_(True) for t in (x, g, b))
    F.layer_norm(xr, (C,), gr, br, 1e-5).backward(dy.double())
    return (x, g, dy, add), (xr.grad, gr.grad, br.grad)


def run_layernorm_bwd(ops, C, M, up=to_dev):
    from diff_sal_amd import _lib

    (x, g, dy, add), (dx, dg, db) = ln_bwd_reference(C, M)
    xd, gd, dyd, addd = (up(t) for t in (x, g, dy, add))
    part = (_lib.load().diffsal_layernorm_bwd_blocks(M, C) * 2 * C, torch.float64)
    for with_add in (False, True):
        poison(xd, part, (2 * C, torch.float32))
        got = ops.layernorm_bwd(xd, dyd, gd, 1e-5, add=addd if with_add else None)
        case = f"C={C} M={M}" + (" +add" if with_add else "")
        check(got[0], dx + add.double() if with_add else dx, LN_BWD_TOL, "layernorm_bwd dx", case, tail=min(4, C))
        check(got[1], dg, LN_BWD_TOL, "layernorm_bwd dgamma", case, tail=min(4, C))
        check(got[2], db, LN_BWD_TOL, "layernorm_bwd dbeta", case, tail=min(4, C))


@pytest.mark.parametrize("C", ic.ROW_WIDTHS)
def test_layernorm_backward(ops, C):
    for M in ic.row_counts(C):
        run_layernorm_bwd(ops, C, M)


def case_layernorm_backward_multi(ops, C, up=to_dev):
    for n in (1, 2, 3):
        refs = [ln_bwd_reference(C, M, str(t)) for t, M in enumerate(multi_rows(C, n))]
        xd, dyd, gd = ([up(r[0][i]) for r in refs] for i in (0, 2, 1))
        poison(*xd)
        dxs, dgs, dbs = ops.layernorm_bwd_multi(xd, dyd, gd, [1e-5] * n)
        for t in range(n):
            case = f"C={C} n={n} tensor {t}"
            check(dxs[t], refs[t][1][0], LN_BWD_TOL, "layernorm_bwd_multi dx", case, tail=min(4, C))
            check(dgs[t], refs[t][1][1], LN_BWD_TOL, "layernorm_bwd_multi dgamma", case, tail=min(4, C))
            check(dbs[t], refs[t][1][2], LN_BWD_TOL, "layernorm_bwd_multi dbeta", case, tail=min(4, C))


@pytest.mark.parametrize("C", ic.ROW_WIDTHS)
def test_layernorm_backward_multi(ops, C):
    case_layernorm_backward_multi(ops, C)


def dwconv3_ref(x, w9, g, b):
    """x NHWC, w9 [9][C] -> LayerNorm of the depthwise 3x3 (pad 1) as tokens [N, H*W, C], float64."""
    C = x.shape[-1]
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w9.double().t().reshape(C, 1, 3, 3), padding=1, groups=C)
    return ln_ref(y.flatten(2).transpose(1, 2), g, b)


def dwpool_ref(x, wkk, g, b, k):
    C = x.shape[-1]
    y = F.conv2d(x.double().permute(0, 3, 1, 2), wkk.double().t().reshape(C, 1, k, k), stride=k, groups=C)
    return ln_ref(y.flatten(2).transpose(1, 2), g, b)


def case_dwconv3_ln(ops, C, W, up=to_dev):
    N, H = ic.DWCONV_NH
    x, w9 = rnd(f"idx{C}", N, H, W, C), rnd("idw9", 9, C, scale=0.3)
    g, b = ln_params(C, "q")
    xd = up(x)
    poison(xd)
    got = ops.dwconv3_ln(xd, up(w9), up(g), up(b))
    check(got, dwconv3_ref(x, w9, g, b), FWD_TOL, "dwconv3_ln", f"C={C} W={W}", tail=min(4, C))


@pytest.mark.parametrize("W", ic.DWCONV_WS)
@pytest.mark.parametrize("C", ic.ROW_WIDTHS)
def test_dwconv3_ln(ops, C, W):
    """W = 19: the strip kernel for C <= 256 (ragged last strip of 3 pixels); W = 15: the generic kernel."""
    case_dwconv3_ln(ops, C, W)


def case_dwpool_ln_kv(ops, C, up=to_dev):
    H, W = ic.DWPOOL_HW
    xk, xv = rnd(f"ipk{C}", 2, H, W, C), rnd(f"ipv{C}", 2, H, W, C)
    (gk, bk), (gv, bv) = ln_params(C, "k"), ln_params(C, "v")
    for k in ic.DWPOOL_KS:
        wk, wv = rnd("ipwk", k * k, C, scale=1.0 / k), rnd("ipwv", k * k, C, scale=1.0 / k)
        n_out = 2 * (H // k) * (W // k) * C
        poison((n_out, torch.float32), (n_out, torch.float32))
        got_k, got_v = ops.dwpool_ln_kv(*(up(t) for t in (xk, xv, wk, wv, gk, bk, gv, bv)), k)
        check(got_k, dwpool_ref(xk, wk, gk, bk, k), FWD_TOL, "dwpool_ln_kv k", f"C={C} k={k}", tail=min(4, C))
        check(got_v, dwpool_ref(xv, wv, gv, bv, k), FWD_TOL, "dwpool_ln_kv v", f"C={C} k={k}", tail=min(4, C))


@pytest.mark.parametrize("C", ic.ROW_WIDTHS)
def test_dwpool_ln_kv(ops, C):
    case_dwpool_ln_kv(ops, C)


def case_qkv_prep_equals_the_two_entries(ops, C, W, up=to_dev):
    N, H = ic.DWCONV_NH
    dv = up
    xn, xa = dv(rnd(f"iqn{C}", N, H, W, C)), dv(rnd(f"iqa{C}", N, H, W, C))
    w9 = dv(rnd("iqw9", 9, C, scale=0.3))
    norms = [tuple(dv(t) for t in ln_params(C, f"q{i}")) for i in range(4)]
    for k in ic.DWPOOL_KS:
        wk, wv = dv(rnd("iqwk", k * k, C, scale=1.0 / k)), dv(rnd("iqwv", k * k, C, scale=1.0 / k))
        qq = ops.dwconv3_ln(xn, w9, *norms[0])
        kk, vv = ops.dwpool_ln_kv(xa, xn, wk, wv, *norms[1], *norms[2], k)
        kvw = (wk, wv, *norms[1], *norms[2], k)
        poison(qq, kk, vv)
        got = ops.qkv_prep(xn, w9, *norms[0], xa, xn, *kvw)
        assert not any(torch.isnan(t).any() for t in got), (C, W, k)
        assert torch.equal(got[0], qq) and torch.equal(got[1], kk) and torch.equal(got[2], vv), (C, W, k)
        normed = ops.layernorm(xn, *norms[3], 1e-5)
        for ln_k in (True, False):
            ref3 = ops.qkv_prep(normed, w9, *norms[0], normed if ln_k else xa, normed, *kvw)
            poison(qq, kk, vv)
            got3 = ops.qkv_prep(xn, w9, *norms[0], xn if ln_k else xa, xn, *kvw, pre_ln=(*norms[3], 1e-5, ln_k))
            assert not any(torch.isnan(t).any() for t in got3), (C, W, k, ln_k)
            assert all(torch.equal(r_, g_) for r_, g_ in zip(ref3, got3)), (C, W, k, ln_k)


@pytest.mark.parametrize("W", ic.DWCONV_WS)
@pytest.mark.parametrize("C", ic.ROW_WIDTHS)
def test_qkv_prep_equals_the_two_entries(ops, C, W):
    """The merged launch == dwconv3_ln + dwpool_ln_kv bit for bit, and the block's first LayerNorm folded into the loads ==
    a layernorm launch in front (key input normalised or not): the property of test_depthwise_projections on every width."""
    case_qkv_prep_equals_the_two_entries(ops, C, W)


def test_row_entries_refuse_more_than_1024_channels(ops):
    """Argument checks before any launch (DIFFSAL_E_SHAPE = -1), as in test_conv_igemm_rejects_bad_channels."""
    C = ic.ROW_REJECTED_WIDTH
    x, v = torch.zeros(3, C, device=DEV), torch.zeros(C, device=DEV)
    with pytest.raises(RuntimeError, match=r"layernorm failed \(code -1\).*1028 > 1024"):
        ops.layernorm(x, v, v)
    with pytest.raises(RuntimeError, match=r"dwconv3_ln failed \(code -1\).*1028 > 1024"):
        ops.dwconv3_ln(torch.zeros(1, 2, 16, C, device=DEV), torch.zeros(9, C, device=DEV), v, v)
    with pytest.raises(RuntimeError, match=r"layernorm_bwd failed \(code -1\).*1028 > 1024"):
        ops.layernorm_bwd(x, x, v)


def case_layernorm_past_the_grid_cap(ops, C, M, up=to_dev):
    x, g, b, ref = ln_inputs(C, M, "fp32")
    xd = up(x)
    poison(xd)
    check(ops.layernorm(xd, up(g), up(b), 1e-5), ref, FWD_TOL, "layernorm past the grid cap", f"C={C} M={M}")


@pytest.mark.parametrize("C,M", ic.LN_PAST_CAP)
def test_layernorm_past_the_grid_cap(ops, C, M):
    """More rows than 8192 workgroups hold: the grid-stride loop."""
    case_layernorm_past_the_grid_cap(ops, C, M)


@pytest.mark.parametrize("C,M", ic.LN_BWD_PAST_CAP)
def test_layernorm_backward_past_the_grid_cap(ops, C, M):
    """More rows than 1024 workgroups hold: the grid-stride loop and the double partial sums of several rows per lane group."""
    run_layernorm_bwd(ops, C, M)


def case_dwconv3_ln_strip_kernel_past_the_grid_cap(ops, up=to_dev):
    N, H, W, C = ic.DWCONV_STRIP_PAST_CAP
    x, w9 = rnd("isx", N, H, W, C), rnd("isw9", 9, C, scale=0.3)
    g, b = ln_params(C, "s")
    xd, w9d, gd, bd = (up(t) for t in (x, w9, g, b))
    poison(xd)
    whole = ops.dwconv3_ln(xd, w9d, gd, bd)
    assert not torch.isnan(whole).any()
    halves = torch.cat([ops.dwconv3_ln(xd[:N // 2], w9d, gd, bd), ops.dwconv3_ln(xd[N // 2:], w9d, gd, bd)])
    assert torch.equal(whole, halves)
    check(whole[-1:], dwconv3_ref(x[-1:], w9, g, b), FWD_TOL, "dwconv3_ln strip past the grid cap", f"N={N} H={H} W={W} C={C}")


def test_dwconv3_ln_strip_kernel_past_the_grid_cap(ops):
    """The first batch whose strips exceed 8192 workgroups x 4 lane groups (G = 64): the whole batch against its two halves (each
    under the cap) bit for bit, and the last image -- where the second trip of the grid-stride loop lands -- against float64."""
    case_dwconv3_ln_strip_kernel_past_the_grid_cap(ops)


# ---- d. MViT pooling -------------------------------------------------------------------------------------------------------------

def pool_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else f"D{v}"


@functools.lru_cache(maxsize=None)
def pool_inputs(D):
    N = 1 + ic.POOL_SIZE[0] * ic.POOL_SIZE[1] * ic.POOL_SIZE[2]
    return (rnd(f"iPq{D}", ic.POOL_B, N, 3, ic.POOL_HEADS, D), rnd(f"iPw{D}", D, 1, 3, 3, 3, scale=0.2),
            rnd("iPg", D, scale=0.1) + 1, rnd("iPb", D, scale=0.1))


def case_pool3d_ln(ops, D, stride, up=to_dev):
    qkv, w, g, b = pool_inputs(D)
    ref, ref_size = mo.attention_pool(qkv[:, :, 1].permute(0, 2, 1, 3).double(), w.double(), stride, ic.POOL_SIZE, g.double(), b.double())
    To, Ho, Wo = ((s - 1) // st + 1 for s, st in zip(ic.POOL_SIZE, stride))
    poison((ic.POOL_B * ic.POOL_HEADS * (1 + To * Ho * Wo) * D, torch.float32))
    got, out_size = ops.pool3d_ln(up(qkv)[:, :, 1], up(w.reshape(D, 27).t().contiguous()), up(g), up(b), ic.POOL_SIZE, stride)
    assert tuple(out_size) == tuple(ref_size) == (To, Ho, Wo)
    check(got, ref, FWD_TOL, "pool3d_ln", f"D={D} stride={stride}")


@pytest.mark.parametrize("stride", ic.POOL_STRIDES, ids=pool_id)
@pytest.mark.parametrize("D", ic.POOL_DS, ids=pool_id)
def test_pool3d_ln(ops, D, stride):
    case_pool3d_ln(ops, D, stride)


def case_pool3d_backward(ops, D, stride, up=to_dev):
    qkv, w, _, _ = pool_inputs(D)
    B, heads, (T, H, W) = ic.POOL_B, ic.POOL_HEADS, ic.POOL_SIZE
    x = qkv[:, :, 1].double().requires_grad_(True)                       # [B, N, heads, D]
    wr = w.double().requires_grad_(True)
    vol = x[:, 1:].reshape(B, T, H, W, heads, D).permute(0, 4, 5, 1, 2, 3).reshape(B * heads, D, T, H, W)
    y = F.conv3d(vol, wr, stride=stride, padding=1, groups=D)
    out = torch.cat([x[:, :1].permute(0, 2, 1, 3), y.reshape(B, heads, D, -1).transpose(2, 3)], dim=2)      # [B, heads, 1 + Lo, D]
    dy = rnd(f"iPdy{D}", *out.shape)
    out.backward(dy.double())
    qd = up(qkv)
    dqkv = up(torch.full_like(qkv, float("nan")))
    poison((27 * D, torch.float32))
    dw = ops.pool3d_bwd(qd[:, :, 1], up(w.reshape(D, 27).t().contiguous()), up(dy), dqkv[:, :, 1], ic.POOL_SIZE, stride)
    assert torch.isnan(dqkv[:, :, 0]).all() and torch.isnan(dqkv[:, :, 2]).all(), "the neighbouring slices were written"
    case = f"D={D} stride={stride}"
    check(dqkv[:, :, 1], x.grad, POOL_BWD_TOL, "pool3d_bwd dx", case)
    check(dw, wr.grad.reshape(D, 27).t(), POOL_BWD_TOL, "pool3d_bwd dw", case)


@pytest.mark.parametrize("stride", ic.POOL_STRIDES, ids=pool_id)
@pytest.mark.parametrize("D", ic.POOL_DS, ids=pool_id)
def test_pool3d_backward(ops, D, stride):
    """dx (written through the strides of the q / k / v slice of the fused-qkv gradient) and the filter gradient against float64
    autograd of the depthwise conv3d with the class token passed through."""
    case_pool3d_backward(ops, D, stride)
