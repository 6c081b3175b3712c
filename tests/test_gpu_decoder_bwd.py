"""The decoder's small training kernels one by one (csrc/backward.hip, col2im of csrc/pack.hip, tapsum_bwd of csrc/tapsum.hip,
csrc/optim.hip) against the fp64 references of tests/_decoder_bwd_ref.py, called through ``ops`` (or the raw binding where ``ops``
cannot select a route) so that every operand can be chosen.

EXACT: integer operands (dyadic weights where the kernel forms them) -- no fp32 partial sum rounds, the assertion is bit-equality with
fp64.  BOUNDED: continuous operands, a per-element bound counted from the kernel's roundings or measured on the fp32 CPU (see the
reference module).  tests/test_decoder_bwd_host.py checks the 2^24 condition of every exact case, what the tables claim to contain,
and that each comparison here fails for a reference made wrong on purpose.  Every comparison yields the worst error / bound ratio it
saw (0 for an exact one); a test hands it to ``record`` (pytest does not let a test function return a value), which keeps the largest
per family and prints it: ``-s`` shows them."""
import numpy as np
import pytest
import torch

from tests import _decoder_bwd_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
WORST = {}


@pytest.fixture(scope="module")
def lib():
    from diff_sal_amd import _lib, autograd_ops, ops

    return ops, autograd_ops, _lib


def to_dev(t):
    """The upload of every case body here; tests/test_gpu_guard_bands.py passes tests/_guard.py's ``put`` in its place."""
    return t.to(DEV)


def dev32(t, up=to_dev):
    return up(t.float().contiguous())


def record(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"[worst error / bound] {family}: {ratio:.3g} (family so far {WORST[family]:.3g})")
    return ratio


# ---- bilinear resize adjoint -----------------------------------------------------------------------------------------------------------
def raw_resize_bwd(lib, dy, h, w, route):
    """diffsal_resize_bilinear_bwd through the binding: 'separable' with a workspace of exactly the size the entry asks for, 'joint4'
    with a null one, 'scalar' (where C % 4 == 0) with the gradient 4 bytes into its buffer."""
    ops, _, _lib = lib
    N, H, W, Cc = dy.shape
    dx = torch.full((N, h, w, Cc), NAN, device=DEV)
    ws, nbytes = None, 0
    if route == "separable":
        ws = torch.full((N * h * W * Cc,), NAN, device=DEV)
        nbytes = ws.numel() * 4
    if route == "scalar" and Cc % 4 == 0:
        buf = torch.empty(dy.numel() + 1, device=DEV)
        buf[1:] = dy.reshape(-1)
        dy = buf[1:].view(N, H, W, Cc)
        assert dy.data_ptr() % 16 == 4
    _lib.check(_lib.load().diffsal_resize_bilinear_bwd(dy.data_ptr(), dx.data_ptr(), N, h, w, H, W, Cc, ops._p(ws), nbytes, ops._stream()),
               "resize_bilinear_bwd")
    return dx


def case_resize_adjoint_is_exact_on_every_route(lib, case, up=to_dev):
    ops, ag, _ = lib
    (h, w), (H, W), Cc = case
    dy = R.resize_operands(case)
    ref = R.resize_bwd64(dy, h, w)
    dyd = dev32(dy, up)
    outs = {r: raw_resize_bwd(lib, dyd, h, w, r) for r in R.resize_routes(case)}
    for r, got in outs.items():
        R.check_exact(got, ref, f"route {r}")
    R.check_exact(ops.resize_bilinear_bwd(dyd, h, w), ref, "ops.resize_bilinear_bwd")
    first = next(iter(outs.values()))
    assert all(torch.equal(first, o) for o in outs.values())
    print("routes:", case, list(outs))
    record("resize (exact)", 0.0)


@pytest.mark.parametrize("case", R.RESIZE_EXACT, ids=R.case_id)
def test_resize_adjoint_is_exact_on_every_route(lib, case):
    case_resize_adjoint_is_exact_on_every_route(lib, case)


def case_resize_adjoint_at_other_ratios_within_the_counted_bound(lib, case, up=to_dev):
    ops, _, _ = lib
    (h, w), (H, W), Cc = case
    dy = R.resize_operands(case, exact=False)
    ref = R.resize_bwd64(dy, h, w)
    dyd = dev32(dy, up)
    worst = 0.0
    for r in R.resize_routes(case):
        worst = max(worst, R.check_bound(raw_resize_bwd(lib, dyd, h, w, r), ref, R.resize_bound(dy, case, r), f"route {r}"))
    worst = max(worst, R.check_bound(ops.resize_bilinear_bwd(dyd, h, w), ref, R.resize_bound(dy, case, "joint4"), "ops"))
    print("routes:", case, R.resize_routes(case))
    record("resize (bounded)", worst)


@pytest.mark.parametrize("case", R.RESIZE_BOUNDED, ids=R.case_id)
def test_resize_adjoint_at_other_ratios_within_the_counted_bound(lib, case):
    case_resize_adjoint_at_other_ratios_within_the_counted_bound(lib, case)


def test_resize_autograd_node_is_the_exact_adjoint(lib):
    _, ag, _ = lib
    case = R.RESIZE_EXACT[0]
    (h, w), (H, W), Cc = case
    dy = R.resize_operands(case)
    x = torch.zeros(2, h, w, Cc, device=DEV, requires_grad=True)
    ag.resize_bilinear(x, H, W).backward(dev32(dy))
    R.check_exact(x.grad, R.resize_bwd64(dy, h, w), "ResizeFn")


# ---- tapsum_bwd ------------------------------------------------------------------------------------------------------------------------
def case_tapsum_bwd_is_exact(lib, case, up=to_dev):
    ops, _, _ = lib
    (H, W), (h, w), Cc, dil = case
    du = R.tapsum_operands(case)
    R.check_exact(ops.tapsum_bwd(dev32(du, up), h, w, dil), R.tapsum_bwd64(du, h, w, dil), "tapsum_bwd")
    record("tapsum_bwd", 0.0)


@pytest.mark.parametrize("case", R.TAPSUM_CASES, ids=R.case_id)
def test_tapsum_bwd_is_exact(lib, case):
    case_tapsum_bwd_is_exact(lib, case)


def test_tapsum_bwd_writes_its_slice_of_a_larger_buffer_and_nothing_else(lib):
    ops, _, _ = lib
    case = R.TAPSUM_SLICE_CASE
    (H, W), (h, w), Cc, dil = case
    du = R.tapsum_operands(case)
    rows, before, after = 2 * h * w, 5, 7
    buf = torch.full((before + rows + after, 9 * Cc), -12345.0, device=DEV)
    # 5 rows of 9 C floats in front: a multiple of 16 bytes for C = 4 (36 floats a row)
    out = ops.tapsum_bwd(dev32(du), h, w, dil, out=buf[before:before + rows].view(2, h, w, 9 * Cc))
    assert out.data_ptr() == buf[before].data_ptr()
    R.check_exact(buf[before:before + rows].view(2, h, w, 9 * Cc), R.tapsum_bwd64(du, h, w, dil), "slice")
    assert bool((buf[:before] == -12345.0).all()) and bool((buf[before + rows:] == -12345.0).all())


def test_tapsum_autograd_node_fills_every_source_block(lib):
    """TapSumFn with two sources: d(y_all) holds each source's adjoint in its block of rows."""
    _, ag, _ = lib
    N, (H, W), Cc, dil, shapes = 2, (8, 12), 4, 1, [(4, 6), (2, 3)]
    du = R.ints(R.generator(77), (N, H, W, Cc))
    rows = sum(N * h * w for h, w in shapes)
    y_all = torch.zeros(rows, 9 * Cc, device=DEV, requires_grad=True)
    ag.tapsum(y_all, shapes, N, H, W, Cc, dil=dil).backward(dev32(du))
    ref = torch.cat([R.tapsum_bwd64(du, h, w, dil).reshape(-1, 9 * Cc) for h, w in shapes], 0)
    R.check_exact(y_all.grad, ref, "TapSumFn")


# ---- col2im ----------------------------------------------------------------------------------------------------------------------------
def case_col2im_is_exact(lib, kind, case, up=to_dev):
    ops, _, _ = lib
    kh, kw, stride, pad, extra, H, W, Cc = case
    cols = R.col2im_operands(case)
    ref = R.col2im64(cols, case)
    fn = ops.col2im_disjoint if kind == "disjoint" else ops.col2im_gather
    got = fn(dev32(cols, up), (2, H, W, Cc), R.col2im_out_hw(case), kh, kw, stride, pad)
    R.check_exact(got, ref, "col2im_" + kind)
    if kind == "disjoint":                                                   # the gather kernel handles disjoint taps too
        R.check_exact(ops.col2im_gather(dev32(cols, up), (2, H, W, Cc), R.col2im_out_hw(case), kh, kw, stride, pad), ref, "gather on disjoint taps")
    record("col2im", 0.0)


@pytest.mark.parametrize("kind,case", [("disjoint", c) for c in R.COL2IM_DISJOINT] + [("gather", c) for c in R.COL2IM_GATHER],
                         ids=lambda v: v if isinstance(v, str) else R.case_id(v))
def test_col2im_is_exact(lib, kind, case):
    case_col2im_is_exact(lib, kind, case)


@pytest.mark.parametrize("kind", ["gather", "disjoint"])
def test_strided_convolution_node_reaches_col2im_and_stays_exact(lib, kind):
    """ConvFn's data gradient of a strided convolution = one product dY W and col2im: the asymmetric-pad 3 x 3 stride-2 Downsample (gather)
    and ReduceTemp's 5 x 1 stride-5 form (disjoint), integer operands, against fp64 autograd of F.conv2d."""
    import torch.nn.functional as F

    ops, ag, _ = lib
    g = R.generator(31)
    Cc = 32
    if kind == "gather":
        N, H, W, kh, kw, stride, asym = 2, 6, 8, 3, 3, (2, 2), (0, 1, 0, 1)
    else:
        N, H, W, kh, kw, stride, asym = 2, 9, 7, 5, 1, (5, 1), (0, 0, 0, 0)
    x = R.ints(g, (N, Cc, H, W), 2).requires_grad_(True)
    w = R.ints(g, (Cc, Cc, kh, kw), 2).requires_grad_(True)
    y = F.conv2d(F.pad(x, asym), w, stride=stride)
    gy = R.ints(g, tuple(y.shape), 2)
    y.backward(gy)
    assert Cc * kh * kw * 4 < R.LIMIT and N * y.shape[2] * y.shape[3] * 4 < R.LIMIT
    xd = dev32(x.detach().permute(0, 2, 3, 1)).requires_grad_(True)
    wd = dev32(w.detach()).requires_grad_(True)
    yd = ag.conv(xd, ops.pack_conv_weight_diff(wd), kh=kh, kw=kw, stride=stride, pad=(0, 0), out_hw=tuple(y.shape[-2:]),
                 w_dgrad=ag.dgrad_weight(wd, stride))
    R.check_exact(yd, y.detach().permute(0, 2, 3, 1), "forward")
    yd.backward(dev32(gy.permute(0, 2, 3, 1)))
    R.check_exact(xd.grad, x.grad.permute(0, 2, 3, 1), "dx through col2im_" + kind)
    R.check_exact(wd.grad, w.grad, "dw")


# ---- depthwise convolution -------------------------------------------------------------------------------------------------------------
def case_dwconv_forward_and_both_gradients_are_exact(lib, case, up=to_dev):
    ops, ag, _ = lib
    Cc, H, W, k, stride, pad = case
    x, w, du = R.dwconv_operands(case)
    out, dx, dw = R.dwconv64(x, w, du, case)
    xd, wd, dud = dev32(x, up), dev32(w, up), dev32(du, up)
    R.check_exact(ops.dwconv(xd, wd, k, stride, pad), out, "dwconv")
    gdx, gdw = ops.dwconv_bwd(xd, wd, dud, k, stride, pad)
    R.check_exact(gdx, dx, "dwconv_bwd_data")
    R.check_exact(gdw, dw, "dwconv_bwd_weight")
    if case == R.DWCONV_CASES[2]:                                            # the autograd node, once
        xl, wl = xd.clone().requires_grad_(True), wd.clone().requires_grad_(True)
        ag.dwconv(xl, wl, k, stride, pad).backward(dud)
        R.check_exact(xl.grad, dx, "DwConvFn dx")
        R.check_exact(wl.grad, dw, "DwConvFn dw")
    record("dwconv", 0.0)


@pytest.mark.parametrize("case", R.DWCONV_CASES, ids=R.case_id)
def test_dwconv_forward_and_both_gradients_are_exact(lib, case):
    case_dwconv_forward_and_both_gradients_are_exact(lib, case)


# ---- head ------------------------------------------------------------------------------------------------------------------------------
def case_head_bwd_is_exact(lib, case, up=to_dev):
    ops, _, _ = lib
    y, w, s, ds = R.head_operands(case)
    dy, dw, db = ops.head_bwd(dev32(y, up), dev32(w, up), dev32(s, up), dev32(ds, up))
    for n, a, b in zip(("dy", "dw", "db"), (dy, dw, db), R.head_bwd64(y, w, s, ds)):
        R.check_exact(a, b, n)
    record("head_bwd", 0.0)


@pytest.mark.parametrize("case", R.HEAD_CASES, ids=R.case_id)
def test_head_bwd_is_exact(lib, case):
    case_head_bwd_is_exact(lib, case)


@pytest.mark.parametrize("case", R.HEAD_E2E_CASES, ids=R.case_id)
def test_head_sigmoid_end_to_end_within_the_measured_bound(lib, case):
    _, ag, _ = lib
    y, w, b, ds = R.head_e2e_operands(case)
    M, Cc = case
    yl, wl, bl = (dev32(t).requires_grad_(True) for t in (y.reshape(1, 1, M, Cc), w, b))
    s = ag.head_sigmoid(yl, wl, bl)
    s.backward(dev32(ds).reshape(s.shape))
    got = dict(s=s.detach().reshape(M), dy=yl.grad.reshape(M, Cc), dw=wl.grad, db=bl.grad)
    worst = max(R.check_bound(got[n], ref, tol, n) for n, tol, ref in R.measured_tols("head", case))
    record("head_sigmoid", worst)


# ---- conv_in ---------------------------------------------------------------------------------------------------------------------------
def case_conv_in_bwd_is_exact(lib, case, up=to_dev):
    ops, ag, _ = lib
    x, dy = R.conv_in_operands(case)
    dw, db = R.conv_in_bwd64(x, dy)
    gdw, gdb = ops.conv_in_bwd(dev32(x, up), dev32(dy, up))
    R.check_exact(gdw, dw, "dw")
    R.check_exact(gdb, db, "db")
    if case == R.CONV_IN_CASES[2]:                                           # the autograd node, once
        Cc = case[3]
        wl, bl = torch.zeros(Cc, 9, device=DEV, requires_grad=True), torch.zeros(Cc, device=DEV, requires_grad=True)
        ag.conv_in(dev32(x, up), wl, bl, 0).backward(dev32(dy, up))
        R.check_exact(wl.grad, dw, "ConvInFn dw")
        R.check_exact(bl.grad, db, "ConvInFn db")
    record("conv_in_bwd", 0.0)


@pytest.mark.parametrize("case", R.CONV_IN_CASES, ids=R.case_id)
def test_conv_in_bwd_is_exact(lib, case):
    case_conv_in_bwd_is_exact(lib, case)


# ---- dense_small -----------------------------------------------------------------------------------------------------------------------
def case_dense_small_bwd_without_swish_is_exact(lib, case, up=to_dev):
    ops, ag, _ = lib
    x, w, dout = R.dense_operands(case, False)
    refs = R.dense_bwd(x, w, dout, False)
    for n, a, b in zip(("dx", "dw", "db"), ops.dense_small_bwd(dev32(x, up), dev32(w, up), dev32(dout, up), False), refs):
        R.check_exact(a, b, n)
    if case == R.DENSE_CASES[5]:                                             # the autograd node, once (the time embedding's shape)
        xl, wl, bl = dev32(x, up).requires_grad_(True), dev32(w, up).requires_grad_(True), torch.zeros(case[2], device=DEV, requires_grad=True)
        ag.dense_small(xl, wl, bl, False).backward(dev32(dout, up))
        for n, a, b in zip(("dx", "dw", "db"), (xl.grad, wl.grad, bl.grad), refs):
            R.check_exact(a, b, n + " (DenseSmallFn)")
    record("dense_small_bwd (exact)", 0.0)


@pytest.mark.parametrize("case", R.DENSE_CASES, ids=R.case_id)
def test_dense_small_bwd_without_swish_is_exact(lib, case):
    case_dense_small_bwd_without_swish_is_exact(lib, case)


def case_dense_small_bwd_with_swish_within_the_measured_bound(lib, case, up=to_dev):
    ops, _, _ = lib
    x, w, dout = R.dense_operands(case, True)
    got = dict(zip(("dx", "dw", "db"), ops.dense_small_bwd(dev32(x, up), dev32(w, up), dev32(dout, up), True)))
    tols = {n: (tol, ref) for n, tol, ref in R.measured_tols("dense", case)}
    worst = max(R.check_bound(got[n], tols[n][1], tols[n][0], n) for n in ("dx", "dw"))
    db_tol = max(case[0] - 1, 0) * R.U * R.dense_mag(x, w, dout, True)[2]                       # COUNTED: no swish on its path, B - 1 additions
    worst = max(worst, R.check_bound(got["db"], tols["db"][1], db_tol, "db"))
    record("dense_small_bwd (swish)", worst)


@pytest.mark.parametrize("case", R.DENSE_CASES, ids=R.case_id)
def test_dense_small_bwd_with_swish_within_the_measured_bound(lib, case):
    case_dense_small_bwd_with_swish_within_the_measured_bound(lib, case)


# ---- audio_fuse ------------------------------------------------------------------------------------------------------------------------
def case_audio_fuse_and_its_backward_within_the_measured_bound(lib, case, up=to_dev):
    ops, ag, _ = lib
    B, T, Cc, h, w, _ = case
    a, x, dout = R.audio_operands(case)
    ad, xd, gd = dev32(a, up), dev32(x, up), dev32(dout, up)
    out = ops.audio_fuse(ad, xd, h, w)
    dx, da = ops.audio_fuse_bwd(ad, xd, gd, h, w)
    got = dict(out=out, dx=dx, da=da)
    worst = max(R.check_bound(got[n], ref, tol, n) for n, tol, ref in R.measured_tols("audio", case))
    if case == R.AUDIO_CASES[3]:                                             # the autograd node, once: the same kernels, the same bits
        al, xl = ad.clone().requires_grad_(True), xd.clone().requires_grad_(True)
        o2 = ag.audio_fuse(al, xl, h, w)
        o2.backward(gd)
        assert torch.equal(o2.detach(), out) and torch.equal(xl.grad, dx) and torch.equal(al.grad, da)
    record("audio_fuse", worst)


@pytest.mark.parametrize("case", R.AUDIO_CASES, ids=R.case_id)
def test_audio_fuse_and_its_backward_within_the_measured_bound(lib, case):
    case_audio_fuse_and_its_backward_within_the_measured_bound(lib, case)


def test_audio_fuse_bwd_refuses_an_up_factor_above_eight(lib):
    """The forward accepts any integer factor; the backward holds at most 8 columns per cell in registers: it returns the shape error and
    writes nothing."""
    ops, _, _lib = lib
    B, T, Cc, h, w, up = R.AUDIO_REFUSED
    a, x, dout = (dev32(t) for t in R.audio_operands(R.AUDIO_REFUSED))
    out = ops.audio_fuse(a, x, h, w)
    assert tuple(out.shape) == (B, Cc, T, h * up, w * up) and bool(torch.isfinite(out).all())
    dx = torch.full_like(x, -12345.0)
    part = torch.full((B * T * h * w * up, Cc), -12345.0, device=DEV)
    rc = _lib.load().diffsal_audio_fuse_bwd(a.data_ptr(), x.data_ptr(), dout.data_ptr(), dx.data_ptr(), part.data_ptr(), B, T, h * up, w * up,
                                            Cc, h, w, ops._stream())
    assert rc == -1 and b"up-factor" in _lib.load().diffsal_last_error()     # DIFFSAL_E_SHAPE
    torch.cuda.synchronize()
    assert bool((dx == -12345.0).all()) and bool((part == -12345.0).all())
    with pytest.raises(RuntimeError, match="up-factor"):
        ops.audio_fuse_bwd(a, x, dout, h, w)


# ---- unpack_frames ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.UNPACK_CASES, ids=R.case_id)
def test_unpack_frames_is_the_permutation(lib, case):
    ops, _, _ = lib
    B, Cc, Tv, Tin, hw = case
    frames = R.nz_ints(R.generator(sum(case)), (B, Tin, hw, Cc))
    got = ops.unpack_frames(dev32(frames).view(B, Tin, hw, 1, Cc), Tv)
    R.check_exact(got.reshape(B, Cc, Tv, hw), R.unpack_frames_ref(frames, Tv), "unpack_frames")


# ---- dropout ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.DROPOUT_NS)
@pytest.mark.parametrize("p", R.DROPOUT_PS)
def test_dropout_mask_is_the_hash_and_its_own_backward(lib, n, p):
    ops, ag, _ = lib
    x = torch.randn(n, generator=R.generator(n)) + 3.0                        # no zeros: the mask is where the output is zero
    assert bool((x != 0).all())
    outs = []
    for seed in R.DROPOUT_SEEDS:
        got = ops.dropout(dev32(x), p, seed)
        ref = R.dropout_ref(x, p, seed)
        assert torch.equal(got.cpu(), ref), f"seed {seed:#x}: {int((got.cpu() != ref).sum())} of {n} elements differ"
        assert torch.equal((got != 0).cpu(), R.dropout_keep(n, p, seed))
        outs.append(got)
        xl = dev32(x).requires_grad_(True)
        y = ag.dropout(xl, p, seed=seed)
        g = torch.randn(n, generator=R.generator(n + 1)) + 3.0
        y.backward(dev32(g))
        assert torch.equal(y.detach(), got) and torch.equal(xl.grad.cpu(), R.dropout_ref(g, p, seed))
    if p > 0 and n >= 1000:
        assert not torch.equal(outs[0], outs[1])                             # the high word of the seed matters


# ---- mse_loss --------------------------------------------------------------------------------------------------------------------------
def case_mse_loss_value_within_the_counted_bound_and_gradient_exact(lib, n, want_grad, up=to_dev):
    ops, _, _ = lib
    pred, tgt = R.mse_operands(n)
    scale = 0.7 / 3
    loss64, dp32, mag = R.mse64(pred, tgt, scale)
    loss, dpred = ops.mse_loss(dev32(pred, up), dev32(tgt, up), scale, want_grad=want_grad)
    worst = R.check_bound(loss.reshape(()), loss64, R.MSE_K * R.U * mag, "loss")
    if want_grad:
        assert torch.equal(dpred.cpu(), dp32), f"{int((dpred.cpu() != dp32).sum())} of {n} gradient elements differ"
    else:
        assert dpred is None
    record("mse_loss", worst)


@pytest.mark.parametrize("n", R.MSE_NS)
@pytest.mark.parametrize("want_grad", [True, False])
def test_mse_loss_value_within_the_counted_bound_and_gradient_exact(lib, n, want_grad):
    case_mse_loss_value_within_the_counted_bound_and_gradient_exact(lib, n, want_grad)


def test_mse_loss_node_runs_a_map_whose_size_is_no_multiple_of_four(lib):
    _, ag, _ = lib
    pred, tgt = (t.reshape(3, 1, 7, 9) for t in R.mse_operands(3 * 7 * 9))
    scale = 0.7 / 3
    loss64, dp32, mag = R.mse64(pred.reshape(-1), tgt.reshape(-1), scale)
    q = dev32(pred).requires_grad_(True)
    loss = ag.mse_loss(q, dev32(tgt), scale)
    (2.0 * loss).backward()
    assert loss.shape == ()
    R.check_bound(loss, loss64, R.MSE_K * R.U * mag, "MseLossFn")
    assert torch.equal(q.grad.cpu().reshape(-1), dp32 * 2.0)                # scale_by: an exact doubling


# ---- grad_norm -------------------------------------------------------------------------------------------------------------------------
def case_grad_norm_within_one_rounding(lib, n, spread, up=to_dev):
    ops, _, _ = lib
    g = R.norm_operands(n, spread)
    for gscale in (1.0, 0.25):
        ref = gscale * g.double().norm()
        worst = R.check_bound(ops.grad_norm(dev32(g, up), gscale).reshape(()), ref, R.NORM_REL * ref, f"gscale {gscale}")
    record("grad_norm", worst)


@pytest.mark.parametrize("n", R.NORM_NS)
@pytest.mark.parametrize("spread", [False, True])
def test_grad_norm_within_one_rounding(lib, n, spread):
    case_grad_norm_within_one_rounding(lib, n, spread)


# ---- adam_step -------------------------------------------------------------------------------------------------------------------------
def run_adam(ops, n, cfg, denom_eps=False, seed=0):
    """One kernel step from a given fp32 state against adam_step64 from the same state -> worst ratio."""
    wd, step, norm_kind, store, gscale = cfg
    hp = R.ADAM_HP
    p, g, m, v = R.adam_operands(n, seed, denom_eps)
    gnorm = float((gscale * g.double().norm()))
    # a norm below / above max_norm: the kernel only reads the device scalar, so the test chooses it
    norm = None if norm_kind == "absent" else np.float32(0.5 * hp["max_norm"] if norm_kind == "below" else 3.0 * hp["max_norm"] + gnorm)
    coef = R.adam_coef(gscale, norm, hp["max_norm"])
    ref = R.adam_step64(p, g, m, v, step=step, wd=wd, coef=coef, lr=hp["lr"], beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"])
    pd, gd, md, vd = dev32(p), dev32(g), dev32(m), dev32(v)
    nd = None if norm is None else torch.tensor([float(norm)], device=DEV)
    ops.adam_step(pd, gd, md, vd, step=step, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=wd, gscale=gscale,
                  norm=nd, max_norm=hp["max_norm"], store_clipped_grad=bool(store))
    what = f"n={n} {cfg}"
    worst = R.check_bound(md, ref["m"], ref["tol_m"], "m " + what)
    worst = max(worst, R.check_bound(vd, ref["v"], ref["tol_v"], "v " + what))
    worst = max(worst, R.check_bound(pd.cpu().double() - p.double(), ref["step"], ref["tol_step"], "step " + what))
    assert torch.equal(gd.cpu(), ref["g"] if store else g), "gradient buffer " + what      # written back only when asked
    return worst


@pytest.mark.parametrize("n", R.ADAM_SMALL)
def test_adam_step_every_switch_combination_at_the_small_sizes(lib, n):
    ops, _, _ = lib
    worst = max(run_adam(ops, n, cfg, seed=i) for i, cfg in enumerate(R.ADAM_GRID))
    record("adam_step", worst)


@pytest.mark.parametrize("n", [n for n in R.ADAM_NS if n not in R.ADAM_SMALL])
@pytest.mark.parametrize("cfg", R.ADAM_LARGE, ids=R.case_id)
def test_adam_step_at_the_large_sizes(lib, n, cfg):
    ops, _, _ = lib
    record("adam_step", run_adam(ops, n, cfg))


@pytest.mark.parametrize("n", [3, 70003])
def test_adam_step_with_a_denominator_of_eps_alone(lib, n):
    ops, _, _ = lib
    record("adam_step", max(run_adam(ops, n, cfg, denom_eps=True) for cfg in R.ADAM_LARGE))
