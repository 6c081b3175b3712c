"""tests/_decoder_bwd_ref.py without a GPU: every reference is tied to torch, every exact case keeps its partial sums below 2^24, the case
tables contain the launch boundaries they claim, the measured bounds are what the fp32 CPU gives, and every comparison of
tests/test_gpu_decoder_bwd.py has power: a reference made wrong the way a kernel could be wrong fails the same check on the same operands.
(A mutation that changes nothing for a case -- a stride-1 walk that starts at tap 0 anyway, weight decay 0 -- is checked on the cases
it does change; each block asserts that there are such cases.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _decoder_bwd_ref as R


def fails(check, *a, **k):
    try:
        check(*a, **k)
    except AssertionError:
        return True
    return False


def f32(t):
    """What the kernel would hand back for an exact case: the fp64 value in fp32."""
    return t.float()


# ---- bilinear adjoint ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.RESIZE_EXACT + R.RESIZE_BOUNDED, ids=R.case_id)
def test_bilinear_matrix_is_torchs_interpolation(case):
    (h, w), (H, W), C = case
    exact = case in R.RESIZE_EXACT
    x = R.ints(R.generator(5), (2, h, w, C))
    ref = F.interpolate(x.float().permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    got = R.resize_fwd64(x, H, W)
    if exact:
        R.check_exact(ref, got, "forward")                                   # bit for bit: integer inputs, dyadic weights
    else:
        assert float((got - ref.double()).abs().max()) <= 2e-6 * 4
    # and the adjoint really is the adjoint: <A x, g> = <x, A^T g>
    g = R.resize_operands(case)
    assert float(((got * g).sum() - (x * R.resize_bwd64(g, h, w)).sum()).abs()) < 1e-9


@pytest.mark.parametrize("case", R.RESIZE_EXACT, ids=R.case_id)
def test_resize_exact_cases_do_not_round(case):
    (h, w), (H, W), C = case
    assert R.resize_partial_max(case) < R.LIMIT
    assert float(R.bilin_slack(H, h).abs().max()) == 0.0 and float(R.bilin_slack(W, w).abs().max()) == 0.0
    ref = R.resize_bwd64(R.resize_operands(case), h, w)
    assert torch.equal(ref.float().double(), ref)


def test_resize_tables_contain_what_they_claim():
    ex, bd = R.RESIZE_EXACT, R.RESIZE_BOUNDED
    assert any((h, w) == (H, W) for (h, w), (H, W), C in ex)                                  # identity
    assert any(h != H and w == W for (h, w), (H, W), C in ex)                                  # one equal axis
    assert any(h > H and w > W for (h, w), (H, W), C in ex + bd)                               # downscale
    assert any(C % 4 and C > 1 for _, _, C in ex) and any(C == 1 for _, _, C in ex + bd)
    assert all(H % h and W % w or (h % H and w % W) for (h, w), (H, W), C in bd if (h, w) != (1, 1))   # no integer ratio
    routes = {r for c in ex + bd for r in R.resize_routes(c)}
    assert routes == {"separable", "joint4", "scalar"}
    assert all(float(R.bilin_slack(H, h).max()) > 0 or float(R.bilin_slack(W, w).max()) > 0 for (h, w), (H, W), C in bd if (h, w) != (1, 1))


@pytest.mark.parametrize("case", R.RESIZE_EXACT + R.RESIZE_BOUNDED, ids=R.case_id)
def test_resize_comparison_has_power(case):
    (h, w), (H, W), C = case
    exact = case in R.RESIZE_EXACT
    dy = R.resize_operands(case, exact=exact)
    ref = R.resize_bwd64(dy, h, w)
    tol = None if exact else max((R.resize_bound(dy, case, r) for r in R.resize_routes(case)), key=lambda t: float(t.sum()))
    check = (lambda got: R.check_exact(f32(got), ref)) if exact else (lambda got: R.check_bound(got, ref, tol))
    assert not fails(check, ref)
    assert fails(check, R.resize_bwd64(dy, h, w, "short"))                  # the window one output short: every case
    if H > h or W > w:                                                       # an upscaled axis has clamped edge outputs
        assert fails(check, R.resize_bwd64(dy, h, w, "edge"))


# ---- tapsum_bwd ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in R.TAPSUM_CASES if c[2] == 4], ids=R.case_id)
def test_tapsum_bwd_reference_is_the_adjoint_of_the_convolution_of_the_upsampled_map(case):
    (H, W), (h, w), C, dil = case
    g = R.generator(9)
    Cin = 3
    z = R.ints(g, (2, Cin, h, w)).requires_grad_(True)
    wt = R.ints(g, (C, Cin, 3, 3))
    du = R.tapsum_operands(case)
    up = z if (h, w) == (H, W) else F.interpolate(z, size=(H, W), mode="bilinear", align_corners=False)
    (F.conv2d(up, wt, padding=dil, dilation=dil) * du.permute(0, 3, 1, 2)).sum().backward()
    dY = R.tapsum_bwd64(du, h, w, dil).reshape(2, h, w, 9, C)
    dz = torch.einsum("nijtc,tcd->ndij", dY, wt.permute(2, 3, 0, 1).reshape(9, C, Cin))
    assert float((dz - z.grad).abs().max()) < 1e-9
    wrong = R.tapsum_bwd64(du, h, w, dil, flip=True).reshape(2, h, w, 9, C)
    assert float((torch.einsum("nijtc,tcd->ndij", wrong, wt.permute(2, 3, 0, 1).reshape(9, C, Cin)) - z.grad).abs().max()) > 0.5


@pytest.mark.parametrize("case", R.TAPSUM_CASES, ids=R.case_id)
def test_tapsum_cases_do_not_round_and_the_comparison_has_power(case):
    (H, W), (h, w), C, dil = case
    assert R.resize_partial_max(((h, w), (H, W), C)) < R.LIMIT
    du = R.tapsum_operands(case)
    ref = R.tapsum_bwd64(du, h, w, dil)
    assert torch.equal(ref.float().double(), ref)
    assert fails(R.check_exact, f32(R.tapsum_bwd64(du, h, w, dil, flip=True)), ref)


def test_tapsum_table_contains_what_it_claims():
    fs = {H // h for (H, W), (h, w), C, dil in R.TAPSUM_CASES}
    assert fs == {1, 2, 4, 8} and any((h, w) == (2, 2) for _, (h, w), _, _ in R.TAPSUM_CASES)
    assert {c[2] for c in R.TAPSUM_CASES} == {4, 12} and {c[3] for c in R.TAPSUM_CASES} == {1, 2}
    assert R.TAPSUM_SLICE_CASE in R.TAPSUM_CASES


# ---- col2im ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.COL2IM_DISJOINT + R.COL2IM_GATHER, ids=R.case_id)
def test_col2im_reference_is_the_adjoint_of_unfold_and_has_power(case):
    kh, kw, stride, pad, extra, H, W, C = case
    Ho, Wo = R.col2im_out_hw(case)
    cols = R.col2im_operands(case)
    ref = R.col2im64(cols, case)
    # adjoint of im2col on the padded image: d/dx of <unfold(pad(x)), cols>
    x = torch.zeros(2, C, H, W, dtype=torch.float64, requires_grad=True)
    xp = F.pad(x, (pad[1], pad[1] + extra[1], pad[0], pad[0] + extra[0]))
    u = F.unfold(xp, (kh, kw), stride=stride)                                # [N, C kh kw, L]
    assert u.shape[-1] == Ho * Wo
    c = cols.reshape(2, Ho * Wo, kh, kw, C).permute(0, 4, 2, 3, 1).reshape(2, C * kh * kw, Ho * Wo)
    (u * c).sum().backward()
    assert torch.equal(x.grad.permute(0, 2, 3, 1), ref)
    assert kh * kw * 4 < R.LIMIT and torch.equal(ref.float().double(), ref)
    assert fails(R.check_exact, f32(R.col2im64(cols, case, wrong=True)), ref)


def test_col2im_tables_contain_what_they_claim():
    for kh, kw, stride, pad, extra, H, W, C in R.COL2IM_DISJOINT:
        assert stride[0] >= kh and stride[1] >= kw
    assert any(stride[0] > kh for kh, kw, stride, *_ in R.COL2IM_DISJOINT)
    assert all(stride[0] < kh for kh, kw, stride, *_ in R.COL2IM_GATHER)
    # rows no window covers: the reference leaves them zero
    c = R.COL2IM_DISJOINT[0]
    assert float(R.col2im64(R.col2im_operands(c), c)[:, 5:].abs().max()) == 0.0
    c = R.COL2IM_DISJOINT[2]
    z = R.col2im64(R.col2im_operands(c), c)
    assert float(z[:, -1].abs().max()) == 0.0 and float(z[:, :, -1].abs().max()) == 0.0
    # the asymmetric-pad Downsample: an output row more than the unpadded image gives
    asym = [c for c in R.COL2IM_GATHER if c[4] != (0, 0)]
    assert asym and all(R.col2im_out_hw(c)[0] == (c[5] - c[0]) // c[2][0] + 2 for c in asym)


# ---- depthwise convolution -------------------------------------------------------------------------------------------------------------
def test_dwconv_table_contains_what_it_claims():
    from diff_sal_amd import _lib

    lib = _lib.load()
    info = []
    for C, H, W, k, stride, pad in R.DWCONV_CASES:
        chunks, P = R.dw_chunks(2, H, W, k, stride, pad)
        assert chunks == lib.diffsal_dwconv_bwd_weight_chunks(2, H, W, k, stride, pad)
        assert max(k * k, P) * 16 < R.LIMIT                                  # operands in [-4, 4]: every partial sum exact
        info.append((C // 4, chunks, P, k, stride, H + 2 * pad))
    c4ns = {i[0] for i in info}
    assert {129, 256} <= c4ns and any(256 % c for c in c4ns)                 # a c4n that does not divide 256; idle lanes; none idle
    assert any(chunks > 1 and P % chunks for _, chunks, P, *_ in info)       # a partition with uneven chunks
    assert any(chunks == 1 for _, chunks, *_ in info)
    assert any(1 < s < k for *_, k, s, _ in info) and any(s > k for *_, k, s, _ in info) and any(s == 1 for *_, k, s, _ in info)
    assert any((Hp - k) % s for *_, k, s, Hp in info)                        # trailing rows no window covers


@pytest.mark.parametrize("case", [c for c in R.DWCONV_CASES if c[0] <= 96], ids=R.case_id)
def test_dwconv_walk_is_the_autograd_gradient_and_both_comparisons_have_power(case):
    C, H, W, k, stride, pad = case
    x, w, du = R.dwconv_operands(case)
    out, dx, dw = R.dwconv64(x, w, du, case)
    assert torch.equal(R.dwconv_bwd_data_walk(du, w, case), dx)
    if stride > 1:
        assert fails(R.check_exact, f32(R.dwconv_bwd_data_walk(du, w, case, start0=True)), dx)
    chunks, P = R.dw_chunks(2, H, W, k, stride, pad)
    for chunk in {0, chunks - 1}:
        assert fails(R.check_exact, f32(R.dwconv_dw_missing_pixel(x, du, case, chunk)), dw)


def test_dwconv_walk_mutation_applies_somewhere():
    assert sum(1 for c in R.DWCONV_CASES if c[4] > 1 and c[0] <= 96) >= 3


# ---- head ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.HEAD_CASES, ids=R.case_id)
def test_head_bwd_reference_is_autograd_exact_and_has_power(case):
    M, C = case
    y, w, s, ds = R.head_operands(case)
    dy, dw, db = R.head_bwd64(y, w, s, ds)
    # autograd of sigmoid(pre) at the pre whose sigmoid is s: d/dy, d/dw, d/db of sum(ds * sigmoid(y w + b)) with s given
    yl, wl = y.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (ds * s * (1 - s) * (yl @ wl)).sum().backward()                          # linearised at s: the same chain rule
    assert torch.equal(yl.grad, dy) and torch.equal(wl.grad, dw)
    assert float(db - (ds * s * (1 - s)).sum()) == 0.0
    assert M * 1 * 4 * 16 < R.LIMIT                                          # |dp| <= 4 / 4 = 1, |y| <= 4, in sixteenths
    for t in (dy, dw, db):
        assert torch.equal(t.float().double(), t)
    assert bool((((ds * s * (1 - s)) * 16) % 1 == 0).all())
    assert fails(R.check_exact, f32(R.head_bwd64(y, w, s, ds, drop_row=M - 1)[2]), db)
    assert fails(R.check_exact, f32(R.head_bwd64(y, w, s, ds, drop_row=0)[2]), db)


def test_head_table_contains_what_it_claims():
    Ms = [m for m, _ in R.HEAD_CASES]
    assert any(m < 64 for m in Ms) and 65 in Ms and any(m // 64 > 1024 for m in Ms)
    c4 = {c // 4 for _, c in R.HEAD_CASES}
    assert {129, 256, 10, 1} <= c4


# ---- conv_in ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CONV_IN_CASES, ids=R.case_id)
def test_conv_in_exactness_and_power(case):
    B, H, W, C = case
    x, dy = R.conv_in_operands(case)
    dw, db = R.conv_in_bwd64(x, dy)
    assert B * H * W * 16 < R.LIMIT
    assert fails(R.check_exact, f32(R.conv_in_bwd64(x, dy, wrap=True)[0]), dw)
    assert torch.equal(R.conv_in_bwd64(x, dy, wrap=True)[1], db)


def test_conv_in_table_contains_what_it_claims():
    P = [b * h * w for b, h, w, _ in R.CONV_IN_CASES]
    assert any(p < R.CONV_IN_CHUNKS for p in P) and any(p > R.CONV_IN_CHUNKS and p % R.CONV_IN_CHUNKS for p in P)
    assert (1, 1, 1, 8) in R.CONV_IN_CASES and {10, 256} <= {c // 4 for *_, c in R.CONV_IN_CASES}
    import re, os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diff_sal_amd", "ops.py")).read()
    assert re.search(r"def conv_in_bwd.*?chunks = %d\b" % R.CONV_IN_CHUNKS, src, re.S)


# ---- dense_small -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.DENSE_CASES, ids=R.case_id)
def test_dense_small_exactness_and_power(case):
    B, K, N = case
    x, w, dout = R.dense_operands(case, False)
    dx, dw, db = R.dense_bwd(x, w, dout, False)
    assert max(N, B) * 16 < R.LIMIT
    assert torch.equal(dx, dout @ w) and torch.equal(dw, dout.t() @ x) and torch.equal(db, dout.sum(0))
    tail = 32 * (N // 32)
    if N % 32:
        assert fails(R.check_exact, f32(R.dense_bwd(x, w, dout, False, tail_from=tail)[0]), dx)
        xs, ws, ds = R.dense_operands(case, True)
        ref, mag, rho = R.dense_bwd(xs.double(), ws.double(), ds.double(), True), R.dense_mag(xs, ws, ds, True), R.MEASURED_RHO[("dense", case)]
        wrong = R.dense_bwd(xs.double(), ws.double(), ds.double(), True, tail_from=tail)[0]
        assert fails(R.check_bound, wrong, ref[0], rho["dx"] * R.U * mag[0])


def test_dense_table_contains_what_it_claims():
    assert any(n % 32 for _, _, n in R.DENSE_CASES) and any(k % 32 for _, k, _ in R.DENSE_CASES)
    assert any(n % 32 == 0 for _, _, n in R.DENSE_CASES) and any(k % 32 == 0 for _, k, _ in R.DENSE_CASES)
    assert any(n < 8 for _, _, n in R.DENSE_CASES) and any(24 < n % 32 for _, _, n in R.DENSE_CASES)      # tail only; a tail of four steps
    x, _, _ = R.dense_operands(R.DENSE_CASES[-1], True)
    assert float(x.min()) < -7.5 and float(x.max()) > 7.5


# ---- audio_fuse ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.AUDIO_CASES, ids=R.case_id)
def test_audio_fuse_reference_and_power(case):
    B, T, C, h, w, up = case
    a, x, dout = (t.double() for t in R.audio_operands(case))
    out, dx, da = R.audio_fuse(a, x, dout, case)
    # the expression of tests/test_gpu_train_ops.py::test_audio_fuse_backward
    al, x5 = a.clone().requires_grad_(True), x.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    av = al.reshape(B, T, h, w, C).permute(0, 4, 1, 2, 3)
    if up > 1:
        av = F.interpolate(av.reshape(B, C * T, h, w), scale_factor=up, mode="nearest").reshape(B, C, T, h * up, w * up)
    o2 = av * F.softmax((av * x5).mean(dim=2, keepdim=True), dim=-1)
    o2.backward(dout)
    assert torch.allclose(o2, out, rtol=0, atol=1e-14) and torch.allclose(x5.grad.permute(0, 2, 3, 4, 1), dx, rtol=0, atol=1e-14)
    assert torch.allclose(al.grad, da, rtol=0, atol=1e-13)
    mags, rho = R.audio_mag(a, x, dout, case), R.MEASURED_RHO[("audio", case)]
    wo, wdx, wda = R.audio_fuse(a, x, dout, case, no_dot=True)
    assert torch.allclose(wo, out, rtol=0, atol=1e-14)                       # the forward is the same: only the backward is wrong
    if w * up > 1:                                                           # a one-pixel row has softmax = 1: the term is zero anyway
        assert fails(R.check_bound, wdx, dx, rho["dx"] * R.U * mags[1]) and fails(R.check_bound, wda, da, rho["da"] * R.U * mags[2])


def test_audio_table_contains_what_it_claims():
    ups = {c[5] for c in R.AUDIO_CASES}
    assert {1, 2, 3, 4, 8} <= ups and any(u & (u - 1) for u in ups)          # an up-factor that is no power of two
    assert any(c[1] == 1 for c in R.AUDIO_CASES) and {1, 2, 3} <= {c[2] // 32 for c in R.AUDIO_CASES}
    assert any((c[4] * c[5]) % 8 and c[4] * c[5] > 8 for c in R.AUDIO_CASES)
    assert R.AUDIO_REFUSED[5] > 8


# ---- the measured bounds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(R.MEASURERS))
def test_measured_bounds_are_four_times_the_fp32_cpu_and_no_looser_than_before(family):
    fn, cases = R.MEASURERS[family]
    for case in cases:
        table = R.MEASURED_RHO[(family, case)]
        for name, worst in fn(case).items():
            want = R.rho(worst)
            # the table holds the ratio rounded up to a decimal; another CPU's libm may move it a little
            assert want <= table[name] * 1.25 and table[name] <= 1.25 * want + 0.4, (family, case, name, worst, table[name])
    # never looser than the assertions these kernels had (max |err| below 2e-5, 5e-5 for the audio gradients, of max |ref|): the
    # tolerance is the smaller of the two, element by element
    for case in cases:
        for n, tol, r in R.measured_tols(family, case):
            assert float(tol.max()) <= R.OLD_REL[family] * float(r.abs().max()) and float(tol.min()) > 0, (family, case, n)


# ---- unpack_frames, dropout ------------------------------------------------------------------------------------------------------------
def test_unpack_frames_reference_has_power():
    for B, C, Tv, Tin, hw in R.UNPACK_CASES:
        frames = R.nz_ints(R.generator(B + C + Tv + Tin + hw), (B, Tin, hw, C))
        ref = R.unpack_frames_ref(frames, Tv)
        vis = torch.zeros(B, C, Tin, hw, dtype=torch.float64, requires_grad=True)       # the forward: NCT(hw) -> frames
        (vis.permute(0, 2, 3, 1) * frames).sum().backward()
        assert torch.equal(vis.grad[:, :, :Tv], ref)
        if Tin > Tv:
            assert fails(R.check_exact, f32(R.unpack_frames_ref(frames, Tv, keep_all=True)), ref)
    assert any(c % 64 and c > 64 for _, c, *_ in R.UNPACK_CASES) and any(tv * hw % 64 for _, _, tv, _, hw in R.UNPACK_CASES)


def _csrc(name):
    import os

    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diff_sal_amd", "csrc", name)).read()


def test_grid_caps_are_the_ones_in_the_code():
    """The sizes 'past the grid cap' are past the caps the launches really have."""
    import re

    bw, op = _csrc("backward.hip"), _csrc("optim.hip")
    m = re.search(r"static int ew_grid_b\(long total\) \{\s*long g = \(total \+ 255\) / 256;\s*return static_cast<int>\(g > (\d+) \? (\d+)", bw)
    assert m and int(m.group(1)) == int(m.group(2)) and int(m.group(1)) * 256 == R.DROPOUT_CAP      # dropout: one element per thread and trip
    m = re.search(r"const int grid = static_cast<int>\(need < (\d+)L \* (\d+) \? need : (\d+)L \* (\d+)\);", op)
    assert m and int(m.group(1)) * int(m.group(2)) * 256 * 4 == R.ADAM_CAP
    assert re.search(r"constexpr int kRedBlock = 256;", op) and re.search(r"diffsal_reduce_blocks\(void\) \{ return 1024; \}", op)
    assert max(R.DROPOUT_NS) > R.DROPOUT_CAP and max(R.ADAM_NS) > R.ADAM_CAP and max(R.MSE_NS) > R.REDUCE_CAP and max(R.NORM_NS) > R.REDUCE_CAP
    # head_bwd: blocks = min(1024, max(1, M // 64)) in ops.head_bwd
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diff_sal_amd", "ops.py")).read()
    assert "blocks = min(1024, max(1, M // 64))" in src


def test_dropout_restatement_keeps_one_minus_p():
    n = 2 ** 16
    for p in R.DROPOUT_PS:
        for seed in R.DROPOUT_SEEDS:
            keep = float(R.dropout_keep(n, p, seed).double().mean())
            assert abs(keep - (1 - p)) <= 3 * (p * (1 - p) / n) ** 0.5, (p, seed, keep)
    a, b = (R.dropout_keep(n, 0.5, s) for s in R.DROPOUT_SEEDS)
    assert (R.DROPOUT_SEEDS[0] & 0xFFFFFFFF) == (R.DROPOUT_SEEDS[1] & 0xFFFFFFFF) and not torch.equal(a, b)
    assert max(R.DROPOUT_NS) > R.DROPOUT_CAP
    x = torch.full((8,), 3.0)
    assert torch.equal(R.dropout_ref(x, 0.0, 1), x)


# ---- mse_loss, grad_norm ---------------------------------------------------------------------------------------------------------------
def test_mse_reference_tables_and_power():
    from diff_sal_amd import _lib

    assert R.REDUCE_CAP == _lib.load().diffsal_reduce_blocks() * 256 * 4
    assert {n % 4 for n in R.MSE_NS} == {0, 1, 2, 3} and max(R.MSE_NS) > R.REDUCE_CAP and min(R.MSE_NS) < 4
    assert {n % 4 for n in R.NORM_NS + R.ADAM_NS} == {0, 1, 2, 3} and max(R.NORM_NS) > R.REDUCE_CAP
    for n in (1, 3, 5, 6, 63):
        pred, tgt = R.mse_operands(n)
        loss, dp, mag = R.mse64(pred, tgt, 0.7 / 3)
        p = pred.clone().requires_grad_(True)
        ref = 0.7 * (p.double() - tgt.double()).square().sum() / 3
        ref.backward()
        assert abs(float(loss) - float(ref)) < 1e-7 * float(ref) and float((dp.double() - p.grad.double()).abs().max()) < 1e-6
        bad_loss, bad_dp, _ = R.mse64(pred, tgt, 0.7 / 3, drop_tail=True)
        assert fails(R.check_bound, bad_loss, loss, R.MSE_K * R.U * mag)
        assert not torch.equal(bad_dp, dp)


def test_grad_norm_operands_span_forty_binades():
    g = R.norm_operands(1000, spread=True)
    e = torch.frexp(g[g != 0])[1]
    assert int(e.max()) - int(e.min()) >= 36
    ref = g.double().norm()
    assert fails(R.check_bound, g[:-1].double().norm() * (1 + 4 * R.NORM_REL), ref, R.NORM_REL * ref)


# ---- adam_step -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", R.ADAM_WD)
def test_adam_restatement_is_torch_adam(wd):
    hp = R.ADAM_HP
    p, g, m, v = (t.double() for t in R.adam_operands(1000))
    ref_p = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([ref_p], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=wd)
    state = (p, m, v)
    for step in (1, 2, 3):
        gs = g * step
        ref_p.grad = gs.clone()
        if step == 1:                                                        # start torch from the same moments
            opt.step()
            st = opt.state[ref_p]
            ref_p.data.copy_(p)
            st["exp_avg"].copy_(m)
            st["exp_avg_sq"].copy_(v)
            st["step"].fill_(0)
        opt.step()
        st = opt.state[ref_p]
        out = R.adam_step64(*[t.float() for t in (state[0], gs, state[1], state[2])], step=step, wd=wd, coef=np.float32(1.0), lr=hp["lr"],
                            beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"])
        # the restatement starts from the fp32 image of the state and rounds its constants to fp32: 1e-7 of the operands, more where
        # m + (g - m) / 10 cancels; a wrong formula (decay, bias corrections) is wrong by a factor
        assert torch.allclose(out["m"], st["exp_avg"], rtol=1e-5, atol=1e-9) and torch.allclose(out["v"], st["exp_avg_sq"], rtol=1e-5, atol=1e-12)
        assert torch.allclose(out["step"], ref_p.detach() - state[0], rtol=1e-4, atol=1e-10)
        for wrong in ("no_bc2",) + (("late_wd",) if wd else ()):
            bad = R.adam_step64(*[t.float() for t in (state[0], gs, state[1], state[2])], step=step, wd=wd, coef=np.float32(1.0), lr=hp["lr"],
                                beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"], wrong=wrong)
            assert not torch.allclose(bad["step"], ref_p.detach() - state[0], rtol=1e-4, atol=1e-10)
        state = (ref_p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())


def test_adam_tables_and_power():
    hp = R.ADAM_HP
    assert max(R.ADAM_NS) > R.ADAM_CAP and {n % 4 for n in R.ADAM_NS} >= {0, 1, 3} and min(R.ADAM_NS) < 4
    for i, name in enumerate(("wd", "step", "norm", "store", "gscale")):
        want = set((R.ADAM_WD, R.ADAM_STEPS, R.ADAM_NORMS, R.ADAM_STORE, R.ADAM_GSCALE)[i])
        assert {c[i] for c in R.ADAM_LARGE} == want and {c[i] for c in R.ADAM_GRID} == want, name
    assert float(R.adam_coef(0.25, np.float32(0.5), 1.0)) == 0.25 and float(R.adam_coef(1.0, np.float32(4.0), 1.0)) < 0.26
    p, g, m, v = R.adam_operands(70003)
    for step in R.ADAM_STEPS:
        kw = dict(step=step, coef=np.float32(1.0), lr=hp["lr"], beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"])
        ref = R.adam_step64(p, g, m, v, wd=0.01, **kw)
        late = R.adam_step64(p, g, m, v, wd=0.01, wrong="late_wd", **kw)
        assert fails(R.check_bound, late["m"], ref["m"], ref["tol_m"]) and fails(R.check_bound, late["v"], ref["v"], ref["tol_v"])
        assert fails(R.check_bound, late["step"], ref["step"], ref["tol_step"])
        nobc = R.adam_step64(p, g, m, v, wd=0.01, wrong="no_bc2", **kw)
        assert fails(R.check_bound, nobc["step"], ref["step"], ref["tol_step"])
        # and the bounds are tight enough to mean something: far below the quantities themselves
        assert float((ref["tol_m"] / ref["m"].abs().clamp_min(1e-12)).median()) < 1e-6
        assert float((ref["tol_step"] / ref["step"].abs().clamp_min(1e-12)).median()) < 2e-2
    z = R.adam_operands(16, denom_eps=True)
    out = R.adam_step64(*z, step=1, wd=0.0, coef=np.float32(1.0), lr=hp["lr"], beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"])
    assert float(out["v"].abs().max()) == 0.0 and bool(torch.isfinite(out["step"]).all()) and float(out["step"].abs().min()) > 0
