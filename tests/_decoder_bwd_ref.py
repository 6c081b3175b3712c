"""fp64 references for the decoder's small training kernels: the spatial adjoints, the parameter-gradient reductions and the optimizer
tail (csrc/backward.hip, col2im in csrc/pack.hip, tapsum_bwd in csrc/tapsum.hip, csrc/optim.hip).

This module holds, for tests/test_decoder_bwd_host.py (no GPU) and tests/test_gpu_decoder_bwd.py:
  * a plain fp64 restatement of every kernel (torch autograd where the operation has a torch form), each with the switch that makes it
    wrong the way a kernel could be wrong (the power checks of the host file);
  * operand generators: small integers (tests/_exact_ref.py) wherever the arithmetic is sums of products, so that every fp32 partial
    sum is exact in any order and "equal" means bit-equal; continuous values where rounding is inherent;
  * the case tables, each row with the launch boundary it sits on, and the bounds.

Two kinds of bound.  COUNTED: k * 2^-24 * sum |terms| per element, k = the fp32 roundings on the path, written next to the reference.
MEASURED (a transcendental on the path: expf, swish, sigmoid): rho * 2^-24 * mag per element, mag = the first-order magnitude written
next to the reference, rho = 4 x max(1, worst err / (2^-24 mag) of fp32 CPU torch autograd of the same expression against fp64 on the
same inputs); the host file measures it and checks the figure kept in the table."""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

from tests._exact_ref import LIMIT, generator, ints  # noqa: F401
from tests._train_nodes_ref import case_id, check_bound, check_elementwise, check_exact  # noqa: F401

U = 2.0 ** -24
f32 = np.float32


def nz_ints(g, shape, r=4):
    """Integers in [-r, r] without zero (a zero operand would hide a wrong tap)."""
    t = ints(g, shape, r)
    return torch.where(t == 0, torch.full_like(t, 3.0), t)


def worst_ratio(got, ref, mag):
    """max |got - ref| / (2^-24 mag) over the elements (0 / 0 counts as 0)."""
    err = (got.detach().double() - ref.detach().double()).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / (U * mag.detach().double()))
    return float(r.max()) if r.numel() else 0.0


# ---- bilinear resize adjoint -----------------------------------------------------------------------------------------------------------
# (h, w) -> (H, W), C.  Exact: power-of-two factors up and down, identity, one equal axis; bounded: every other ratio.
RESIZE_EXACT = [((3, 5), (6, 10), 8), ((2, 3), (32, 48), 4), ((5, 4), (10, 8), 1), ((5, 4), (10, 8), 6), ((4, 6), (4, 6), 8),
                ((4, 6), (8, 6), 8), ((8, 12), (4, 6), 4), ((16, 8), (2, 1), 4)]
RESIZE_BOUNDED = [((3, 5), (7, 9), 4), ((7, 9), (3, 5), 4), ((5, 7), (12, 20), 1), ((1, 1), (5, 3), 4)]


def resize_routes(case):
    """The routes of diffsal_resize_bilinear_bwd a case can take: 'separable' (C % 4 == 0, a workspace, not the identity), 'joint4' (C % 4
    == 0 without a workspace: the raw binding with a null one; what ops selects at the identity), 'scalar' (C % 4 != 0, or a gradient
    that is not 16-byte aligned: a view 4 bytes into a buffer)."""
    (h, w), (H, W), C = case
    if C % 4:
        return ["scalar"]
    return (["separable"] if (h, w) != (H, W) else []) + ["joint4", "scalar"]


def bilin_axis(L, l):
    """fp32 restatement of bilin_coord (csrc/common.h) for the L outputs of an axis with l inputs: -> (i0, i1, w0, w1, p) numpy
    arrays, w0 = fl(1 - l1), w1 = l1, p = (Y + 0.5) scale.  scale = fl(l / L) as the entry point forms it."""
    scale = f32(l) / f32(L)
    Y = np.arange(L, dtype=f32)
    p = (Y + f32(0.5)) * scale
    s = np.maximum(p - f32(0.5), f32(0))
    i0 = np.minimum(s.astype(np.int32), l - 1)
    i1 = i0 + (i0 < l - 1)
    l1 = (s - i0.astype(f32)).astype(f32)
    return i0, i1, (f32(1) - l1).astype(f32), l1, p


def bilin_matrix(L, l, wrong=None):
    """A [L x l] in fp64: output Y takes w0 of input i0 and w1 of i1; where the two coincide (the clamped edge) the kernel's weight is
    fl(w0 + w1).  ``wrong``: 'edge' leaves out the clamped edge tap (w1 where i1 == i0), 'short' ends every input's gather window one
    output early (its last contributing output is missed)."""
    i0, i1, w0, w1, _ = bilin_axis(L, l)
    A = np.zeros((L, l))
    for Y in range(L):
        if i0[Y] == i1[Y]:
            A[Y, i0[Y]] = float(w0[Y]) if wrong == "edge" else float(f32(w0[Y] + w1[Y]))
        else:
            A[Y, i0[Y]], A[Y, i1[Y]] = float(w0[Y]), float(w1[Y])
    if wrong == "short":
        for i in range(l):
            nzr = np.nonzero(A[:, i])[0]
            if len(nzr):
                A[nzr[-1], i] = 0.0
    return torch.from_numpy(A)


def bilin_slack(L, l):
    """dA [L x l]: how far a weight may sit from bilin_matrix's when the compiler forms (Y + 0.5) scale - 0.5 with one rounding (a fused
    multiply-add) instead of two: the coordinate moves by at most ulp(p) / 2 + ulp(s) <= 2 ulp(p), and with it both weights -- or,
    across an integer, the taps one place on.  Zero where the arithmetic is exact (p a dyadic number of few bits)."""
    i0, _, _, _, p = bilin_axis(L, l)
    scale = f32(l) / f32(L)
    exact = np.all((np.arange(L) + 0.5) * float(scale) == p.astype(np.float64))
    D = np.zeros((L, l))
    if not exact:
        for Y in range(L):
            for i in range(max(0, i0[Y] - 1), min(l, i0[Y] + 3)):
                D[Y, i] = 2.0 * float(np.spacing(f32(max(p[Y], 0.5))))
    return torch.from_numpy(D)


def resize_operands(case, N=2, exact=True, seed=0):
    (h, w), (H, W), C = case
    g = generator(2000 + seed + 17 * H + W + C)
    return ints(g, (N, H, W, C)) if exact else torch.randn(N, H, W, C, generator=g).float().double()


def resize_bwd64(dy, h, w, wrong=None):
    """dx [N, h, w, C] = A_y^T dy A_x in fp64."""
    N, H, W, C = dy.shape
    return torch.einsum("yi,xj,nyxc->nijc", bilin_matrix(H, h, wrong), bilin_matrix(W, w, wrong), dy.double())


def resize_fwd64(x, H, W):
    """y [N, H, W, C] = A_y x A_x^T: the forward the adjoint belongs to (the host file ties it to F.interpolate)."""
    N, h, w, C = x.shape
    return torch.einsum("yi,xj,nijc->nyxc", bilin_matrix(H, h), bilin_matrix(W, w), x.double())


def resize_taps(case):
    """(ny, nx): the most outputs any one input gathers from, per axis."""
    (h, w), (H, W), C = case
    return int((bilin_matrix(H, h) != 0).sum(0).max()), int((bilin_matrix(W, w) != 0).sum(0).max())


def resize_bound(dy, case, route):
    """COUNTED.  separable: a chain of ny fmaf per element of the row pass, then nx of the column pass: k = ny + nx.  joint / scalar: one
    product wy wx and one fmaf per tap pair: k = ny nx + 1.  Plus the weights' own slack (bilin_slack) on |dy|."""
    (h, w), (H, W), C = case
    ny, nx = resize_taps(case)
    k = ny + nx if route == "separable" else ny * nx + 1
    Ay, Ax = bilin_matrix(H, h).abs(), bilin_matrix(W, w).abs()
    Dy, Dx = bilin_slack(H, h), bilin_slack(W, w)
    a = dy.double().abs()
    e = lambda P, Q: torch.einsum("yi,xj,nyxc->nijc", P, Q, a)
    return k * U * e(Ay, Ax) + e(Dy, Ax + Dx) + e(Ay, Dx)


def dyadic_bits(A):
    """Smallest q with A 2^q integral."""
    for q in range(0, 13):
        if bool(((A * 2.0 ** q) == (A * 2.0 ** q).round()).all()):
            return q
    raise AssertionError("not dyadic")


def resize_partial_max(case, r=4):
    """Largest |partial sum| of an exact case in units of its last bit: sum |wy| sum |wx| r 2^(qy + qx)."""
    (h, w), (H, W), C = case
    Ay, Ax = bilin_matrix(H, h), bilin_matrix(W, w)
    return float(Ay.abs().sum(0).max() * Ax.abs().sum(0).max()) * r * 2.0 ** (dyadic_bits(Ay) + dyadic_bits(Ax))


# ---- tapsum_bwd ------------------------------------------------------------------------------------------------------------------------
# (H, W), (h, w), C, dil: factor 1 (h == H), 2, 4, and 8 with h = w = 2 (the smallest map the entry accepts)
TAPSUM_CASES = [((8, 12), hw, C, dil) for hw in ((8, 12), (4, 6), (2, 3)) for C in (4, 12) for dil in (1, 2)] + \
               [((16, 16), (2, 2), C, dil) for C in (4, 12) for dil in (1, 2)]
TAPSUM_SLICE_CASE = ((8, 12), (4, 6), 4, 2)


def tapsum_operands(case, N=2, seed=0):
    (H, W), (h, w), C, dil = case
    return ints(generator(2100 + seed + H + 3 * h + C + dil), (N, H, W, C))


def shift_tap(du, ky, kx, dil, flip=False):
    """S[n, Y, X] = du[n, Y - dil (ky - 1), X - dil (kx - 1)], zero outside the image (``flip``: the shift's sign reversed)."""
    N, H, W, C = du.shape
    sy, sx = dil * (ky - 1), dil * (kx - 1)
    if flip:
        sy, sx = -sy, -sx
    out = torch.zeros_like(du)
    ys, xs = slice(max(0, sy), min(H, H + sy)), slice(max(0, sx), min(W, W + sx))
    yd, xd = slice(max(0, -sy), min(H, H - sy)), slice(max(0, -sx), min(W, W - sx))
    out[:, ys, xs] = du[:, yd, xd]
    return out


def tapsum_bwd64(du, h, w, dil, flip=False):
    """dY [N, h, w, 9 C] (tap-major): per tap A_y^T shift_tap(dU) A_x."""
    N, H, W, C = du.shape
    Ay, Ax = bilin_matrix(H, h), bilin_matrix(W, w)
    taps = [torch.einsum("yi,xj,nyxc->nijc", Ay, Ax, shift_tap(du.double(), ky, kx, dil, flip)) for ky in range(3) for kx in range(3)]
    return torch.stack(taps, 3).reshape(N, h, w, 9 * C)


# ---- col2im ----------------------------------------------------------------------------------------------------------------------------
# (kh, kw, stride, pad, extra; H, W; C); extra = rows / columns the forward padded on the bottom / right only (the asymmetric-pad
# Downsample): the output size counts them, the gradient has no pixel for them.
COL2IM_DISJOINT = [(5, 1, (5, 1), (0, 0), (0, 0), 9, 7, 4),          # ReduceTemp's form: rows 5-8 have no window
                   (3, 3, (4, 4), (0, 0), (0, 0), 10, 14, 12),       # stride > kernel: a gap after every window
                   (2, 2, (2, 2), (0, 0), (0, 0), 5, 7, 4),          # last row and column uncovered
                   (3, 3, (3, 3), (1, 1), (0, 0), 7, 8, 4)]          # padding: the first window starts outside
COL2IM_GATHER = [(3, 3, (2, 2), (0, 0), (0, 0), 7, 9, 4),
                 (3, 3, (2, 2), (1, 1), (0, 0), 6, 6, 12),
                 (5, 5, (2, 2), (2, 2), (0, 0), 7, 5, 4),
                 (3, 1, (2, 1), (1, 0), (0, 0), 9, 4, 4),
                 (3, 3, (2, 2), (0, 0), (1, 1), 6, 8, 4)]            # out_hw of the asymmetric-pad Downsample: 3 x 4, not the 2 x 3 of pad 0


def col2im_out_hw(case):
    kh, kw, stride, pad, extra, H, W, C = case
    return (H + 2 * pad[0] + extra[0] - kh) // stride[0] + 1, (W + 2 * pad[1] + extra[1] - kw) // stride[1] + 1


def col2im_operands(case, N=2, seed=0):
    kh, kw, stride, pad, extra, H, W, C = case
    Ho, Wo = col2im_out_hw(case)
    return nz_ints(generator(2200 + seed + kh + 5 * H + W + C), (N * Ho * Wo, kh * kw * C))


def col2im64(cols, case, N=2, wrong=False):
    """dx [N, H, W, C] by F.fold in fp64; the columns are (ky, kx, c), fold wants (c, ky, kx).  ``wrong``: the taps read as (kx, ky)
    (a kh x 1 kernel has no transpose: there ky is reversed instead)."""
    kh, kw, stride, pad, extra, H, W, C = case
    Ho, Wo = col2im_out_hw(case)
    c5 = cols.double().reshape(N, Ho * Wo, kh, kw, C)
    if wrong:
        c5 = c5.reshape(N, Ho * Wo, kw, kh, C).transpose(2, 3) if kh == kw else c5.flip(2)
    blocks = c5.permute(0, 4, 2, 3, 1).reshape(N, C * kh * kw, Ho * Wo)
    Hp, Wp = H + 2 * pad[0] + extra[0], W + 2 * pad[1] + extra[1]
    full = F.fold(blocks, (Hp, Wp), (kh, kw), stride=stride)                 # onto the padded image, then cut the padding off
    return full[:, :, pad[0]:pad[0] + H, pad[1]:pad[1] + W].permute(0, 2, 3, 1).contiguous()


# ---- depthwise convolution -------------------------------------------------------------------------------------------------------------
# C, H, W, k, stride, pad
DWCONV_CASES = [(4, 5, 7, 3, 1, 1),            # baseline
                (8, 9, 13, 4, 4, 0),           # trailing rows uncovered
                (12, 7, 5, 3, 2, 1),           # 1 < stride < k
                (8, 4, 4, 2, 3, 0),            # stride > k
                (40, 6, 6, 2, 2, 0),           # c4n = 10: 256 / 10 = 25 pixel lanes, 6 threads idle
                (96, 16, 32, 16, 16, 0),       # chunk count falls to 1
                (516, 3, 3, 3, 1, 1),          # c4n = 129: one pixel lane, 127 threads idle
                (1024, 3, 3, 3, 1, 1),         # c4n = 256: one pixel lane, no thread idle
                (8, 7, 11, 3, 1, 1)]           # P = 154 over 3 chunks: boundaries at 51 and 102


def dw_chunks(N, H, W, k, stride, pad):
    """diffsal_dwconv_bwd_weight_chunks restated."""
    P = N * ((H + 2 * pad - k) // stride + 1) * ((W + 2 * pad - k) // stride + 1)
    chunks = max(1, 2048 // (k * k))
    while chunks > 1 and P // chunks < 32:
        chunks >>= 1
    return min(chunks, 256), P


def dwconv_operands(case, N=2, seed=0):
    C, H, W, k, stride, pad = case
    g = generator(2300 + seed + C + 3 * H + k)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return nz_ints(g, (N, H, W, C)), nz_ints(g, (k * k, C)), nz_ints(g, (N, Ho, Wo, C))


def dwconv64(x, w, du, case):
    """(out, dx, dw) by fp64 autograd of F.conv2d(groups = C); NHWC, w [k k, C]."""
    C, H, W, k, stride, pad = case
    xl = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    wl = w.double().t().reshape(C, 1, k, k).clone().requires_grad_(True)
    out = F.conv2d(xl, wl, stride=stride, padding=pad, groups=C)
    out.backward(du.double().permute(0, 3, 1, 2))
    return out.detach().permute(0, 2, 3, 1).contiguous(), xl.grad.permute(0, 2, 3, 1).contiguous(), wl.grad.reshape(C, k * k).t().contiguous()


def dwconv_bwd_data_walk(du, w, case, start0=False):
    """The tap walk of dwconv_bwd_data_kernel: for an input row iy the taps ky = (iy + pad) % stride, + stride, ... < k, each from output
    (iy + pad - ky) / stride.  ``start0``: the walk begins at tap 0 (the quotient then truncates: the wrong output row)."""
    C, H, W, k, stride, pad = case
    N, Ho, Wo, _ = du.shape
    dx = torch.zeros(N, H, W, C, dtype=torch.float64)
    for iy in range(H):
        for ky in range(0 if start0 else (iy + pad) % stride, k, stride):
            oy = (iy + pad - ky) // stride
            if iy + pad - ky < 0 or oy >= Ho:
                continue
            for ix in range(W):
                for kx in range(0 if start0 else (ix + pad) % stride, k, stride):
                    ox = (ix + pad - kx) // stride
                    if ix + pad - kx < 0 or ox >= Wo:
                        continue
                    dx[:, iy, ix] += du[:, oy, ox].double() * w[ky * k + kx].double()
    return dx


def dwconv_dw_missing_pixel(x, du, case, chunk=0):
    """The weight gradient without the last pixel of chunk ``chunk`` (pe - 1 of the partition P chunk / chunks)."""
    C, H, W, k, stride, pad = case
    N = x.shape[0]
    chunks, P = dw_chunks(N, H, W, k, stride, pad)
    pix = P * (chunk + 1) // chunks - 1
    du2 = du.clone().reshape(P, C)
    du2[pix] = 0
    return dwconv64(x, torch.ones(k * k, C), du2.reshape(du.shape), case)[2]


# ---- head_bwd ----------------------------------------------------------------------------------------------------------------------------
# (M, C); blocks = min(1024, max(1, M // 64)), rows per pass rpp = 256 / (C / 4)
HEAD_CASES = [(1, 4),                          # one row, one block, 63 row lanes idle
              (63, 96), (65, 96),              # M // 64 = 0 -> 1 block; 65 -> still 1 block, 7 passes of 10 rows
              (130, 40),                       # c4n = 10 (does not divide 256), 2 blocks
              (100, 516),                      # c4n = 129
              (200, 1024),                     # c4n = 256, 3 blocks
              (64 * 1024 + 77, 4)]             # M // 64 = 1025: the block cap of 1024
HEAD_S = (0.25, 0.5, 0.75)


def head_operands(case, seed=0):
    """y [M, C], w [C], ds [M] integers; s_out from {1/4, 1/2, 3/4}: ds s (1 - s) is a multiple of 1/16, every product exact."""
    M, C = case
    g = generator(2400 + seed + M + C)
    s = torch.tensor(HEAD_S, dtype=torch.float64)[torch.randint(0, 3, (M,), generator=g)]
    return nz_ints(g, (M, C)), nz_ints(g, (C,)), s, nz_ints(g, (M,))


def head_bwd64(y, w, s, ds, drop_row=None):
    """(dy [M, C], dw [C], db [1]).  ``drop_row``: the bias sum misses that row."""
    dp = ds.double() * s.double() * (1.0 - s.double())
    dpb = dp.clone()
    if drop_row is not None:
        dpb[drop_row] = 0
    return dp[:, None] * w.double()[None], (dp[:, None] * y.double()).sum(0), dpb.sum().reshape(1)


HEAD_E2E_CASES = [(63, 96), (130, 40), (100, 516)]


def head_e2e_operands(case, seed=0):
    M, C = case
    g = generator(2450 + seed + M + C)
    return (torch.randn(M, C, generator=g), 0.2 * torch.randn(C, generator=g), torch.randn(1, generator=g), torch.randn(M, generator=g))


def head_e2e(y, w, b, ds):
    """(s, dy, dw, db) of s = sigmoid(y w + b) under autograd, in the operands' precision."""
    yl, wl, bl = (t.detach().clone().requires_grad_(True) for t in (y, w, b))
    s = torch.sigmoid(yl @ wl + bl)
    s.backward(ds)
    return s.detach(), yl.grad, wl.grad, bl.grad


def head_e2e_mag(y, w, b, ds):
    """MEASURED.  First-order magnitudes: e = sum |y| |w| + |b| (what the rounding of the logit scales with), s' = s (1 - s);
    s: s (1 + e);  dpre = ds s': D = |ds| (s' (1 + e) + s) -- the last term because 1 - s is formed from the rounded s and cancels where
    s is close to 1;  dy: D |w|;  dw: sum_m D |y|;  db: sum_m D."""
    y, w, b, ds = (t.double() for t in (y, w, b, ds))
    e = 1.0 + y.abs() @ w.abs() + b.abs()
    s = torch.sigmoid(y @ w + b)
    dp = ds.abs() * (s * (1 - s) * e + s)
    return s * e, dp[:, None] * w.abs()[None], (dp[:, None] * y.abs()).sum(0), dp.sum().reshape(1)


# ---- conv_in_bwd -----------------------------------------------------------------------------------------------------------------------
# (B, H, W, C); always 128 chunks
CONV_IN_CHUNKS = 128
CONV_IN_CASES = [(1, 1, 1, 8),                 # 1 x 1 image: eight of nine taps fall outside; P = 1 < chunks
                 (1, 3, 3, 4),                 # P = 9 < chunks: 119 empty chunks
                 (2, 5, 7, 96),                # P = 70 < chunks
                 (3, 24, 40, 40),              # c4n = 10, P = 2880: chunks of 22 and 23 pixels
                 (1, 12, 11, 1024)]            # c4n = 256, P = 132: chunks of 1 and 2 pixels


def conv_in_operands(case, seed=0):
    B, H, W, C = case
    g = generator(2500 + seed + H + W + C)
    return nz_ints(g, (B, 1, H, W)), nz_ints(g, (B, H, W, C))


def conv_in_bwd64(x, dy, wrap=False):
    """(dw [C, 9], db [C]) of conv2d(x, w, b, padding = 1) by fp64 autograd.  ``wrap``: the border taps are not skipped -- they read
    the flat image at the index the tap's offset gives (the neighbouring row's or image's pixel, circularly)."""
    B, _, H, W = x.shape
    C = dy.shape[-1]
    g = dy.double().reshape(B * H * W, C)
    if wrap:
        flat = x.double().reshape(-1)
        idx = torch.arange(B * H * W)
        dw = torch.stack([(flat[(idx + (ky - 1) * W + (kx - 1)) % (B * H * W)][:, None] * g).sum(0) for ky in range(3) for kx in range(3)], 1)
        return dw, g.sum(0)
    wl = torch.zeros(C, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    bl = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wl, bl, padding=1).backward(dy.double().permute(0, 3, 1, 2))
    return wl.grad.reshape(C, 9), bl.grad


# ---- dense_small_bwd -------------------------------------------------------------------------------------------------------------------
# (B, K, N): the din kernel walks n in steps of 32 (four sums) while n + 24 < N, then a tail in steps of 8; k in blocks of 32
DENSE_CASES = [(1, 1, 1), (4, 33, 5), (3, 32, 8), (2, 40, 33), (1, 31, 57), (4, 384, 1344)]


def dense_operands(case, swish, seed=0):
    B, K, N = case
    g = generator(2600 + seed + B + K + N)
    if not swish:
        return nz_ints(g, (B, K)), nz_ints(g, (N, K)), nz_ints(g, (B, N))
    x = (16.0 * torch.rand(B, K, generator=g) - 8.0)                         # across [-8, 8]
    return x, torch.randn(N, K, generator=g) * 0.05, torch.randn(B, N, generator=g)


def dense_bwd(x, w, dout, swish, tail_from=None):
    """(dx, dw, db) of out = W f(x) + b (f = swish or the identity) under autograd in the operands' precision.  ``tail_from``: dx
    without the rows n >= tail_from of W (the din kernel's tail loop left out)."""
    xl, wl = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    bl = torch.zeros(w.shape[0], dtype=x.dtype, requires_grad=True)
    f = xl * torch.sigmoid(xl) if swish else xl
    d = dout.clone()
    out = F.linear(f, wl, bl)
    if tail_from is not None:
        out = out[:, :tail_from]
        d = d[:, :tail_from]
    out.backward(d)
    return xl.grad, wl.grad, bl.grad


def dense_mag(x, w, dout, swish):
    """Magnitudes: dx: F sum_n |dout| |w|, F = sg (1 + |x| (1 - sg)) (swish' = sg (1 + x (1 - sg)) with its terms taken positive: near
    its root at x = -1.28 the derivative cancels, its rounding does not) or 1;  dw: sum_b |dout| |f(x)|;  db: sum_b |dout|.  With swish
    these are MEASURED bounds' magnitudes; db is COUNTED: B - 1 additions."""
    x, w, dout = x.double(), w.double(), dout.double()
    sg = torch.sigmoid(x)
    f, fp = (x * sg, sg * (1 + x.abs() * (1 - sg))) if swish else (x, torch.ones_like(x))
    return fp.abs() * (dout.abs() @ w.abs()), dout.abs().t() @ f.abs(), dout.abs().sum(0)


# ---- audio_fuse ------------------------------------------------------------------------------------------------------------------------
# (B, T, C, h, w, up): workgroup = (b, row, 32-channel slab); the backward holds `up` <= 8 columns per audio cell in registers
AUDIO_CASES = [(1, 1, 32, 2, 2, 1),            # T = 1, one slab
               (2, 9, 64, 2, 4, 2),
               (1, 3, 32, 2, 3, 4),            # W = 12: not a multiple of 8 above 8
               (1, 9, 32, 3, 5, 3),            # up 3 (no power of two), W = 15
               (1, 2, 96, 1, 1, 8),            # three slabs, one audio cell
               (2, 2, 32, 2, 4, 1)]            # H = h: no upsampling
AUDIO_REFUSED = (1, 1, 32, 1, 1, 16)           # the forward takes any integer factor, the backward refuses above 8


def audio_operands(case, seed=0):
    B, T, C, h, w, up = case
    g = generator(2700 + seed + T + C + 3 * h + w + up)
    return (torch.randn(B * T, h * w, C, generator=g), torch.randn(B, T, h * up, w * up, C, generator=g),
            torch.randn(B, C, T, h * up, w * up, generator=g))


def audio_fuse_fn(a_small, x, case, no_dot=False):
    """out [B, C, T, H, W] = a softmax_x(mean_t a x), a = nearest-up(a_small), differentiable.  ``no_dot``: the softmax's backward
    without its - sum ds s term (the softmax treated as s * const)."""
    B, T, C, h, w, up = case
    a = a_small.reshape(B, T, h, w, C).permute(0, 4, 1, 2, 3)
    if up > 1:
        a = a.repeat_interleave(up, 3).repeat_interleave(up, 4)
    m = (a * x.permute(0, 4, 1, 2, 3)).mean(dim=2, keepdim=True)
    if no_dot:
        e = torch.exp(m - m.max(-1, keepdim=True)[0].detach())
        s = e / e.sum(-1, keepdim=True).detach()
    else:
        s = F.softmax(m, dim=-1)
    return a * s


def audio_fuse(a_small, x, dout, case, no_dot=False):
    """(out, dx [B, T, H, W, C], da [B T, h w, C]) under autograd in the operands' precision."""
    al, xl = a_small.detach().clone().requires_grad_(True), x.detach().clone().requires_grad_(True)
    out = audio_fuse_fn(al, xl, case, no_dot)
    out.backward(dout)
    return out.detach(), xl.grad, al.grad


def audio_mag(a_small, x, dout, case):
    """MEASURED.  With a, s, ds = sum_t dout a, dm = s (ds - sum_x ds s) as in the kernel and E = 1 + max_x mean_t |a| |x| (what an error
    of the logits scales with):  out: |a| s E;  dx: D |a| / T with D = s (|ds| + sum_x |ds| s) E;  da: sum over the cell of
    |dout| s E + D |x| / T."""
    B, T, C, h, w, up = case
    a_small, x, dout = a_small.double(), x.double(), dout.double()
    a = a_small.reshape(B, T, h, w, C).permute(0, 4, 1, 2, 3)
    if up > 1:
        a = a.repeat_interleave(up, 3).repeat_interleave(up, 4)
    xc = x.permute(0, 4, 1, 2, 3)
    s = F.softmax((a * xc).mean(2, keepdim=True), dim=-1)
    E = 1.0 + (a.abs() * xc.abs()).mean(2, keepdim=True).max(-1, keepdim=True)[0]
    ads = (dout.abs() * a.abs()).sum(2, keepdim=True)
    D = s * (ads + (ads * s).sum(-1, keepdim=True)) * E
    m_out = a.abs() * s * E
    m_dx = (D * a.abs() / T).permute(0, 2, 3, 4, 1)
    cell = dout.abs() * s * E + D * xc.abs() / T                              # [B, C, T, H, W]
    m_da = cell.reshape(B, C, T, h, up, w, up).sum((4, 6)).permute(0, 2, 3, 4, 1).reshape(B * T, h * w, C)
    return m_out, m_dx.contiguous(), m_da


# rho per case and output, MEASURED on the fp32 CPU (tests/test_decoder_bwd_host.py re-measures and checks them): 4 x max(1, worst ratio)
def rho(worst):
    return 4.0 * max(1.0, worst)


# ---- unpack_frames ---------------------------------------------------------------------------------------------------------------------
# (B, C, Tv, Tin, hw): 64 x 64 tiles over (q = t hw + pixel, channel)
UNPACK_CASES = [(2, 65, 2, 3, 33), (1, 4, 8, 9, 1), (1, 64, 1, 1, 64)]


def unpack_frames_ref(frames, Tv, keep_all=False):
    """[B, Tin, hw, C] -> [B, C, Tv, hw]: the first Tv frames, channels first (``keep_all``: the LAST Tv frames -- wrong on purpose)."""
    f = frames[:, -Tv:] if keep_all else frames[:, :Tv]
    return f.permute(0, 3, 1, 2).contiguous()


# ---- dropout ---------------------------------------------------------------------------------------------------------------------------
DROPOUT_CAP = 4096 * 256                       # ew_grid_b: at most 4096 blocks of 256 threads, one element per thread and trip
DROPOUT_NS = (1, 1000, 2 ** 16 + 3, DROPOUT_CAP + 5)
DROPOUT_PS = (0.0, 0.1, 0.5)
DROPOUT_SEEDS = (1234, (0x0BADC0DE << 32) | 1234)              # the same low word, two high words


def hash_u32(a, b):
    """csrc/backward.hip: h = a * 0x9E3779B1 ^ (b + 0x7F4A7C15); h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35;
    h ^= h >> 16 -- on numpy.uint32 arrays (the products wrap)."""
    a, b = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)
    with np.errstate(over="ignore"):
        h = (a * np.uint32(0x9E3779B1)) ^ (b + np.uint32(0x7F4A7C15))
        h ^= h >> np.uint32(16)
        h = h * np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h = h * np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return h


def dropout_keep(n, p, seed):
    """bool [n]: element i is kept iff hash(hash(i_lo, seed_lo), i_hi ^ seed_hi) >= (unsigned)(fl(p) 2^32)."""
    i = np.arange(n, dtype=np.uint64)
    lo, hi = (i & np.uint64(0xFFFFFFFF)).astype(np.uint32), (i >> np.uint64(32)).astype(np.uint32)
    h = hash_u32(hash_u32(lo, np.uint32(seed & 0xFFFFFFFF)), hi ^ np.uint32((seed >> 32) & 0xFFFFFFFF))
    thr = np.uint32(int(float(f32(p)) * 4294967296.0))
    return torch.from_numpy(h >= thr)


def dropout_ref(x, p, seed):
    """fp32: kept values are fl(x fl(1 / (1 - p)))."""
    scale = f32(1.0) / (f32(1.0) - f32(p))
    return torch.where(dropout_keep(x.numel(), p, seed).reshape(x.shape), x * torch.tensor(scale), torch.zeros_like(x))


# ---- mse_loss, grad_norm ---------------------------------------------------------------------------------------------------------------
REDUCE_CAP = 1024 * 256 * 4                    # diffsal_reduce_blocks() blocks of 256 threads, four elements per thread and trip
MSE_NS = (1, 3, 5, 6, 63, 4096, 2 ** 20 + 260, 3 * 2 ** 20 + 5)          # tail only; tails of 1, 2, 3; one trip; past the grid cap
MSE_K = 7                                      # p - t rounds once (twice in the square), the four-term fmaf chain 4, the cast to fp32 1
NORM_NS = (1, 2, 3, 5, 1000, 2 ** 22 + 3)
NORM_REL = 2.0 ** -23                          # fp64 sum of exact products, one rounding to fp32, one ulp of room for the fp64 sum order


def mse_operands(n, seed=0):
    g = generator(2800 + seed + n % 9973)
    return torch.rand(n, generator=g), torch.rand(n, generator=g)


def mse64(pred, target, loss_scale, drop_tail=False):
    """(loss fp64 scalar, dpred fp32 = fl(2 s) fl(p - t) as the kernel rounds, sum |terms| of the loss).  loss_scale enters as its fp32
    value.  ``drop_tail``: the n % 4 last elements are left out of the sum and keep a zero gradient."""
    s = float(f32(loss_scale))
    d32 = pred.float() - target.float()
    dp = torch.tensor(f32(2.0) * f32(loss_scale)) * d32
    d = pred.double() - target.double()
    if drop_tail:
        keep = pred.numel() // 4 * 4
        d, dp = d[:keep], torch.cat([dp[:keep], torch.zeros(pred.numel() - keep)])
    return s * (d * d).sum(), dp, s * (d * d).sum()


def norm_operands(n, spread=False, seed=0):
    g = generator(2900 + seed + n % 9973)
    x = torch.randn(n, generator=g)
    if spread:                                                               # entries across 2^-20 .. 2^20
        x = x * torch.exp2(torch.randint(-20, 21, (n,), generator=g).float())
    return x


# ---- adam_step -------------------------------------------------------------------------------------------------------------------------
ADAM_CAP = 4096 * 256 * 4                      # the grid cap of diffsal_adam_step: 256 * 16 blocks, 256 threads, four elements a trip
ADAM_NS = (1, 3, 4, 7, 70003, 2 ** 22 + 1027)
ADAM_SMALL = tuple(n for n in ADAM_NS if n <= 7)
ADAM_WD = (0.0, 0.01)
ADAM_STEPS = (1, 2, 1000)
ADAM_NORMS = ("absent", "below", "above")
ADAM_STORE = (0, 1)
ADAM_GSCALE = (1.0, 0.25)
ADAM_GRID = list(itertools.product(ADAM_WD, ADAM_STEPS, ADAM_NORMS, ADAM_STORE, ADAM_GSCALE))
# for the two large sizes: every value of every switch at least once
ADAM_LARGE = [(0.0, 1, "absent", 0, 1.0), (0.01, 2, "above", 1, 0.25), (0.01, 1000, "below", 1, 1.0), (0.0, 1000, "above", 0, 0.25)]
ADAM_HP = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=1.0)


def adam_operands(n, seed=0, denom_eps=False):
    """(p, g, m, v) fp32.  ``denom_eps``: v = 0 and g = 0, so the denominator of the step is eps alone."""
    gen = generator(3000 + seed + n % 9973)
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.01
    m, v = torch.randn(n, generator=gen) * 0.01, torch.rand(n, generator=gen) * 1e-4
    if denom_eps:
        g, v, m = torch.zeros(n), torch.zeros(n), m * 1e-6
    return p, g, m, v


def adam_coef(gscale, norm, max_norm):
    """The gradient's factor in fp32, as adam_kernel forms it: gscale * min(1, max_norm / (norm + 1e-6))."""
    c = f32(gscale)
    if norm is not None and max_norm > 0:
        c = c * min(f32(1.0), f32(max_norm) / (f32(norm) + f32(1e-6)))
    return f32(c)


def adam_step64(p, g, m, v, *, step, wd, coef, lr, beta1, beta2, eps, wrong=None):
    """One step of adam_one in fp64 from fp32 state, the constants rounded to fp32 exactly as diffsal_adam_step rounds them.
    -> dict(m, v, step (the change of p), g (the gradient written back: fl(g coef))) and the COUNTED bounds tol_m, tol_v, tol_step.
    ``wrong``: 'late_wd' adds the weight decay after the moment update (the moments see the bare gradient), 'no_bc2' leaves out the
    second bias correction."""
    omb1, b2, omb2 = float(f32(1.0 - beta1)), float(f32(beta2)), float(f32(1.0 - beta2))
    e, w = float(f32(eps)), float(f32(wd))
    ss = float(f32(lr / (1.0 - beta1 ** step)))
    bc2 = 1.0 if wrong == "no_bc2" else float(f32(np.sqrt(1.0 - beta2 ** step)))
    P, G, M, V = (t.double() for t in (p, g, m, v))
    g1 = G * float(coef)
    g2 = g1 if wrong == "late_wd" else g1 + w * P
    m2 = M + (g2 - M) * omb1
    v2 = omb2 * g2 * g2 + V * b2
    sq = v2.sqrt()
    den = sq / bc2 + e
    q = m2 / den
    stp = -ss * q
    if wrong == "late_wd":
        stp = stp - ss * w * P
    # roundings: g1 (1), the fmaf of the decay (1, only with wd), g2 - m (1), the fmaf of m (1): k = 4
    dg2 = U * (g1.abs() + (g2.abs() if w != 0 else 0.0))
    tol_m = omb1 * (dg2 + U * (g2 - M).abs()) + U * m2.abs()
    # g2^2 (1, on top of 2 |g2| dg2), v beta2 (1), the fmaf (1): k = 3 + those of g2
    tol_v = omb2 * (2 * g2.abs() * dg2 + U * g2 * g2) + U * (V * b2).abs() + U * v2.abs()
    # sqrtf (1), / bc2 (1), + eps (1), m / denom (1), the fmaf into p (1, of |p_new|): k = 5 + those of m and v
    d_sq = torch.where(sq > 0, 0.5 * tol_v / sq.clamp_min(1e-300), torch.zeros_like(sq)) + U * sq
    d_den = d_sq / bc2 + U * sq / bc2 + U * den
    d_q = tol_m / den + m2.abs() * d_den / (den * den) + U * q.abs()
    tol_step = ss * d_q + U * (P + stp).abs()
    g_out = (g.float() * torch.tensor(f32(coef))).float()
    fo = 1.0 + 2.0 ** -10                                                    # the bounds are first order: the products of roundings left out
    return dict(m=m2, v=v2, step=stp, g=g_out, tol_m=fo * tol_m, tol_v=fo * tol_v, tol_step=fo * tol_step)


# ---- the MEASURED bounds ---------------------------------------------------------------------------------------------------------------
def measure_dense(case):
    x, w, dout = dense_operands(case, True)
    ref, got = dense_bwd(x.double(), w.double(), dout.double(), True), dense_bwd(x, w, dout, True)
    return {n: worst_ratio(a, b, mg) for n, a, b, mg in zip(("dx", "dw", "db"), got, ref, dense_mag(x, w, dout, True))}


def measure_head(case):
    ops_ = head_e2e_operands(case)
    ref, got = head_e2e(*[t.double() for t in ops_]), head_e2e(*ops_)
    return {n: worst_ratio(a, b, mg) for n, a, b, mg in zip(("s", "dy", "dw", "db"), got, ref, head_e2e_mag(*ops_))}


def measure_audio(case):
    a, x, dout = audio_operands(case)
    ref, got = audio_fuse(a.double(), x.double(), dout.double(), case), audio_fuse(a, x, dout, case)
    return {n: worst_ratio(p, q, mg) for n, p, q, mg in zip(("out", "dx", "da"), got, ref, audio_mag(a, x, dout, case))}


MEASURERS = {"dense": (measure_dense, DENSE_CASES), "head": (measure_head, HEAD_E2E_CASES), "audio": (measure_audio, AUDIO_CASES)}

# rho = 4 x max(1, worst ratio of the fp32 CPU) per family, case and output, the ratio rounded up to one decimal
MEASURED_RHO = {
    ('dense', (1, 1, 1)): {'dx': 4.0, 'dw': 4.0, 'db': 4.0},
    ('dense', (4, 33, 5)): {'dx': 26.0, 'dw': 11.6, 'db': 4.0},
    ('dense', (3, 32, 8)): {'dx': 23.6, 'dw': 10.0, 'db': 4.0},
    ('dense', (2, 40, 33)): {'dx': 10.4, 'dw': 11.2, 'db': 4.0},
    ('dense', (1, 31, 57)): {'dx': 4.0, 'dw': 9.6, 'db': 4.0},
    ('dense', (4, 384, 1344)): {'dx': 4.4, 'dw': 16.8, 'db': 8.0},
    ('head', (63, 96)): {'s': 4.0, 'dy': 4.0, 'dw': 4.0, 'db': 4.0},
    ('head', (130, 40)): {'s': 4.0, 'dy': 4.0, 'dw': 4.0, 'db': 4.0},
    ('head', (100, 516)): {'s': 4.0, 'dy': 4.8, 'dw': 4.0, 'db': 4.0},
    ('audio', (1, 1, 32, 2, 2, 1)): {'out': 6.8, 'dx': 10.8, 'da': 8.0},
    ('audio', (2, 9, 64, 2, 4, 2)): {'out': 12.0, 'dx': 6.0, 'da': 5.2},
    ('audio', (1, 3, 32, 2, 3, 4)): {'out': 10.8, 'dx': 8.4, 'da': 4.0},
    ('audio', (1, 9, 32, 3, 5, 3)): {'out': 11.2, 'dx': 6.8, 'da': 4.0},
    ('audio', (1, 2, 96, 1, 1, 8)): {'out': 10.8, 'dx': 10.4, 'da': 4.0},
    ('audio', (2, 2, 32, 2, 4, 1)): {'out': 8.8, 'dx': 7.2, 'da': 8.0},
}


# what tests/test_gpu_train_ops.py accepts for these kernels, of max |ref|: a measured bound is never looser
OLD_REL = {"dense": 2e-5, "head": 2e-5, "audio": 5e-5}
_FAMILY = {"dense": (lambda c: dense_operands(c, True), lambda o, c: dense_bwd(*[t.double() for t in o], True), lambda o, c: dense_mag(*o, True),
                     ("dx", "dw", "db")),
           "head": (head_e2e_operands, lambda o, c: head_e2e(*[t.double() for t in o]), lambda o, c: head_e2e_mag(*o), ("s", "dy", "dw", "db")),
           "audio": (audio_operands, lambda o, c: audio_fuse(*[t.double() for t in o], c), lambda o, c: audio_mag(*o, c), ("out", "dx", "da"))}


def measured_tols(family, case):
    """[(name, tol, ref)] per output of a MEASURED family: tol = min(rho 2^-24 mag, OLD_REL max |ref|) element by element; ref in fp64."""
    make, ref, mag, names = _FAMILY[family]
    o = make(case)
    rho_ = MEASURED_RHO[(family, case)]
    return [(n, torch.minimum(rho_[n] * U * mg, torch.full_like(mg, OLD_REL[family] * float(r.abs().max()))), r)
            for n, r, mg in zip(names, ref(o, case), mag(o, case))]
