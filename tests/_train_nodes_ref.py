"""fp64 references for the kernels every training step runs outside the matrix pipe: the four saliency loss terms and their fused
backward (csrc/metrics.hip), the encoder's tape nodes (relative-position projection and tables, max-pool with arg-max, the token
transposes; csrc/mvit.hip, csrc/mvit_pool.hip) and the gradient gather of the optimizer (csrc/optim.hip).

This module holds, for tests/test_train_nodes_host.py (no GPU) and tests/test_gpu_loss_terms.py / test_gpu_encoder_nodes.py:
  * ``loss_terms64`` / ``loss_grad64``: CC / SIM / NSS / KL per image as a plain fp64 torch restatement of the formulas in
    csrc/metrics.hip's comments (unbiased std, eps = 2.2204e-16, min-max then sum normalisation for SIM) under autograd, and
    ``loss_grad_closed64``: the closed forms of metric_bwd_kernel, with switches that make it deliberately wrong (power checks);
  * the operand generators (seeded ``torch.Generator``): the loss-input families and the small integers of tests/_exact_ref.py;
  * fp64 references of the encoder nodes, each with the switch that breaks it the way a kernel could be broken;
  * ``check_bound`` / ``check_elementwise`` and the case tables shared by the host file and the GPU files.
"""
import types

import torch
import torch.nn.functional as F

from tests._exact_ref import LIMIT, generator, ints  # noqa: F401  (re-exported: the GPU files take them from here)

EPS = 2.2204e-16
TERMS = ("cc", "sim", "nss", "kl")


# ---- comparison --------------------------------------------------------------------------------------------------------------------
def check_bound(got, ref, tol, what=""):
    """|got - ref| <= tol for every element (``tol`` a tensor of ref's shape); reports the worst index; -> worst |err| / tol
    (0 / 0 counts as 0: an element whose bound is zero has to be exact)."""
    got, ref, tol = got.detach().double().cpu(), ref.detach().double().cpu(), tol.detach().double().cpu()
    assert got.shape == ref.shape == tol.shape, (what, tuple(got.shape), tuple(ref.shape), tuple(tol.shape))
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)          # err > 0 with tol == 0 -> inf
    worst = int(ratio.argmax()) if ratio.numel() else 0
    w = float(ratio.flatten()[worst]) if ratio.numel() else 0.0
    if not w <= 1.0:
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), ratio.shape)) if ratio.dim() else ()
        raise AssertionError(f"{what}: worst element {idx}: got {float(got.flatten()[worst])!r}, reference {float(ref.flatten()[worst])!r}, "
                             f"|err| {float(err.flatten()[worst]):.3e} = {w:.3g} x its bound {float(tol.flatten()[worst]):.3e}; "
                             f"{int((ratio > 1).sum())} of {ratio.numel()} elements exceed theirs")
    return w


def check_elementwise(got, ref, rel, floor, what=""):
    """|got - ref| <= rel * |ref| + floor * max|ref| for every element; -> the worst observed ratio of error to bound."""
    r = ref.detach().double().cpu()
    return check_bound(got, r, rel * r.abs() + floor * (float(r.abs().max()) if r.numel() else 0.0), what)


def check_exact(got, ref, what=""):
    """``got`` (fp32 or integer, any device) equals the fp64 / integer reference cast to its type, bit for bit (torch.equal);
    reports the first differing index."""
    g = got.detach().cpu()
    r = ref.detach().cpu().to(g.dtype)
    assert g.shape == r.shape, (what, tuple(g.shape), tuple(r.shape))
    if not torch.equal(g, r):
        bad = (g != r).nonzero()
        at = tuple(int(i) for i in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.numel()} elements differ; first at {at}: got {g[at].item()!r}, reference {r[at].item()!r}")


# ---- the four loss terms -----------------------------------------------------------------------------------------------------------
def loss_terms64(pred, gt):
    """[B, 4] = (cc, sim, nss, kl) per image in fp64 (differentiable with respect to ``pred``)."""
    s, g = pred.double().flatten(1), gt.double().flatten(1)
    ms, mg = s.mean(1, keepdim=True), g.mean(1, keepdim=True)
    sd_s, sd_g = s.std(1, keepdim=True), g.std(1, keepdim=True)              # torch.std: unbiased
    a, b = (s - ms) / sd_s, (g - mg) / sd_g
    cc = (a * b).sum(1) / ((a * a).sum(1) * (b * b).sum(1)).sqrt()
    nss = (((s - ms) / (sd_s + EPS)) * g).sum(1) / g.sum(1)
    sk, gk = s / s.sum(1, keepdim=True), g / g.sum(1, keepdim=True)
    kl = (gk * torch.log(EPS + gk / (sk + EPS))).sum(1)

    def minmax_sum(x):
        x = (x - x.min(1, keepdim=True)[0]) / (x.max(1, keepdim=True)[0] - x.min(1, keepdim=True)[0])
        return x / x.sum(1, keepdim=True)

    sim = torch.minimum(minmax_sum(s), minmax_sum(g)).sum(1)
    return torch.stack([cc, sim, nss, kl], 1)


def loss_grad64(pred, gt, w4, flip=False):
    """d((terms.mean(0) * w4).sum()) / d pred in fp64, in pred's shape.  ``flip``: the same sums over the pixels in reverse order (a
    second summation order, to tell the reference's own spread from a kernel's error; it moves the arg-min spike to the LAST minimum)."""
    p = pred.detach().double().flatten(1)
    g = gt.detach().double().flatten(1)
    if flip:
        p, g = p.flip(1), g.flip(1)
    p = p.contiguous().requires_grad_(True)
    (loss_terms64(p, g).mean(0) * torch.as_tensor(w4).double()).sum().backward()
    d = p.grad.flip(1) if flip else p.grad
    return d.reshape(pred.shape)


def loss_grad_closed64(pred, gt, w4, *, spike=True, last_min=False, biased_std=False):
    """The closed forms of metric_bwd_kernel (csrc/metrics.hip) in fp64 with centred sums.  The keyword switches make it wrong on
    purpose: no arg-min spike, the spike on the last minimum, NSS with the biased standard deviation."""
    s, g = pred.detach().double().flatten(1), gt.detach().double().flatten(1)
    B, n = s.shape
    w = torch.as_tensor(w4).double() / B
    S, G = s.sum(1, keepdim=True), g.sum(1, keepdim=True)
    mu_s, mu_g = S / n, G / n
    ds, dg = s - mu_s, g - mu_g
    css, cgg, csg = (ds * ds).sum(1, keepdim=True), (dg * dg).sum(1, keepdim=True), (ds * dg).sum(1, keepdim=True)
    cc = csg / (css * cgg).sqrt()
    out = w[0] * (dg / (css * cgg).sqrt() - cc * ds / css)
    sigma = (css / (n if biased_std else n - 1)).sqrt()
    A = (ds * g).sum(1, keepdim=True)
    out = out + w[2] * ((g - G / n) / ((sigma + EPS) * G) - A * ds / ((n if biased_std else n - 1) * sigma * (sigma + EPS) ** 2 * G))
    sk, gk = s / S, g / G
    ak = -gk * gk / ((sk + EPS) ** 2 * (EPS + gk / (sk + EPS)))
    out = out + w[3] * (ak - (ak * sk).sum(1, keepdim=True)) / S
    mn = s.min(1, keepdim=True)[0]
    gmn, gmx = g.min(1, keepdim=True)[0], g.max(1, keepdim=True)[0]
    U = S - n * mn
    st = (s - mn) / U
    gn = (g - gmn) / (gmx - gmn)
    gt_ = gn / gn.sum(1, keepdim=True)
    c = torch.where(st < gt_, 1.0, torch.where(st == gt_, 0.5, 0.0)).double()
    P, Cs = (c * st).sum(1, keepdim=True), c.sum(1, keepdim=True)
    d_sim = (c - P) / U
    if spike:
        is_min = s == mn
        pos = torch.arange(n).expand(B, n)
        at = torch.where(is_min, pos, torch.full_like(pos, -1 if last_min else n))
        at = at.max(1)[0] if last_min else at.min(1)[0]
        d_sim[torch.arange(B), at] -= ((Cs - n * P) / U).squeeze(1)
    out = out + w[1] * d_sim
    return out.reshape(pred.shape)


def first_min_is_where_torch_puts_it():
    """torch.min(dim) on the CPU returns the FIRST of equal minima -- the index csrc/metrics.hip documents for the SIM spike."""
    return int(torch.tensor([[3.0, 1.0, 2.0, 1.0, 1.0]]).min(1)[1]) == 1


# pred in (0, 1], gt >= 0 with a positive sum; both fp32 (the fp64 reference sees exactly these values)
def _u(g, B, n):
    return 1.0 - torch.rand(B, n, generator=g)                               # (0, 1]


def _sparse_gt(g, B, n):
    gt = (torch.rand(B, n, generator=g) > 0.9).float() + 0.01 * torch.rand(B, n, generator=g)
    gt[:, 0] += 1.0                                                          # a fixation in every image, also at n = 3
    return gt


def _binary_gt(g, B, n):
    gt = (torch.rand(B, n, generator=g) > 0.9).float()
    gt[:, n // 2] = 1.0
    gt[:, 0] = 0.0                                                           # min exactly 0, sum > 0
    return gt


def loss_inputs(family, B, n, seed=0):
    """(pred, gt) fp32 [B, n] of one family."""
    g = generator(1000 + seed + 7 * n + B)
    if family == "uniform":
        return _u(g, B, n), _sparse_gt(g, B, n)
    if family == "binary":
        return _u(g, B, n), _binary_gt(g, B, n)
    if family == "eighths":                                                  # the minimum 1/8 is attained ~ n / 8 times
        return torch.ceil(_u(g, B, n) * 8) / 8, _sparse_gt(g, B, n)
    if family == "zeros":                                                    # exact zeros of pred only where gt is zero too
        pred, gt = _u(g, B, n), _binary_gt(g, B, n)
        drop = (gt == 0) & (torch.rand(B, n, generator=g) < 0.3)
        drop[:, 0] = True
        return torch.where(drop, torch.zeros_like(pred), pred), gt
    if family == "flat":                                                     # 0.5 + 1e-3 u; fp32 has ~16000 values there, so the unique
        pred = (0.5 + 1e-3 * _u(g, B, n)).clamp_min(0.5 + 2.0 ** -23)        # minimum is placed: exactly 0.5 at one pixel
        pred[:, n // 3] = 0.5
        return pred, _sparse_gt(g, B, n)
    if family == "scale100":                                                 # image b: pred / 100^b, gt * 100^b
        k = (100.0 ** torch.arange(B, dtype=torch.float64))[:, None]
        return (_u(g, B, n).double() / k).float(), (_sparse_gt(g, B, n).double() * k).float()
    if family == "identical":                                                # forward only: image 1 has pred == gt
        pred, gt = _u(g, B, n), _sparse_gt(g, B, n)
        gt[1] = pred[1]
        return pred, gt
    raise KeyError(family)


LOSS_SHAPES = [(1, 3), (2, 5), (3, 63), (2, 64), (2, 65), (1, 257), (2, 1000), (3, 16385)]      # n < / = / > the 64 chunks, B = 1
LOSS_FAMILIES = ("uniform", "binary", "eighths", "zeros", "flat", "scale100")
FAMILY_SHAPES = [(2, 300), (3, 16385)]
DUPLICATED_MIN = ("eighths", "zeros")                                        # every other case needs a unique minimum of pred
LOSS_CASES = [("uniform", B, n) for B, n in LOSS_SHAPES] + [(f, B, n) for f in LOSS_FAMILIES for B, n in FAMILY_SHAPES]
FORWARD_ONLY_CASES = [("identical", 3, 300), ("identical", 2, 16385)]
UPSTREAM = -300.0
UNIT_W4 = [tuple(f if i == k else 0.0 for i in range(4)) for k in range(4) for f in (1.0, UPSTREAM)]
MIXED_W4 = (-0.7, -0.4, -0.05, 1.3)                                          # (cc, sim, nss, kl): the weight mix of the 'all' fixture
LOSS_REL = 2.0 ** -22                                                        # fp64 arithmetic, ONE rounding to fp32 (2^-24), two ulp of room


def case_id(c):
    """pytest id of a case tuple: fields joined by '-', nested sizes by 'x'."""
    return "-".join("x".join(case_id(u) if isinstance(u, (tuple, list)) else str(u) for u in v) if isinstance(v, (tuple, list))
                    else str(v) for v in c)


def hw_of(n):
    """(h, w) with h * w = n, h the largest divisor up to sqrt(n)."""
    h = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return h, n // h


def loss_floor(pred):
    """The absolute part of the bound, in units of max|ref|: 1e-9, or the cancellation of the one-pass variance sum s^2 - n mu^2
    (relative error (mean^2 / var) * 2^-53 per sum; 2^-48 leaves room for the 64-chunk sums and for var's use in a quotient)."""
    p = pred.double().flatten(1)
    return max(1e-9, float((p.mean(1) ** 2 / p.var(1, unbiased=False)).max()) * 2.0 ** -48)


def minima_mask(pred):
    p = pred.flatten(1)
    return (p == p.min(1, keepdim=True)[0]).reshape(pred.shape)


def check_loss_grad(got, ref, pred, rel, floor, what=""):
    """The gradient comparison of the GPU file: every pixel that is not a minimum of pred elementwise; the SUM over the minima; and
    the minima elementwise (the spike sits on the FIRST one).  -> worst ratio."""
    got, ref = got.detach().double().cpu().reshape(pred.shape), ref.detach().double().cpu().reshape(pred.shape)
    tol = rel * ref.abs() + floor * float(ref.abs().max())
    mins = minima_mask(pred)
    w = check_bound(got[~mins], ref[~mins], tol[~mins], what + " (pixels off the minimum)")
    B = pred.shape[0]
    m = mins.reshape(B, -1).double()
    w = max(w, check_bound((got.reshape(B, -1) * m).sum(1), (ref.reshape(B, -1) * m).sum(1), (tol.reshape(B, -1) * m).sum(1),
                           what + " (sum over the minima)"))
    return max(w, check_bound(got[mins], ref[mins], tol[mins], what + " (spike on the first minimum)"))


# ---- relative-position projection ----------------------------------------------------------------------------------------------------
RELPOS_CASES = [
    # q_size, k_size, E, BH, D
    ((1, 1, 1), (1, 1, 1), 32, 1, 96),          # one query, 31 empty chunks
    ((3, 5, 7), (3, 5, 7), 32, 3, 96),          # odd key counts, chunk edges mid-row
    ((8, 7, 12), (8, 7, 12), 32, 2, 96),        # full t slot
    ((2, 8, 16), (2, 8, 16), 32, 1, 96),        # full h and w slots
    ((2, 14, 24), (2, 14, 24), 48, 1, 96),      # E = 48 near full
    ((1, 16, 24), (1, 16, 24), 48, 1, 96),      # E = 48 full
    ((2, 5, 7), (2, 3, 4), 32, 4, 64),          # generic-D kernels
    ((2, 5, 7), (2, 3, 4), 48, 4, 64),
    ((2, 3, 4), (2, 3, 12), 32, 2, 512),        # two passes of the table kernel's item loop (3 column quads * 128 channel quads > 256)
]


def slot_offsets(E):
    return 0, 8, (16 if E == 32 else 24)


def relpos_operands(case, seed=0):
    """Integer operands in [-4, 4] as fp64: q [1, BH, 1 + L, D], (Rt, Rh, Rw), the upstream gradient of extra [1, BH, 1 + L, E] and
    a tensor to accumulate dq into."""
    q_size, k_size, E, BH, D = case
    g = generator(300 + seed + D + BH)
    L = q_size[0] * q_size[1] * q_size[2]
    q = ints(g, (1, BH, 1 + L, D))
    Rs = [ints(g, (a, b, D)) for a, b in zip(q_size, k_size)]
    dE = ints(g, (1, BH, 1 + L, E))
    acc = ints(g, (1, BH, 1 + L, D))
    return q, Rs, dE, acc


def relpos_extra64(q, Rs, q_size, k_size, E, swap_hw=False):
    """extra [B, H, 1 + L, E]: slots t [0, kt), h [8, 8 + kh), w [w0, w0 + kw); class-token row and unused slots zero.
    ``swap_hw``: the h and w products land at each other's slot offset (wrong on purpose)."""
    B, H, N, D = q.shape
    t0, h0, w0 = slot_offsets(E)
    if swap_hw:
        h0, w0 = w0, h0
    rq = q[:, :, 1:].reshape(B, H, *q_size, D)
    parts = [torch.einsum("bythwc,tkc->bythwk", rq, Rs[0]), torch.einsum("bythwc,hkc->bythwk", rq, Rs[1]),
             torch.einsum("bythwc,wkc->bythwk", rq, Rs[2])]
    ex = torch.zeros(B, H, N, E + 24, dtype=q.dtype)                        # room for a swapped layout; cut back to E below
    for p, o, k in zip(parts, (t0, h0, w0), k_size):
        ex[:, :, 1:, o:o + k] = ex[:, :, 1:, o:o + k] + p.reshape(B, H, N - 1, k)
    return ex[..., :E]


def relpos_bwd64(q, Rs, dE, q_size, k_size, E, dq_accum=None, overwrite=False, swap_hw=False):
    """(dq, dRt, dRh, dRw) of sum(extra * dE) by fp64 autograd of the einsum form; dq is added to ``dq_accum`` when given
    (``overwrite``: it replaces it -- wrong on purpose)."""
    ql = q.detach().clone().requires_grad_(True)
    Rl = [r.detach().clone().requires_grad_(True) for r in Rs]
    (relpos_extra64(ql, Rl, q_size, k_size, E, swap_hw) * dE).sum().backward()
    dq = ql.grad if (dq_accum is None or overwrite) else dq_accum + ql.grad
    return dq, Rl[0].grad, Rl[1].grad, Rl[2].grad


def relpos_sum_bound(case, r=4):
    """The largest |partial sum| any of the three kernels can form with operands in [-r, r] (the accumulated dq included)."""
    q_size, k_size, E, BH, D = case
    L = q_size[0] * q_size[1] * q_size[2]
    per_axis = [BH * L // a for a in q_size]                                 # queries that share a coordinate
    return max(D * r * r, sum(k_size) * r * r + r, max(per_axis) * r * r)


ATTENTION_CASES = [(2, 2, (2, 5, 7), (2, 3, 4)), (1, 1, (2, 6, 10), (2, 3, 5))]      # B, H, q_size, k_size


# ---- relative-position tables ------------------------------------------------------------------------------------------------------
REL_GEOMS = [(15, 8, 8), (27, 14, 7), (13, 7, 7), (111, 56, 7)]                      # (table length, q, k) per axis
# every table above has the length of its grid (2 max(q, k) - 1): one tap of weight 1.  The mixed block adds a table resampled up
# (27 rows for a grid that wants 47) and one resampled down (111 for 55): two taps with fractional weights, three row counts in a launch
REL_MIXED = ((15, 8, 8), (27, 24, 12), (111, 28, 7))
REL_BLOCKS = [(g, g, g) for g in REL_GEOMS] + [REL_MIXED]
REL_DS = (96, 4)


def rel_plan(rel_len, q, k, dev="cpu"):
    """MViT._rel_plan without building an encoder (the method only needs a cache to write to)."""
    from diff_sal_amd.mvit import MViT

    return MViT._rel_plan(types.SimpleNamespace(_const_tables={}), rel_len, q, k, dev)


def rel_table64(rel, pl):
    """-> (gathered table [q, k, D] in fp64, its elementwise bound 2^-22 (|w0 a| + |w1 b|): two products and a sum in fp32)."""
    i2, w2 = pl["idx2"].long().cpu(), pl["w2"].double().cpu()
    r = rel.double().cpu()
    a, b = w2[:, :1] * r[i2[:, 0]], w2[:, 1:] * r[i2[:, 1]]
    shape = (pl["q"], pl["k"], r.shape[1])
    return (a + b).view(shape), (2.0 ** -22 * (a.abs() + b.abs())).view(shape)


def rel_table_bwd64(dout, pl, drop_row=None):
    """-> (drel [len, D] = the CSR sum in fp64, its bound nnz_row 2^-24 sum |w| |g|: an fmaf chain of nnz_row terms).
    ``drop_row``: that table row gets nothing (wrong on purpose)."""
    ptr, col, w = pl["csr_ptr"].long().cpu(), pl["csr_col"].long().cpu(), pl["csr_w"].double().cpu()
    flat = dout.double().cpu().reshape(-1, dout.shape[-1])
    row = torch.repeat_interleave(torch.arange(pl["len"]), ptr[1:] - ptr[:-1])
    if drop_row is not None:
        w = torch.where(row == drop_row, torch.zeros_like(w), w)
    d = torch.zeros(pl["len"], flat.shape[1], dtype=torch.float64).index_add_(0, row, w[:, None] * flat[col])
    mag = torch.zeros_like(d).index_add_(0, row, w.abs()[:, None] * flat[col].abs())
    return d, (ptr[1:] - ptr[:-1]).double()[:, None] * 2.0 ** -24 * mag


# ---- max-pool with arg-max ---------------------------------------------------------------------------------------------------------
MAXPOOL_CASES = [((2, 6, 9), (1, 3, 3), (1, 2, 2)), ((3, 5, 7), (3, 3, 3), (1, 1, 1)), ((2, 4, 4), (1, 3, 3), (1, 1, 1))]
MAXPOOL_CS = (4, 64, 96)


def maxpool_operands(case, C, negative=False, seed=0, B=2):
    """x [B, 1 + T*H*W, C] drawn from {0, 1, 2} (``negative``: from {-3, -2, -1}) and an integer dy, fp32."""
    size, kernel, stride = case
    g = generator(500 + seed + C)
    x = torch.randint(0, 3, (B, 1 + size[0] * size[1] * size[2], C), generator=g).float() - (3.0 if negative else 0.0)
    out_size = [(s + 2 * (k // 2) - k) // st + 1 for s, k, st in zip(size, kernel, stride)]
    dy = ints(g, (B, 1 + out_size[0] * out_size[1] * out_size[2], C)).float()
    return x, dy


def maxpool_ref(x, case, last=False):
    """(out, idx) of the token max-pool by a walk over the window positions in (t, y, x) order: a later position replaces the
    maximum only if it is greater (``last``: if it is greater OR EQUAL -- the tie rule torch does not have).  idx = 1-based input
    token, 0 for the class token."""
    size, kernel, stride = case
    B, N, C = x.shape
    T, H, W = size
    pad = [k // 2 for k in kernel]
    To, Ho, Wo = [(s + 2 * p - k) // st + 1 for s, p, k, st in zip(size, pad, kernel, stride)]
    v = x[:, 1:].reshape(B, T, H, W, C).double()
    tok = (1 + torch.arange(T * H * W)).reshape(1, T, H, W, 1).expand(B, T, H, W, C)
    vp = F.pad(v, (0, 0, pad[2], pad[2], pad[1], pad[1], pad[0], pad[0]), value=float("-inf"))
    tp = F.pad(tok, (0, 0, pad[2], pad[2], pad[1], pad[1], pad[0], pad[0]), value=0)
    best = torch.full((B, To, Ho, Wo, C), float("-inf"), dtype=torch.float64)
    arg = torch.zeros((B, To, Ho, Wo, C), dtype=torch.long)
    for a in range(kernel[0]):
        for e in range(kernel[1]):
            for f in range(kernel[2]):
                sl = (slice(None), slice(a, a + (To - 1) * stride[0] + 1, stride[0]), slice(e, e + (Ho - 1) * stride[1] + 1, stride[1]),
                      slice(f, f + (Wo - 1) * stride[2] + 1, stride[2]))
                cand, ct = vp[sl], tp[sl]
                take = (cand >= best) if last else (cand > best)
                take = take & (cand > float("-inf"))
                best, arg = torch.where(take, cand, best), torch.where(take, ct, arg)
    out = torch.cat([x[:, :1].double(), best.reshape(B, -1, C)], 1).float()
    idx = torch.cat([torch.zeros(B, 1, C, dtype=torch.long), arg.reshape(B, -1, C)], 1).int()
    return out, idx


def maxpool_torch(x, case, dy=None):
    """F.max_pool3d on the CPU: (out, idx as above[, dx by autograd])."""
    size, kernel, stride = case
    B, N, C = x.shape
    xl = x.detach().clone().requires_grad_(dy is not None)
    t = xl[:, 1:].reshape(B, *size, C).permute(0, 4, 1, 2, 3)
    o, i = F.max_pool3d(t, kernel, stride, tuple(k // 2 for k in kernel), return_indices=True)
    out = torch.cat([xl[:, :1], o.reshape(B, C, -1).transpose(1, 2)], 1)
    idx = torch.cat([torch.zeros(B, 1, C, dtype=torch.long), 1 + i.reshape(B, C, -1).transpose(1, 2)], 1).int()
    if dy is None:
        return out.detach(), idx
    out.backward(dy)
    return out.detach(), idx, xl.grad


def maxpool_bwd_from_idx(dy, idx, n_in):
    """dx [B, n_in, C]: every output's gradient goes to the token its idx names (class token: row 0)."""
    return torch.zeros(dy.shape[0], n_in, dy.shape[2], dtype=dy.dtype).scatter_add_(1, idx.long(), dy)


def maxpool_tie_share(x, case):
    """Share of the windows (class-token row excluded) in which the maximum is attained more than once."""
    _, first = maxpool_ref(x, case)
    _, last = maxpool_ref(x, case, last=True)
    return float((first[:, 1:] != last[:, 1:]).double().mean())


# ---- token transposes --------------------------------------------------------------------------------------------------------------
TRANSPOSE_LS = (1, 63, 64, 65, 130)                                          # the kernel works on 64 x 64 tiles with edge guards
TRANSPOSE_CS = (4, 64, 65, 96)
TRANSPOSE_CASES = [(L, C, off) for L in TRANSPOSE_LS for C in TRANSPOSE_CS for off in (0, 1)]


def transpose_operands(L, C, off, B=2, seed=0):
    g = generator(700 + seed + 131 * L + C + off)
    return ints(g, (B, off + L, C)).float(), ints(g, (B, C, L)).float()


def channels_first_ref(x, off, ignore_off=False):
    """[B, off + L, C] -> [B, C, L] (``ignore_off``: rows 0 .. L instead of off .. off + L -- wrong on purpose)."""
    L = x.shape[1] - off
    return (x[:, :L] if ignore_off else x[:, off:]).transpose(1, 2).contiguous()


def channels_first_bwd_ref(dy, off):
    """[B, C, L] -> [B, off + L, C], the rows below ``off`` zero."""
    return F.pad(dy.transpose(1, 2), (0, 0, off, 0)).contiguous()


# ---- pooling convolutions outside the fused D = 96 path ------------------------------------------------------------------------------
QKVPOOL_CASE = dict(B=2, heads=2, D=64, size=(3, 5, 6), stride_q=(1, 2, 2), stride_kv=(1, 1, 1))


def qkv_pool64(qkv, ws, size, strides):
    """The three depthwise Conv3d(3x3x3, padding 1) of attention_pool on qkv [B, N, 3, heads, D] in fp64 (class token passed through)."""
    B, N, _, heads, D = qkv.shape
    outs = []
    for i in range(3):
        x = qkv[:, :, i].permute(0, 2, 1, 3)
        t = x[:, :, 1:].reshape(B * heads, *size, D).permute(0, 4, 1, 2, 3)
        t = F.conv3d(t, ws[i], None, stride=strides[i], padding=1, groups=D)
        outs.append(torch.cat([x[:, :, :1], t.reshape(B, heads, D, -1).transpose(2, 3)], 2))
    return outs


# ---- gradient gather (csrc/optim.hip) --------------------------------------------------------------------------------------------------
COPY_SIZES = (1, 3, 4, 5, 1023, 70001)                                       # vector body, tail of 1 to 3, nothing but a tail
COPY_COUNTS = (1, 48, 49, 100)                                               # the pointer table holds 48 sources per launch
SENTINEL = -12345.0


def copy_plan(count):
    """[(size, misaligned)] for ``count`` sources: the sizes in turn, each once 16-byte aligned and once as t[1:] (4 bytes off: the
    scalar path), and the destination offsets: multiples of 64 elements with a gap after every slot."""
    plan = [(COPY_SIZES[(i // 2) % len(COPY_SIZES)], i % 2 == 1) for i in range(count)]
    offs, o = [], 64
    for n, _ in plan:
        offs.append(o)
        o += (n + 63) // 64 * 64 + 64
    return plan, offs, o
