"""Exact-operand references for the matrix kernels.

With small-integer operands every product and every partial sum of a GEMM / convolution is an integer below 2^24, so an fp32
accumulator holds it exactly in ANY summation order (tile shape, K split, slab sums, DMA ring depth).  The only rounding left is the
one store to the storage type: one fp64 reference per problem has to be matched bit for bit by every route, and sums lifted above
2^8 (bf16) / 2^11 (fp16) land on rounding ties all the time -- truncation, ties-away and a lost or doubled k term all show.

This module holds, for tests/test_exact_ref_host.py (no GPU) and tests/test_gpu_exact_products.py:
  * the operand generators (seeded ``torch.Generator``, integers in [-r, r], scale in {0.5, 1, 2}, a lifting bias for 16-bit storage);
  * the fp64 references with the library's epilogue order  relu((conv + bias) * scale + shift + rowvec) + residual  and one rounding;
  * the conditions that make the comparison exact (``conditions``) and the power of a case (``tie_shares``);
  * ``check_equal`` and the case tables of the GPU file.
"""
import dataclasses
import functools
import re

import torch
import torch.nn.functional as F

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
BOTH16 = ("bf16", "fp16")
SIG_BITS = {"bf16": 8, "fp16": 11}          # significand bits, hidden one included: integers up to 2^SIG_BITS are exact
FP16_MAX = 65504.0
LIMIT = float(2 ** 24)                      # integers below are exact in fp32, and so is every sum of them that stays below
FULL = ("bias", "bn", "rowvec", "relu", "res")


# ---- operands ----------------------------------------------------------------------------------------------------------------------
def generator(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def ints(g, shape, r=4):
    """Integers uniform in [-r, r] as fp64."""
    return torch.randint(-r, r + 1, tuple(shape), generator=g).double()


def scales(g, n):
    """Per-channel scale from {0.5, 1, 2}: a power of two never rounds."""
    return torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (n,), generator=g)]


def lift(g, n, dname, binades=4):
    """Odd integers of either sign, their binade uniform among the ``binades`` binades from 2^SIG_BITS on ([256, 4096) for bf16,
    [2048, 32768) for fp16 with four): as an fp32 bias it is free of rounding and carries the sums to where the storage type has a
    spacing of 2 .. 2^binades, so that a share of 1/2 .. 2^-binades of the integers are ties."""
    lo = 2.0 ** (SIG_BITS[dname] + torch.randint(0, binades, (n,), generator=g).double())
    mag = torch.floor(lo + torch.rand(n, generator=g, dtype=torch.float64) * lo)
    mag = torch.where(mag % 2 == 0, mag + 1, mag)
    sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return sign * mag


def to_storage(t, dname):
    """``t`` (fp32 / fp64, on any device) in the storage type; the values must survive the conversion."""
    out = t.to(DTYPES[dname])
    assert torch.equal(out.double(), t.double()), f"operand is not representable in {dname}"
    return out


def pack_k_order(w):
    """[Cout, Cin, KH, KW] -> [Cout, K] with k ordered (ci // 32, tap, ci % 32), Cin a multiple of 32: the packed layout of
    include/diffsal.h, written out here so that the references do not depend on the library's pack kernel."""
    Cout, Cin, kh, kw = w.shape
    if Cin % 32:
        return w.permute(0, 2, 3, 1).reshape(Cout, kh * kw * Cin).contiguous()
    return w.reshape(Cout, Cin // 32, 32, kh * kw).permute(0, 1, 3, 2).reshape(Cout, kh * kw * Cin).contiguous()


# ---- rounding analysis -------------------------------------------------------------------------------------------------------------
def _ulp(v, dname):
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -14))        # |v| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v), e - SIG_BITS[dname])


def tie_shares(exact, dname):
    """(share of values that are rounding ties in the storage type, share that is not representable at all)."""
    q = (exact / _ulp(exact, dname)).abs()
    frac = q - q.floor()
    return (frac == 0.5).double().mean().item(), (frac != 0).double().mean().item()


def is_tie(exact, dname):
    q = (exact / _ulp(exact, dname)).abs()
    return (q - q.floor()) == 0.5


def round_store(exact, dname):
    """The one rounding of the store (round to nearest even); fp32 storage holds the exact value."""
    out = exact.to(DTYPES[dname])
    if dname == "fp32":
        assert torch.equal(out.double(), exact), "an fp32 case must not round at all"
    return out


def truncate_store(exact, dname):
    """MUTATION: the store chops the low bits instead of rounding to nearest even."""
    u = _ulp(exact, dname)
    return (torch.sign(exact) * (exact.abs() / u).floor() * u).to(DTYPES[dname])


# ---- problems ----------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Conv:
    """A convolution / plain product (xshape = (1, 1, M, K), k = 1) with its epilogue.  epi: subset of FULL; a 16-bit problem gets the
    lifting vector (``lift``, of ``binades`` binades) as its bias, or without one as its shift."""
    dname: str
    xshape: tuple           # N, H, W, Cin
    Cout: int
    k: int = 1
    stride: int = 1
    pad: int = 0
    dil: int = 1
    out_hw: tuple = None
    epi: tuple = ("bias",)
    r: int = 4
    binades: int = 4
    seed: int = 0

    @property
    def K(self):
        return self.k * self.k * self.xshape[3]

    def hw(self):
        if self.out_hw is not None:
            return tuple(self.out_hw)
        N, H, W, _ = self.xshape
        f = lambda n: (n + 2 * self.pad - self.dil * (self.k - 1) - 1) // self.stride + 1
        return f(H), f(W)

    def geometry(self):
        return (self.xshape, self.Cout, self.k, self.stride, self.pad, self.dil, self.hw(), self.r, self.seed)


def _conv64(x, w, c):
    """fp64 / fp32 convolution of NHWC x with [Cout, Cin, k, k] w, bottom / right padding implied by the output size -> NHWC."""
    N, H, W, _ = c.xshape
    Ho, Wo = c.hw()
    pb = (Ho - 1) * c.stride + c.dil * (c.k - 1) + 1 - H - c.pad
    pr = (Wo - 1) * c.stride + c.dil * (c.k - 1) + 1 - W - c.pad
    xp = F.pad(x.permute(0, 3, 1, 2), (c.pad, max(pr, 0), c.pad, max(pb, 0)))
    y = F.conv2d(xp, w, None, stride=c.stride, dilation=c.dil)
    return y[:, :, :Ho, :Wo].permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _operands(geom):
    """x, w and the fp64 sums of one geometry (shared by its storage types and epilogues, never changed afterwards)."""
    xshape, Cout, k, stride, pad, dil, hw, r, seed = geom
    c = Conv("fp32", xshape, Cout, k, stride, pad, dil, hw, r=r, seed=seed)
    g = generator(1000 + seed)
    x = ints(g, xshape, r)
    w = ints(g, (Cout, xshape[3], k, k), r)
    acc = _conv64(x, w, c)
    absacc = _conv64(x.abs(), w.abs(), c)
    return x, w, acc, absacc


def epilogue(acc, p):
    """The library's order on the accumulator (tests/test_gpu_lowp.py::test_conv_igemm_16bit_epilogue), in acc's own precision."""
    t = lambda v: None if v is None else v.to(acc.dtype)
    v = acc
    if p.bias is not None:
        v = v + t(p.bias)
    if p.scale is not None:
        v = v * t(p.scale) + t(p.shift)
    if p.rowvec is not None:
        v = v + t(p.rowvec)[:, None, None, :]
    if p.relu:
        v = torch.relu(v)
    if p.residual is not None:
        v = v + t(p.residual)
    return v


class Problem:
    pass


@functools.lru_cache(maxsize=None)
def problem(c):
    """Operands (fp64 integers), exact result and rounded reference of one ``Conv``."""
    p = Problem()
    p.spec = c
    p.x, p.w, p.acc, p.absacc = _operands(c.geometry())
    g = generator(2000 + c.seed + 7 * len(c.epi))
    N, Cout = c.xshape[0], c.Cout
    p.bias = p.scale = p.shift = p.rowvec = p.residual = None
    if "bias" in c.epi:
        p.bias = lift(g, Cout, c.dname, c.binades) if c.dname != "fp32" else ints(g, (Cout,), 64)
    if "bn" in c.epi:
        p.scale, p.shift = scales(g, Cout), ints(g, (Cout,), c.r)
        if c.dname != "fp32" and "bias" not in c.epi:       # no bias to lift the sums: the shift does it
            p.shift = lift(g, Cout, c.dname, c.binades)
    if "rowvec" in c.epi:
        p.rowvec = ints(g, (N, Cout), c.r)
    p.relu = "relu" in c.epi
    if "res" in c.epi:
        p.residual = ints(g, (N, *c.hw(), Cout), c.r)
        to_storage(p.residual, c.dname)
    p.exact = epilogue(p.acc, p)
    p.ref = round_store(p.exact, c.dname)
    return p


def magnitude_bound(p):
    """Condition (a): the largest value any summation order can meet on the way to an output, in units of the finest grid the values
    live on (1, or 1/2 once a scale of 0.5 applies): below 2^24 every fp32 operation on the way is exact."""
    b = p.absacc
    if p.bias is not None:
        b = b + p.bias.abs()
    unit = 1.0
    if p.scale is not None:
        b = b * p.scale.abs() + p.shift.abs()
        unit = 0.5
    if p.rowvec is not None:
        b = b + p.rowvec.abs()[:, None, None, :]
    if p.residual is not None:
        b = b + p.residual.abs()
    return b.max().item() / unit


def conditions(exact, bound, dname, what):
    """Conditions (a) - (c) of a case from its exact values and magnitude bound; returns (tie share, inexact share)."""
    assert bound < LIMIT, f"{what}: magnitude bound {bound:.3g} is not below 2^24"
    if dname == "fp32":
        return 0.0, 0.0
    if dname == "fp16":
        assert exact.abs().max().item() <= FP16_MAX, f"{what}: {exact.abs().max().item()} overflows fp16"
    ties, inexact = tie_shares(exact, dname)
    assert ties >= 0.02, f"{what}: only {ties:.2%} of the outputs are rounding ties"
    assert inexact >= 0.10, f"{what}: only {inexact:.2%} of the outputs need rounding"
    return ties, inexact


def check_equal(got, ref, what, exact=None, dname=None):
    """Bit equality of ``got`` with ``ref``; prints the case's power, and on failure says where the mismatches sit."""
    got = got.detach().cpu().reshape(ref.shape)
    assert got.dtype == ref.dtype, (what, got.dtype, ref.dtype)
    if exact is not None and dname in SIG_BITS:
        t, i = tie_shares(exact, dname)
        print(f"  {what}: {t:.1%} ties, {i:.1%} inexact")
    else:
        print(f"  {what}: no rounding (exact in {ref.dtype})")
    if torch.equal(got, ref):
        return
    bad = (got != ref) | (got.isnan() != ref.isnan())
    idx = bad.nonzero()
    lines = [f"{what}: {int(bad.sum())} of {bad.numel()} outputs differ"]
    for ix in idx[:8].tolist():
        ix = tuple(ix)
        e = "" if exact is None else f", exact {exact[ix].item()!r}"
        lines.append(f"  {ix}: got {got[ix].item()!r}, ref {ref[ix].item()!r}{e}")
    lo, hi = idx.min(0).values.tolist(), idx.max(0).values.tolist()
    lines.append(f"  index range {lo} .. {hi}")
    if exact is not None and dname in SIG_BITS:
        on = is_tie(exact, dname)[bad].double().mean().item()
        lines.append(f"  {on:.1%} of the mismatches sit on rounding ties" + (" (ties only: the rounding mode)" if on == 1.0 else ""))
    raise AssertionError("\n".join(lines))


# ---- case tables -------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Route:
    id: str
    spec: Conv
    switches: tuple          # ((name without DIFFSAL_, value), ...)
    kernel: str              # regex on diffsal_last_gemm_kernel()


def _sw(d):
    return tuple(sorted(d.items()))


def _epi16(dname, epi, K):
    """16-bit storage: a case always needs sums where the storage type rounds.  With a bias the lifting bias does it, else the shift
    of the BN affine; a table entry with neither keeps its epilogue and gets larger operands instead (sum ~ r^2 sqrt(K) / 3)."""
    if dname == "fp32" or "bias" in epi or "bn" in epi:
        return dict(epi=tuple(epi))
    return dict(epi=tuple(epi), r=16 if K < 2000 else 12)


def route_rows():
    """Every row of ROWS in tests/test_gpu_conv_routes.py in each storage type it lists: with a bias, as there, and with the kernel's
    full epilogue (lin_stream's is bias, activation, residual: anything more sends the launch to the tiled kernel)."""
    from tests.test_gpu_conv_routes import ROWS

    out = []
    for i, (rid, dnames, xshape, Cout, k, stride, pad, out_hw, sw, kernel, _) in enumerate(ROWS):
        for dname in dnames:
            for tag, epi in (("bias", ("bias",)), ("full", ("bias", "relu", "res") if rid == "lin_stream" else FULL)):
                # a scale of 2 on [2048, 32768) would leave fp16: three binades under the full epilogue
                spec = Conv(dname, xshape, Cout, k, stride, pad, 1, out_hw, epi=epi, binades=3 if tag == "full" else 4, seed=i)
                out.append(Route(f"{rid}-{dname}-{tag}", spec, _sw(sw), kernel))
    return out


IGEMM_CFGS = [None, 0, 1, 2, 3, 4, 5]
IGEMM_SHAPES = [(130, 96, 100), (777, 384, 96)]
# tile shapes of csrc/igemm.hip's launch<WM, WN, TM, TN> by configuration
IGEMM_TEMPLATES = {0: "2, 2, 2, 3", 1: "2, 2, 2, 2", 2: "4, 1, 1, 3", 3: "2, 2, 1, 2", 4: "2, 2, 2, 1", 5: "2, 2, 1, 1"}


def igemm_cfg_routes():
    """DIFFSAL_IGEMM_CFG None and 0..5 x DIFFSAL_NO_PERSIST 0 / 1 on fp32 (tests/test_gpu_ops.py::test_persistent_linear_kernel_fp32);
    bias, ReLU and residual -- what ops.linear passes."""
    out = []
    for cfg in IGEMM_CFGS:
        for M, K, N in IGEMM_SHAPES:
            for nop in (0, 1):
                sw = {"GEMM_DMA": 0, "NO_PERSIST": nop}
                if cfg is not None:
                    sw["IGEMM_CFG"] = cfg
                # the planner's own choice may split K, which the persistent kernel does not do; a forced tile shape never splits
                name = "igemm_kernel<" if nop else "igemm_linear_kernel<"
                kern = "^" + re.escape(name + IGEMM_TEMPLATES[cfg]) if cfg is not None else ("^igemm_kernel<" if nop else r"^igemm_(linear_)?kernel<")
                spec = Conv("fp32", (1, 1, M, K), N, epi=("bias", "relu", "res"), seed=100 + M)
                out.append(Route(f"igemm-cfg{cfg}-{M}x{K}x{N}-{'onetile' if nop else 'persistent'}", spec, _sw(sw), kern))
    return out


def igemm16_cfg_routes():
    """DIFFSAL_IGEMM16_CFG 0..7 on bf16 and fp16 (tests/test_gpu_lowp.py::test_conv_igemm_16bit_every_tile_shape: no epilogue)."""
    out = []
    for dname in BOTH16:
        for cfg in range(8):
            spec = Conv(dname, (2, 19, 27, 96), 224, 3, 1, 1, **_epi16(dname, (), 864), seed=200)
            out.append(Route(f"igemm16-cfg{cfg}-{dname}", spec, _sw({"IGEMM16_CFG": cfg}), r"^igemm16_kernel<"))
    return out


# tests/test_gpu_stream16.py::CONV_DMA_CASES (N, H, W, Cin, Cout, pad, dil, epilogue) and the three tile settings of its test
CONV16_TILES = [("256x96", 0, 0), ("128x96", 0, 1), ("192x192", 1, 0)]
_EPI_NAMES = {"bn_relu_res": ("bn", "relu", "res"), "bn_relu": ("bn", "relu"), "bias_rowvec": ("bias", "rowvec"), "bias": ("bias",), "none": ()}


def conv16_tile_routes():
    from tests.test_gpu_stream16 import CONV_DMA_CASES

    out = []
    for i, (N, H, W, Cin, Cout, pad, dil, epi) in enumerate(CONV_DMA_CASES):
        for dname in BOTH16:
            spec = Conv(dname, (N, H, W, Cin), Cout, 3, 1, pad, dil, **_epi16(dname, _EPI_NAMES[epi], 9 * Cin), seed=300 + i)
            for tid, tile, half in CONV16_TILES:
                kern = r"^conv16_dma_kernel<.*x 192 channels" if tile == 1 else r"^conv16_dma_kernel<(?!.*x 192 channels)"
                out.append(Route(f"conv16_dma-{tid}-case{i}-{dname}", spec,
                                 _sw({"FORCE_HALO": 2, "CONV16_TILE": tile, "CONV16_HALF": half}), kern))
    return out


# the stride-2 asymmetric-pad, stride-4 and dilation-2 rows of CONV_CASES (tests/test_gpu_ops.py, tests/test_gpu_lowp.py)
STRIDED_CASES = [("stride2-asym", (2, 14, 24, 192), 192, 3, 2, 0, 1, (7, 12)), ("stride4-asym", (1, 30, 46, 96), 96, 3, 4, 0, 1, (8, 12)),
                 ("dilation2", (3, 14, 24, 384), 192, 3, 1, 2, 2, None)]


def strided_routes():
    out = []
    for i, (cid, xshape, Cout, k, s, p, d, hw) in enumerate(STRIDED_CASES):
        for dname in DTYPES:
            spec = Conv(dname, xshape, Cout, k, s, p, d, hw, epi=FULL, binades=3, seed=400 + i)
            # the generic tiled kernel of the storage type, whatever the planner's thresholds for the LDS-DMA and halo forms say
            out.append(Route(f"{cid}-{dname}-full", spec, _sw({"CONV_DMA": 0, "NO_HALO": 1}), r"^igemm_kernel<" if dname == "fp32" else r"^igemm16_kernel<"))
    return out


def forward_routes():
    return route_rows() + igemm_cfg_routes() + igemm16_cfg_routes() + conv16_tile_routes() + strided_routes()


# ---- the remaining forward entry points ---------------------------------------------------------------------------------------------
M_PAIR = 648
PAIR_CASES = [("grouped-dma", "fp32", 768, 1536, {}, r"^gemm_dma_kernel<float, 3, 3, 3, 2, true, true>"),
              ("paired-tiled", "fp32", 384, 768, {}, r"^igemm_kernel<.*pair"),
              ("pair16-bf16", "bf16", 768, 768, {}, r"^igemm16_kernel<.*pair"),
              ("pair16-fp16", "fp16", 768, 768, {}, r"^igemm16_kernel<.*pair")]


def pair_specs(case):
    _, dname, K, N, _, _ = case
    return [Conv(dname, (1, 1, M_PAIR, K), N, seed=500 + i) for i in range(2)]


GROUP_SHAPES = [(648, 768, 768), (648, 384, 384), (1000, 96, 200), (130, 192, 100)]     # four problems, four shapes, ragged M and N


def group_specs():
    return [Conv("fp32", (1, 1, M, K), N, seed=520 + i) for i, (M, K, N) in enumerate(GROUP_SHAPES)]


F32OUT_CASES = [(dname, tile) for dname in BOTH16 for tile in (3, 4)]


def f32out_spec(dname):
    return Conv(dname, (1, 1, 700, 192), 864, seed=540)


def bf16x3_spec():
    return Conv("fp32", (2, 14, 24, 96), 192, 3, 1, 1, epi=("bias",), seed=560)


def all_conv_specs():
    """Every distinct Conv of the forward tables (the host test walks them once each)."""
    specs = [r.spec for r in forward_routes()]
    for case in PAIR_CASES:
        specs += pair_specs(case)
    specs += group_specs() + [f32out_spec(d) for d in BOTH16] + [bf16x3_spec()]
    return list(dict.fromkeys(specs))


# ---- tap and up2 forms (fp32) --------------------------------------------------------------------------------------------------------
# N, Cin, Cout, (H, W), dil: one source at factor 2 (bilinear weights 1/4, 3/4: multiples of 1/16), tests/test_gpu_ops.py::TAPSUM_CASES
TAPSUM_CASES = [(3, 64, 96, (16, 24), 2), (2, 32, 64, (6, 10), 1), (3, 64, 96, (14, 24), 2)]
UP2_CASES = [(2, 3, 5, 96, 12), (2, 7, 9, 96, 68), (3, 13, 12, 192, 96)]       # N, h, w, Cin, Cout (tests/test_gpu_upconv.py::CASES)


@functools.lru_cache(maxsize=None)
def up2_problem(N, h, w, Cin, Cout, dil, epi, seed):
    """conv3x3(dilation dil, padding dil)(bilinear_up2(z)) with bias / BN affine / ReLU: z [N,h,w,Cin], wt [Cout,Cin,3,3].  Every value
    is a multiple of 1/16 (1/32 after a scale of 0.5): condition (a) on 16 (32) x the magnitudes."""
    p = Problem()
    g = generator(seed)
    p.z, p.wt = ints(g, (N, h, w, Cin)), ints(g, (Cout, Cin, 3, 3))
    p.bias = ints(g, (Cout,), 64) if "bias" in epi else None
    p.scale, p.shift = (scales(g, Cout), ints(g, (Cout,))) if "bn" in epi else (None, None)
    p.rowvec = p.residual = None
    p.relu = "relu" in epi
    up = lambda t: F.interpolate(t.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False)
    p.up = up(p.z)
    assert torch.equal((p.up * 16).round(), p.up * 16)
    p.acc = F.conv2d(p.up, p.wt, None, padding=dil, dilation=dil).permute(0, 2, 3, 1).contiguous()
    p.absacc = F.conv2d(up(p.z.abs()), p.wt.abs(), None, padding=dil, dilation=dil).permute(0, 2, 3, 1)
    p.exact = epilogue(p.acc, p)
    p.ref = p.exact.float()
    assert torch.equal(p.ref.double(), p.exact)
    p.bound = 16 * magnitude_bound(p)
    return p


# ---- gradients ---------------------------------------------------------------------------------------------------------------------
WGRAD_SHAPES = [(333, 32, 4), (5000, 160, 100), (3024, 768, 864)]           # M, K, N of test_wgrad_dma_kernel_equals_the_register_staged_kernel
WGRAD_CFGS = [0, 1, 2, 3, 4]                                                # kNumWgradCfgs = 5 in csrc/wgrad.hip
WGRAD_DMA = [0, 1, 2]
WGRAD_SPLITS = [1, 5]
WGRAD_CONV = (2, 14, 24, 96, 192)                                           # N, H, W, Cin, Cout of the 3x3 / padding 1 weight gradient


@functools.lru_cache(maxsize=None)
def wgrad_problem(N, H, W, Cin, Cout, k, seed):
    """dW (packed k order) and db of y = conv(x, w) (k x k, stride 1, padding k // 2) from integer x and dy: sums of N H W products of
    magnitude <= 16, exact below 2^24."""
    p = Problem()
    g = generator(seed)
    p.x, p.dy = ints(g, (N, H, W, Cin)), ints(g, (N, H, W, Cout))
    M = N * H * W
    p.bound = 16.0 * M
    xs, dys = p.x.permute(0, 3, 1, 2), p.dy.permute(0, 3, 1, 2)
    dw = torch.nn.grad.conv2d_weight(xs, (Cout, Cin, k, k), dys, padding=k // 2)
    p.dw = pack_k_order(dw)
    p.db = p.dy.reshape(M, Cout).sum(0)
    p.dw_ref, p.db_ref = p.dw.float(), p.db.float()
    assert torch.equal(p.dw_ref.double(), p.dw) and torch.equal(p.db_ref.double(), p.db)
    return p


SEGMENTED_CASES = [(4, 84, 96, 192), (18, 36, 192, 336)]                    # segments, rows per segment, K, Cout
COLSUM_CASES = [(756, 1536, 756), (3000, 2048, 750), (64, 4, 8)]            # M, C, segment rows (tests/test_gpu_train_ops.py)
# the four small rows of CASES in tests/test_gpu_train_ops.py: N, H, W, Cin, Cout, k, stride, pad, dil, asym, act
BACKWARD_CASES = [(2, 14, 24, 96, 192, 3, 1, 1, 1, False, 0), (3, 12, 20, 64, 96, 3, 1, 2, 2, False, 1),
                  (2, 15, 23, 96, 96, 3, 2, 0, 1, True, 0), (1, 30, 46, 96, 96, 3, 4, 0, 1, True, 0)]
LINEAR_BWD = (3, 50, 96, 192)                                               # lead, rows, K, N


@functools.lru_cache(maxsize=None)
def backward_problem(case, dtype=torch.float64, flip=False):
    """y = act(conv(x, w) + bias + rowvec) and its gradients for an integer gy by torch autograd in ``dtype`` (NCHW; ``flip``: the
    channels reversed, i.e. every sum in another order)."""
    N, H, W, Cin, Cout, k, s, pd, d, asym, act = case
    g = generator(700 + H)
    p = Problem()
    p.x, p.w = ints(g, (N, Cin, H, W)), ints(g, (Cout, Cin, k, k))
    p.b, p.rv = ints(g, (Cout,), 64), ints(g, (N, Cout))
    f = (lambda t, dim: t.flip(dim)) if flip else (lambda t, dim: t)
    leaf = lambda t: t.clone().to(dtype).requires_grad_(True)       # (a copy: the problem's own tensors stay plain data)
    x, w = leaf(f(p.x, 1)), leaf(f(f(p.w, 1), 0))
    b, rv = leaf(f(p.b, 0)), leaf(f(p.rv, 1))
    xin = F.pad(x, (0, 1, 0, 1)) if asym else x
    y = F.conv2d(xin, w, b, stride=s, padding=0 if asym else pd, dilation=d) + rv[:, :, None, None]
    y = F.relu(y) if act else y
    gen2 = generator(800 + H)
    p.gy = ints(gen2, tuple(y.shape))
    y.backward(f(p.gy, 1).to(dtype))
    p.y = f(y.detach(), 1)
    p.dx, p.dw, p.db, p.drv = f(x.grad, 1), f(f(w.grad, 0), 1), f(b.grad, 0), f(rv.grad, 1)
    # condition (a): forward sums <= 16 K + 64 + 4, dx sums <= 16 k^2 Cout, dw sums <= 16 N Ho Wo (+ the same for db, drv)
    p.bound = max(16.0 * k * k * Cin + 68, 16.0 * k * k * Cout, 16.0 * N * y.shape[2] * y.shape[3])
    return p


@functools.lru_cache(maxsize=None)
def linear_backward_problem(dtype=torch.float64, flip=False):
    """y = x w^T + b + r and its gradients for an integer gy (torch autograd in ``dtype``; ``flip``: K and N reversed)."""
    lead, rows, K, N = LINEAR_BWD
    g = generator(860)
    p = Problem()
    p.x, p.w, p.b = ints(g, (lead, rows, K)), ints(g, (N, K)), ints(g, (N,), 64)
    p.r, p.gy = ints(g, (lead, rows, N)), ints(g, (lead, rows, N))
    f = (lambda t, *dims: t.flip(*dims)) if flip else (lambda t, *dims: t)
    leaf = lambda t: t.clone().to(dtype).requires_grad_(True)
    x, w = leaf(f(p.x, 2)), leaf(f(p.w, 0, 1))
    b, r = leaf(f(p.b, 0)), leaf(f(p.r, 2))
    y = F.linear(x, w, b) + r
    y.backward(f(p.gy, 2).to(dtype))
    p.y, p.dx, p.dw, p.db, p.dr = f(y.detach(), 2), f(x.grad, 2), f(w.grad, 0, 1), f(b.grad, 0), f(r.grad, 2)
    p.bound = max(16.0 * K + 68, 16.0 * N, 16.0 * lead * rows)
    return p


@functools.lru_cache(maxsize=None)
def segmented_problem(segments, rows, K, Cout):
    """out[s] = dy_s^T x_s over ``segments`` equal row blocks, and the per-segment column sums of dy."""
    g = generator(870 + segments)
    p = Problem()
    p.x, p.dy = ints(g, (segments * rows, K)), ints(g, (segments * rows, Cout))
    p.out = torch.einsum("srn,srk->snk", p.dy.view(segments, rows, Cout), p.x.view(segments, rows, K))
    p.bound = 16.0 * rows
    return p


@functools.lru_cache(maxsize=None)
def colsum_problem(M, C, seg):
    p = Problem()
    p.dy = ints(generator(880 + C), (M, C), 64)
    p.out = p.dy.view(M // seg, seg, C).sum(1)
    p.bound = 64.0 * seg
    return p


# ---- Winograd F(4x4, 3x3) ----------------------------------------------------------------------------------------------------------
# The transforms of csrc/wino4.hip use integer constants only (input: 4, -5, -4, 2, -2; output: 2, 4, 8), so with U built in integers
# and x in {-1, 0, 1} every value of the path is an integer; the result is 576 x the convolution.
WINO_G24 = [[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]]                  # 24 G
WINO_BT = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]]
WINO_AT = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]
WINO_CASES = [(2, 12, 20, 96, 96, 1), (2, 12, 20, 96, 96, 2)]                                        # N, H, W, Cin, Cout, dilation


@functools.lru_cache(maxsize=None)
def wino_problem(N, H, W, Cin, Cout, dil):
    """x in {-1, 0, 1}, w = 576 w' with w' in {-1, 0, 1}: U = (24 G) w' (24 G)^T in int64 ([36, Cout, Cin]), reference 576 conv(x, w')."""
    p = Problem()
    g = generator(900 + dil)
    p.x = ints(g, (N, H, W, Cin), 1)
    p.w1 = ints(g, (Cout, Cin, 3, 3), 1)
    G = torch.tensor(WINO_G24, dtype=torch.int64)
    U = torch.einsum("ia,ocab,jb->ijoc", G, p.w1.long(), G)
    p.U = U.reshape(36, Cout, Cin).double()
    p.exact = 576.0 * F.conv2d(p.x.permute(0, 3, 1, 2), p.w1, None, padding=dil, dilation=dil).permute(0, 2, 3, 1).contiguous()
    p.ref = p.exact.float()
    assert torch.equal(p.ref.double(), p.exact)
    # the bound of the issue with the kernel's own matrices: sum |A^T| (sum_c |V| |U|) |A| per output tile, V = B^T d B of the
    # actual (zero-padded, dilation-strided) input tiles
    BT, AT = torch.tensor(WINO_BT, dtype=torch.float64), torch.tensor(WINO_AT, dtype=torch.float64)
    worst = 0.0
    xs = p.x.permute(0, 3, 1, 2)
    for py in range(dil):
        for px in range(dil):
            sub = xs[:, :, py::dil, px::dil]                        # a dilated 3x3 convolution is a plain one on each sub-grid
            h, w_ = sub.shape[2:]
            ty, tx = (h + 3) // 4, (w_ + 3) // 4
            padded = F.pad(sub, (1, 4 * tx + 1 - w_, 1, 4 * ty + 1 - h))
            tiles = padded.unfold(2, 6, 4).unfold(3, 6, 4)          # [N, Cin, ty, tx, 6, 6]
            V = torch.einsum("ia,nctxab,jb->ntxijc", BT, tiles, BT)
            assert V.abs().max().item() * 1.0 < LIMIT
            Mabs = torch.einsum("ntxijc,ijoc->ntxijo", V.abs(), p.U.abs().reshape(6, 6, Cout, Cin))
            worst = max(worst, torch.einsum("ai,ntxijo,bj->ntxabo", AT.abs(), Mabs, AT.abs()).max().item())
    p.bound = worst
    return p
