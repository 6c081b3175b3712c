"""Every route of the matrix kernels, bit for bit against fp64 (tests/_exact_ref.py).

Integer operands in [-4, 4] (larger where noted there): every product and partial sum is an integer below 2^24, so the fp32 accumulator is
exact under any tile shape, K split, slab sum or DMA ring depth, and the one store to the storage type is the only rounding.  A lifting
bias carries the 16-bit sums above 2^8 (bf16) / 2^11 (fp16), where 6 - 50 % of the integers are rounding ties: a store that truncates or
rounds ties away, a k term lost or doubled on a ragged stage, a halo edge or a split boundary, and a wrong element of a small output all
break ``torch.equal``.  tests/test_exact_ref_host.py proves the conditions and the power of every case without a GPU.

Every case prints the kernel that ran (``diffsal_last_gemm_kernel()``, asserted where a route is forced) and its tie / inexact shares.

Left out, because the design rounds there more than once (not single-rounding, so not exact by this method):
  * ``up2_conv3x3_d2`` on 16-bit storage: ``c_ext`` is rounded to the storage type before it is interpolated, and so are the tap products (the bar
    of tests/test_gpu_upconv.py::test_up2_conv_commute_16bit_storage is 3x the one-rounding bar for that reason);
  * GELU and sigmoid epilogues (the ``tapsum`` head among them): transcendental, covered by tests/test_gpu_value_range.py.  The switch
    DIFFSAL_TAPSUM_ROWS_FORM selects lane mappings of the head kernel only; the plain ``tapsum`` runs under both values all the same.
"""
import re

import pytest
import torch

from tests import _exact_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from diff_sal_amd import ops as o

    assert torch.cuda.is_available()
    return o


def kernel_name():
    from diff_sal_amd import _lib

    return _lib.load().diffsal_last_gemm_kernel().decode()


def to_dev(t):
    return t.to(DEV)


def dev(t, up=to_dev):
    """fp64 integers of a problem -> contiguous fp32 on the device (exact), None stays None.  ``up`` uploads: ``.to(DEV)``, or
    tests/_guard.py's ``put`` where tests/test_gpu_guard_bands.py runs the case bodies of this file between guard bands."""
    return None if t is None else up(t.float().contiguous())


def store(t, dname, up=to_dev):
    return None if t is None else up(E.to_storage(dev(t), dname))


def packed(ops, w, dname, up=to_dev):
    """The library's packed weight in the storage type; it must be the permutation tests/_exact_ref.py::pack_k_order writes out."""
    wp = ops.cast(ops.pack_conv_weight(dev(w, up)), E.DTYPES[dname])
    assert torch.equal(wp.double().cpu(), E.pack_k_order(w))
    return wp


def set_switches(tuning, switches):
    for k, v in switches:
        tuning.set("DIFFSAL_" + k, v)


def run_conv(ops, c, p, up=to_dev, **over):
    kw = dict(kh=c.k, kw=c.k, stride=(c.stride, c.stride), pad=(c.pad, c.pad), dil=(c.dil, c.dil), out_hw=c.hw(), bias=dev(p.bias, up),
              scale=dev(p.scale, up), shift=dev(p.shift, up), rowvec=dev(p.rowvec, up),
              residual=None if p.residual is None else store(p.residual, c.dname, up), act=ops.ACT_RELU if p.relu else ops.ACT_NONE)
    kw.update(over)
    return ops.conv_igemm(store(p.x, c.dname, up), packed(ops, p.w, c.dname, up), **kw)


ROUTES = E.forward_routes()


def case_forward_route_equals_fp64(ops, tuning, route, up=to_dev):
    """ROWS of tests/test_gpu_conv_routes.py in every storage type with a bias and with the full epilogue, every tile configuration
    of igemm / igemm16 / conv16_dma, and the strided and dilated convolutions of CONV_CASES with the full epilogue."""
    c = route.spec
    p = E.problem(c)
    set_switches(tuning, route.switches)
    got = run_conv(ops, c, p, up)
    name = kernel_name()
    print(f"{route.id}: {name}")
    assert re.search(route.kernel, name), (route.kernel, name)
    assert got.dtype == E.DTYPES[c.dname]
    E.check_equal(got, p.ref, route.id, p.exact, c.dname)


@pytest.mark.parametrize("route", ROUTES, ids=[r.id for r in ROUTES])
def test_forward_route_equals_fp64(ops, tuning, route):
    case_forward_route_equals_fp64(ops, tuning, route)


def case_linear_pair_equals_fp64(ops, tuning, case, up=to_dev):
    """Both routes of test_linear_pair_routes_on_twice_the_reported_workspace (grouped LDS-DMA, paired tiled) and the 16-bit pair."""
    cid, dname, K, N, sw, kernel = case
    set_switches(tuning, tuple(sw.items()))
    specs = E.pair_specs(case)
    ps = [E.problem(c) for c in specs]
    xs = [store(p.x, dname, up).view(E.M_PAIR, K) for p in ps]
    ws = [packed(ops, p.w, dname, up) for p in ps]
    ys = ops.linear_pair(xs[0], xs[1], ws[0], ws[1], dev(ps[0].bias, up), dev(ps[1].bias, up))
    name = kernel_name()
    print(f"pair {cid}: {name}")
    assert re.search(kernel, name), name
    for i in range(2):
        E.check_equal(ys[i], ps[i].ref.view(E.M_PAIR, N), f"pair {cid}[{i}]", ps[i].exact.view(E.M_PAIR, N), dname)


@pytest.mark.parametrize("case", E.PAIR_CASES, ids=[c[0] for c in E.PAIR_CASES])
def test_linear_pair_equals_fp64(ops, tuning, case):
    case_linear_pair_equals_fp64(ops, tuning, case)


def case_linear_group_equals_fp64(ops, up=to_dev):
    """ops.linear_group / conv_igemm_group: four plain products of four shapes (ragged M and N) in one launch."""
    ps = [E.problem(c) for c in E.group_specs()]
    ys = ops.linear_group([dev(p.x, up).view(M, K) for p, (M, K, N) in zip(ps, E.GROUP_SHAPES)], [packed(ops, p.w, "fp32", up) for p in ps],
                          [dev(p.bias, up) for p in ps])
    name = kernel_name()
    print(f"group: {name}")
    assert re.search(r"^gemm_dma_kernel<float, 3, 3, 3, 2, true, true> .*4 problems", name), name
    for i, (p, y) in enumerate(zip(ps, ys)):
        E.check_equal(y, p.ref.view(y.shape), f"group[{i}]")


def test_linear_group_equals_fp64(ops):
    case_linear_group_equals_fp64(ops)


def case_linear_fp32_out_of_16bit_operands_is_not_rounded(ops, tuning, dname, tile, up=to_dev):
    """linear(out_f32=True): the exact integers, although they are far from representable in the storage type."""
    c = E.f32out_spec(dname)
    p = E.problem(c)
    tuning.set("DIFFSAL_GEMM_DMA16", tile)
    M, K = c.xshape[2:]
    got = ops.linear(store(p.x, dname, up).view(M, K), packed(ops, p.w, dname, up), dev(p.bias, up), out_f32=True)
    name = kernel_name()
    print(f"f32out {dname} tile {tile}: {name}")
    assert "gemm16_dma2_kernel" in name and ("192x192" in name) == (tile == 4), name
    assert E.tie_shares(p.exact, dname)[1] > 0.10
    E.check_equal(got, p.exact.float().view(M, c.Cout), f"f32out-{dname}-{tile}")


@pytest.mark.parametrize("dname,tile", E.F32OUT_CASES, ids=[f"{d}-tile{t}" for d, t in E.F32OUT_CASES])
def test_linear_fp32_out_of_16bit_operands_is_not_rounded(ops, tuning, dname, tile):
    case_linear_fp32_out_of_16bit_operands_is_not_rounded(ops, tuning, dname, tile)


def case_bf16x3_precision_is_exact_on_small_integers(ops, split, up=to_dev):
    """Integers up to 4 have a zero low half: hi*hi alone is the product, and the result is the exact integers."""
    c = E.bf16x3_spec()
    p = E.problem(c)
    wp = packed(ops, p.w, "fp32", up)
    with ops.gemm_precision("bf16x3"):
        got = run_conv(ops, c, p, up) if not split else ops.conv_igemm(
            dev(p.x, up), ops.split_weight(wp), kh=3, kw=3, pad=(1, 1), bias=dev(p.bias, up))
    name = kernel_name()
    print(f"bf16x3 split={split}: {name}")
    assert re.search(r"^igemm_kernel<\d, \d, \d, \d, 1>", name), name
    E.check_equal(got, p.ref, f"bf16x3-{split}")


@pytest.mark.parametrize("split", [False, True], ids=["split-in-kernel", "split_weight"])
def test_bf16x3_precision_is_exact_on_small_integers(ops, split):
    case_bf16x3_precision_is_exact_on_small_integers(ops, split)


# ---- tap and up2 forms (fp32) --------------------------------------------------------------------------------------------------------
def case_tapsum_of_tap_weight_products_equals_fp64(ops, tuning, i, form, up=to_dev):
    N, Cin, Cout, (H, W), dil = E.TAPSUM_CASES[i]
    p = E.up2_problem(N, H // 2, W // 2, Cin, Cout, dil, ("bias", "bn", "relu"), 600 + i)
    assert p.bound < E.LIMIT
    if form is not None:
        tuning.set("DIFFSAL_TAPSUM_ROWS_FORM", form)
    y9 = ops.linear(dev(p.z, up), ops.tap_weight(dev(p.wt, up)), None)
    print(f"tapsum {E.TAPSUM_CASES[i]} form {form}: tap products on {kernel_name()}")
    got = ops.tapsum([y9], H, W, Cout, dil=dil, bias=dev(p.bias, up), scale=dev(p.scale, up), shift=dev(p.shift, up), act=ops.ACT_RELU)
    E.check_equal(got, p.ref, f"tapsum-{i}-{form}")


@pytest.mark.parametrize("form", [None, 1, 3])
@pytest.mark.parametrize("i", range(len(E.TAPSUM_CASES)), ids=[str(c) for c in E.TAPSUM_CASES])
def test_tapsum_of_tap_weight_products_equals_fp64(ops, tuning, i, form):
    case_tapsum_of_tap_weight_products_equals_fp64(ops, tuning, i, form)


def case_up2_conv3x3_d2_equals_fp64(ops, tuning, i, ring_only, up=to_dev):
    """Bilinear x2 then the dilation-2 convolution, both in double; the direct (not Winograd) kernel on the extended grid.  ``ring_only``
    writes the 3-pixel border ring alone: that ring is compared, and c_ext with the convolution on the extended source grid."""
    import torch.nn.functional as F

    N, h, w, Cin, Cout = E.UP2_CASES[i]
    p = E.up2_problem(N, h, w, Cin, Cout, 2, ("bn", "relu"), 620 + i)
    assert p.bound < E.LIMIT
    tuning.set("DIFFSAL_NO_WINOGRAD", 1)
    wd = dev(p.wt, up)
    tapw = up(wd.permute(2, 3, 0, 1).reshape(9 * Cout, Cin).contiguous())
    res = ops.up2_conv3x3_d2(dev(p.z, up), ops.pack_conv_weight(wd), None, tapw, scale=dev(p.scale, up), shift=dev(p.shift, up), act=ops.ACT_RELU,
                             ring_only=ring_only)
    print(f"up2 {E.UP2_CASES[i]} ring_only={ring_only}: border tap products on {kernel_name()}")
    if not ring_only:
        E.check_equal(res, p.ref, f"up2-{i}")
        return
    out, c_ext = res
    ring = torch.ones(2 * h, 2 * w, dtype=torch.bool)
    ring[3:2 * h - 3, 3:2 * w - 3] = False
    E.check_equal(out.cpu()[:, ring], p.ref[:, ring], f"up2-ring-{i}")
    ext = F.conv2d(p.z.permute(0, 3, 1, 2), p.wt, None, padding=2).permute(0, 2, 3, 1).contiguous()
    E.check_equal(c_ext, ext.float(), f"up2-c_ext-{i}")


@pytest.mark.parametrize("ring_only", [False, True], ids=["direct", "ring_only"])
@pytest.mark.parametrize("i", range(len(E.UP2_CASES)), ids=[str(c) for c in E.UP2_CASES])
def test_up2_conv3x3_d2_equals_fp64(ops, tuning, i, ring_only):
    case_up2_conv3x3_d2_equals_fp64(ops, tuning, i, ring_only)


# ---- gradients ---------------------------------------------------------------------------------------------------------------------
WGRAD_ROUTES = [(cfg, dma) for cfg in E.WGRAD_CFGS for dma in (E.WGRAD_DMA if cfg == 0 else [None])]


def case_plain_wgrad_equals_fp64(ops, tuning, i, cfg, dma, up=to_dev):
    """conv_wgrad(want_bias=True) of a plain product under every tile shape of csrc/wgrad.hip (kNumWgradCfgs = 5), the register-staged
    and both LDS-DMA forms of tile 0, and one or five splits of M: dW and db are the fp64 integers."""
    M, K, N = E.WGRAD_SHAPES[i]
    p = E.wgrad_problem(1, 1, M, K, N, 1, 640 + i)
    assert p.bound < E.LIMIT
    tuning.set("DIFFSAL_WGRAD_CFG", cfg)
    if dma is not None:
        tuning.set("DIFFSAL_WGRAD_DMA", dma)
    for splits in E.WGRAD_SPLITS:
        tuning.set("DIFFSAL_WGRAD_SPLITS", splits)
        dw, db = ops.conv_wgrad(dev(p.x, up), dev(p.dy, up), want_bias=True)
        E.check_equal(dw, p.dw_ref, f"wgrad {M}x{K}x{N} cfg {cfg} dma {dma} splits {splits}: dW")
        E.check_equal(db, p.db_ref, f"wgrad {M}x{K}x{N} cfg {cfg} dma {dma} splits {splits}: db")


@pytest.mark.parametrize("cfg,dma", WGRAD_ROUTES, ids=[f"cfg{c}-dma{d}" for c, d in WGRAD_ROUTES])
@pytest.mark.parametrize("i", range(len(E.WGRAD_SHAPES)), ids=[str(s) for s in E.WGRAD_SHAPES])
def test_plain_wgrad_equals_fp64(ops, tuning, i, cfg, dma):
    case_plain_wgrad_equals_fp64(ops, tuning, i, cfg, dma)


def case_conv3x3_wgrad_equals_fp64(ops, tuning, cfg, up=to_dev):
    p = E.wgrad_problem(*E.WGRAD_CONV, 3, 650)
    assert p.bound < E.LIMIT
    tuning.set("DIFFSAL_WGRAD_CFG", cfg)
    for splits in E.WGRAD_SPLITS:
        tuning.set("DIFFSAL_WGRAD_SPLITS", splits)
        dw, db = ops.conv_wgrad(dev(p.x, up), dev(p.dy, up), kh=3, kw=3, pad=(1, 1), want_bias=True)
        E.check_equal(dw, p.dw_ref, f"wgrad 3x3 cfg {cfg} splits {splits}: dW")
        E.check_equal(db, p.db_ref, f"wgrad 3x3 cfg {cfg} splits {splits}: db")


@pytest.mark.parametrize("cfg", E.WGRAD_CFGS)
def test_conv3x3_wgrad_equals_fp64(ops, tuning, cfg):
    case_conv3x3_wgrad_equals_fp64(ops, tuning, cfg)


def case_wgrad_segmented_equals_fp64(ops, case, up=to_dev):
    p = E.segmented_problem(*case)
    E.check_equal(ops.wgrad_segmented(dev(p.x, up), dev(p.dy, up), case[0]), p.out.float(), f"wgrad_segmented {case}")


@pytest.mark.parametrize("case", E.SEGMENTED_CASES, ids=str)
def test_wgrad_segmented_equals_fp64(ops, case):
    case_wgrad_segmented_equals_fp64(ops, case)


def case_colsum_equals_fp64(ops, case, up=to_dev):
    """Segmented and wide (C = 1536, 2048) column sums."""
    M, C, seg = case
    p = E.colsum_problem(*case)
    E.check_equal(ops.colsum(dev(p.dy, up), seg), p.out.float(), f"colsum {case}")


@pytest.mark.parametrize("case", E.COLSUM_CASES, ids=str)
def test_colsum_equals_fp64(ops, case):
    case_colsum_equals_fp64(ops, case)


def case_conv_backward_equals_fp64_autograd(ops, case, up=to_dev):
    """autograd_ops.conv with an integer gy: y, dx, dw, dbias and drowvec are fp64 autograd's integers -- the data-gradient weight pack,
    the flipped-kernel convolution (stride 1), col2im_gather (stride 2) and col2im_disjoint (stride 4), the ReLU mask."""
    from diff_sal_amd import autograd_ops as ag

    N, H, W, Cin, Cout, k, s, pd, d, asym, act = case
    p = E.backward_problem(case)
    assert p.bound < E.LIMIT
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    xd, wd = dev(nhwc(p.x), up).requires_grad_(True), dev(p.w, up).requires_grad_(True)
    bd, rvd = dev(p.b, up).requires_grad_(True), dev(p.rv, up).requires_grad_(True)
    yd = ag.conv(xd, ops.pack_conv_weight_diff(wd), kh=k, kw=k, stride=(s, s), pad=(0, 0) if asym else (pd, pd), dil=(d, d),
                 out_hw=tuple(p.y.shape[-2:]), bias=bd, rowvec=rvd, act=act, w_dgrad=ag.dgrad_weight(wd, (s, s)))
    print(f"backward {case}: forward on {kernel_name()}")
    E.check_equal(yd, nhwc(p.y).float(), "y")
    yd.backward(dev(nhwc(p.gy), up))
    print(f"backward {case}: last product of the backward on {kernel_name()}")
    E.check_equal(xd.grad, nhwc(p.dx).float(), "dx")
    E.check_equal(wd.grad, p.dw.float(), "dw")
    E.check_equal(bd.grad, p.db.float(), "dbias")
    E.check_equal(rvd.grad, p.drv.float(), "drowvec")


@pytest.mark.parametrize("case", E.BACKWARD_CASES, ids=str)
def test_conv_backward_equals_fp64_autograd(ops, case):
    case_conv_backward_equals_fp64_autograd(ops, case)


def case_linear_backward_with_residual_equals_fp64_autograd(ops, tuning, dma, up=to_dev):
    from diff_sal_amd import autograd_ops as ag

    p = E.linear_backward_problem()
    assert p.bound < E.LIMIT
    tuning.set("DIFFSAL_GEMM_DMA", dma)
    xd, wd, bd, rd = (dev(t, up).requires_grad_(True) for t in (p.x, p.w, p.b, p.r))
    yd = ag.linear(xd, wd, bd, residual=rd)
    fwd = kernel_name()
    E.check_equal(yd, p.y.float(), "y")
    yd.backward(dev(p.gy, up))
    print(f"linear backward GEMM_DMA={dma}: forward on {fwd}, data gradient on {kernel_name()}")
    assert ("gemm_dma_kernel" in fwd) == (dma == 1), fwd
    for got, ref, what in ((xd.grad, p.dx, "dx"), (wd.grad, p.dw, "dw"), (bd.grad, p.db, "db"), (rd.grad, p.dr, "dr")):
        E.check_equal(got, ref.float(), what)


@pytest.mark.parametrize("dma", [0, 1])
def test_linear_backward_with_residual_equals_fp64_autograd(ops, tuning, dma):
    case_linear_backward_with_residual_equals_fp64_autograd(ops, tuning, dma)


# ---- Winograd F(4x4, 3x3) ----------------------------------------------------------------------------------------------------------
def case_winograd_f4x4_is_exact_on_an_integer_transform(ops, case, up=to_dev):
    """The headline path, whose bar elsewhere is 1e-4.  ``pack_wino4_weight`` is not exact (1/6 in fp64), so U = (24 G) w' (24 G)^T is built
    in int64 from w' in {-1, 0, 1} and handed to conv3x3_wino4_ex with x in {-1, 0, 1}: csrc/wino4.hip's input and output transforms use
    the integer constants 4, -5, -4, 2, -2 and 2, 4, 8 only, and the bound sum |A^T| (sum |V| |U|) |A| with those matrices is 1.1e7 < 2^24
    (tests/test_exact_ref_host.py), so every value on the way is an exact integer and the result is 576 x the convolution."""
    N, H, W, Cin, Cout, dil = case
    p = E.wino_problem(*case)
    assert p.bound < E.LIMIT
    got = ops.conv3x3_wino4_ex(dev(p.x, up), dev(p.U, up), dil=dil)[0]
    name = kernel_name()
    print(f"winograd {case}: {name}")
    assert name.startswith("wino4_input_kernel"), name
    E.check_equal(got, p.ref, f"winograd dilation {dil}")


@pytest.mark.parametrize("case", E.WINO_CASES, ids=str)
def test_winograd_f4x4_is_exact_on_an_integer_transform(ops, case):
    case_winograd_f4x4_is_exact_on_an_integer_transform(ops, case)
