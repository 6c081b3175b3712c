"""diffsal_conv_igemm_ws_bytes is the largest workspace any candidate kernel could use for the descriptor.  CPU only: the query is a
host function of the loaded library (as in tests/test_instantiation_cases_host.py).  A candidate's own need is read with the switches
that leave it alone on the list (the generic kernel with the LDS-DMA kernel switched off, or with its own plan forced); gemm_dma's
K split, which no switch isolates, is pinned on the two rows tests/test_gpu_conv_routes.py launches."""
import ctypes as C

import pytest

from diff_sal_amd import _lib

# (N, H, W, Cin, Cout, k, stride, pad, dil, out_hw): plain products and convolutions of one step at 1, 4 and 64 clips, and odd ones
PRODUCTS = [(756, 768, 768), (756, 768, 1536), (756, 1536, 768), (756, 768, 3456), (3024, 384, 384), (3024, 768, 384), (12096, 192, 864),
            (648, 768, 768), (162, 768, 1536), (10368, 768, 768), (7140, 768, 864), (1344, 384, 768), (193536, 96, 192), (3096576, 96, 96),
            (48384, 768, 768), (2692, 3072, 768), (3000, 288, 200), (700, 192, 864)]
CONVS = [(1, 28, 48, 768, 768, 3, 2, 0, 1, (14, 24)), (4, 14, 24, 768, 768, 3, 2, 0, 1, (7, 12)), (4, 56, 96, 192, 192, 3, 2, 0, 1, (28, 48)),
         (1, 14, 24, 768, 768, 3, 1, 1, 1, None), (4, 14, 24, 768, 768, 3, 1, 1, 1, None), (36, 56, 96, 96, 96, 3, 1, 2, 2, None),
         (36, 14, 24, 768, 384, 3, 1, 2, 2, None), (4, 112, 192, 768, 96, 3, 1, 1, 1, None), (64, 56, 96, 192, 192, 3, 1, 1, 1, None),
         (3, 13, 19, 96, 100, 3, 1, 1, 1, None), (9, 9, 16, 768, 384, 3, 1, 2, 1, (9, 14))]
ROWFORMS = [(4, 9, 84, 768, 768), (4, 9, 5376, 96, 768), (64, 9, 336, 384, 768)]        # ReduceTemp: (5, 1) kernel, stride (5, 1), one frame left


def descriptors(dtype, precision=0, w_format=0):
    out = []
    for M, K, N in PRODUCTS:
        out.append(_lib.ConvDesc(1, 1, M, K, 1, M, N, 1, 1, 1, 1, 0, 0, 1, 1, 0, 0, w_format, precision, dtype))
    for N, H, W, Cin, Cout, k, st, pad, dil, ohw in CONVS:
        Ho, Wo = ohw or ((H + 2 * pad - dil * (k - 1) - 1) // st + 1, (W + 2 * pad - dil * (k - 1) - 1) // st + 1)
        out.append(_lib.ConvDesc(N, H, W, Cin, Ho, Wo, Cout, k, k, st, st, pad, pad, dil, dil, 0, 0, w_format, precision, dtype))
    for B, T, HW, Cc, Co in ROWFORMS:
        out.append(_lib.ConvDesc(B, T, HW, Cc, 1, HW, Co, 5, 1, 5, 1, 0, 0, 1, 1, 0, 0, w_format, precision, dtype))
    return out


def query(d, **sw):
    for k, v in sw.items():
        _lib.set_tuning("DIFFSAL_" + k, v)
    try:
        return _lib.load().diffsal_conv_igemm_ws_bytes(C.byref(d))
    finally:
        for k in sw:
            _lib.set_tuning("DIFFSAL_" + k, None)


def dims(d):
    return d.N * d.Ho * d.Wo, d.KH * d.KW * d.Cin, d.Cout


def is_linear(d):
    return (d.KH, d.KW, d.stride_h, d.stride_w, d.pad_t, d.pad_l) == (1, 1, 1, 1, 0, 0) and (d.Ho, d.Wo) == (d.H, d.W)


@pytest.mark.parametrize("precision,w_format", [(0, 0), (1, 0), (1, 1)], ids=["fp32", "bf16x3", "bf16x3-presplit"])
def test_fp32_query_covers_the_tiled_kernel(precision, w_format):
    n_more = 0
    for d in descriptors(_lib.F32, precision, w_format):
        off = "GEMM_DMA" if is_linear(d) else "CONV_DMA"
        tiled = query(d, **{off: 0})                                    # the tiled kernel alone
        assert query(d) >= tiled, dims(d)
        for cfg in (1, 2):                                              # gemm_dma offered on every shape it accepts
            assert query(d, **{off: cfg}) >= tiled, (dims(d), cfg)
            n_more += query(d, **{off: cfg}) > tiled
        if precision != 0:                                              # gemm_dma is exact arithmetic only
            assert query(d) == query(d, **{off: 1}) == tiled, dims(d)
    assert precision != 0 or n_more >= 5            # the table does reach rows where gemm_dma's K split asks for more


@pytest.mark.parametrize("dtype", [_lib.BF16, _lib.F16], ids=["bf16", "fp16"])
def test_16_bit_query_covers_the_generic_kernel(dtype):
    for d in descriptors(dtype):
        generic = query(d, GEMM_DMA16=0)
        assert query(d) >= generic and query(d, GEMM_DMA16=1) >= generic, dims(d)
        for v in (0, 2, 8, 13, 21):                                     # a forced tile / split of the generic kernel stands alone
            forced = query(d, IGEMM16_CFG=v)
            assert forced == query(d, IGEMM16_CFG=v, GEMM_DMA16=1, FORCE_HALO=2), (dims(d), v)


def test_a_shape_the_halo_kernel_takes_reports_no_workspace():
    """mt_proj at 4 clips: 86016 pixels, 3 x 3, K = 6912.  The halo kernels need no workspace, and the generic kernel is reached only
    with pointers its K split could not use either: it runs unsplit, so the maximum over the list is 0 -- no exception in the query.
    Without the halo kernel on the list the generic kernel plans its split."""
    d = _lib.ConvDesc(4, 112, 192, 768, 112, 192, 96, 3, 3, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, _lib.BF16)
    assert query(d) == 0 and query(d, NO_STREAM16=1) == 0
    assert query(d, NO_HALO=1) > 0


def test_known_rows():
    """the rows tests/test_gpu_conv_routes.py launches.  Plain product: the tiled kernel alone and gemm_dma's split 4 both ask for
    4 slabs; stride-2 convolution: the tiled kernel's 16 slabs exceed the 8 of gemm_dma's split (its launch prints split-K 8), and the
    query is the larger.  The slab counts follow the planners' cost-model constants: a retune of those is expected to move this pin."""
    plain = _lib.ConvDesc(1, 1, 756, 768, 1, 756, 768, 1, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0, _lib.F32)
    conv = _lib.ConvDesc(1, 28, 48, 768, 14, 24, 768, 3, 3, 2, 2, 0, 0, 1, 1, 0, 0, 0, 0, _lib.F32)
    assert query(plain) == 4 * 756 * 768 * 4
    assert query(conv) == query(conv, CONV_DMA=0) == 16 * 336 * 768 * 4 >= 8 * 336 * 768 * 4
