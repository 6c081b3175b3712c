"""Every route of diffsal_conv_igemm / diffsal_linear_pair, called through the raw binding with the caller's own workspace.

Per row: (a) with a workspace of exactly ``diffsal_conv_igemm_ws_bytes(d)`` bytes the named kernel runs; (b) a workspace four times
as large plus 1 MiB gives the same bits -- a query that under-reports makes gemm_dma drop its K split, and the sums change; (c) the
result meets an fp64 reference within the bar of the neighbouring tests: 2e-5 (tests/test_gpu_ops.py) on fp32, OP_RTOL of
tests/test_gpu_stream16.py on 16-bit storage."""
import ctypes as C
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import salunet_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
RTOL = {"fp32": 2e-5, "bf16": 6e-3, "fp16": 8e-4}
BOTH16 = ("bf16", "fp16")


def rnd(name, *shape, scale=1.0):
    return orc.synth_tensor(name, shape, scale)


def rel_err(got, ref):
    ref = ref.float().cpu()
    return (got.float().cpu() - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)


class switches:
    def __init__(self, sw):
        self.sw = sw

    def __enter__(self):
        from diff_sal_amd import _lib

        for k, v in self.sw.items():
            _lib.set_tuning("DIFFSAL_" + k, v)

    def __exit__(self, *a):
        from diff_sal_amd import _lib

        for k in self.sw:
            _lib.set_tuning("DIFFSAL_" + k, None)


def _desc(x, Cout, kh, kw, stride, pad, out_hw):
    from diff_sal_amd import _lib, ops

    N, H, W, Cin = x.shape
    return _lib.ConvDesc(N, H, W, Cin, out_hw[0], out_hw[1], Cout, kh, kw, stride[0], stride[1], pad[0], pad[1], 1, 1, 0, 0, 0,
                         _lib.PREC_FP32, ops._dt(x))


def _workspace(nbytes):
    return torch.full((nbytes // 4 + 4,), float("nan"), device=DEV, dtype=torch.float32) if nbytes else None


def _raw_conv(d, x, w, bias, out, ws, nbytes):
    from diff_sal_amd import _lib, ops

    lib = _lib.load()
    _lib.check(lib.diffsal_conv_igemm(C.byref(d), x.data_ptr(), w.data_ptr(), ops._p(bias), None, None, None, None, out.data_ptr(),
                                      ops._p(ws), nbytes, ops._stream()), "conv_igemm")
    return lib.diffsal_last_gemm_kernel().decode()


def _splits(name):
    m = re.search(r"split-K (\d+)", name)
    return int(m.group(1)) if m else 1


# (id, storage types, input NHWC, Cout, k, stride, pad, out_hw, switches, kernel expected (regex), K split expected)
PLAIN = dict(k=1, stride=1, pad=0)
ROWS = [
    ("plain-gemm_dma-split", ("fp32",), (1, 1, 756, 768), 768, 1, 1, 0, (1, 756), {}, r"^gemm_dma_kernel<float, 3, 3, 3, 2, false", True),
    ("plain-tiled", ("fp32",), (1, 1, 756, 768), 768, 1, 1, 0, (1, 756), {"GEMM_DMA": 0}, r"^igemm_(linear_)?kernel<", None),
    ("conv-gemm_dma-split", ("fp32",), (1, 28, 48, 768), 768, 3, 2, 0, (14, 24), {}, r"^gemm_dma_kernel<float, 3, 3, 3, 2, true", True),
    ("conv-tiled", ("fp32",), (1, 28, 48, 768), 768, 3, 2, 0, (14, 24), {"CONV_DMA": 0}, r"^igemm_kernel<", None),
    # lin_stream.hip's own guard: M >= 65536, K and N in {96, 192}
    ("lin_stream", ("fp32",), (1, 1, 65536, 96), 96, 1, 1, 0, (1, 65536), {}, r"^lin_stream_kernel", None),
    ("generic16-split", BOTH16, (1, 14, 24, 768), 768, 3, 1, 1, (14, 24), {}, r"^igemm16_kernel<", True),
    ("conv16_dma", BOTH16, (1, 16, 32, 64), 64, 3, 1, 1, (16, 32), {"FORCE_HALO": 2}, r"^conv16_dma_kernel<", None),
    ("conv16_halo", BOTH16, (1, 16, 32, 64), 64, 3, 1, 1, (16, 32), {"FORCE_HALO": 1}, r"^conv16_halo_kernel<", None),
    ("gemm16_dma2-256x96", BOTH16, (1, 1, 700, 192), 864, 1, 1, 0, (1, 700), {"GEMM_DMA16": 3}, r"^gemm16_dma2_kernel<.*\[256x96 tile", None),
    ("gemm16_dma2-192x192", BOTH16, (1, 1, 700, 192), 864, 1, 1, 0, (1, 700), {"GEMM_DMA16": 4}, r"^gemm16_dma2_kernel<.*\[192x192 tile", None),
    ("gemm_dma16-96x96", BOTH16, (1, 1, 700, 192), 864, 1, 1, 0, (1, 700), {"GEMM_DMA16": 1}, r"^gemm_dma_kernel<(__bf16|_Float16), 3, 3, 3, 2", None),
    ("gemm_dma16-192x192", BOTH16, (1, 1, 700, 192), 864, 1, 1, 0, (1, 700), {"GEMM_DMA16": 2}, r"^gemm_dma_kernel<(__bf16|_Float16), 6, 6, 3, 1", None),
]
CASES = [pytest.param(dname, *row[2:], id=f"{row[0]}-{dname}") for row in ROWS for dname in row[1]]


@pytest.mark.parametrize("dname,xshape,Cout,k,stride,pad,out_hw,sw,kernel,split", CASES)
def test_route_runs_on_exactly_the_reported_workspace(dname, xshape, Cout, k, stride, pad, out_hw, sw, kernel, split):
    from diff_sal_amd import _lib, ops

    dt = DTYPES[dname]
    N, H, W, Cin = xshape
    x32 = rnd("cr_x", *xshape)
    w32 = rnd("cr_w", Cout, Cin, k, k, scale=(k * k * Cin) ** -0.5)
    b = rnd("cr_b", Cout).to(DEV)
    x = x32.to(DEV).to(dt)
    w = ops.cast(ops.pack_conv_weight(w32.to(DEV)), dt)
    d = _desc(x, Cout, k, k, (stride, stride), (pad, pad), out_hw)
    lib = _lib.load()
    outs, names = [], []
    with switches(sw):
        need = lib.diffsal_conv_igemm_ws_bytes(C.byref(d))
        for nbytes in (need, 4 * need + (1 << 20)):
            ws = _workspace(nbytes)
            out = torch.full((N, out_hw[0], out_hw[1], Cout), float("nan"), device=DEV, dtype=dt)
            names.append(_raw_conv(d, x, w, b, out, ws, nbytes))
            outs.append(out)
    print(f"{dname} {xshape} -> {Cout}: ws_bytes {need}, kernel {names[0]}")
    assert re.search(kernel, names[0]), names[0]
    assert names[1] == names[0]
    if split:
        assert need > 0 and _splits(names[0]) > 1, (need, names[0])
    assert torch.equal(outs[0], outs[1])
    # fp64 reference on the storage type's rounded operands; bottom / right padding implied by out_hw
    xr, wr = x.double().cpu().permute(0, 3, 1, 2), w32.to(DEV).to(dt).double().cpu()
    pb, pr = (out_hw[0] - 1) * stride + k - H - pad, (out_hw[1] - 1) * stride + k - W - pad
    ref = F.conv2d(F.pad(xr, (pad, max(pr, 0), pad, max(pb, 0))), wr, b.double().cpu(), stride=stride).permute(0, 2, 3, 1)
    err = rel_err(outs[0], ref)
    print(f"  rel err {err:.3g} (bar {RTOL[dname]})")
    assert err < RTOL[dname]


@pytest.mark.parametrize("K,N,kernel", [(768, 1536, r"^gemm_dma_kernel<float, 3, 3, 3, 2, true, true>"), (384, 768, r"^igemm_kernel<.*pair")],
                         ids=["grouped-dma", "paired-tiled"])
def test_linear_pair_routes_on_twice_the_reported_workspace(K, N, kernel):
    from diff_sal_amd import _lib, ops

    M = 648
    lib = _lib.load()
    xs = [rnd("cr_px%d" % i, M, K).to(DEV) for i in range(2)]
    wts = [rnd("cr_pw%d" % i, N, K, scale=K ** -0.5).to(DEV) for i in range(2)]
    bs = [rnd("cr_pb%d" % i, N).to(DEV) for i in range(2)]
    d = _desc(xs[0].view(1, 1, M, K), N, 1, 1, (1, 1), (0, 0), (1, M))
    need = 2 * lib.diffsal_conv_igemm_ws_bytes(C.byref(d))
    res = []
    for nbytes in (need, 4 * need + (1 << 20)):
        ws = _workspace(nbytes)
        ys = [torch.full((M, N), float("nan"), device=DEV) for _ in range(2)]
        _lib.check(lib.diffsal_linear_pair(C.byref(d), xs[0].data_ptr(), xs[1].data_ptr(), wts[0].data_ptr(), wts[1].data_ptr(),
                                           bs[0].data_ptr(), bs[1].data_ptr(), ys[0].data_ptr(), ys[1].data_ptr(), ops._p(ws), nbytes,
                                           ops._stream()), "linear_pair")
        res.append((lib.diffsal_last_gemm_kernel().decode(), ys))
    print(f"pair K={K} N={N}: ws_bytes {need}, kernel {res[0][0]}")
    assert re.search(kernel, res[0][0]), res[0][0]
    assert res[1][0] == res[0][0]
    for i in range(2):
        assert torch.equal(res[0][1][i], res[1][1][i])
        ref = xs[i].double() @ wts[i].double().t() + bs[i].double()
        assert rel_err(res[0][1][i], ref) < RTOL["fp32"]


def test_row_form_declines_a_tile_that_spans_past_the_32_bit_offsets():
    """gemm16_dma2's row form addresses a tile's input rows with 32-bit offsets from the tile's first image, and a 256-row tile of
    W = 1 maps spans 258 images: at 8 MiB per image that is past 2^31, so the kernel declines and the generic kernel runs.  Integer
    operands: every fp32 sum is exact, so the bits do not depend on the generic kernel's K split."""
    from diff_sal_amd import _lib

    Nimg, H, Cin, KH, Cout = 258, 4096, 1024, 2, 64
    assert 2 * H * Cin * 2 < 2 ** 31 <= (256 // 1 + 2) * H * Cin * 2
    lib = _lib.load()
    g = torch.Generator(device="cpu").manual_seed(7)
    x = torch.zeros((Nimg, H, 1, Cin), device=DEV, dtype=torch.bfloat16)
    x[:, :KH] = torch.randint(-4, 5, (Nimg, KH, 1, Cin), generator=g).to(DEV).to(torch.bfloat16)
    w = torch.randint(-4, 5, (Cout, KH * Cin), generator=g).to(DEV).to(torch.bfloat16)
    d = _lib.ConvDesc(Nimg, H, 1, Cin, 1, 1, Cout, KH, 1, KH, 1, 0, 0, 1, 1, 0, 0, 0, _lib.PREC_FP32, _lib.BF16)

    def run(sw):
        with switches(sw):
            need = lib.diffsal_conv_igemm_ws_bytes(C.byref(d))
            out = torch.full((Nimg, 1, 1, Cout), float("nan"), device=DEV, dtype=torch.bfloat16)
            return _raw_conv(d, x, w, None, out, _workspace(need), need), out
    name, got = run({"GEMM_DMA16": 3})
    assert "gemm16_dma2_kernel" not in name, name
    name0, want = run({"GEMM_DMA16": 0, "IGEMM16_CFG": 0})
    assert "igemm16" in name0, name0
    assert torch.equal(got, want)
    # K is ordered (32-channel chunk, tap, channel)
    wr = w.double().view(Cout, Cin // 32, KH, 32).permute(0, 2, 1, 3).reshape(Cout, KH, Cin)
    ref = torch.einsum("ntc,otc->no", x[:, :KH, 0].double(), wr)
    assert torch.equal(got.view(Nimg, Cout).double(), ref.to(torch.bfloat16).double())
