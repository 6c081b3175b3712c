"""The exact-operand references of tests/_exact_ref.py, checked without a GPU, for every case table of
tests/test_gpu_exact_products.py:

  * conditions (a) - (c): magnitudes below 2^24, nothing beyond fp16's range, and enough power -- at least 2 % of a 16-bit case's
    outputs are rounding ties and at least 10 % need rounding;
  * the fp64 reference equals an fp32 torch evaluation in two different summation orders: order really does not matter;
  * two mutations of the reference -- the store truncates, one k index is dropped -- change at least 1 % of the outputs, so a kernel
    with either fault cannot match.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import _exact_ref as E

SPECS = E.all_conv_specs()


def _id(c):
    return f"{c.dname}-{'x'.join(map(str, c.xshape))}-{c.Cout}-k{c.k}s{c.stride}p{c.pad}d{c.dil}-{'+'.join(c.epi) or 'none'}-r{c.r}-{c.seed}"


def _two_orders(x, w, c):
    """fp32 sums: the whole K at once, and three channel chunks, last first, added up in fp32."""
    x32, w32 = x.float(), w.float()
    a = E._conv64(x32, w32, c)
    Cin = c.xshape[3]
    cuts = [0, Cin // 3, 2 * Cin // 3, Cin]
    b = None
    for lo, hi in reversed(list(zip(cuts[:-1], cuts[1:]))):
        part = E._conv64(x32[..., lo:hi].flip(-1), w32[:, lo:hi].flip(1), dataclass_with(c, hi - lo))
        b = part if b is None else b + part
    return a, b


def dataclass_with(c, Cin):
    import dataclasses

    return dataclasses.replace(c, xshape=(*c.xshape[:3], Cin), out_hw=c.hw())


def _share(a, b):
    return (a != b).double().mean().item()


@pytest.mark.parametrize("c", SPECS, ids=[_id(c) for c in SPECS])
def test_forward_case_is_exact_and_has_power(c):
    p = E.problem(c)
    ties, inexact = E.conditions(p.exact, E.magnitude_bound(p), c.dname, _id(c))
    print(f"{_id(c)}: bound {E.magnitude_bound(p):.3g}, {ties:.1%} ties, {inexact:.1%} inexact")
    if c.dname != "fp32":
        E.to_storage(p.x, c.dname), E.to_storage(p.w, c.dname)
    for acc32 in _two_orders(p.x, p.w, c):
        assert acc32.dtype == torch.float32
        assert torch.equal(E.epilogue(acc32, p).double(), p.exact)
    # mutation 1: truncation instead of round-to-nearest-even
    if c.dname != "fp32":
        assert _share(E.truncate_store(p.exact, c.dname), p.ref) >= 0.01
    # mutation 2: one k index (a channel of one tap) never reaches the sum
    ci, tap = c.xshape[3] // 2, (c.k * c.k) // 2
    wm = torch.zeros_like(p.w[:, ci:ci + 1])
    wm.view(c.Cout, -1)[:, tap] = p.w[:, ci].reshape(c.Cout, -1)[:, tap]
    lost = E._conv64(p.x[..., ci:ci + 1].contiguous(), wm, dataclass_with(c, 1))
    assert _share(E.round_store(E.epilogue(p.acc - lost, p), c.dname), p.ref) >= 0.01


def test_rounding_analysis_on_known_values():
    v = torch.tensor([257.0, 258.0, 259.0, 513.0, 514.0, 515.0, -257.0, 0.0, 3.0])
    assert E.is_tie(v.double(), "bf16").tolist() == [True, False, True, False, True, False, True, False, False]
    assert E.round_store(v.double(), "bf16").tolist() == [256.0, 258.0, 260.0, 512.0, 512.0, 516.0, -256.0, 0.0, 3.0]
    assert E.truncate_store(v.double(), "bf16").tolist() == [256.0, 258.0, 258.0, 512.0, 512.0, 512.0, -256.0, 0.0, 3.0]
    h = torch.tensor([2049.0, 2051.0, 4098.0, 4100.0, 1000.5]).double()
    assert E.is_tie(h, "fp16").tolist() == [True, True, True, False, False]
    assert E.round_store(h, "fp16").tolist() == [2048.0, 2052.0, 4096.0, 4100.0, 1000.5]
    with pytest.raises(AssertionError):
        E.to_storage(torch.tensor([257.0]), "bf16")
    with pytest.raises(AssertionError, match="1 of 2 outputs differ"):
        E.check_equal(torch.tensor([256.0, 260.0]).bfloat16(), torch.tensor([256.0, 258.0]).bfloat16(), "x", torch.tensor([257.0, 259.0]).double(), "bf16")


def test_pack_k_order_is_chunk_tap_channel():
    w = torch.arange(2 * 64 * 9, dtype=torch.float64).reshape(2, 64, 3, 3)
    pk = E.pack_k_order(w)
    for co, ci, a, b in ((0, 0, 0, 0), (1, 33, 2, 1), (0, 63, 1, 2)):
        assert pk[co, (ci // 32) * 9 * 32 + (a * 3 + b) * 32 + ci % 32] == w[co, ci, a, b]


@pytest.mark.parametrize("case", [(N, Cin, Cout, *hw, dil, ("bias", "bn", "relu"), 600 + i) for i, (N, Cin, Cout, hw, dil) in enumerate(E.TAPSUM_CASES)]
                         + [(N, Cin, Cout, 2 * h, 2 * w, 2, ("bn", "relu"), 620 + i) for i, (N, h, w, Cin, Cout) in enumerate(E.UP2_CASES)],
                         ids=str)
def test_up2_case_is_exact(case):
    N, Cin, Cout, H, W, dil, epi, seed = case
    p = E.up2_problem(N, H // 2, W // 2, Cin, Cout, dil, epi, seed)
    assert p.bound < E.LIMIT
    up32 = p.up.float()
    a = F.conv2d(up32, p.wt.float(), None, padding=dil, dilation=dil).permute(0, 2, 3, 1)
    b = F.conv2d(up32.flip(1), p.wt.float().flip(1), None, padding=dil, dilation=dil).permute(0, 2, 3, 1)
    for acc32 in (a, b):
        assert torch.equal(E.epilogue(acc32.contiguous(), p).double(), p.exact)
    wm = p.wt.clone()
    wm[:, Cin // 2, 1, 1] = 0
    mut = E.epilogue(F.conv2d(p.up, wm, None, padding=dil, dilation=dil).permute(0, 2, 3, 1), p)
    assert _share(mut, p.exact) >= 0.01


WGRADS = [(1, 1, M, K, N, 1, 640 + i) for i, (M, K, N) in enumerate(E.WGRAD_SHAPES)] + [(*E.WGRAD_CONV, 3, 650)]


@pytest.mark.parametrize("case", WGRADS, ids=str)
def test_wgrad_case_is_exact(case):
    N, H, W, Cin, Cout, k, seed = case
    p = E.wgrad_problem(*case)
    assert p.bound < E.LIMIT and 4.0 * N * H * W < E.LIMIT
    xs, dys = p.x.float().permute(0, 3, 1, 2), p.dy.float().permute(0, 3, 1, 2)
    a = torch.nn.grad.conv2d_weight(xs, (Cout, Cin, k, k), dys, padding=k // 2)
    b = torch.nn.grad.conv2d_weight(xs.flip(0, 2, 3), (Cout, Cin, k, k), dys.flip(0, 2, 3), padding=k // 2).flip(2, 3)   # rows in reverse
    assert torch.equal(E.pack_k_order(a).double(), p.dw) and torch.equal(E.pack_k_order(b).double(), p.dw)
    assert torch.equal(p.dy.float().reshape(-1, Cout).flip(0).sum(0).double(), p.db)
    # one row (pixel) dropped from the sums
    xm = p.x.clone()
    xm[N - 1, H // 2, W // 2] = 0
    mut = E.pack_k_order(torch.nn.grad.conv2d_weight(xm.permute(0, 3, 1, 2), (Cout, Cin, k, k), p.dy.permute(0, 3, 1, 2), padding=k // 2))
    assert _share(mut, p.dw) >= 0.01


@pytest.mark.parametrize("case", E.BACKWARD_CASES, ids=str)
def test_backward_case_is_exact(case):
    p = E.backward_problem(case)
    assert p.bound < E.LIMIT
    for flip in (False, True):
        q = E.backward_problem(case, torch.float32, flip)
        for name in ("y", "dx", "dw", "db", "drv"):
            assert torch.equal(getattr(q, name).double(), getattr(p, name)), (name, flip)
    if case[-1]:       # the ReLU mask matters: a share of the outputs is clipped, and a share is exactly zero
        assert (p.y == 0).double().mean().item() > 0.3


def test_linear_backward_and_reductions_are_exact():
    p = E.linear_backward_problem()
    assert p.bound < E.LIMIT
    for flip in (False, True):
        q = E.linear_backward_problem(torch.float32, flip)
        for name in ("y", "dx", "dw", "db", "dr"):
            assert torch.equal(getattr(q, name).double(), getattr(p, name)), (name, flip)
    for case in E.SEGMENTED_CASES:
        s_ = E.segmented_problem(*case)
        segments, rows, K, Cout = case
        assert s_.bound < E.LIMIT
        got = torch.stack([s_.dy.float()[i * rows:(i + 1) * rows].flip(0).t() @ s_.x.float()[i * rows:(i + 1) * rows].flip(0) for i in range(segments)])
        assert torch.equal(got.double(), s_.out)
        assert _share(torch.einsum("srn,srk->snk", s_.dy.view(segments, rows, Cout)[:, 1:], s_.x.view(segments, rows, K)[:, 1:]), s_.out) >= 0.01
    for case in E.COLSUM_CASES:
        c_ = E.colsum_problem(*case)
        M, C, seg = case
        assert c_.bound < E.LIMIT
        assert torch.equal(c_.dy.float().view(M // seg, seg, C).flip(1).sum(1).double(), c_.out)
        assert _share(c_.dy.view(M // seg, seg, C)[:, 1:].sum(1), c_.out) >= 0.01


@pytest.mark.parametrize("case", E.WINO_CASES, ids=str)
def test_winograd_case_is_exact(case):
    """F(4x4, 3x3) with integer U and x in {-1, 0, 1}: the textbook evaluation A^T [(U . V)] A in fp32, with the kernel's own
    matrices, gives 576 x the convolution exactly, and the magnitude bound of every sum on the way is below 2^24."""
    N, H, W, Cin, Cout, dil = case
    p = E.wino_problem(*case)
    print(f"winograd {case}: bound {p.bound:.4g} of {E.LIMIT:.4g}")
    assert p.bound < E.LIMIT
    assert p.U.abs().max().item() <= 576 and torch.equal(p.U, p.U.round())
    BT, AT = torch.tensor(E.WINO_BT, dtype=torch.float32), torch.tensor(E.WINO_AT, dtype=torch.float32)
    xs = p.x.float().permute(0, 3, 1, 2)
    out = torch.zeros(N, H, W, Cout)
    U = p.U.float().reshape(6, 6, Cout, Cin)
    for py in range(dil):
        for px in range(dil):
            sub = xs[:, :, py::dil, px::dil]
            h, w_ = sub.shape[2:]
            ty, tx = (h + 3) // 4, (w_ + 3) // 4
            tiles = F.pad(sub, (1, 4 * tx + 1 - w_, 1, 4 * ty + 1 - h)).unfold(2, 6, 4).unfold(3, 6, 4)
            V = torch.einsum("ia,nctxab,jb->ntxijc", BT, tiles, BT)
            Mm = torch.einsum("ntxijc,ijoc->ntxijo", V, U)
            Y = torch.einsum("ai,ntxijo,bj->ntaxbo", AT, Mm, AT).reshape(N, 4 * ty, 4 * tx, Cout)
            out[:, py::dil, px::dil] = Y[:, :h, :w_]
    assert torch.equal(out.double(), p.exact)
