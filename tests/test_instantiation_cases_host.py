"""The case tables of tests/_instantiation_cases.py reach every lane-group instantiation.  CPU only: like tests/test_abi.py this
calls nothing but host planner functions of the loaded library.  Every expected set below is written out by hand, so a row
deleted from a table fails here with the name of the instantiation that lost its case."""
from collections import Counter

from diff_sal_amd import _lib
from tests import _instantiation_cases as ic


def assert_same(got, expected, what):
    got, expected = Counter(got), Counter(expected)
    missing, extra = sorted((expected - got).elements()), sorted((got - expected).elements())
    assert not missing and not extra, f"{what}: no case left for {missing}; unexpected {extra}"


def test_mirrors_match_the_library_planners():
    """With 256 queries / rows the workgroup count of the backward planners equals G."""
    lib = _lib.load()
    for C, heads, _, _ in ic.ATTN_BWD_CASES:
        assert lib.diffsal_attention_bwd_blocks(256, C, heads) == ic.attention_g(C // heads), (C, heads)
    # the forward rule (attention_t in csrc/misc.hip) is a second copy of the same formula without a planner: the mirror
    # covers it by reading; its head dims go through the backward planner here as heads = 1 (any d % 4 == 0 is a valid C)
    for C, heads, _, _ in ic.ATTN_FWD_CASES:
        assert lib.diffsal_attention_bwd_blocks(256, C // heads, 1) == ic.attention_g(C // heads), (C, heads)
    assert_same(ic.LN_PAST_CAP, [(32, 8192 * 32 + 5)], "layernorm past the grid cap")
    assert_same(ic.LN_BWD_PAST_CAP, [(32, 1024 * 32 + 37), (768, 1024 * 4 + 3)], "layernorm_bwd past the grid cap")
    for C in ic.ROW_WIDTHS + tuple(c for c, _ in ic.LN_PAST_CAP + ic.LN_BWD_PAST_CAP):
        assert lib.diffsal_layernorm_bwd_blocks(256, C) == ic.row_dispatch(C)[0], C
    for C, M in ic.LN_BWD_PAST_CAP:
        G = ic.row_dispatch(C)[0]
        assert -(-M // (256 // G)) > ic.LN_BWD_GRID_CAP == lib.diffsal_layernorm_bwd_blocks(M, C), (C, M)
    for C, M in ic.LN_PAST_CAP:
        assert -(-M // (256 // ic.row_dispatch(C)[0])) > ic.LN_GRID_CAP
    assert ic.row_dispatch(ic.ROW_REJECTED_WIDTH) is None and ic.row_dispatch(ic.ROW_REJECTED_WIDTH - 4) == (64, 4)


ALL_ATTENTION = [(lk, g) for lk in ic.LK_BUCKETS for g in ic.ATTENTION_GS]


def check_attention_table(cases, head_rows, expected_rows, expected_raised, what):
    assert_same([c[:3] for c in cases if c[3]], expected_raised, f"{what}, raised LDS")
    assert_same({(ic.lk_bucket(Lk), ic.attention_g(C // h)) for C, h, Lk, _ in cases}, ALL_ATTENTION, f"{what} (LK, G)")
    # (G, fewest, most float4 pieces per lane, heads) of each (C, heads) row
    assert_same([(ic.attention_g(C // h),) + ic.attention_pieces(C // h) + (h,) for C, h in head_rows], expected_rows, f"{what} rows")
    # every row meets both edges of every key bucket
    for C, h in head_rows:
        assert_same([Lk for c, hh, Lk, _ in cases if (c, hh) == (C, h)], [1, 4, 5, 8, 9, 18, 19, 32], f"{what} C={C} heads={h} Lk")
    for C, h, Lk, raised in cases:
        lds = ic.attention_lds_bytes(C, h, Lk)
        assert C % h == 0 and (C // h) % 4 == 0 and 1 <= Lk <= 32
        if raised:
            assert ic.LDS_STATIC_LIMIT < lds <= ic.LDS_RAISED_LIMIT, f"{what} C={C} heads={h} Lk={Lk}: {lds} bytes of LDS is no raised launch"
        else:
            assert lds <= ic.LDS_STATIC_LIMIT, f"{what} C={C} heads={h} Lk={Lk}: {lds} bytes of LDS needs the raised mark"
    assert len(set(cases)) == len(cases) and len({ic.attention_id(c) for c in cases}) == len(cases)


def test_attention_forward_table_reaches_every_instantiation():
    check_attention_table(ic.ATTN_FWD_CASES, ic.ATTN_FWD_HEADS,
                          [(1, 4, 4, 2), (1, 5, 5, 3), (4, 1, 2, 2), (4, 2, 3, 4), (4, 3, 3, 2), (8, 3, 3, 2), (8, 3, 4, 2), (8, 4, 4, 1),
                           (16, 3, 3, 4), (16, 3, 4, 2), (16, 6, 6, 2)], [(768, 2, 32), (640, 1, 32)], "attention forward")
    exact = [c for c in ic.ATTN_FWD_CASES if ic.attention_lds_bytes(*c[:3]) == ic.LDS_RAISED_LIMIT]
    assert [ic.attention_id(c) for c in exact] == ["C640-h1-Lk32-lds160KiB"]
    assert ic.lk_bucket(32) == 32 and ic.attention_g(640) == 16


def test_attention_backward_table_reaches_every_instantiation():
    check_attention_table(ic.ATTN_BWD_CASES, ic.ATTN_BWD_HEADS,
                          [(1, 4, 4, 2), (1, 4, 4, 4), (4, 2, 2, 1), (4, 3, 3, 2), (4, 2, 3, 4), (8, 3, 3, 2), (8, 3, 4, 2), (8, 4, 4, 1),
                           (8, 3, 3, 4), (16, 3, 3, 2), (16, 3, 4, 2), (16, 3, 3, 4), (16, 6, 6, 2), (16, 3, 3, 1)], [(768, 2, 32)], "attention backward")
    assert all(C % 32 == 0 and h in (1, 2, 4) for C, h, _, _ in ic.ATTN_BWD_CASES)       # what the pass-2 GEMM and the entry accept
    # heads 1, 2 and 4 with every G each can reach (one head of a C % 32 == 0 row is at least 32 wide: never G = 1)
    assert_same({(h, ic.attention_g(C // h)) for C, h in ic.ATTN_BWD_HEADS},
                [(1, 4), (1, 8), (1, 16), (2, 1), (2, 4), (2, 8), (2, 16), (4, 1), (4, 4), (4, 8), (4, 16)], "attention backward (heads, G)")
    # the padded P / dS columns (ld > heads * Lk) of ops.attention_bwd
    padded = [(C, h, Lk) for C, h, Lk, _ in ic.ATTN_BWD_CASES if h * Lk % 4]
    assert len(padded) >= 3 and {(1, 5), (1, 9), (2, 19)} <= {(h, Lk) for _, h, Lk in padded}
    # end to end through autograd_ops.attention: two of the cases above, one ragged head dim and one one-head row, padded ld in both
    assert_same(ic.ATTN_AUTOGRAD, [(224, 2, 19), (32, 1, 5)], "attention autograd")
    for C, h, Lk in ic.ATTN_AUTOGRAD:
        assert (C, h, Lk, False) in ic.ATTN_BWD_CASES and h * Lk % 4


def test_row_table_reaches_every_instantiation_full_and_ragged():
    # (G, NV, lanes holding a float4 of the last piece): lanes == G is a full width
    assert_same([ic.row_dispatch(C) + (ic.row_last_piece_lanes(C),) for C in ic.ROW_WIDTHS],
                [(8, 1, 1), (8, 1, 5), (8, 1, 8), (16, 1, 9), (16, 1, 16), (32, 1, 17), (32, 1, 25), (32, 1, 32), (64, 1, 33), (64, 1, 50),
                 (64, 1, 64), (64, 2, 1), (64, 2, 32), (64, 2, 64), (64, 3, 1), (64, 3, 64), (64, 4, 1), (64, 4, 58), (64, 4, 64)], "row widths")
    for inst in ic.ROW_INSTANTIATIONS:
        mine = [C for C in ic.ROW_WIDTHS if ic.row_dispatch(C) == inst]
        assert any(ic.row_last_piece_lanes(C) == inst[0] for C in mine), f"rows {inst}: no full width"
        assert any(ic.row_last_piece_lanes(C) < inst[0] for C in mine), f"rows {inst}: no ragged width"
    for C in ic.ROW_WIDTHS:
        rows = 256 // ic.row_dispatch(C)[0]
        many, one = ic.row_counts(C)
        assert C % 4 == 0 and many > 2 * rows and many % rows and one == 1
    # the strip form of dwconv3_ln: taken and left per width, ragged last strip, and the first batch past its grid cap
    assert_same(ic.DWCONV_WS, [19, 15], "dwconv3_ln widths")
    assert 19 >= 16 > 15 and 19 % 8 == 3
    N, H, W, C = ic.DWCONV_STRIP_PAST_CAP
    strips_w = -(-W // 8)
    assert ic.row_dispatch(C) == (64, 1) and C <= 256 and W >= 16 and N % 2 == 0
    assert N * H * strips_w > ic.LN_GRID_CAP * 4 >= N * (H - 1) * strips_w and N // 2 * H * strips_w <= ic.LN_GRID_CAP * 4
    assert_same(ic.DWPOOL_KS, [1, 2, 3], "dwpool_ln_kv kernels")
    assert all(s % k for s in ic.DWPOOL_HW for k in ic.DWPOOL_KS if k > 1)


def test_pooling_table_reaches_every_instantiation():
    """The pooling rules (diffsal_pool3d_ln, diffsal_pool3d_bwd_data in csrc/mvit.hip) have no planner: mirrored by reading."""
    # (G, float4 lanes in use)
    assert_same([(ic.pool_g(D), D // 4) for D in ic.POOL_DS],
                [(8, 5), (8, 8), (16, 12), (16, 16), (32, 24), (32, 32), (64, 40), (64, 64)], "pooling widths")
    assert_same({ic.pool_g(D) for D in ic.POOL_DS}, ic.POOL_GS, "pooling G")
    # (temporal stride, NCS)
    assert_same([(s[0], ic.pool_ncs(s)) for s in ic.POOL_STRIDES], [(1, 3), (1, 2), (1, 1), (1, 0), (2, 2)], "pooling strides")
    assert all(D % 4 == 0 and D <= 256 for D in ic.POOL_DS)
