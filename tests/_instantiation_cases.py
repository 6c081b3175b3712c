"""Case tables for tests/test_gpu_instantiations.py, and Python mirrors of the host rules that pick a template
instantiation from a shape.  No torch, no GPU code: tests/test_instantiation_cases_host.py checks on the CPU that the
tables reach every instantiation (against the library's own planner functions where it has one).

A lane group of G lanes owns one row / token / (query, head) pair and holds NV float4 pieces of it:
  rows       csrc/norm.hip DS_ROW_DISPATCH, csrc/backward.hip DS_ROW_DISPATCH_B   C -> (G, NV)
  attention  csrc/misc.hip attention_t, csrc/backward.hip attention_g             head dim -> G, key count -> LK
  pooling    csrc/mvit.hip diffsal_pool3d_ln / diffsal_pool3d_bwd_data            D -> G, stride -> NCS
"""

# ---- mirrors of the dispatch rules -------------------------------------------------------------------------------------------

ROW_INSTANTIATIONS = ((8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4))
LK_BUCKETS = (4, 8, 18, 32)
ATTENTION_GS = (1, 4, 8, 16)
POOL_GS = (8, 16, 32, 64)
LDS_STATIC_LIMIT = 64 * 1024      # above this the launcher raises the kernel's dynamic LDS limit ...
LDS_RAISED_LIMIT = 160 * 1024     # ... to this, the most the entry points accept


def row_dispatch(C):
    """DS_ROW_DISPATCH / DS_ROW_DISPATCH_B: width -> (G, NV); None past 1024 channels (the entry refuses)."""
    c4 = C // 4
    for limit, inst in zip((8, 16, 32, 64, 128, 192, 256), ROW_INSTANTIATIONS):
        if c4 <= limit:
            return inst
    return None


def row_last_piece_lanes(C):
    """Lanes that hold a float4 in the LAST of the NV pieces: G = full, fewer = a ragged width."""
    G, NV = row_dispatch(C)
    return C // 4 - G * (NV - 1)


def attention_g(d):
    """Lanes per (query, head) for head dim d: about 3 float4 pieces per lane, at most 16 lanes, never 2."""
    nf4 = d // 4
    G = 1
    while G < 16 and nf4 // (2 * G) >= 3:
        G *= 2
    return 4 if G == 2 else G


def attention_pieces(d):
    """(fewest, most) float4 pieces of the head dim that a lane of the group holds: unequal = a ragged head dim."""
    G, nf4 = attention_g(d), d // 4
    return nf4 // G, -(-nf4 // G)


def lk_bucket(Lk):
    for b in LK_BUCKETS:
        if Lk <= b:
            return b
    return None


def attention_lds_bytes(C, heads, Lk):
    return 2 * Lk * (C // heads) * 4


def attention_lq(d):
    """Queries per image: two full workgroups of 256 / G queries and a ragged third."""
    return 2 * (256 // attention_g(d)) + 3


def pool_g(D):
    return 8 if D <= 32 else 16 if D <= 64 else 32 if D <= 128 else 64


def pool_ncs(stride):
    """pool3d_bwd_data: candidate taps per spatial axis; 0 = all 27 taps tried (unequal spatial strides)."""
    _, sh, sw = stride
    if sh != sw:
        return 0
    return 3 if sh == 1 else 2 if sh == 2 else 1


# ---- attention -----------------------------------------------------------------------------------------------------------------

LK_EDGES = (1, 4, 5, 8, 9, 18, 19, 32)          # both edges of every key bucket

# (C, heads) of the forward: every G with a head dim whose float4 count is and is not a multiple of G, heads 1 .. 4
ATTN_FWD_HEADS = (
    (32, 2),      # d = 16   G = 1
    (60, 3),      # d = 20   G = 1, nf4 = 5
    (48, 2),      # d = 24   G = 4, lanes hold 2, 2, 1, 1
    (160, 4),     # d = 40   G = 4, lanes hold 3, 3, 2, 2
    (96, 2),      # d = 48   G = 4
    (192, 2),     # d = 96   G = 8
    (224, 2),     # d = 112  G = 8, ragged
    (128, 1),     # d = 128  G = 8
    (768, 4),     # d = 192  G = 16
    (416, 2),     # d = 208  G = 16, ragged
    (768, 2),     # d = 384  G = 16
)
# (C, heads, Lk) whose K | V of one head exceed 64 KiB of LDS: the raised-limit launch
ATTN_FWD_RAISED = (
    (768, 2, 32),     # 98304 bytes
    (640, 1, 32),     # 163840 bytes = 160 KiB exactly: the largest the entry accepts
)

# backward: the pass-2 GEMM needs C % 32 == 0; heads 1, 2 and 4 with every G each can reach
ATTN_BWD_HEADS = (
    (32, 2),      # d = 16   G = 1
    (64, 4),      # d = 16   G = 1
    (32, 1),      # d = 32   G = 4
    (96, 2),      # d = 48   G = 4
    (160, 4),     # d = 40   G = 4, ragged
    (192, 2),     # d = 96   G = 8: the model's C = 192 stage
    (224, 2),     # d = 112  G = 8, ragged
    (128, 1),     # d = 128  G = 8
    (384, 4),     # d = 96   G = 8 with four heads
    (384, 2),     # d = 192  G = 16
    (416, 2),     # d = 208  G = 16, ragged
    (768, 4),     # d = 192  G = 16
    (768, 2),     # d = 384  G = 16
    (192, 1),     # d = 192  G = 16 with one head
)
ATTN_BWD_RAISED = ((768, 2, 32),)
# two of the above, end to end through autograd_ops.attention
ATTN_AUTOGRAD = ((224, 2, 19), (32, 1, 5))


def _attention_cases(head_rows, raised):
    cases = [(C, h, Lk, (C, h, Lk) in raised) for C, h in head_rows for Lk in LK_EDGES]
    have = {c[:3] for c in cases}
    return tuple(cases + [(C, h, Lk, True) for C, h, Lk in raised if (C, h, Lk) not in have])


# (C, heads, Lk, raised)
ATTN_FWD_CASES = _attention_cases(ATTN_FWD_HEADS, ATTN_FWD_RAISED)
ATTN_BWD_CASES = _attention_cases(ATTN_BWD_HEADS, ATTN_BWD_RAISED)


def attention_id(case):
    C, h, Lk, raised = case
    if attention_lds_bytes(C, h, Lk) == LDS_RAISED_LIMIT:
        return f"C{C}-h{h}-Lk{Lk}-lds160KiB"
    return f"C{C}-h{h}-Lk{Lk}" + ("-raised" if raised else "")


# ---- row family ----------------------------------------------------------------------------------------------------------------

ROW_WIDTHS = (4, 20, 32, 36, 64, 68, 100, 128, 132, 200, 256, 260, 384, 512, 516, 768, 772, 1000, 1024)
ROW_REJECTED_WIDTH = 1028                      # first width past (64, 4): refused before any launch


def row_counts(C):
    """Row counts per width: not a multiple of the 256 / G rows of a workgroup (two full workgroups and a ragged third), and 1."""
    return (2 * (256 // row_dispatch(C)[0]) + 3, 1)


LN_GRID_CAP = 8192          # csrc/norm.hip row_grid
LN_BWD_GRID_CAP = 1024      # diffsal_layernorm_bwd_blocks
# past the grid caps: (C, M)
LN_PAST_CAP = ((32, LN_GRID_CAP * 32 + 5),)
LN_BWD_PAST_CAP = ((32, LN_BWD_GRID_CAP * 32 + 37), (768, LN_BWD_GRID_CAP * 4 + 3))
# dwconv3_ln strip kernel, G = 64 (4 strips of 8 pixels per workgroup): (N, H, W, C) whose strip count first exceeds 8192 * 4
DWCONV_STRIP_PAST_CAP = (4, 2731, 19, 132)

DWCONV_WS = (19, 15)        # 19: strip kernel for C <= 256, ragged last strip of 3; 15: generic kernel
DWCONV_NH = (2, 5)
DWPOOL_KS = (1, 2, 3)
DWPOOL_HW = (5, 7)


# ---- MViT pooling --------------------------------------------------------------------------------------------------------------

POOL_DS = (20, 32, 48, 64, 96, 128, 160, 256)
POOL_STRIDES = ((1, 1, 1), (1, 2, 2), (1, 4, 4), (1, 2, 4), (2, 2, 2))
POOL_B, POOL_HEADS, POOL_SIZE = 2, 2, (3, 5, 7)
