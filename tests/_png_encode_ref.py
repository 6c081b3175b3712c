"""The PNG export restated in NumPy (include/diffsal.h, "PNG export"): an 8-bit map -> the complete file, byte for byte what
csrc/png_encode.hip and tools/png_encode_host_check.cpp write.  The file's bytes are a function of the pixels alone; this module is
their definition outside the C++ header.  It counts what its inputs exercise (``new_counters``), so that the fixture's case set can
be held to its coverage.  The fixtures (tests/golden/png_encode.npz) are inputs, this module's files and the counters, written by
tools/gen_png_encode_golden.py."""
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_encode.npz")
SEGMENT = 16384
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
COUNTERS = ("filter0", "filter1", "filter2", "filter3", "filter4", "match258", "remainder1", "remainder2", "previous_segment", "limit15",
            "limit7", "rep16", "rep17", "rep18", "full_segment", "segment_of_1")


def new_counters():
    return dict.fromkeys(COUNTERS, 0)


def capacity(H: int, W: int) -> int:
    """diffsal_png_encode_capacity: 15 bits per stream byte, 4092 header bits and a 15-bit end symbol per block, 63 bytes of
    framing, rounded up to 16"""
    S = H * (W + 1)
    nseg = -(-S // SEGMENT)
    return (63 + (15 * S + 4107 * nseg + 7) // 8 + 15) & ~15


# ---- filters (PNG 9.2) on the raw neighbours ------------------------------------------------------------------------------------
def filtered(img: np.ndarray, ctr=None):
    """uint8 [H, W] -> (the filtered scanlines uint8 [H * (W + 1)], the filter of every row)"""
    x = img.astype(np.int32)
    a = np.zeros_like(x)
    a[:, 1:] = x[:, :-1]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 1:] = x[:-1, :-1]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255      # [5, H, W]
    cost = np.minimum(cand, 256 - cand).sum(axis=2)                               # [5, H]
    f = np.argmin(cost, axis=0)                                                   # the first of the least: a tie goes to the lowest
    H, W = img.shape
    out = np.empty((H, W + 1), dtype=np.uint8)
    out[:, 0] = f
    out[:, 1:] = cand[f, np.arange(H)]
    if ctr is not None:
        for k in range(5):
            ctr[f"filter{k}"] += int((f == k).sum())
    return out.reshape(-1), f


# ---- tokens: distance 1 only ----------------------------------------------------------------------------------------------------
def tokens(d: np.ndarray, prev, ctr=None):
    """the segment's bytes d (prev: the stream byte in front of it, None at the stream's start) -> (position, literal or -1,
    match length or 0) of every token, in order"""
    n = d.size
    idx = np.arange(n)
    eq = np.zeros(n, dtype=bool)
    eq[1:] = d[1:] == d[:-1]
    if prev is not None:
        eq[0] = d[0] == prev
    s = np.maximum.accumulate(np.where(eq, -1, idx)) + 1                    # the run's first position
    e = np.minimum.accumulate(np.where(eq, n, idx)[::-1])[::-1]             # behind its last
    L, o = e - s, idx - s
    rem = L - 258 * (o // 258)                                              # what is left of the run at this piece's start
    piece = eq & (L >= 3) & (rem >= 3)
    start = piece & (o % 258 == 0)
    take = ~piece | start
    pos = idx[take]
    lit = np.where(start, -1, d.astype(np.int64))[take]
    length = np.where(start, np.minimum(rem, 258), 0)[take]
    if ctr is not None:
        first = eq & (idx == s) & (L >= 3)                                  # a run that is coded with matches, once
        ctr["match258"] += int((length == 258).sum())
        ctr["remainder1"] += int((first & (L % 258 == 1)).sum())
        ctr["remainder2"] += int((first & (L % 258 == 2)).sum())
        ctr["previous_segment"] += int(prev is not None and bool(start[0]))
    return pos, lit, length


def length_symbol(length: int):
    """match length 3..258 -> (symbol, extra bits, their value)"""
    if length == 258:
        return 285, 0, 0
    if length < 11:
        return 254 + length, 0, 0
    v = length - 3
    e = v.bit_length() - 3
    return 257 + 4 * e + (v >> e), e, v & ((1 << e) - 1)


# ---- length-limited canonical codes ---------------------------------------------------------------------------------------------
def limited_lengths(counts, limit: int):
    """Code lengths from symbol counts, complete (Kraft sum exactly 1), none above ``limit``.  Symbols with a count, and symbols 0
    and 1 as well if fewer than two have one, in ascending order of (count, symbol); Huffman's tree by the two-queue
    method, a leaf before an internal node of equal weight; the tree's count of codes per length, lengths above the limit folded
    into it and the Kraft sum repaired by moving the deepest code that can move one level down (miniz's rule); then the lengths
    are handed out along the order, the longest to the rarest.  Returns (lengths, whether the limit changed anything)."""
    n = len(counts)
    used = [i for i in range(n) if counts[i]]
    if len(used) < 2:
        used = sorted(set(used) | {0, 1})
    order = sorted(used, key=lambda i: (counts[i], i))
    m = len(order)
    w = [counts[i] for i in order] + [0] * (m - 1)
    parent = [0] * (2 * m - 1)
    leaf, inner = 0, m
    for node in range(m, 2 * m - 1):
        for _ in range(2):
            if leaf < m and (inner >= node or w[leaf] <= w[inner]):
                k, leaf = leaf, leaf + 1
            else:
                k, inner = inner, inner + 1
            w[node] += w[k]
            parent[k] = node
    depth = [0] * (2 * m - 1)
    for node in range(2 * m - 3, -1, -1):
        depth[node] = depth[parent[node]] + 1
    num = [0] * (max(m, limit + 1) + 1)
    for k in range(m):
        num[depth[k]] += 1
    limited = max(depth[:m]) > limit
    if limited:
        for i in range(limit + 1, len(num)):
            num[limit] += num[i]
            num[i] = 0
        total = sum(num[i] << (limit - i) for i in range(1, limit + 1))
        while total != 1 << limit:
            num[limit] -= 1
            for i in range(limit - 1, 0, -1):
                if num[i]:
                    num[i] -= 1
                    num[i + 1] += 2
                    break
            total -= 1
    lens = [0] * n
    r = 0
    for length in range(limit, 0, -1):
        for _ in range(num[length]):
            lens[order[r]] = length
            r += 1
    assert r == m and sum(1 << (limit - v) for v in lens if v) == 1 << limit
    return lens, limited


def canonical(lens):
    """RFC 1951 3.2.2: symbol -> its code, bit-reversed (the stream takes a code's first bit first)"""
    count = [0] * 16
    for v in lens:
        count[v] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lens)
    for i, v in enumerate(lens):
        if v:
            out[i] = int(format(nxt[v], f"0{v}b")[::-1], 2)
            nxt[v] += 1
    return out


def run_lengths(seq, ctr=None):
    """the code lengths as (code-length symbol, extra bits, their value): a run of zeros in pieces of 138 (18) while 11 or more
    are left, then 17 for 3..10, else zeros; another value once, then 16 in pieces of 6 while 3 or more are left, then the value"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, j = seq[i], i
        while j < n and seq[j] == v:
            j += 1
        L, i = j - i, j
        if v == 0:
            while L >= 11:
                c = min(L, 138)
                out.append((18, 7, c - 11))
                L -= c
            if L >= 3:
                out.append((17, 3, L - 3))
                L = 0
        else:
            out.append((v, 0, 0))
            L -= 1
            while L >= 3:
                c = min(L, 6)
                out.append((16, 2, c - 3))
                L -= c
        out.extend([(v, 0, 0)] * L)
    if ctr is not None:
        for k in (16, 17, 18):
            ctr[f"rep{k}"] += sum(1 for s, _, _ in out if s == k)
    return out


def block(d: np.ndarray, prev, final: bool, ctr=None):
    """one segment -> (values, bit counts) of everything the block puts into the stream, in order"""
    pos, lit, length = tokens(d, prev, ctr)
    sym = lit.copy()
    ebits = np.zeros(sym.size, dtype=np.int64)
    eval_ = np.zeros(sym.size, dtype=np.int64)
    for k in np.flatnonzero(length):
        sym[k], ebits[k], eval_[k] = length_symbol(int(length[k]))
    counts = np.bincount(sym, minlength=286).tolist()
    counts[256] += 1
    lens, lim15 = limited_lengths(counts, 15)
    codes = canonical(lens)
    nlen = max(257, max(i for i in range(286) if lens[i]) + 1)
    rl = run_lengths(lens[:nlen] + [1], ctr)      # one distance code: symbol 0, length 1
    ccount = [0] * 19
    for s, _, _ in rl:
        ccount[s] += 1
    clens, lim7 = limited_lengths(ccount, 7)
    ccodes = canonical(clens)
    ncl = max(4, max(k for k in range(19) if clens[CLEN_ORDER[k]]) + 1)
    vals, bits = [1 if final else 0, 2, nlen - 257, 0, ncl - 4], [1, 2, 5, 5, 4]
    for k in range(ncl):
        vals.append(clens[CLEN_ORDER[k]])
        bits.append(3)
    for s, eb, ev in rl:
        vals.append(ccodes[s] | (ev << clens[s]))
        bits.append(clens[s] + eb)
    assert sum(bits) <= 4092
    lens_a, codes_a = np.asarray(lens, dtype=np.int64), np.asarray(codes, dtype=np.int64)
    match = length > 0
    tv = codes_a[sym] | (eval_ << lens_a[sym])               # the code, the extra bits, and for a match the distance code: one 0 bit
    tb = lens_a[sym] + ebits + match
    vals = np.concatenate([np.asarray(vals, dtype=np.int64), tv, [codes[256]]])
    bits = np.concatenate([np.asarray(bits, dtype=np.int64), tb, [lens[256]]])
    if ctr is not None:
        ctr["limit15"] += int(lim15)
        ctr["limit7"] += int(lim7)
        ctr["full_segment"] += int(d.size == SEGMENT)
        ctr["segment_of_1"] += int(d.size == 1)
    return vals, bits


def deflate(stream: np.ndarray, ctr=None) -> bytes:
    vals, bits = [], []
    for at in range(0, stream.size, SEGMENT):
        v, b = block(stream[at:at + SEGMENT], int(stream[at - 1]) if at else None, at + SEGMENT >= stream.size, ctr)
        vals.append(v)
        bits.append(b)
    vals, bits = np.concatenate(vals), np.concatenate(bits)
    offs = np.cumsum(bits) - bits
    out = np.zeros((int(bits.sum()) + 7) // 8 * 8, dtype=np.uint8)
    for k in range(int(bits.max())):
        m = bits > k
        out[offs[m] + k] = (vals[m] >> k) & 1
    return np.packbits(out, bitorder="little").tobytes()


def _chunk(kind: bytes, payload: bytes) -> bytes:
    return len(payload).to_bytes(4, "big") + kind + payload + zlib.crc32(kind + payload).to_bytes(4, "big")


def adler32(data: np.ndarray) -> int:
    a, b = 1, 0
    for at in range(0, data.size, 4096):
        part = data[at:at + 4096].astype(np.int64)
        b = (b + part.size * a + int((np.arange(part.size, 0, -1) * part).sum())) % 65521
        a = (a + int(part.sum())) % 65521
    return (b << 16) | a


def encode(img: np.ndarray, ctr=None) -> bytes:
    """the file of the uint8 [H, W] map"""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2 and 1 <= img.shape[1] <= 8192 and 1 <= img.shape[0] <= 65535
    H, W = img.shape
    stream, _ = filtered(img, ctr)
    idat = b"\x78\x01" + deflate(stream, ctr) + adler32(stream).to_bytes(4, "big")
    ihdr = W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes([8, 0, 0, 0, 0])
    out = SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", idat) + _chunk(b"IEND", b"")
    assert len(out) == 57 + len(idat) <= capacity(H, W)
    return out


def saliency_like(seed: int, H: int, W: int, blobs: int = 4, noise: int = 0) -> np.ndarray:
    """a flat background with Gaussian blobs, quantised like a prediction (max 255, min 0); `noise`: uniform noise of that
    amplitude on top.  A seeded formula: the tests make their full-size maps with it instead of storing them"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    m = np.zeros((H, W))
    for _ in range(blobs):
        cy, cx = rng.uniform(0.15, 0.85) * H, rng.uniform(0.15, 0.85) * W
        s = rng.uniform(0.04, 0.12) * max(H, W)
        m += rng.uniform(0.3, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    m = np.maximum(m - 0.05, 0.0)
    if noise:
        m += rng.uniform(0, noise / 255.0, size=m.shape)
    m = (m - m.min()) / (m.max() - m.min())
    return np.floor(m * 255.0 + 0.5).astype(np.uint8)


def load_cases(path: str = GOLDEN):
    """{name: dict(img uint8 [H, W], file bytes)}, the recorded counters"""
    z = np.load(path)
    names = [str(n) for n in z["names"]]
    cases = {n: dict(img=z[f"img_{k}"], file=z[f"file_{k}"].tobytes()) for k, n in enumerate(names)}
    return cases, {str(n): int(v) for n, v in zip(z["counter_names"], z["counters"])}
