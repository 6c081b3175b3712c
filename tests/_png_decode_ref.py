"""NumPy / pure-Python restatement of the PNG decode (include/diffsal.h, "PNG decode", (a)-(e)): its own chunk walk, its own inflate
of RFC 1951 (bit by bit, canonical codes, no look-up), the five filters, sample unpacking, the palette, Pillow's RGB and L, Adler-32
and the status bits, with counters of what a file exercises.  No diff_sal_amd, no zlib, no PIL: the fixtures
(tests/golden/png_decode.npz) are files and Pillow's pixels, written by tools/gen_png_decode_golden.py."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_decode.npz")

BAD_BLOCK, BAD_STORED, BAD_LENGTHS, BAD_SYMBOL, BAD_DISTANCE, NO_INPUT, SHORT, LONG, BAD_FILTER, BAD_ADLER = (1 << k for k in range(10))
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
COUNTERS = ("stored", "fixed", "dynamic", "rep16", "rep17", "rep18", "long_code", "overlap", "max_distance", "filter0", "filter1", "filter2",
            "filter3", "filter4", "type0", "type2", "type3", "type4", "type6", "depth1", "depth2", "depth4", "depth8")
_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385,
          24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def new_counters():
    return dict.fromkeys(COUNTERS, 0)


def chunks(data: bytes):
    """[(type, payload)] of a PNG file, the signature checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at + 8 <= len(data):
        n = int.from_bytes(data[at:at + 4], "big")
        out.append((data[at + 4:at + 8], data[at + 8:at + 8 + n]))
        at += 12 + n
        if out[-1][0] == b"IEND":
            break
    return out


def header(data: bytes) -> dict:
    """H, W, color_type, bit_depth, stream (the IDAT payloads joined), palette (768 bytes, zero-padded)"""
    d = dict(palette=bytes(768))
    parts = []
    for kind, p in chunks(data):
        if kind == b"IHDR":
            d.update(W=int.from_bytes(p[0:4], "big"), H=int.from_bytes(p[4:8], "big"), bit_depth=p[8], color_type=p[9])
        elif kind == b"PLTE":
            d["palette"] = (p[:768] + bytes(768))[:768]
        elif kind == b"IDAT":
            parts.append(p)
    d["stream"] = b"".join(parts)
    return d


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


class _Bits:
    def __init__(self, data: bytes):
        self.data, self.pos, self.total = data, 0, 8 * len(data)

    def get(self, n: int) -> int:
        v = 0
        for k in range(n):
            if self.pos >= self.total:
                raise _Stop(NO_INPUT)
            v |= ((self.data[self.pos >> 3] >> (self.pos & 7)) & 1) << k
            self.pos += 1
        return v


def _table(lens, allow_empty=False, complete_only=False):
    """canonical code: (count per length, symbols in code order); zlib's rules for what is refused: an over-subscribed set, an
    incomplete one unless it is a single 1-bit code, and any incomplete code-length code (``complete_only``)"""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    left, maxlen = 1, 0
    for n in range(1, 16):
        left = (left << 1) - count[n]
        if left < 0:
            raise _Stop(BAD_LENGTHS)
        if count[n]:
            maxlen = n
    if maxlen == 0:
        if not allow_empty:
            raise _Stop(BAD_LENGTHS)
    elif left > 0 and (complete_only or maxlen != 1):
        raise _Stop(BAD_LENGTHS)
    symbols = [s for n in range(1, 16) for s, ln in enumerate(lens) if ln == n]
    return count, symbols


def _symbol(bits: _Bits, table, ctr=None, bad=BAD_SYMBOL) -> int:
    count, symbols = table
    code = first = index = 0
    for n in range(1, 16):
        code |= bits.get(1)
        if code - count[n] < first:
            if ctr is not None and n > 9:
                ctr["long_code"] += 1
            return symbols[index + code - first]
        index += count[n]
        first = (first + count[n]) << 1
        code <<= 1
    raise _Stop(bad)


def inflate(stream: bytes, want: int, ctr=None):
    """The zlib stream -> (bytearray of at most ``want`` bytes, status, Adler-32 of the stream's trailer or None).  Stops at the
    first error, as the device does."""
    ctr = new_counters() if ctr is None else ctr
    out = bytearray()
    bits = _Bits(stream)
    status, adler = 0, None
    try:
        bits.get(16)
        fixed = None
        while True:
            last, kind = bits.get(1), bits.get(2)
            if kind == 3:
                raise _Stop(BAD_BLOCK)
            if kind == 0:
                ctr["stored"] += 1
                bits.get(-bits.pos & 7)
                n, nn = bits.get(16), bits.get(16)
                if n ^ 0xFFFF != nn:
                    raise _Stop(BAD_STORED)
                for _ in range(n):
                    v = bits.get(8)
                    if len(out) >= want:
                        raise _Stop(LONG)
                    out.append(v)
            else:
                if kind == 1:
                    ctr["fixed"] += 1
                    if fixed is None:
                        fixed = (_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _table([5] * 32))
                    lit, dist = fixed
                else:
                    ctr["dynamic"] += 1
                    nlen, ndist, ncode = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
                    if nlen > 286 or ndist > 30:
                        raise _Stop(BAD_LENGTHS)
                    cl = [0] * 19
                    for i in range(ncode):
                        cl[_ORDER[i]] = bits.get(3)
                    clen = _table(cl, complete_only=True)
                    lens = []
                    while len(lens) < nlen + ndist:
                        s = _symbol(bits, clen, bad=BAD_LENGTHS)
                        if s < 16:
                            lens.append(s)
                            continue
                        if s == 16:
                            if not lens:
                                raise _Stop(BAD_LENGTHS)
                            val, rep = lens[-1], 3 + bits.get(2)
                        elif s == 17:
                            val, rep = 0, 3 + bits.get(3)
                        else:
                            val, rep = 0, 11 + bits.get(7)
                        ctr[f"rep{s}"] += 1
                        if len(lens) + rep > nlen + ndist:
                            raise _Stop(BAD_LENGTHS)
                        lens += [val] * rep
                    if lens[256] == 0:
                        raise _Stop(BAD_LENGTHS)
                    lit, dist = _table(lens[:nlen]), _table(lens[nlen:], allow_empty=True)
                while True:
                    s = _symbol(bits, lit, ctr)
                    if s == 256:
                        break
                    if s < 256:
                        if len(out) >= want:
                            raise _Stop(LONG)
                        out.append(s)
                        continue
                    s -= 257
                    if s >= 29:
                        raise _Stop(BAD_SYMBOL)
                    length = _LBASE[s] + bits.get(_LEXT[s])
                    d = _symbol(bits, dist, ctr)
                    if d >= 30:
                        raise _Stop(BAD_SYMBOL)
                    d = _DBASE[d] + bits.get(_DEXT[d])
                    if d > len(out):
                        raise _Stop(BAD_DISTANCE)
                    if d < length:
                        ctr["overlap"] += 1
                    ctr["max_distance"] = max(ctr["max_distance"], d)
                    take = min(length, want - len(out))
                    for _ in range(take):
                        out.append(out[-d])
                    if take < length:
                        raise _Stop(LONG)
            if last:
                break
        bits.get(-bits.pos & 7)
        adler = int.from_bytes(bytes(bits.get(8) for _ in range(4)), "big")
    except _Stop as e:
        status |= e.status
    if len(out) < want and not status & LONG:
        status |= SHORT
    return out, status, adler


def adler32(data) -> int:
    a, b = 1, 0
    for v in data:
        a = (a + v) % 65521
        b = (b + a) % 65521
    return (b << 16) | a


def unfilter(raw: bytes, H: int, row_bytes: int, bpp: int, ctr=None):
    """H rows of 1 + row_bytes filtered bytes -> (uint8 [H, row_bytes], status)"""
    ctr = new_counters() if ctr is None else ctr
    rows = np.zeros((H + 1, row_bytes + bpp), dtype=np.int64)      # a zero row above, bpp zero bytes to the left
    status = 0
    for r in range(H):
        line = raw[r * (1 + row_bytes):(r + 1) * (1 + row_bytes)]
        f = line[0]
        if f > 4:
            status |= BAD_FILTER
            f = 0
        ctr[f"filter{f}"] += 1
        x = np.frombuffer(bytes(line[1:]), dtype=np.uint8).astype(np.int64)
        cur, up = rows[r + 1], rows[r]
        if f == 0:
            cur[bpp:] = x
        elif f == 2:
            cur[bpp:] = (x + up[bpp:]) & 255
        else:
            for i in range(row_bytes):
                a, b, c = int(cur[i]), int(up[i + bpp]), int(up[i])
                if f == 1:
                    p = a
                elif f == 3:
                    p = (a + b) >> 1
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if pa <= pb and pa <= pc else b if pb <= pc else c
                cur[i + bpp] = (int(x[i]) + p) & 255
    return rows[1:, bpp:].astype(np.uint8), status


def convert(rows: np.ndarray, W: int, color_type: int, bit_depth: int, palette: bytes):
    """reconstructed rows -> (Pillow's RGB [H, W, 3], Pillow's L [H, W])"""
    H = rows.shape[0]
    if bit_depth < 8:
        ppb = 8 // bit_depth
        shifts = (8 - bit_depth * (np.arange(ppb) + 1)).astype(np.uint8)
        samples = ((rows[:, :, None] >> shifts) & ((1 << bit_depth) - 1)).reshape(H, -1)[:, :W]
    else:
        samples = rows.reshape(H, W, CHANNELS[color_type])
    pal = np.frombuffer(bytes(palette), dtype=np.uint8).reshape(256, 3)
    if color_type == 3:
        rgb = pal[samples.reshape(H, W)]
    elif color_type in (0, 4):
        grey = samples if bit_depth < 8 else samples[:, :, 0]
        grey = (grey.astype(np.uint16) * {1: 255, 2: 85, 4: 17, 8: 1}[bit_depth]).astype(np.uint8)
        return np.repeat(grey[:, :, None], 3, axis=2), grey
    else:
        rgb = samples[:, :, :3]
    c = rgb.astype(np.int64)
    lum = ((19595 * c[:, :, 0] + 38470 * c[:, :, 1] + 7471 * c[:, :, 2] + 0x8000) >> 16).astype(np.uint8)
    return np.ascontiguousarray(rgb), lum


def decode(data: bytes, ctr=None):
    """One file -> (RGB, L, status)"""
    ctr = new_counters() if ctr is None else ctr
    h = header(data)
    H, W, ct, depth = h["H"], h["W"], h["color_type"], h["bit_depth"]
    ctr[f"type{ct}"] += 1
    ctr[f"depth{depth}"] += 1
    row_bytes = (W * CHANNELS[ct] * depth + 7) // 8
    bpp = CHANNELS[ct] if depth == 8 else 1
    want = H * (1 + row_bytes)
    raw, status, adler = inflate(h["stream"], want, ctr)
    if adler is not None and adler32(raw) != adler:
        status |= BAD_ADLER
    raw = bytes(raw) + bytes(want - len(raw))
    rows, st = unfilter(raw, H, row_bytes, bpp, ctr)
    rgb, lum = convert(rows, W, ct, depth, h["palette"])
    return rgb, lum, status | st


def load_cases(path: str = GOLDEN):
    """({name: dict(file bytes, rgb, l, H, W, color_type, bit_depth)}, recorded counters, {name: (bytes, base case, expected bit)})"""
    z = np.load(path)
    names = [str(n) for n in z["names"]]
    cases = {}
    for n in names:
        geo = z[f"{n}/geom"]
        cases[n] = dict(file=z[f"{n}/file"].tobytes(), rgb=z[f"{n}/rgb"], l=z[f"{n}/l"], H=int(geo[0]), W=int(geo[1]), color_type=int(geo[2]),
                        bit_depth=int(geo[3]))
    counters = dict(zip((str(k) for k in z["counter_names"]), (int(v) for v in z["counter_values"])))
    damaged = {}
    for n, base, bit in zip(z["damaged_names"], z["damaged_base"], z["damaged_bit"]):
        damaged[str(n)] = (z[f"damaged/{n}"].tobytes(), str(base), int(bit))
    return cases, counters, damaged


def groups(cases):
    """{(H, W, color_type, bit_depth): [names]}: what one call takes"""
    out = {}
    for n, c in cases.items():
        out.setdefault((c["H"], c["W"], c["color_type"], c["bit_depth"]), []).append(n)
    return out
