"""NumPy restatement of the JPEG decode (include/diffsal.h, "JPEG decode", (a)-(f)): its own marker walk, the Huffman decode of T.81
F.2 bit by bit, dequantisation, libjpeg's slow-integer inverse DCT and range limit (tests/_jpeg_ref.idct, the export's read-back),
libjpeg's chroma up-sampling, its YCbCr -> RGB and Pillow's L.  All integer arithmetic, in int64 here.  ``decode`` also counts what
a file exercised (``new_counters``), so that the fixture's case set can be held to its coverage.  The fixtures
(tests/golden/jpeg_decode.npz) are Pillow's files and pixels, written by tools/gen_jpeg_decode_golden.py."""
import os

import numpy as np

from tests._jpeg_ref import ZIGZAG, idct

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_decode.npz")


def new_counters():
    return dict(long_code=0, zrl=0, no_eob=0, dc_cat0=0, dc_cat8=0, diff_neg=0, diff_pos=0, stuffed_ff=0, restart_wrap=0,
                replicate_h2v1=0, replicate_h2v2=0, fancy_first_col=0, fancy_last_col=0, fancy_first_row=0, fancy_last_row=0,
                clamp_lo=0, clamp_hi=0)


def walk(data):
    """The header of a well-formed baseline file: dict(H, W, comps [(id, h, v, tq)], qt {id: int64 [64] natural}, huff {(class, id):
    {(length, code): symbol}}, restart, scan [(component, dc table, ac table)], scan_at)"""
    assert data[:2] == b"\xFF\xD8"
    out = dict(qt={}, huff={}, restart=0)
    at = 2
    while True:
        assert data[at] == 0xFF
        m, n = data[at + 1], (data[at + 2] << 8) | data[at + 3]
        p = data[at + 4:at + 2 + n]
        if m == 0xDB:
            while p:
                assert p[0] >> 4 == 0
                t = np.zeros(64, dtype=np.int64)
                t[ZIGZAG] = list(p[1:65])
                out["qt"][p[0] & 15] = t
                p = p[65:]
        elif m == 0xC4:
            while p:
                counts, codes, code, k = list(p[1:17]), {}, 0, 17
                for length in range(1, 17):      # Annex C: codes in order of length
                    for _ in range(counts[length - 1]):
                        codes[(length, code)] = p[k]
                        code += 1
                        k += 1
                    code <<= 1
                out["huff"][(p[0] >> 4, p[0] & 15)] = codes
                p = p[k:]
        elif m == 0xC0:
            assert p[0] == 8
            out["H"], out["W"] = (p[1] << 8) | p[2], (p[3] << 8) | p[4]
            out["comps"] = [(p[6 + 3 * c], p[7 + 3 * c] >> 4, p[7 + 3 * c] & 15, p[8 + 3 * c]) for c in range(p[5])]
        elif m == 0xDD:
            out["restart"] = (p[0] << 8) | p[1]
        elif m == 0xDA:
            out["scan"] = [(p[1 + 2 * c], p[2 + 2 * c] >> 4, p[2 + 2 * c] & 15) for c in range(p[0])]
            out["scan_at"] = at + 2 + n
            return out
        at += 2 + n


def segments(data, scan_at):
    """[(begin, end)] of the restart intervals of the scan, markers left out, and the scan's end; a plain loop over the bytes"""
    out, begin, i = [], scan_at, scan_at
    while i + 1 < len(data):
        if data[i] == 0xFF and data[i + 1] not in (0x00, 0xFF):
            out.append((begin, i))
            if not 0xD0 <= data[i + 1] <= 0xD7:
                return out, i
            begin = i + 2
            i += 2
            continue
        i += 1
    raise AssertionError("no marker behind the scan")


class _Bits:
    def __init__(self, raw, k):
        body = raw.replace(b"\xFF\x00", b"\xFF")
        k["stuffed_ff"] += raw.count(b"\xFF\x00")
        self.n = 8 * len(body) + 64
        self.v = int.from_bytes(body + bytes(8), "big")
        self.pos = 0

    def take(self, n):
        if n == 0:
            return 0
        self.pos += n
        assert self.pos <= self.n, "the segment ran out of bits"
        return (self.v >> (self.n - self.pos)) & ((1 << n) - 1)

    def symbol(self, codes, k):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.take(1)
            if (length, code) in codes:
                k["long_code"] += length > 9
                return codes[(length, code)]
        raise AssertionError("no code matches")


def _extend(v, n):
    return v - (1 << n) + 1 if n and v < (1 << (n - 1)) else v


def coefficients(data, hd, k):
    """[(int64 [bh, bw, 64] natural order)] per component, MCU padding included"""
    comps = hd["comps"]
    nc = len(comps)
    hs, vs = (comps[0][1], comps[0][2]) if nc == 3 else (1, 1)
    H, W = hd["H"], hd["W"]
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    fac = [(hs, vs) if c == 0 else (1, 1) for c in range(nc)]
    coef = [np.zeros((my * v, mx * h, 64), dtype=np.int64) for h, v in fac]
    segs, _ = segments(data, hd["scan_at"])
    ri = hd["restart"]
    assert len(segs) == (-(-(mx * my) // ri) if ri else 1)
    k["restart_wrap"] += len(segs) - 1 > 8
    for s, (b, e) in enumerate(segs):
        bits = _Bits(data[b:e].rstrip(b"\xFF") if data[e - 1:e] == b"\xFF" else data[b:e], k)
        pred = [0] * nc
        first = s * ri
        for m in range(first, min(first + ri, mx * my) if ri else mx * my):
            for c in range(nc):
                h, v = fac[c]
                dc, ac = hd["huff"][(0, hd["scan"][c][1])], hd["huff"][(1, hd["scan"][c][2])]
                for blk in range(h * v):
                    out = coef[c][(m // mx) * v + blk // h, (m % mx) * h + blk % h]
                    t = bits.symbol(dc, k)
                    diff = _extend(bits.take(t), t)
                    k["dc_cat0"] += t == 0
                    k["dc_cat8"] += t >= 8
                    k["diff_neg"] += diff < 0
                    k["diff_pos"] += diff > 0
                    pred[c] += diff
                    out[0] = pred[c]
                    i = 1
                    while i < 64:
                        rs = bits.symbol(ac, k)
                        r, sz = rs >> 4, rs & 15
                        if sz == 0:
                            if r != 15:
                                break
                            k["zrl"] += 1
                            i += 16
                            continue
                        i += r
                        assert i <= 63
                        out[ZIGZAG[i]] = _extend(bits.take(sz), sz)
                        i += 1
                    k["no_eob"] += out[63] != 0
        assert bits.pos <= bits.n - 64, "the segment ran out of bits"
    return coef, (hs, vs)


def _planes(coef, hd):
    out = []
    for c, cf in enumerate(coef):
        bh, bw, _ = cf.shape
        px = idct((cf * hd["qt"][hd["comps"][c][3]]).reshape(bh, bw, 8, 8))
        out.append(px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8).astype(np.int64))
    return out


def _up_h(x, lo, hi, shift):
    """out[2i] = (3 x[i] + x[i-1] + lo) >> shift, out[2i+1] = (3 x[i] + x[i+1] + hi) >> shift along the last axis, the edge sample
    standing in for the missing neighbour (which makes the first and last column the special forms of (d))"""
    left = np.concatenate([x[:, :1], x[:, :-1]], axis=1)
    right = np.concatenate([x[:, 1:], x[:, -1:]], axis=1)
    out = np.empty((x.shape[0], 2 * x.shape[1]), dtype=np.int64)
    out[:, 0::2] = (3 * x + left + lo) >> shift
    out[:, 1::2] = (3 * x + right + hi) >> shift
    return out


def upsample(x, hs, vs, H, W, k):
    """one chroma plane (MCU-padded) -> [H, W]"""
    cw, ch = -(-W // hs), -(-H // vs)
    x = x[:ch, :cw]      # samples of the padding are never read
    if hs == 1:
        return x
    if cw <= 2:
        k["replicate_h2v1" if vs == 1 else "replicate_h2v2"] += 1
        return np.repeat(np.repeat(x, vs, axis=0), 2, axis=1)[:H, :W]
    k["fancy_first_col"] += 1
    k["fancy_last_col"] += W == 2 * cw
    if vs == 1:
        return _up_h(x, 1, 2, 2)[:H, :W]
    k["fancy_first_row"] += 1
    k["fancy_last_row"] += H == 2 * ch
    r = np.empty((2 * ch, cw), dtype=np.int64)
    r[0::2] = 3 * x + np.concatenate([x[:1], x[:-1]])
    r[1::2] = 3 * x + np.concatenate([x[1:], x[-1:]])
    return _up_h(r, 8, 7, 4)[:H, :W]


def decode(data, mode="RGB", counters=None):
    """uint8 [H, W, 3] (RGB) or [H, W] (L) of one baseline file: what Pillow's Image.open(f).convert(mode) returns"""
    k = new_counters() if counters is None else counters
    data = bytes(data)
    hd = walk(data)
    H, W = hd["H"], hd["W"]
    coef, (hs, vs) = coefficients(data, hd, k)
    planes = _planes(coef, hd)
    y = planes[0][:H, :W]
    if len(planes) == 1:
        return y.astype(np.uint8) if mode == "L" else np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    cb, cr = (upsample(p, hs, vs, H, W, k) - 128 for p in planes[1:])
    rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], axis=2)
    k["clamp_lo"] += int((rgb < 0).sum())
    k["clamp_hi"] += int((rgb > 255).sum())
    rgb = np.clip(rgb, 0, 255)
    if mode == "L":
        return ((19595 * rgb[..., 0] + 38470 * rgb[..., 1] + 7471 * rgb[..., 2] + 32768) >> 16).astype(np.uint8)
    return rgb.astype(np.uint8)


def load_cases():
    """{name: dict(file bytes, rgb [H, W, 3], l [H, W], H, W, ncomp, hs, vs, restart, nseg)}, the recorded counters, and the three
    damaged files {name: bytes} that tools/jpeg_decode_host_check.cpp decoded to a non-zero status"""
    z = np.load(GOLDEN)
    cases = {}
    for n in (str(n) for n in z["names"]):
        c = {"file": z[f"{n}/file"].tobytes(), "rgb": z[f"{n}/rgb"], "l": z[f"{n}/l"]}
        c.update({key: int(v) for key, v in zip(("H", "W", "ncomp", "hs", "vs", "restart", "nseg"), z[f"{n}/geometry"])})
        cases[n] = c
    counters = {str(key): int(v) for key, v in zip(z["counter_names"], z["counter_values"])}
    damaged = {str(n): z[f"damaged/{n}"].tobytes() for n in z["damaged_names"]}
    return cases, counters, damaged


def groups(cases):
    """the names of the cases that may share a call: {(H, W, ncomp, hs, vs): [names]}"""
    out = {}
    for n, c in cases.items():
        out.setdefault((c["H"], c["W"], c["ncomp"], c["hs"], c["vs"]), []).append(n)
    return out
