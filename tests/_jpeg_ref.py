"""NumPy restatement of the JPEG export (include/diffsal.h, "JPEG export"): the quantisation table, libjpeg's slow-integer forward
DCT and quantiser, the Annex K Huffman coding with byte stuffing, the file layout, and the pixels a default libjpeg decoder reads
back (dequantise, slow-integer inverse DCT, range limit).  All integer arithmetic, in int64 here; ``_fits32`` checks that every
intermediate of the transforms fits the 32-bit integers the kernels use.  ``encode`` also counts what its input exercised
(``new_counters``), so that the fixture's case set can be held to its coverage.  The fixtures (tests/golden/jpeg_export.npz) are
Pillow's bytes and pixels, written by tools/gen_jpeg_golden.py."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_export.npz")
QUALITIES = (95, 100, 75, 30)

# ITU-T T.81 Annex K.1 (luminance), natural order
BASE_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                   80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72,
                   92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
                   42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62,
                   63])
# Annex K.3: number of codes of each length 1..16, then the symbols in code order
DC_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_VALS = [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
           0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
           0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
           0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
           0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
           0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
           0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5,
           0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]

C = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137, f1_961=16069,
         f2_053=16819, f2_562=20995, f3_072=25172)
CONST_BITS, PASS1_BITS = 13, 2


def quant_table(quality=95):
    """jpeg_quality_scaling and jpeg_add_quant_table with force_baseline: int64 [64], natural order."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality {quality} outside 1..100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((BASE_Q * s + 50) // 100, 1, 255)


def _codes(bits, vals):
    """symbol -> (code, length), codes handed out in order of length (Annex C)"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODE, AC_CODE = _codes(DC_BITS, DC_VALS), _codes(AC_BITS, AC_VALS)


def _fits32(*arrays):
    for a in arrays:
        assert np.abs(a).max(initial=0) < 2 ** 31, "an intermediate leaves 32 bits"


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, shift_dc, n):
    """one pass of jfdctint along the last axis; the even outputs 0 and 4 are scaled by shift_dc(x), the others descaled by n"""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    o[0], o[4] = shift_dc(t10 + t11), shift_dc(t10 - t11)
    z1 = (t12 + t13) * C["f0_541"]
    o[2] = _descale(z1 + t13 * C["f0_765"], n)
    o[6] = _descale(z1 - t12 * C["f1_847"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * C["f1_175"]
    t4, t5, t6, t7 = t4 * C["f0_298"], t5 * C["f2_053"], t6 * C["f3_072"], t7 * C["f1_501"]
    z1, z2, z3, z4 = -z1 * C["f0_899"], -z2 * C["f2_562"], -z3 * C["f1_961"] + z5, -z4 * C["f0_390"] + z5
    _fits32(t4, t5, t6, t7, z1, z2, z3, z4, z5)
    o[7], o[5], o[3], o[1] = (_descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n))
    return np.stack(o, axis=-1)


def fdct(blocks):
    """jfdctint on [..., 8, 8] int64 samples - 128: rows, then columns; the result carries a factor 8"""
    r = _fdct_pass(blocks, lambda x: x << PASS1_BITS, CONST_BITS - PASS1_BITS)
    c = _fdct_pass(np.swapaxes(r, -1, -2), lambda x: _descale(x, PASS1_BITS), CONST_BITS + PASS1_BITS)
    return np.swapaxes(c, -1, -2)


def _idct_pass(d, n):
    d = [d[..., i] for i in range(8)]
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * C["f0_541"]
    t2, t3 = z1 - z3 * C["f1_847"], z1 + z2 * C["f0_765"]
    t0, t1 = (d[0] + d[4]) << CONST_BITS, (d[0] - d[4]) << CONST_BITS
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * C["f1_175"]
    t0, t1, t2, t3 = t0 * C["f0_298"], t1 * C["f2_053"], t2 * C["f3_072"], t3 * C["f1_501"]
    z1, z2, z3, z4 = -z1 * C["f0_899"], -z2 * C["f2_562"], -z3 * C["f1_961"] + z5, -z4 * C["f0_390"] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    _fits32(t10, t11, t12, t13, t0, t1, t2, t3, z1, z2, z3, z4, z5, t10 + t3, t10 - t3, t11 + t2, t11 - t2, t12 + t1, t12 - t1, t13 + t0,
            t13 - t0)
    o = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([_descale(v, n) for v in o], axis=-1)


def idct(coefs):
    """jidctint on dequantised [..., 8, 8] int64 coefficients: columns, then rows, then libjpeg's range limit: the sum + 128 clamped
    to 0..255, read through a table indexed by the low 10 bits (the plain clamp wherever the sum lies in -512..511)"""
    c = np.swapaxes(_idct_pass(np.swapaxes(coefs, -1, -2), CONST_BITS - PASS1_BITS), -1, -2)
    v = _idct_pass(c, CONST_BITS + PASS1_BITS + 3) & 1023
    return np.where(v < 128, v + 128, np.where(v < 512, 255, np.where(v < 896, 0, v - 896))).astype(np.uint8)


def _blocks(u8):
    """[h, w] uint8 -> [bh, bw, 8, 8] int64 samples - 128, padded by replicating the last column, then the last row"""
    h, w = u8.shape
    bh, bw = (h + 7) // 8, (w + 7) // 8
    p = np.pad(u8.astype(np.int64), ((0, bh * 8 - h), (0, bw * 8 - w)), mode="edge") - 128
    return p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)


def quantised(u8, quality=95):
    """[nblk, 64] quantised coefficients, blocks in raster order, natural order inside a block"""
    d = fdct(_blocks(u8)).reshape(-1, 64)
    div = 8 * quant_table(quality)
    return np.sign(d) * ((np.abs(d) + div // 2) // div)


def decode(u8, quality=95):
    """the pixels a default libjpeg decoder returns for encode(u8, quality): uint8 [h, w]"""
    h, w = u8.shape
    bh, bw = (h + 7) // 8, (w + 7) // 8
    c = (quantised(u8, quality) * quant_table(quality)).reshape(bh, bw, 8, 8)
    return idct(c).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)[:h, :w].copy()


def header(h, w, quality=95):
    """everything in front of the scan data"""
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f"{h} x {w}: 1..65535 per axis")
    t = quant_table(quality)
    out = bytearray(b"\xFF\xD8\xFF\xE0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += b"\xFF\xDB\x00\x43\x00" + bytes(int(t[z]) for z in ZIGZAG)
    out += b"\xFF\xC0\x00\x0B\x08" + bytes([h >> 8, h & 255, w >> 8, w & 255]) + b"\x01\x01\x11\x00"
    out += b"\xFF\xC4" + bytes([0, 19 + len(DC_VALS), 0x00]) + bytes(DC_BITS) + bytes(DC_VALS)
    out += b"\xFF\xC4" + bytes([0, 19 + len(AC_VALS), 0x10]) + bytes(AC_BITS) + bytes(AC_VALS)
    out += b"\xFF\xDA\x00\x08\x01\x01\x00\x00\x3F\x00"
    return bytes(out)


def new_counters():
    return dict(zrl=0, no_eob=0, stuffed_ff=0, padded_last_ff=0, max_dc_cat=0, max_ac_cat=0, dc_neg=0, dc_pos=0, all_eob_images=0)


def encode(u8, quality=95, counters=None):
    """the complete file for one [h, w] uint8 image; ``counters`` (new_counters) is updated with what the image exercised"""
    k = new_counters() if counters is None else counters
    coef = quantised(u8, quality)[:, ZIGZAG].tolist()
    out = bytearray()
    acc = nacc = 0
    n_eob_only = 0

    def put(code, n):
        nonlocal acc, nacc
        acc = (acc << n) | code
        nacc += n
        while nacc >= 8:
            byte = (acc >> (nacc - 8)) & 255
            out.append(byte)
            if byte == 255:
                out.append(0)
                k["stuffed_ff"] += 1
            nacc -= 8
        acc &= (1 << nacc) - 1

    def put_value(v, n):      # a negative value is coded as v - 1 in the low n bits
        if n:
            put((v if v >= 0 else v - 1) & ((1 << n) - 1), n)

    pred = 0
    for zz in coef:
        diff = zz[0] - pred
        pred = zz[0]
        n = abs(diff).bit_length()
        k["max_dc_cat"] = max(k["max_dc_cat"], n)
        k["dc_neg"] += diff < 0
        k["dc_pos"] += diff > 0
        put(*DC_CODE[n])
        put_value(diff, n)
        run = 0
        for v in zz[1:]:
            if v == 0:
                run += 1
                continue
            while run > 15:
                put(*AC_CODE[0xF0])
                k["zrl"] += 1
                run -= 16
            n = abs(v).bit_length()
            k["max_ac_cat"] = max(k["max_ac_cat"], n)
            put(*AC_CODE[(run << 4) | n])
            put_value(v, n)
            run = 0
        if run:
            put(*AC_CODE[0x00])
            n_eob_only += run == 63
        else:
            k["no_eob"] += 1
    if nacc:      # the last byte is filled with 1-bits; an FF made that way is stuffed like any other
        before = k["stuffed_ff"]
        put((1 << (8 - nacc)) - 1, 8 - nacc)
        k["padded_last_ff"] += k["stuffed_ff"] - before
        k["stuffed_ff"] = before
    k["all_eob_images"] += n_eob_only == len(coef)
    h, w = u8.shape
    return header(h, w, quality) + bytes(out) + b"\xFF\xD9"


BIG_SHAPE, BIG_SEED = (3, 224, 384), 20240611


def big_input():
    """the full-size case, uint8 [3, 224, 384]: saliency-like blobs with mild noise, in integer arithmetic from a seed (the same
    bytes wherever it is rebuilt)"""
    B, H, W = BIG_SHAPE
    rng = np.random.default_rng(BIG_SEED)
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    out = np.zeros(BIG_SHAPE, dtype=np.uint8)
    for b in range(B):
        acc = np.zeros((H, W), dtype=np.int64)
        for _ in range(3 + b):
            cy, cx, s, a = int(rng.integers(20, H - 20)), int(rng.integers(20, W - 20)), int(rng.integers(12, 60)), int(rng.integers(90, 250))
            acc += a * s * s // (s * s + (y - cy) ** 2 + (x - cx) ** 2)
        acc += rng.integers(-3, 4, size=(H, W))
        out[b] = np.clip(acc, 0, 255)
    return out


def sha256(data):
    return hashlib.sha256(bytes(data)).hexdigest()


def load_cases():
    """{name: dict(u8 [h, w], quality -> dict(file bytes, decoded [h, w]))} and the big case's record"""
    z = np.load(GOLDEN)
    names = [str(n) for n in z["names"]]
    cases = {}
    for n in names:
        c = {"u8": z[f"{n}/u8"], "q": {}}
        for q in z[f"{n}/qualities"].tolist():
            c["q"][int(q)] = {"file": z[f"{n}/q{q}/file"].tobytes(), "decoded": z[f"{n}/q{q}/decoded"]}
        cases[n] = c
    big = {"lengths": z["big/lengths"].tolist(), "sha256": [str(s) for s in z["big/sha256"]], "rows": z["big/rows"], "cols": z["big/cols"],
           "decoded": z["big/decoded"], "quality": int(z["big/quality"])}
    counters = {str(k): int(v) for k, v in zip(z["counter_names"], z["counter_values"])}
    return cases, big, counters
