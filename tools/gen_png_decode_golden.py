#!/usr/bin/env python
"""Writes tests/golden/png_decode.npz: PNG files and the pixels Pillow decodes from them (``convert('RGB')``, ``convert('L')``), the
fixtures of tests/test_png_decode_host.py and tests/test_gpu_png_decode.py.  Needs numpy, zlib and PIL only; no diff_sal_amd, no GPU.

Files are made two ways: ``Image.save`` (default, ``compress_level=1``, ``optimize=True``) on noise / smooth / flat content in
Pillow's modes L, RGB, P, LA, RGBA and 1; and chunks assembled here around ``zlib.compressobj`` or around a small fixed-code
deflate writer, for what Pillow never writes: each filter type on every row and the five cycling, stored blocks (one file needs two),
Z_FIXED / Z_RLE / Z_FILTERED, IDAT split into chunks of 1, 5 and 4096 bytes, tRNS, a 5-entry PLTE, every sub-byte depth at widths
that leave a part-filled last byte, a match at distance 32768 and matches with distance < length at distances 1, 2, 3.

It also records damaged copies (cut in mid-stream, a zeroed range, the last Adler byte flipped, a forged far distance, block type 3,
a stream two rows short, a stream one row long).  A damaged file may reach a GPU only after tools/png_decode_host_check.cpp, built
with -fsanitize=address,undefined, decoded it to a non-zero status without a report: pass the binary with --host-check, or no
damaged copy is written.

Before it writes, it checks on every case that the restatement tests/_png_decode_ref.py reproduces Pillow's pixels in both modes and
that every coverage counter is non-zero; tests/test_png_decode_host.py asserts the recorded counters again.  --embed PATH also writes
the host check's embedded files (tools/png_decode_host_check_files.h).
From scratch this takes two passes, because the host check includes the header that --embed writes: first
``python tools/gen_png_decode_golden.py --embed tools/png_decode_host_check_files.h`` (no damaged copy is recorded), then build
tools/png_decode_host_check.cpp with the sanitizers, then the full run below.  The header does not depend on the host check, so the
second pass rewrites it unchanged.
usage: python tools/gen_png_decode_golden.py --host-check ./png_decode_host_check [--embed tools/png_decode_host_check_files.h]"""
import argparse
import io
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _png_decode_ref as ref  # noqa: E402

SMALL = [(1, 1), (1, 5), (2, 3), (7, 13), (9, 5), (16, 16), (17, 33), (40, 3), (33, 48)]
LARGE = [(65, 70), (130, 9), (120, 160)]
CHANNELS = ref.CHANNELS


def content(kind, H, W, C, rng):
    """uint8 [H, W, C]"""
    if kind == "noise":
        return rng.integers(0, 256, size=(H, W, C), dtype=np.uint8)
    if kind == "flat":
        return np.broadcast_to(rng.integers(0, 256, size=(1, 1, C), dtype=np.uint8), (H, W, C)).copy()
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(3 * x + 2 * y + 40 * c) for c in range(C)], axis=2) + rng.integers(0, 3, size=(H, W, C))
    return (base % 256).astype(np.uint8)


def chunk(kind: bytes, payload: bytes) -> bytes:
    return len(payload).to_bytes(4, "big") + kind + payload + zlib.crc32(kind + payload).to_bytes(4, "big")


def assemble(H, W, ctype, depth, stream: bytes, split=None, plte=None, trns=None) -> bytes:
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes([depth, ctype, 0, 0, 0]))
    if plte is not None:
        out += chunk(b"PLTE", plte)
    if trns is not None:
        out += chunk(b"tRNS", trns)
    step = len(stream) if not split else split
    for at in range(0, len(stream), step):
        out += chunk(b"IDAT", stream[at:at + step])
    return out + chunk(b"IEND", b"")


def pack_rows(samples: np.ndarray, depth: int) -> np.ndarray:
    """samples uint8 [H, W * channels] -> the rows' bytes [H, row_bytes]"""
    if depth == 8:
        return samples
    H, n = samples.shape
    ppb = 8 // depth
    padded = np.zeros((H, -(-n // ppb) * ppb), dtype=np.uint8)
    padded[:, :n] = samples
    shifts = (8 - depth * (np.arange(ppb) + 1)).astype(np.uint8)
    return (padded.reshape(H, -1, ppb) << shifts).sum(axis=2).astype(np.uint8)


def filter_rows(rows: np.ndarray, bpp: int, filters) -> bytes:
    """the forward filters of PNG 9.2: rows [H, row_bytes] -> H * (1 + row_bytes) filtered bytes"""
    H, n = rows.shape
    r = np.zeros((H + 1, n + bpp), dtype=np.int64)
    r[1:, bpp:] = rows
    out = bytearray()
    for y in range(H):
        f = filters[y % len(filters)]
        x, a, b, c = r[y + 1, bpp:], r[y + 1, :n], r[y, bpp:], r[y, :n]
        if f == 0:
            p = 0 * x
        elif f == 1:
            p = a
        elif f == 2:
            p = b
        elif f == 3:
            p = (a + b) >> 1
        else:
            pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
            p = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        out += bytes([f]) + ((x - p) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def deflate(raw: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    return c.compress(raw) + c.flush()


class FixedWriter:
    """deflate with the fixed codes, written here so that a stream can hold what zlib never emits: items are bytes (literals) or
    (length, distance) matches"""

    def __init__(self):
        self.bits = []

    def put(self, value, n):      # least significant bit first
        self.bits += [(value >> k) & 1 for k in range(n)]

    def code(self, value, n):     # a Huffman code: most significant bit first
        self.bits += [(value >> (n - 1 - k)) & 1 for k in range(n)]

    def literal_or_length(self, s):
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def block(self, items, last=True, block_type=1):
        self.put(1 if last else 0, 1)
        self.put(block_type, 2)
        for it in items:
            if isinstance(it, tuple):
                length, dist = it
                s = max(k for k in range(29) if ref._LBASE[k] <= length) if length < 258 else 28
                self.literal_or_length(257 + s)
                self.put(length - ref._LBASE[s], ref._LEXT[s])
                d = max(k for k in range(30) if ref._DBASE[k] <= dist)
                self.code(d, 5)
                self.put(dist - ref._DBASE[d], ref._DEXT[d])
            else:
                self.literal_or_length(it)
        self.literal_or_length(256)

    def stream(self, raw_for_adler: bytes) -> bytes:
        bits = self.bits + [0] * (-len(self.bits) % 8)
        body = bytes(sum(b << k for k, b in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8))
        return b"\x78\x01" + body + zlib.adler32(raw_for_adler).to_bytes(4, "big")


def with_matches(raw: bytes, matches) -> list:
    """raw as literals, except that at each (position, length, distance) of `matches` a match stands for the bytes it reproduces"""
    items, at = [], 0
    for pos, length, dist in sorted(matches):
        assert pos >= at and all(raw[pos + k] == raw[pos + k - dist] for k in range(length))
        items += list(raw[at:pos]) + [(length, dist)]
        at = pos + length
    return items + list(raw[at:])


def pillow_pixels(data: bytes):
    im = Image.open(io.BytesIO(data))
    return np.asarray(im.convert("RGB")), np.asarray(Image.open(io.BytesIO(data)).convert("L"))


def hand_case(H, W, ctype, depth, kind, rng, filters=(0,), level=6, strategy=zlib.Z_DEFAULT_STRATEGY, split=None, trns=None, ncolours=None,
              rows_short=0, rows_long=0):
    C = CHANNELS[ctype]
    top = ncolours if ncolours else (1 << depth) if depth < 8 else 256
    img = content(kind, H, W, C, rng)
    samples = (img.astype(np.int64) % top if ctype == 3 or depth < 8 else img).astype(np.uint8).reshape(H, W * C)
    rows = pack_rows(samples, depth)
    raw = filter_rows(rows, C if depth == 8 else 1, filters)
    stride = 1 + rows.shape[1]
    if rows_short:
        raw = raw[:-rows_short * stride]
    if rows_long:
        raw = raw + raw[-rows_long * stride:]
    plte = rng.integers(0, 256, size=3 * top, dtype=np.uint8).tobytes() if ctype == 3 else None
    return assemble(H, W, ctype, depth, deflate(raw, level, strategy), split=split, plte=plte, trns=trns), raw


def make_cases():
    rng = np.random.default_rng(20240607)
    cases = {}

    def add(name, data):
        assert name not in cases, name
        cases[name] = data

    # 1. Pillow's own files
    options = [dict(), dict(compress_level=1), dict(optimize=True)]
    k = 0
    for (H, W) in SMALL + LARGE:
        large = (H, W) in LARGE
        for mode in ("L", "RGB", "P", "LA", "RGBA", "1"):
            if large and mode not in ("RGB", "L"):
                continue
            for kind in (("smooth",) if large else ("noise", "smooth", "flat") if mode in ("RGB", "L", "1") else ("noise", "smooth")):
                C = {"L": 1, "RGB": 3, "P": 1, "LA": 2, "RGBA": 4, "1": 1}[mode]
                img = content(kind, H, W, C, rng)
                if mode == "1":
                    im = Image.fromarray((img[:, :, 0] > 127))
                elif mode == "P":
                    im = Image.fromarray(img[:, :, 0], "L").convert("P")
                    im.putpalette(rng.integers(0, 256, size=768, dtype=np.uint8).tobytes())
                else:
                    im = Image.fromarray(img[:, :, 0] if C == 1 else img, mode)
                buf = io.BytesIO()
                im.save(buf, "PNG", **options[k % 3])
                add(f"{H}x{W}_pil_{mode}_{kind}_{'dlo'[k % 3]}", buf.getvalue())
                k += 1
    # 2. assembled here
    for f in range(5):      # each filter on every row
        add(f"17x33_hand_rgb_filter{f}", hand_case(17, 33, 2, 8, "smooth", rng, filters=(f,))[0])
        add(f"7x13_hand_grey_filter{f}", hand_case(7, 13, 0, 8, "noise", rng, filters=(f,))[0])
        add(f"33x48_hand_rgba_filter{f}", hand_case(33, 48, 6, 8, "smooth", rng, filters=(f,))[0])
    cyc = (0, 1, 2, 3, 4)
    add("33x48_hand_rgb_cycle", hand_case(33, 48, 2, 8, "noise", rng, filters=cyc)[0])
    add("65x70_hand_rgba_cycle", hand_case(65, 70, 6, 8, "smooth", rng, filters=(4, 3, 2, 1, 0))[0])
    add("65x70_hand_rgba_cycle_idat4096", hand_case(65, 70, 6, 8, "noise", rng, filters=cyc, split=4096)[0])
    add("130x9_hand_grey_cycle", hand_case(130, 9, 0, 8, "noise", rng, filters=cyc)[0])
    add("130x9_hand_la_cycle", hand_case(130, 9, 4, 8, "smooth", rng, filters=(3, 4))[0])
    add("120x160_hand_rgb_cycle", hand_case(120, 160, 2, 8, "smooth", rng, filters=cyc)[0])
    add("16x16_hand_rgb_stored", hand_case(16, 16, 2, 8, "noise", rng, level=0)[0])
    add("120x160_hand_rgba_stored2", hand_case(120, 160, 6, 8, "smooth", rng, filters=(1,), level=0)[0])      # 76920 bytes: two stored blocks
    for name, st in (("fixed", zlib.Z_FIXED), ("rle", zlib.Z_RLE), ("filtered", zlib.Z_FILTERED)):
        add(f"33x48_hand_rgb_{name}", hand_case(33, 48, 2, 8, "smooth", rng, filters=cyc, strategy=st)[0])
        add(f"17x33_hand_pal8_{name}", hand_case(17, 33, 3, 8, "noise", rng, filters=(0, 4), strategy=st)[0])
    add("9x5_hand_rgb_idat1", hand_case(9, 5, 2, 8, "noise", rng, filters=cyc, split=1)[0])
    add("17x33_hand_rgb_idat5", hand_case(17, 33, 2, 8, "noise", rng, filters=cyc, split=5)[0])
    add("7x13_hand_grey_trns", hand_case(7, 13, 0, 8, "noise", rng, trns=b"\x00\x40")[0])
    add("7x13_hand_rgb_trns", hand_case(7, 13, 2, 8, "noise", rng, filters=(4,), trns=b"\x00\x10\x00\x20\x00\x30")[0])
    add("7x13_hand_pal8_trns", hand_case(7, 13, 3, 8, "noise", rng, filters=(1,), trns=bytes(range(0, 250, 10)))[0])
    add("17x33_hand_pal8_plte5", hand_case(17, 33, 3, 8, "noise", rng, filters=cyc, ncolours=5)[0])
    add("17x33_hand_pal4_plte5", hand_case(17, 33, 3, 4, "noise", rng, filters=cyc, ncolours=5)[0])
    for depth in (1, 2, 4):      # widths that leave a part-filled last byte
        for ctype, tag in ((0, "grey"), (3, "pal")):
            for (H, W) in ((17, 33), (7, 13), (1, 5), (9, 5), (40, 3), (130, 9), (2, 3), (1, 1)):
                add(f"{H}x{W}_hand_{tag}{depth}", hand_case(H, W, ctype, depth, "noise", rng, filters=cyc)[0])
    # matches zlib never writes, through the fixed-code writer: distance 32768; distance < length at 1, 2, 3
    H, W = 120, 160
    img = content("smooth", H, W, 3, rng)
    raw = bytearray(filter_rows(img.reshape(H, W * 3), 3, (0,)))
    stride = 1 + 3 * W
    src = 2 * stride + 1      # behind a filter byte, inside row 2
    dst = src + 32768
    assert dst // stride == (dst + 99) // stride and src // stride == (src + 99) // stride and dst % stride
    raw[dst:dst + 100] = raw[src:src + 100]
    w = FixedWriter()
    w.block(with_matches(bytes(raw), [(dst, 100, 32768)]))
    add("120x160_hand_rgb_far", assemble(H, W, 2, 8, w.stream(bytes(raw))))
    H, W = 16, 16
    img = content("flat", H, W, 3, rng)
    raw = bytearray(filter_rows(img.reshape(H, W * 3), 3, (0,)))
    stride = 1 + 3 * W
    raw[1 + 8 * stride:9 * stride] = bytes([7]) * 48                 # row 8: period 1
    raw[1 + 9 * stride:10 * stride] = bytes([1, 250]) * 24           # row 9: period 2
    m = [(4, 40, 3), (2 + 8 * stride, 47, 1), (3 + 9 * stride, 46, 2), (1 + 12 * stride + 3, 45, 3)]
    w = FixedWriter()
    w.block(with_matches(bytes(raw), m))
    add("16x16_hand_rgb_overlap", assemble(H, W, 2, 8, w.stream(bytes(raw))))
    return cases


def find(cases, prefix):
    return next(n for n in sorted(cases) if n.startswith(prefix))


def make_damaged(cases):
    """{name: (bytes, the intact case it stands next to, the status bit expected)}"""
    rng = np.random.default_rng(7)
    base = find(cases, "33x48_pil_RGB_noise")
    h = ref.header(cases[base])
    s = h["stream"]
    out = {}
    out["cut"] = (assemble(33, 48, 2, 8, s[:len(s) // 2]), ref.NO_INPUT)
    z = bytearray(s)
    z[len(s) // 3:len(s) // 3 + 64] = bytes(64)
    out["zeroed"] = (assemble(33, 48, 2, 8, bytes(z)), 0)
    out["adler"] = (assemble(33, 48, 2, 8, s[:-1] + bytes([s[-1] ^ 1])), ref.BAD_ADLER)
    raw = hand_case(33, 48, 2, 8, "noise", rng)[1]
    w = FixedWriter()
    w.block(list(raw[:50]) + [(20, 51)] + list(raw[70:]))
    out["far"] = (assemble(33, 48, 2, 8, w.stream(raw)), ref.BAD_DISTANCE)
    w = FixedWriter()
    w.block(list(raw[:500]), last=False)
    w.block([], block_type=3)
    out["type3"] = (assemble(33, 48, 2, 8, w.stream(raw)), ref.BAD_BLOCK)
    out["short"] = (hand_case(33, 48, 2, 8, "noise", rng, filters=(0, 1, 2, 3, 4), rows_short=2)[0], ref.SHORT)
    out["long"] = (hand_case(33, 48, 2, 8, "noise", rng, filters=(0, 1, 2, 3, 4), rows_long=1)[0], ref.LONG)
    return {k: (v[0], base, v[1]) for k, v in out.items()}


def host_check(binary, data: bytes) -> int:
    """the status tools/png_decode_host_check.cpp gives the file, under its sanitizers"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "f.png")
        with open(path, "wb") as f:
            f.write(data)
        r = subprocess.run([binary, "RGB", os.path.join(d, "out.raw"), path], capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"host check failed:\n{r.stdout}\n{r.stderr}")
        return int(r.stdout.split("status")[1].split()[0])


def fnv(a: np.ndarray) -> int:
    h = 0x811C9DC5
    for v in a.tobytes():
        h = ((h ^ v) * 0x01000193) & 0xFFFFFFFF
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-check", help="the sanitizer build of tools/png_decode_host_check.cpp; without it no damaged copy is recorded")
    ap.add_argument("--embed", help="also write the host check's embedded files to this header")
    args = ap.parse_args()
    cases = make_cases()
    ctr = ref.new_counters()
    store = {"names": np.array(sorted(cases))}
    for name in sorted(cases):
        data = cases[name]
        rgb, lum = pillow_pixels(data)
        got_rgb, got_l, status = ref.decode(data, ctr)
        assert status == 0 and np.array_equal(got_rgb, rgb) and np.array_equal(got_l, lum), name
        h = ref.header(data)
        assert name.startswith(f"{h['H']}x{h['W']}_"), name
        store[f"{name}/file"] = np.frombuffer(data, dtype=np.uint8)
        store[f"{name}/rgb"], store[f"{name}/l"] = rgb, lum
        store[f"{name}/geom"] = np.array([h["H"], h["W"], h["color_type"], h["bit_depth"]], dtype=np.int32)
    assert ctr["max_distance"] == 32768 and all(ctr[k] > 0 for k in ref.COUNTERS), ctr
    store["counter_names"], store["counter_values"] = np.array(ref.COUNTERS), np.array([ctr[k] for k in ref.COUNTERS], dtype=np.int64)
    names, bases, bits = [], [], []
    if args.host_check:
        for name, (data, base, bit) in make_damaged(cases).items():
            status = ref.decode(data)[2]
            seen = host_check(args.host_check, data)
            assert status != 0 and seen == status and (bit == 0 or status & bit), (name, status, seen, bit)
            names.append(name), bases.append(base), bits.append(bit if bit else status)
            store[f"damaged/{name}"] = np.frombuffer(data, dtype=np.uint8)
        for name in sorted(cases):      # and every intact case decodes clean there
            assert host_check(args.host_check, cases[name]) == 0, name
    store["damaged_names"], store["damaged_base"], store["damaged_bit"] = np.array(names), np.array(bases), np.array(bits, dtype=np.int32)
    np.savez_compressed(ref.GOLDEN, **store)
    print(f"{len(cases)} cases, {len(names)} damaged, {os.path.getsize(ref.GOLDEN)} bytes; counters {ctr}")
    if args.embed:
        pick = [find(cases, p) for p in ("7x13_pil_RGB_noise", "17x33_hand_pal4_plte5", "9x5_hand_rgb_idat1", "16x16_hand_rgb_overlap",
                                         "33x48_hand_rgb_cycle", "16x16_hand_rgb_stored", "17x33_pil_LA_smooth", "130x9_hand_grey2")]
        with open(args.embed, "w") as f:
            f.write("// Written by tools/gen_png_decode_golden.py --embed: PNG files of the fixture and FNV-1a of Pillow's RGB and L pixels.\n")
            f.write("struct Embedded { const char* name; const unsigned char* data; unsigned size; unsigned rgb, l; };\n")
            for i, name in enumerate(pick):
                data = cases[name]
                f.write(f"static const unsigned char kFile{i}[] = {{" + ",".join(str(b) for b in data) + "};\n")
            f.write("static const Embedded kEmbedded[] = {\n")
            for i, name in enumerate(pick):
                rgb, lum = pillow_pixels(cases[name])
                f.write(f'  {{"{name}", kFile{i}, sizeof(kFile{i}), {fnv(rgb)}u, {fnv(lum)}u}},\n')
            f.write("};\n")


if __name__ == "__main__":
    main()
