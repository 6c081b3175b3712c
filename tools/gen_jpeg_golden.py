#!/usr/bin/env python3
"""Writes tests/golden/jpeg_export.npz: what Pillow (libjpeg-turbo) makes of the JPEG export's test images.  Per case the uint8
input and, per quality, the bytes of ``Image.fromarray(u8).save(f, "JPEG", quality=q)`` and the pixels ``Image.open`` reads back from
them.  The full-size case (3 x 224 x 384, rebuilt from a seed by tests/_jpeg_ref.big_input) records the length and SHA-256 of each
file and the decoded pixels on a grid of rows and columns.  Needs numpy and PIL only; no test runs it.

Before it writes, it checks on every case that the restatement tests/_jpeg_ref.py reproduces Pillow's bytes and pixels (the header's
DQT and DHT segments, i.e. the quantisation and Huffman tables, included), and that the case set exercises what the coder can do
(COVERAGE below, counted by the restatement's encoder); tests/test_jpeg_host.py asserts the recorded counters again.
usage: python tools/gen_jpeg_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import _jpeg_ref as ref  # noqa: E402

# counter -> the least the case set must reach
COVERAGE = dict(zrl=1, no_eob=1, stuffed_ff=1, padded_last_ff=1, max_dc_cat=11, max_ac_cat=10, dc_neg=1, dc_pos=1, all_eob_images=1)
ALL_Q = list(ref.QUALITIES)


def pillow(u8, q):
    f = io.BytesIO()
    Image.fromarray(u8).save(f, "JPEG", quality=q)
    data = f.getvalue()
    img = Image.open(io.BytesIO(data))
    assert img.mode == "L" and img.size == (u8.shape[1], u8.shape[0])
    return data, np.asarray(img).copy()


def smooth(h, w, rng, noise=2):
    y, x = np.mgrid[0:h, 0:w]
    v = 128 + 90 * np.sin(x / 9.0 + 0.3) * np.cos(y / 7.0) + rng.integers(-noise, noise + 1, size=(h, w))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def padded_ff_image():
    """an 8 x 8 image whose scan ends in a partial byte that the 1-bit fill turns into FF (found by the restatement: cheap)"""
    for seed in range(100000):
        u8 = np.random.default_rng(seed).integers(0, 256, size=(8, 8), dtype=np.uint8)
        k = ref.new_counters()
        ref.encode(u8, 95, k)
        if k["padded_last_ff"]:
            return u8
    raise SystemExit("no seed gives a padded last byte of FF")


def cases():
    rng = np.random.default_rng(20240612)
    rnd = lambda h, w: rng.integers(0, 256, size=(h, w), dtype=np.uint8)      # noqa: E731
    y, x = np.mgrid[0:8, 0:8]
    hf = np.clip(np.rint(128 + 120 * np.cos((2 * x + 1) * 7 * np.pi / 16) * np.cos((2 * y + 1) * 7 * np.pi / 16)), 0, 255).astype(np.uint8)
    out = {
        "r1x1": (rnd(1, 1), [95]),
        "r3x17": (rnd(3, 17), [95]),
        "r8x8": (rnd(8, 8), [95]),
        "r13x21": (rnd(13, 21), ALL_Q),      # edge replication on both axes
        "r16x24": (rnd(16, 24), ALL_Q),
        "s37x50": (smooth(37, 50, rng), [95]),
        "flat24x24": (np.full((24, 24), 77, dtype=np.uint8), [95]),      # every block is EOB alone
        "bw24x32": ((rng.integers(0, 2, size=(24, 32)) * 255).astype(np.uint8), [95]),      # many FF bytes in the scan
        "padff8x8": (padded_ff_image(), [95]),
        "dc11_8x32": (np.repeat(np.array([0, 255, 0, 255], dtype=np.uint8), 8)[None].repeat(8, 0), [95, 100]),      # flat 0 / 255 blocks
        "ac10_8x8": (np.repeat(np.array([0, 255], dtype=np.uint8), 4)[None].repeat(8, 0), [95, 100]),      # a step inside the block
        "hf8x16": (np.concatenate([hf, 255 - hf], axis=1), [95, 75]),      # coefficient 63 alone: ZRLs, no EOB
        "s1x4097": (smooth(1, 4097, rng, noise=6), [95]),      # 513 blocks: more than two chunks of the offset scan, odd
    }
    return out


def main():
    arrays, names = {}, []
    k = ref.new_counters()
    for name, (u8, qs) in cases().items():
        names.append(name)
        arrays[f"{name}/u8"] = u8
        arrays[f"{name}/qualities"] = np.array(qs, dtype=np.int64)
        for q in qs:
            data, dec = pillow(u8, q)
            mine = ref.encode(u8, q, k)
            assert data[:len(ref.header(*u8.shape, q))] == ref.header(*u8.shape, q), (name, q, "header / tables")
            assert mine == data, (name, q, "file bytes")
            assert np.array_equal(ref.decode(u8, q), dec), (name, q, "decoded pixels")
            arrays[f"{name}/q{q}/file"] = np.frombuffer(data, dtype=np.uint8)
            arrays[f"{name}/q{q}/decoded"] = dec
        print(name, u8.shape, qs, [len(arrays[f"{name}/q{q}/file"]) for q in qs])
    big = ref.big_input()
    rows = np.array(sorted(set(range(0, big.shape[1], 7)) | {big.shape[1] - 1}))
    cols = np.array(sorted(set(range(0, big.shape[2], 5)) | {big.shape[2] - 1}))
    lengths, shas, grid = [], [], []
    for img in big:
        data, dec = pillow(img, 95)
        assert ref.encode(img, 95, k) == data and np.array_equal(ref.decode(img, 95), dec), "big"
        lengths.append(len(data))
        shas.append(ref.sha256(data))
        grid.append(dec[rows][:, cols])
    arrays.update({"big/lengths": np.array(lengths, dtype=np.int64), "big/sha256": np.array(shas), "big/rows": rows, "big/cols": cols,
                   "big/decoded": np.stack(grid), "big/quality": np.int64(95)})
    print("big", big.shape, lengths)
    print("coverage", k)
    for name, least in COVERAGE.items():
        assert k[name] >= least, f"the case set lost its coverage of {name}: {k[name]} < {least}"
    arrays["names"] = np.array(names)
    arrays["counter_names"] = np.array(list(k))
    arrays["counter_values"] = np.array([int(v) for v in k.values()], dtype=np.int64)
    np.savez_compressed(ref.GOLDEN, **arrays)
    print("wrote", ref.GOLDEN, os.path.getsize(ref.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
