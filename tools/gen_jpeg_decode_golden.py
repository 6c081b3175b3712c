#!/usr/bin/env python3
"""Writes tests/golden/jpeg_decode.npz: JPEG files written by Pillow (libjpeg-turbo) from synthetic images, and the pixels
``Image.open(f).convert("RGB" | "L")`` reads back from them.  Per case the file's bytes, both pixel arrays and the geometry the
parser must find (H, W, components, luma sampling, restart interval, segment count).  Three damaged copies of one file are stored as
well: cut in mid-scan, a byte range of the scan zeroed, the scan replaced by FF fill; each was decoded by
tools/jpeg_decode_host_check.cpp under a sanitizer (non-zero status, no report) before it was recorded.  Needs numpy and PIL only; no
test runs it.

Before it writes, it checks on every case that the restatement tests/_jpeg_decode_ref.py reproduces Pillow's pixels in both modes,
that the restatement refuses the damaged copies, and that the case set exercises what the decoder can do (every counter of
``new_counters`` non-zero); tests/test_jpeg_decode_host.py asserts the recorded counters again.
usage: python tools/gen_jpeg_decode_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import _jpeg_decode_ref as ref  # noqa: E402

SHAPES = [(1, 1), (2, 3), (1, 4), (1, 5), (3, 6), (5, 4), (2, 7), (9, 5), (8, 8), (16, 16), (17, 33), (31, 18), (37, 53), (40, 3), (33, 48)]
BIG = (120, 160)
# name -> (luma sampling or None for one component, Pillow's save arguments)
ENCODINGS = {
    "420": ((2, 2), dict(subsampling=2, quality=75)),
    "422": ((2, 1), dict(subsampling=1, quality=90)),
    "444": ((1, 1), dict(subsampling=0, quality=95)),
    "grey": (None, dict(quality=50)),
    "420opt": ((2, 2), dict(subsampling=2, quality=30, optimize=True)),
    "422q100": ((2, 1), dict(subsampling=1, quality=100)),
    "420rst": ((2, 2), dict(subsampling=2, quality=90)),      # restart_marker_blocks 1, 2, 3 in turn
    "444rst": ((1, 1), dict(subsampling=0, quality=75)),
}


def content(kind, h, w, rng):
    if kind == "noise":
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if kind == "flat":
        return np.broadcast_to(np.array([200, 30, 90], dtype=np.uint8), (h, w, 3)).copy()
    y, x = np.mgrid[0:h, 0:w]
    v = np.stack([128 + 110 * np.sin(x / 5.0 + c) * np.cos(y / 4.0 - c) for c in range(3)], axis=-1) + rng.integers(-12, 13, size=(h, w, 3))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def pillow(img, grey, kw):
    f = io.BytesIO()
    (Image.fromarray(img[..., 0]) if grey else Image.fromarray(img)).save(f, "JPEG", **kw)
    data = f.getvalue()
    return data, np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).copy(), np.asarray(Image.open(io.BytesIO(data)).convert("L")).copy()


def main():
    rng = np.random.default_rng(20240915)
    arrays, names, k = {}, [], ref.new_counters()
    kinds = ["noise", "smooth", "flat"]

    def add(name, img, samp, kw):
        data, rgb, l = pillow(img, samp is None, kw)
        assert np.array_equal(ref.decode(data, "RGB", k), rgb), (name, "RGB")
        assert np.array_equal(ref.decode(data, "L"), l), (name, "L")
        hd = ref.walk(data)
        segs, _ = ref.segments(data, hd["scan_at"])
        h, w = img.shape[:2]
        hs, vs = samp or (1, 1)
        arrays[f"{name}/file"] = np.frombuffer(data, dtype=np.uint8)
        arrays[f"{name}/rgb"], arrays[f"{name}/l"] = rgb, l
        arrays[f"{name}/geometry"] = np.array([h, w, 1 if samp is None else 3, hs, vs, hd["restart"], len(segs)], dtype=np.int64)
        names.append(name)
        return data

    n = 0
    for h, w in SHAPES:
        for enc, (samp, kw) in ENCODINGS.items():
            kind = kinds[n % 3]
            kw = dict(kw)
            if enc.endswith("rst"):
                kw["restart_marker_blocks"] = 1 + n % 3
            add(f"{h}x{w}_{enc}_{kind}", content(kind, h, w, rng), samp, kw)
            n += 1
    add("120x160_422rows_smooth", content("smooth", *BIG, rng), (2, 1), dict(subsampling=1, quality=90, restart_marker_rows=1))
    # saturated colours next to each other: the colour conversion leaves 0..255 on both sides
    sat = np.zeros((16, 16, 3), dtype=np.uint8)
    sat[:, ::2] = (255, 0, 255)
    sat[::2, :, 1] = 255
    base = add("16x16_444_saturated", sat, (1, 1), dict(subsampling=0, quality=50))
    base = add("16x16_420_base", content("noise", 16, 16, rng), (2, 2), dict(subsampling=2, quality=75))
    at = ref.walk(base)["scan_at"]
    span = len(base) - 2 - at
    damaged = {"cut": base[:at + span // 2], "ff": base[:at] + b"\xFF" * span + base[-2:]}
    for lo in range(at + 8, at + span - 24):      # the first zeroed range the restatement cannot decode
        bad = base[:lo] + bytes(16) + base[lo + 16:]
        try:
            ref.decode(bad)
        except (AssertionError, IndexError, KeyError):
            damaged["zeroed"] = bad
            break
    for name, bad in damaged.items():
        try:
            ref.decode(bad)
        except (AssertionError, IndexError, KeyError):
            arrays[f"damaged/{name}"] = np.frombuffer(bad, dtype=np.uint8)
        else:
            raise SystemExit(f"the restatement decodes the damaged file {name}")
    print("coverage", k)
    for name, v in k.items():
        assert v > 0, f"the case set does not exercise {name}"
    arrays["names"] = np.array(names)
    arrays["damaged_names"] = np.array(sorted(damaged))
    arrays["counter_names"] = np.array(list(k))
    arrays["counter_values"] = np.array([int(v) for v in k.values()], dtype=np.int64)
    np.savez_compressed(ref.GOLDEN, **arrays)
    print("wrote", ref.GOLDEN, len(names), "cases", os.path.getsize(ref.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
