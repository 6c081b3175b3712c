#!/usr/bin/env python
"""Writes tests/golden/png_encode.npz: the inputs of the PNG export's tests, the files the NumPy restatement
(tests/_png_encode_ref.py) makes of them and the restatement's coverage counters: the fixtures of tests/test_png_encode_host.py and
tests/test_gpu_png_encode.py.  Needs numpy, zlib and PIL only; no diff_sal_amd, no GPU.

The cases are the smallest shapes at which each stage can go wrong: no row above, no pixel to the left, rows that are no multiple of
four bytes, the widest row, a stream that is one run, no match at all, two segments of large bytes (the Adler sums), a stream of
exactly one segment, a second segment of one byte (smooth and as a run cut at the boundary), a second segment that opens with a
match, rows with runs of exactly 2, 3, 257 .. 261, 516 and 517 equal bytes, two crafted maps that drive the literal/length code past
15 bits and the code-length code past 7 bits before limiting, and three saliency-like maps.  Before it writes, every file is decoded
by zlib and by Pillow back to the input, and every coverage counter must be non-zero.

--host-check PATH: the sanitizer build of tools/png_encode_host_check.cpp; its file of every case must equal the restatement's.

usage: python tools/gen_png_encode_golden.py [--host-check ./png_encode_host_check]"""
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
from tests import _png_encode_ref as ref  # noqa: E402

RUNS = (2, 3, 257, 258, 259, 260, 261, 516, 517)


def eq_runs(stream: np.ndarray):
    """the lengths of the maximal runs of positions that equal the byte in front of them (one segment)"""
    eq = np.concatenate([[False], stream[1:] == stream[:-1], [False]])
    edges = np.flatnonzero(np.diff(eq.astype(np.int8)))
    return (edges[1::2] - edges[0::2]).tolist()


def runs_map(rng):
    """one row: constant stretches between noise.  Under the Sub filter a stretch of k pixels is one difference and k - 1 zeros:
    k - 2 positions that equal the byte in front of them"""
    parts = []
    for r in RUNS:
        parts.append(rng.randint(40, 216, size=12))
        parts.append(np.full(r + 2, rng.randint(100, 250)))
    parts.append(rng.randint(40, 216, size=12))
    return np.concatenate(parts).astype(np.uint8)[None]


def spread(counts):
    """byte values with the given counts in an order that never holds four equal bytes in a row: the commonest value that may
    stand next, else the next commonest"""
    left = dict(counts)
    out = []
    while left:
        order = sorted(left, key=lambda v: (-left[v], v))
        pick = order[0]
        if len(out) >= 2 and out[-1] == pick and out[-2] == pick:
            if len(order) == 1:
                raise ValueError("cannot avoid a run")
            pick = order[1]
        out.append(pick)
        left[pick] -= 1
        if not left[pick]:
            del left[pick]
    return out


def from_filtered_sub(fbytes):
    """the one-row map whose Sub-filtered bytes are fbytes (the running sum modulo 256)"""
    return (np.cumsum(np.asarray(fbytes, dtype=np.int64)) % 256).astype(np.uint8)[None]


def limit15_map():
    """symbol counts 1 1 1 3 4 7 11 18 ...: each above the sum of all before the one in front of it, so Huffman's tree is a chain
    17 deep.  The counts include the end-of-block symbol (1) and the row's filter byte (a literal 1)"""
    w = [1, 1, 1]
    while len(w) < 17:
        w.append(sum(w[:-1]) + 1)
    w.sort()
    counts = {}
    values = list(range(16, -1, -1))      # the commonest symbol is byte 0, the rarest byte 15; byte 16 stands for the end symbol
    for k, c in enumerate(w[1:]):         # w[0] is the end-of-block symbol
        counts[values[k + 1]] = c
    counts[1] -= 1                        # the filter byte
    return from_filtered_sub(spread({v: c for v, c in counts.items() if c}))


def limit7_map():
    """a dyadic histogram (count 2^(13 - length), 8192 tokens with the end symbol) fixes the literal lengths: 25 of length 6, 41 of 7,
    67 of 8, 9 of 9, 5 of 10, 3 of 11, 13 of 12, 2 of 13 (byte 0 and the end symbol), 92 unused bytes in one run.  The code-length
    symbols then count 1 (18) 1 (the distance length) 2 3 5 9 13 25 41 67: a chain 9 deep"""
    want = {6: 25, 7: 41, 8: 67, 9: 9, 10: 5, 11: 3, 12: 13}
    assert sum(n << (13 - v) for v, n in want.items()) + 2 == 8192
    lengths = []
    left = dict(want)
    while left:      # never three equal lengths side by side: no use of symbol 16 disturbs the counts
        order = sorted(left, key=lambda v: (-left[v], v))
        pick = order[0]
        if len(lengths) >= 2 and lengths[-1] == pick and lengths[-2] == pick:
            pick = order[1]
        lengths.append(pick)
        left[pick] -= 1
        if not left[pick]:
            del left[pick]
    values = list(range(1, 82)) + list(range(174, 256))      # bytes 82..173 stay unused: one run of 92 zeros
    assert len(values) == len(lengths) == 163
    counts = {v: 1 << (13 - n) for v, n in zip(values, lengths)}
    counts[0] = 1
    counts[1] -= 1      # the filter byte
    return from_filtered_sub(spread(counts))


def cases():
    rng = np.random.RandomState(20260)
    noise = lambda h, w, lo=0: rng.randint(lo, 256, size=(h, w)).astype(np.uint8)      # noqa: E731
    out = {
        "1x1": noise(1, 1), "1x5": noise(1, 5), "300x1": noise(300, 1),
        "7x13_smooth": ref.saliency_like(1, 7, 13, blobs=1), "17x33_smooth": ref.saliency_like(2, 17, 33, blobs=2),
        "2x8192_smooth_noise": ref.saliency_like(3, 2, 8192, blobs=3, noise=3),
        "16x16_zeros": np.zeros((16, 16), dtype=np.uint8),
        "33x48_noise": noise(33, 48),
        "120x160_noise_large": noise(120, 160, 200),
        "128x127_smooth": ref.saliency_like(4, 128, 127),
        "113x144_smooth": ref.saliency_like(5, 113, 144),
        "113x144_zeros": np.zeros((113, 144), dtype=np.uint8),
        "130x130_zeros": np.zeros((130, 130), dtype=np.uint8),
        "1xW_runs": runs_map(rng), "1xW_limit15": limit15_map(), "1xW_limit7": limit7_map(),
        "64x70_blobs_a": ref.saliency_like(6, 64, 70), "64x70_blobs_b": ref.saliency_like(7, 64, 70, blobs=2),
        "64x70_blobs_noise": ref.saliency_like(8, 64, 70, noise=10),
    }
    return {n.replace("1xW", f"1x{v.shape[1]}"): v for n, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-check", help="the sanitizer build of tools/png_encode_host_check.cpp")
    ap.add_argument("--out", default=ref.GOLDEN)
    args = ap.parse_args()
    total = ref.new_counters()
    store = {}
    names = []
    for k, (name, img) in enumerate(cases().items()):
        H, W = img.shape
        assert name.startswith(f"{H}x{W}"), (name, img.shape)
        one = ref.new_counters()
        data = ref.encode(img, one)
        for n, v in one.items():
            total[n] += v
        # from the outside: zlib and Pillow read the input back
        idat = data[41:-16]
        raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(H, W + 1)
        assert raw[:, 0].max() <= 4
        back = np.asarray(Image.open(io.BytesIO(data)))
        assert back.dtype == np.uint8 and np.array_equal(back, img), name
        assert len(data) <= ref.capacity(H, W)
        if name.endswith("_runs"):
            assert raw[0, 0] == 1 and set(RUNS) <= set(eq_runs(raw.reshape(-1))), eq_runs(raw.reshape(-1))
        if name.endswith("_limit15"):
            assert one["limit15"] == 1 and raw[0, 0] == 1, one
        if name.endswith("_limit7"):
            assert one["limit7"] == 1 and one["limit15"] == 0 and raw[0, 0] == 1, one
        if name == "128x127_smooth":
            assert one["full_segment"] == 1 and one["segment_of_1"] == 0
        if name.startswith("113x144"):
            assert one["full_segment"] == 1 and one["segment_of_1"] == 1
        if name == "130x130_zeros":
            assert one["previous_segment"] == 1
        if name == "33x48_noise":
            assert all(r < 3 for r in eq_runs(raw.reshape(-1))), "a match in the noise"
        if args.host_check:
            with tempfile.TemporaryDirectory() as d:
                src, dst = os.path.join(d, "in.raw"), os.path.join(d, "out.png")
                img.tofile(src)
                subprocess.run([args.host_check, src, str(H), str(W), dst], check=True)
                with open(dst, "rb") as f:
                    assert f.read() == data, f"{name}: the host check's file differs from the restatement's"
        names.append(name)
        store[f"img_{k}"] = img
        store[f"file_{k}"] = np.frombuffer(data, dtype=np.uint8)
        print(f"{name}: {len(data)} bytes, capacity {ref.capacity(H, W)}")
    for n in ref.COUNTERS:
        assert total[n] > 0, f"no case exercises {n}"
    print(total)
    np.savez_compressed(args.out, names=np.array(names), counter_names=np.array(ref.COUNTERS), counters=np.array([total[n] for n in ref.COUNTERS]),
                        **store)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes" + ("" if args.host_check else " (the host check was not run)"))


if __name__ == "__main__":
    main()
