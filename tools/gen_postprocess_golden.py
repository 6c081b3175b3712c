"""Writes tests/golden/postprocess.npz: seeded float32 maps and what the CPU libraries the benchmark protocol rests on give for
them -- the bytes of ``normalize_data``'s expression on float32 input, the floats ``plt.imread`` returns for a real in-memory PNG of
those bytes, ``scipy.ndimage.zoom(..., order, mode='mirror', grid_mode=True)`` of that float map for orders 1 and 3 with float64
and float32 output, before and after the clip to the input's range, and the metric rows of tests/_eval_metrics_ref.py on the
clipped float32 maps (order 3 for AUC-Judd, CC, SIM; order 1 for NSS, as the reference resizes them).

    python tools/gen_postprocess_golden.py

Needs numpy, scipy, PIL and matplotlib; no GPU.  The two larger cases are recorded at a grid of rows and columns (every few, the
last, and the kernels' tile edges), stored with them as ``rows`` / ``cols``; the input of the largest is not stored but rebuilt by
``tests/_postprocess_ref.big_input``.  No test runs this tool."""
import io
import os
import sys

import matplotlib.pyplot as plt
import numpy as np
from PIL import Image
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _eval_metrics_ref as mref  # noqa: E402
from tests import _postprocess_ref as pref  # noqa: E402


def normalize_data(data):      # the reference's expression (R/util/utils.py:11-16), on a float32 array
    data_min = np.min(data)
    data_max = np.max(data)
    return np.clip((data - data_min) * (255.0 / (data_max - data_min)), 0, 255).astype(np.uint8)


def png_roundtrip(q):
    buf = io.BytesIO()
    Image.fromarray(q).save(buf, format="PNG")
    buf.seek(0)
    out = plt.imread(buf, format="png")
    assert out.dtype == np.float32 and out.shape == q.shape
    return out


def make_pred(rng, B, h, w, flat=None, edge=False):
    """Random float32 maps with ties: exact repeats, a plateau, values on byte boundaries k / 255 of a [0, 1] range; ``edge``
    adds a step from the minimum to the maximum, which the cubic spline overshoots on both sides."""
    p = rng.random((B, h, w), dtype=np.float32)
    for b in range(B):
        n = h * w
        v = p[b].reshape(-1)
        idx = rng.permutation(n)
        k = max(1, n // 6)
        v[idx[:k]] = v[idx[k:2 * k]]                                         # exact repeats
        v[idx[2 * k:3 * k]] = (rng.integers(0, 256, size=k) / 255.0).astype(np.float32)      # byte boundaries once min = 0, max = 1
        v[idx[3 * k]], v[idx[3 * k + 1]] = 0.0, 1.0
        if h >= 4 and w >= 4:
            p[b, 1:3, 1:4] = p[b, 1, 1]                                      # plateau
        if edge:
            p[b, 4:7, 5:8], p[b, 4:7, 8:11] = 0.0, 1.0
    if flat is not None:
        p[flat] = np.float32(0.375)
    return p


def main():
    out_path = os.path.join(ROOT, "tests", "golden", "postprocess.npz")
    rng = np.random.default_rng(20240921)
    specs = {      # name: (B, (h, w), (H, W), flat image, metrics?, recorded grid)
        "s4x5": (2, (4, 5), (5, 9), None, False, None),                  # mirror periods 6 and 8: shorter than any truncation
        "s7x12": (2, (7, 12), (11, 20), None, True, None),               # the overshoot case
        "s2x3": (1, (2, 3), (2, 7), None, False, None),                  # n = 2, an equal axis
        "s33x70": (3, (33, 70), (67, 131), 1, True, (5, (31, 32, 63, 64, 65), 7, (63, 64, 65, 127, 128, 129))),
        "big": (2, (224, 384), (360, 640), None, False, (23, (3, 4, 31, 32, 255, 256), 29, (63, 64, 127, 128, 511, 512))),
    }
    blob = {"cases": np.array(list(specs))}
    for name, (B, (h, w), (H, W), flat, with_metrics, grid) in specs.items():
        pred = pref.big_input(B, h, w) if name == "big" else make_pred(rng, B, h, w, flat, edge=name == "s7x12")
        u8 = np.zeros((B, h, w), dtype=np.uint8)
        for b in range(B):
            if b != flat:
                u8[b] = normalize_data(pred[b])
            assert np.array_equal(u8[b], pref.to_uint8(pred[b])), (name, b)
        imread = np.stack([png_roundtrip(u8[b]) for b in range(B)])
        assert np.array_equal(imread, u8.astype(np.float32) / np.float32(255))
        rows = np.arange(H) if grid is None else pref.sample_index(H, grid[0], grid[1])
        cols = np.arange(W) if grid is None else pref.sample_index(W, grid[2], grid[3])
        if name != "big":
            blob[f"{name}/pred"] = pred
        blob[f"{name}/size"] = np.array([H, W], dtype=np.int64)
        blob[f"{name}/u8"] = u8 if grid is None or name != "big" else u8[:, ::7, ::5]
        blob[f"{name}/imread"] = imread if grid is None or name != "big" else imread[:, ::7, ::5]
        blob[f"{name}/rows"], blob[f"{name}/cols"] = rows, cols
        maps = {}
        for order in (1, 3):
            z64 = np.stack([ndimage.zoom(imread[b].astype(np.float64), (H / h, W / w), order=order, mode="mirror", grid_mode=True)
                            for b in range(B)])
            z32 = np.stack([ndimage.zoom(imread[b], (H / h, W / w), order=order, mode="mirror", grid_mode=True) for b in range(B)])
            assert z64.shape == (B, H, W) and z32.dtype == np.float32
            assert np.array_equal(z32, z64.astype(np.float32)), (name, order)      # scipy's float32 output is its float64 rounded once
            lo = imread.reshape(B, -1).min(1)[:, None, None]
            hi = imread.reshape(B, -1).max(1)[:, None, None]
            c64, c32 = np.clip(z64, lo, hi), np.clip(z32, lo, hi)
            assert np.array_equal(c32, c64.astype(np.float32))
            maps[order] = c32
            pick = lambda a: a[:, rows][:, :, cols]      # noqa: E731
            blob[f"{name}/zoom{order}_f64"], blob[f"{name}/zoom{order}_f32"] = pick(z64), pick(z32)
            blob[f"{name}/clip{order}_f64"], blob[f"{name}/clip{order}_f32"] = pick(c64), pick(c32)
            print(name, "order", order, "range before the clip", z64.min(), z64.max())
            if name == "s7x12" and order == 3:      # every image of the overshoot case overshoots on both sides
                assert (z64.reshape(B, -1).min(1) < -0.01).all() and (z64.reshape(B, -1).max(1) > 1.01).all()
        if with_metrics:
            n = H * W
            fix = np.zeros((B, n), dtype=np.uint8)
            for b in range(B):
                fix[b, rng.choice(n, max(5, n // 40), replace=False)] = 1
            fix = fix.reshape(B, H, W)
            gt = (rng.integers(0, 16, size=(B, H, W)) / 15.0).astype(np.float32) ** 2
            blob[f"{name}/fix"], blob[f"{name}/gt"] = fix, gt
            exp = {"auc_judd": [mref.auc_judd(maps[3][b], fix[b]) for b in range(B)],
                   "cc": [mref.cc(maps[3][b], gt[b]) if b != flat else np.nan for b in range(B)],
                   "nss": [mref.nss(maps[1][b], fix[b]) for b in range(B)],
                   "sim": [mref.sim(maps[3][b], gt[b]) if b != flat else np.nan for b in range(B)]}
            for k, v in exp.items():
                blob[f"{name}/expected/{k}"] = np.array(v, dtype=np.float64)
                print(name, k, v)
    np.savez_compressed(out_path, **blob)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
