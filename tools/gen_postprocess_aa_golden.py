"""Writes tests/golden/postprocess_aa.npz: float32 maps (byte / 255 of seeded maps, as ``plt.imread`` returns them) and what scipy
gives for the anti-aliased downscale skimage (>= 0.19) runs on them -- the Gaussian's weights (scipy's own table), the float32
``scipy.ndimage.gaussian_filter(map, sigma, mode='mirror')`` with ``sigma = max(0, (in / out - 1) / 2)`` per axis, and
``scipy.ndimage.zoom(filtered, ..., order, mode='mirror', grid_mode=True)`` for orders 1 and 3 with float64 and float32 output,
before and after the clip to the range of the UNFILTERED map.

    python tools/gen_postprocess_aa_golden.py [--host-check ./postprocess_gauss_host_check]

Needs numpy and scipy; no GPU.  The small cases are recorded in full.  The two 224 x 384 cases are recorded at a grid of rows and
columns (every few, the last, and the kernels' tile edges), stored with them (``frows`` / ``fcols`` for the filtered map, ``rows``
/ ``cols`` for the zooms); their input is not stored but rebuilt by ``tests/_postprocess_aa_ref.big_input``.  The tool also holds
the NumPy restatement (tests/_postprocess_aa_ref.py) to scipy on every pixel of every case: the Gaussian stage exactly, the zoom
to 1e-12.  ``--host-check PATH`` runs the sanitizer build of tools/postprocess_gauss_host_check.cpp over every case: its filtered
map must equal scipy's bit for bit.  No test runs this tool."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np
from scipy import ndimage
from scipy.ndimage import _filters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _postprocess_aa_ref as aref  # noqa: E402
from tests import _postprocess_ref as pref  # noqa: E402


def make_map(rng, B, h, w, flat=None):
    """byte / 255 of random maps with exact repeats and a plateau"""
    p = rng.random((B, h, w), dtype=np.float32)
    for b in range(B):
        v = p[b].reshape(-1)
        idx = rng.permutation(h * w)
        k = max(1, h * w // 6)
        v[idx[:k]] = v[idx[k:2 * k]]
        if h >= 4 and w >= 4:
            p[b, 1:3, 1:4] = p[b, 1, 1]
    if flat is not None:
        p[flat] = np.float32(0.375)
    return np.stack([pref.from_uint8(pref.to_uint8(q)) for q in p])


def edge_map():
    """12 x 20: isolated bright pixels and one-pixel lines on black, beside a block: every 1.0 has a 0.0 neighbour along both axes
    (the Gaussian lowers the maximum) and the cubic spline overshoots the steps on both sides"""
    m = np.zeros((1, 12, 20), dtype=np.float32)
    m[0, 2, 3] = m[0, 5, 9] = m[0, 9, 15] = 1.0
    m[0, 7, 2:7:2] = 1.0
    m[0, 3:6, 14] = 1.0
    m[0, 10, 5] = np.float32(128 / 255)
    return m


def scipy_weights(n, N):
    sigma = max(0.0, (n / N - 1) / 2)
    if not sigma > 1e-15:
        return sigma, None
    r = int(4.0 * sigma + 0.5)
    return sigma, _filters._gaussian_kernel1d(sigma, 0, r)[::-1][r:]


def host_check(path, m, wy, wx, want):
    with tempfile.TemporaryDirectory() as d:
        names = [os.path.join(d, n) for n in ("in.f32", "wy.f64", "wx.f64", "out.f32")]
        m.astype(np.float32).tofile(names[0])
        for g, n in ((wy, names[1]), (wx, names[2])):
            (np.zeros(0) if g is None else g).astype(np.float64).tofile(n)
        subprocess.check_call([path, names[0], str(m.shape[0]), str(m.shape[1]), names[1], names[2], names[3]])
        got = np.fromfile(names[3], dtype=np.float32).reshape(m.shape)
    assert np.array_equal(got, want), "the host check's filtered map differs from scipy's"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-check", help="the sanitizer build of tools/postprocess_gauss_host_check.cpp")
    args = ap.parse_args()
    out_path = os.path.join(ROOT, "tests", "golden", "postprocess_aa.npz")
    rng = np.random.default_rng(20241021)
    # filtered-map grid: the y tiles are 32 rows, the x segments 128 columns; zoom grid: interp tiles of 16 rows x 64 columns
    fgrid = (23, (31, 32, 63, 64, 191, 192), 29, (127, 128, 255, 256))
    specs = {      # name: (B, (h, w), (H, W), flat image, zoom grid)
        "a8x12": (2, (8, 12), (7, 9), None, None),              # radius 0 on one axis, 1 on the other
        "a16x24": (1, (16, 24), (7, 24), None, None),           # one axis untouched
        "a12x20": (2, (12, 20), (15, 11), None, None),          # one axis up, one down
        "a6x7": (1, (6, 7), (1, 2), None, None),                # radius 10 on 6 samples: several mirror folds
        "a5x200": (1, (5, 200), (5, 20), None, None),           # radius 18 across x segments
        "a70x33": (1, (70, 33), (20, 33), None, None),          # halo rows across y tiles
        "a33x70": (3, (33, 70), (16, 35), 1, None),             # a batch with a flat image
        "edge12x20": (1, (12, 20), (8, 13), None, None),        # filtered maximum below the maximum, cubic overshoot
        "big_strong": (2, (224, 384), (100, 120), None, (7, (15, 16, 31, 32, 63, 64), 9, (63, 64))),
        "big_mild": (2, (224, 384), (180, 320), None, (13, (15, 16, 31, 32, 127, 128), 19, (63, 64, 127, 128, 255, 256))),
    }
    blob = {"cases": np.array(list(specs))}
    for name, (B, (h, w), (H, W), flat, grid) in specs.items():
        big = name.startswith("big")
        m = aref.big_input() if big else edge_map() if name.startswith("edge") else make_map(rng, B, h, w, flat)
        assert m.shape == (B, h, w) and m.dtype == np.float32
        (sy, wy), (sx, wx) = scipy_weights(h, H), scipy_weights(w, W)
        for g, mine in ((wy, aref.gaussian_weights(h, H)), (wx, aref.gaussian_weights(w, W))):
            assert (g is None) == (mine is None) and (g is None or np.array_equal(g, mine)), name
        filtered = np.stack([ndimage.gaussian_filter(m[b], (sy, sx), mode="mirror") for b in range(B)])
        assert filtered.dtype == np.float32
        mine = np.stack([aref.gauss(m[b], wy, wx) for b in range(B)])
        assert np.array_equal(mine, filtered), (name, int((mine != filtered).sum()))      # the restatement: 0 differing pixels
        if args.host_check:
            for b in range(B):
                host_check(args.host_check, m[b], wy, wx, filtered[b])
        frows = pref.sample_index(h, fgrid[0], fgrid[1]) if big else np.arange(h)
        fcols = pref.sample_index(w, fgrid[2], fgrid[3]) if big else np.arange(w)
        rows = pref.sample_index(H, grid[0], grid[1]) if big else np.arange(H)
        cols = pref.sample_index(W, grid[2], grid[3]) if big else np.arange(W)
        if not big:
            blob[f"{name}/map"] = m
        blob[f"{name}/size"] = np.array([H, W], dtype=np.int64)
        blob[f"{name}/wy"] = np.zeros(0) if wy is None else wy
        blob[f"{name}/wx"] = np.zeros(0) if wx is None else wx
        blob[f"{name}/filtered"] = filtered[:, frows][:, :, fcols]
        blob[f"{name}/frows"], blob[f"{name}/fcols"], blob[f"{name}/rows"], blob[f"{name}/cols"] = frows, fcols, rows, cols
        lo = m.reshape(B, -1).min(1)[:, None, None]
        hi = m.reshape(B, -1).max(1)[:, None, None]
        print(f"{name}: sigma ({sy:.4f}, {sx:.4f}) radius ({0 if wy is None else len(wy) - 1}, {0 if wx is None else len(wx) - 1}); "
              f"input max {m.max()}, filtered max {filtered.max()}")
        for order in (1, 3):
            z64 = np.stack([ndimage.zoom(filtered[b].astype(np.float64), (H / h, W / w), order=order, mode="mirror", grid_mode=True)
                            for b in range(B)])
            z32 = np.stack([ndimage.zoom(filtered[b], (H / h, W / w), order=order, mode="mirror", grid_mode=True) for b in range(B)])
            assert z64.shape == (B, H, W) and z32.dtype == np.float32
            assert np.array_equal(z32, z64.astype(np.float32)), (name, order)      # scipy's float32 output is its float64 rounded once
            c64, c32 = np.clip(z64, lo, hi), np.clip(z32, lo, hi)
            assert np.array_equal(c32, c64.astype(np.float32))
            d = max(float(np.abs(aref.zoom(filtered[b], (H, W), order) - z64[b]).max()) for b in range(B))
            assert d <= 1e-12, (name, order, d)
            pick = lambda a: a[:, rows][:, :, cols]      # noqa: E731
            blob[f"{name}/zoom{order}_f64"], blob[f"{name}/zoom{order}_f32"] = pick(z64), pick(z32)
            blob[f"{name}/clip{order}_f64"], blob[f"{name}/clip{order}_f32"] = pick(c64), pick(c32)
            print(f"  order {order}: range before the clip [{z64.min()}, {z64.max()}], restatement |d| {d:.2e}")
            if name.startswith("edge") and order == 3:
                assert filtered.max() < m.max() and z64.max() > filtered.max() and z64.min() < m.min(), name
    np.savez_compressed(out_path, **blob)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
