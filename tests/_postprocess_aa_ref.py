"""NumPy restatement of the anti-aliased resize (include/diffsal.h, "benchmark post-processing", diffsal_map_resize_aa): the
Gaussian's weights, the Gaussian stage operation for operation as scipy's correlate1d runs a symmetric kernel (float64, one
rounding to float32 per axis, rows first), and the spline zoom of the filtered map at any ratio, built from the pieces of
tests/_postprocess_ref.py.  One image at a time.  ``load_cases`` reads the fixtures of tools/gen_postprocess_aa_golden.py.
Test-side only: the package never imports it."""
import os

import numpy as np

from tests import _postprocess_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "postprocess_aa.npz")
ORDERS = ref.ORDERS
BIG = ("big_strong", "big_mild")      # 224 x 384 inputs: rebuilt by ``big_input``, recorded on a grid


def load_cases():
    """{case: {"map" [B, h, w] f32 (absent for the 224 x 384 cases), "size" (H, W), "wy" / "wx" (centre first; empty = no pass),
    "filtered" f32, "frows" / "fcols" (the grid ``filtered`` is recorded at), "rows" / "cols" (the grid of the zooms),
    "zoom{order}_f64", "zoom{order}_f32", "clip{order}_f64", "clip{order}_f32"}}"""
    z = np.load(GOLDEN)
    out = {}
    for name in z["cases"]:
        name = str(name)
        pre = name + "/"
        c = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
        c["size"] = tuple(int(v) for v in c["size"])
        for k in ("wy", "wx"):
            c[k] = c[k] if c[k].size else None
        out[name] = c
    return out


def big_input():
    """The float map of the 224 x 384 cases: the byte / 255 of the 8-bit export of ``_postprocess_ref.big_input()``"""
    return np.stack([ref.from_uint8(ref.to_uint8(p)) for p in ref.big_input()])


def gaussian_weights(n, N):
    """r + 1 float64 weights of the axis n -> N, centre first, or None for sigma <= 1e-15"""
    sigma = max(0.0, (n / N - 1) / 2)
    if not sigma > 1e-15:
        return None
    r = int(4.0 * sigma + 0.5)
    k = np.arange(-r, r + 1)
    g = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    g = g / g.sum()
    return g[r:]


def _gauss_axis0(x32, g):
    """one pass along axis 0: acc = x[i] g[0]; for k = r .. 1: acc += (x[i - k] + x[i + k]) g[k]; float32(acc)"""
    x = np.asarray(x32, dtype=np.float32).astype(np.float64)
    n, r = x.shape[0], len(g) - 1
    i = np.arange(n)
    acc = x * g[0]
    for k in range(r, 0, -1):
        acc = acc + (x[ref.mirror(i - k, n)] + x[ref.mirror(i + k, n)]) * g[k]
    return acc.astype(np.float32)


def gauss(x32, wy, wx):
    """the Gaussian stage of one [h, w] float32 image: rows first, the second pass reads the float32 result of the first"""
    out = np.asarray(x32, dtype=np.float32)
    if wy is not None:
        out = _gauss_axis0(out, wy)
    if wx is not None:
        out = _gauss_axis0(out.T, wx).T
    return np.ascontiguousarray(out)


def zoom(x32, size, order=3):
    """float64 spline zoom of one [h, w] float32 image to any size (``_postprocess_ref.resize`` without its upscale-only check)"""
    s = np.asarray(x32, dtype=np.float32).astype(np.float64)
    h, w = s.shape
    H, W = size
    c = s
    if order == 3:
        c = ref._coefficients_axis0(ref._coefficients_axis0(s.T).T)
    return ref._axis_matrix(h, H, order) @ c @ ref._axis_matrix(w, W, order).T


def resize_aa(x32, size, order=3, clip=True):
    """float64 result for one [h, w] float32 image: filter where an axis shrinks, zoom, clip to the UNFILTERED range"""
    x = np.asarray(x32, dtype=np.float32)
    out = zoom(gauss(x, gaussian_weights(x.shape[0], size[0]), gaussian_weights(x.shape[1], size[1])), size, order)
    return np.clip(out, np.float64(x.min()), np.float64(x.max())) if clip else out
