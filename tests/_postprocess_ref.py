"""NumPy restatement of the benchmark post-processing (include/diffsal.h, "benchmark post-processing"): the 8-bit export in
float32, byte / 255, and the spline resize in float64 -- a linear solve for the B-spline coefficients, then direct sums.  One image
at a time.  ``load_cases`` reads the fixtures of tools/gen_postprocess_golden.py.  Test-side only: the package never imports it."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "postprocess.npz")
ORDERS = (1, 3)


def load_cases():
    """{case: {"pred" [B, h, w] f32, "size" (H, W), "u8", "imread", "zoom{order}_f64", "zoom{order}_f32", "clip{order}_f64",
    "clip{order}_f32", optionally "fix", "gt", "expected" {metric: [B]}}}"""
    z = np.load(GOLDEN)
    out = {}
    for name in z["cases"]:
        name = str(name)
        pre = name + "/"
        c = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre) and not k.startswith(pre + "expected/")}
        c["size"] = tuple(int(v) for v in c["size"])
        exp = {k[len(pre) + 9:]: z[k] for k in z.files if k.startswith(pre + "expected/")}
        if exp:
            c["expected"] = exp
        out[name] = c
    return out


def to_uint8(x32):
    """normalize_data in float32; a flat image gives zeros (the reference divides by zero)."""
    x = np.asarray(x32, dtype=np.float32)
    mn, mx = x.min(), x.max()
    if not mx > mn:
        return np.zeros(x.shape, dtype=np.uint8)
    s = np.float32(255.0) / np.float32(mx - mn)
    v = ((x - mn).astype(np.float32) * s).astype(np.float32)
    return np.trunc(np.clip(v, np.float32(0), np.float32(255))).astype(np.uint8)


def from_uint8(q):
    return np.asarray(q).astype(np.float32) / np.float32(255)


def mirror(j, n):
    p = 2 * (n - 1)
    j = np.mod(j, p)
    return np.where(j > n - 1, p - j, j)


def _coefficients_axis0(s):
    """Solve (c[i-1] + 4 c[i] + c[i+1]) / 6 = s[i] along axis 0 under the whole-sample mirror boundary."""
    n = s.shape[0]
    A = np.zeros((n, n))
    for i in range(n):
        for d, wgt in ((-1, 1.0), (0, 4.0), (1, 1.0)):
            A[i, int(mirror(i + d, n))] += wgt / 6.0
    return np.linalg.solve(A, s)


def beta3(t):
    a = np.abs(t)
    return np.where(a < 1, (4 - 6 * a * a + 3 * a ** 3) / 6, np.where(a < 2, (2 - a) ** 3 / 6, 0.0))


def _axis_matrix(n, N, order):
    """[N, n] matrix that takes the samples (order 1) or coefficients (order 3) of an axis to the N output positions."""
    M = np.zeros((N, n))
    for o in range(N):
        x = (o + 0.5) * (n / N) - 0.5
        f = int(np.floor(x))
        if order == 1:
            taps = ((f, 1.0 - (x - f)), (f + 1, x - f))
        else:
            taps = tuple((k, float(beta3(x - k))) for k in range(f - 1, f + 3))
        for k, wgt in taps:
            M[o, int(mirror(k, n))] += wgt
    return M


def resize(x32, size, order=3, clip=True):
    """float64 result for one [h, w] float32 image."""
    if order not in ORDERS:
        raise ValueError(order)
    s = np.asarray(x32, dtype=np.float32).astype(np.float64)
    h, w = s.shape
    H, W = size
    if h < 2 or w < 2 or H < h or W < w:
        raise ValueError((h, w, H, W))
    c = s
    if order == 3:
        c = _coefficients_axis0(_coefficients_axis0(s.T).T)
    out = _axis_matrix(h, H, order) @ c @ _axis_matrix(w, W, order).T
    return np.clip(out, s.min(), s.max()) if clip else out


def big_input(B=2, h=224, w=384):
    """The input of the 224 x 384 case, too large to store: exact integer arithmetic, so every platform builds the same float32
    map.  A hash-like field of 251 levels with a plateau and a block of exact repeats."""
    b, y, x = np.meshgrid(np.arange(B, dtype=np.int64), np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    v = (x * x * 31 + y * y * 17 + x * y * 7 + b * 101 + (x // 5) * (y // 3)) % 251
    v[:, 40:60, 100:180] = 97                      # plateau
    v[:, 100:120, :64] = v[:, 130:150, 64:128]     # exact repeats
    return (v.astype(np.float32) * np.float32(0.0037) + np.float32(0.011)).astype(np.float32)


def sample_index(N, step, extra=()):
    """Rows / columns at which the larger cases are recorded: every ``step``-th, the last, and the given tile edges."""
    return np.array(sorted(set(range(0, N, step)) | {N - 1} | {e for e in extra if 0 <= e < N}), dtype=np.int64)
