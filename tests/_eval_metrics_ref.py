"""NumPy restatement of the benchmark metrics (include/diffsal.h, "benchmark metrics"; R/metrics/metrics.py): one image at a time,
float32 range normalisation as numpy does it on a float32 map, integer counts, fp64 trapezoids.  The device-generator layouts
(jitter, Borji locations, sAUC selection) are built on ``tests/_philox_ref.bits``.  Test-side only: the package never imports it."""
import os

import numpy as np

from tests import _philox_ref as philox

DRAW = 0x40000000      # | purpose: 0 jitter, 1 Borji locations, 2 sAUC keys
METRICS = ("auc_judd", "auc_borji", "auc_shuffled", "cc", "nss", "sim")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_metrics.npz")


def load_cases():
    """The fixtures of tools/gen_eval_metrics_golden.py: {case: inputs, location tables, n_rep, expected values per metric}."""
    z = np.load(GOLDEN)
    out = {}
    for name in z["cases"]:
        name = str(name)
        c = {k: z[f"{name}/{k}"] for k in ("pred", "gt", "fix", "other", "rand_borji", "rand_shuffled")}
        c["n_rep"] = int(z[f"{name}/n_rep"])
        c["expected"] = {k: z[f"{name}/expected/{k}"] for k in METRICS}
        out[name] = c
    return out


CASES = load_cases()


def _trapz(y, x):
    d = np.diff(x)
    return float((d * (y[1:] + y[:-1]) / 2.0).sum())


def normalize_range(s):
    """(s - min) / (max - min) in the array's own type (float32 for the AUC metrics: R/metrics/utils.py:47)."""
    return (s - s.min()) / (s.max() - s.min())


def _degenerate(S, F):
    return F.sum() == 0 or F.sum() == F.size or not (S.max() > S.min())


def jittered(s32, seed, image_id):
    """s' = float(double(s) + u * 1e-7), u = (word >> 8) * 2^-24, element p of purpose 0."""
    w = philox.bits(seed, [image_id], DRAW | 0, s32.size)[0]
    u = (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return (s32.ravel().astype(np.float64) + u * 1e-7).astype(np.float32)


def auc_judd(s32, fix):
    s = np.asarray(s32, dtype=np.float32).ravel()
    F = np.asarray(fix).ravel() > 0.5
    if _degenerate(s, F):
        return float("nan")
    S = normalize_range(s)
    S_fix = S[F]
    n_fix, n = len(S_fix), len(S)
    order = np.sort(S)
    thresholds = np.sort(S_fix)[::-1]
    above = n - np.searchsorted(order, thresholds, side="left")      # #{j : S_j >= thresh}
    k = np.arange(n_fix)
    tp = np.concatenate([[0.0], (k + 1) / float(n_fix), [1.0]])
    fp = np.concatenate([[0.0], (above - k - 1) / float(n - n_fix), [1.0]])
    return _trapz(tp, fp)


def auc_borji(s32, fix, locations, step=0.1):
    """locations: one integer array of pixel indices per repetition (entries < 0 are unused slots)."""
    s = np.asarray(s32, dtype=np.float32).ravel()
    F = np.asarray(fix).ravel() > 0.5
    if _degenerate(s, F):
        return float("nan")
    S = normalize_range(s)
    S_fix = S[F]
    n_fix = len(S_fix)
    auc = []
    for loc in locations:
        loc = np.asarray(loc)
        S_rand = S[loc[loc >= 0]]
        m = float(max(S_fix.max(), S_rand.max())) if len(S_rand) else float(S_fix.max())
        nt = int(np.ceil(m / step))
        th = (np.arange(nt) * step)[::-1]                # fp64 thresholds k * step, descending
        tp = np.concatenate([[0.0], [(S_fix >= t).sum() / float(n_fix) for t in th], [1.0]])
        fp = np.concatenate([[0.0], [(S_rand >= t).sum() / float(n_fix) for t in th], [1.0]])
        auc.append(_trapz(tp, fp))
    total = 0.0
    for a in auc:      # index order
        total += a
    return total / len(auc)


def cc(s32, g32):
    a, b = np.asarray(s32, dtype=np.float64).ravel(), np.asarray(g32, dtype=np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def nss(s32, fix):
    s = np.asarray(s32, dtype=np.float64).ravel()
    F = np.asarray(fix).ravel() > 0.5
    if _degenerate(s, F):
        return float("nan")
    return float(((s - s.mean()) / s.std())[F].mean())


def sim(s32, g32):
    a, b = np.asarray(s32, dtype=np.float64).ravel(), np.asarray(g32, dtype=np.float64).ravel()
    a, b = normalize_range(a), normalize_range(b)
    return float(np.minimum(a / a.sum(), b / b.sum()).sum())


def borji_locations(fix, seed, image_id, n_rep):
    """Purpose 1: element p * n_rep + rep, p a fixated pixel -> location (uint64(word) * n) >> 32.  One array per repetition."""
    F = np.asarray(fix).ravel() > 0.5
    n = F.size
    w = philox.bits(seed, [image_id], DRAW | 1, n * n_rep)[0].reshape(n, n_rep)
    loc = (w[F].astype(np.uint64) * np.uint64(n)) >> np.uint64(32)
    return [loc[:, r].astype(np.int64) for r in range(n_rep)]


def shuffled_locations(fix, other, seed, image_id, n_rep):
    """Purpose 2: element p * n_rep + rep is the key of pixel p of ``other``; a repetition takes the min(n_fix, n_other)
    pixels with the smallest (word, p) pairs."""
    F = np.asarray(fix).ravel() > 0.5
    O = np.nonzero(np.asarray(other).ravel() > 0.5)[0]
    n = F.size
    m = min(int(F.sum()), len(O))
    w = philox.bits(seed, [image_id], DRAW | 2, n * n_rep)[0].reshape(n, n_rep)
    out = []
    for r in range(n_rep):
        key = (w[O, r].astype(np.uint64) << np.uint64(32)) | O.astype(np.uint64)
        out.append(O[np.argsort(key, kind="stable")[:m]].astype(np.int64))
    return out


def auc_shuffled(s32, fix, other, locations, step=0.1):
    if (np.asarray(other).ravel() > 0.5).sum() == 0:
        return float("nan")
    return auc_borji(s32, fix, locations, step)
