"""Writes tests/golden/eval_metrics.npz: seeded inputs, the explicit random-location tables and the values the reference's
R/metrics/metrics.py gives for them on the CPU (AUC_Judd with jitter=False, AUC_Borji, AUC_shuffled on float32 maps; CC, NSS, SIM on
float64 copies of the same float32 values).

    python tools/gen_eval_metrics_golden.py --reference /path/to/reference/checkout

The reference's module is imported as it is.  It imports ``skimage`` for the resize of mismatched shapes, which is never called
here (all shapes match), so a three-name stand-in is enough when skimage is not installed.  Both AUC_Borji and AUC_shuffled go
through AUC_Borji's ``rand_sampler`` hook with samplers of this file, so that the sampled pixel indices can be recorded: Borji
draws n_fix uniform locations per repetition, sAUC a permutation prefix of the other map's fixated pixels, as the reference's
own samplers do.  Nothing of the reference is written to the file but numbers; no test runs this tool."""
import argparse
import importlib
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_reference(path):
    try:
        importlib.import_module("skimage")
    except ImportError:
        sk = types.ModuleType("skimage")
        sk.transform = types.ModuleType("skimage.transform")
        sk.exposure = types.ModuleType("skimage.exposure")
        sk.img_as_float = lambda x: np.asarray(x, dtype=np.float64)

        def resize(*a, **k):
            raise RuntimeError("the fixtures never resize")
        sk.transform.resize = resize
        sys.modules.update({"skimage": sk, "skimage.transform": sk.transform, "skimage.exposure": sk.exposure})
    sys.path.insert(0, path)
    return importlib.import_module("metrics.metrics")


def make_case(rng, H, W, n_fixes, n_rep, levels=0):
    B, n = len(n_fixes), H * W
    pred = rng.random((B, H, W), dtype=np.float32)
    if levels:
        pred = (np.floor(pred * levels) / levels).astype(np.float32)
    gt = rng.random((B, H, W), dtype=np.float32) ** 2
    fix = np.zeros((B, n), dtype=np.uint8)
    other = np.zeros((B, n), dtype=np.uint8)
    for b, nf in enumerate(n_fixes):
        fix[b, rng.choice(n, nf, replace=False)] = 1
        other[b, rng.choice(n, min(n, max(3, (3 * nf) // 2 if b % 2 == 0 else nf // 2)), replace=False)] = 1
    return dict(pred=pred, gt=gt, fix=fix.reshape(B, H, W), other=other.reshape(B, H, W), n_rep=n_rep)


def score(M, case, rng):
    pred, gt, fix, other, n_rep = case["pred"], case["gt"], case["fix"], case["other"], case["n_rep"]
    B = pred.shape[0]
    n = pred[0].size
    cap = int(fix.reshape(B, -1).sum(1).max())
    rb = -np.ones((B, n_rep, cap), dtype=np.int32)
    rs = -np.ones((B, n_rep, cap), dtype=np.int32)
    exp = {k: np.zeros(B) for k in ("auc_judd", "auc_borji", "auc_shuffled", "cc", "nss", "sim")}
    for b in range(B):
        def uniform(S, F, n_rep_, n_fix, b=b):
            r = rng.integers(0, n, size=(n_fix, n_rep_))
            rb[b, :, :n_fix] = r.T
            return S[r]

        def from_other(S, F, n_rep_, n_fix, b=b):
            fixated = np.nonzero(other[b].ravel())[0]
            r = np.stack([fixated[rng.permutation(len(fixated))[:n_fix]] for _ in range(n_rep_)], axis=1)
            rs[b, :, :r.shape[0]] = r.T
            return S[r]

        exp["auc_judd"][b] = M.AUC_Judd(pred[b].copy(), fix[b], jitter=False)
        exp["auc_borji"][b] = M.AUC_Borji(pred[b].copy(), fix[b], n_rep, 0.1, uniform)
        exp["auc_shuffled"][b] = M.AUC_Borji(pred[b].copy(), fix[b], n_rep, 0.1, from_other)
        p64, g64 = pred[b].astype(np.float64), gt[b].astype(np.float64)
        exp["cc"][b] = M.CC(p64, g64)
        exp["nss"][b] = M.NSS(p64, fix[b])
        exp["sim"][b] = M.SIM(p64, g64)
    return rb, rs, exp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (the directory that holds metrics/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "eval_metrics.npz"))
    args = ap.parse_args()
    warnings.simplefilter("ignore", DeprecationWarning)      # np.trapz
    M = load_reference(os.path.abspath(args.reference))
    rng = np.random.default_rng(20240607)
    cases = {
        "small": make_case(rng, 24, 40, [1, 37, 24 * 40 - 1], 10),       # one fixation, a few, a single non-fixated pixel
        "odd": make_case(rng, 23, 37, [50, 11], 10),                     # odd sizes: every tail path
        "tiles": make_case(rng, 96, 160, [700], 6),                      # several pixel chunks and fixation tiles, neither a multiple
        "ties": make_case(rng, 24, 40, [60, 300], 10, levels=8),         # a map quantised to 8 levels
    }
    blob = {"cases": np.array(sorted(cases))}
    for name, case in cases.items():
        rb, rs, exp = score(M, case, rng)
        for k in ("pred", "gt", "fix", "other"):
            blob[f"{name}/{k}"] = case[k]
        blob[f"{name}/n_rep"] = np.int64(case["n_rep"])
        blob[f"{name}/rand_borji"], blob[f"{name}/rand_shuffled"] = rb, rs
        for k, v in exp.items():
            blob[f"{name}/expected/{k}"] = v
            print(name, k, v)
    np.savez_compressed(args.out, **blob)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
