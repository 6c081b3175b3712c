#!/usr/bin/env python3
"""Times diff_sal_amd.eval_metrics.benchmark_metrics with HIP events at the DHF1K validation shape: B = 64 frames of 360 x 640 with
300 fixations each (`other`: 3000 fixated pixels), Borji / sAUC locations from the device generator with n_rep = 100.
Prints one JSON line: ms per call for the shared passes alone (NSS only: stats + image + prep + final), AUC-Judd alone, each
sweep alone and all six metrics, and the compare rate of the Judd count pass (B n n_fix compares over Judd minus shared time).
Every time is of the whole Python entry point (workspace allocation, uint8 conversion of the maps, NaN fill of the output), and
Judd minus shared still holds the rank kernel, Judd's share of `final` and two launches: the compare rate printed is a lower bound
on the count kernel's own rate.
usage: python tools/bench_eval_metrics.py [B H W n_fix]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_sal_amd import eval_metrics as em  # noqa: E402

B, H, W, NFIX = (int(v) for v in sys.argv[1:5]) if len(sys.argv) >= 5 else (64, 360, 640, 300)
NOTHER, NREP, WARM, REP = 10 * NFIX, 100, 3, 20

g = torch.Generator(device="cuda").manual_seed(0)
pred = torch.rand((B, 1, H, W), device="cuda", generator=g)
gt = torch.rand((B, 1, H, W), device="cuda", generator=g) ** 2


def points(k):
    m = torch.zeros((B, H * W), dtype=torch.uint8, device="cuda")
    idx = torch.rand((B, H * W), device="cuda", generator=g).topk(k, dim=1).indices
    return m.scatter_(1, idx, 1).view(B, H, W)


fix, other = points(NFIX), points(NOTHER)
ids = torch.arange(B, dtype=torch.int64, device="cuda")
seed = torch.tensor([1], dtype=torch.int64, device="cuda")


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REP):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REP


kw = dict(n_rep=NREP, seed=seed, image_ids=ids)
res = {
    "shape": [B, H, W], "n_fix": NFIX, "n_other": NOTHER, "n_rep": NREP,
    "shared_ms": timed(lambda: em.benchmark_metrics(pred, fix, metrics=("nss",))),
    "judd_ms": timed(lambda: em.benchmark_metrics(pred, fix, metrics=("auc_judd",))),
    "borji_ms": timed(lambda: em.benchmark_metrics(pred, fix, metrics=("auc_borji",), **kw)),
    "sauc_ms": timed(lambda: em.benchmark_metrics(pred, fix, other=other, metrics=("auc_shuffled",), **kw)),
    "all_six_ms": timed(lambda: em.benchmark_metrics(pred, fix, gt, other, **kw)),
}
count_ms = res["judd_ms"] - res["shared_ms"]
res["judd_count_ms"] = count_ms
res["judd_compares"] = B * H * W * NFIX
res["judd_gcompares_per_s"] = B * H * W * NFIX / (count_ms * 1e-3) / 1e9 if count_ms > 0 else None
res["map_bytes"] = B * H * W * 5
print(json.dumps(res))
