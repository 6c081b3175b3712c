#!/usr/bin/env python3
"""Times the PNG export (diff_sal_amd.png.encode / save_predictions) with HIP events at the evaluation shape of the visual sets:
B in {1, 4, 64} maps of 224 x 384, in one process.  Per B: ``encode`` (the files in device memory; the median of REGIONS regions of
CALLS calls on a warmed device, the whole Python entry point with output and workspace allocation); ``png.save_predictions`` end to
end (quantise, encode, two host copies, the files written) against ``postprocess.save_predictions`` (quantise, one host copy,
Pillow's encoder once per file, serially), the path it replaces, on the same predictions into a fresh directory each (wall clock
around a synchronise); the ratio of the files' sizes to Pillow's.  The input is saliency-like (smooth blobs on a flat background
with mild noise), because the coder's work depends on the content.  Prints one JSON line.  Start it under a time limit:
usage: timeout 300 python tools/bench_png_encode.py"""
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_sal_amd import png  # noqa: E402
from diff_sal_amd import postprocess as pp  # noqa: E402

h, w = 224, 384
WARM, REGIONS, CALLS, SAVES = 5, 9, 50, 5

if not torch.cuda.is_available():
    raise SystemExit("bench_png_encode needs the GPU: a time taken elsewhere says nothing")


def predictions(B):
    g = torch.Generator(device="cuda").manual_seed(B)
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    pred = torch.zeros((B, h, w), device="cuda")
    for _ in range(4):
        cy, cx = torch.rand((B, 1, 1), device="cuda", generator=g) * h, torch.rand((B, 1, 1), device="cuda", generator=g) * w
        s = 12 + 48 * torch.rand((B, 1, 1), device="cuda", generator=g)
        pred += torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    pred = (pred - 0.08).clamp_min(0)      # a flat background, as the sampler's maps have
    return pred + 0.004 * torch.rand((B, h, w), device="cuda", generator=g) * (pred > 0)


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REGIONS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / CALLS)
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def saved(fn, pred, B):
    """wall clock of fn(pred, video ids, frame ids, root) into a fresh directory, and the files' sizes"""
    ms, sizes = [], None
    vids, fids = [f"v{b // 16}" for b in range(B)], list(range(1, B + 1))
    for i in range(1 + SAVES):
        with tempfile.TemporaryDirectory() as root:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            paths = fn(pred, vids, fids, root)
            if i:
                ms.append((time.perf_counter() - t0) * 1e3)
            sizes = [os.path.getsize(p) for p in paths]
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}, sizes


res = {"shape": [h, w], "regions": REGIONS, "calls_per_region": CALLS, "saves": SAVES, "launches": "1 clear + 5 kernels", "capacity": png.capacity(h, w)}
for B in (1, 4, 64):
    pred = predictions(B)
    u8 = pp.to_uint8(pred)
    one = {"encode": timed(lambda: png.encode(u8))}
    one["png_save_predictions"], ours = saved(png.save_predictions, pred, B)
    try:
        one["postprocess_save_predictions"], pillow = saved(pp.save_predictions, pred, B)
        one["file_bytes_mean"], one["pillow_file_bytes_mean"] = sum(ours) / B, sum(pillow) / B
        one["size_ratio_to_pillow"] = sum(ours) / sum(pillow)
    except ImportError:
        one["postprocess_save_predictions"] = "not measured: PIL does not import"
        one["file_bytes_mean"] = sum(ours) / B
    res[f"B{B}"] = one
print(json.dumps(res))
