#!/usr/bin/env python3
"""Times the benchmark post-processing (diff_sal_amd.postprocess) with HIP events at the DHF1K evaluation shape: B = 64 predictions
of 224 x 384 -> annotations of 360 x 640.  Three entries: the 8-bit export alone (to_uint8), the order-1 resize and the order-3
resize (both with the clip, as protocol_metrics calls them).  Each time is the median of REGIONS regions of CALLS calls on a warmed
device and covers the whole Python entry point (output and workspace allocation included).  Beside each time stands its HBM floor:
the bytes that must cross HBM once (input read once, output written once) over the bandwidth a float4 copy reaches on the MI355X
(6.29 TB/s measured, of 8 TB/s peak), and the time as a multiple of that floor.  The kernels move more than the floor's bytes
(the export reads its input twice, order 3 keeps two float64 arrays of the input's size between its passes), most of it through
the caches.  A downscale leg follows (resize(..., anti_aliasing=True), orders 1 and 3 with the clip, and antialias alone) at
two targets: 180 x 320, where both Gaussian radii are 0 and the call is the plain zoom, and 100 x 120 (radii 2 and 4), where both
Gaussian passes run.  Prints one JSON line.
usage: python tools/bench_postprocess.py [B h w H W]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_sal_amd import postprocess as pp  # noqa: E402

B, h, w, H, W = (int(v) for v in sys.argv[1:6]) if len(sys.argv) >= 6 else (64, 224, 384, 360, 640)
WARM, REGIONS, CALLS = 5, 9, 20
HBM_BYTES_PER_S = 6.29e12

if not torch.cuda.is_available():
    raise SystemExit("bench_postprocess needs the GPU: a time taken elsewhere says nothing")
g = torch.Generator(device="cuda").manual_seed(0)
pred = torch.rand((B, h, w), device="cuda", generator=g)
m = pp.from_uint8(pp.to_uint8(pred))


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
    return statistics.median(ms), min(ms), max(ms)


def entry(fn, nbytes):
    med, lo, hi = timed(fn)
    floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
    return {"ms": med, "ms_min": lo, "ms_max": hi, "bytes_once_through": nbytes, "hbm_floor_ms": floor_ms, "times_floor": med / floor_ms}


res = {
    "shape": [B, h, w, H, W], "regions": REGIONS, "calls_per_region": CALLS, "hbm_bytes_per_s": HBM_BYTES_PER_S,
    "to_uint8": entry(lambda: pp.to_uint8(pred), B * h * w * 5),
    "resize_order1": entry(lambda: pp.resize(m, (H, W), order=1), B * (h * w + H * W) * 4),
    "resize_order3": entry(lambda: pp.resize(m, (H, W), order=3), B * (h * w + H * W) * 4),
}
for Hd, Wd in ((180, 320), (100, 120)):
    once = B * (h * w + Hd * Wd) * 4
    res[f"downscale_{Hd}x{Wd}"] = {
        "radii": [0 if g is None else len(g) - 1 for g in (pp.gaussian_weights(h, Hd), pp.gaussian_weights(w, Wd))],
        "antialias": entry(lambda: pp.antialias(m, (Hd, Wd)), B * h * w * 8),
        "resize_order1": entry(lambda: pp.resize(m, (Hd, Wd), order=1, anti_aliasing=True), once),
        "resize_order3": entry(lambda: pp.resize(m, (Hd, Wd), order=3, anti_aliasing=True), once),
    }
print(json.dumps(res))
