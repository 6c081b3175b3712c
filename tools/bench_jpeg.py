#!/usr/bin/env python3
"""Times the JPEG export (diff_sal_amd.jpeg) with HIP events at the evaluation shape of the audio-visual sets: B = 64 maps of
224 x 384, quality 95.  Three entries: ``encode`` (the files), ``encode`` with the read-back pixels, and ``roundtrip`` (the pixels
alone, one launch).  Each time is the median of REGIONS regions of CALLS calls on a warmed device and covers the whole Python entry
point (output and workspace allocation included).  Beside them stands the host path the export replaces, on the same machine: one
device-to-host copy of the uint8 maps plus Pillow's encoder in a pool of 16 threads (wall clock around a synchronise; Pillow's
encoder releases the GIL), which is what a user had to do per batch to get the same files.  The input is saliency-like (smooth blobs
with mild noise, quantised by ``postprocess.to_uint8``), because the coder's work depends on the content.  Prints one JSON line.
usage: python tools/bench_jpeg.py [B h w]"""
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_sal_amd import jpeg  # noqa: E402
from diff_sal_amd import postprocess as pp  # noqa: E402

B, h, w = (int(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (64, 224, 384)
WARM, REGIONS, CALLS, HOST_THREADS = 5, 9, 200, 16

if not torch.cuda.is_available():
    raise SystemExit("bench_jpeg needs the GPU: a time taken elsewhere says nothing")
g = torch.Generator(device="cuda").manual_seed(0)
yy, xx = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
pred = torch.zeros((B, h, w), device="cuda")
for _ in range(4):
    cy, cx = torch.rand((B, 1, 1), device="cuda", generator=g) * h, torch.rand((B, 1, 1), device="cuda", generator=g) * w
    s = 12 + 48 * torch.rand((B, 1, 1), device="cuda", generator=g)
    pred += torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
pred += 0.01 * torch.rand((B, h, w), device="cuda", generator=g)
u8 = pp.to_uint8(pred)


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


def host_path():
    from PIL import Image

    def one(img):
        f = io.BytesIO()
        Image.fromarray(img).save(f, "JPEG", quality=95)
        return f.getvalue()

    with ThreadPoolExecutor(HOST_THREADS) as pool:
        ms = []
        for i in range(WARM + REGIONS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            files = list(pool.map(one, u8.cpu().numpy()))
            if i >= WARM:
                ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "threads": HOST_THREADS}, files


data, lengths = jpeg.encode(u8)
n = lengths.cpu().numpy()
res = {
    "shape": [B, h, w], "quality": 95, "regions": REGIONS, "calls_per_region": CALLS,
    "file_bytes_mean": float(n.mean()), "capacity": jpeg.capacity(h, w),
    "launches": {"encode": "1 clear + 6 kernels", "roundtrip": "1 kernel"},
    "encode": timed(lambda: jpeg.encode(u8)),
    "encode_with_decoded": timed(lambda: jpeg.encode(u8, return_decoded=True)),
    "roundtrip": timed(lambda: jpeg.roundtrip(u8)),
}
try:
    res["host_copy_plus_pillow"], files = host_path()
    host = data.cpu().numpy()
    res["files_equal_pillow"] = all(host[b, :n[b]].tobytes() == files[b] for b in range(B))
except ImportError:
    res["host_copy_plus_pillow"] = "not measured: PIL does not import"
print(json.dumps(res))
