#!/usr/bin/env python3
"""Times the PNG decode (diff_sal_amd.png.decode) at the frame size of the visual sets: N = 1, 16 and 64 files of 360 x 640, RGB
(the frames) and L (the annotation maps), written by Pillow with its defaults from video-like synthetic content (smooth shapes, a
fixed texture, mild noise), generated on the fly.  Per entry: the device time per call from events around the two launches on
descriptors already uploaded (``device_ms``; the split between the two launches comes from ``--trace``), the wall clock of ``png.decode`` end to
end -- the host's chunk walk, the one copy, the launches -- around a synchronise, ``pack_ms`` for the host part alone, and beside
them the path it replaces on the same machine: Pillow decoding the same files on one thread.  Warm-up, then the median of REGIONS
timed regions per entry.  Also prints t(N = 64) / t(N = 1) of the device time: files are independent workgroups, so a ratio
anywhere near 64 would mean the launch serialises them.  Prints one JSON line.

``--trace`` runs three decodes of each N = 1 and N = 64 set and nothing else: run it under ``rocprofv3 --kernel-trace --stats`` for
the time of each launch (``png_inflate_kernel``, ``png_unfilter_kernel``).
usage: python tools/bench_png_decode.py [--trace]"""
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_sal_amd import ops, png  # noqa: E402

H, W, WARM, REGIONS = 360, 640, 3, 9

if not torch.cuda.is_available():
    raise SystemExit("bench_png_decode needs the GPU: a time taken elsewhere says nothing")
from PIL import Image  # noqa: E402


def frames(n):
    """n video-like uint8 frames [360, 640, 3]: drifting gradients and blobs, a fixed texture, noise of a few levels"""
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    texture = rng.integers(-18, 19, size=(H, W, 1)).astype(np.float32)
    out = []
    for t in range(n):
        base = np.stack([128 + 90 * np.sin((x + 3 * t) / (40.0 + 9 * c)) * np.cos((y - 2 * t) / (31.0 + 5 * c)) for c in range(3)], axis=-1)
        blob = 70 * np.exp(-((x - 320 - 2 * t) ** 2 + (y - 180) ** 2) / (2 * 60.0 ** 2))[..., None]
        out.append(np.clip(base + blob + texture + rng.integers(-4, 5, size=(H, W, 3)), 0, 255).astype(np.uint8))
    return out


def maps(n):
    """n annotation-like uint8 maps [360, 640]: a few drifting Gaussian blobs on black"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    out = []
    for t in range(n):
        m = sum(np.exp(-((x - 160 * k - 3 * t) ** 2 + (y - 90 * k) ** 2) / (2 * (25.0 + 10 * k) ** 2)) for k in (1, 2, 3))
        out.append(np.clip(255 * m / m.max(), 0, 255).astype(np.uint8))
    return out


def files_of(imgs):
    out = []
    for img in imgs:
        f = io.BytesIO()
        Image.fromarray(img).save(f, "PNG")
        out.append(f.getvalue())
    return out


def wall(fn):
    ms = []
    for i in range(WARM + REGIONS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= WARM:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def host_only(fn):
    ms = []
    for i in range(WARM + REGIONS):
        t0 = time.perf_counter()
        fn()
        if i >= WARM:
            ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def device_only(files, mode):
    """events around ops.png_decode on an uploaded buffer: the two launches (and the allocator's work for out, status, workspace)"""
    p = png.pack(files)
    buf = torch.from_numpy(p["host"]).to("cuda")
    N, at = p["N"], p["desc_at"]
    args = (buf[:at], buf[at:].view(N, png.FILE_DTYPE.itemsize), N, p["H"], p["W"], p["color_type"], p["bit_depth"], mode == "L")
    ms = []
    for i in range(WARM + REGIONS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        ops.png_decode(*args)
        b.record()
        torch.cuda.synchronize()
        if i >= WARM:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms)


sets = {"RGB": files_of(frames(64)), "L": files_of(maps(64))}
if "--trace" in sys.argv:
    for mode, files in sets.items():
        for n in (1, 64):
            for _ in range(3):
                png.decode(files[:n], mode=mode)
    torch.cuda.synchronize()
    raise SystemExit(0)

res = {"frame": [H, W], "regions": REGIONS, "launches": "2 kernels (inflate, unfilter + convert + Adler-32), a wave per file in both"}
for mode, all_files in sets.items():
    dev = {}
    for n in (1, 16, 64):
        files = all_files[:n]

        def pillow_path():
            return np.stack([np.asarray(Image.open(io.BytesIO(f)).convert(mode)) for f in files])

        dev[n] = device_only(files, mode)
        entry = {"file_bytes_mean": float(np.mean([len(f) for f in files])), "device_ms": dev[n],
                 "decode_end_to_end": wall(lambda: png.decode(files, mode=mode)), "pack_ms": host_only(lambda: png.pack(files)),
                 "pillow_one_thread_ms": host_only(pillow_path)}
        entry["equal_pillow"] = bool(np.array_equal(png.decode(files, mode=mode).cpu().numpy(), pillow_path()))
        res[f"{mode}_N{n}"] = entry
    res[f"{mode}_t64_over_t1"] = dev[64] / dev[1]
print(json.dumps(res))
