#!/usr/bin/env python3
"""Times the JPEG decode (diff_sal_amd.jpeg.decode) at the frame size of the audio-visual sets: N = 64 and N = 300 files of
640 x 360, 4:2:0, quality 90, written by Pillow from video-like synthetic frames (smooth shapes, texture, mild noise), once without
restart markers and once with one restart interval per MCU row.  The device side is ``jpeg.decode`` end to end -- the host's marker
walk, the one copy and the launches -- as wall clock around a synchronise; ``pack_ms`` is the host part alone.  Beside it stands
the path it replaces, on the same machine: Pillow decoding the same files in a pool of 16 threads (its decoder releases the GIL) plus
the upload of the decoded pixels.  Warm-up, then the median of REGIONS timed regions per entry.  Prints one JSON line.

``--trace`` runs three decodes of each N = 300 set and nothing else: run it under ``rocprofv3 --kernel-trace --stats`` for the
per-launch split (the profiler slows the host: take the end-to-end numbers from a run without it).
usage: python tools/bench_jpeg_decode.py [--trace]"""
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_sal_amd import jpeg  # noqa: E402

H, W, QUALITY, WARM, REGIONS, HOST_THREADS = 360, 640, 90, 3, 9, 16

if not torch.cuda.is_available():
    raise SystemExit("bench_jpeg_decode needs the GPU: a time taken elsewhere says nothing")
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


def files_of(imgs, **kw):
    out = []
    for img in imgs:
        f = io.BytesIO()
        Image.fromarray(img).save(f, "JPEG", quality=QUALITY, subsampling=2, **kw)
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


imgs = frames(300)
sets = {"no_restart": files_of(imgs), "restart_per_mcu_row": files_of(imgs, restart_marker_rows=1)}
if "--trace" in sys.argv:
    for files in sets.values():
        for _ in range(3):
            jpeg.decode(files)
    torch.cuda.synchronize()
    raise SystemExit(0)

res = {"frame": [H, W], "quality": QUALITY, "sampling": "4:2:0", "regions": REGIONS, "host_threads": HOST_THREADS,
       "launches": "1 clear + 3 kernels (entropy, transform, colour)"}
with ThreadPoolExecutor(HOST_THREADS) as pool:
    def pillow_path(files):
        px = np.stack(list(pool.map(lambda f: np.asarray(Image.open(io.BytesIO(f)).convert("RGB")), files)))
        return torch.from_numpy(px).to("cuda")

    for name, all_files in sets.items():
        for n in (64, 300):
            files = all_files[:n]
            entry = {"file_bytes_mean": float(np.mean([len(f) for f in files])), "segments_per_file": int(jpeg.parse_file(files[0])["desc"]["nseg"]),
                     "device": wall(lambda: jpeg.decode(files)), "pack_ms": host_only(lambda: jpeg.pack(files)),
                     "pillow_16_threads_plus_upload": wall(lambda: pillow_path(files))}
            entry["equal_pillow"] = bool(torch.equal(jpeg.decode(files), pillow_path(files)))
            res[f"{name}_N{n}"] = entry
print(json.dumps(res))
