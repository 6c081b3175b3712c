#!/usr/bin/env python3
"""Times the video front end (diff_sal_amd.video_input) with HIP events on the protocol chain, 64 decoded frames of 360 x 640 and
of 1080 x 1920: ``img.resize((320, 240))`` bicubic, then 224 x 384 bilinear, then clips of 16 frames through the look-up table.

Per source size: the chain and each of its two resizes in the fused form, in the two-pass form and in the form ``fused=None``
picks (alternating, in the same run), the gather of 4 clips of 16 frames, and the gather of sixteen overlapping clips (starts
0 .. 15) from the one transformed video.  Each
device time is the median of REGIONS regions of CALLS calls on a warmed device.  Beside each time stand frames / s, the bytes the
step must move once (its input and its output; the two-pass form's workspace is not counted: it is the form's own cost), the
effective GB / s and the share of the once-through floor at the 6.29 TB / s a copy kernel reaches on an MI355X (bound: memory;
the arithmetic is a few dozen integer multiply-adds per byte read and far from its own bound).  Where Pillow imports, its time for
the same chain on the same frames, one frame after the other on one thread (Pillow's resize is single-threaded), by the wall clock.
Prints one JSON line.
usage: python tools/bench_video_input.py"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_sal_amd import video_input as vi  # noqa: E402
from tests import _video_input_ref as ref  # noqa: E402

WARM, REGIONS, CALLS = 3, 9, 10
HBM_COPY = 6.29e12      # bytes / s of a float4 copy on an MI355X
FRAMES, PRE, SIZE, T = 64, (240, 320), (224, 384), 16

if not torch.cuda.is_available():
    raise SystemExit("bench_video_input needs the GPU: a time taken elsewhere says nothing")


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


def rated(entry, nbytes, frames):
    entry["bytes"] = nbytes
    entry["frames_per_s"] = frames / (entry["ms"] * 1e-3)
    entry["GB_per_s"] = nbytes / (entry["ms"] * 1e-3) / 1e9
    entry["floor_ms"] = nbytes / HBM_COPY * 1e3
    entry["share_of_floor"] = entry["floor_ms"] / entry["ms"]
    return entry


res = {"frames": FRAMES, "pre_size": list(PRE), "size": list(SIZE), "regions": REGIONS, "calls_per_region": CALLS,
       "hbm_copy_bytes_per_s": HBM_COPY}
try:
    import PIL
    from PIL import Image
    res["pillow"] = PIL.__version__
except ImportError:
    Image = None

for H0, W0 in ((360, 640), (1080, 1920)):
    x = ref.noise((FRAMES, H0, W0, 3), 41)
    xd = torch.from_numpy(x).cuda()
    src, mid_b, out_b = x.size, FRAMES * PRE[0] * PRE[1] * 3, FRAMES * SIZE[0] * SIZE[1] * 3
    mid = vi.resize_u8(xd, PRE, "bicubic")
    out = vi.resize_u8(mid, SIZE, "bilinear")
    entry = {"band_rows": [vi.band_rows((H0, W0), PRE, 3, "bicubic"), vi.band_rows(PRE, SIZE, 3, "bilinear")]}
    for name, fused in (("fused", True), ("two_pass", False), ("auto", None)):      # the forms alternate within the run
        assert torch.equal(vi.transform_frames(xd, SIZE, PRE, fused=fused), out)
        entry[name] = {
            "chain": rated(timed(lambda: vi.transform_frames(xd, SIZE, PRE, fused=fused)), src + 2 * mid_b + out_b, FRAMES),
            "pre_resize": rated(timed(lambda: vi.resize_u8(xd, PRE, "bicubic", fused=fused)), src + mid_b, FRAMES),
            "resize": rated(timed(lambda: vi.resize_u8(mid, SIZE, "bilinear", fused=fused)), mid_b + out_b, FRAMES),
        }
    entry["fused_over_two_pass"] = entry["fused"]["chain"]["ms"] / entry["two_pass"]["chain"]["ms"]
    per_clip_in, per_clip_out = T * SIZE[0] * SIZE[1] * 3, T * SIZE[0] * SIZE[1] * 3 * 4
    for name, starts in (("gather_4_clips", [0, 16, 32, 48]), ("gather_16_overlapping_clips", list(range(16)))):
        idx = torch.tensor([[s + t for t in range(T)] for s in starts], dtype=torch.int32, device="cuda")
        B = len(starts)
        entry[name] = rated(timed(lambda: vi.gather_clips(out, idx)), B * (per_clip_in + per_clip_out), B * T)
    idx16 = torch.tensor([[s + t for t in range(T)] for s in range(16)], dtype=torch.int32, device="cuda")
    # the sixteen overlapping clips end to end: their 31 frames transformed once, then the gather
    entry["clips_16_overlapping_end_to_end"] = rated(timed(lambda: vi.clip_rgb(xd[:31], idx16, SIZE, PRE)),
                                                     31 * (src + 2 * mid_b + out_b) // FRAMES + 16 * (per_clip_in + per_clip_out), 16 * T)
    if Image is not None:
        n_host = 8
        imgs = [Image.fromarray(f, "RGB") for f in x[:n_host]]
        t0 = time.perf_counter()
        host = [np.asarray(im.resize((PRE[1], PRE[0])).resize((SIZE[1], SIZE[0]), Image.BILINEAR)) for im in imgs]
        dt = time.perf_counter() - t0
        assert np.array_equal(np.stack(host), out[:n_host].cpu().numpy())
        entry["pillow_one_thread"] = {"frames": n_host, "ms_per_frame": dt / n_host * 1e3, "frames_per_s": n_host / dt, "threads": 1}
    res[f"{H0}x{W0}"] = entry
    del xd, mid, out
print(json.dumps(res))
