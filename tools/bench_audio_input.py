#!/usr/bin/env python3
"""Times the audio front end (diff_sal_amd.audio_input.clip_audio) with HIP events at B = 4 and B = 64 clips of one 16 kHz int16
video: window 35280 samples, output [B, 1, 9, 112, 192].  Each device time is the median of REGIONS regions of CALLS calls on a
warmed device; it is taken with the per-clip table already on the device (``clip_audio`` with GPU ``starts`` / ``ends``: no host
copy, no synchronisation) and, separately, with host lists (the checked path, which uploads them).  The two launches are also
timed alone.  The comparison is what a user does without this module: the NumPy restatement of the reference's pipeline
(tests/_audio_input_ref.py, numpy's rfft in float64 and torch's float32 resize), one clip after the other, on at most 16 threads,
plus the host-to-device copy of the stacked result.  The host side is timed with the wall clock over HOST_REPS passes.  Beside the
log-mel time stands its arithmetic: 2 x 2 x 235 x 400 fp64 operations per frame over the MI355X's 78.6 TFLOP/s vector fp64 peak.
Prints one JSON line.
usage: python tools/bench_audio_input.py"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_sal_amd import audio_input as ai  # noqa: E402
from diff_sal_amd import ops  # noqa: E402
from tests import _audio_input_ref as ref  # noqa: E402

WARM, REGIONS, CALLS, HOST_REPS = 5, 9, 20, 3
FP64_PEAK = 78.6e12
SIZE, WINDOW, FPS, SECONDS = (112, 192), 35280, 25, 60

if not torch.cuda.is_available():
    raise SystemExit("bench_audio_input needs the GPU: a time taken elsewhere says nothing")
torch.set_num_threads(min(16, torch.get_num_threads()))
video = ref.signal("video", SECONDS * ref.RATE)
n_frames = SECONDS * FPS
starts, ends = ai.excerpt_table(n_frames, FPS, ref.RATE, video.shape[0])
wav = torch.from_numpy(video).cuda()


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


def host_pipeline(s, e):
    out = np.stack([ref.clip_audio(video, a, b, WINDOW, *SIZE) for a, b in zip(s, e)])
    t = torch.from_numpy(out).cuda()
    torch.cuda.synchronize()
    return t


res = {"size": list(SIZE), "window": WINDOW, "regions": REGIONS, "calls_per_region": CALLS, "host_threads": torch.get_num_threads()}
for B in (4, 64):
    first = 1 + (np.arange(B) * 17) % (n_frames - 16)
    s, e = [int(starts[a]) for a in first], [int(ends[a + 15]) for a in first]
    sd, ed = torch.tensor(s, dtype=torch.int32, device="cuda"), torch.tensor(e, dtype=torch.int32, device="cuda")
    Fn = ai.frames_needed(WINDOW)
    tables = ai._tables(wav.device)
    lm = ops.logmel(wav[None], 0, None, None, sd, ed, B, WINDOW, Fn, tables)
    flops = 2.0 * 2 * 235 * 400 * B * Fn
    entry = {"clip_audio_device_table": timed(lambda: ai.clip_audio(wav, sd, ed, size=SIZE)),
             "clip_audio_host_table": timed(lambda: ai.clip_audio(wav, s, e, size=SIZE)),
             "logmel": timed(lambda: ops.logmel(wav[None], 0, None, None, sd, ed, B, WINDOW, Fn, tables)),
             "examples_resize": timed(lambda: ops.audio_examples(lm, None, ai.num_examples(WINDOW), *SIZE))}
    entry["logmel"]["fp64_flop"] = flops
    entry["logmel"]["fp64_floor_ms"] = flops / FP64_PEAK * 1e3
    entry["logmel"]["share_of_fp64_peak"] = entry["logmel"]["fp64_floor_ms"] / entry["logmel"]["ms"]
    host_pipeline(s[:1], e[:1])
    hs = []
    for _ in range(HOST_REPS):
        t0 = time.perf_counter()
        host_pipeline(s, e)
        hs.append((time.perf_counter() - t0) * 1e3)
    entry["host_numpy_plus_copy_ms"] = statistics.median(hs)
    entry["host_over_device"] = entry["host_numpy_plus_copy_ms"] / entry["clip_audio_device_table"]["ms"]
    res[f"B{B}"] = entry
print(json.dumps(res))
