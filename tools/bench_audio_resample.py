#!/usr/bin/env python3
"""Times the audio front end's resampling stage with HIP events: B = 64 (and 4) clips of one 22050 Hz int16 video, window 35280
samples, output [B, 1, 9, 112, 192].  Each time is the median of REGIONS regions of CALLS calls on a warmed device, with the
per-clip table already on the device (no host copy, no synchronisation inside a region).  Timed: ``resample_excerpts`` alone for
the 24560 samples the 152 frames read, the three-launch ``clip_audio(..., sample_rate=22050, resample="kaiser_best")``, its
``logmel`` launch on the resampled wave alone, and, in the same run, the two-launch ``clip_audio`` of the same clips taken as
16 kHz input.  Beside the resample time stand its taps (counted on the host from the loop bounds of include/diffsal.h; a tap is
one 16-byte table load, one LDS read and four fp64 operations), what they are per second, and the launch's share of the chain.
Prints one JSON line.
usage: python tools/bench_audio_resample.py"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_sal_amd import audio_input as ai  # noqa: E402
from diff_sal_amd import ops  # noqa: E402
from tests import _audio_input_ref as ref  # noqa: E402

WARM, REGIONS, CALLS = 5, 9, 10
SIZE, WINDOW, FPS, SECONDS, RATE = (112, 192), 35280, 25, 60, 22050

if not torch.cuda.is_available():
    raise SystemExit("bench_audio_resample needs the GPU: a time taken elsewhere says nothing")
video = ref.signal("video", SECONDS * RATE)
n_frames = SECONDS * FPS
starts, ends = ai.excerpt_table(n_frames, FPS, RATE, video.shape[0])
starts16, ends16 = ai.excerpt_table(n_frames, FPS, ref.RATE, SECONDS * ref.RATE)
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


def taps(n, window, sr):
    """taps of outputs 0 .. n - 1 of one clip: the loop bounds of include/diffsal.h"""
    half, num_table = ai.resample_filter("kaiser_best")
    ratio = 16000.0 / sr
    scale, step = min(1.0, ratio), int(min(1.0, ratio) * num_table)
    time = np.arange(n) * (1.0 / ratio)
    m = time.astype(np.int64)
    frac = scale * (time - m)
    left = np.minimum(m + 1, (half.size - (frac * num_table).astype(np.int64)) // step)
    right = np.minimum(window - m - 1, (half.size - ((scale - frac) * num_table).astype(np.int64)) // step)
    return int(left.sum() + right.sum())


n_out = ai.resampled_length(WINDOW, RATE)
Fn = ai.frames_needed(n_out)
need = ai.STFT_WINDOW + ai.STFT_HOP * (Fn - 1)
res = {"size": list(SIZE), "window": WINDOW, "sample_rate": RATE, "resampled": n_out, "frames": Fn, "samples_resampled": need,
       "regions": REGIONS, "calls_per_region": CALLS}
ai.warm("cuda", sample_rate=RATE, resample="kaiser_best", clips=64)
table, num_table = ai._resample_tables(wav.device, RATE, 16000, "kaiser_best")
for B in (4, 64):
    first = 1 + (np.arange(B) * 17) % (n_frames - 16)
    s, e = [int(starts[a]) for a in first], [int(ends[a + 15]) for a in first]
    sd, ed = torch.tensor(s, dtype=torch.int32, device="cuda"), torch.tensor(e, dtype=torch.int32, device="cuda")
    s16 = torch.tensor([int(starts16[a]) for a in first], dtype=torch.int32, device="cuda")
    e16 = torch.tensor([int(ends16[a + 15]) for a in first], dtype=torch.int32, device="cuda")
    wav16 = wav[:SECONDS * ref.RATE]
    y = ops.resample_excerpts(wav[None], 0, None, None, sd, ed, B, WINDOW, RATE, 16000, table, num_table, need)
    zeros, last, iota = ai._unit_clips(wav.device, B)
    entry = {"resample_excerpts": timed(lambda: ops.resample_excerpts(wav[None], 0, None, None, sd, ed, B, WINDOW, RATE, 16000, table,
                                                                      num_table, need)),
             "logmel_on_resampled": timed(lambda: ops.logmel(y, 2, None, iota, zeros, last, B, need, Fn, ai._tables(wav.device))),
             "clip_audio_22050_three_launches": timed(lambda: ai.clip_audio(wav, sd, ed, size=SIZE, sample_rate=RATE, resample="kaiser_best")),
             "clip_audio_16000_two_launches": timed(lambda: ai.clip_audio(wav16, s16, e16, size=SIZE))}
    r = entry["resample_excerpts"]
    r["taps"] = taps(need, WINDOW, RATE) * B
    r["table_loads_per_s"] = r["taps"] / (r["ms"] * 1e-3)
    r["table_bytes_per_s"] = 16.0 * r["table_loads_per_s"]
    r["fp64_ops_per_s"] = 4.0 * r["table_loads_per_s"]
    r["share_of_chain"] = r["ms"] / entry["clip_audio_22050_three_launches"]["ms"]
    res[f"B{B}"] = entry
print(json.dumps(res))
