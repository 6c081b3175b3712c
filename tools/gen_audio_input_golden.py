"""Writes tests/golden/audio_input.npz: what the reference's own ``mel_features.py`` gives for the seeded int16 signals of
tests/_audio_input_ref.py -- the float64 log-mel spectrogram of each centred excerpt cast to float32 (the cast
``waveform_to_examples`` applies), the shape ``mel_features.frame(log_mel, 64, 11)`` returns, the mel matrix and the Hann window --
plus a CRC of every rebuilt signal, so that a platform that rebuilds another signal is noticed.

    python tools/gen_audio_input_golden.py --reference <checkout of the reference>

``mel_features.py`` and ``vggish_params.py`` are loaded by file path, at generation time only (``vggish_input.py`` and
``saliency_db.py`` need resampy, soundfile and torchaudio; their few lines of logic are restated in tests/_audio_input_ref.py).
Needs numpy; no GPU.  The batch video's clips are recorded for the 152 frames the nine examples read.  No test runs this tool."""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _audio_input_ref as ref  # noqa: E402


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    a = ap.parse_args()
    d = os.path.join(a.reference, "datasets", "torchvggish")
    mf, vp = load(os.path.join(d, "mel_features.py"), "mel_features"), load(os.path.join(d, "vggish_params.py"), "vggish_params")

    def reference_log_mel(x):
        return mf.log_mel_spectrogram(x, audio_sample_rate=vp.SAMPLE_RATE, log_offset=vp.LOG_OFFSET,
                                      window_length_secs=vp.STFT_WINDOW_LENGTH_SECONDS, hop_length_secs=vp.STFT_HOP_LENGTH_SECONDS,
                                      num_mel_bins=vp.NUM_MEL_BINS, lower_edge_hertz=vp.MEL_MIN_HZ, upper_edge_hertz=vp.MEL_MAX_HZ)

    features_rate = 1.0 / vp.STFT_HOP_LENGTH_SECONDS
    ex_len, ex_hop = int(round(vp.EXAMPLE_WINDOW_SECONDS * features_rate)), int(round(vp.EXAMPLE_HOP_SECONDS * features_rate))
    assert (ex_len, ex_hop) == (ref.EX_FRAMES, ref.EX_HOP)
    blob = {"window": mf.periodic_hann(ref.WIN),
            "mel": mf.spectrogram_to_mel_matrix(num_mel_bins=vp.NUM_MEL_BINS, num_spectrogram_bins=ref.NFFT // 2 + 1,
                                                audio_sample_rate=vp.SAMPLE_RATE, lower_edge_hertz=vp.MEL_MIN_HZ,
                                                upper_edge_hertz=vp.MEL_MAX_HZ)}
    for s in ref.SIGNALS:
        blob[f"crc/{s}"] = np.array(ref.crc(ref.signal(s)), dtype=np.int64)
    video = ref.signal("video", ref.VIDEO_SAMPLES)
    blob["crc/video"] = np.array(ref.crc(video), dtype=np.int64)
    worst = 0.0
    for name, (sig, window, v) in ref.CASES.items():
        x = ref.padded_excerpt(ref.signal(sig)[:v], 0, v - 1, window)
        lm = reference_log_mel(x)
        blob[f"{name}/logmel"] = lm.astype(np.float32)
        blob[f"{name}/examples_shape"] = np.array(mf.frame(lm, ex_len, ex_hop).shape, dtype=np.int64)
        worst = max(worst, float(np.abs(ref.log_mel(x) - lm).max()))
        print(name, lm.shape, blob[f"{name}/examples_shape"], "range", lm.min(), lm.max())
    starts, ends = ref.excerpt_table(ref.VIDEO_FRAMES, ref.VIDEO_FPS, ref.RATE, video.shape[0])
    parities = set()
    for fa, fb in ref.VIDEO_CLIPS:
        x = ref.padded_excerpt(video, starts[fa], ends[fb], ref.FULL)
        v = len(video[starts[fa]:ends[fb] + 1])
        parities.add(v % 2)
        lm = reference_log_mel(x)
        blob[f"video/{fa}_{fb}/logmel"] = lm[:152].astype(np.float32)
        worst = max(worst, float(np.abs(ref.log_mel(x) - lm).max()))
        print("video clip", fa, fb, "samples", starts[fa], ends[fb], "v", v)
    assert parities == {0, 1}, "the batch needs an odd and an even excerpt"
    assert ends[ref.VIDEO_FRAMES] == video.shape[0], "the last clip must be clamped at the end of the audio"
    print("restatement against the reference, float64: worst |d| =", worst)
    out = os.path.join(ROOT, "tests", "golden", "audio_input.npz")
    np.savez_compressed(out, **blob)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
