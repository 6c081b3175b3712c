"""NumPy restatement of the audio front end (include/diffsal.h, "audio front end"): the excerpt table, the centred excerpt, the
float64 log-mel spectrogram (numpy's rfft, a dense product with the mel matrix), the examples, the nine-example index map and the
resize (the reference's own operation: ``F.interpolate`` on the CPU in float32).  One clip at a time.  ``load_cases`` reads the
fixtures of tools/gen_audio_input_golden.py; ``signal`` rebuilds their int16 inputs from seeds (the fixture keeps a CRC of each).
Test-side only: the package never imports it."""
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio_input.npz")
RATE, WIN, HOP, NFFT, BANDS = 16000, 400, 160, 512, 64
EX_FRAMES, EX_HOP, NINE = 64, 11, 9
FULL = 35280                                            # int(22050 / 10 * 16)
SIGNALS = ("noise", "tone", "chirp", "lsb", "silence")
# name: (signal, window, v): the excerpt is signal[:v], centred in `window` zeros
CASES = {"full_noise": ("noise", FULL, FULL), "full_tone": ("tone", FULL, FULL), "full_chirp": ("chirp", FULL, FULL),
         "full_lsb": ("lsb", FULL, FULL), "full_silence": ("silence", FULL, FULL),
         "w10480": ("noise", 10480, 10001), "w12345": ("tone", 12345, 12000), "w15760": ("chirp", 15760, 15760)}
# the batch video: 2.475 s of noise at 29.97 frames per second; clips as (first frame, last frame) of the excerpt table
VIDEO_FPS, VIDEO_FRAMES, VIDEO_SAMPLES = 29.97, 75, 39600
VIDEO_CLIPS = ((1, 16), (9, 24), (4, 19), (60, 75))


def signal(name, n=FULL):
    """The int16 test signals: 0.2-sigma noise, a full-scale 1 kHz tone (the precision worst case: quiet bands next to a loud
    one), a 50 Hz - 7.9 kHz chirp, +-2-LSB noise, silence, and the batch video's noise."""
    t = np.arange(n, dtype=np.float64) / RATE
    if name == "noise":
        x = np.random.default_rng(101).standard_normal(n) * 0.2 * 32768.0
    elif name == "tone":
        x = 32767.0 * np.sin(2 * np.pi * 1000.0 * t)
    elif name == "chirp":
        x = 0.7 * 32768.0 * np.sin(2 * np.pi * (50.0 * t + 0.5 * (7850.0 / (n / RATE)) * t * t))
    elif name == "lsb":
        return np.random.default_rng(103).integers(-2, 3, size=n).astype(np.int16)
    elif name == "silence":
        return np.zeros(n, dtype=np.int16)
    elif name == "video":
        x = np.random.default_rng(107).standard_normal(n) * 0.1 * 32768.0
        x[n // 2:] *= np.linspace(1.0, 0.02, n - n // 2)
    else:
        raise KeyError(name)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def load_cases():
    """{"window" [400], "mel" [257, 64], "crc/<signal>", "<case>/logmel" [F, 64] f32, "<case>/examples_shape",
    "video/<a>_<b>/logmel" [152, 64] f32}"""
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def excerpt_table(n_frames, fps, rate, n_samples):
    """First and last sample of video frames 1 .. n_frames (entry 0 is zero), all frames at once: a frame is centred on
    (f - 1) * (1.0 / fps) * rate and owns rate / fps / 2 samples on either side; the start is clamped at 0, the end at
    n_samples, both truncated.  numpy's int64-times-float64 products are the same IEEE operations as Python's, in this order."""
    centre = np.arange(n_frames) * (1.0 / float(fps)) * rate
    half = rate / float(fps) / 2
    starts = np.concatenate([[0], np.maximum(0, centre - half).astype(np.int64)])
    ends = np.concatenate([[0], np.minimum(n_samples, np.abs(centre + half)).astype(np.int64)])
    return starts, ends


def to_float(wav):
    wav = np.asarray(wav)
    return wav / 32768.0 if wav.dtype == np.int16 else wav.astype(np.float64)


def padded_excerpt(wav, start, end, window):
    """R/datasets/saliency_db.py:463-484: wav[start : end + 1] (numpy clamps the slice) centred in ``window`` zeros."""
    tmp = to_float(wav)[start:end + 1]
    v = tmp.shape[0]
    if v > window:
        raise ValueError("excerpt longer than the window")
    out = np.zeros((window,))
    lo = window // 2 - v // 2
    out[lo:lo + v] = tmp
    return out


def hann_window():
    return 0.5 - 0.5 * np.cos(np.arange(WIN) * (2 * np.pi / WIN))


def mel_matrix():
    def mel(f):
        return 1127.0 * np.log(1.0 + (f / 700.0))
    bins = mel(np.linspace(0.0, RATE / 2., NFFT // 2 + 1))[:, None]
    edges = np.linspace(mel(125.0), mel(7500.0), BANDS + 2)
    lower, center, upper = edges[None, :-2], edges[None, 1:-1], edges[None, 2:]
    m = np.maximum(0.0, np.minimum((bins - lower) / (center - lower), (upper - bins) / (upper - center)))
    m[0, :] = 0.0
    return m


def frame(data, length, hop):
    n = 1 + (data.shape[0] - length) // hop
    if n < 1:
        raise ValueError("too short for one frame")
    return np.stack([data[i * hop:i * hop + length] for i in range(n)])


def log_mel(x):
    """float64 log-mel [F, 64] of a float64 excerpt."""
    spec = np.abs(np.fft.rfft(frame(x, WIN, HOP) * hann_window(), NFFT))
    return np.log(np.dot(spec, mel_matrix()) + 0.01)


def nine_map(E):
    j = np.arange(NINE)
    if E >= NINE:
        return j
    r = NINE // E
    return np.where(j < E * r, j // r, (j - E * r) // r)


def examples(lm):
    """[9, 64, 64] float32: the examples of a log-mel array, repeated to nine as get_mel_feature does."""
    ex = frame(lm, EX_FRAMES, EX_HOP).astype(np.float32)
    return ex[nine_map(ex.shape[0])]


def resize(ex9, h, w):
    """[9, 64, 64] -> [9, h, w] as transforms.Resize does on a tensor (antialias off)."""
    import torch
    import torch.nn.functional as F
    return F.interpolate(torch.from_numpy(np.ascontiguousarray(ex9))[:, None], size=(h, w), mode="bilinear", align_corners=False)[:, 0].numpy()


def clip_audio(wav, start, end, window, h, w, exists=True):
    """[1, 9, h, w] float32 of one clip."""
    if not exists:
        return np.zeros((1, NINE, h, w), dtype=np.float32)
    return resize(examples(log_mel(padded_excerpt(wav, start, end, window))), h, w)[None]
