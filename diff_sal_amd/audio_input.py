"""From PCM samples in device memory to the ``audio [B, 1, 9, h, w]`` tensor ``VideoSaliencyModel.forward_vggish`` reads
(csrc/audio_input.hip, arithmetic in include/diffsal.h "audio front end").  The reference builds that tensor per clip on the host
in numpy:

* R/datasets/saliency_db.py:208-222 tabulates, per video, the first and last sample of every frame: ``excerpt_table``;
* R/datasets/saliency_db.py:449-497 (``get_mel_feature``) cuts ``wav[starts[a] : ends[b] + 1]``, centres it in a zero buffer of
  ``window`` samples and calls R/datasets/torchvggish/vggish_input.py:30-82 (``waveform_to_examples``), which takes the log-mel
  spectrogram of R/datasets/torchvggish/mel_features.py:71-223 (periodic Hann window of 400 samples, hop 160, magnitude of the
  512-point rfft, 257 x 64 HTK mel matrix, ``log(x + 0.01)``, all float64) and frames it into examples of 64 frames, hop 11,
  cast to float32: ``log_mel`` and ``examples``;
* the examples are repeated to nine (``repeat_interleave`` then ``cat`` with the head of the *repeated* list), and
  R/datasets/saliency_db.py:303-305,351-354 resizes each to half the frame size with ``transforms.Resize`` on a tensor, the
  plain ``F.interpolate(mode="bilinear", align_corners=False)`` in float32, and stacks them: ``clip_audio``.

``clip_audio`` is two launches for all clips of a batch: ``logmel`` (float64, only the frames the nine examples need) and
``examples_resize``.  The centring and zero padding are index arithmetic on the video's waveform; no padded excerpt exists in
memory.

**Input at another rate** (the reference's audio-visual sets: ``max_audio_Fs = 22050``).  The reference reads a file at its native
rate, tabulates ``starts`` / ``ends`` at that rate and hands the padded buffer of ``window`` native-rate samples to
``waveform_to_examples(audioexcer, sample_rate=Fs)``, which calls ``resampy.resample(data, Fs, 16000)`` on it
(R/datasets/torchvggish/vggish_input.py:52-53): per clip, in float64, after the padding.  ``resample="kaiser_best"`` (resampy's
default filter; or ``"kaiser_fast"``, or a ``(half_window, num_table)`` pair) does that on the device: ``resample_excerpts`` is one
more launch in front of ``logmel``, resampy 0.4.2's interpolation loop with every float64 operation in the library's order, so its
output equals a NumPy restatement of the loop bit for bit (include/diffsal.h states it; tests/_audio_resample_ref.py restates it).
Only the samples the frames need are resampled; ``num_frames`` / ``num_examples`` / ``frames_needed`` are taken of
``resampled_length(window, sample_rate)``: 25600 samples, 158 frames and exactly nine examples for the 35280-sample window at
22050 Hz.  Resampling the whole file once when it is loaded is *not* the same computation: the excerpt table lives at the native
rate, the filter sees the zero padding at the excerpt's edges, and the length is ``int(window * 16000 / Fs)``.  Without
``resample=`` a ``sample_rate`` other than 16000 raises, as it always did.  ``audio_type`` "spec" and "ori" of the reference are
not built.

Each of ``starts`` / ``ends`` / ``wav_len`` / ``video`` / ``exists`` given on the host (a sequence, a numpy array, a CPU tensor)
is range-checked here and uploaded; a clip longer than the window raises, as the reference's broadcast does, whenever ``starts``,
``ends``, ``wav_len`` and ``video`` are all on the host (or absent).  An argument given as a GPU tensor is used as it is, with no
host copy and no synchronisation; with all of them on the GPU the call can be captured in a graph.  What could not be checked the
kernel makes safe: it clamps the way numpy slicing does and centre-crops a clip longer than the window.  The first call on a
device uploads the kernel's tables from host memory, which a capture does not allow: call once (or ``warm(device)``; with
``sample_rate=`` and ``resample=`` for the resampling tables, which are kept per device, rates and filter) before capturing.  The resize is the plain bilinear form, also for ``h`` or ``w`` below 64: a torchvision whose tensor ``Resize``
defaults to ``antialias=True`` gives other values when it shrinks an axis (for an upscale the two forms are the same filter).
GPU only: a CPU ``wav`` raises.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, ops

Tensor = torch.Tensor

# R/datasets/torchvggish/vggish_params.py
SAMPLE_RATE = 16000
STFT_WINDOW_LENGTH_SECONDS = 0.025
STFT_HOP_LENGTH_SECONDS = 0.010
NUM_MEL_BINS = 64
MEL_MIN_HZ = 125
MEL_MAX_HZ = 7500
LOG_OFFSET = 0.01
EXAMPLE_WINDOW_SECONDS = 0.64
EXAMPLE_HOP_SECONDS = 0.11

STFT_WINDOW = int(round(SAMPLE_RATE * STFT_WINDOW_LENGTH_SECONDS))                       # 400 samples
STFT_HOP = int(round(SAMPLE_RATE * STFT_HOP_LENGTH_SECONDS))                             # 160 samples
FFT_LENGTH = 2 ** int(np.ceil(np.log(STFT_WINDOW) / np.log(2.0)))                        # 512
NUM_SPECTROGRAM_BINS = FFT_LENGTH // 2 + 1                                               # 257
EXAMPLE_FRAMES = int(round(EXAMPLE_WINDOW_SECONDS * (1.0 / STFT_HOP_LENGTH_SECONDS)))    # 64 log-mel frames
EXAMPLE_HOP = int(round(EXAMPLE_HOP_SECONDS * (1.0 / STFT_HOP_LENGTH_SECONDS)))          # 11 log-mel frames
NUM_EXAMPLES = 9                                                                         # audio_len of get_mel_feature
DEFAULT_WINDOW = int(22050 / 10 * 16)                                                    # max_audio_win for 16 frames: 35280

# the kernel's tables (include/diffsal.h): bins 5..239 carry mel weight, a band has at most 17 non-zero weights
BIN_LO, BIN_COUNT, BIN_PITCH, BAND_TAPS = 5, 235, 256, 17
TABLE_DOUBLES = 2 * STFT_WINDOW * BIN_PITCH + NUM_MEL_BINS * BAND_TAPS + NUM_MEL_BINS


def hann_window(length: int = STFT_WINDOW) -> np.ndarray:
    """The periodic Hann window mel_features.py applies (one cosine period over ``length`` samples, not ``length - 1``), float64."""
    phase = np.arange(length) * (2 * np.pi / length)
    return 0.5 - 0.5 * np.cos(phase)


def mel_matrix() -> np.ndarray:
    """The 257 x 64 HTK mel matrix mel_features.py builds for 16 kHz, 125-7500 Hz, float64.  With mel(f) = 1127 ln(1 + f / 700),
    the 66 band edges are equally spaced in mel; band m rises linearly (in mel) from edge m to edge m + 1 and falls to edge m + 2,
    clipped at zero; the DC row is zero.  All 64 bands at once, in the element-wise operation order that reproduces the
    reference's matrix exactly (tests/test_audio_input_host.py)."""
    def mel(f):
        return 1127.0 * np.log(1.0 + (f / 700.0))
    bin_mel = mel(np.linspace(0.0, SAMPLE_RATE / 2.0, NUM_SPECTROGRAM_BINS))[:, None]      # [257, 1]
    edge = np.linspace(mel(float(MEL_MIN_HZ)), mel(float(MEL_MAX_HZ)), NUM_MEL_BINS + 2)
    left, peak, right = edge[None, :-2], edge[None, 1:-1], edge[None, 2:]                  # [1, 64] each
    rising = (bin_mel - left) / (peak - left)
    falling = (right - bin_mel) / (right - peak)
    weights = np.clip(np.minimum(rising, falling), 0.0, None)
    weights[0] = 0.0
    return weights


def num_frames(window: int) -> int:
    """Log-mel frames of a ``window``-sample excerpt: 1 + floor((window - 400) / 160)."""
    return 1 + (int(window) - STFT_WINDOW) // STFT_HOP if window >= STFT_WINDOW else 0


def num_examples(window: int) -> int:
    """Examples of a ``window``-sample excerpt: 1 + floor((frames - 64) / 11)."""
    F = num_frames(window)
    return 1 + (F - EXAMPLE_FRAMES) // EXAMPLE_HOP if F >= EXAMPLE_FRAMES else 0


def example_map(E: int) -> np.ndarray:
    """Source example of each of the nine outputs for ``E`` available ones: what ``repeat_interleave(x, 9 // E)`` followed by
    ``cat([x, x[:9 % E]])`` (the tail from the repeated list) and ``[:9]`` select."""
    if E < 1:
        raise ValueError(f"audio_input: {E} examples (the window is too short for one)")
    j = np.arange(NUM_EXAMPLES)
    if E >= NUM_EXAMPLES:
        return j
    r = NUM_EXAMPLES // E
    return np.where(j < E * r, j // r, (j - E * r) // r)


def frames_needed(window: int) -> int:
    """Log-mel frames the nine examples read: 64 + 11 (min(E, 9) - 1)."""
    E = num_examples(window)
    if E < 1:
        raise ValueError(f"audio_input: a window of {window} samples is too short for one example of {EXAMPLE_FRAMES} frames "
                         f"({STFT_WINDOW + (EXAMPLE_FRAMES - 1) * STFT_HOP} samples)")
    return EXAMPLE_FRAMES + EXAMPLE_HOP * (min(E, NUM_EXAMPLES) - 1)


def excerpt_table(n_frames: int, fps: float, sample_rate: int, n_samples: int) -> Tuple[np.ndarray, np.ndarray]:
    """``starts``, ``ends`` (int64, ``n_frames + 1`` entries, entry 0 zero) as R/datasets/saliency_db.py:208-222 tabulates them:
    video frame f = 1 .. n_frames is centred on sample ``(f - 1) * (1.0 / fps) * sample_rate`` and owns half a frame period of
    audio on either side, the start clamped at 0, the end at ``n_samples``, both truncated.  The float64 operation order is the
    reference's (the reciprocal of ``fps`` is formed first): a product that lands a last bit below an integer truncates
    differently otherwise."""
    fps = float(fps)
    half = (sample_rate / fps) / 2
    per_frame = 1.0 / fps
    starts = np.zeros(n_frames + 1, dtype=np.int64)
    ends = np.zeros(n_frames + 1, dtype=np.int64)
    for f in range(1, n_frames + 1):
        centre = (f - 1) * per_frame * sample_rate
        starts[f] = int(max(0, centre - half))
        ends[f] = int(min(n_samples, abs(centre + half)))
    return starts, ends


def device_tables() -> np.ndarray:
    """The float64 table ``diffsal_logmel`` reads (layout in include/diffsal.h): the Hann window folded into the DFT basis
    ``hann[n] (cos, sin)(2 pi n k / 512)`` for n < 400 and bins k = 5 + c, c < 235 (columns 235..255 zero), the 17 mel weights of
    each band from its first non-zero bin on, and that bin's column."""
    n = np.arange(STFT_WINDOW, dtype=np.int64)[:, None]
    k = BIN_LO + np.arange(BIN_COUNT, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((n * k) % FFT_LENGTH).astype(np.float64) / FFT_LENGTH      # the angle reduced exactly first
    basis = np.zeros((STFT_WINDOW, BIN_PITCH, 2))
    basis[:, :BIN_COUNT, 0] = hann_window()[:, None] * np.cos(ang)
    basis[:, :BIN_COUNT, 1] = hann_window()[:, None] * np.sin(ang)
    m = mel_matrix()
    nz = np.nonzero(m.any(axis=1))[0]
    if nz[0] < BIN_LO or nz[-1] >= BIN_LO + BIN_COUNT:
        raise AssertionError("mel weight outside bins 5..239")
    w = np.zeros((NUM_MEL_BINS, BAND_TAPS))
    first = np.zeros(NUM_MEL_BINS)
    for b in range(NUM_MEL_BINS):
        idx = np.nonzero(m[:, b])[0]
        if idx[-1] - idx[0] >= BAND_TAPS:
            raise AssertionError("a mel band wider than 17 bins")
        w[b, :idx[-1] - idx[0] + 1] = m[idx[0]:idx[-1] + 1, b]
        first[b] = idx[0] - BIN_LO
    t = np.concatenate([basis.reshape(-1), w.reshape(-1), first])
    assert t.size == TABLE_DOUBLES
    return t


# resampy 0.4.2's stored filters as sinc_window(num_zeros, precision, rolloff) with a Kaiser window of the given beta designs them
RESAMPLE_FILTERS = {"kaiser_best": (64, 9, 0.9475937167399596, 14.769656459379492),
                    "kaiser_fast": (16, 9, 0.85, 8.555504641634386)}


def resample_filter(name: str = "kaiser_best") -> Tuple[np.ndarray, int]:
    """``(half_window, num_table)`` of resampy's ``kaiser_best`` / ``kaiser_fast``: the right half of a Kaiser-windowed sinc,
    float64, ``num_table = 2 ** precision`` entries per zero crossing and ``num_zeros * num_table + 1`` entries in all
    (resampy.filters.sinc_window, in its operation order)."""
    try:
        num_zeros, precision, rolloff, beta = RESAMPLE_FILTERS[name]
    except (KeyError, TypeError):
        raise ValueError(f"audio_input: resample filter {name!r} is not one of {sorted(RESAMPLE_FILTERS)}") from None
    num_table = 2 ** precision
    n = num_table * num_zeros
    sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=n + 1, endpoint=True))
    taper = np.kaiser(2 * n + 1, beta)[n:]
    return taper * sinc_win, num_table


def resampled_length(n: int, sr_orig: int, sr_new: int = SAMPLE_RATE) -> int:
    """Samples ``resampy.resample`` returns for ``n`` input samples: ``int(n * sr_new / sr_orig)``."""
    return int(int(n) * int(sr_new) / int(sr_orig))


def resample_table(half_window: np.ndarray, num_table: int, sr_orig: int, sr_new: int = SAMPLE_RATE) -> np.ndarray:
    """The float64 ``[nwin, 2]`` table ``diffsal_resample_excerpts`` reads: ``(win[j], delta[j])`` with ``win`` the half window,
    multiplied by ``sr_new / sr_orig`` when that is below one, and ``delta = diff(win)`` with a final zero -- the values
    resampy.core.resample forms, so a tap is one 16-byte load."""
    win = np.array(half_window, dtype=np.float64).reshape(-1)
    ratio = float(sr_new) / sr_orig
    if ratio < 1:
        win = ratio * win
    delta = np.diff(win, append=win[-1])
    return np.ascontiguousarray(np.stack([win, delta], axis=1))


_TABLES = {}
_UNIT = {}


def _dev_key(device: torch.device):
    return (device.type, device.index if device.index is not None else torch.cuda.current_device())


def _tables(device: torch.device) -> Tensor:
    key = _dev_key(device)
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = torch.from_numpy(device_tables()).to(device)
    return t


def _resample_tables(device: torch.device, sr_orig: int, sr_new: int, filt) -> Tuple[Tensor, int]:
    """``([nwin, 2] float64 on the device, num_table)``; a named filter's table is kept per (device, rates, filter), a caller's own
    ``(half_window, num_table)`` pair is built and uploaded on every call."""
    if isinstance(filt, str):
        key = _dev_key(device) + (int(sr_orig), int(sr_new), filt)
        hit = _TABLES.get(key)
        if hit is None:
            hw, num_table = resample_filter(filt)
            hit = _TABLES[key] = (torch.from_numpy(resample_table(hw, num_table, sr_orig, sr_new)).to(device), num_table)
        return hit
    try:
        hw, num_table = filt
        hw = np.asarray(hw, dtype=np.float64)
        num_table = int(num_table)
    except (TypeError, ValueError):
        raise ValueError(f"audio_input: filter must be one of {sorted(RESAMPLE_FILTERS)} or a (half_window, num_table) pair") from None
    if hw.ndim != 1 or hw.size < 2 or num_table < 1:
        raise ValueError(f"audio_input: a filter pair is (half_window [nwin >= 2], num_table >= 1), got {hw.shape}, {num_table}")
    return torch.from_numpy(resample_table(hw, num_table, sr_orig, sr_new)).to(device), num_table


def _unit_clips(device: torch.device, B: int) -> Tuple[Tensor, Tensor, Tensor]:
    """``starts`` (zeros), ``ends`` (2^31 - 2: clamped to the row's length) and ``video`` (0, 1, ..) for ``B`` clips that are each
    one whole row of a [B, n] wave: what ``logmel`` is given after ``resample_excerpts``.  One int32 [3, N] tensor per device."""
    key = _dev_key(device)
    t = _UNIT.get(key)
    if t is None or t.shape[1] < B:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"audio_input: the index table for {B} resampled clips is not on the device yet and a capture cannot "
                               f"upload it: call warm(device, sample_rate=..., resample=..., clips={B}) first")
        N = max(1024, 1 << (int(B) - 1).bit_length())
        host = np.stack([np.zeros(N, dtype=np.int32), np.full(N, 2 ** 31 - 2, dtype=np.int32), np.arange(N, dtype=np.int32)])
        t = _UNIT[key] = torch.from_numpy(host).to(device)
    return t[0, :B], t[1, :B], t[2, :B]


def warm(device, *, sample_rate: Optional[int] = None, resample=None, sr_new: int = SAMPLE_RATE, clips: int = 1) -> None:
    """Build and upload the kernel's tables for ``device`` now (otherwise the first call does it); with ``sample_rate`` and
    ``resample`` also the resampling table of those rates and that filter and the index table for ``clips`` clips."""
    device = torch.device(device)
    _tables(device)
    if resample is not None and sample_rate is not None and int(sample_rate) != sr_new:
        _resample_tables(device, _rate(sample_rate), sr_new, resample)
        _unit_clips(device, clips)


_WAV_DTYPES = dict(zip((torch.int16, torch.float32, torch.float64), _lib.constants("WAV_", "I16 F32 F64")))


def _wav2(wav, wav_len, video):
    if not isinstance(wav, Tensor) or not wav.is_cuda:
        raise RuntimeError("diff_sal_amd audio_input runs on the GPU only (no CPU fallback); wav is on "
                           f"{getattr(wav, 'device', type(wav).__name__)}")
    if wav.dtype not in _WAV_DTYPES:
        raise ValueError(f"audio_input: wav must be int16, float32 or float64, got {wav.dtype}")
    if wav.dim() == 1:
        if video is not None:
            raise ValueError("audio_input: video indices go with a [V, Lmax] wav")
        wav = wav[None]
    elif wav.dim() == 2:
        if wav_len is None or video is None:
            raise ValueError("audio_input: a [V, Lmax] wav needs wav_len [V] and a per-clip video [B] index")
    else:
        raise ValueError(f"audio_input: wav must be 1-D or [V, Lmax], got {tuple(wav.shape)}")
    if wav.numel() == 0:
        raise ValueError("audio_input: wav is empty")
    return wav.contiguous()


def _on_device(x) -> bool:
    return isinstance(x, Tensor) and x.is_cuda


def _host(x, what, n=None):
    a = np.asarray(x.numpy() if isinstance(x, Tensor) else x).reshape(-1)
    if a.dtype == np.bool_:
        a = a.astype(np.int64)
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"audio_input: {what} must hold integers, got {a.dtype}")
    if n is not None and a.size != n:
        raise ValueError(f"audio_input: {what} has {a.size} entries, expected {n}")
    return a.astype(np.int64)


def _clip_args(wav: Tensor, starts, ends, window, wav_len, video, exists):
    """Device copies of the per-clip arguments: starts, ends, video (int32), wav_len (int64), exists (uint8).  Every argument
    given on the host is range-checked; the excerpt lengths are checked when starts, ends, wav_len and video are all known here."""
    V, L = wav.shape
    dev = wav.device
    np_of = {torch.int32: np.int32, torch.int64: np.int64, torch.uint8: np.uint8}

    def up(x, host, dtype, what, n):
        if x is None:
            return None
        if host is not None:
            return torch.from_numpy(host.astype(np_of[dtype])).to(dev)
        if x.dim() != 1 or x.numel() != n or x.is_floating_point():
            raise ValueError(f"audio_input: {what} must be {n} integers, got {x.dtype} {tuple(x.shape)}")
        return x.to(dtype).contiguous()

    B = int(starts.numel() if isinstance(starts, Tensor) else np.asarray(starts).size)
    if B < 1:
        raise ValueError("audio_input: no clips")
    s = None if _on_device(starts) else _host(starts, "starts", B)
    e = None if _on_device(ends) else _host(ends, "ends", B)
    ln = None if wav_len is None or _on_device(wav_len) else _host(wav_len, "wav_len", V)
    vi = None if video is None or _on_device(video) else _host(video, "video", B)
    ex = None if exists is None or _on_device(exists) else _host(exists, "exists", B)
    for a, what in ((s, "starts"), (e, "ends")):
        if a is not None and ((a < 0).any() or a.max() >= 2 ** 31 - 1):
            raise ValueError(f"audio_input: {what} must be sample indices in 0 .. 2^31 - 2")
    if vi is not None and ((vi < 0).any() or (vi >= V).any()):
        raise ValueError(f"audio_input: video index outside 0 .. {V - 1}")
    if ln is not None and ((ln < 0).any() or (ln > L).any()):
        raise ValueError(f"audio_input: wav_len outside 0 .. {L}")
    if s is not None and e is not None and (wav_len is None or ln is not None) and (video is None or vi is not None):
        n = (np.full(V, L, dtype=np.int64) if ln is None else ln)[np.zeros(B, dtype=np.int64) if vi is None else vi]
        v = np.maximum(np.minimum(e + 1, n) - np.minimum(s, n), 0)      # len(wav[s : e + 1]), numpy's clamping
        if (v > window).any():
            b = int(np.argmax(v > window))
            raise ValueError(f"audio_input: clip {b} spans {int(v[b])} samples, more than the window of {window} (the reference "
                             "fails here too)")
    return (B, up(starts, s, torch.int32, "starts", B), up(ends, e, torch.int32, "ends", B), up(wav_len, ln, torch.int64, "wav_len", V),
            up(video, vi, torch.int32, "video", B), up(exists, ex, torch.uint8, "exists", B))


def _rate(sample_rate) -> int:
    if sample_rate != int(sample_rate) or int(sample_rate) < 1:
        raise ValueError(f"audio_input: sample_rate {sample_rate} is not a positive integer")
    return int(sample_rate)


def _check_rate(sample_rate, resample=None) -> bool:
    """True if the call resamples: ``resample`` given and a rate other than 16000.  Another rate without ``resample`` raises."""
    if sample_rate == SAMPLE_RATE:
        return False
    if resample is None:
        raise ValueError(f"audio_input: sample_rate {sample_rate} is not {SAMPLE_RATE}; resampling is not part of this front end unless "
                         "it is asked for: resample on load, or pass resample=\"kaiser_best\" for the reference's per-clip resampy step")
    _rate(sample_rate)
    return True


def resample_excerpts(wav: Tensor, starts, ends, *, window: int, sample_rate: int, sr_new: int = SAMPLE_RATE, filter="kaiser_best",
                      wav_len=None, video=None, samples: Optional[int] = None) -> Tensor:
    """Per clip what ``resampy.resample(audioexcer, sample_rate, sr_new)`` returns for the excerpt ``wav[starts[b] : ends[b] + 1]``
    centred in ``window`` zero samples: ``[B, n]`` float64 with ``n = resampled_length(window, sample_rate, sr_new)``, or its first
    ``samples`` columns.  ``filter`` is "kaiser_best", "kaiser_fast" or a ``(half_window, num_table)`` pair such as the library's
    own stored table.  Bit-equal to the restatement of resampy 0.4.2's loop in include/diffsal.h, whatever the batch."""
    sr_orig, sr_new = _rate(sample_rate), _rate(sr_new)
    if sr_orig == sr_new:
        raise ValueError(f"audio_input: resample_excerpts from {sr_orig} Hz to {sr_new} Hz: the reference does not resample there")
    window = int(window)
    n_out = resampled_length(window, sr_orig, sr_new)
    n = n_out if samples is None else int(samples)
    if window < 1 or not 1 <= n <= n_out:
        raise ValueError(f"audio_input: {n} samples asked of a window of {window} at {sr_orig} Hz, which gives {n_out} at {sr_new} Hz")
    w2 = _wav2(wav, wav_len, video)
    B, s, e, ln, vi, _ = _clip_args(w2, starts, ends, window, wav_len, video, None)
    table, num_table = _resample_tables(w2.device, sr_orig, sr_new, filter)
    return ops.resample_excerpts(w2, _WAV_DTYPES[w2.dtype], ln, vi, s, e, B, window, sr_orig, sr_new, table, num_table, n)


def _resampled_logmel(w2: Tensor, B, s, e, ln, vi, window: int, sample_rate, resample, n_frames: int, out_f64: bool) -> Tensor:
    """``resample_excerpts`` for the ``400 + 160 (n_frames - 1)`` samples the frames read, then ``logmel`` on that [B, n] float64
    wave: one "video" per clip, the whole row as its excerpt, a window of n samples (frame f reads samples 160 f .. 160 f + 399 of
    the resampled buffer whatever follows them)."""
    n = STFT_WINDOW + STFT_HOP * (n_frames - 1)
    table, num_table = _resample_tables(w2.device, int(sample_rate), SAMPLE_RATE, resample)
    zeros, last, iota = _unit_clips(w2.device, B)
    y = ops.resample_excerpts(w2, _WAV_DTYPES[w2.dtype], ln, vi, s, e, B, window, int(sample_rate), SAMPLE_RATE, table, num_table, n)
    return ops.logmel(y, _WAV_DTYPES[torch.float64], None, iota, zeros, last, B, n, n_frames, _tables(w2.device), out_f64=out_f64)


def log_mel(wav: Tensor, starts, ends, *, window: int = DEFAULT_WINDOW, wav_len=None, video=None, dtype: torch.dtype = torch.float32,
            sample_rate: int = SAMPLE_RATE, frames: Optional[int] = None, resample=None) -> Tensor:
    """Log-mel spectrogram ``[B, F, 64]`` of each clip's excerpt ``wav[starts[b] : ends[b] + 1]`` centred in ``window`` zero
    samples, computed in float64; ``F = num_frames(window)`` or the first ``frames`` of them.  float32, or with
    ``dtype=torch.float64`` the value before the rounding (what the tests compare).  With ``resample=`` and a ``sample_rate`` other
    than 16000 the padded excerpt is resampled first and ``F = num_frames(resampled_length(window, sample_rate))``."""
    resampling = _check_rate(sample_rate, resample)
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"audio_input: dtype must be float32 or float64, got {dtype}")
    window = int(window)
    n_out = resampled_length(window, sample_rate) if resampling else window
    F = num_frames(n_out)
    if F < 1:
        raise ValueError(f"audio_input: a window of {n_out} samples is shorter than one frame of {STFT_WINDOW}")
    if frames is not None:
        if resampling and not 1 <= int(frames) <= F:
            raise ValueError(f"audio_input: {frames} frames asked of a window that holds {F}")
        F = int(frames)
    w2 = _wav2(wav, wav_len, video)
    B, s, e, ln, vi, _ = _clip_args(w2, starts, ends, window, wav_len, video, None)
    if resampling:
        return _resampled_logmel(w2, B, s, e, ln, vi, window, sample_rate, resample, F, dtype == torch.float64)
    return ops.logmel(w2, _WAV_DTYPES[w2.dtype], ln, vi, s, e, B, window, F, _tables(w2.device), out_f64=dtype == torch.float64)


def clip_audio(wav: Tensor, starts, ends, *, size=(112, 192), window: int = DEFAULT_WINDOW, exists=None,
               sample_rate: int = SAMPLE_RATE, wav_len=None, video=None, resample=None) -> Tensor:
    """The reference's ``data['audio']`` for a batch of clips, ``[B, 1, 9, h, w]`` float32 with ``size = (h, w)`` (half the
    frame size): nine examples of 64 log-mel frames x 64 bands each, bilinearly resized as ``F.interpolate(mode="bilinear",
    align_corners=False)`` does in float32.  Clips with ``exists[b]`` false are zeros.  With ``resample=`` and a ``sample_rate``
    other than 16000, ``starts`` / ``ends`` / ``window`` are at ``sample_rate`` and the padded excerpt is resampled first (three
    launches)."""
    resampling = _check_rate(sample_rate, resample)
    window = int(window)
    n_out = resampled_length(window, sample_rate) if resampling else window
    Fn = frames_needed(n_out)
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"audio_input: size must be (h, w), got {size!r}") from None
    w2 = _wav2(wav, wav_len, video)
    B, s, e, ln, vi, ex = _clip_args(w2, starts, ends, window, wav_len, video, exists)
    if resampling:
        lm = _resampled_logmel(w2, B, s, e, ln, vi, window, sample_rate, resample, Fn, False)
    else:
        lm = ops.logmel(w2, _WAV_DTYPES[w2.dtype], ln, vi, s, e, B, window, Fn, _tables(w2.device), out_f64=False)
    return ops.audio_examples(lm, ex, num_examples(n_out), h, w)


def examples(wav: Tensor, starts, ends, *, window: int = DEFAULT_WINDOW, exists=None, sample_rate: int = SAMPLE_RATE, wav_len=None,
             video=None, resample=None) -> Tensor:
    """What ``get_mel_feature`` returns per clip, ``[B, 9, 1, 64, 64]`` float32, contiguous: the nine examples before the resize
    (``clip_audio`` at 64 x 64, where the resize is the identity; the two singleton axes trade places without a copy)."""
    out = clip_audio(wav, starts, ends, size=(EXAMPLE_FRAMES, NUM_MEL_BINS), window=window, exists=exists, sample_rate=sample_rate,
                     wav_len=wav_len, video=video, resample=resample)
    return out.view(out.shape[0], NUM_EXAMPLES, 1, EXAMPLE_FRAMES, NUM_MEL_BINS)
