"""The audio front end without a GPU: the NumPy restatement (tests/_audio_input_ref.py) against the fixtures recorded from the
reference's mel_features.py (tools/gen_audio_input_golden.py), the package's host-side tables and index arithmetic against the
fixtures, against recorded values and against torch's own operators, and the argument checks of the C ABI, which precede any launch.

Bars.  The restatement runs the same numpy calls as the reference: bit-equal in float32.  The mel matrix and the window: exact.
The direct DFT the kernel computes, evaluated here in numpy from the table the kernel reads: 1e-9 in float64 -- 400-term sums of
terms below 1 carry about 400 x 1.1e-16 = 4e-14 of rounding, which ``log(x + 0.01)`` amplifies by at most 1 / 0.01 to 4e-12;
the FFT it is compared with has an error of its own of that size."""
import numpy as np
import pytest
import torch

from diff_sal_amd import _lib, audio_input as ai
from tests import _audio_input_ref as ref

GOLD = ref.load_cases()


def _signal(name):
    x = ref.signal("video", ref.VIDEO_SAMPLES) if name == "video" else ref.signal(name)
    assert ref.crc(x) == int(GOLD[f"crc/{name}"]), f"signal {name} is not the one the fixture was recorded from"
    return x


def test_signals_are_the_ones_the_fixture_was_recorded_from():
    for s in ref.SIGNALS + ("video",):
        _signal(s)
    assert np.abs(_signal("tone")).max() == 32767 and np.abs(_signal("lsb")).max() == 2 and not _signal("silence").any()


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_restatement_equals_the_reference_fixture(name):
    sig, window, v = ref.CASES[name]
    x = ref.padded_excerpt(_signal(sig)[:v], 0, v - 1, window)
    lm = ref.log_mel(x)
    want = GOLD[f"{name}/logmel"]
    assert lm.shape == want.shape == (ai.num_frames(window), 64)
    assert np.array_equal(lm.astype(np.float32), want)
    assert tuple(GOLD[f"{name}/examples_shape"]) == (ai.num_examples(window), 64, 64)
    assert ref.examples(lm).shape == (9, 64, 64)
    if sig == "silence":
        assert (want == np.float32(np.log(0.01))).all()


def test_restatement_equals_the_fixture_on_the_batch_video():
    video = _signal("video")
    starts, ends = ref.excerpt_table(ref.VIDEO_FRAMES, ref.VIDEO_FPS, ref.RATE, video.shape[0])
    vs = []
    for fa, fb in ref.VIDEO_CLIPS:
        lm = ref.log_mel(ref.padded_excerpt(video, starts[fa], ends[fb], ref.FULL))
        assert np.array_equal(lm[:152].astype(np.float32), GOLD[f"video/{fa}_{fb}/logmel"])
        vs.append(len(video[starts[fa]:ends[fb] + 1]))
    assert {v % 2 for v in vs} == {0, 1} and max(vs) < ref.FULL                   # an odd and an even excerpt, all padded
    assert ends[ref.VIDEO_CLIPS[-1][1]] == video.shape[0]                         # the last clip is clamped at the end of the audio


def test_mel_matrix_and_window_are_the_reference_s_exactly():
    assert np.array_equal(ai.mel_matrix(), GOLD["mel"]) and np.array_equal(ai.hann_window(), GOLD["window"])
    assert np.array_equal(ref.mel_matrix(), GOLD["mel"]) and np.array_equal(ref.hann_window(), GOLD["window"])
    m = GOLD["mel"]
    rows = np.nonzero(m.any(axis=1))[0]
    assert rows[0] == ai.BIN_LO and rows[-1] == ai.BIN_LO + ai.BIN_COUNT - 1      # bins 5..239
    assert max(int(np.count_nonzero(m[:, b])) for b in range(64)) == ai.BAND_TAPS
    assert (ai.STFT_WINDOW, ai.STFT_HOP, ai.FFT_LENGTH, ai.EXAMPLE_FRAMES, ai.EXAMPLE_HOP, ai.DEFAULT_WINDOW) == (400, 160, 512, 64, 11, 35280)
    assert [ai.num_examples(w) for w in (10480, 12345, 15760, 35280)] == [1, 2, 4, 15]
    assert [ai.num_frames(w) for w in (10480, 12345, 15760, 35280)] == [64, 75, 97, 219] and ai.frames_needed(35280) == 152


@pytest.mark.parametrize("name", ["full_tone", "full_noise", "w12345", "full_silence"])
def test_the_kernel_s_table_reproduces_the_reference(name):
    """The direct DFT of include/diffsal.h evaluated in numpy from ``device_tables``: what the kernel computes, up to the order
    of its sums."""
    sig, window, v = ref.CASES[name]
    x = ref.padded_excerpt(_signal(sig)[:v], 0, v - 1, window)
    t = ai.device_tables()
    assert t.size == ai.TABLE_DOUBLES == _lib.load().diffsal_logmel_table_doubles()
    nb = 2 * ai.STFT_WINDOW * ai.BIN_PITCH
    basis = t[:nb].reshape(ai.STFT_WINDOW, ai.BIN_PITCH, 2)
    w = t[nb:nb + 64 * ai.BAND_TAPS].reshape(64, ai.BAND_TAPS)
    first = t[nb + 64 * ai.BAND_TAPS:].astype(int)
    assert not basis[:, ai.BIN_COUNT:].any() and first.min() >= 0 and first.max() + ai.BAND_TAPS <= ai.BIN_PITCH
    fr = ref.frame(x, 400, 160)
    mag = np.hypot(fr @ basis[:, :, 0], fr @ basis[:, :, 1])
    mel = np.stack([(mag[:, first[b]:first[b] + ai.BAND_TAPS] * w[b]).sum(1) for b in range(64)], axis=1)
    got = np.log(mel + 0.01)
    want = ref.log_mel(x)
    d = float(np.abs(got - want).max())
    print(f"{name}: direct DFT from the table against the FFT, float64: worst |d| = {d:.2e}")
    assert d <= 1e-9
    assert (np.abs(got.astype(np.float32) - GOLD[f"{name}/logmel"]) <= np.spacing(np.abs(GOLD[f"{name}/logmel"]))).all()


@pytest.mark.parametrize("E", [1, 2, 4, 5, 9, 15])
def test_index_map_is_repeat_interleave_then_cat(E):
    """Each example is repeated 9 // E times (not at all when that is 0), the first 9 % E entries of the REPEATED list are
    appended, and nine are kept: with torch's own operators on example numbers."""
    numbers = torch.arange(E)
    repeated = torch.repeat_interleave(numbers, 9 // E) if 9 // E > 0 else numbers
    want = torch.cat([repeated, repeated[:9 % E]])[:9].numpy()
    assert want.shape == (9,)
    assert np.array_equal(ai.example_map(E), want) and np.array_equal(ref.nine_map(E), want)
    if E == 4:
        assert want.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 0]      # the ninth is the head of the repeated list, not example 1
    if E == 5:
        assert want.tolist() == [0, 1, 2, 3, 4, 0, 1, 2, 3]


# (fps, frames, samples): first entries of starts / ends, last three of each.  The values are the issue's formulas,
# int(max(0, (f - 1) * (1.0 / fps) * Fs - Fs / fps / 2)) and int(min(n_samples, |(f - 1) * (1.0 / fps) * Fs + Fs / fps / 2|)), Fs = 16000.
# By hand: at 25 fps a frame is 640 samples, so frame f covers 640 (f - 1) -+ 320; at 30 fps 533 1/3, so frame 4 starts at
# int(1600 - 266 2/3) = 1333 and frame 6 at exactly 2400; at 10 fps 1600, so frame 12 starts at 16800, beyond the 16000 samples
# (a start is clamped at 0 only), while the ends stop at 16000; at 29.97 fps frame 16 ends at int(8008.008 + 266.934) = 8274.
TABLES = {
    (25, 40, 32000): ([0, 0, 320, 960, 1600, 2240, 2880, 3520], [23360, 24000, 24640],
                      [0, 320, 960, 1600, 2240, 2880, 3520, 4160], [24000, 24640, 25280]),
    (29.97, 75, 39600): ([0, 0, 266, 800, 1334, 1868, 2402, 2936], [38171, 38705, 39239],
                         [0, 266, 800, 1334, 1868, 2402, 2936, 3470], [38705, 39239, 39600]),
    (10, 12, 16000): ([0, 0, 800, 2400, 4000, 5600, 7200, 8800], [13600, 15200, 16800],
                      [0, 800, 2400, 4000, 5600, 7200, 8800, 10400], [15200, 16000, 16000]),
    (30, 20, 9000): ([0, 0, 266, 800, 1333, 1866, 2400, 2933], [8800, 9333, 9866],
                     [0, 266, 800, 1333, 1866, 2400, 2933, 3466], [9000, 9000, 9000]),
}


@pytest.mark.parametrize("fps,n_frames,n_samples", sorted(TABLES))
def test_excerpt_table_against_recorded_values_and_the_restatement(fps, n_frames, n_samples):
    starts, ends = ai.excerpt_table(n_frames, fps, 16000, n_samples)
    s_head, s_tail, e_head, e_tail = TABLES[(fps, n_frames, n_samples)]
    assert starts.shape == ends.shape == (n_frames + 1,)
    assert starts[:8].tolist() == s_head and starts[-3:].tolist() == s_tail
    assert ends[:8].tolist() == e_head and ends[-3:].tolist() == e_tail
    ws, we = ref.excerpt_table(n_frames, fps, 16000, n_samples)      # the vectorised restatement, every entry
    assert np.array_equal(starts, ws) and np.array_equal(ends, we)
    if fps == 29.97:      # the clips of the batch video
        assert [int(starts[a]) for a, _ in ref.VIDEO_CLIPS] == [0, 4004, 1334, 31231]
        assert [int(ends[b]) for _, b in ref.VIDEO_CLIPS] == [8274, 12545, 9876, 39600]
    if fps in (29.97, 30, 10):
        assert ends[-1] == n_samples                                 # the last frames run past the end of the audio


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib.load()
    P = 256      # never dereferenced: every check precedes the launch

    def logmel(rate=16000, dtype=0, V=1, L=48000, B=2, window=35280, frames=152, f64=0, wav=P, tables=P):
        return lib.diffsal_logmel(wav, dtype, V, L, None, None, P, P, B, rate, window, frames, tables, f64, P, None)

    assert logmel(rate=44100) == -4 and b"16000" in lib.diffsal_last_error() and b"resample on load" in lib.diffsal_last_error()
    assert logmel(dtype=3) == -4 and b"wav_dtype" in lib.diffsal_last_error()
    assert logmel(f64=2) == -4
    assert logmel(B=0) == -1 and logmel(V=0) == -1 and logmel(L=0) == -1
    assert logmel(window=399) == -1 and b"one frame" in lib.diffsal_last_error()
    assert logmel(frames=220) == -1 and b"holds 219" in lib.diffsal_last_error()
    assert logmel(frames=0) == -1
    assert logmel(wav=None) == -4 and logmel(tables=None) == -4
    assert logmel(tables=264) == -4 and b"aligned" in lib.diffsal_last_error()

    def examples(B=2, frames=152, E=15, h=112, w=192, lm=P):
        return lib.diffsal_audio_examples(lm, None, B, frames, E, h, w, P, None)

    assert examples(E=0) == -1 and b"too short for one example" in lib.diffsal_last_error()
    assert examples(frames=151) == -1 and b"read 152" in lib.diffsal_last_error()
    assert examples(frames=74, E=2) == -1 and examples(frames=63, E=1) == -1
    assert examples(B=0) == -1 and examples(h=0) == -1 and examples(w=5000) == -1
    assert examples(lm=None) == -4


def test_python_argument_rules_without_a_gpu():
    cpu = torch.zeros(48000, dtype=torch.int16)
    with pytest.raises(ValueError, match="resample on load"):
        ai.clip_audio(cpu, [0], [100], sample_rate=22050)
    with pytest.raises(RuntimeError, match="GPU only"):
        ai.clip_audio(cpu, [0], [100])
    with pytest.raises(RuntimeError, match="GPU only"):
        ai.log_mel(cpu, [0], [100])
    with pytest.raises(ValueError, match="too short for one example"):
        ai.clip_audio(cpu, [0], [100], window=10479)
    with pytest.raises(ValueError, match="too short"):
        ai.example_map(0)
