"""The resampling stage of the audio front end without a GPU: the NumPy restatement of resampy 0.4.2's loop
(tests/_audio_resample_ref.py) -- lengths, tap counts, the filter's pass band and stop band, the recorded fixture, the library itself
where it is installed -- the package's host functions against it bit for bit, and the argument checks of the C entry point, which
all precede the launch.

Filter bars.  The restatement was measured once: 32000 -> 16000 (``step`` exact) gives a 1 kHz tone to 1.2e-8 and leaves 6.4e-9 of
a 9 kHz tone; 22050 -> 16000 gives a 1 kHz tone to 6e-4, the error of the library's truncated table step (371 for 371.52), which is
to be reproduced.  The bars are about ten times those figures, so that a last-place difference between two Bessel-function
implementations cannot fail them while a wrong roll-off, beta, table size or step does; the band at 22050 says the truncated step
is neither repaired nor made worse."""
import numpy as np
import pytest
import torch

from diff_sal_amd import _lib
from diff_sal_amd import audio_input as ai
from tests import _audio_input_ref as ref
from tests import _audio_resample_ref as rs

WINDOW = 35280


def _tone(freq, sr, n):
    return np.sin(2 * np.pi * freq * np.arange(n) / sr)


# ------------------------------------------------------------------------------------------------------ lengths and tap counts
@pytest.mark.parametrize("sr,n_out,step,taps", [(22050, 25600, 371, 175), (44100, 12800, 185, 353), (48000, 11760, 170, 383),
                                                (11025, 51200, 512, 127), (8000, 70560, 512, 127), (32000, 17640, 256, 255)])
def test_lengths_steps_and_tap_counts(sr, n_out, step, taps):
    """taps: both wings of an output in the middle of a long input.  With off in [0, step) on the left and (0, step] on the right,
    an output has between 2 (nwin // step) - 1 and 2 (nwin // step) + 1 taps; the recorded figures are what the restatement gives"""
    assert rs.out_len(WINDOW, sr) == n_out == ai.resampled_length(WINDOW, sr)
    assert rs.index_step(sr, 16000, 512) == step
    got = []
    rs.resample(np.ones(4000), sr, 16000, taps=got)
    wing = 32769 // step
    assert 2 * wing - 1 <= got[0] <= 2 * wing + 1
    assert got[0] == taps, got


def test_the_protocol_window_gives_158_frames_and_nine_examples():
    n = ai.resampled_length(ai.DEFAULT_WINDOW, 22050)
    assert (n, ai.num_frames(n), ai.num_examples(n), ai.frames_needed(n)) == (25600, 158, 9, 152)
    assert (ai.num_frames(WINDOW), ai.num_examples(WINDOW)) == (219, 15)      # the same window taken for 16 kHz samples


def test_the_vectorised_restatement_is_the_scalar_loop():
    x = ref.signal("noise")[:700] / 32768.0
    for sr, filt in ((22050, "kaiser_best"), (48000, "kaiser_best"), (8000, "kaiser_fast")):
        assert np.array_equal(rs.resample(x, sr, 16000, filt), rs.resample_scalar(x, sr, 16000, filt)), (sr, filt)
    assert np.array_equal(rs.resample(x, 22050, n_out=100), rs.resample(x, 22050)[:100])


# --------------------------------------------------------------------------------------------------------- package host functions
@pytest.mark.parametrize("name", sorted(rs.FILTERS))
def test_package_filter_table_and_length_are_the_restatement(name):
    half, num_table = ai.resample_filter(name)
    want, want_table = rs.get_filter(name)
    assert num_table == want_table == 512 and half.dtype == np.float64
    assert half.shape == ({"kaiser_best": 32769, "kaiser_fast": 8193}[name],)
    assert np.array_equal(half, want)
    for sr in (22050, 44100, 8000):
        t = ai.resample_table(half, num_table, sr)
        win, delta = rs.scaled_filter(want, sr, 16000)
        assert t.shape == (half.shape[0], 2) and t.dtype == np.float64 and t.flags.c_contiguous
        assert np.array_equal(t[:, 0], win) and np.array_equal(t[:, 1], delta) and t[-1, 1] == 0.0
    assert np.array_equal(ai.resample_table(half, num_table, 8000)[:, 0], want)      # an upsample leaves the window unscaled
    with pytest.raises(ValueError, match="kaiser_best"):
        ai.resample_filter("sinc")


def test_lengths_from_python_and_from_the_library_agree():
    lib = _lib.load()
    rng = np.random.default_rng(5)
    for sr in (22050, 44100, 48000, 11025, 8000, 32000, 12345):
        for n in [0, 1, 2, WINDOW, 1 << 24] + rng.integers(1, 1 << 24, size=50).tolist():
            assert ai.resampled_length(n, sr) == rs.out_len(n, sr) == lib.diffsal_resample_length(n, sr, 16000), (n, sr)
    assert lib.diffsal_resample_length(-1, 22050, 16000) == -1 and lib.diffsal_resample_length(5, 0, 16000) == -1


# ---------------------------------------------------------------------------------------------------------------- filter properties
def test_pass_band_and_stop_band_at_an_exact_step():
    n = 6000
    y = rs.resample(_tone(1000.0, 32000, n), 32000)
    mid = slice(300, y.shape[0] - 300)
    err = np.abs(y - _tone(1000.0, 16000, y.shape[0]))[mid].max()
    stop = np.abs(rs.resample(_tone(9000.0, 32000, n), 32000))[mid].max()
    up = rs.resample(_tone(1000.0, 8000, 3000), 8000)
    up_err = np.abs(up - _tone(1000.0, 16000, up.shape[0]))[300:-300].max()
    print(f"32000 -> 16000: 1 kHz error {err:.2e}, 9 kHz residual {stop:.2e}; 8000 -> 16000: 1 kHz error {up_err:.2e}")
    assert err < 1e-6 and stop < 1e-6 and up_err < 1e-6


def test_the_truncated_step_at_22050_is_reproduced():
    y = rs.resample(_tone(1000.0, 22050, 6000), 22050)
    err = np.abs(y - _tone(1000.0, 16000, y.shape[0]))[300:-300].max()
    print(f"22050 -> 16000: 1 kHz error {err:.2e}")
    assert 1e-4 < err < 2e-3


# ------------------------------------------------------------------------------------------------------------ fixture and library
def test_recorded_fixture():
    gold = rs.load_golden()
    print("fixture produced by:", str(gold["source"]))
    from_library = str(gold["source"]) != "restatement"
    for sig, sr, filt in rs.GOLDEN_CASES:
        key = rs.golden_key(sig, sr, filt)
        y = rs.resample(ref.signal(sig)[:rs.GOLDEN_INPUT] / 32768.0, sr, 16000, filt)
        assert y.shape[0] == int(gold[key + "/length"])
        if from_library:      # the bar of the comparison with the library below
            assert np.abs(y[::rs.GOLDEN_STRIDE] - gold[key + "/samples"]).max() <= 2.0 ** -24, key
        else:
            assert np.array_equal(y[::rs.GOLDEN_STRIDE], gold[key + "/samples"]), key
            assert np.add.accumulate(y)[-1] == float(gold[key + "/sum"]), key


def test_against_the_library_where_it_is_installed():
    """2^-24: half a float32 step at unit scale -- the inputs lie in [-1, 1] and everything downstream is rounded to float32"""
    resampy = pytest.importorskip("resampy")
    stored = resampy.filters.get_filter("kaiser_best")
    assert len(stored[0]) == 32769 and stored[1] == 512
    worst = 0.0
    for sig in ("noise", "chirp"):
        x = ref.signal(sig) / 32768.0
        for sr in (22050, 44100, 8000):
            d = float(np.abs(rs.resample(x, sr) - resampy.resample(x, sr, 16000)).max())
            print(f"{sig} {sr} -> 16000: restatement against resampy {resampy.__version__}: worst |d| = {d:.3e}")
            worst = max(worst, d)
    assert worst <= 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib.load()
    P = 256      # never dereferenced: every check precedes the launch

    def call(dtype=0, V=1, L=48000, B=2, window=35280, sr=22050, to=16000, table=P, nwin=32769, num_table=512, n=25600, wav=P, out=P):
        return lib.diffsal_resample_excerpts(wav, dtype, V, L, None, None, P, P, B, window, sr, to, table, nwin, num_table, n, out, None)

    assert call(sr=16000) == -4 and b"equal" in lib.diffsal_last_error()
    assert call(sr=0) == -4 and b"positive" in lib.diffsal_last_error()
    assert call(to=-16000) == -4 and b"positive" in lib.diffsal_last_error()
    assert call(dtype=3) == -4 and b"wav_dtype" in lib.diffsal_last_error()
    assert call(n=25601) == -1 and b"gives 25600" in lib.diffsal_last_error()
    assert call(n=0) == -1
    assert call(sr=44100, n=12801) == -1 and b"gives 12800" in lib.diffsal_last_error()
    assert call(table=264) == -4 and b"aligned" in lib.diffsal_last_error()
    assert call(table=None) == -4 and call(wav=None) == -4 and call(out=None) == -4
    assert call(nwin=1) == -1
    assert call(num_table=1) == -1 and b"steps 0" in lib.diffsal_last_error()            # int(0.7256 * 1) = 0
    assert call(sr=16000 * 40, window=1 << 20, n=100) == -1 and b"stages" in lib.diffsal_last_error()      # 255 * 40 inputs a tile
    assert call(B=0) == -1 and call(V=0) == -1 and call(L=0) == -1 and call(window=0) == -1


def test_python_argument_rules_without_a_gpu():
    cpu = torch.zeros(48000, dtype=torch.int16)
    for fn in (ai.clip_audio, ai.log_mel, ai.examples):
        with pytest.raises(ValueError, match="resample on load"):
            fn(cpu, [0], [100], sample_rate=22050)                                       # without the keyword: as it always was
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(cpu, [0], [100], sample_rate=22050, resample="kaiser_best")
    with pytest.raises(RuntimeError, match="GPU only"):
        ai.resample_excerpts(cpu, [0], [100], window=1500, sample_rate=22050)
    with pytest.raises(ValueError, match="does not resample there"):
        ai.resample_excerpts(cpu, [0], [100], window=1500, sample_rate=16000)
    with pytest.raises(ValueError, match="samples asked"):
        ai.resample_excerpts(cpu, [0], [100], window=1500, sample_rate=22050, samples=1089)      # int(1500 * 16000 / 22050) = 1088
    with pytest.raises(ValueError, match="positive integer"):
        ai.clip_audio(cpu, [0], [100], sample_rate=22050.5, resample="kaiser_best")
    with pytest.raises(ValueError, match="too short for one example"):
        ai.clip_audio(cpu, [0], [100], window=14000, sample_rate=22050, resample="kaiser_best")      # 10158 samples at 16 kHz
