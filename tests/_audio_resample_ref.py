"""NumPy restatement of the audio front end's resampling stage (include/diffsal.h, "audio front end"): resampy 0.4.2's
``resampy.core.resample`` and ``resampy.interp._resample_loop`` with its ``kaiser_best`` / ``kaiser_fast`` filters designed as
``resampy.filters.sinc_window`` designs them.  ``resample`` walks the tap index and carries every output sample along as one
vector, so each output's sum is formed in the library's order -- left wing in ascending i, then right wing in ascending k, every
product and every sum one float64 operation (numpy's element-wise ufuncs do not fuse) -- and is what the device must reproduce
bit for bit.  Test-side only: the package never imports it."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio_resample.npz")
FILTERS = {"kaiser_best": dict(num_zeros=64, precision=9, rolloff=0.9475937167399596, beta=14.769656459379492),
           "kaiser_fast": dict(num_zeros=16, precision=9, rolloff=0.85, beta=8.555504641634386)}
_MEMO = {}


def sinc_window(num_zeros, precision, rolloff, beta):
    """(half window [num_zeros * 2^precision + 1], 2^precision)"""
    num_bits = 2 ** precision
    n = num_bits * num_zeros
    sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=n + 1, endpoint=True))
    taper = np.kaiser(2 * n + 1, beta)[n:]
    return taper * sinc_win, num_bits


def get_filter(name):
    if name not in _MEMO:
        _MEMO[name] = sinc_window(**FILTERS[name])
    return _MEMO[name]


def out_len(n, sr_orig, sr_new=16000):
    return int(n * sr_new / sr_orig)


def scaled_filter(half_window, sr_orig, sr_new):
    """(win, delta): the window multiplied by the ratio for a downsample, and its differences with a final zero"""
    ratio = float(sr_new) / sr_orig
    win = np.array(half_window, dtype=np.float64)
    if ratio < 1:
        win = ratio * win
    return win, np.diff(win, append=win[-1])


def index_step(sr_orig, sr_new, num_table):
    return int(min(1.0, float(sr_new) / sr_orig) * num_table)


def resample(x, sr_orig, sr_new=16000, filt="kaiser_best", n_out=None, taps=None):
    """``resampy.resample(x, sr_orig, sr_new, filter=filt)`` of a 1-D float64 ``x`` (or its first ``n_out`` samples); ``filt`` is a
    name or a ``(half_window, num_table)`` pair.  ``taps``, a list, receives the largest tap count of one output."""
    x = np.asarray(x, dtype=np.float64)
    half, num_table = get_filter(filt) if isinstance(filt, str) else filt
    ratio = float(sr_new) / sr_orig
    n = x.shape[0]
    full = out_len(n, sr_orig, sr_new)
    n_out = full if n_out is None else n_out
    assert 0 <= n_out <= full
    win, delta = scaled_filter(half, sr_orig, sr_new)
    nwin = win.shape[0]
    scale = min(1.0, ratio)
    inc = 1.0 / ratio
    step = int(scale * num_table)
    time = np.arange(n_out) * inc
    m = time.astype(np.int64)
    y = np.zeros(n_out)
    count = np.zeros(n_out, dtype=np.int64)
    frac = scale * (time - m)
    for wing in (0, 1):
        if wing:
            frac = scale - frac
        f = frac * num_table
        off = f.astype(np.int64)
        eta = f - off
        limit = np.minimum(m + 1 if wing == 0 else n - m - 1, (nwin - off) // step)
        count += np.maximum(limit, 0)
        for i in range(int(limit.max()) if n_out else 0):
            on = np.nonzero(i < limit)[0]
            j = off[on] + i * step
            xi = x[m[on] - i] if wing == 0 else x[m[on] + i + 1]
            y[on] = y[on] + (win[j] + eta[on] * delta[j]) * xi
    if taps is not None:
        taps.append(int(count.max()) if n_out else 0)
    return y


def resample_scalar(x, sr_orig, sr_new=16000, filt="kaiser_best"):
    """The loop of include/diffsal.h as written, one output and one tap at a time (slow: for short inputs, to check ``resample``)."""
    x = np.asarray(x, dtype=np.float64)
    half, num_table = get_filter(filt) if isinstance(filt, str) else filt
    ratio = float(sr_new) / sr_orig
    n = x.shape[0]
    win, delta = scaled_filter(half, sr_orig, sr_new)
    nwin = win.shape[0]
    scale, inc = min(1.0, ratio), 1.0 / ratio
    step = int(scale * num_table)
    y = np.zeros(out_len(n, sr_orig, sr_new))
    for t in range(y.shape[0]):
        time = t * inc
        m = int(time)
        frac = scale * (time - m)
        f = frac * num_table
        off = int(f)
        eta = f - off
        acc = 0.0
        for i in range(min(m + 1, (nwin - off) // step)):
            acc = acc + (win[off + i * step] + eta * delta[off + i * step]) * x[m - i]
        frac = scale - frac
        f = frac * num_table
        off = int(f)
        eta = f - off
        for k in range(min(n - m - 1, (nwin - off) // step)):
            acc = acc + (win[off + k * step] + eta * delta[off + k * step]) * x[m + k + 1]
        y[t] = acc
    return y


# the seeded signals of tests/_audio_input_ref.py the fixture records, resampled from a full window: (signal, sr_orig, filter)
GOLDEN_CASES = (("noise", 22050, "kaiser_best"), ("tone", 22050, "kaiser_best"), ("chirp", 22050, "kaiser_best"),
                ("lsb", 22050, "kaiser_best"), ("noise", 44100, "kaiser_best"), ("chirp", 48000, "kaiser_best"),
                ("noise", 8000, "kaiser_best"), ("chirp", 11025, "kaiser_best"), ("noise", 22050, "kaiser_fast"))
GOLDEN_STRIDE = 97
GOLDEN_INPUT = 6000      # samples of the signal that are resampled


def golden_key(sig, sr, filt):
    return f"{sig}_{sr}_{filt}"


def load_golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}
