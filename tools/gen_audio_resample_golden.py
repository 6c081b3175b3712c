"""Writes tests/golden/audio_resample.npz: the seeded int16 signals of tests/_audio_input_ref.py (their first 6000 samples, divided
by 32768) resampled to 16000 Hz from the rates and with the filters of ``GOLDEN_CASES`` in tests/_audio_resample_ref.py -- every
97th output sample, the output's length and its float64 sum taken in ascending order -- and a ``source`` field naming what
produced them: ``resampy <version>`` where the library can be imported, else ``restatement`` (tests/_audio_resample_ref.py).  A
few KB that pin the restatement against drift, and against the library once it has been run where the library exists.

    python tools/gen_audio_resample_golden.py

Needs numpy; no GPU.  No test runs this tool."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _audio_input_ref as ref  # noqa: E402
from tests import _audio_resample_ref as rs  # noqa: E402


def main():
    try:
        import resampy
        source = f"resampy {resampy.__version__}"

        def run(x, sr, filt):
            return resampy.resample(x, sr, 16000, filter=filt)
    except ImportError:
        source = "restatement"

        def run(x, sr, filt):
            return rs.resample(x, sr, 16000, filt)
    blob = {"source": np.array(source)}
    for sig, sr, filt in rs.GOLDEN_CASES:
        x = ref.signal(sig)[:rs.GOLDEN_INPUT] / 32768.0
        y = run(x, sr, filt)
        key = rs.golden_key(sig, sr, filt)
        blob[key + "/samples"] = y[::rs.GOLDEN_STRIDE]
        blob[key + "/length"] = np.array(y.shape[0], dtype=np.int64)
        blob[key + "/sum"] = np.array(np.add.accumulate(y)[-1])
        if source != "restatement":
            print(key, "restatement against the library: worst |d| =", float(np.abs(rs.resample(x, sr, 16000, filt) - y).max()))
        print(key, y.shape[0], "samples, sum", float(blob[key + "/sum"]))
    out = rs.GOLDEN
    np.savez_compressed(out, **blob)
    print(source, out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
