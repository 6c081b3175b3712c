"""bench.py on the GPU: a plain run times exactly --steps steps once and prints the headline line only; --dump-outputs writes
what the last timed step returned, the same arrays for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    j = _plain_run(tmp_path / "a")
    assert j["unit"] == "denoise-steps/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert j["steps"] == 3 and j["warmup"] == 1 and j["repeats"] == 1 and len(j["ms_per_step_all_regions"]) == 1
    assert j["ms_per_step"] > 0 and j["value"] == pytest.approx(4 * 1e3 / j["ms_per_step"], rel=1e-3)
    for k in ("roofline", "alt_precision", "end_to_end", "train", "cpu_baseline"):
        assert k not in j, k                 # --full only
    # the third evaluation of a trajectory is a fused step: it hands the sampler the noise prediction and the next solver state
    assert sorted(os.listdir(tmp_path / "a")) == ["noise_pred.npy", "x_next.npy"]
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("noise_pred", "x_next")}
    for n, v in a.items():
        assert v.dtype == np.float32 and v.shape == (4, 1, 224, 384) and np.isfinite(v).all(), n
    assert float(np.abs(a["x_next"]).max()) > 0
    # same arguments, same inputs: a second run computes the same arrays
    _plain_run(tmp_path / "b")
    for n, v in a.items():
        w = np.load(tmp_path / "b" / f"{n}.npy")
        assert np.abs(w - v).max() <= 1e-5 * max(1.0, float(np.abs(v).max())), n
