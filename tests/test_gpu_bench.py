"""bench.py on the GPU: a plain run prints the contract line without the records that --full adds,
--steps sets the number of timed steps, and a plain run times the very steps a --full run times:
what --dump-outputs writes for the last timed step is identical in both."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, ENVS = 7, 2048
ARGS = ["--gpus", "1", "--steps", str(STEPS), "--warmup", "3", "--envs", str(ENVS), "--profile-steps", "12"]
NAMES = ("obs", "reward", "done", "terminal_observation")


@pytest.mark.parametrize("launch", [[], ["--rollout", "5"]], ids=["step", "rollout5"])
def test_plain_and_full_runs_time_the_same_steps(launch, tmp_path):
    extra = {"plain": [], "full": ["--full", "--no-cpu-baseline", "--no-rollout-line"]}
    procs = {k: subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + launch + x +
                                 ["--dump-outputs", str(tmp_path / k)], stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, text=True) for k, x in extra.items()}
    lines = {}
    for k, p in procs.items():
        out, err = p.communicate(timeout=170)
        assert p.returncode == 0, err[-2000:]
        js = [ln for ln in out.splitlines() if ln.startswith("{")]
        assert len(js) == 1, out
        lines[k] = json.loads(js[0])
    for k, d in lines.items():
        assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        assert d["steps"] == STEPS and d["ms_per_step"] > 0
        assert d["value"] == pytest.approx(ENVS * STEPS / (d["ms_per_step"] * STEPS * 1e-3), rel=1e-9)
        assert d["full"] is (k == "full")
    assert not {"roofline", "cpu_baseline", "open_loop_rollout"} & set(lines["plain"])
    assert lines["full"]["roofline"]["kernel_ms"] > 0
    assert lines["plain"]["config"] == {**lines["full"]["config"],
                                        "action_fill_ms_per_step": lines["plain"]["config"]["action_fill_ms_per_step"]}
    for n in NAMES:
        a, b = (np.load(str(tmp_path / k / (n + ".npy"))) for k in ("plain", "full"))
        assert a.dtype == np.float32 and a.shape[0] == ENVS and np.isfinite(a).all()
        assert np.array_equal(a, b), n
    assert np.load(str(tmp_path / "plain" / "obs.npy")).any()
