"""bench.py: a plain run does only what its headline needs; --full adds the gate-skip pass, the per-kernel family /
roofline pass, the HBM-bound kernel rows and the CPU baseline, each of which its --no-* option switches off."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EXTRAS = {"roofline", "families", "gate_skip", "hbm_bound_kernels", "cpu_baseline"}


def _run(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2", "--batch", "8", "--eager",
           *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout)


@pytest.mark.gpu
def test_plain_run_is_the_headline_only():
    line = _run()
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(line)
    assert not EXTRAS & set(line), sorted(EXTRAS & set(line))
    assert line["steps"] == 3 and line["warmup"] == 2 and line["losses_finite"] is True
    assert abs(line["value"] - 8 * 3 / (line["ms_per_step"] * 3e-3)) < 0.01 * line["value"]


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements():
    line = _run("--full", "--no-pmc", "--no-cpu-baseline")
    assert EXTRAS - set(line) == {"cpu_baseline"}
    assert line["roofline"]["kernel"] != "none" and line["roofline"]["launches_per_step"] > 0
    assert line["families"]["groups"] and line["families"]["ms_per_step_one_stream"] > 0
    assert line["gate_skip"]["steps"] == 3 and line["gate_skip"]["value"] > 0
    assert set(line["hbm_bound_kernels"]["rows"]) == {"cognitive_fc1_fwd", "bn_apply", "bn_bwd_apply_2streams",
                                                      "rmsprop_encoder"}
