"""bench.py --dump-outputs: one more step of the timed path, from the seeded state, on the last timed step's batch, as
DIR/<name>.npy within a byte budget, the same files for the same arguments; --steps sets the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


class _FakeStep:
    """outputs() / state_dict() shaped like a step's: float arrays of several sizes and an integer BatchNorm counter."""

    def outputs(self):
        g = torch.Generator().manual_seed(1)
        return {"x_tilde": torch.randn(16, 3, 32, 32, generator=g), "mus": torch.randn(16, 8, generator=g)}

    def state_dict(self):
        g = torch.Generator().manual_seed(2)
        return {"enc.fc.weight": torch.randn(300, 200, generator=g), "enc.bn.bias": torch.randn(200, generator=g),
                "enc.bn.num_batches_tracked": torch.tensor(5, dtype=torch.int64)}


def test_dump_within_budget_and_reproducible(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)
    logs = {"loss_encoder": 1.25, "train_dis": True}
    a = bench.dump_outputs(_FakeStep(), logs, str(tmp_path / "a"))
    b = bench.dump_outputs(_FakeStep(), logs, str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and len(names) == a["files"] == 7
    assert a["bytes"] == sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 200_000
    # the two large arrays are cut to seeded samples of their flattened elements, the small ones are whole
    assert set(a["sampled"]) == {"out.x_tilde", "param.enc.fc.weight"}
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), n
    full = _FakeStep().state_dict()["enc.fc.weight"].reshape(-1).numpy()
    w = np.load(tmp_path / "a" / "param.enc.fc.weight.npy")
    assert w.shape == (a["sampled"]["param.enc.fc.weight"]["kept"],) and np.isin(w, full).all()
    assert np.load(tmp_path / "a" / "out.mus.npy").shape == (16, 8)
    assert float(np.load(tmp_path / "a" / "log.loss_encoder.npy")) == 1.25
    assert float(np.load(tmp_path / "a" / "log.train_dis.npy")) == 1.0
    assert np.load(tmp_path / "a" / "param.enc.bn.num_batches_tracked.npy").dtype == np.float64


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr


@pytest.mark.gpu
def test_bench_dump_outputs_end_to_end(tmp_path):
    """An eager run (no launch-mode probe): the engine's own step count before the reset is warm-up + timed steps, and
    the dump is one step from the seeded state on the last timed step's batch.  Two runs with the default launch-mode
    choice: the same files, equal up to the unordered sums of the timed path (the first optimizer update after the reset
    turns a gradient element at rounding level into +-3.16 lr, hence a norm criterion for the arrays)."""
    def run(out, *extra):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2", "--batch", "8",
               "--no-cpu-baseline", "--no-hbm-rows", "--no-pmc", "--no-gate-pass", "--dump-outputs", str(out), *extra]
        env = {k: v for k, v in os.environ.items() if k != "FMRI_DETERMINISTIC"}
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads(r.stdout)
    line = run(tmp_path / "eager", "--eager")
    d = line["dump_outputs"]
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and d["launch"] == "eager" and d["batch"] == 2
    assert d["bn_counter_before_reset"] == ["encoder.conv.0.bn.num_batches_tracked", 2 + 3]
    out = tmp_path / "eager"
    assert int(np.load(out / "param.encoder.conv.0.bn.num_batches_tracked.npy")) == 1
    assert np.load(out / "out.x_tilde.npy").shape == (8, 3, 64, 64)
    assert d["bytes"] <= 64 * 10**6 and d["files"] == len(os.listdir(out))
    run(tmp_path / "a")
    run(tmp_path / "b")
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    for n in names:
        x, y = (np.load(tmp_path / r / n).astype(np.float64) for r in ("a", "b"))
        assert np.isfinite(x).all() and np.isfinite(y).all(), n
        if n.startswith("log."):
            assert x == pytest.approx(y, rel=1e-4, abs=1e-6), n
        else:
            assert np.linalg.norm(x - y) <= 1e-2 * np.linalg.norm(y) + 1e-6, n
