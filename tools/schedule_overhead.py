#!/usr/bin/env python3
"""GPU box: cost of the device-side epoch-end schedule and training log (``schedule=EpochSchedule(...)``,
``log=TrainLog(...)``, fmri_hip/schedule.py) on the Stage-I step at B = 256, 64 x 64 x 3.

Two fed Stage-I steps in one process, the same pool, seeds and weights, one built with schedule + log and one without,
in the same launch mode -- recorded with ``capture()`` (``graph``) and, separately, issued eagerly (``eager``) -- timed
alternately with device events: warm-up, then ``repeats`` windows of ``steps`` steps each.  The pool is small enough that the
windows cross epoch boundaries (``--pool`` / batch steps per epoch), so the schedule's epoch-end arithmetic is inside the
measurement.  What the two launches add per step is also timed alone (``launches_alone``: fmri_epoch_begin +
fmri_trainlog_append, back to back on an idle stream).

Prints one JSON line.

usage: tools/schedule_overhead.py [--batch 256] [--pool 2048] [--steps 100] [--repeats 5] [--warmup 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "thesis-fmri-reconstruction_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _windows(fns, n, repeats):
    """ms per call of every callable in ``fns`` (dict), the callables alternating window by window."""
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / n)
    return {k: dict(median=round(float(np.median(v)), 5), min=round(min(v), 5), max=round(max(v), 5),
                    all=[round(u, 5) for u in v]) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--pool", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from fmri_hip import lib, ops
    from fmri_hip.feed import DeviceDataset, DeviceFeed
    from fmri_hip.params import ArchConfig
    from fmri_hip.rng import DeviceRng
    from fmri_hip.schedule import EpochSchedule, TrainLog
    from fmri_hip.steps import Stage1Step
    lib.load()
    dev = torch.device("cuda:0")
    B, N, S = a.batch, a.pool, 64
    gen = torch.Generator(device=dev).manual_seed(0)
    pool = torch.randint(0, 256, (N, S, S, 3), dtype=torch.uint8, device=dev, generator=gen)
    ds = DeviceDataset(pool)
    cfg = ArchConfig.px64()
    out = {"batch": B, "pool": N, "steps_per_epoch": N // B, "steps": a.steps, "repeats": a.repeats}

    def make(on):
        g = DeviceRng(7, dev)
        feed = DeviceFeed(ds, B, 11, rng=g, flip=True, max_shift=5)
        extra = dict(schedule=EpochSchedule(lr_gamma=0.98), log=TrainLog(capacity=4096)) if on else {}
        st = Stage1Step(cfg, dev, rng=g, feed=feed, **extra)
        st.load_recipe(1, True)
        return st

    for mode in ("graph", "eager"):
        steps = {"off": make(False), "on": make(True)}
        fns = {k: (st.capture() if mode == "graph" else st.step) for k, st in steps.items()}
        for fn in fns.values():
            for _ in range(a.warmup):
                fn()
        ops.join_side()
        torch.cuda.synchronize()
        t = _windows(fns, a.steps, a.repeats)
        ops.join_side()
        torch.cuda.synchronize()
        on = steps["on"]
        h = on.history()
        out[mode] = {"ms_per_step": t, "on_minus_off_ms": round(t["on"]["median"] - t["off"]["median"], 4),
                     "off_spread_ms": round(t["off"]["max"] - t["off"]["min"], 4),
                     "losses_finite": bool(all(np.isfinite(h[k]).all() for k in on.log.losses)),
                     "steps_logged": int(h["step"][-1]) + 1, "epochs_crossed": int(h["epoch"][-1]),
                     "lr_last": float(h["lr_encoder"][-1]), "position": list(on.feed.position())}
        if mode == "eager":
            alone = {"launches_alone": lambda: (on._epoch_begin(), on._log_append())}
            out["launches_alone_ms"] = _windows(alone, 1000, a.repeats)["launches_alone"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
