#!/usr/bin/env python3
"""GPU box: cost of the numerics monitor (``monitor=True``) on the Stage-I step at B = 256, eager launches.

Two engines (monitor off / on) in one process, timed alternately: 20 warm-up steps each, then 5 repeats of 100 steps
per engine, each repeat timed with device events.  Prints one JSON line: per-engine median and spread (min, max) in
ms/step, and the median overhead.

usage: tools/monitor_overhead.py [--batch 256] [--steps 100] [--repeats 5] [--warmup 20]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from fmri_hip import lib
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import Stage1Step
    lib.load()
    dev = torch.device("cuda:0")
    cfg = ArchConfig.px64()
    rs = np.random.RandomState(0)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(dev)
    B = a.batch
    x, e, z = torch.tanh(t(B, 3, 64, 64)), t(B, cfg.latent_dim), t(B, cfg.latent_dim)
    eng = {}
    for on in (False, True):
        st = Stage1Step(cfg, dev, monitor=on)
        st.load_recipe(1, True)
        for _ in range(a.warmup):
            st.step(x, e, z)
        eng["on" if on else "off"] = st
    torch.cuda.synchronize()
    times = {"off": [], "on": []}
    for _ in range(a.repeats):
        for k in ("off", "on"):
            st = eng[k]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                st.step(x, e, z)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.steps)
    num = eng["on"].numerics()
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({"batch": B, "steps": a.steps, "repeats": a.repeats,
                      "ms_per_step": {k: dict(median=round(med[k], 4), min=round(min(v), 4), max=round(max(v), 4),
                                              all=[round(u, 4) for u in v]) for k, v in times.items()},
                      "overhead_ms": round(med["on"] - med["off"], 4),
                      "overhead_pct": round(100.0 * (med["on"] / med["off"] - 1.0), 2),
                      "losses_finite": num["losses_finite"],
                      "grad_norm": {k: v["norm"] for k, v in num["grad"].items()}}))


if __name__ == "__main__":
    main()
