#!/usr/bin/env python3
"""GPU box: cost of the device-side noise draws (``rng=DeviceRng(...)``, fmri_hip/rng.py) on the Stage-I step at B = 256.

Two engines in one process -- one handed its noise (``step(x, eps, z_p)``), one drawing it (``step(x)``: two
fmri_rng_normal launches + one fmri_rng_advance) -- timed alternately in two launch modes, eager and ``capture()``
replay: 20 warm-up steps each, then 5 repeats of 100 steps per engine, each repeat timed with device events.  Prints one
JSON line: per mode and engine the median and spread (min, max) in ms/step, and the median overhead.

usage: tools/rng_overhead.py [--batch 256] [--steps 100] [--repeats 5] [--warmup 20]
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
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import Stage1Step
    lib.load()
    dev = torch.device("cuda:0")
    cfg = ArchConfig.px64()
    rs = np.random.RandomState(0)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(dev)
    B = a.batch
    x, e, z = torch.tanh(t(B, 3, 64, 64)), t(B, cfg.latent_dim), t(B, cfg.latent_dim)
    out = {"batch": B, "steps": a.steps, "repeats": a.repeats}
    for mode in ("eager", "graph"):
        run = {}
        for k in ("handed", "drawn"):
            st = Stage1Step(cfg, dev, rng=DeviceRng(7, dev) if k == "drawn" else None)
            st.load_recipe(1, True)
            args = (x,) if k == "drawn" else (x, e, z)
            fn = (lambda st=st, args=args: st.step(*args)) if mode == "eager" else st.capture(*args)
            for _ in range(a.warmup):
                fn()
            run[k] = (st, fn)
        torch.cuda.synchronize()
        times = {"handed": [], "drawn": []}
        for _ in range(a.repeats):
            for k in ("handed", "drawn"):
                fn = run[k][1]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.steps)
        med = {k: float(np.median(v)) for k, v in times.items()}
        finite = all(bool(np.isfinite(v)) for k in run for v in run[k][0].logs().values())
        out[mode] = {"ms_per_step": {k: dict(median=round(med[k], 4), min=round(min(v), 4), max=round(max(v), 4),
                                             all=[round(u, 4) for u in v]) for k, v in times.items()},
                     "overhead_ms": round(med["drawn"] - med["handed"], 4),
                     "overhead_pct": round(100.0 * (med["drawn"] / med["handed"] - 1.0), 2),
                     "losses_finite": finite}
        del run
    print(json.dumps(out))


if __name__ == "__main__":
    main()
