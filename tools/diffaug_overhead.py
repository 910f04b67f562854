#!/usr/bin/env python3
"""GPU box: cost of the differentiable augmentation (``augment=DiffAugment()``, fmri_hip/augment.py) at Stage-I's real
sizes: 64 x 64 px, z = 128.

1. Kernel rate: ``fmri_diffaug_fwd`` on [3B,64,64,8] and ``fmri_diffaug_bwd`` on two [2B,64,64,8] cotangents under a
   drawn table, each against ``ops.axpby`` (the library's plain one-read-one-write pass) over the same bytes, alternately
   in one process with device events.  Reported as ms per call, GB/s and the ratio of the rates.
2. End to end: a Stage-I step at ``--batch`` recorded with ``capture()`` -- fed, with ``rng=`` -- without the keyword, with
   ``augment=DiffAugment()`` and without it again, timed alternately, ``repeats`` windows of ``steps`` replays.

Prints one JSON line.

usage: tools/diffaug_overhead.py [--kernels-only] [--batch 256] [--pool 20000] [--calls 100] [--steps 100] [--repeats 5] [--warmup 20]
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

from state_overhead import _windows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--pool", type=int, default=20000)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true", help="part 1 only")
    a = ap.parse_args()
    from fmri_hip import ops
    from fmri_hip.augment import DiffAugment
    from fmri_hip.feed import DeviceDataset, DeviceFeed
    from fmri_hip.params import ArchConfig
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import Stage1Step
    dev = torch.device("cuda:0")
    B, N, S = a.batch, a.pool, 64
    out = {"batch": B, "pool": N, "calls": a.calls, "steps": a.steps, "repeats": a.repeats}

    # ---- 1. the two kernels against axpby over the same bytes ------------------------------------------------------------
    aug = DiffAugment()
    table = aug.table(DeviceRng(3, dev), B, S)
    x = (torch.rand(3 * B, S, S, 8, device=dev) * 2 - 1).half()
    g = torch.randn(2, 2 * B, S, S, 8, device=dev).mul_(16).half()
    xo, go = torch.empty_like(x), torch.empty_like(g)
    fns = {"diffaug_fwd": lambda: ops.diffaug_fwd(x, table, B, 0, out=xo),
           "axpby_fwd_bytes": lambda: ops.axpby(x, None, 0.5, 0.0, out=xo),
           "diffaug_bwd": lambda: ops.diffaug_bwd(g[0], g[1], table, B, B, out=(go[0], go[1])),
           "axpby_bwd_bytes": lambda: ops.axpby(g, None, 0.5, 0.0, out=go)}
    for fn in fns.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    t = _windows(fns, a.calls, a.repeats)
    moved = {"diffaug_fwd": 4 * x.numel(), "axpby_fwd_bytes": 4 * x.numel(), "diffaug_bwd": 4 * g.numel(),
             "axpby_bwd_bytes": 4 * g.numel()}
    gbps = {k: round(moved[k] / (t[k]["median"] * 1e-3) / 1e9, 1) for k in t}
    out["kernels"] = {"bytes_moved": moved, "ms_per_call": t, "GBps": gbps,
                      "fwd_rate_over_axpby": round(gbps["diffaug_fwd"] / gbps["axpby_fwd_bytes"], 3),
                      "bwd_rate_over_axpby": round(gbps["diffaug_bwd"] / gbps["axpby_bwd_bytes"], 3)}
    del x, g, xo, go, fns
    if a.kernels_only:
        print(json.dumps(out))
        return

    # ---- 2. a recorded Stage-I step without the keyword, with it, and without it again -----------------------------------
    gen = torch.Generator(device=dev).manual_seed(0)
    ds = DeviceDataset(torch.randint(0, 256, (N, S, S, 3), dtype=torch.uint8, device=dev, generator=gen))
    cfg = ArchConfig.px64()

    def make(augment):
        rng = DeviceRng(7, dev)
        feed = DeviceFeed(ds, B, 11, rng=rng, flip=True, max_shift=5)
        st = Stage1Step(cfg, dev, rng=rng, feed=feed, **({"augment": augment} if augment is not None else {}))
        st.load_recipe(1, True)
        return st

    run = {}
    for k, augment in (("without_keyword", None), ("augment", DiffAugment()), ("without_keyword_again", None)):
        st = make(augment)
        fn = st.capture()
        for _ in range(a.warmup):
            fn()
        run[k] = (st, fn)
    torch.cuda.synchronize()
    t = _windows({k: v[1] for k, v in run.items()}, a.steps, a.repeats)
    plain = t["without_keyword"]
    out["step_graph"] = {
        "ms_per_step": t,
        "augment_minus_without_us": round(1e3 * (t["augment"]["median"] - plain["median"]), 2),
        "again_minus_without_us": round(1e3 * (t["without_keyword_again"]["median"] - plain["median"]), 2),
        "spread_without_us": round(1e3 * (plain["max"] - plain["min"]), 2),
        "bytes_estimate_us": round((4 * 3 * B * S * S * 8 + 4 * 2 * 2 * B * S * S * 8)
                                   / (out["kernels"]["GBps"]["axpby_fwd_bytes"] * 1e9) * 1e6, 1),
        "losses_finite": all(bool(np.isfinite(v)) for k in run for v in run[k][0].logs().values())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
