#!/usr/bin/env python3
"""GPU box: cost of the weight average (``ema=WeightEma(...)``, fmri_hip/ema.py) at Stage-I's real sizes: 64 x 64 px, z = 128.

1. One update launch over ALL shadowed segments of a step with the three networks shadowed (12 bytes per float: read w, e;
   write e) against one firing ``fmri_state_copy`` of the same step's state (8 bytes per float: read, write), alternately in
   one process with device events.  Both are pure streaming; reported as ms per call, GB/s and ns per MB moved.
2. End to end: a Stage-I step at ``--batch`` recorded with ``capture()`` -- fed, with ``rng=`` -- without the keyword, with
   the default networks (encoder + decoder) and with all three, timed alternately, ``repeats`` windows of ``steps`` replays.

Prints one JSON line.

usage: tools/ema_overhead.py [--batch 256] [--pool 50000] [--calls 100] [--steps 100] [--repeats 5] [--warmup 20]
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
    ap.add_argument("--pool", type=int, default=50000)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from fmri_hip.ema import WeightEma
    from fmri_hip.feed import DeviceDataset, DeviceFeed
    from fmri_hip.params import ArchConfig
    from fmri_hip.rng import DeviceRng
    from fmri_hip.state import StateRing
    from fmri_hip.steps import Stage1Step
    dev = torch.device("cuda:0")
    B, N, S = a.batch, a.pool, 64
    gen = torch.Generator(device=dev).manual_seed(0)
    ds = DeviceDataset(torch.randint(0, 256, (N, S, S, 3), dtype=torch.uint8, device=dev, generator=gen))
    cfg = ArchConfig.px64()
    ALL = ("encoder", "decoder", "discriminator")
    out = {"batch": B, "pool": N, "calls": a.calls, "steps": a.steps, "repeats": a.repeats}

    def make(nets, ring=None):
        g = DeviceRng(7, dev)
        feed = DeviceFeed(ds, B, 11, rng=g, flip=True, max_shift=5)
        kw = {}
        if nets is not None:
            kw["ema"] = WeightEma(nets=None if nets == "default" else nets)
        if ring is not None:
            kw["checkpoints"] = ring
        st = Stage1Step(cfg, dev, rng=g, feed=feed, **kw)
        st.load_recipe(1, True)
        return st

    # ---- 1. one update launch against one firing state copy ----------------------------------------------------------------
    ring = StateRing(capacity=1, every=1)
    st = make(ALL, ring)
    st.step()
    st.step()
    st.feed.set_position(1, 0)                      # the first batch of epoch 1: every launch from here fires into slot 0
    table = st.ema._all_table
    fns = {"ema_update": lambda: table.update(st.ema.state), "ema_swap": table.swap, "state_copy": ring.launch}
    for fn in fns.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    t = _windows(fns, a.calls, a.repeats)
    moved = {"ema_update": 12 * table.n, "ema_swap": 16 * table.n, "state_copy": 2 * ring.payload_bytes}
    out["launch"] = {
        "floats": table.n, "segments": len(table.pairs), "bytes_moved": moved, "ms_per_call": t,
        "GBps": {k: round(moved[k] / (t[k]["median"] * 1e-3) / 1e9, 1) for k in t},
        "ns_per_MB": {k: round(t[k]["median"] * 1e6 / (moved[k] / 1e6), 3) for k in t}}
    out["launch"]["update_over_copy_time_per_byte"] = round(out["launch"]["ns_per_MB"]["ema_update"]
                                                            / out["launch"]["ns_per_MB"]["state_copy"], 3)
    del st, ring, table, fns

    # ---- 2. a recorded Stage-I step without the keyword, with the default networks, with all three -----------------------------
    run = {}
    for k, nets in (("without_keyword", None), ("default_nets", "default"), ("all_three", ALL),
                    ("without_keyword_again", None)):
        st = make(nets)
        fn = st.capture()
        for _ in range(a.warmup):
            fn()
        run[k] = (st, fn)
    torch.cuda.synchronize()
    t = _windows({k: v[1] for k, v in run.items()}, a.steps, a.repeats)
    plain = t["without_keyword"]
    out["step_graph"] = {
        "ms_per_step": t,
        "shadowed_floats": {k: run[k][0].ema._all_table.n for k in ("default_nets", "all_three")},
        "default_minus_without_us": round(1e3 * (t["default_nets"]["median"] - plain["median"]), 2),
        "all_three_minus_without_us": round(1e3 * (t["all_three"]["median"] - plain["median"]), 2),
        "again_minus_without_us": round(1e3 * (t["without_keyword_again"]["median"] - plain["median"]), 2),
        "spread_without_us": round(1e3 * (plain["max"] - plain["min"]), 2),
        "losses_finite": all(bool(np.isfinite(v)) for k in run for v in run[k][0].logs().values())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
