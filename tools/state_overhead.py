#!/usr/bin/env python3
"""GPU box: cost of the device-side training-state ring (``checkpoints=StateRing(...)``, fmri_hip/state.py) at Stage-I's
real state: 64 x 64 px, z = 128.

1. One FIRING snapshot launch (fmri_state_copy over the step's own segment table, the feed parked at the first batch of
   epoch 1) with the slot side plain and non-temporal (fmri_state_nontemporal), against ``torch.Tensor.copy_`` of ONE
   contiguous buffer of the same byte count -- the box's plain device-to-device rate -- and against the chain of
   per-tensor ``copy_`` calls over the same segments, the alternative the launch replaces.  Timed alternately in one
   process with device events: warm-up, then ``repeats`` windows of ``calls`` calls each.  GB/s counts the payload once.
   The gathered slot is compared with the live tensors byte for byte first.
2. The NON-firing launch end to end: a Stage-I step at ``--batch`` recorded with ``capture()`` -- fed, with ``rng=`` --
   with ``checkpoints=StateRing(2, every=5)`` and without the keyword, timed alternately, ``repeats`` windows of ``steps``
   replays.  The feed is parked behind the first batch of epoch 1, so no replay of the windows fires (checked: the ring
   stays empty).  A second step without the keyword, built last, shows what two identical step objects differ by.

Prints one JSON line.

usage: tools/state_overhead.py [--batch 256] [--pool 50000] [--calls 100] [--steps 100] [--repeats 5] [--warmup 20]
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
    ap.add_argument("--pool", type=int, default=50000)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from fmri_hip import lib
    from fmri_hip.feed import DeviceDataset, DeviceFeed
    from fmri_hip.params import ArchConfig
    from fmri_hip.rng import DeviceRng
    from fmri_hip.schedule import TrainLog
    from fmri_hip.state import StateRing
    from fmri_hip.steps import Stage1Step
    L = lib.load()
    dev = torch.device("cuda:0")
    B, N, S = a.batch, a.pool, 64
    gen = torch.Generator(device=dev).manual_seed(0)
    pool = torch.randint(0, 256, (N, S, S, 3), dtype=torch.uint8, device=dev, generator=gen)
    ds = DeviceDataset(pool)
    cfg = ArchConfig.px64()
    out = {"batch": B, "pool": N, "calls": a.calls, "steps": a.steps, "repeats": a.repeats}

    def make(ring):
        g = DeviceRng(7, dev)
        feed = DeviceFeed(ds, B, 11, rng=g, flip=True, max_shift=5)
        kw = {} if ring is None else {"checkpoints": ring}
        st = Stage1Step(cfg, dev, rng=g, feed=feed, log=TrainLog(4096), **kw)
        st.load_recipe(1, True)
        return st

    # ---- 1. one firing launch against copy_ ----------------------------------------------------------------------------
    ring = StateRing(capacity=1, every=1)
    st = make(ring)
    st.step()
    st.step()
    st.feed.set_position(1, 0)                      # the first batch of epoch 1: every launch from here fires into slot 0
    nbytes = ring.payload_bytes
    ring.launch()
    torch.cuda.synchronize()
    raw = ring.buf[:ring.slot_bytes]
    same = all(torch.equal(raw[s.offset:s.offset + s.nbytes], s.tensor.reshape(-1).view(torch.uint8))
               for s in ring.segments)
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)
    clones = [(torch.empty_like(s.tensor), s.tensor) for s in ring.segments]

    def policy(nt):
        def run():
            L.fmri_state_nontemporal(nt)
            ring.launch()
        return run

    def chain():
        for d, s in clones:
            d.copy_(s)
    fns = {"state_copy_plain": policy(0), "state_copy_nontemporal": policy(1), "copy_one_buffer": lambda: dst.copy_(src),
           "copy_per_tensor": chain}
    for fn in fns.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    t = _windows(fns, a.calls, a.repeats)
    L.fmri_state_nontemporal(1)                     # the library's default
    ref = t["copy_one_buffer"]
    bound = ref["max"] + (ref["max"] - ref["min"])
    out["snapshot"] = {
        "payload_bytes": nbytes, "segments": len(ring.segments), "slot_equals_live": bool(same), "ms_per_call": t,
        "GBps": {k: round(nbytes / (v["median"] * 1e-3) / 1e9, 1) for k, v in t.items()},
        "bound_ms": round(bound, 5),
        "within_bound": {k: bool(t[k]["median"] <= bound) for k in ("state_copy_plain", "state_copy_nontemporal")}}
    del st, ring, src, dst, clones

    # ---- 2. a recorded Stage-I step with the (non-firing) launch and without the keyword -------------------------------
    run = {}
    for k in ("without_keyword", "every_5", "without_keyword_again"):
        r = StateRing(capacity=2, every=5) if k == "every_5" else None
        st = make(r)
        fn = st.capture()
        st.feed.set_position(1, B)                  # behind the first batch of epoch 1: the next firing step is epoch 6's
        for _ in range(a.warmup):
            fn()
        run[k] = (st, fn, r)
    torch.cuda.synchronize()
    t = _windows({k: v[1] for k, v in run.items()}, a.steps, a.repeats)
    plain = t["without_keyword"]
    out["step_graph"] = {"ms_per_step": t,
                         "every_5_minus_without_us": round(1e3 * (t["every_5"]["median"] - plain["median"]), 2),
                         "spread_without_us": round(1e3 * (plain["max"] - plain["min"]), 2),
                         "again_minus_without_us": round(1e3 * (t["without_keyword_again"]["median"] - plain["median"]), 2),
                         "position": list(run["every_5"][0].feed.position()),
                         "slots_written": len(run["every_5"][2].states()),
                         "losses_finite": all(bool(np.isfinite(v)) for k in run for v in run[k][0].logs().values())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
