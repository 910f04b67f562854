#!/usr/bin/env python3
"""GPU box: cost of the device-resident dataset feed (``feed=DeviceFeed(...)``, fmri_hip/feed.py) at B = 256, 64 x 64 x 3,
a pool of 50 000 images.

1. The feed alone: ``feed.next()`` (indices + flips + shifts + gathering ingest + sampler advance + generator advance)
   against the composition it replaces, ``pool.index_select(0, idx)`` + ``ops.ingest_u8(..., want16=False, want32=True)``
   with precomputed indices, flips and shifts (the favourable case for the composition: it draws nothing).  Both are
   timed alternately in one process with device events: warm-up, then ``repeats`` windows of ``calls`` calls each.  The
   outputs of one batch are compared bit for bit first.  Algorithmic bytes of a batch: the uint8 images read once and
   the fp32 NCHW batch written once.
2. The opt-in end to end: a Stage-I step recorded with ``capture()`` -- with ``rng=`` and ``feed=``, and with ``rng=``
   and one static batch (bench.py's situation) -- timed alternately, ``repeats`` windows of ``steps`` replays.

Prints one JSON line.

usage: tools/feed_overhead.py [--batch 256] [--pool 50000] [--calls 200] [--steps 100] [--repeats 5] [--warmup 20]
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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from fmri_hip import lib, ops
    from fmri_hip.feed import DeviceDataset, DeviceFeed
    from fmri_hip.params import ArchConfig
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import Stage1Step
    lib.load()
    dev = torch.device("cuda:0")
    B, N, S = a.batch, a.pool, 64
    gen = torch.Generator(device=dev).manual_seed(0)
    pool = torch.randint(0, 256, (N, S, S, 3), dtype=torch.uint8, device=dev, generator=gen)
    ds = DeviceDataset(pool)
    out = {"batch": B, "pool": N, "calls": a.calls, "steps": a.steps, "repeats": a.repeats}

    # ---- 1. the feed alone against index_select + ingest_u8 ----------------------------------------------------------
    g = DeviceRng(7, dev)
    feed = DeviceFeed(ds, B, 11, rng=g, flip=True, max_shift=5)
    feed.next()
    idx, flip, shift = feed.idx.clone(), feed.flip.clone(), feed.shift.clone()
    idx64 = idx.long()

    def composed():
        return ops.ingest_u8(pool.index_select(0, idx64), flip=flip, shift=shift, want16=False, want32=True)[1]
    out["feed_equals_composition"] = bool(torch.equal(feed.x, composed()))
    fns = {"feed_next": feed.next, "index_select_ingest": composed}
    for fn in fns.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    t = _windows(fns, a.calls, a.repeats)
    nbytes = B * S * S * 3 * (1 + 4)
    out["feed"] = {"ms_per_call": t, "algorithmic_bytes": nbytes,
                   "feed_GBps": round(nbytes / (t["feed_next"]["median"] * 1e-3) / 1e9, 1),
                   "composition_GBps": round(nbytes / (t["index_select_ingest"]["median"] * 1e-3) / 1e9, 1),
                   "feed_minus_composition_ms": round(t["feed_next"]["median"] - t["index_select_ingest"]["median"], 5),
                   "clamped": feed.clamped()}

    # ---- 2. a recorded Stage-I step with and without the feed --------------------------------------------------------
    cfg = ArchConfig.px64()
    x = ops.ingest_u8(pool[:B].contiguous(), want16=False, want32=True)[1]
    run = {}
    for k in ("static_batch", "fed"):
        gk = DeviceRng(7, dev)
        fk = DeviceFeed(ds, B, 11, rng=gk, flip=True, max_shift=5) if k == "fed" else None
        st = Stage1Step(cfg, dev, rng=gk, feed=fk)
        st.load_recipe(1, True)
        fn = st.capture() if k == "fed" else st.capture(x)
        for _ in range(a.warmup):
            fn()
        run[k] = (st, fn, fk)
    torch.cuda.synchronize()
    t = _windows({k: v[1] for k, v in run.items()}, a.steps, a.repeats)
    finite = all(bool(np.isfinite(v)) for k in run for v in run[k][0].logs().values())
    out["step_graph"] = {"ms_per_step": t,
                         "fed_minus_static_ms": round(t["fed"]["median"] - t["static_batch"]["median"], 4),
                         "losses_finite": finite, "position": list(run["fed"][2].position()),
                         "clamped": run["fed"][2].clamped()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
