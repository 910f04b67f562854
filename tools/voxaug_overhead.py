#!/usr/bin/env python3
"""GPU box: cost of the fMRI-row augmentation (``fmri_augment=VoxelAugment()``, fmri_hip/voxaug.py) at Stage II's real
sizes: B = 256 rows of V = 4096 voxels, 64 x 64 px, z = 128.

1. Kernel rate: ``fmri_voxaug_apply`` under a drawn table (noise and dropout on), under the neutral table (no draws:
   the memory side alone) and with noise only / dropout only, against ``fmri_rows_f32_to_f16`` on the same rows (the
   conversion it replaces: the same 4 B read + 2 B written per element) and against ``ops.axpby`` over the same number of
   bytes (the library's plain one-read-one-write pass).  A call takes a few microseconds, less than the host needs to
   issue it, so ``calls`` calls of each are recorded into a HIP graph and the replays are timed, alternately in one
   process with device events.  Reported as ms per call, GB/s and the ratios of the rates.
2. End to end: a Stage-II step at ``--batch`` recorded with ``capture()`` -- fed, with ``rng=`` -- without the keyword,
   with ``fmri_augment=VoxelAugment()`` and without it again, timed alternately, ``repeats`` windows of ``steps`` replays.

Prints one JSON line.

usage: tools/voxaug_overhead.py [--kernels-only] [--batch 256] [--voxels 4096] [--pool 4096] [--calls 100] [--steps 100] [--repeats 5] [--warmup 20]
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


def _graphed(fn, n):
    """``n`` calls of ``fn`` as one recorded chain; returns the replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            for _ in range(n):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    return graph.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--voxels", type=int, default=4096)
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true", help="part 1 only")
    a = ap.parse_args()
    from fmri_hip import lib, ops
    from fmri_hip.feed import DeviceDataset, DeviceFeed
    from fmri_hip.params import ArchConfig
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import CognitiveStep
    from fmri_hip.voxaug import VoxelAugment
    dev = torch.device("cuda:0")
    B, V, N, S = a.batch, a.voxels, a.pool, 64
    out = {"batch": B, "voxels": V, "pool": N, "calls": a.calls, "steps": a.steps, "repeats": a.repeats}

    # ---- 1. the apply kernel against the conversion it replaces and against axpby over the same bytes --------------------
    g = DeviceRng(3, dev)
    x = torch.randn(B, V, device=dev)
    y16 = torch.empty(B, ops.pad8(V), dtype=torch.float16, device=dev)
    tables = {"voxaug_apply": VoxelAugment().table(g, B, V),
              "voxaug_apply_neutral": VoxelAugment.neutral(B, dev),
              "voxaug_apply_noise_only": VoxelAugment(dropout=0.0).table(g, B, V),
              "voxaug_apply_dropout_only": VoxelAugment(noise=0.0).table(g, B, V)}
    nbytes = 6 * B * V                                             # 4 read + 2 written per element
    h = torch.empty(nbytes // 4, dtype=torch.float16, device=dev)   # axpby: 2 B read + 2 B written per fp16 element
    ho = torch.empty_like(h)
    P = lib.ptr
    fns = {k: (lambda t=t: VoxelAugment.apply(x, t, g, out16=y16)) for k, t in tables.items()}
    fns["rows_f32_to_f16"] = lambda: lib.call("fmri_rows_f32_to_f16", P(x), P(y16), B, V, ops.pad8(V), 1.0)
    fns["axpby_same_bytes"] = lambda: ops.axpby(h, None, 0.5, 0.0, out=ho)
    fns["voxaug_params"] = lambda: VoxelAugment().table(g, B, V, out=tables["voxaug_apply"])
    for fn in fns.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    replays = {k: _graphed(fn, a.calls) for k, fn in fns.items()}
    for r in replays.values():
        r()
    torch.cuda.synchronize()
    t = _windows(replays, 1, a.repeats)
    t = {k: {q: ([round(u / a.calls, 6) for u in v] if q == "all" else round(v / a.calls, 6)) for q, v in d.items()}
         for k, d in t.items()}
    gbps = {k: round(nbytes / (t[k]["median"] * 1e-3) / 1e9, 1) for k in t if k != "voxaug_params"}
    out["kernels"] = {"bytes_moved": nbytes, "ms_per_call": t, "GBps": gbps,
                      "apply_rate_over_rows_f32_to_f16": round(gbps["voxaug_apply"] / gbps["rows_f32_to_f16"], 3),
                      "apply_rate_over_axpby": round(gbps["voxaug_apply"] / gbps["axpby_same_bytes"], 3),
                      "neutral_rate_over_axpby": round(gbps["voxaug_apply_neutral"] / gbps["axpby_same_bytes"], 3)}
    del x, y16, h, ho, fns, replays
    if a.kernels_only:
        print(json.dumps(out))
        return

    # ---- 2. a recorded Stage-II step without the keyword, with it, and without it again ----------------------------------
    gen = torch.Generator(device=dev).manual_seed(0)
    ds = DeviceDataset(torch.randint(0, 256, (N, S, S, 3), dtype=torch.uint8, device=dev, generator=gen),
                       torch.randn(N, V, device=dev, generator=gen))
    cfg = ArchConfig.px64()

    def make(va):
        rng = DeviceRng(7, dev)
        feed = DeviceFeed(ds, B, 11, rng=rng, flip=True, max_shift=5)
        st = CognitiveStep(cfg, V, dev, 2, rng=rng, feed=feed, **({"fmri_augment": va} if va is not None else {}))
        st.load_recipe(3, True)
        return st

    run = {}
    for k, va in (("without_keyword", None), ("fmri_augment", VoxelAugment()), ("without_keyword_again", None)):
        st = make(va)
        fn = st.capture()
        for _ in range(a.warmup):
            fn()
        run[k] = (st, fn)
    torch.cuda.synchronize()
    t = _windows({k: v[1] for k, v in run.items()}, a.steps, a.repeats)
    plain = t["without_keyword"]
    out["step_graph"] = {
        "ms_per_step": t,
        "augment_minus_without_us": round(1e3 * (t["fmri_augment"]["median"] - plain["median"]), 2),
        "again_minus_without_us": round(1e3 * (t["without_keyword_again"]["median"] - plain["median"]), 2),
        "spread_without_us": round(1e3 * (plain["max"] - plain["min"]), 2),
        "bytes_estimate_us": round(nbytes / (out["kernels"]["GBps"]["axpby_same_bytes"] * 1e9) * 1e6, 2),
        "losses_finite": all(bool(np.isfinite(v)) for k in run for v in run[k][0].logs().values())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
