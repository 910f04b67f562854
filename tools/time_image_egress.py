#!/usr/bin/env python3
"""Time a validation pass of a Stage-I step (px64) with and without the on-device pictures (fmri_hip/egress.py), and the
host path they replace, in one process:

  plain        Evaluator(...).run()
  grids        ... grids=GridSink(): two grids (three launches each) on the last batch
  dump         ... dump=ImageDump(resize=200): two fmri_images_u8 per batch
  all          ... grids, dump and generate=100 (one more decoder forward of 100 rows and its grid)
  host         the plain pass, and per batch what a user did with last_output() / last_truth() before: both tensors to
               the host (a sync each), then per image F.interpolate(size=200), min / max, normalise, quantise with torch
               on the CPU, and the two grids of the last batch the same way (no file is written)

HIP events around the pass for the device variants, wall clock (the pass ends in a synchronise) for all of them;
warm-up first, median / min / max of the repeats, the variants alternating twice.  Kernel launches and memsets per pass
come from a torch profiler run of their own.  ``--root``: time the tree at that path instead (a checkout of the parent
commit has no fmri_hip.egress: only ``plain`` is measured there).  Prints one JSON line.

    python tools/time_image_egress.py [--n 1024] [--batch 256] [--reps 20] [--root PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--root", default=os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    for p in (root, os.path.join(root, "thesis-fmri-reconstruction_amd")):
        sys.path.insert(0, p)
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("time_image_egress.py needs an MI355X")
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.feed import DeviceDataset
    from fmri_hip.ops import nhwc_to_images
    from fmri_hip.params import ArchConfig
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import Stage1Step
    try:
        from fmri_hip.egress import GridSink, ImageDump
    except ImportError:
        GridSink = ImageDump = None
    dev = "cuda:0"
    step = Stage1Step(ArchConfig.px64(), dev)
    step.load_recipe(0, True)
    pool = torch.randint(0, 256, (args.n, 64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
    ds = DeviceDataset(pool)

    def measure(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ev_ms, wall_ms = [], []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            b.synchronize()
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            ev_ms.append(a.elapsed_time(b))
        r = lambda v: [round(x, 4) for x in (statistics.median(v), min(v), max(v))]
        return {"gpu_ms": r(ev_ms), "wall_ms": r(wall_ms)}

    def device_ops(fn):
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        try:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
        except Exception as e:
            return f"not measured: {type(e).__name__}: {e}"
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        sets = [n for n in names if "memset" in n.lower()]
        return len(names) - len(sets), len(sets)

    def make(**kw):
        return Evaluator(step, ds, batch=args.batch, rng=DeviceRng(1, dev), **kw)

    variants = {"plain": make()}
    if GridSink is not None:
        variants["grids"] = make(grids=GridSink(capacity=4))
        variants["dump"] = make(dump=ImageDump(resize=200))
        variants["all"] = make(grids=GridSink(capacity=4), dump=ImageDump(resize=200), generate=100)

    def u8(im):                                      # save_image(normalize=True) of one [1, 3, H, W] tensor, without the file
        lo, hi = float(im.min()), float(im.max())
        im = im.clone().clamp_(lo, hi).add_(-lo).div_(hi - lo + 1e-5)
        return im.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)

    def host_pass():
        ev = variants["plain"]
        bns = [bn for net in (ev.enc, ev.dec) for bn in net.all_bns()]
        for bn in bns:
            bn.eval_mode = True
        try:
            for r0, b in ev.ranges:
                pred16, x16 = ev._forward(r0, b)
                ev._metrics(pred16, x16, ev._bm[0], ev._acc, 0)
                for t in (nhwc_to_images(pred16, 3).cpu(), nhwc_to_images(x16, 3).cpu()):
                    for i in range(b):
                        u8(F.interpolate(t[i:i + 1], size=200))
            for t in (nhwc_to_images(pred16[:25], 3).cpu(), nhwc_to_images(x16[:25], 3).cpu()):
                u8(t)                                # the grid's range and bytes (the tiling itself is copies)
        finally:
            for bn in bns:
                bn.eval_mode = False

    res = {"root": os.path.relpath(root), "n": args.n, "batch": args.batch, "batches": len(variants["plain"].ranges),
           "reps": args.reps, "has_egress": GridSink is not None}
    for rnd in (0, 1):
        for name, ev in variants.items():
            res[f"{name}_{rnd}"] = measure(ev.run)
    for name, ev in variants.items():
        res[f"{name}_launches_memsets"] = device_ops(ev.run)
    if GridSink is not None:
        args.reps = max(3, args.reps // 4)
        res["host_path"] = measure(host_pass)
        ev = variants["all"]
        t0 = time.perf_counter()
        g, d = ev.grids.images(), ev.dump.images()
        res["readback_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        res["readback_MiB"] = round((sum(v.nbytes for v in g.values()) + sum(v.nbytes for v in d.values())) / 2 ** 20, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
