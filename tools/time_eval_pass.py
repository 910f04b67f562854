#!/usr/bin/env python3
"""Time a validation pass of a Stage-I step (px64) on the device, two ways, alternating in one process:

  (a) fmri_hip.evaluate.Evaluator.run(): eval-mode forward -> fmri_image_metrics (two launches per batch) -> one ring row
  (b) the same eval-mode forward followed by the pieces the project had before: two nhwc_to_images, fmri_pcc, fmri_ssim
      (train.train_utils), a torch MSE -- once enqueue-only and once with the ``.item()`` per metric a host loop needs

HIP events around the pass (which ends in a device synchronise), warm-up first, median / min / max of the repeats; the
metrics of one batch alone the same way.  Kernel launches and memsets per batch of the metrics part are counted by a
torch profiler run of their own.  Prints one JSON line.

    python tools/time_eval_pass.py [--n 1024] [--batch 256] [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "thesis-fmri-reconstruction_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def gpu_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return [round(v, 4) for v in (statistics.median(ts), min(ts), max(ts))]


def device_ops(fn):
    """(kernel launches, memsets) ``fn`` puts on the device, from the profiler's device-side events."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
    except Exception as e:                       # (a build of torch without device tracing: the count is not measured)
        return f"not measured: {type(e).__name__}: {e}"
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    sets = [n for n in names if "memset" in n.lower()]
    return len(names) - len(sets), len(sets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_eval_pass.py needs an MI355X")
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.feed import DeviceDataset
    from fmri_hip.ops import nhwc_to_images
    from fmri_hip.params import ArchConfig
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import Stage1Step
    from train.train_utils import PearsonCorrelation, StructuralSimilarity
    dev = "cuda:0"
    step = Stage1Step(ArchConfig.px64(), dev)
    step.load_recipe(0, True)
    pool = torch.randint(0, 256, (args.n, 64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
    ev = Evaluator(step, DeviceDataset(pool), batch=args.batch, rng=DeviceRng(1, dev))
    pcc, ssim = PearsonCorrelation(), StructuralSimilarity()

    def pieces(pred16, x16, sync):
        a, b = nhwc_to_images(pred16, 3), nhwc_to_images(x16, 3)
        vals = pcc(a, b), ssim(a, b), torch.nn.functional.mse_loss(a, b)
        return [v.item() for v in vals] if sync else vals

    def old_pass(sync):
        bns = [bn for net in (ev.enc, ev.dec) for bn in net.all_bns()]
        for bn in bns:
            bn.eval_mode = True
        try:
            for r0, b in ev.ranges:
                pieces(*ev._forward(r0, b), sync)
        finally:
            for bn in bns:
                bn.eval_mode = False

    res = {"n": args.n, "batch": args.batch, "batches": len(ev.ranges), "reps": args.reps}
    # alternate the two ways twice: the spread between equal measurements is the noise
    for rnd in (0, 1):
        res[f"a_evaluator_pass_ms_{rnd}"] = gpu_ms(ev.run, args.reps)
        res[f"b_old_pieces_pass_ms_{rnd}"] = gpu_ms(lambda: old_pass(False), args.reps)
        res[f"b_old_pieces_pass_item_ms_{rnd}"] = gpu_ms(lambda: old_pass(True), args.reps)
    pred16, x16 = ev._pred16, ev._x16
    out7 = torch.zeros(7, dtype=torch.float32, device=dev)
    new_metrics = lambda: ev._metrics(pred16, x16, out7, ev._acc, 1)
    res["a_metrics_per_batch_ms"] = gpu_ms(new_metrics, args.reps)
    res["b_metrics_per_batch_ms"] = gpu_ms(lambda: pieces(pred16, x16, False), args.reps)
    res["a_metrics_launches_memsets_per_batch"] = device_ops(new_metrics)
    res["b_metrics_launches_memsets_per_batch"] = device_ops(lambda: pieces(pred16, x16, False))
    # the two ways agree on the last batch (fp32 single-pair kernels against the fp64 one: 4e-6)
    new_metrics()
    got, old = out7[:3].tolist(), pieces(pred16, x16, True)
    res["last_batch_new"], res["last_batch_old"] = got, old
    assert abs(got[0] - old[0]) < 4e-6 and abs(got[1] - old[1]) < 4e-6 and abs(got[2] - old[2]) < 1e-5 * old[2], (got, old)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
