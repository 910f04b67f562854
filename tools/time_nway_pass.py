#!/usr/bin/env python3
"""Time n-way identification of one batch of 64 x 64 x 3 images on the device, two ways, alternating in one process:

  (a) one fmri_nway_scores (csrc/nway.hip) on the engine's fp16 [n, 64, 64, 8] tensors, persistent workspace and outputs
  (b) what a user of the fused steps could compose before it, on the same tensors: two nhwc_to_images, ident.pcc_matrix,
      ident.ssim_matrix and the torch counting of ident.n_way_expected up to, but not including, its ``.tolist()``

at n = 64 and n = 256, and a Stage-I validation pass (px64) over ``--n`` images with and without ``identify=5``.  HIP
events, warm-up first, median / min / max of the repeats; the two ways alternate twice, so the spread between equal
measurements shows the noise.  Kernel launches and memsets per call are counted by a torch profiler run of their own.
Prints one JSON line.

    python tools/time_nway_pass.py [--n 1024] [--batch 256] [--reps 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "thesis-fmri-reconstruction_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from time_eval_pass import device_ops, gpu_ms  # noqa: E402

TOP = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 256])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_nway_pass.py needs an MI355X")
    from fmri_hip import ident, lib
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.feed import DeviceDataset
    from fmri_hip.ops import nhwc_to_images
    from fmri_hip.params import ArchConfig
    from fmri_hip.rng import SID_DISTRACT, DeviceRng
    from fmri_hip.steps import Stage1Step
    dev = "cuda:0"
    P = lib.ptr
    res = {"reps": args.reps, "top": TOP}
    g = torch.Generator().manual_seed(0)
    for n in args.sizes:
        # correlated pairs, as reconstructions are: pred = a mix of its truth, another truth and noise
        truth = torch.rand(n, 3, 64, 64, generator=g) * 2 - 1
        pred = 0.5 * truth + 0.3 * truth.roll(1, 0) + 0.2 * (torch.rand(n, 3, 64, 64, generator=g) * 2 - 1)
        p16 = torch.zeros(n, 64, 64, 8, dtype=torch.float16)
        t16 = torch.zeros(n, 64, 64, 8, dtype=torch.float16)
        p16[..., :3], t16[..., :3] = pred.permute(0, 2, 3, 1).half(), truth.permute(0, 2, 3, 1).half()
        p16, t16 = p16.to(dev), t16.to(dev)
        rng = DeviceRng(1, dev)
        nb = lib.load().fmri_nway_ws_bytes(n, 64, 64)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        S = torch.empty(2, n, n, dtype=torch.float32, device=dev)
        d = torch.empty(n, TOP - 1, dtype=torch.int32, device=dev)
        out8 = torch.empty(8, dtype=torch.float32, device=dev)
        acc = torch.zeros(6, dtype=torch.float64, device=dev)

        def new():
            lib.call("fmri_nway_scores", P(p16), P(t16), n, 64, 64, 3, 8, TOP, P(rng._state), SID_DISTRACT, P(ws), nb,
                     P(S[0]), P(S[1]), P(d), P(out8), P(acc), 0)

        def old():
            a, b = nhwc_to_images(p16, 3), nhwc_to_images(t16, 3)
            return torch.stack([(M < M.diagonal()[:, None]).sum(1) for M in (ident.pcc_matrix(a, b),
                                                                             ident.ssim_matrix(a, b))])

        for rnd in (0, 1):
            res[f"n{n}_a_nway_scores_ms_{rnd}"] = gpu_ms(new, args.reps)
            res[f"n{n}_b_composition_ms_{rnd}"] = gpu_ms(old, args.reps)
        res[f"n{n}_a_launches_memsets"] = device_ops(new)
        res[f"n{n}_b_launches_memsets"] = device_ops(old)
        res[f"n{n}_ws_MiB"] = round(nb / 2 ** 20, 1)
        # the two ways count the same (both are within 2e-6 of fp64; a count differs only on a near-tie)
        new()
        cnt_new = torch.stack([(M < M.diagonal()[:, None]).sum(1) for M in (S[0], S[1])])
        res[f"n{n}_counts_differ"] = int((cnt_new != old()).sum().item())
        res[f"n{n}_max_abs_diff"] = [round((S[0] - ident.pcc_matrix(nhwc_to_images(p16, 3), nhwc_to_images(t16, 3)))
                                           .abs().max().item(), 9),
                                     round((S[1] - ident.ssim_matrix(nhwc_to_images(p16, 3), nhwc_to_images(t16, 3)))
                                           .abs().max().item(), 9)]
        res[f"n{n}_out8"] = [round(v, 6) for v in out8.tolist()]
        del ws

    step = Stage1Step(ArchConfig.px64(), dev)
    step.load_recipe(0, True)
    pool = torch.randint(0, 256, (args.n, 64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
    plain = Evaluator(step, DeviceDataset(pool), batch=args.batch, rng=DeviceRng(1, dev))
    identify = Evaluator(step, DeviceDataset(pool), batch=args.batch, rng=DeviceRng(1, dev), identify=TOP)
    res.update(pass_images=args.n, pass_batch=args.batch, pass_batches=len(plain.ranges))
    for rnd in (0, 1):
        res[f"pass_plain_ms_{rnd}"] = gpu_ms(plain.run, args.reps)
        res[f"pass_identify_ms_{rnd}"] = gpu_ms(identify.run, args.reps)
    res["pass_plain_launches_memsets"] = device_ops(plain.run)
    res["pass_identify_launches_memsets"] = device_ops(identify.run)
    h = identify.history()
    res["pass_columns"] = {k: float(h[k][-1]) for k in ("nway_PCC", "nway_SSIM", "nway_exp_PCC", "nway_exp_SSIM")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
