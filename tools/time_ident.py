#!/usr/bin/env python3
"""Time n-way identification at the inference configuration (N = 64, 3 x 100 x 100): the engine's
fmri_hip.ident.objective_assessment for top 2 / 5 / 10 and ssim_matrix / pcc_matrix (HIP events around the call, which
ends in a device synchronise; warm-up first, median of repeats), against the CPU oracle (tests/ident_oracle.py, torch
with 16 threads) on the same data and draws, and against the reference's own per-comparison loop restated on the CPU
(two PearsonCorrelation and two StructuralSimilarity calls per draw, oracle/metrics_oracle.py).  Checks that the
engine's score equals the oracle's.  Prints one JSON line.

    python tools/time_ident.py [--n 64] [--px 100] [--reps 20] [--cpu-reps 3]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "thesis-fmri-reconstruction_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import ident_oracle as IO  # noqa: E402
from oracle import metrics_oracle as MO  # noqa: E402


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
    return statistics.median(ts), min(ts), max(ts)


def cpu_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def reference_loop(out, tgt, top):
    """The reference's per-comparison work (train_utils.py:791-807): PCC and SSIM of ground truth and distractor per draw."""
    tp = [0, 0]
    for idx in range(len(out)):
        numbers = [j for j in range(len(out)) if j != idx]
        sp = ss = 0
        for _ in range(top - 1):
            r = random.choice(numbers)
            sp += MO.pearson_correlation(out[idx], tgt[idx]) > MO.pearson_correlation(out[idx], tgt[r])
            a = out[idx:idx + 1]
            ss += MO.structural_similarity(a, tgt[idx:idx + 1])[0] > MO.structural_similarity(a, tgt[r:r + 1])[0]
        tp[0] += sp == top - 1
        tp[1] += ss == top - 1
    return tp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--px", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ident.py needs an MI355X")
    torch.set_num_threads(args.threads)
    from fmri_hip import ident
    pred, truth = IO.synth_batch(args.n, 3, args.px, args.px, 1234)
    pd = pred.cuda()
    loader = [truth]                       # host targets, moved to the device once per batch by the engine
    model = IO.StoredModel(loader, [pd])
    res = {"n": args.n, "px": args.px, "reps": args.reps, "cpu_threads": args.threads}
    td = truth.cuda()
    res["ssim_matrix_ms"] = gpu_ms(lambda: ident.ssim_matrix(pd, td), args.reps)
    res["pcc_matrix_ms"] = gpu_ms(lambda: ident.pcc_matrix(pd, td), args.reps)
    res["cpu_oracle_ssim_matrix_ms"] = cpu_ms(lambda: IO.ssim_matrix(pred, truth), args.cpu_reps)
    for top in (2, 5, 10):
        def engine():
            random.seed(top)
            return ident.objective_assessment(model, loader, top=top)
        res[f"objective_top{top}_ms"] = gpu_ms(engine, args.reps)

        def oracle():
            random.seed(top)
            return IO.objective_assessment([pred], [truth], top)[0]
        res[f"cpu_oracle_top{top}_ms"] = cpu_ms(oracle, args.cpu_reps)
        res[f"cpu_reference_loop_top{top}_ms"] = cpu_ms(lambda: reference_loop(pred, truth, top), 1)
        got, want = engine(), oracle()
        res[f"score_top{top}"] = got.tolist()
        assert torch.equal(got, want), (top, got, want)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
