"""Cost of the contrastive latent alignment on one MI355X (profiles/contrast.md):

    python tools/time_contrast.py [--out FILE]

(a) fmri_latent_nce at (n, d) = (256, 128) and (1024, 128), with and without dq, beside fmri_mmd_imq -- the kernel of the
    same structure -- at the same shapes, the four alternating in one process: device time per call from replays of a
    HIP graph that holds 50 calls (an eager call is bound by the host);
(b) a recorded WaeStep(stage=2) at B = 256, V = 4096 with and without contrast=, alternating, and a second plain step as
    the measure of the run-to-run spread.
Medians over 9 rounds of 20 replays, with the minimum and maximum of the rounds."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "thesis-fmri-reconstruction_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from fmri_hip.contrast import LatentContrast, latent_nce      # noqa: E402
from fmri_hip.mmd import mmd_imq                              # noqa: E402
from fmri_hip.params import ArchConfig                         # noqa: E402
from fmri_hip.wae_steps import WaeStep                         # noqa: E402

DEV = "cuda:0"
OUT = None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if OUT is not None:
        OUT.write(line + "\n")
        OUT.flush()


def graph_of(fn, calls):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    return g


def timed(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps          # ms per run


def alternate(variants, reps, rounds):
    """variants: name -> zero-argument run; returns name -> list of per-round ms."""
    for run in variants.values():
        timed(run, reps)                        # warm-up
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, run in variants.items():
            res[k].append(timed(run, reps))
    return res


def kernels():
    CALLS = 50
    for n, d in ((256, 128), (1024, 128)):
        g = torch.Generator().manual_seed(7 * n + d)
        t = (0.6 * torch.randn(n, d, generator=g) + 0.1).to(DEV)
        q = ((2.5 / d ** 0.5) * t.cpu() + 0.45 * torch.randn(n, d, generator=g) + 0.05).to(DEV)
        total = torch.zeros(1, device=DEV)
        top1 = torch.zeros(1, device=DEV)
        dq = torch.empty(n, d, device=DEV)
        fns = {
            "latent_nce +dq": lambda: latent_nce(q, t, 0.07, total=total, top1=top1, dq=dq),
            "latent_nce value": lambda: latent_nce(q, t, 0.07, total=total, top1=top1),
            "mmd_imq +dq": lambda: mmd_imq(q, t, 0.25, total=total, dq=dq),
            "mmd_imq value": lambda: mmd_imq(q, t, 0.25, total=total),
        }
        graphs = {k: graph_of(f, CALLS) for k, f in fns.items()}
        res = alternate({k: g.replay for k, g in graphs.items()}, reps=20, rounds=9)
        for k, v in res.items():
            us = [x * 1e3 / CALLS for x in v]
            say(f"kernel n={n} d={d} {k:18s}: median {statistics.median(us):7.2f} us/call  min {min(us):7.2f}  max "
                f"{max(us):7.2f}  (9 rounds x 20 replays of a {CALLS}-call graph)")


def steps():
    cfg, V, B = ArchConfig.px64(), 4096, 256
    rs = np.random.RandomState(11)
    x = torch.tanh(torch.from_numpy(rs.standard_normal((B, 3, 64, 64)).astype(np.float32))).to(DEV)
    fm = torch.from_numpy(rs.standard_normal((B, V)).astype(np.float32)).to(DEV)
    runs = {}
    keep = []
    for name, con in (("plain", None), ("contrast", LatentContrast(1.0, 0.07)), ("plain again", None)):
        st = WaeStep(cfg, DEV, 2, V, contrast=con)
        st.load_recipe(5, False)
        keep.append(st)
        runs[name] = st.capture(x, None, fm)
    res = alternate(runs, reps=20, rounds=9)
    med = {}
    for k, v in res.items():
        med[k] = statistics.median(v)
        say(f"recorded WaeStep(stage=2) B={B} V={V} {k:12s}: median {med[k]:.4f} ms/step  min {min(v):.4f}  max "
            f"{max(v):.4f}  (9 rounds x 20 replays)")
    say(f"difference contrast - plain: {1e3 * (med['contrast'] - med['plain']):.1f} us;  plain again - plain: "
        f"{1e3 * (med['plain again'] - med['plain']):.1f} us")
    say("logs with contrast:", keep[1].logs())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_contrast.py needs an MI355X: a timing without the device says nothing")
    if a.out:
        OUT = open(a.out, "w")
    kernels()
    steps()
    say("done")
