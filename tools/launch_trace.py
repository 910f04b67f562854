"""What the host issues and what the steps compute, as hashes: compare two checkouts of a host-side refactor.

    python tools/launch_trace.py [--root CHECKOUT] > trace.txt        # one process; diff the files of two checkouts

Wraps ``fmri_hip.lib.call`` and records per launch the entry point, every argument ``lib._SIGS`` types as an integer or
a float (pointers only as null / non-null: addresses differ between runs) and the stream (0, 1, ... in order of first
appearance).  Under FMRI_DETERMINISTIC=1, with recipe weights and the oracle's synthetic batch (B = 4, 64 px, the voxel
counts of the ``*_b4`` goldens) it runs every step class and launch mode and prints per configuration the number of
launches, a SHA-256 of the trace and a SHA-256 of the state the steps left (scalar blocks, parameters, optimizer state).
Nothing is asserted about the hardware."""
import argparse
import ctypes
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.abspath(os.path.join(os.path.dirname(__file__), "..")),
                help="the checkout whose package, oracle and goldens are used (default: this one)")
ap.add_argument("--only", default="", help="run only the configurations whose name contains this")
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
os.environ["FMRI_DETERMINISTIC"] = "1"
for p in (ROOT, os.path.join(ROOT, "thesis-fmri-reconstruction_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fmri_hip import lib, ops  # noqa: E402
from fmri_hip.params import ArchConfig  # noqa: E402
from fmri_hip.steps import CognitiveStep, Stage1Step  # noqa: E402
from fmri_hip.wae_steps import DualStage1Step, WaeStep  # noqa: E402
from oracle import vaegan_oracle as O  # noqa: E402

DEV = "cuda:0"
B = 4
ops.set_deterministic(True)
TRACE, STREAMS = [], {}
_call = lib.call


def traced_call(name, *a):
    rec = [name]
    for t, v in zip(lib._SIGS[name], a):
        if t is ctypes.c_void_p:
            rec.append("-" if v is None or (isinstance(v, int) and v == 0) else "p")
        else:
            rec.append(repr(float(v)) if t is ctypes.c_float else repr(int(v)))
    rec.append("s%d" % STREAMS.setdefault(lib.stream(), len(STREAMS)))
    TRACE.append(" ".join(rec))
    _call(name, *a)


lib.call = traced_call


def golden_v(name):
    return int(np.load(os.path.join(ROOT, "tests", "golden", name))["meta/V"])


def state_hash(st):
    h = hashlib.sha256()
    tensors = [st.scal] + ([st.wscal] if hasattr(st, "wscal") else [])
    seen = set()
    for n in ("enc", "img_enc", "cog", "teacher_enc", "dec", "dis", "wd"):
        net = getattr(st, n, None)
        if net is not None and id(net) not in seen:
            seen.add(id(net))
            tensors.append(net.group.data)
    for n in ("opt_enc", "opt_dec", "opt_dis", "opt_wd"):
        o = getattr(st, n, None)
        if o is not None:
            tensors += [t for t in (o.s1, o.s2, o.lr_dev, o.t_dev) if t is not None]
    torch.cuda.synchronize()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def run(name, make, drive):
    """``make()`` -> step; ``drive(step)`` issues the launches that are traced."""
    if args.only not in name:
        return
    st = make()
    st.load_recipe(0, True)
    torch.cuda.synchronize()
    TRACE.clear()
    STREAMS.clear()
    drive(st)
    ops.join_side()
    n, th = len(TRACE), hashlib.sha256("\n".join(TRACE).encode()).hexdigest()
    print(f"{name:34s} launches {n:5d}  trace {th[:24]}  state {state_hash(st)[:24]}", flush=True)


def main():
    cfg_o, cfg = O.ArchCfg.px64(), ArchConfig.px64()
    V2, VW = golden_v("stage2_b4.npz"), golden_v("wae2_b4.npz")

    def batch(V=0):
        d = O.synth_batch(B, cfg_o, n_voxels=V, seed=1234, steps=1) if V else O.synth_batch(B, cfg_o, seed=1234, steps=1)
        nz = [d["noise"][0, i].to(DEV) for i in range(d["noise"].shape[1])]
        return d["x"].to(DEV), (d["fmri"].to(DEV) if V else None), nz

    x, _, nz = batch()
    eager = lambda *a, **k: (lambda st: [st.step(*a, **k) for _ in range(2)])

    def recorded(*a):
        def drive(st):
            replay = st.capture(*a)          # the trace holds the warm-up steps and the recording
            replay()
            replay()
        return drive

    def hybrid(st):
        step = st.capture_forward(x, nz[0], nz[1])
        step()
        step()

    for mode in ("vae-gan", "beta-vae", "dcgan", "vae"):
        run(f"stage1 {mode}", lambda: Stage1Step(cfg, DEV, mode=mode), eager(x, nz[0], nz[1]))
    xc, fm, nzc = batch(V2)
    for stage in (2, 3):
        for mode in ("vae-gan", "vae"):
            run(f"cognitive stage{stage} {mode}", lambda: CognitiveStep(cfg, V2, DEV, stage, mode=mode),
                eager(fm, xc, nzc[0], nzc[1], nzc[2]))
    xw, fw_, _ = batch(VW)
    for pen in ("gan", "mmd"):
        run(f"wae stage1 {pen}", lambda: WaeStep(cfg, DEV, 1, penalty=pen), eager(x, nz[2]))
        for stage in (2, 3):
            run(f"wae stage{stage} {pen}", lambda: WaeStep(cfg, DEV, stage, VW, penalty=pen), eager(xw, fmri=fw_))
    for mode in ("vae-gan", "beta-vae", "dcgan", "vae"):
        run(f"dual1 {mode}", lambda: DualStage1Step(cfg, DEV, mode=mode), eager(x, nz[0], nz[1], nz[2]))
    run("stage1 capture", lambda: Stage1Step(cfg, DEV), recorded(x, nz[0], nz[1]))
    run("wae stage1 capture", lambda: WaeStep(cfg, DEV, 1), recorded(x, nz[2]))
    run("stage1 capture_forward", lambda: Stage1Step(cfg, DEV), hybrid)

    # the collective path with one rank (FMRI_FORCE_DIST=1), last: the process group stays up until the end
    if "dist" in args.only or not args.only:
        import torch.distributed as dist
        os.environ["FMRI_FORCE_DIST"] = "1"
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29571")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        run("stage1 dist eager", lambda: Stage1Step(cfg, DEV, distributed=True), eager(x, nz[0], nz[1]))
        run("stage1 dist capture", lambda: Stage1Step(cfg, DEV, distributed=True), recorded(x, nz[0], nz[1]))
        torch.cuda.synchronize()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
