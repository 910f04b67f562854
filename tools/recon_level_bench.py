"""GPU box: what ``--recon_level`` 1 / 2 / 3 costs, as a plain timing script (bench.py is not involved).

    python tools/recon_level_bench.py [--out profiles/recon_level.md] [--api-root CHECKOUT]

Writes a Markdown file with
  * per level, B = 256 at 64 px: ms per step of the fused ``Stage1Step(recon_level=level)`` -- median of ``--repeats``
    windows of ``--steps`` steps, each window closed by a device synchronise -- and of the LITERAL Stage-I loop body on
    the drop-in modules (``VaeGan(recon_level=level)``, three ``backward()`` passes, three torch.optim steps: what a user
    of that option ran before the fused steps took it).  ``--api-root``: time that loop in a child process on another
    checkout (the parent commit), built there;
  * the loss head alone -- feature MSE forward + backward -- at F = 65 536 and 131 072, B = 256, through the per-sample
    entry points (fmri_feat_mse / fmri_feat_mse_bwd) and the chunked ones (fmri_feat_mse_wide / fmri_feat_mse_bwd_wide)
    on the same tensors in the same process, alternating, with fmri_set_deterministic off and on (device events).
Nothing is asserted; a path that finds no GPU fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
ap.add_argument("--out", default=None)
ap.add_argument("--api-root", default=None, help="checkout whose drop-in modules run the literal loop (default: --root)")
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--api-steps", type=int, default=50)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--only-api", type=int, default=0, help="(child) time the literal loop at this level, print one JSON line")
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
for p in (ROOT, os.path.join(ROOT, "thesis-fmri-reconstruction_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
B = args.batch
if not torch.cuda.is_available():
    raise SystemExit("recon_level_bench: needs the GPU")


def windows(step, n, repeats, warmup):
    """ms per step of ``repeats`` windows of ``n`` steps (host clock around work that ends in a synchronise)."""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / n)
    return out


def time_api(level):
    import configs.models_config as mc
    mc.use_px64()
    import models.vae_gan as vg
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.uniform(-1, 1, (B, 3, 64, 64)).astype(np.float32)).to(DEV)
    model = vg.VaeGan(device=DEV, z_size=128, recon_level=level).to(DEV)
    model.train()
    mk = lambda p: torch.optim.RMSprop(params=p, lr=1e-4, alpha=0.9, eps=1e-8, weight_decay=0, momentum=0,
                                       centered=False)
    oe, od, os_ = mk(model.encoder.parameters()), mk(model.decoder.parameters()), mk(model.discriminator.parameters())
    lam = 1e-6

    def step():                                     # train/train_vgan_stage1.py:330-432, mode 'vae-gan'
        x_tilde, disc_class, disc_layer, mus, lv = model(x)
        nle, kld, mse, bo, bp, bs = vg.VaeGan.loss(x, x_tilde, disc_layer[:B], disc_layer[B:-B], disc_layer[-B:],
                                                   disc_class[:B], disc_class[B:-B], disc_class[-B:], mus, lv)
        le = torch.sum(kld) + torch.sum(mse)
        ld = torch.sum(bo) + torch.sum(bp) + torch.sum(bs)
        lg = torch.sum(lam * mse) - (1.0 - lam) * ld
        model.zero_grad(); le.backward(retain_graph=True); oe.step()            # noqa: E702
        model.zero_grad(); lg.backward(retain_graph=True); od.step()            # noqa: E702
        model.discriminator.zero_grad(); ld.backward(); os_.step()              # noqa: E702
    return windows(step, args.api_steps, args.repeats, 15)


if args.only_api:
    print("API_JSON " + json.dumps(time_api(args.only_api)), flush=True)
    sys.exit(0)

from fmri_hip import lib, ops  # noqa: E402
from fmri_hip.params import ArchConfig  # noqa: E402
from fmri_hip.steps import Stage1Step  # noqa: E402

_P = lib.ptr


def time_fused(level):
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.uniform(-1, 1, (B, 3, 64, 64)).astype(np.float32)).to(DEV)
    e, z = (torch.from_numpy(rs.standard_normal((B, 128)).astype(np.float32)).to(DEV) for _ in range(2))
    st = Stage1Step(ArchConfig.px64(), DEV, recon_level=level)
    st.load_recipe(0, False)
    out = windows(lambda: st.step(x, e, z), args.steps, args.repeats, 10)
    ops.join_side()
    logs = st.logs()
    del st
    torch.cuda.empty_cache()
    return out, logs


def api_times(level):
    if args.api_root is None:
        return time_api(level)
    cmd = [sys.executable, os.path.abspath(__file__), "--root", os.path.abspath(args.api_root), "--only-api", str(level),
           "--batch", str(B), "--api-steps", str(args.api_steps), "--repeats", str(args.repeats)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    for line in r.stdout.splitlines():
        if line.startswith("API_JSON "):
            return json.loads(line[len("API_JSON "):])
    raise RuntimeError("literal loop on " + args.api_root + " failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])


def time_head(F, iters=20, repeats=5):
    """us per (forward + backward) of the loss head, old and new entry points alternating on the same tensors."""
    g = torch.Generator(device=DEV).manual_seed(F)
    feat = torch.randn(3 * B, F, generator=g, device=DEV, dtype=torch.float32).half()
    dfeat = torch.empty_like(feat)
    total = torch.zeros(1, dtype=torch.float32, device=DEV)
    norm = torch.ones(1, dtype=torch.float32, device=DEV)
    n = int(lib.load().fmri_feat_mse_wide_ws_floats(B, F))
    ws = torch.empty(n, dtype=torch.float32, device=DEV)

    def old():
        lib.call("fmri_feat_mse", _P(feat), B, F, None, _P(total))
        lib.call("fmri_feat_mse_bwd", _P(feat), B, F, _P(dfeat), 16.0, _P(norm))

    def new(zero_rows):
        lib.call("fmri_feat_mse_wide", _P(feat), B, F, None, _P(total), _P(ws), n)
        lib.call("fmri_feat_mse_bwd_wide", _P(feat), B, F, _P(dfeat), 16.0, _P(norm), zero_rows)
    variants = [("per-sample kernels", old), ("chunked kernels, zero rows written", lambda: new(1)),
                ("chunked kernels, zero rows skipped", lambda: new(0))]
    res = {}
    for det in (False, True):
        was = ops.set_deterministic(det)
        try:
            for _, fn in variants:
                fn()
            torch.cuda.synchronize()
            acc = {name: [] for name, _ in variants}
            for _ in range(repeats):
                for name, fn in variants:                   # alternating: every repeat visits every variant
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    acc[name].append(1e3 * e0.elapsed_time(e1) / iters)
            res[det] = {k: (statistics.median(v), min(v), max(v)) for k, v in acc.items()}
        finally:
            ops.set_deterministic(was)
    return res


def main():
    lines = ["# `--recon_level` 1 / 2 / 3: fused step, module-API loop, loss head", "",
             f"`python tools/recon_level_bench.py` on {torch.cuda.get_device_name(0)}; B = {B}, 64 px.  Step times: median "
             f"(min .. max) of {args.repeats} windows, each closed by a device synchronise; {args.steps} steps per window "
             f"for the fused step, {args.api_steps} for the literal loop.  Nothing else ran in the process.", ""]
    lines += ["## Step", "",
              "| recon_level | F per image | fused `Stage1Step`, ms / step | literal loop on the drop-in modules, ms / step | ratio |",
              "|---|---|---|---|---|"]
    fmt = lambda v: f"{statistics.median(v):.2f} ({min(v):.2f} .. {max(v):.2f})"
    for level in (1, 2, 3):
        fused, logs = time_fused(level)
        api = api_times(level)
        F = {1: 131072, 2: 65536, 3: 16384}[level]
        lines.append(f"| {level} | {F} | {fmt(fused)} | {fmt(api)} | "
                     f"{statistics.median(api) / statistics.median(fused):.2f} x |")
        print(lines[-1], "| last mse", logs["mse"], flush=True)
    where = ("this checkout" if args.api_root is None else
             "a checkout of the parent commit, built there, in a child process of the same call")
    lines += ["", f"The literal loop (`VaeGan(recon_level=level)`, three `backward()` passes, three `torch.optim.RMSprop` steps: "
              f"train_vgan_stage1.py:330-432) ran on {where}.", ""]
    lines += ["## Loss head alone (feature MSE forward + backward), B = 256", "",
              "Device events around 20 calls of forward + backward, median (min .. max) of 5 repeats, variants "
              "alternating inside each repeat, same tensors, same process.", "",
              "| F | deterministic | variant | us / (forward + backward) |", "|---|---|---|---|"]
    verdict = []
    for F in (65536, 131072):
        res = time_head(F)
        for det in (False, True):
            for name, (med, lo, hi) in res[det].items():
                lines.append(f"| {F} | {'on' if det else 'off'} | {name} | {med:.1f} ({lo:.1f} .. {hi:.1f}) |")
                print(lines[-1], flush=True)
            old = res[det]["per-sample kernels"][0]
            new = res[det]["chunked kernels, zero rows written"][0]
            skip = res[det]["chunked kernels, zero rows skipped"][0]
            word = "equal within the spread" if abs(new / old - 1) < 0.02 else ("chunked faster" if new < old else
                                                                                 "chunked NOT faster")
            verdict.append(f"* F = {F}, deterministic {'on' if det else 'off'}: chunked / per-sample = {new / old:.2f} like "
                           f"for like (zero rows written): {word}; {skip / old:.2f} as the step calls it (zero rows "
                           f"skipped).")
    lines += [""] + verdict + [""]
    text = "\n".join(lines)
    print(text)
    out = args.out or os.path.join(ROOT, "profiles", "recon_level.md")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
