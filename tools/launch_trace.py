"""What the host issues and what the steps compute, as hashes: compare two checkouts of a host-side refactor.

    python tools/launch_trace.py [--root CHECKOUT] > trace.txt        # one process; diff the files of two checkouts

Wraps ``fmri_hip.lib.call`` and records per launch the entry point, every argument ``lib.prototype`` types as an integer or
a float (pointers only as null / non-null: addresses differ between runs) and the stream (0, 1, ... in order of first
appearance).  Under FMRI_DETERMINISTIC=1, with recipe weights and the oracle's synthetic batch (B = 4, 64 px, the voxel
counts of the ``*_b4`` goldens) it runs every step class and launch mode and prints per configuration the number of
launches, a SHA-256 of the trace and a SHA-256 of the state the steps left (scalar blocks, parameters, optimizer state,
the device state of the step's generator, of its feed and of a generator the feed has to itself).  The ``draws`` rows
are the steps that draw from a generator -- noise, a feed's flips and shifts, the augmentation tables, the fMRI rows --
eager and, where a recording is what training runs, as ``capture()`` + two replays.
It also runs recon_level 1 and 2, an eval-mode forward and the drop-in module API (one Stage-I loop body, lone
Encoder / Decoder blocks), hashing their outputs and parameter gradients in place of a state.
Nothing is asserted about the hardware."""
import argparse
import ctypes
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.abspath(os.path.join(os.path.dirname(__file__), "..")),
                help="the checkout whose package, oracle and goldens are used (default: this one)")
ap.add_argument("--only", default="", help="run only the configurations whose name contains one of these (comma-separated)")
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
    for t, v in zip(lib.prototype(name)[0], a):
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


def state_tensors(st):
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
    rng, feed = getattr(st, "rng", None), getattr(st, "feed", None)
    if rng is not None:
        tensors.append(rng._state)           # a wrong advance shows here even where the step's numbers agree
    if feed is not None:
        tensors.append(feed._state)
        if feed.rng is not None and feed.rng is not rng:
            tensors.append(feed.rng._state)
    return tensors


def tensors_hash(tensors):
    h = hashlib.sha256()
    torch.cuda.synchronize()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def run(name, make, drive):
    """``make()`` -> step or module; ``drive(it)`` issues the launches that are traced and returns the tensors to hash
    ("out"), or None for the state a step left ("state")."""
    if not any(s in name for s in args.only.split(",")):
        return
    st = make()
    if hasattr(st, "load_recipe"):
        st.load_recipe(0, True)
    torch.cuda.synchronize()
    TRACE.clear()
    STREAMS.clear()
    outs = drive(st)
    ops.join_side()
    n, th = len(TRACE), hashlib.sha256("\n".join(TRACE).encode()).hexdigest()
    what, hashed = ("state", state_tensors(st)) if outs is None else ("out", outs)
    print(f"{name:34s} launches {n:5d}  trace {th[:24]}  {what} {tensors_hash(hashed)[:24]}", flush=True)


def draws(cfg, x, nz, xc, fm, nzc, V2, xw, fmw, VW):
    """The steps that draw from a generator: everything that goes through the step's one advance per step."""
    from fmri_hip.augment import DiffAugment
    from fmri_hip.feed import DeviceDataset, DeviceFeed
    from fmri_hip.rng import DeviceRng
    from fmri_hip.voxaug import VoxelAugment
    rs = np.random.RandomState(7)
    pool = torch.from_numpy(rs.randint(0, 256, (16, 64, 64, 3), dtype=np.uint8)).to(DEV)
    rows = {V: torch.from_numpy(rs.standard_normal((16, V)).astype(np.float32)).to(DEV) for V in (V2, VW)}
    handed = DiffAugment().table(DeviceRng(9, DEV), B, 64)

    def rng():
        return DeviceRng(5, DEV)

    def fed(cls, *a, V=0, shared=True, **kw):
        """A step on a feed that flips and shifts on the step's generator, or on one of its own."""
        g = rng()
        ds = DeviceDataset(pool, rows[V] if V else None)
        return cls(cfg, *a, rng=g, feed=DeviceFeed(ds, B, 77, rng=g if shared else DeviceRng(6, DEV), flip=True,
                                                   max_shift=2), **kw)

    def both(name, make, *a):
        run(f"draws {name}", make, steps(*a))
        run(f"draws {name} capture", make, recorded(*a))

    both("stage1 rng", lambda: Stage1Step(cfg, DEV, rng=rng()), x)
    both("stage1 rng augment", lambda: Stage1Step(cfg, DEV, rng=rng(), augment=DiffAugment()), x)
    both("stage1 fed", lambda: fed(Stage1Step, DEV))
    run("draws stage1 fed own rng", lambda: fed(Stage1Step, DEV, shared=False), steps())
    both("cognitive stage2 fed all", lambda: fed(CognitiveStep, V2, DEV, 2, V=V2, augment=DiffAugment(),
                                                 fmri_augment=VoxelAugment()))
    run("draws cognitive stage3 handed aug", lambda: CognitiveStep(cfg, V2, DEV, 3, augment=DiffAugment()),
        steps(fm, xc, nzc[0], nzc[1], aug=handed))
    run("draws wae stage1 rng", lambda: WaeStep(cfg, DEV, 1, rng=rng()), steps(x))
    run("draws wae stage2 rng fmri_augment",
        lambda: WaeStep(cfg, DEV, 2, VW, rng=rng(), fmri_augment=VoxelAugment()), steps(xw, fmri=fmw))
    run("draws wae stage2 fed", lambda: fed(WaeStep, DEV, 2, VW, V=VW), steps())
    both("dual1 rng augment", lambda: DualStage1Step(cfg, DEV, rng=rng(), augment=DiffAugment()), x)


def steps(*a, **k):
    def drive(st):
        for _ in range(2):
            st.step(*a, **k)
    return drive


def recorded(*a):
    def drive(st):
        replay = st.capture(*a)          # the trace holds the warm-up steps and the recording
        replay()
        replay()
    return drive


def main():
    cfg_o, cfg = O.ArchCfg.px64(), ArchConfig.px64()
    V2, VW = golden_v("stage2_b4.npz"), golden_v("wae2_b4.npz")

    def batch(V=0):
        d = O.synth_batch(B, cfg_o, n_voxels=V, seed=1234, steps=1) if V else O.synth_batch(B, cfg_o, seed=1234, steps=1)
        nz = [d["noise"][0, i].to(DEV) for i in range(d["noise"].shape[1])]
        return d["x"].to(DEV), (d["fmri"].to(DEV) if V else None), nz

    x, _, nz = batch()

    eager = steps

    def hybrid(st):
        step = st.capture_forward(x, nz[0], nz[1])
        step()
        step()

    def eval_forward(st):
        """One forward with every BatchNorm in eval mode (the affine epilogue of the convolutions)."""
        for net in (st.enc, st.dec, st.dis):
            for bn in net.all_bns():
                bn.eval_mode = True
        fw = st.forward(x, nz[0], nz[1])
        return [fw[k] for k in ("head32", "disc_in", "feat", "logit32")] + [st.scal]

    # ---- the drop-in module API (models/vae_gan.py, imported as ``vg`` below): autograd bridges around the networks
    def vaegan(level):
        model = vg.VaeGan(device=DEV, z_size=128, recon_level=level).to(DEV)
        model.load_state_dict(O.fill_state(O.vaegan_spec(cfg_o), 0, True))
        return model

    def api_loop(model):
        """The Stage-I loop body (train_vgan_stage1.py) without the optimizers: forward, the three backward calls."""
        hp = O.GanHyper()
        model.train()
        z_p = nz[1].clone().requires_grad_(True)
        mus, lv = model.encoder(x)
        x_tilde = model.decoder(nz[0] * torch.exp(0.5 * lv) + mus)
        x_p = model.decoder(z_p)
        disc_layer = model.discriminator(x, x_tilde, x_p, "REC")
        disc_class = model.discriminator(x, x_tilde, x_p, "GAN")
        nle, kld, mse, bo, bp, bs = vg.VaeGan.loss(x, x_tilde, disc_layer[:B], disc_layer[B:-B], disc_layer[-B:],
                                                   disc_class[:B], disc_class[B:-B], disc_class[-B:], mus, lv)
        loss_encoder = torch.sum(kld) + torch.sum(mse)
        loss_discriminator = torch.sum(bo) + torch.sum(bp) + torch.sum(bs)
        loss_decoder = torch.sum(hp.lambda_mse * mse) - (1.0 - hp.lambda_mse) * loss_discriminator
        outs = [mus, lv, x_tilde, x_p, disc_layer, disc_class]
        model.zero_grad()
        for loss, part in ((loss_encoder, model.encoder), (loss_decoder, model.decoder),
                           (loss_discriminator, model.discriminator)):
            loss.backward(retain_graph=True)
            outs += [p.grad.clone() for p in part.parameters()]
            model.zero_grad()
        return outs

    def lone_block(kind):
        torch.manual_seed(3)
        blk = vg.EncoderBlock(64, 128) if kind == "enc" else vg.DecoderBlock(128, 64, out=True)
        return blk.to(DEV)

    def block_forward(kind, train):
        def drive(blk):
            blk.train(train)
            xb = torch.randn(3, 64 if kind == "enc" else 128, 12, 12, generator=torch.Generator().manual_seed(4))
            with torch.no_grad():
                got = blk(xb.half().float().to(DEV), True) if kind == "enc" else blk(xb.half().float().to(DEV))
            return list(got) if kind == "enc" else [got]
        return drive

    for mode in ("vae-gan", "beta-vae", "dcgan", "vae"):
        run(f"stage1 {mode}", lambda: Stage1Step(cfg, DEV, mode=mode), eager(x, nz[0], nz[1]))
    xc, fm, nzc = batch(V2)
    for stage in (2, 3):
        for mode in ("vae-gan", "vae"):
            run(f"cognitive stage{stage} {mode}", lambda: CognitiveStep(cfg, V2, DEV, stage, mode=mode),
                eager(fm, xc, nzc[0], nzc[1], nzc[2]))
    # fmri_augment=: the table and the apply launch in place of the fp32 -> fp16 conversion of the rows (new rows: the
    # rows above are the steps built without the keyword)
    from fmri_hip.rng import DeviceRng
    from fmri_hip.voxaug import VoxelAugment
    run("cognitive stage2 vae-gan fmri_augment",
        lambda: CognitiveStep(cfg, V2, DEV, 2, rng=DeviceRng(5, DEV), fmri_augment=VoxelAugment()),
        eager(fm, xc, nzc[0], nzc[1], nzc[2]))
    xw, fw_, _ = batch(VW)
    draws(cfg, x, nz, xc, fm, nzc, V2, xw, fw_, VW)
    for pen in ("gan", "mmd"):
        run(f"wae stage1 {pen}", lambda: WaeStep(cfg, DEV, 1, penalty=pen), eager(x, nz[2]))
        for stage in (2, 3):
            run(f"wae stage{stage} {pen}", lambda: WaeStep(cfg, DEV, stage, VW, penalty=pen), eager(xw, fmri=fw_))
    for mode in ("vae-gan", "beta-vae", "dcgan", "vae"):
        run(f"dual1 {mode}", lambda: DualStage1Step(cfg, DEV, mode=mode), eager(x, nz[0], nz[1], nz[2]))
    run("stage1 capture", lambda: Stage1Step(cfg, DEV), recorded(x, nz[0], nz[1]))
    run("wae stage1 capture", lambda: WaeStep(cfg, DEV, 1), recorded(x, nz[2]))
    run("stage1 capture_forward", lambda: Stage1Step(cfg, DEV), hybrid)

    # recon_level 1 / 2 (stream B joins the discriminator backward late), an eval-mode forward, the module API
    for level in (1, 2):
        run(f"stage1 vae-gan level{level}", lambda: Stage1Step(cfg, DEV, recon_level=level), eager(x, nz[0], nz[1]))
    run("stage1 dcgan level1", lambda: Stage1Step(cfg, DEV, mode="dcgan", recon_level=1), eager(x, nz[0], nz[1]))
    run("dual1 vae-gan level2", lambda: DualStage1Step(cfg, DEV, recon_level=2), eager(x, nz[0], nz[1], nz[2]))
    run("stage1 eval forward", lambda: Stage1Step(cfg, DEV), eval_forward)
    import configs.models_config as mc
    mc.use_px64()
    import models.vae_gan as vg
    for level in (3, 2):
        run(f"api stage1 loop level{level}", lambda: vaegan(level), api_loop)
    for kind in ("enc", "dec"):
        for train in (True, False):
            run(f"api lone {kind} block {'train' if train else 'eval'}", lambda: lone_block(kind),
                block_forward(kind, train))

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
