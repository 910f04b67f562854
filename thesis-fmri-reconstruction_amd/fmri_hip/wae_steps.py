"""Fused WAE training steps: our restatement of the inline loop bodies of the reference's WAE scripts.

    WaeStep(stage=1)   train/train_wae_stage1.py:259-311   image -> image, encoder + decoder + latent-D (Adam)
    WaeStep(stage=2)   train/train_wae_stage2.py:276-328   fMRI -> image, cognitive encoder + latent-D trained
    WaeStep(stage=3)   train/train_wae_stage3.py:297-347   fMRI -> image, decoder + latent-D trained
    DualStage1Step     train/wae_vgan_stage1.py:284-441    Stage-I VAE/GAN step + latent-D phase + latent penalty

Every script runs two phases per batch with an optimizer step in between:
  D phase  latent discriminator on "real" vs "fake" latents (both detached), two log-losses, one update;
  G phase  the generator side is run AGAIN (same weights -> same activations, so the engine runs it once and
           lets the train-mode BatchNorm layers take the matching number of running-stat updates), the UPDATED
           discriminator scores the latents, and reconstruction + penalty are back-propagated.
Nothing synchronises with the host inside a step; fp16 cotangents are kept in range with static scales and the
device-side unit-RMS re-normalisation of the encoder cotangent (same scheme as steps.py).

WaeStep(penalty="mmd") replaces the adversarial latent penalty with the IMQ-kernel MMD of the WAE paper (fmri_hip.mmd,
csrc/mmd.hip): no D phase, the latent discriminator is neither run nor updated; the generator-side forward passes (and
their BatchNorm running-statistic updates) stay those of the script.  The reference has no MMD step: this one is pinned
by the formula and by an oracle composed of the reference's encoder / decoder / Adam pieces (tests/mmd_oracle.py).
DualStage1Step keeps the adversarial penalty only.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import lib
from .nets import CognitiveEncoderNet, DecoderNet, EncoderNet, WaeDiscriminatorNet
from .contrast import N_MAX, LatentContrast, latent_nce
from .mmd import mmd_imq
from .ops import images_to_nhwc, nhwc_to_images, pad8, require_gpu, rows_to_f16
from .params import ArchConfig
from .rng import SID_EPS, SID_ZFAKE, SID_ZP, DeviceRng
from .step_base import S_NE, _Dist, _Optim, _StepBase
from .steps import LOG_KEYS, GanHyper, Scales, Stage1Step

_P = lib.ptr

# slots of the scalar block used by the WAE steps (sums over the global batch; [0, 4) are all-reduced)
W_REC, W_PEN, W_DFAKE, W_DREAL = 0, 1, 2, 3
W_LOG_KEYS = ("loss_reconstruction", "loss_penalty", "loss_discriminator_fake", "loss_discriminator_real")
# contrast= only: two of the block's free slots [26, 32), all-reduced with the four above (the slots between them are
# still zero at that point of a WAE step)
W_CON, W_TOP1 = 26, 27
W_CON_KEYS = ("loss_contrast", "latent_top1")


@dataclass
class WaeHyper:
    """Stage I: train/train_wae_stage1.py:221-224 (lr from configs/wae_config.py); Stage II/III: hard-coded
    train/train_wae_stage2.py:237-239."""
    lr_enc: float = 1e-4
    lr_dec: float = 1e-4
    lr_dis: float = 0.5e-4
    lam: float = 10.0
    betas: tuple = (0.5, 0.999)
    lam_mmd: float = 10.0          # penalty="mmd": weight of MMD_u (Stage I: lam_mmd * n * MMD_u, the sum convention)
    mmd_sigma2: float = 0.25       # penalty="mmd": IMQ bandwidth sigma^2, the variance of the Stage-I prior 0.5 * N(0, I)

    @staticmethod
    def stage23() -> "WaeHyper":
        return WaeHyper(lr_enc=1e-3, lr_dec=1e-3, lr_dis=5e-4)


class _LatentDiscPhase:
    """The latent-discriminator pieces shared by WaeStep and DualStage1Step."""

    def _dis_phase(self, wd: WaeDiscriminatorNet, opt: _Optim, z_real16, z_fake16, lam: float, scal, dd: _Dist):
        """D phase on detached latents: l_fake = -lam*sum log(d_fake+1e-3), l_real = -lam*sum log(1-d_real+1e-3)
        (e.g. train_wae_stage1.py:278-288); one forward over [real ; fake], gradients, optimizer step."""
        B = z_real16.shape[0]
        dev = z_real16.device
        zz = torch.cat([z_real16, z_fake16], 0)
        logit32, ctx = wd.forward(zz)
        dlogit = torch.empty(2 * B, 8, dtype=torch.float16, device=dev)
        lib.call("fmri_wae_logloss", _P(logit32[:B]), 1, B, 1, lam, _P(scal[W_DREAL:W_DREAL + 1]), None,
                 _P(dlogit[:B]), 8, 1.0)
        lib.call("fmri_wae_logloss", _P(logit32[B:]), 1, B, 0, lam, _P(scal[W_DFAKE:W_DFAKE + 1]), None,
                 _P(dlogit[B:]), 8, 1.0)
        wd.group.zero_grad()
        wd.backward(ctx, dlogit, 1.0, True, False)
        dd.all_reduce(wd.group.grad)
        opt.step()

    def _penalty(self, wd: WaeDiscriminatorNet, z16, w: float, gscale: float, scal, need_dz: bool):
        """G-phase penalty -w*sum log(d(z)+1e-3) with the updated discriminator; returns d penalty / d z (fp32,
        true scale) or None."""
        B = z16.shape[0]
        logit32, ctx = wd.forward(z16)
        dlogit = torch.empty(B, 8, dtype=torch.float16, device=z16.device) if need_dz else None
        lib.call("fmri_wae_logloss", _P(logit32), 1, B, 0, w, _P(scal[W_PEN:W_PEN + 1]), None, _P(dlogit), 8, gscale)
        if not need_dz:
            return None
        return wd.backward(ctx, dlogit, gscale, False, True)


class WaeStep(_LatentDiscPhase, _StepBase):
    """WAE/GAN Stage I / II / III step.

    ``penalty``: "gan" (default) the scripts' latent discriminator; "mmd" the IMQ-kernel MMD_u between the trained
    encoder's means q = head[:, :Z] (fp32) and the other side p -- Stage I the prior sample 0.5 * z_fake_noise, Stages
    II / III the Stage-I teacher's means -- with the statistic over the GLOBAL batch (data parallel: q and p gathered by
    one SUM all-reduce of a zero-padded buffer).  loss_penalty is lam_mmd * n * MMD_u in Stage I, lam_mmd * MMD_u in
    Stages II / III (the "sum" / "mean" conventions of the GAN penalty); Stage III logs it without back-propagating it;
    the two discriminator losses log 0.

    ``contrast``: a fmri_hip.contrast.LatentContrast (Stages II / III) adds weight * InfoNCE(q, t) (csrc/contrast.hip)
    between the cognitive means q = head[:, :Z] and the teacher's means t, beside either penalty: row i of the fMRI batch
    is told to retrieve row i of the image batch, which neither penalty says.  A batch mean over the GLOBAL batch (q and
    t gathered as for the MMD); Stage II back-propagates it into the cognitive encoder, Stage III logs it only.  The logs
    gain ``loss_contrast`` and ``latent_top1`` (the in-batch top-1 retrieval rate).  Without the keyword the step issues
    the launches and logs the four values it always did."""

    def __init__(self, cfg: ArchConfig, device, stage: int = 1, n_voxels: int = 0, hp: Optional[WaeHyper] = None,
                 scales: Optional[Scales] = None, distributed: bool = False, sync_bn: bool = True,
                 penalty: str = "gan", monitor: bool = False, rng: Optional[DeviceRng] = None, feed=None,
                 schedule=None, log=None, checkpoints=None, ema=None, fmri_augment=None,
                 contrast: Optional[LatentContrast] = None):
        """``fmri_augment``: a fmri_hip.voxaug.VoxelAugment in front of the cognitive encoder (Stages II / III, needs
        ``rng``; see steps.CognitiveStep); ``step(..., fmri_aug=table)`` pins the per-row parameters.
        ``ema``: a fmri_hip.ema.WeightEma (see steps.Stage1Step) over the networks this stage trains.
        ``checkpoints``: a fmri_hip.state.StateRing (see steps.Stage1Step); Adam's moments and step counts are state.
        ``monitor``: record the step's numerics on the device (``numerics()``, fmri_hip/monitor.py).
        ``schedule``: a fmri_hip.schedule.EpochSchedule (needs ``feed``) -- the scripts' three ``StepLR(step_size, gamma)``
        (train_wae_stage1.py:226-228, 334-336) on the device; all three optimizers follow it unless ``lr_mask`` says
        otherwise, and a margin / equilibrium / lambda_mse decay is a ValueError (a WAE step has none of them).
        ``log``: a fmri_hip.schedule.TrainLog (see steps.Stage1Step).
        ``rng``: a fmri_hip.rng.DeviceRng; Stage I's ``step(x)`` then draws ``z_fake_noise`` on the device (see
        steps.Stage1Step; Stages II / III take no noise).
        ``feed``: a fmri_hip.feed.DeviceFeed (Stages II / III: over a dataset with fMRI rows); ``step()`` then draws its
        batch itself (see steps.Stage1Step)."""
        assert stage in (1, 2, 3)
        if penalty not in ("gan", "mmd"):
            raise ValueError(f"WaeStep: penalty must be 'gan' or 'mmd', got {penalty!r}")
        if fmri_augment is not None and stage == 1:
            raise ValueError("WaeStep: fmri_augment= needs stage 2 or 3 (Stage I reads no fMRI rows)")
        if contrast is not None and stage == 1:
            raise ValueError("WaeStep: contrast= needs stage 2 or 3 (Stage I has no second modality to align with)")
        if contrast is not None and not isinstance(contrast, LatentContrast):
            raise ValueError(f"WaeStep: contrast must be a fmri_hip.contrast.LatentContrast, got {type(contrast).__name__}")
        if contrast is not None and (cfg.latent_dim % 64 or not 64 <= cfg.latent_dim <= 1024):
            raise ValueError(f"WaeStep: contrast= needs a latent size that is a multiple of 64, at most 1024 (csrc/contrast.hip); "
                             f"latent_dim is {cfg.latent_dim}")
        self.penalty, self.contrast = penalty, contrast
        self.cfg, self.stage, self.n_voxels = cfg, stage, n_voxels
        self.sc = Scales() if scales is None else scales
        self.hp = hp if hp is not None else (WaeHyper() if stage == 1 else WaeHyper.stage23())
        self.img_enc = EncoderNet(cfg, device)                       # Stage I: trained; II/III: Stage-I teacher
        self.cog = CognitiveEncoderNet(cfg, n_voxels, device) if stage > 1 else None
        self.dec = DecoderNet(cfg, device, self.img_enc.size)
        self.dec.fc_bn.enable_lazy_running()
        self.wd = WaeDiscriminatorNet(cfg, device)
        self._init_step(device, [n for n in (self.img_enc, self.cog, self.dec) if n is not None], distributed, sync_bn)
        self._pre_replay = [self.dec.fc_bn._running_in]
        hp_ = self.hp
        self.enc = self.img_enc if stage == 1 else self.cog          # the network `model.encoder` refers to
        self.opt_enc = _Optim(self.enc.group, "adam", hp_.lr_enc, betas=hp_.betas)
        self.opt_dec = _Optim(self.dec.group, "adam", hp_.lr_dec, betas=hp_.betas)
        self.opt_dis = _Optim(self.wd.group, "adam", hp_.lr_dis, betas=hp_.betas)
        self.optims = [self.opt_enc, self.opt_dec, self.opt_dis]
        if feed is not None and stage > 1 and (feed.fmri is None or feed.fmri.shape[1] != n_voxels):
            raise ValueError("WaeStep: feed needs a dataset with fp32 fMRI rows of n_voxels columns")
        self._init_rng(rng, feed)
        self._init_fmri_augment(fmri_augment)
        self._init_monitor(monitor, [("encoder", self.opt_enc, self.enc), ("decoder", self.opt_dec, self.dec),
                                     ("discriminator", self.opt_dis, self.wd)], 1)
        self._init_extras(schedule, log, checkpoints, ema)

    def _trained(self):
        """Stage II freezes the decoder, Stage III the cognitive encoder; the latent discriminator trains under the GAN
        penalty only."""
        on = {"encoder": self.stage != 3, "decoder": self.stage != 2, "discriminator": self.penalty == "gan"}
        return [n for n in super()._trained() if on[n]]

    # ---- parameters (the golden-fixture recipes of tests/golden/make_golden.py) --------------------------
    def load_recipe(self, seed: int, perturb: Optional[bool] = None):
        if self.stage == 1:
            rs = np.random.RandomState(seed)
            for n in (self.img_enc, self.dec, self.wd):
                n.group.load_recipe(rs, bool(perturb))
        else:
            rs = np.random.RandomState(seed)
            for n in (self.img_enc, self.dec):
                n.group.load_recipe(rs, True)
            self.cog.group.load_recipe(np.random.RandomState(seed + 100), True)
            self.wd.group.load_recipe(np.random.RandomState(seed + 200), True)

    def _state_groups(self):
        nets = [("encoder.", self.enc), ("decoder.", self.dec), ("discriminator.", self.wd)]
        if self.stage > 1:
            nets.append(("teacher_net.encoder.", self.img_enc))
        return nets

    # ---- the step --------------------------------------------------------------------------------------------
    def step(self, image: Optional[torch.Tensor] = None, z_fake_noise: Optional[torch.Tensor] = None,
             fmri: Optional[torch.Tensor] = None, fmri_aug: Optional[torch.Tensor] = None):
        """(``capture()`` records it whole: Adam's step count and the learning rates live on the device, and the ~300
        launches of a few microseconds each are bound by the host when issued eagerly.)
        Stage I: step(x, z_fake_noise) with z_fake = 0.5 * noise (train_wae_stage1.py:276); step(x) draws the noise
        with the step's ``rng``.  Stage II/III: step(image, fmri=fmri).  With a ``feed``: step() / step(None, noise).
        ``fmri_aug`` (steps with ``fmri_augment=``): the fp32 [B, 8] table of this step's fMRI augmentation; left out,
        the ``rng`` draws it."""
        st = self.stage
        fed = self._fed(image) if st == 1 else self._fed(image, fmri)
        fmri16 = None
        if fed is not None:
            image, fmri, fmri16 = fed
        require_gpu(image)
        cfg, hp, sc = self.cfg, self.hp, self.sc
        B, _, H, W = image.shape
        if self.contrast is not None and not 2 <= B * self.dd.world <= N_MAX:     # (before the step draws anything)
            raise ValueError(f"WaeStep: contrast= needs a global batch of 2 to {N_MAX} rows (in-batch negatives; "
                             f"csrc/contrast.hip), got {B} x {self.dd.world} ranks")
        with self.draws:                         # (Stages II / III draw no noise: the round is the feed's and the rows')
            if st == 1:
                z_fake_noise, = self._noise(B, ("z_fake_noise", SID_ZFAKE, z_fake_noise))
            else:
                _, rows16 = self._fmri_rows(fmri_aug, fmri)
                if rows16 is not None:
                    fmri16 = rows16
        Z, zp = cfg.latent_dim, pad8(cfg.latent_dim)
        dev = image.device
        Bg = B * self.dd.world
        self.scal.zero_()
        if self.mon is not None:
            self.mon.zero()
        x16 = images_to_nhwc(image)
        gan = self.penalty == "gan"

        def latent16(head32, rows=B):
            z16 = torch.empty(rows, zp, dtype=torch.float16, device=dev)
            lib.call("fmri_latent_fwd", _P(head32), None, rows, Z, zp, _P(z16), None, None, 0)     # z = mu
            return z16

        # ---- generator-side forwards (run once; BN running stats take the script's number of updates) ------
        if st == 1:
            head32, ectx = self.img_enc.forward(x16, updates=2)                       # :275 and :296
            z16 = latent16(head32)
            if gan:
                z_real16, z_fake16 = z16, rows_to_f16(z_fake_noise, 0.5)
            else:
                p32 = z_fake_noise.float() * 0.5                                      # :276
            y, dctx = self.dec.forward(z16, 1)                                        # :297
        else:
            head_t, _ = self.img_enc.forward(x16, updates=2 if st == 2 else 1)        # stage 2: :284,:293; 3: :312
            z_t16 = latent16(head_t) if gan or st == 2 else None
            head32, ectx = self.cog.forward(rows_to_f16(fmri) if fmri16 is None else fmri16, updates=2)             # :292,:314 / :311,:333
            z16 = latent16(head32)
            z_real16, z_fake16 = z_t16, z16
            p32 = head_t
            if st == 2:
                # decoder call order: x_gt = dec(z_teacher) (:285, unused, moves BN statistics), then x_recon
                yy, dctx = self.dec.forward(torch.cat([z_t16, z16], 0), 2, stat_order=(0, 1))
                y = yy[B:]
                g_rec = 1
            else:
                y, dctx = self.dec.forward(z16, 1)
        if st != 2:
            g_rec = 0

        # ---- D phase (GAN penalty only) --------------------------------------------------------------------------
        if gan:
            self._dis_phase(self.wd, self.opt_dis, z_real16, z_fake16, hp.lam, self.scal, self.dd)

        # ---- G phase ---------------------------------------------------------------------------------------------
        npix = B * H * W
        if st == 1:
            rec_w, rec_scale = 1.0, 1.0                                  # sum 0.5 (x~ - x)^2, d/dx~ = x~ - x
            pen_w, pen_scale = hp.lam, 1.0                               # -lam * sum log
        else:
            n_el = float(Bg * 3 * H * W)
            rec_w, rec_scale = 2.0 / n_el, n_el / 2.0                   # MSELoss(mean): (2/N) * 0.5 sum (.)^2
            pen_w, pen_scale = hp.lam / Bg, float(Bg)                    # -lam * mean log
        dxt = torch.empty(B, H, W, 8, dtype=torch.float16, device=dev)
        lib.call("fmri_pixel_sq", _P(x16), _P(y), npix, 3, 8, _P(self.scal[W_REC:W_REC + 1]), _P(dxt), 1.0)
        self.scal[W_REC:W_REC + 1].mul_(rec_w)
        train_enc = st != 3
        if gan:
            dz_pen = self._penalty(self.wd, z16, pen_w, pen_scale, self.scal, need_dz=train_enc)
        else:
            mmd_w = hp.lam_mmd * Bg if st == 1 else hp.lam_mmd
            rows = self._global_rows(head32, p32)
            dz_pen = self._mmd_penalty(rows, B, mmd_w, need_dz=train_enc)
        if self.contrast is not None:
            # (Stages II / III: the MMD's other side is the teacher's means too -- one gather serves both terms)
            dz_con = self._contrast_term(rows if not gan else self._global_rows(head32, head_t), B, need_dz=train_enc)
            if dz_con is not None:
                dz_pen = dz_pen[:, :Z] + dz_con
        self.dd.all_reduce(self.scal[:4] if self.contrast is None else self.scal[:W_TOP1 + 1])

        train_dec = st != 2
        if train_dec:
            self.dec.group.zero_grad()
        entries = [dict(g=g_rec, scale=rec_scale, train=train_dec, need_dz=train_enc)]
        dz_rec = self.dec.backward(dctx, dxt, entries)
        if train_dec:
            self.dd.all_reduce_async(self.dec.group.grad)           # runs under the encoder's backward pass
        if train_enc:
            dz = dz_rec[0] + dz_pen[:, :Z]
            dhead32 = torch.zeros(B, 2 * Z, dtype=torch.float32, device=dev)        # l_var gets no gradient
            dhead32[:, :Z] = dz
            dhead16 = self._renorm(dhead32, sc.enc, None, Bg)
            self.enc.group.zero_grad()
            self.enc.backward(ectx, dhead16, sc.enc)
            self.dd.all_reduce_async(self.enc.group.grad)
        self.dd.wait_all()
        if train_enc:
            self.opt_enc.step(gdev=self.scal[S_NE:S_NE + 1])
        if train_dec:
            self.opt_dec.step()
        self.fw = dict(B=B, y=y, x16=x16, head32=head32, Z=Z)      # (x16: what Evaluator.train_batch compares y with)
        if self.contrast is not None:
            self.fw["head_t"] = head_t
        if self.mon is not None:
            self.mon.tail(head32, Z, [self.scal[:len(W_LOG_KEYS)]], None)
        self._log_append()
        return self.scal

    def _global_rows(self, head32, other32):
        """(q, p): the first Z columns of this rank's two [B, >= Z] fp32 blocks over the GLOBAL batch -- views without data
        parallelism; with it every rank fills its slice of a zero buffer [2, n_global, Z] and one SUM all-reduce gathers
        both sides."""
        B, Z = head32.shape[0], self.cfg.latent_dim
        dd, rank = self.dd, self.dd.rank
        if not dd.on:
            return head32[:, :Z], other32[:, :Z]
        buf = torch.zeros(2, B * dd.world, Z, dtype=torch.float32, device=head32.device)
        buf[0, rank * B:(rank + 1) * B] = head32[:, :Z]
        buf[1, rank * B:(rank + 1) * B] = other32[:, :Z]
        dd.all_reduce(buf)
        return buf[0], buf[1]

    def _own_rows(self, dq, B: int):
        """This rank's rows of a gradient over the global batch (None stays None)."""
        if dq is None or not self.dd.on:
            return dq
        return dq[self.dd.rank * B:(self.dd.rank + 1) * B]

    def _mmd_penalty(self, rows, B: int, w: float, need_dz: bool):
        """w * MMD_u(q, p) into the penalty slot and, with need_dz, d/dq of it for this rank's B rows (fp32 [B, Z], true
        scale).  ``rows`` = _global_rows(head32, p32): q the trained encoder's means, p the other side, over the global
        batch -- every rank evaluates the same global statistic (only rank 0 adds it to the slot, which the loss
        all-reduce then sums) and keeps the gradient rows of its own samples."""
        q, p = rows
        dq = torch.empty(q.shape, dtype=torch.float32, device=q.device) if need_dz else None
        mmd_imq(q, p, self.hp.mmd_sigma2, w=w, total=self.scal[W_PEN:W_PEN + 1] if self.dd.rank == 0 else None, dq=dq)
        return self._own_rows(dq, B)

    def _contrast_term(self, rows, B: int, need_dz: bool):
        """weight * InfoNCE(q, t) into W_CON, the in-batch top-1 rate into W_TOP1 and, with need_dz, d/dq of the term for
        this rank's B rows (fp32 [B, Z], true scale).  ``rows`` = _global_rows(head32, head_t), as for _mmd_penalty: every
        rank evaluates the same statistic, only rank 0 adds the two values to the slots."""
        (q, t), con, first = rows, self.contrast, self.dd.rank == 0
        dq = torch.empty(q.shape, dtype=torch.float32, device=q.device) if need_dz else None
        latent_nce(q, t, con.temperature, con.symmetric, w=con.weight,
                   total=self.scal[W_CON:W_CON + 1] if first else None,
                   top1=self.scal[W_TOP1:W_TOP1 + 1] if first else None, dq=dq)
        return self._own_rows(dq, B)

    # ---- views for tests / API -----------------------------------------------------------------------------
    def _log_slots(self):
        slots = list(enumerate(W_LOG_KEYS))
        if self.contrast is not None:
            slots += [(W_CON, W_CON_KEYS[0]), (W_TOP1, W_CON_KEYS[1])]
        return slots

    def _log_columns(self):
        # (latent_top1 is a rate, not a loss)
        losses = W_LOG_KEYS if self.contrast is None else W_LOG_KEYS + W_CON_KEYS[:1]
        return [(k, self.scal, i) for i, k in self._log_slots()], losses

    def logs(self):
        v = self.scal.tolist()
        return {k: v[i] for i, k in self._log_slots()}

    def outputs(self):
        fw = self.fw
        out = dict(x_recon=nhwc_to_images(fw["y"], 3), z_real=fw["head32"][:, :fw["Z"]].clone())
        if "head_t" in fw:
            out["z_teacher"] = fw["head_t"][:, :fw["Z"]].clone()       # (contrast= only: the other side of the term)
        return out

    def named_grads(self):
        """True-scale gradients of the last step (syncs; tests only)."""
        ne = self.scal[S_NE].item()
        out = {}
        if self.penalty == "gan":
            for k, v in self.wd.group.grads.items():
                out["discriminator." + k] = v.clone()
        if self.stage != 3:
            for k, v in self.enc.group.grads.items():
                out["encoder." + k] = v / ne
        if self.stage != 2:
            for k, v in self.dec.group.grads.items():
                out["decoder." + k] = v.clone()
        return out


class DualStage1Step(Stage1Step, _LatentDiscPhase):
    """Dual WAE + VAE/GAN Stage-I step (train/wae_vgan_stage1.py:284-441; ``mode``: its four loss compositions,
    :311-364, as in Stage1Step -- 'vae-gan' default, 'beta-vae', 'dcgan' (the encoder is never stepped, :419), 'vae'):
    the Stage-I VAE/GAN step plus a WAE latent discriminator (RMSprop) trained on the encoder means, whose penalty
    gradient is added to the encoder's VAE/GAN gradient.  The encoder runs three times per batch in the script (one pass here, three
    running-stat updates) and the decoder three times (z, z_p, mu -- the last only moves BN statistics).

    ``torch14_zero_grad=True`` reproduces the pinned torch 1.4: the script's `optimizer_decoder.step()` at :417
    runs on zeroed gradients from the second iteration on, which only decays the decoder's RMSprop state."""

    def __init__(self, cfg: ArchConfig, device, hp: Optional[GanHyper] = None, scales: Optional[Scales] = None,
                 lam: float = 1.0, distributed: bool = False, sync_bn: bool = True, torch14_zero_grad: bool = True,
                 mode: str = "vae-gan", monitor: bool = False, rng: Optional[DeviceRng] = None, feed=None,
                 schedule=None, log=None, recon_level: int = 3, checkpoints=None, ema=None, augment=None):
        """``augment``: a fmri_hip.augment.DiffAugment in front of the IMAGE discriminator (see Stage1Step).
        ``ema``: a fmri_hip.ema.WeightEma (see Stage1Step); ``"wae_discriminator"`` names the latent discriminator.
        ``checkpoints``: a fmri_hip.state.StateRing (see Stage1Step).
        ``recon_level``: the script's ``--recon_level`` (wae_vgan_stage1.py:71,199), as in Stage1Step.
        ``rng``: a fmri_hip.rng.DeviceRng; ``step(x)`` then draws ``eps``, ``z_p`` and ``z_fake_noise`` on the device
        (see Stage1Step).  ``feed``: a fmri_hip.feed.DeviceFeed; ``step()`` then draws its batch itself (Stage1Step).
        ``schedule`` / ``log``: see Stage1Step.  By default the lr schedule covers what ``set_hyper(lr=)`` covers:
        encoder, decoder and image discriminator; the latent discriminator (registered fourth) keeps its rate.  The
        script itself rebinds ``lr_discriminator`` to the LATENT discriminator's scheduler (wae_vgan_stage1.py:246-250), so
        there the image discriminator's rate never decays and the latent discriminator's does:
        ``EpochSchedule(..., lr_mask=(True, True, False, True))`` reproduces that literally."""
        super().__init__(cfg, device, hp, scales, distributed, sync_bn, mode=mode, rng=rng, feed=feed,
                         recon_level=recon_level, augment=augment)
        hp = self.hp
        self.lam = lam
        self.torch14 = torch14_zero_grad
        self.wd = WaeDiscriminatorNet(cfg, device)
        self.opt_wd = _Optim(self.wd.group, "rmsprop", hp.lr, hp.alpha, hp.eps)
        self.optims.append(self.opt_wd)
        self.wscal = torch.zeros(8, dtype=torch.float32, device=device)
        self.enc_updates = 3
        self.extra_mu_decoder_pass = True
        self._it = 0
        self._init_monitor(monitor, [("encoder", self.opt_enc, self.enc), ("decoder", self.opt_dec, self.dec),
                                     ("discriminator", self.opt_dis, self.dis),
                                     ("wae_discriminator", self.opt_wd, self.wd)], 2)
        self._init_extras(schedule, log, checkpoints, ema)    # (the base constructor ran with none: ``optims`` was not complete)

    def _monitor_losses(self):
        return [self.scal[:len(LOG_KEYS)], self.wscal[:len(W_LOG_KEYS)]]

    def load_recipe(self, seed: int, perturb: bool = False):
        super().load_recipe(seed, perturb)
        self.wd.group.load_recipe(np.random.RandomState(seed + 200), perturb)

    def _state_groups(self):
        return super()._state_groups() + [("wae_discriminator.", self.wd)]

    def _host_state(self):
        """The iteration count behind ``torch14_zero_grad`` (it decides whether a step decays the decoder's RMSprop state
        first); a recorded step has it baked in as > 0."""
        return {"it": self._it}

    def _restored(self, host):
        super()._restored(host)
        self._it = int(host.get("it", self._it))

    def step(self, x=None, eps=None, z_p=None, z_fake_noise=None, aug=None):
        fed = self._fed(x)
        if fed is not None:
            x = fed[0]
        require_gpu(x)
        with self.draws:
            table = self._aug_table(aug, x.shape[0], x.shape[2])
            eps, z_p, z_fake_noise = self._noise(x.shape[0], ("eps", SID_EPS, eps), ("z_p", SID_ZP, z_p),
                                                 ("z_fake_noise", SID_ZFAKE, z_fake_noise))
        fw = self._forward(x, eps, z_p, table)
        self.gate(fw["B"] * self.dd.world)
        B, Z = fw["B"], self.cfg.latent_dim
        zp = pad8(Z)
        self.wscal.zero_()
        mu16 = torch.empty(B, zp, dtype=torch.float16, device=x.device)
        lib.call("fmri_latent_fwd", _P(fw["head32"]), None, B, Z, zp, _P(mu16), None, None, 0)
        self._dis_phase(self.wd, self.opt_wd, mu16, rows_to_f16(z_fake_noise, 0.5), self.lam, self.wscal, self.dd)
        dz_pen = self._penalty(self.wd, mu16, self.lam, 1.0, self.wscal, need_dz=True)
        self.dd.all_reduce(self.wscal[:4])
        if self.torch14 and self._it > 0:
            self.opt_dec.s1.mul_(self.hp.alpha)                       # :417 on zeroed grads: state decay only
        self._it += 1
        self.backward(extra_dmu=dz_pen)
        self.apply()
        self._log_append()
        return self.scal

    def _log_columns(self):
        cols, losses = super()._log_columns()
        extra = [("loss_penalty", self.wscal, W_PEN), ("loss_discriminator_fake", self.wscal, W_DFAKE),
                 ("loss_discriminator_real", self.wscal, W_DREAL)]
        return cols + extra, tuple(losses) + tuple(n for n, _, _ in extra)

    def logs(self):
        out = super().logs()
        v = self.wscal.tolist()
        out.update(loss_penalty=v[W_PEN], loss_discriminator_fake=v[W_DFAKE], loss_discriminator_real=v[W_DREAL])
        return out

    def named_grads(self):
        out = super().named_grads()
        for k, v in self.wd.group.grads.items():
            out["wae_discriminator." + k] = v.clone()
        return out
