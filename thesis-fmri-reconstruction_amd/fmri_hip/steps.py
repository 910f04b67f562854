"""Fused training steps: our restatement of the inline loop bodies of the reference scripts.

    Stage1Step   train/train_vgan_stage1.py:316-432   (mode 'vae-gan')
    Stage2Step   train/train_vgan_stage2.py:321-407
    Stage3Step   train/train_vgan_stage3.py:324-411
    (WAE Stage I/II/III and the Dual WAE+VAE/GAN step live in wae_steps.py; what every step is built on -- the
     optimizers, the data-parallel glue and its graph-segment recorder, noise / feed / capture -- in step_base.py)

Contract: one forward -> the three gradient sets, each of its own loss w.r.t. its own
sub-network, all evaluated at the pre-update weights -> gated optimizer steps.  The discriminator is run
once (REC+GAN fused, BN running stats updated twice like the reference); its backward carries two
cotangent streams (A = d L_dis, B = d sum(mse)) so that decoder gets lambda*B-(1-lambda)*A and the
encoder gets B (+KL) from a single saved forward.  Nothing in a step synchronises with the host: the
equilibrium gate is evaluated on the device and gates the fused optimizer kernels through a flag, and the
fp16 cotangent streams are normalised by device-side factors (see csrc/loss.hip) that the optimizer
kernels divide out again.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import lib, ops
from .nets import (CognitiveEncoderNet, DecoderNet, DiscriminatorNet, EncoderNet, WaeDiscriminatorNet,
                   refresh_net)
from .ops import axpby, images_to_nhwc, nhwc_to_images, pad8, require_gpu, rows_to_f16
from .params import ArchConfig
from .rng import SID_EPS, SID_EPS_TEACHER, SID_ZP, DeviceRng
from .step_base import (S_BCE_O, S_BCE_P, S_BCE_S, S_KL, S_MSE, S_NLE, S_LENC, S_LDIS, S_LDEC, S_DL2, S_NA, S_NB,  # noqa: F401
                        S_RATIO, S_ONE, S_ESQ, S_NE, S_NP, S_C1, S_C2, S_C3, S_GDEC, S_KLW, S_ZMAX, _attach_reducers,
                        _Dist, _host_copy, _Optim, _SegmentRecorder, _small_group, _SMALL_GROUP, _StepBase)

_P = lib.ptr

# loss compositions of train/train_vgan_stage1.py:359-388 (csrc/loss.hip enum Mode)
MODES = {"vae-gan": 0, "beta-vae": 1, "dcgan": 2, "vae": 3}
N_REDUCED = 10      # slots [0, N_REDUCED) are sums over the batch -> all-reduced in data-parallel runs
LOG_KEYS = ("bce_orig", "bce_pred", "bce_samp", "kl", "mse", "nle", "loss_encoder", "loss_discriminator",
            "loss_decoder")


@dataclass
class GanHyper:
    """configs/gan_config.py:19-31."""
    lr: float = 1e-4
    lambda_mse: float = 1e-6
    margin: float = 0.35
    equilibrium: float = 0.68
    alpha: float = 0.9
    eps: float = 1e-8
    beta: float = 1.0      # KL factor of mode 'beta-vae' (configs/gan_config.py:32)


@dataclass
class Scales:
    """Static power-of-two factors on top of the device-side unit-RMS normalisation of each cotangent
    stream (stored = true * norm * scale): they centre the streams inside fp16's normal range."""
    a: float = 512.0       # d L_dis stream through the discriminator (starts at unit RMS per logit)
    b: float = 16.0        # d sum(mse) stream through discriminator / decoder (unit RMS per feature)
    dec: float = 2048.0    # lambda*B - (1-lambda)*A through the decoder (carries norm nA)
    enc: float = 16.0      # encoder backward (carries norm nB)
    p: float = 16.0        # d nle / d x_tilde through the decoder (mode 'vae'; carries norm nP)


class _GanStepBase(_StepBase):
    """The VAE/GAN pieces of the Stage-I/II/III steps: hyper-parameters, loss kernels, gate, starting cotangents,
    logging."""

    def _init_common(self, device, hp, scales, distributed, sync_bn, nets):
        self._init_step(device, nets, distributed, sync_bn)
        # fresh instances: GanHyper / Scales are mutable (the per-epoch decays are written as step.set_hyper(...))
        self.hp = GanHyper() if hp is None else hp
        self.sc = Scales() if scales is None else scales
        self.mode = "vae-gan"
        # [lambda_mse, equilibrium, margin, beta] on the device: read by the gate kernel, so a recorded step follows
        # the per-epoch decays (train_vgan_stage1.py:451-458)
        self.hp_dev = torch.tensor([self.hp.lambda_mse, self.hp.equilibrium, self.hp.margin, self.hp.beta],
                                   dtype=torch.float32, device=device)
        self.flags = torch.zeros(2, dtype=torch.int32, device=device)
        # per decoder call group: the power of two its latent rows are stored scaled by (ops.latent_ranged); the groups
        # fed with caller noise keep 1
        self.zs = torch.ones(4, dtype=torch.float32, device=device)

    def _latent(self, head32, eps, z16_rows, group: int, kl_slot: Optional[int]):
        """z = eps * sigma + mu of decoder call group ``group`` into ``z16_rows``, range-safe (ops.latent_ranged): the
        rows are stored at the power-of-two scale self.zs[group]; with SyncBN the decoder's batch is the global one, so
        the range is the global maximum."""
        B, Z = head32.shape[0], head32.shape[1] // 2
        ops.latent_ranged(head32, eps, B, Z, z16_rows, self._slot(S_ZMAX + group), self.zs[group:group + 1],
                          kl_total=None if kl_slot is None else self._slot(kl_slot), sample=True,
                          max_reduce=self.dd.all_reduce_max if (self.dd.on and self.dd.sync_bn) else None)

    def set_hyper(self, lr: Optional[float] = None, lambda_mse: Optional[float] = None,
                  equilibrium: Optional[float] = None, margin: Optional[float] = None, beta: Optional[float] = None):
        """The epoch-end updates of the scripts (lr_*.step(), margin *= decay_margin, equilibrium *= decay_equilibrium,
        lambda_mse *= decay_mse; train_vgan_stage1.py:448-458) -- host copies and the device values the kernels read.
        A step built with ``schedule=`` makes those updates itself, on the device: lr / lambda_mse / equilibrium / margin
        then belong to the schedule (RuntimeError) and ``self.hp`` keeps the BASE values the schedule started from
        (``schedule.values()`` has the current ones); ``beta`` is not scheduled and is set as ever."""
        hp = self.hp
        if self.schedule is not None:
            owned = [n for n, v in (("lr", lr), ("lambda_mse", lambda_mse), ("equilibrium", equilibrium),
                                    ("margin", margin)) if v is not None]
            if owned:
                raise RuntimeError(f"set_hyper({', '.join(owned)}): owned by the step's EpochSchedule")
            if beta is not None:
                hp.beta = float(beta)
                self.hp_dev[3:4].fill_(hp.beta)
            return
        if lr is not None:
            hp.lr = float(lr)
            # encoder, decoder, discriminator: the Dual step's latent discriminator (registered fourth) keeps its rate
            for o in self.optims[:3]:
                o.set_lr(lr)
        for name, v in (("lambda_mse", lambda_mse), ("equilibrium", equilibrium), ("margin", margin), ("beta", beta)):
            if v is not None:
                setattr(hp, name, float(v))
        self.hp_dev.copy_(torch.tensor([hp.lambda_mse, hp.equilibrium, hp.margin, hp.beta], dtype=torch.float32))

    def _discriminate(self, disc_in, B, table):
        """The discriminator's forward pass on the 3B images ``[orig | pred | sampled]`` -- with ``augment=`` on their
        transforms under ``table`` (``_aug_table``; ``disc_in`` itself stays what it is for the pixel term and the
        views).  Returns (feat, logit32, ctx, what ``fw`` notes about the augmentation)."""
        if self.augment is None:
            return (*self.dis.forward(disc_in), {})
        disc_aug = self.augment.forward(disc_in, table, B)
        return (*self.dis.forward(disc_aug), dict(disc_aug=disc_aug, aug=table))

    def _gan_losses(self, feat, logit32, B, x16, xt16, H, W):
        """BCE / feature-mse / pixel terms of VaeGan.loss into the scalar block (+ all-reduce)."""
        dev = feat.device
        F = feat[0].numel()
        prob = torch.empty(3 * B, dtype=torch.float32, device=dev)
        lib.call("fmri_gan_head_parts", _P(logit32), 1, B, _P(prob), _P(self.scal), self._dis_parts())
        if self.dis.level == 3:
            lib.call("fmri_feat_mse", _P(feat), B, F, None, _P(self._slot(S_MSE)))
        else:
            # recon_level 1 / 2: rows of 131 072 / 65 536 halves at 64 px -- the chunked head (csrc/featloss.hip)
            n = lib.load().fmri_feat_mse_wide_ws_floats(B, F)
            ws = torch.empty(n, dtype=torch.float32, device=dev)
            lib.call("fmri_feat_mse_wide", _P(feat), B, F, None, _P(self._slot(S_MSE)), _P(ws), n)
        lib.call("fmri_pixel_sq", _P(x16), _P(xt16), B * H * W, 3, 8, _P(self._slot(S_NLE)), None, 1.0)
        if not getattr(self, "_defer_loss_reduce", False):
            self.dd.all_reduce(self.scal[:N_REDUCED])
        return prob, F

    def _dis_parts(self) -> int:
        """Terms of the back-propagated discriminator loss: orig | pred | sampled ('dcgan' / 'vae': orig + sampled)."""
        return 5 if self.mode in ("dcgan", "vae") else 7

    def _gate(self, B_global, F, gate_on=True, force_dis=-1, force_dec=-1):
        fw = self.fw
        lib.call("fmri_compose_gate_dev", _P(self.scal), _P(self.flags), float(B_global), float(F),
                 float(3 * fw["H"] * fw["W"]), _P(self.hp_dev), MODES[self.mode], 1 if gate_on else 0, force_dis,
                 force_dec)

    def _gate_flag(self, i: int):
        """The equilibrium gate's device flag i (0 = discriminator, 1 = decoder) as the condition of a sub-network's
        weight gradients (ops.begin_grads), or None when ``gate_skip`` is off."""
        return self.flags[i:i + 1] if self.gate_skip else None

    def _logit_cotangent(self, B):
        """fp16 starting cotangent of stream A: d L_dis / d logits of the last forward, S_NA <- its norm factor."""
        logit32 = self.fw["logit32"]
        dlogit16 = torch.empty(3 * B, 8, dtype=torch.float16, device=logit32.device)
        lib.call("fmri_gan_head_bwd_parts", _P(logit32), 1, B, _P(dlogit16), 8, self.sc.a, _P(self._slot(S_NA)),
                 self._dis_parts())
        return dlogit16

    def _start_cotangents(self, B):
        """fp16 starting cotangents of stream A (logits) and stream B (the raw features of discriminator block
        ``recon_level``: shapes are taken from ``fw["feat"]``), and what ``DiscriminatorNet.backward`` may know about the
        latter (its ``stack`` / ``zero_tail`` arguments)."""
        feat = self.fw["feat"]
        dev = feat.device
        dlogit16 = self._logit_cotangent(B)
        # stream B's cotangent is written straight into the second half of the buffer that stacks both streams for the
        # discriminator's conv backward (DiscriminatorNet fills the first half with stream A: no concatenation copy)
        stack = torch.empty((2 * feat.shape[0],) + tuple(feat.shape[1:]), dtype=feat.dtype, device=dev)
        dfeat16 = stack[feat.shape[0]:]
        if self.dis.level == 3:
            lib.call("fmri_feat_mse_bwd", _P(feat), B, feat[0].numel(), _P(dfeat16), self.sc.b, _P(self._slot(S_NB)))
        else:
            # the sampled images' zero rows are written only if the join layer's data gradient reads them
            lib.call("fmri_feat_mse_bwd_wide", _P(feat), B, feat[0].numel(), _P(dfeat16), self.sc.b,
                     _P(self._slot(S_NB)), 1 if self.dis.reads_zero_tail() else 0)
        # (zero_tail: the rows of the sampled images are exact zeros)
        return dlogit16, dfeat16, dict(stack=stack, zero_tail=B)

    def _encoder_cotangent(self, dz, norm_slot: int, kl_dev=None, extra_dmu=None):
        """Decoder-side dz (carried at the device factor of ``norm_slot``: S_NB or S_NP) -> the encoder's fp16 head
        cotangent: dz and the KL term (device weight ``kl_dev``, default the slot's factor) through the
        reparameterisation, ``extra_dmu`` (fp32 [B, z], true scale) added on the means at the same factor, then the
        unit-RMS re-normalisation (S_NE <- factor * nE)."""
        fw = self.fw
        B, Z = fw["B"], self.cfg.latent_dim
        norm = self._slot(norm_slot)
        dhead32 = torch.empty(B, 2 * Z, dtype=torch.float32, device=dz.device)
        lib.call("fmri_latent_bwd", _P(fw["head32"]), _P(fw["eps"]), _P(dz), Z, 1.0, 1.0,
                 _P(norm if kl_dev is None else kl_dev), B, Z, 1.0, None, _P(dhead32), 1)
        if extra_dmu is not None:
            dhead32[:, :Z].addcmul_(extra_dmu, norm)
        return self._renorm(dhead32, self.sc.enc, norm, B * self.dd.world)

    def _log_columns(self):
        cols = [(k, self.scal, i) for i, k in enumerate(LOG_KEYS)]
        return cols + [("train_dis", self.flags, 0), ("train_dec", self.flags, 1)], LOG_KEYS

    def _init_extras(self, schedule, log, checkpoints=None, ema=None):
        """lr: encoder, decoder, discriminator, as ``set_hyper``."""
        super()._init_extras(schedule, log, checkpoints, ema, [i < 3 for i in range(len(self.optims))], self.hp,
                             self.hp_dev)

    def _state_tensors(self):
        out = super()._state_tensors()
        out["hp"] = self.hp_dev
        return out

    def _restored(self, host):
        """``self.hp`` follows the restored device block -- under a schedule only ``beta``: the rest keeps the BASE values
        the schedule started from (``set_hyper``)."""
        super()._restored(host)
        hp, v = self.hp, self.hp_dev.tolist()
        hp.beta = _host_copy(hp.beta, v[3])
        if self.schedule is None:
            hp.lambda_mse, hp.equilibrium, hp.margin = (_host_copy(h, d) for h, d in
                                                         zip((hp.lambda_mse, hp.equilibrium, hp.margin), v))
            hp.lr = self.optims[0].lr

    def logs(self):
        v = self.scal.tolist()
        out = {k: v[i] for i, k in enumerate(LOG_KEYS)}
        f = self.flags.tolist()
        out["train_dis"], out["train_dec"] = bool(f[0]), bool(f[1])
        return out

    def _monitor_tail(self):
        if self.mon is not None:
            self.mon.tail(self.fw["head32"], self.cfg.latent_dim, self._monitor_losses(), self.zs)

    def _monitor_losses(self):
        return [self.scal[:len(LOG_KEYS)]]

    # ---- reference-shaped views of the last forward (API / parity tests) -----------------------------
    outputs_gt_x = False         # whether ``outputs()`` has the ground-truth image (the steps that are not handed it as x)

    def outputs(self):
        fw, cfg = self.fw, self.cfg
        B, Z = fw["B"], cfg.latent_dim
        d = fw["disc_in"]
        feat = fw["feat"]
        n3, h, w, c = feat.shape
        out = dict(gt_x=nhwc_to_images(d[:B], 3)) if self.outputs_gt_x else {}
        out.update(
            x_tilde=nhwc_to_images(d[B:2 * B], 3), x_p=nhwc_to_images(d[2 * B:], 3),
            disc_class=fw["prob"].reshape(3 * B, 1).clone(),
            disc_layer=nhwc_to_images(feat, c).reshape(n3, -1),
            mus=fw["head32"][:, :Z].clone(), log_variances=fw["head32"][:, Z:].clone())
        return out

    def named_grads(self):
        """True-scale gradients (the device normalisation factors divided out) of the sub-networks the step trains --
        syncs; tests/API only.  After ``backward()``; ``step()`` does not leave any (FlatGroup.check_grads_readable)."""
        s = self.scal.tolist()
        out = {}
        for pre, n, slot in self._subnets():
            if slot is None:
                continue
            n.group.check_grads_readable()
            for k, v in n.group.grads.items():
                out[pre + k] = v / s[slot]
        return out


class Stage1Step(_GanStepBase):
    """Stage-I VAE/GAN step (image -> image)."""

    def __init__(self, cfg: ArchConfig, device, hp: Optional[GanHyper] = None, scales: Optional[Scales] = None,
                 distributed: bool = False, sync_bn: bool = True, mode: str = "vae-gan", gate_skip: bool = True,
                 monitor: bool = False, rng: Optional[DeviceRng] = None, feed=None, schedule=None, log=None,
                 recon_level: int = 3, checkpoints=None, ema=None, augment=None):
        """``augment``: a fmri_hip.augment.DiffAugment; every image the discriminator sees -- orig, pred and sampled -- then
        goes through one random colour / translation / cutout transform (one launch in front of the discriminator's
        forward pass), and the image cotangents that come back out of the discriminator go through its adjoint (one
        launch) before anything reads them.  The pixel ``nle`` term, ``outputs()``, the evaluator and the grids keep the
        un-augmented images.  The per-image parameters follow the noise convention: a table passed as
        ``step(..., aug=table)`` is used as it is; left out, it is drawn by the step's ``rng`` at the offset of the noise
        draws (ValueError without one), recorded steps draw a fresh one at every replay; ``last_augment()`` reads it.
        None: nothing is added.
        ``ema``: a fmri_hip.ema.WeightEma; the step then keeps an exponential moving average of the weights and BatchNorm
        statistics of the networks it names (default: the trained ones the eval forward uses) on the device -- one launch
        behind every optimizer update, two at the end of the step, recorded steps included; ``ema_state_dict()`` reads it,
        ``Evaluator(..., weights="ema")`` evaluates with it.  None: nothing is added.
        ``checkpoints``: a fmri_hip.state.StateRing; with its ``every`` set, one predicated launch behind
        ``fmri_epoch_begin`` keeps the whole training state of the epochs the scripts save (``idx_epoch % every == 0``) in a
        device ring, recorded steps included; ``snapshot()`` takes the state now, ``ring.states()`` reads the ring with
        one sync and ``restore(state)`` continues a run bit for bit (fmri_hip/state.py).  None: nothing is added.
        ``recon_level`` (1, 2 or 3; the scripts' ``--recon_level``, train_vgan_stage1.py:62,237): the discriminator
        block whose raw convolution output is the feature tensor of the ``mse`` term.  The parameters, and so
        ``state_dict()``, are the same at every level.  Below 3 the feature cotangent joins the logit cotangent below the
        top block (DiscriminatorNet.backward) and the loss head runs on the chunked kernels of csrc/featloss.hip; 3 (the
        default) issues the launches it always did.
        ``monitor``: record the step's numerics on the device (``numerics()``, fmri_hip/monitor.py).
        ``schedule``: a fmri_hip.schedule.EpochSchedule (needs ``feed``); the epoch-end block of the scripts -- lr decay,
        margin / equilibrium / lambda_mse decays with their clamps -- then happens on the device, as the first launch of
        the step whose batch opens a new epoch, recorded steps included; ``self.hp`` keeps the base values.
        ``log``: a fmri_hip.schedule.TrainLog; the last launch of every step then appends what ``logs()`` would return, the
        batch's epoch and the learning rates to a device ring -- ``history()`` / ``epoch_means()`` read it with one sync.
        ``rng``: a fmri_hip.rng.DeviceRng; ``step(x)`` then draws ``eps`` and ``z_p`` on the device (``last_noise()``)
        and a step recorded with ``capture(x)`` draws fresh noise at every replay.  Noise passed to ``step`` is used as
        it is, with or without ``rng``.
        ``feed``: a fmri_hip.feed.DeviceFeed; ``step()`` then takes no batch -- the feed draws the next shuffled,
        augmented batch of its device-resident dataset as the step's first launches -- and ``capture()`` records a step
        that replays whole epochs with no host work (a batch passed to such a step is a ValueError, as is none passed
        to a step without a feed).
        ``mode``: the loss composition of train_vgan_stage1.py:359-388 -- 'vae-gan' (default), 'beta-vae' (KL weight
        hp.beta / batch), 'dcgan' (pixel nle, encoder not trained), 'vae' (pixel nle, discriminator not trained unless
        the gate re-arms both).  ``gate_skip``: in ``step`` the weight-gradient GEMMs of the decoder / discriminator are
        conditioned on the equilibrium gate's device flags (fmri_wgrad_if) -- a sub-network the gate does not train in a
        step gets no gradients, as in the reference (`if train_dec: loss_decoder.backward()`,
        train_vgan_stage1.py:420-431); False: they always run and only the update is conditional."""
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}")
        self.cfg = cfg
        self.gate_skip = bool(gate_skip)
        self.enc = EncoderNet(cfg, device)
        self.dec = DecoderNet(cfg, device, self.enc.size)
        self.dec.fc_bn.enable_lazy_running()
        self.dis = DiscriminatorNet(cfg, device, recon_level)
        self._init_common(device, hp, scales, distributed, sync_bn, (self.enc, self.dec, self.dis))
        self._pre_replay = [self.dec.fc_bn._running_in]      # reloads after an outside write of the buffers only
        self._init_rng(rng, feed)
        self._init_augment(augment)
        self.mode = mode
        hp = self.hp
        self.opt_enc = _Optim(self.enc.group, "rmsprop", hp.lr, hp.alpha, hp.eps)
        self.opt_dec = _Optim(self.dec.group, "rmsprop", hp.lr, hp.alpha, hp.eps)
        self.opt_dis = _Optim(self.dis.group, "rmsprop", hp.lr, hp.alpha, hp.eps)
        self.optims = [self.opt_enc, self.opt_dec, self.opt_dis]
        self.enc_updates = 1                 # encoder passes per batch in the script (BN running-stat updates)
        self.extra_mu_decoder_pass = False   # DualStage1Step (wae_steps.py)
        self._init_monitor(monitor, [("encoder", self.opt_enc, self.enc), ("decoder", self.opt_dec, self.dec),
                                     ("discriminator", self.opt_dis, self.dis)], 1)
        self._init_extras(schedule, log, checkpoints, ema)

    # ---- parameters -----------------------------------------------------------------------------
    def _subnets(self):
        """(state-dict prefix, network, slot of the device factor its gradients carry) per sub-network."""
        return (("encoder.", self.enc, S_NE), ("decoder.", self.dec, S_GDEC), ("discriminator.", self.dis, S_NA))

    def _trained(self):
        """'dcgan' never steps the encoder (``apply``)."""
        return [n for n in super()._trained() if not (n == "encoder" and self.mode == "dcgan")]

    def load_recipe(self, seed: int, perturb: bool = False):
        rs = np.random.RandomState(seed)
        for _, n, _ in self._subnets():
            n.group.load_recipe(rs, perturb)

    def _state_groups(self):
        return [(pre, n) for pre, n, _ in self._subnets()]

    def load_state_dict(self, sd):
        for pre, n, _ in self._subnets():
            n.group.load_state_dict(sd, pre)

    # ---- the step ---------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, eps: Optional[torch.Tensor] = None, z_p: Optional[torch.Tensor] = None,
                aug: Optional[torch.Tensor] = None):
        require_gpu(x)
        B, _, H, W = x.shape
        with self.draws:
            table = self._aug_table(aug, B, H)
            eps, z_p = self._noise(B, ("eps", SID_EPS, eps), ("z_p", SID_ZP, z_p))
        return self._forward(x, eps, z_p, table)

    def _forward(self, x, eps, z_p, table):
        """The launches of ``forward`` behind the draws: on noise that is there and the augmentation table of
        ``_aug_table`` (DualStage1Step.step draws a third noise input in the same round and enters here)."""
        cfg = self.cfg
        B, _, H, W = x.shape
        Z, zp = cfg.latent_dim, pad8(cfg.latent_dim)
        dev = x.device
        self.scal.zero_()
        if self.mon is not None:
            self.mon.zero()
        # decoder groups: z (x_tilde), z_p (x_p) and -- Dual step only -- mu (wae_vgan_stage1.py:406, BN statistics)
        G = 3 if self.extra_mu_decoder_pass else 2
        dec_out = torch.empty((1 + G) * B, H, W, 8, dtype=torch.float16, device=dev)
        disc_in = dec_out[:3 * B]
        images_to_nhwc(x, out=disc_in[:B])
        head32, ectx = self.enc.forward(disc_in[:B], updates=self.enc_updates)
        z16 = torch.empty(G * B, zp, dtype=torch.float16, device=dev)
        eps = eps.contiguous().float()
        self._latent(head32, eps, z16[:B], 0, S_KL)
        lib.call("fmri_rows_f32_to_f16", _P(z_p.contiguous().float()), _P(z16[B:]), B, Z, zp, 1.0)
        if G == 3:
            lib.call("fmri_latent_fwd", _P(head32), None, B, Z, zp, _P(z16[2 * B:]), None, None, 0)
        _, dctx = self.dec.forward(z16, G, out=dec_out[B:], zscale=self.zs)
        feat, logit32, sctx, seen = self._discriminate(disc_in, B, table)
        prob, F = self._gan_losses(feat, logit32, B, disc_in[:B], disc_in[B:2 * B], H, W)
        self.fw = dict(B=B, H=H, W=W, F=F, disc_in=disc_in, head32=head32, eps=eps, ectx=ectx, dctx=dctx, sctx=sctx,
                       feat=feat, logit32=logit32, prob=prob, **seen)
        return self.fw

    def gate(self, B_global: int):
        self._gate(B_global, self.fw["F"], True)

    def backward(self, extra_dmu: Optional[torch.Tensor] = None, early_apply: bool = False):
        """``extra_dmu`` [B, z] fp32: an additional true-scale cotangent on the encoder means (Dual step).
        ``early_apply`` (one GPU, used by ``step``): the discriminator's and the decoder's optimizer update + weight
        repack are queued on the side stream right behind their last weight gradient, i.e. they run under the backward
        pass of the next sub-network instead of after the whole backward (nothing later in the step reads those weights);
        ``apply`` then only updates the encoder."""
        if self.mode in ("dcgan", "vae"):
            return self._backward_pixel(early_apply, extra_dmu)
        fw, sc, hp, cfg = self.fw, self.sc, self.hp, self.cfg
        B, H, W = fw["B"], fw["H"], fw["W"]
        Z = cfg.latent_dim
        dev = fw["disc_in"].device
        # ``early_apply`` also says that nobody reads reference-layout gradients between this pass and the updates: on one
        # GPU the weight gradients then stay in their GEMM layout until the sub-network's one fmri_apply_batch launch
        fuse = early_apply and self.dd.recorder is None
        ops.begin_grads(self.enc.group, fuse)
        ops.begin_grads(self.dec.group, fuse, gate=self._gate_flag(1))
        ops.begin_grads(self.dis.group, fuse, gate=self._gate_flag(0))
        dlogit16, dfeat16, stacked = self._start_cotangents(B)
        # weight gradients run on the side stream (ops.side_run) and are joined once, at the end of the backward pass, so
        # that a sub-network's last weight gradients overlap the next one's backward
        dp = self.dd.on
        # ``early``: a sub-network's gradient reduction (data parallel), optimizer update and weight repack are queued on the
        # SIDE stream right behind its last weight gradient -- the main stream neither joins the side stream nor waits for
        # the collective before it goes on with the next sub-network's backward pass.  (Recording into graph segments
        # keeps everything on one stream: the round-3 order with asynchronous collectives joined at the end.)
        early = early_apply and ops._SIDE["on"] and self.dd.recorder is None
        self._applied_early = early
        dimg_a, dimg_b = self.dis.backward(fw["sctx"], dlogit16, sc.a, dfeat16, sc.b, True, slice(B, 3 * B),
                                           join=dp and not early, **stacked)
        dimg_a, dimg_b = self._aug_adjoint(dimg_a, dimg_b, slice(B, 3 * B))
        if early:
            ops.side_run(dev, lambda: self._reduce_apply(self.opt_dis, self.dis, self.flags[0:1], S_NA))
        else:
            self._reduce_async(self.dis.group)
        # decoder cotangent, stored = dec * nA * (lambda*B_true - (1-lambda)*A_true); the weights lambda*nA/nB and
        # 1-lambda are device scalars written by the gate kernel (a recorded step follows the lambda schedule)
        cot = torch.empty(3 * B, H, W, 8, dtype=torch.float16, device=dev)
        # block order [x_tilde: feature loss (encoder path) | x_tilde: decoder loss | x_p: decoder loss]: the two blocks
        # that go through the SAME forward activations (group 0) are adjacent, so the decoder's BatchNorm backward takes
        # them in one pass (BatchNorm.backward2), and the two training blocks are adjacent, so every decoder weight
        # gradient is one launch over 2B rows
        cot[:B].copy_(dimg_b[:B])
        axpby(dimg_b, dimg_a, sc.dec / sc.b, -sc.dec / sc.a, out=cot[B:], a_dev=self._slot(S_C1),
              b_dev=self._slot(S_C2))
        entries = [dict(g=0, scale=sc.b, train=False, need_dz=True), dict(g=0, scale=sc.dec, train=True),
                   dict(g=1, scale=sc.dec, train=True)]
        dz = self.dec.backward(fw["dctx"], cot, entries, join=dp and not early)[0]  # = nB * dz_true
        if early:
            ops.side_run(dev, lambda: self._reduce_apply(self.opt_dec, self.dec, self.flags[1:2], S_GDEC))
        else:
            self._reduce_async(self.dec.group)
        # KL weight: 1, or beta / batch for 'beta-vae' (train_vgan_stage1.py:360-362).  The gate kernel writes it to
        # the device slot S_KLW from the device-resident hyper-parameters, so that a recorded (HIP-graph) step follows
        # set_hyper(beta=...) in the encoder GRADIENT as well as in the logged loss: weight = S_KLW * nB on the device
        kl_dev = torch.mul(self._slot(S_KLW), self._slot(S_NB)) if self.mode == "beta-vae" else None
        dhead16 = self._encoder_cotangent(dz, S_NB, kl_dev, extra_dmu)          # S_NE = nB * nE
        eg = self.enc.group
        tail = eg.offsets["fc.0.weight"]
        if early and dp:
            # the fc.0 ... l_var tail (93 % of the buffer) is reduced on the side stream as soon as the fc weight gradient
            # is final there, under the conv backward; the conv head right behind the last weight gradient
            def reduce_part(part):                  # (side stream) the weight gradients queued so far -> reference layout
                ops.materialize_grads(eg)
                self.dd.all_reduce(part)
            self.enc.backward(fw["ectx"], dhead16, sc.enc, join=False, after_fc_join=False,
                              after_fc=lambda: ops.side_run(dev, lambda: reduce_part(eg.grad[tail:])))
            ops.side_run(dev, lambda: reduce_part(eg.grad[:tail]))
            ops.join_side()
            return
        self.enc.backward(fw["ectx"], dhead16, sc.enc,                  # grads = S_NE * true
                          after_fc=(lambda: self._reduce_async(eg, eg.grad[tail:])) if dp else None)
        if dp:
            ops.materialize_grads(eg)
        self.dd.all_reduce(eg.grad[:tail])
        self.dd.wait_all()

    def _backward_pixel(self, early_apply: bool, extra_dmu: Optional[torch.Tensor] = None):
        """Modes 'dcgan' and 'vae' (train_vgan_stage1.py:374-388): the reconstruction term is the pixel nle.
        ``extra_dmu``: see ``backward`` (mode 'vae' of the Dual step; 'dcgan' does not train the encoder).

        dcgan: decoder <- lambda*d nle - (1-lambda)*d(bce_orig + bce_sampled) on [x_tilde ; x_p], discriminator <-
               d(bce_orig + bce_sampled), encoder not trained.
        vae  : encoder <- d(KL + nle) through the decoder, decoder <- lambda*d nle, discriminator <- d(bce_orig +
               bce_sampled), applied only if the gate re-armed it (flags[0])."""
        fw, sc, cfg = self.fw, self.sc, self.cfg
        B, H, W = fw["B"], fw["H"], fw["W"]
        Z = cfg.latent_dim
        d_in = fw["disc_in"]
        dev = d_in.device
        dp = self.dd.on
        self._applied_early = False
        for n in (self.enc, self.dec, self.dis):
            n.group.zero_grad()
        dlogit16 = self._logit_cotangent(B)
        x16, xt16 = d_in[:B], d_in[B:2 * B]
        if self.mode == "dcgan":
            dimg_a, _ = self.dis.backward(fw["sctx"], dlogit16, sc.a, None, sc.b, True, slice(B, 3 * B), join=dp)
            dimg_a, _ = self._aug_adjoint(dimg_a, None, slice(B, 3 * B))
            self.dd.all_reduce_async(self.dis.group.grad)
            # stored = dec * nA * (lambda * d nle - (1-lambda) * A), d nle / d x_tilde = x_tilde - x
            dnle = axpby(xt16, x16, 1.0, -1.0)
            cot = torch.empty(2 * B, H, W, 8, dtype=torch.float16, device=dev)
            axpby(dnle, dimg_a[:B], sc.dec, -sc.dec / sc.a, out=cot[:B], a_dev=self._slot(S_C3),
                  b_dev=self._slot(S_C2))
            axpby(dimg_a[B:], None, -sc.dec / sc.a, 0.0, out=cot[B:], a_dev=self._slot(S_C2))
            entries = [dict(g=0, scale=sc.dec, train=True), dict(g=1, scale=sc.dec, train=True)]
            # (joined on one GPU too: no encoder pass follows whose join would cover the weight gradients still running
            # on the side stream, and ``apply`` reads them on this one)
            self.dec.backward(fw["dctx"], cot, entries)
            self.dd.all_reduce_async(self.dec.group.grad)
            self.dd.wait_all()
            return
        # vae
        self.dis.backward(fw["sctx"], dlogit16, sc.a, None, sc.b, True, None, join=dp)
        self.dd.all_reduce_async(self.dis.group.grad)
        # stored = p * nP * (x_tilde - x); the decoder gradients carry nP and are scaled by lambda in the optimizer
        cot = axpby(xt16, x16, sc.p, -sc.p, a_dev=self._slot(S_NP), b_dev=self._slot(S_NP))
        entries = [dict(g=0, scale=sc.p, train=True, need_dz=True)]
        dz = self.dec.backward(fw["dctx"], cot, entries, join=dp)[0]        # = nP * dz_true
        self.dd.all_reduce_async(self.dec.group.grad)
        dhead16 = self._encoder_cotangent(dz, S_NP, extra_dmu=extra_dmu)        # S_NE = nP * nE
        eg = self.enc.group
        tail = eg.offsets["fc.0.weight"]
        self.enc.backward(fw["ectx"], dhead16, sc.enc,
                          after_fc=(lambda: self.dd.all_reduce_async(eg.grad[tail:])) if dp else None)
        self.dd.all_reduce(eg.grad[:tail])
        self.dd.wait_all()

    def _reduce_apply(self, opt, net, flag, slot):
        """(current stream = the side stream) SUM all-reduce of the sub-network's gradient buffer over the ranks -- nothing
        on one GPU --, then its optimizer update and the refresh of everything derived from its weights."""
        if self.dd.on:
            ops.materialize_grads(net.group)         # deferred weight gradients -> reference layout, one launch
        self.dd.all_reduce(net.group.grad)
        self._apply_one(opt, net, flag, slot)

    def _apply_one(self, opt, net, flag, slot):
        """Optimizer update of one sub-network + refresh of everything derived from its weights (current stream)."""
        opt.step(flag, gdev=self._slot(slot))
        refresh_net(net)

    def apply(self):
        self._monitor_tail()
        if self.mode != "dcgan":                         # 'dcgan': train_enc = False (train_vgan_stage1.py:376)
            self.opt_enc.step(None, gdev=self._slot(S_NE))
        if getattr(self, "_applied_early", False):
            self._applied_early = False
            return
        self.opt_dec.step(self.flags[1:2], gdev=self._slot(S_GDEC))
        self.opt_dis.step(self.flags[0:1], gdev=self._slot(S_NA))

    def capture_forward(self, x, eps=None, z_p=None, warmup: int = 2, aug=None):
        """Hybrid launch mode (one GPU): the forward pass + gate -- a dependent chain with nothing to overlap -- is
        recorded into a HIP graph, the backward pass and the updates stay eagerly issued launches on two streams
        (``ops.side_run``).  Halves the Python work per step, which is what decides whether a slow host can keep the
        two-stream backward fed.  Also available to data-parallel runs with per-rank BN statistics (no collective in
        the forward pass).  Returns a zero-argument callable running one full step on the static inputs."""
        if self.dd.on and self.dd.sync_bn:
            raise RuntimeError("capture_forward: the forward pass holds SyncBN collectives (use capture())")
        # data parallel with per-rank BN statistics: the forward pass's only collective is the sum of the loss scalars at
        # its very end; that all-reduce, the gate and the backward pass with its gradient reductions stay eager
        gate_in_graph = not self.dd.on
        nets = (self.enc, self.dec, self.dis)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self.step(x, eps, z_p, aug)
            ops.join_side()
            for n in nets:
                refresh_net(n)               # so that the recorded forward contains no refresh launches
        torch.cuda.current_stream().wait_stream(side)
        B = x.shape[0]
        graph = torch.cuda.CUDAGraph()
        # thread_local: the communication backend's watchdog thread may touch the device while this thread records
        self._defer_loss_reduce = not gate_in_graph      # the forward's only collective (sum of the loss scalars)
        try:
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                self.forward(x, eps, z_p, aug)
                if gate_in_graph:
                    self.gate(B)
        finally:
            self._defer_loss_reduce = False

        fw_captured = self.fw                 # the tensors the recorded forward writes

        def run():
            if self.ema is not None:
                self.ema.prime()
            for n in nets:
                refresh_net(n)               # no-ops for the sub-networks the last backward refreshed early
            graph.replay()
            self.fw = fw_captured            # an eager step() / forward() in between rebinds self.fw to its own batch
            if not gate_in_graph:
                self.dd.all_reduce(self.scal[:N_REDUCED])
                self.gate(B * self.dd.world)
            self.backward(early_apply=True)
            self.apply()
            self._log_append()
            return self.scal
        self._fwd_graph = graph
        return run

    def step(self, x=None, eps=None, z_p=None, aug=None):
        """One full training step; returns the device scalar block (see LOG_KEYS) without syncing.  ``eps`` / ``z_p``
        left out: drawn by the step's ``rng`` (ValueError without one).  ``x`` left out: the step's ``feed`` draws it.
        ``aug`` (steps with ``augment=``): the fp32 [2B, 8] table of this step's transforms; left out, the ``rng`` draws it."""
        fed = self._fed(x)
        if fed is not None:
            x = fed[0]
        fw = self.forward(x, eps, z_p, aug)
        self.gate(fw["B"] * self.dd.world)
        self.backward(early_apply=True)
        self.apply()
        self._log_append()
        return self.scal


class CognitiveStep(_GanStepBase):
    """Stage-II / Stage-III steps of the Dual-VAE/GAN (fMRI -> image), `VaeGanCognitive` wiring
    (models/vae_gan.py:352-395) + the loop bodies train/train_vgan_stage2.py:321-407 (stage=2: decoder
    frozen, teacher distillation, encoder + discriminator trained, no gate, grads clamped to +-1) and
    train/train_vgan_stage3.py:324-411 (stage=3: cognitive encoder frozen, decoder + discriminator trained,
    gate on, clamp +-1)."""

    def __init__(self, cfg: ArchConfig, n_voxels: int, device, stage: int, hp: Optional[GanHyper] = None,
                 scales: Optional[Scales] = None, distributed: bool = False, sync_bn: bool = True,
                 gate_skip: bool = True, mode: str = "vae-gan", monitor: bool = False,
                 rng: Optional[DeviceRng] = None, feed=None, schedule=None, log=None, checkpoints=None, ema=None,
                 augment=None, fmri_augment=None):
        """``fmri_augment``: a fmri_hip.voxaug.VoxelAugment (needs ``rng``); the rows the cognitive encoder reads are then
        the fMRI rows under trial noise, voxel dropout, a masked span and gain jitter -- two launches (the per-row table,
        the transform) in place of the fp32 -> fp16 conversion, drawn at the offset of the noise draws, fresh at every
        replay of a recorded step.  ``step(..., fmri_aug=table)`` pins the per-row parameters (fp32 [B, 8]);
        ``last_fmri_augment()`` / ``last_fmri16()`` read the table and the rows.  A feed's ``fmri`` / ``fmri16``, the
        teacher, the images and the evaluator keep the clean rows.  None: nothing is added.
        ``augment``: a fmri_hip.augment.DiffAugment (see Stage1Step); in Stage II, mode 'vae-gan', the "real" image that
        shares its transform with x_tilde is the teacher's reconstruction.
        ``ema``: a fmri_hip.ema.WeightEma (see Stage1Step): by default the cognitive encoder in Stage II, the decoder in
        Stage III -- a frozen network has no average.
        ``checkpoints``: a fmri_hip.state.StateRing (see Stage1Step); the frozen networks and the teacher are state too.
        The discriminator keeps ``recon_level`` 3: the Stage-II / Stage-III scripts build theirs with the default
        (train_vgan_stage2.py:213, train_vgan_stage3.py:231), so there is no such option here.
        ``monitor``: record the step's numerics on the device (``numerics()``, fmri_hip/monitor.py).
        ``schedule`` / ``log``: device-side epoch-end schedule and per-step training log (see Stage1Step).
        ``rng``: a fmri_hip.rng.DeviceRng; ``step(fmri, image)`` then draws ``eps``, ``z_p`` and -- where the teacher
        samples (stage 2, mode 'vae-gan') -- ``eps_teacher`` on the device (see Stage1Step).
        ``feed``: a fmri_hip.feed.DeviceFeed over a dataset with fMRI rows; ``step()`` then draws the image and the fMRI
        row of the same samples itself (see Stage1Step).
        ``mode``: 'vae-gan' (default) or 'vae' -- the scripts' `--mode vae` (train_vgan_stage2.py:234-238,362-366;
        train_vgan_stage3.py:370-374): no teacher net (the discriminator's "real" slot is the ground-truth image), the
        reconstruction term is the PIXEL nle instead of the feature mse, the discriminator loss bce_orig + bce_sampled.
        Stage II: encoder <- d(KL + nle) through the frozen decoder, discriminator trained (the script's train_dis = False
        is overwritten two lines later).  Stage III: decoder <- lambda * d nle, discriminator updated only in a step whose
        gate re-arms both."""
        assert stage in (2, 3)
        if mode not in ("vae-gan", "vae"):
            raise ValueError("mode must be 'vae-gan' or 'vae'")
        self.cfg, self.stage, self.n_voxels = cfg, stage, n_voxels
        self.gate_skip = bool(gate_skip)
        self.cog = CognitiveEncoderNet(cfg, n_voxels, device)
        self.dec = DecoderNet(cfg, device, cfg.encoder_channels[2])
        self.dec.fc_bn.enable_lazy_running()
        self.dis = DiscriminatorNet(cfg, device)
        self.teacher_enc = EncoderNet(cfg, device) if (stage == 2 and mode != "vae") else None
        nets = [self.cog, self.dec, self.dis] + ([self.teacher_enc] if self.teacher_enc is not None else [])
        self._init_common(device, hp, scales, distributed, sync_bn, nets)
        self._pre_replay = [self.dec.fc_bn._running_in]      # reloads after an outside write of the buffers only
        if feed is not None and (feed.fmri is None or feed.fmri.shape[1] != n_voxels):
            raise ValueError("CognitiveStep: feed needs a dataset with fp32 fMRI rows of n_voxels columns")
        self._init_rng(rng, feed)
        self._init_augment(augment)
        self._init_fmri_augment(fmri_augment)
        self.mode = mode
        hp = self.hp
        self.opt_enc = _Optim(self.cog.group, "rmsprop", hp.lr, hp.alpha, hp.eps)
        self.opt_dec = _Optim(self.dec.group, "rmsprop", hp.lr, hp.alpha, hp.eps)
        self.opt_dis = _Optim(self.dis.group, "rmsprop", hp.lr, hp.alpha, hp.eps)
        self.optims = [self.opt_enc, self.opt_dec, self.opt_dis]
        self._init_monitor(monitor, [("encoder", self.opt_enc, self.cog), ("decoder", self.opt_dec, self.dec),
                                     ("discriminator", self.opt_dis, self.dis)], 1)
        self._init_extras(schedule, log, checkpoints, ema)

    outputs_gt_x = True

    def _trained(self):
        return ["encoder", "discriminator"] if self.stage == 2 else ["decoder", "discriminator"]

    def load_recipe(self, seed: int, perturb: bool = False):
        """Teacher VaeGan weights from seed, cognitive encoder from seed+100 (the golden-fixture recipe)."""
        rs = np.random.RandomState(seed)
        enc_tmp = self.teacher_enc if self.teacher_enc is not None else EncoderNet(self.cfg, self.device)
        for n in (enc_tmp, self.dec, self.dis):
            n.group.load_recipe(rs, perturb)
        self.cog.group.load_recipe(np.random.RandomState(seed + 100), perturb)

    def _subnets(self):
        """(state-dict prefix, network, slot of the device factor its gradients carry or None: not trained in this
        stage) per sub-network."""
        st = self.stage
        nets = [("encoder.", self.cog, S_NE if st == 2 else None), ("decoder.", self.dec, S_GDEC if st == 3 else None),
                ("discriminator.", self.dis, S_NA)]
        if self.teacher_enc is not None:
            nets.append(("teacher_net.encoder.", self.teacher_enc, None))
        return nets

    def _state_groups(self):
        nets = [(pre, n) for pre, n, _ in self._subnets()]
        if self.teacher_enc is not None:         # the teacher's decoder / discriminator are the model's own
            nets += [("teacher_net." + pre, n) for pre, n in nets[1:3]]
        return nets

    def load_state_dict(self, sd):
        """A Stage-II / Stage-III checkpoint as the scripts write it (``model.state_dict()`` of ``VaeGanCognitive``):
        ``encoder.`` = cognitive encoder, ``decoder.``, ``discriminator.`` and, for stage 2, ``teacher_net.encoder.``
        (train/train_vgan_stage3.py:241 loads the Stage-II file this way; its ``teacher_net.decoder./discriminator.``
        entries alias ``decoder.`` / ``discriminator.`` in Stage II and are not needed in Stage III)."""
        for pre, n, _ in self._subnets():
            n.group.load_state_dict(sd, pre)

    def load_teacher(self, sd):
        """A Stage-I ``VaeGan`` checkpoint as the teacher (train/train_vgan_stage2.py:212-217,230): its decoder and
        discriminator become the model's own (frozen decoder, trained discriminator), its encoder the teacher encoder."""
        if self.teacher_enc is not None:
            self.teacher_enc.group.load_state_dict(sd, "encoder.")
        self.dec.group.load_state_dict(sd, "decoder.")
        self.dis.group.load_state_dict(sd, "discriminator.")

    def forward(self, fmri: torch.Tensor, image: torch.Tensor, eps: Optional[torch.Tensor] = None,
                z_p: Optional[torch.Tensor] = None, eps_teacher: Optional[torch.Tensor] = None,
                fmri16: Optional[torch.Tensor] = None, aug: Optional[torch.Tensor] = None,
                fmri_aug: Optional[torch.Tensor] = None):
        """``fmri16``: the fp16 [B, pad8(V)] rows of ``fmri`` where the caller already has them (a feed's gather pass
        writes both); otherwise they are made here.  With ``fmri_augment=`` the encoder reads the augmented rows instead
        (``fmri_aug``: their fp32 [B, 8] table; left out, the ``rng`` draws it)."""
        require_gpu(fmri)
        cfg = self.cfg
        B, _, H, W = image.shape
        with self.draws:
            table = self._aug_table(aug, B, H)
            _, rows16 = self._fmri_rows(fmri_aug, fmri)
            if self.teacher_enc is not None:
                eps, z_p, eps_teacher = self._noise(B, ("eps", SID_EPS, eps), ("z_p", SID_ZP, z_p),
                                                    ("eps_teacher", SID_EPS_TEACHER, eps_teacher))
            else:
                eps, z_p = self._noise(B, ("eps", SID_EPS, eps), ("z_p", SID_ZP, z_p))
        Z, zp = cfg.latent_dim, pad8(cfg.latent_dim)
        dev = image.device
        self.scal.zero_()
        if self.mon is not None:
            self.mon.zero()
        disc_in = torch.empty(3 * B, H, W, 8, dtype=torch.float16, device=dev)
        if rows16 is not None:
            fmri16 = rows16
        elif fmri16 is None:
            fmri16 = rows_to_f16(fmri)
        head32, cctx = self.cog.forward(fmri16)
        eps = eps.contiguous().float()
        if self.teacher_enc is not None:
            # decoder groups in disc_in row order: 0 = teacher reconstruction ("real"), 1 = x_tilde, 2 = x_p
            z16 = torch.empty(3 * B, zp, dtype=torch.float16, device=dev)
            img16 = images_to_nhwc(image)
            head_t, _ = self.teacher_enc.forward(img16)
            self._latent(head_t, eps_teacher.contiguous().float(), z16[:B], 0, None)
            self._latent(head32, eps, z16[B:2 * B], 1, S_KL)
            lib.call("fmri_rows_f32_to_f16", _P(z_p.contiguous().float()), _P(z16[2 * B:]), B, Z, zp, 1.0)
            # reference call order of the decoder: x_tilde, teacher reconstruction, x_p (vae_gan.py:365,377,390)
            _, dctx = self.dec.forward(z16, 3, out=disc_in, stat_order=(1, 0, 2), zscale=self.zs)
            g_tilde, g_p = 1, 2
        else:
            z16 = torch.empty(2 * B, zp, dtype=torch.float16, device=dev)
            images_to_nhwc(image, out=disc_in[:B])
            self._latent(head32, eps, z16[:B], 0, S_KL)
            lib.call("fmri_rows_f32_to_f16", _P(z_p.contiguous().float()), _P(z16[B:]), B, Z, zp, 1.0)
            _, dctx = self.dec.forward(z16, 2, out=disc_in[B:], zscale=self.zs)
            g_tilde, g_p = 0, 1
        feat, logit32, sctx, seen = self._discriminate(disc_in, B, table)
        prob, F = self._gan_losses(feat, logit32, B, disc_in[:B], disc_in[B:2 * B], H, W)
        self.fw = dict(B=B, H=H, W=W, F=F, disc_in=disc_in, head32=head32, eps=eps, cctx=cctx, dctx=dctx, sctx=sctx,
                       feat=feat, logit32=logit32, prob=prob, g_tilde=g_tilde, g_p=g_p, **seen)
        return self.fw

    def gate(self, B_global: int):
        if self.stage == 2:
            self._gate(B_global, self.fw["F"], False, 1, 0)          # train_dis = True, train_dec = False
        else:
            self._gate(B_global, self.fw["F"], True)

    def backward(self, fuse: bool = False):
        """``fuse`` (used by ``step``): the updates follow right behind and nobody reads reference-layout gradients in
        between -- weight gradients stay in their GEMM layout until the sub-network's one fmri_apply_batch launch
        (ops.begin_grads)."""
        fw, sc, hp, cfg = self.fw, self.sc, self.hp, self.cfg
        B, H, W, Z = fw["B"], fw["H"], fw["W"], cfg.latent_dim
        dev = fw["disc_in"].device
        fuse = fuse and self.dd.recorder is None
        if self.mode == "vae":
            return self._backward_pixel(fuse)
        dlogit16, dfeat16, stacked = self._start_cotangents(B)
        # (gate flags: see Stage1Step -- no gradients for a sub-network the gate does not train)
        if self.stage == 2:
            ops.begin_grads(self.cog.group, fuse)
            ops.begin_grads(self.dis.group, fuse, gate=self._gate_flag(0))
            _, dimg_b = self.dis.backward(fw["sctx"], dlogit16, sc.a, dfeat16, sc.b, True, slice(B, 2 * B),
                                          img_streams=(False, True), **stacked)
            _, dimg_b = self._aug_adjoint(None, dimg_b, slice(B, 2 * B))
            self._reduce_async(self.dis.group)                  # under the decoder / cognitive-encoder backward
            entries = [dict(g=fw["g_tilde"], scale=sc.b, train=False, need_dz=True)]
            dz = self.dec.backward(fw["dctx"], dimg_b, entries)[0]
            dhead16 = self._encoder_cotangent(dz, S_NB)
            self.cog.backward(fw["cctx"], dhead16, sc.enc)
            self._reduce_async(self.cog.group)
            self.dd.wait_all()
        else:
            ops.begin_grads(self.dec.group, fuse, gate=self._gate_flag(1))
            ops.begin_grads(self.dis.group, fuse, gate=self._gate_flag(0))
            dimg_a, dimg_b = self.dis.backward(fw["sctx"], dlogit16, sc.a, dfeat16, sc.b, True, slice(B, 3 * B),
                                               **stacked)
            dimg_a, dimg_b = self._aug_adjoint(dimg_a, dimg_b, slice(B, 3 * B))
            self._reduce_async(self.dis.group)                  # under the decoder backward
            cot = axpby(dimg_b, dimg_a, sc.dec / sc.b, -sc.dec / sc.a, a_dev=self._slot(S_C1), b_dev=self._slot(S_C2))
            entries = [dict(g=0, scale=sc.dec, train=True), dict(g=1, scale=sc.dec, train=True)]
            self.dec.backward(fw["dctx"], cot, entries)
            self._reduce_async(self.dec.group)
            self.dd.wait_all()

    def _backward_pixel(self, fuse: bool):
        """mode 'vae' (train_vgan_stage2.py:362-366, train_vgan_stage3.py:370-374): the reconstruction term is the pixel
        nle, d nle / d x_tilde = x_tilde - x_gt; the discriminator's loss is bce_orig + bce_sampled (no image gradient
        is needed: nothing upstream of it trains on a discriminator term)."""
        fw, sc, cfg = self.fw, self.sc, self.cfg
        B, H, W, Z = fw["B"], fw["H"], fw["W"], cfg.latent_dim
        d_in = fw["disc_in"]
        dev = d_in.device
        dlogit16 = self._logit_cotangent(B)
        x16, xt16 = d_in[:B], d_in[B:2 * B]
        if self.stage == 2:
            ops.begin_grads(self.cog.group, fuse)
            ops.begin_grads(self.dis.group, fuse, gate=self._gate_flag(0))
        else:
            ops.begin_grads(self.dec.group, fuse, gate=self._gate_flag(1))
            ops.begin_grads(self.dis.group, fuse, gate=self._gate_flag(0))
        self.dis.backward(fw["sctx"], dlogit16, sc.a, None, sc.b, True, None)
        self._reduce_async(self.dis.group)
        # stored = p * nP * (x_tilde - x_gt)
        cot = axpby(xt16, x16, sc.p, -sc.p, a_dev=self._slot(S_NP), b_dev=self._slot(S_NP))
        if self.stage == 2:
            entries = [dict(g=fw["g_tilde"], scale=sc.p, train=False, need_dz=True)]
            dz = self.dec.backward(fw["dctx"], cot, entries)[0]                  # = nP * dz_true
            dhead16 = self._encoder_cotangent(dz, S_NP)                         # S_NE = nP * nE
            self.cog.backward(fw["cctx"], dhead16, sc.enc)
            self._reduce_async(self.cog.group)
        else:
            # the decoder gradients carry nP; the optimizer divides by S_GDEC = nP / lambda (loss_decoder = lambda * nle)
            entries = [dict(g=fw["g_tilde"], scale=sc.p, train=True)]
            self.dec.backward(fw["dctx"], cot, entries)
            self._reduce_async(self.dec.group)
        self.dd.wait_all()

    def apply(self):
        self._monitor_tail()
        if self.stage == 2:
            self.opt_enc.step(None, clamp=1.0, gdev=self._slot(S_NE))
            self.opt_dis.step(self.flags[0:1], clamp=1.0, gdev=self._slot(S_NA))
        else:
            # (S_GDEC: nA in mode 'vae-gan', nP / lambda in mode 'vae' -- the gate kernel writes it)
            self.opt_dec.step(self.flags[1:2], clamp=1.0, gdev=self._slot(S_GDEC))
            self.opt_dis.step(self.flags[0:1], clamp=1.0, gdev=self._slot(S_NA))

    def step(self, fmri=None, image=None, eps=None, z_p=None, eps_teacher=None, aug=None, fmri_aug=None):
        fed = self._fed(fmri, image)
        fmri16 = None
        if fed is not None:
            image, fmri, fmri16 = fed
        fw = self.forward(fmri, image, eps, z_p, eps_teacher, fmri16=fmri16, aug=aug, fmri_aug=fmri_aug)
        self.gate(fw["B"] * self.dd.world)
        self.backward(fuse=True)
        self.apply()
        self._log_append()
        return self.scal
