"""Sub-networks of the VAE/GAN as explicit forward / backward passes over the HIP operators.

Mirrors (reference models/vae_gan.py): Encoder :63-96, Decoder :99-132, Discriminator :135-187,
CognitiveEncoder :190-232, WaeDiscriminator :499-529.  Parameter names/shapes are the reference
state-dict entries; activations are fp16 NHWC, statistics/losses/master weights fp32.

Backward passes are written by hand (no autograd inside the engine): each returns/accumulates exactly
the gradients the training-step bodies consume, and supports several cotangent "streams" through one
saved forward pass (the two-stream trick of SURVEY 8a-14).
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import ctypes
import os

import torch

from . import lib, ops
from .ops import (ACT_NONE, ACT_RELU, ACT_TANH, BatchNorm, ConvLayer, DenseLayer, act_backward, join_side, pad8,
                  repack_group)
from .params import (ArchConfig, FlatGroup, cognitive_encoder_spec, decoder_spec, discriminator_spec, encoder_spec,
                     wae_discriminator_spec)

_P = lib.ptr


class FusedHeads:
    """l_mu | l_var as one N = 2z GEMM (models/vae_gan.py:84-85,91-92).  The group lays the two heads out side by side
    (FlatGroup.heads_adjacent), so the concatenated weight / bias and their gradients are views of the flat buffers: no
    copies, the weight gradient accumulates in place, the fp16 copies are part of the group's batched repack.  (Groups
    with another layout fall back to concatenated scratch copies refreshed when the masters change.)"""

    def __init__(self, group: FlatGroup, k_in: int, z: int):
        self.group, self.z, self.k_in = group, z, k_in
        dev = group.device
        self.direct = bool(getattr(group, "heads_adjacent", False))
        if self.direct:
            ow, ob = group.offsets["l_mu.weight"], group.offsets["l_mu.bias"]
            assert group.offsets["l_var.weight"] == ow + z * k_in and group.offsets["l_var.bias"] == ob + z
            self.wcat = group.data[ow:ow + 2 * z * k_in].view(2 * z, k_in)
            self.gw = group.grad[ow:ow + 2 * z * k_in].view(2 * z, k_in)
            self.bcat = group.data[ob:ob + 2 * z]
            self.gb = group.grad[ob:ob + 2 * z]
            self.dense = DenseLayer(group, (self.wcat, self.gw), (self.bcat, self.gb), k_in, 2 * z)
            return
        self.wcat = torch.empty(2 * z, k_in, dtype=torch.float32, device=dev)
        self.bcat = torch.empty(2 * z, dtype=torch.float32, device=dev)
        self.gw = torch.zeros(2 * z, k_in, dtype=torch.float32, device=dev)
        self._vg = _Versioned(group)
        self.dense = DenseLayer(self._vg, (self.wcat, self.gw), (self.bcat, None), k_in, 2 * z)
        self._v = -1

    def refresh(self):
        """Bring the concatenated scratch weights and their fp16 GEMM copies up to date now (instead of lazily at the
        next forward)."""
        if self.direct:
            return                                   # views of the masters; packed with the group
        self._sync()
        repack_group(self._vg)

    def _sync(self):
        if self.direct:
            return
        if self._v != self.group.version:
            v = self.group.views
            z = self.z
            self.wcat[:z].copy_(v["l_mu.weight"])
            self.wcat[z:].copy_(v["l_var.weight"])
            self.bcat[:z].copy_(v["l_mu.bias"])
            self.bcat[z:].copy_(v["l_var.bias"])
            self._v = self.group.version

    def forward(self, h16):
        self._sync()
        _, head32 = self.dense.forward(h16, ACT_NONE, want16=False, want32=True)
        return head32                                   # [B, 2z] fp32 (mu | logvar), bias added

    def backward(self, h16, dhead16, scale, need_dgrad=True):
        if self.direct:
            self.dense.wgrad(h16, dhead16, scale)        # side stream, accumulates into the flat gradient buffer
            self.dense.bias_grad(dhead16, scale)
        else:
            self._sync()
            g = self.group.grads
            z = self.z
            self.gw.zero_()
            self.dense._wgrad(h16, dhead16, scale)      # current stream: gw is read right below
            g["l_mu.weight"].add_(self.gw[:z])
            g["l_var.weight"].add_(self.gw[z:])
            bs = dhead16.float().sum(0) * (1.0 / scale)
            g["l_mu.bias"].add_(bs[:z])
            g["l_var.bias"].add_(bs[z:2 * z])
        if not need_dgrad:
            return None
        dh, _ = self.dense.dgrad(dhead16)
        return dh


_MLP_ON = os.environ.get("FMRI_MLP") != "off"        # fused latent-discriminator kernels (csrc/mlp.hip)


def _bwd_epi(**kw):
    """``bn_bwd`` argument of ``ConvLayer.dgrad`` when the BatchNorm-backward epilogue is switched on (ops._EPI_BWD)."""
    return kw if ops._EPI_BWD else None


class ConvBlock:
    """One conv / deconv + BatchNorm(+ ReLU) block: the two steps every network writes the same way.  The BatchNorm half
    of the forward stays with the networks (``BatchNorm.forward`` per call against the decoder's ``forward_groups``
    over its call groups: with SyncBN these exchange and finalize differently)."""

    def __init__(self, conv: ConvLayer, bn: BatchNorm):
        self.conv, self.bn = conv, bn

    def conv_forward(self, h: torch.Tensor, groups: int = 1, keep_raw: bool = False):
        """The convolution of the block on ``h`` -> (tensor, whether it already is the BatchNorm's output).
        eval: the BatchNorm rides in the convolution's epilogue where its kernel has one (no raw tensor then), unless
        the caller needs the raw tensor (``keep_raw``); train: the epilogue is asked for the batch statistics of each
        of ``groups`` equal image ranges (``conv.take_stats(g)``)."""
        conv, bn = self.conv, self.bn
        if bn.eval_mode and not bn.perm and not keep_raw:
            out = conv.forward(h, affine=bn.eval_affine())
            return out, conv.aff_applied
        return conv.forward(h, bn_groups=0 if bn.eval_mode else groups), False

    def dgrad_below(self, draw: torch.Tensor, below: "ConvBlock", raw_below, groups, hi: int, wi: int):
        """Data gradient of this block's convolution into the block ``below`` -> (cotangent of below's activation,
        ``take_bwd_stats()``).  With the BatchNorm-backward epilogue on, the kernel masks with below's ReLU and reduces
        its BatchNorm backward sums: one statistics group (first image of ``raw_below``, BNSaved) per cotangent block."""
        d = self.conv.dgrad(draw, hi, wi, bn_bwd=_bwd_epi(bn=below.bn, x=raw_below, groups=groups))
        return d, self.conv.take_bwd_stats()


class Cot(NamedTuple):
    """One cotangent block of B rows through a saved forward pass: ``g`` = forward call group whose activations it
    belongs to, ``scale`` = loss scale it carries, ``train`` = accumulate parameter gradients, ``img`` = its image
    gradient is wanted (discriminator), ``need_dz`` = its latent gradient is wanted (decoder)."""
    g: int
    scale: float
    train: bool
    img: bool = True
    need_dz: bool = False


def _rows(t: torch.Tensor, lo: int, hi: int) -> torch.Tensor:
    """Rows lo .. hi-1 of ``t``; ``t`` itself where that is all of it (one cotangent block, one forward group: the
    backward passes of the encoder and the discriminator build no views)."""
    return t if lo == 0 and hi == t.shape[0] else t[lo:hi]


def _bn_backward_blocks(bn: BatchNorm, raw_all, sv_all, cots, B: int, d_all, draw_all, stat):
    """BatchNorm backward of every cotangent block of one layer: ``d_all`` -> ``draw_all`` ([E*B, ...] both), block e
    through rows g*B.. of ``raw_all`` and ``sv_all[g]``.  Two adjacent blocks through the same forward activations, at
    most one of them training, are one two-stream pass (the gamma / beta gradients come from whichever trains).  With
    SyncBN the reductions of all blocks run first (phase 1) into one [2E][C] buffer that is exchanged ONCE, then the
    apply passes (phase 2).  The discriminator's two streams are the pair (A, B): paired with the parameter gradients
    from A whenever B does not train.  Its callers never train B next to A (the fused steps pass train=True,
    train_b=False; the module API passes one stream), so the pairing with the gradients from B, and the single
    exchange for two training streams, are the decoder's cases only."""
    E = len(cots)
    sync = bn.reducer is not None
    sums_all = torch.empty(2 * E, bn.C, dtype=torch.float32, device=d_all.device) if sync else None
    for phase in ((1, 2) if sync else (3,)):
        if phase == 2:
            bn.reducer(sums_all)
        e = 0
        while e < E:
            en = cots[e]
            nx = cots[e + 1] if e + 1 < E else None
            sm = sums_all[2 * e:] if sync else None
            if nx is not None and nx.g == en.g and not (nx.train and en.train):
                ps = 1 if nx.train else 0
                tr = nx if nx.train else en
                bn.backward2(_rows(raw_all, en.g * B, (en.g + 1) * B), _rows(d_all, e * B, (e + 2) * B), sv_all[en.g],
                             True, tr.scale if tr.train else None, out=_rows(draw_all, e * B, (e + 2) * B),
                             param_stream=ps, stat=stat, stat_group=e, sums=sm[:4] if sync else None, phase=phase)
                e += 2
            else:
                bn.backward(_rows(raw_all, en.g * B, (en.g + 1) * B), _rows(d_all, e * B, (e + 1) * B), sv_all[en.g],
                            True, en.scale if en.train else None, out=_rows(draw_all, e * B, (e + 1) * B), stat=stat,
                            stat_group=e, sums=sm[:2] if sync else None, phase=phase)
                e += 1


def _wgrad_runs(cots):
    """Weight-gradient runs [(first block, blocks, first forward group, scale)]: consecutive training blocks with the same
    scale through consecutive forward groups are one launch over all their rows (2 x 256 images as one 512-image launch:
    638 vs 806 us for the decoder's four conv layers, tools/probes/wgrad_n512.py).  The discriminator's streams all go
    through group 0 and never merge: one run per training stream."""
    runs, e, E = [], 0, len(cots)
    while e < E:
        if not cots[e].train:
            e += 1
            continue
        f = e
        while (f + 1 < E and cots[f + 1].train and cots[f + 1].scale == cots[e].scale
               and cots[f + 1].g == cots[f].g + 1):
            f += 1
        runs.append((e, f - e + 1, cots[e].g, cots[e].scale))
        e = f + 1
    return runs


def _wgrad_blocks(layer, x_all, d_all, runs, B: int):
    """Issue ``layer``'s weight gradient (side stream) for every run of ``_wgrad_runs``."""
    for e0, n, g0, scale in runs:
        layer.wgrad(_rows(x_all, g0 * B, (g0 + n) * B), _rows(d_all, e0 * B, (e0 + n) * B), scale)


def _dgrad_live(conv: ConvLayer, d: torch.Tensor, live: int, hi: int, wi: int, relu_y=None):
    """Data gradient of ``d`` whose rows from ``live`` on are exact zeros: the kernel (per image) skips them, the result
    there is zero."""
    out = torch.empty(d.shape[0], hi, wi, conv.cinp, dtype=torch.float16, device=d.device)
    conv.dgrad(d[:live], hi, wi, out=out[:live], relu_y=relu_y)
    out[live:].zero_()
    return out


def refresh_net(net):
    """Everything a sub-network derives from its master parameters -- fp16 GEMM weights, (C,H,W)-permuted BatchNorm
    vectors, the fused heads' concatenated weights -- refreshed NOW on the current stream.  They are otherwise
    refreshed lazily inside the next forward; a recorded forward (HIP graph) must not contain those launches."""
    repack_group(net.group)
    for bn in net.all_bns():
        bn._params()
        if bn._lazy:
            bn._running_in()             # reloads only after an outside write of the buffers (load_state_dict)
    heads = getattr(net, "heads", None)
    if heads is not None:
        heads.refresh()


class _Versioned:
    """Adapter so scratch-weight layers follow the owning group's version counter."""

    def __init__(self, group):
        self._g = group

    @property
    def version(self):
        return self._g.version


class _JoinedBackward:
    """Mixin of the networks: the public ``backward`` around each network's ``_backward``."""

    def backward(self, *args, join: bool = True, **kwargs):
        """``_backward`` + join of the side stream its weight gradients were issued on (ops.side_run).  ``join=False``
        leaves them in flight (the caller joins with ops.join_side() before the gradients are read)."""
        out = self._backward(*args, **kwargs)
        if join:
            join_side()
        return out


# ------------------------------------------------------------------------------------------------
class EncoderNet(_JoinedBackward):
    def __init__(self, cfg: ArchConfig, device, channel_in: int = 3):
        self.cfg = cfg
        self.group = FlatGroup(encoder_spec(cfg, channel_in), device)
        g = self.group
        self.blocks = []
        cin = channel_in
        for i, c in enumerate(cfg.encoder_channels[:3]):
            self.blocks.append(ConvBlock(ConvLayer(g, f"conv.{i}.conv.weight", None, "conv", cin, c, cfg.kernel_size,
                                                   cfg.stride, cfg.padding), BatchNorm(g, f"conv.{i}.bn.", c)))
            cin = c
        self.size = cin
        hw = cfg.fc_input * cfg.fc_input
        self.fc = DenseLayer(g, "fc.0.weight", None, hw * cin, cfg.fc_output, in_perm=(cin, hw))
        self.fc_bn = BatchNorm(g, "fc.1.", cfg.fc_output)
        self.heads = FusedHeads(g, cfg.fc_output, cfg.latent_dim)

    def all_bns(self):
        return [blk.bn for blk in self.blocks] + [self.fc_bn]

    def forward(self, x16: torch.Tensor, train_stats: bool = True, updates: Optional[int] = None):
        """x16 [B,H,W,8] fp16 -> (head32 [B,2z], ctx).  ``updates`` = number of running-stat updates this call
        stands for (the WAE scripts run the same encoder pass two or three times per step)."""
        acts, raws, svs = [x16], [], []
        h = x16
        upd = (1 if train_stats else 0) if updates is None else updates
        for blk in self.blocks:
            raw, done = blk.conv_forward(h)
            if done:
                h, raw, sv = raw, None, None
            else:
                h, sv = blk.bn.forward(raw, relu=True, updates=upd, stat_acc=blk.conv.take_stats())
            raws.append(raw)
            svs.append(sv)
            acts.append(h)
        flat = h.reshape(h.shape[0], -1)
        raw_fc, _ = self.fc.forward(flat)
        hfc, svfc = self.fc_bn.forward(raw_fc, relu=True, updates=upd)
        head32 = self.heads.forward(hfc)
        return head32, dict(acts=acts, raws=raws, svs=svs, flat=flat, raw_fc=raw_fc, hfc=hfc, svfc=svfc)

    def _backward(self, ctx, dhead16: torch.Tensor, scale: float, after_fc=None, after_fc_join: bool = True):
        """Accumulate encoder parameter gradients of (1/scale)*<dhead16, head>.  ``after_fc`` is called once the
        gradients of fc.0 / fc.1 / l_mu / l_var -- the tail of the flat buffer from ``fc.0.weight`` on, 93 % of its
        bytes -- are issued, so a data-parallel run can start reducing them under the conv backward;
        ``after_fc_join`` first joins the side stream they were issued on (a hook that itself runs on the side stream
        does not need that)."""
        dh = self.heads.backward(ctx["hfc"], dhead16, scale)
        draw_fc, _ = self.fc_bn.backward(ctx["raw_fc"], dh, ctx["svfc"], True, scale)
        self.fc.wgrad(ctx["flat"], draw_fc, scale)
        if after_fc is not None:
            if after_fc_join:
                join_side()                             # fc.0 weight gradient (side stream) is final
            after_fc()
        dflat, _ = self.fc.dgrad(draw_fc)
        d = dflat.reshape(ctx["acts"][3].shape)
        stat = None
        one, n = (Cot(0, scale, True),), d.shape[0]
        raws, svs = ctx["raws"], ctx["svs"]
        # Issue order inside a layer: the data gradient (main stream: the next link of the backward chain) BEFORE the weight
        # gradient (side stream) -- both become ready at the same moment, and the one issued first gets the free CUs first
        # (same-call A/B of the order, three pairs: 6.540-6.546 ms against 6.562-6.593 per step).
        for i in (2, 1, 0):
            blk = self.blocks[i]
            draw = torch.empty_like(d)
            _bn_backward_blocks(blk.bn, raws[i], [svs[i]], one, n, d, draw, stat)
            if i > 0:
                _, hi, wi, _ = ctx["acts"][i].shape
                d, stat = blk.dgrad_below(draw, self.blocks[i - 1], raws[i - 1], [(0, svs[i - 1])], hi, wi)
            blk.conv.wgrad(ctx["acts"][i], draw, scale)


class CognitiveEncoderNet(_JoinedBackward):
    def __init__(self, cfg: ArchConfig, n_voxels: int, device):
        self.cfg, self.n_voxels = cfg, n_voxels
        self.group = FlatGroup(cognitive_encoder_spec(cfg, n_voxels), device)
        g = self.group
        self.fc1 = DenseLayer(g, "fc1.0.weight", None, n_voxels, 1024)
        self.fc1_bn = BatchNorm(g, "fc1.1.", 1024)
        self.heads = FusedHeads(g, 1024, cfg.latent_dim)

    def all_bns(self):
        return [self.fc1_bn]

    def forward(self, fmri16: torch.Tensor, train_stats: bool = True, updates: Optional[int] = None):
        raw, _ = self.fc1.forward(fmri16)
        upd = (1 if train_stats else 0) if updates is None else updates
        h, sv = self.fc1_bn.forward(raw, relu=True, updates=upd)
        return self.heads.forward(h), dict(x=fmri16, raw=raw, h=h, sv=sv)

    def _backward(self, ctx, dhead16, scale):
        dh = self.heads.backward(ctx["h"], dhead16, scale)
        draw, _ = self.fc1_bn.backward(ctx["raw"], dh, ctx["sv"], True, scale)
        self.fc1.wgrad(ctx["x"], draw, scale)


# ------------------------------------------------------------------------------------------------
class DecoderNet(_JoinedBackward):
    def __init__(self, cfg: ArchConfig, device, size: Optional[int] = None):
        self.cfg = cfg
        size = cfg.encoder_channels[2] if size is None else size
        self.group = FlatGroup(decoder_spec(cfg, size), device)
        g = self.group
        hw = cfg.fc_input * cfg.fc_input
        self.size0 = size
        self.fc = DenseLayer(g, "fc.0.weight", None, cfg.latent_dim, hw * size, out_perm=(size, hw))
        self.fc_bn = BatchNorm(g, "fc.1.", hw * size, perm=(size, hw))
        chans = [(size, size), (size, cfg.decoder_channels[1]), (cfg.decoder_channels[1], cfg.decoder_channels[2])]
        self.blocks = [ConvBlock(ConvLayer(g, f"conv.{i}.conv.weight", None, "deconv", ci, co, cfg.kernel_size, cfg.stride,
                                           cfg.padding, 1 if cfg.output_pad_dec[i] else 0),
                                 BatchNorm(g, f"conv.{i}.bn.", co)) for i, (ci, co) in enumerate(chans)]
        self.c3 = ConvLayer(g, "conv.3.0.weight", "conv.3.0.bias", "conv", cfg.decoder_channels[2],
                            cfg.decoder_channels[3], 5, 1, 2)

    def all_bns(self):
        return [self.fc_bn] + [blk.bn for blk in self.blocks]

    def forward(self, z16: torch.Tensor, groups: int, out: Optional[torch.Tensor] = None, train_stats: bool = True,
                stat_order=None, zscale: Optional[torch.Tensor] = None):
        """z16 [G*B, zp]: G independent decoder calls (own BN batch statistics each, reference
        models/vae_gan.py:279,282) executed as one batch.  ``stat_order`` = order in which the groups'
        running-stat updates are applied (the reference's call order).  ``zscale`` (device fp32 [>= G]): group g's rows
        hold zscale[g] * z (``ops.latent_ranged``: a latent whose sigma left fp16's range); None = all 1.
        Returns (images fp16 [G*B,H,W,8], ctx)."""
        GB = z16.shape[0]
        B = GB // groups
        f = self.cfg.fc_input
        upd = 1 if train_stats else 0
        order = list(range(groups)) if stat_order is None else list(stat_order)
        raw_fc, _ = self.fc.forward(z16)
        act_fc = torch.empty_like(raw_fc)
        grows = lambda t: [t[gi * B:(gi + 1) * B] for gi in range(groups)]
        # the call groups of one layer are ready together: with SyncBN their statistics travel in ONE all-reduce
        ins = None if zscale is None else [zscale[gi:gi + 1] for gi in range(groups)]
        sv_fc = self.fc_bn.forward_groups(grows(raw_fc), True, upd, grows(act_fc), [None] * groups, order, in_scales=ins)
        h = act_fc.reshape(GB, f, f, self.size0)
        acts, raws, svs = [h], [], []
        for blk in self.blocks:
            raw, done = blk.conv_forward(h, groups)
            if done:
                h, raw, sl = raw, None, [None] * groups
            else:
                h = torch.empty_like(raw)
                sl = blk.bn.forward_groups(grows(raw), True, upd, grows(h),
                                           [blk.conv.take_stats(gi) for gi in range(groups)], order)
            raws.append(raw)
            svs.append(sl)
            acts.append(h)
        y = self.c3.forward(h, ACT_TANH, out=out)
        return y, dict(z=z16, raw_fc=raw_fc, sv_fc=sv_fc, acts=acts, raws=raws, svs=svs, y=y, B=B, groups=groups,
                       zscale=zscale)

    def _backward(self, ctx, cot: torch.Tensor, entries: List[dict]):
        """cot [E*B,H,W,8] fp16 stacks E cotangent blocks w.r.t. the decoder output; entries[e] =
        dict(g=<forward group whose activations it belongs to>, scale=<float>, train=<accumulate param grads>,
        need_dz=<bool>).  Returns {e: dz fp32 [B, z] (true scale)} for entries with need_dz."""
        B = ctx["B"]
        cots = [Cot(en["g"], en["scale"], en["train"], need_dz=bool(en.get("need_dz"))) for en in entries]
        E = len(cots)
        rows = lambda t, i: t[i * B:(i + 1) * B]
        runs = _wgrad_runs(cots)
        y = ctx["y"]
        raws, svs = ctx["raws"], ctx["svs"]
        dpre = torch.empty_like(cot)
        for e, en in enumerate(cots):
            colsum = None
            if en.train:
                colsum = torch.empty(2 * pad8(self.c3.cout), dtype=torch.float32, device=cot.device)
            # the bias gradient of conv.3 rides in the fold of the column sums (its first cout entries)
            act_backward(rows(y, en.g), rows(cot, e), ACT_TANH, colsum, out=rows(dpre, e),
                         dbias=self.c3.bg if en.train else None, dbias_scale=1.0 / en.scale)
        _wgrad_blocks(self.c3, ctx["acts"][3], dpre, runs, B)
        _, hi, wi, _ = ctx["acts"][3].shape
        d = self.c3.dgrad(dpre, hi, wi)
        stat = None
        for i in (2, 1, 0):
            blk = self.blocks[i]
            draw = torch.empty_like(d)
            _bn_backward_blocks(blk.bn, raws[i], svs[i], cots, B, d, draw, stat)
            _, hi, wi, _ = ctx["acts"][i].shape
            if i > 0:
                # one statistics group per cotangent block: its forward call's rows of the saved tensor and statistics
                d, stat = blk.dgrad_below(draw, self.blocks[i - 1], raws[i - 1],
                                          [(en.g * B, svs[i - 1][en.g]) for en in cots], hi, wi)
            else:
                d = blk.conv.dgrad(draw, hi, wi)
            _wgrad_blocks(blk.conv, ctx["acts"][i], draw, runs, B)     # (after the data gradient: see EncoderNet._backward)
        dflat = d.reshape(E * B, -1)
        draw_fc = torch.empty_like(dflat)
        out = {}
        _bn_backward_blocks(self.fc_bn, ctx["raw_fc"], ctx["sv_fc"], cots, B, dflat, draw_fc, None)
        _wgrad_blocks(self.fc, ctx["z"], draw_fc, runs, B)
        for e, en in enumerate(cots):
            if en.need_dz:
                _, dz32 = self.fc.dgrad(rows(draw_fc, e).contiguous(), want32=True)
                out[e] = dz32 * (1.0 / en.scale)
                if ctx.get("zscale") is not None:
                    # the group's rows were stored as s * z: d/dz = s * d/d(stored rows)
                    out[e] *= ctx["zscale"][en.g:en.g + 1]
        return out


# ------------------------------------------------------------------------------------------------
class DiscriminatorNet(_JoinedBackward):
    def __init__(self, cfg: ArchConfig, device, recon_level: int = 3):
        # models/vae_gan.py:139-173: the 'REC' output is the RAW convolution output of block ``recon_level``.  Block 0 is
        # an nn.Sequential, which does not take the reference's ``lay(ten, True)`` call (TypeError), and a level past
        # the last block makes its forward return None: levels 1..3 are the ones the reference can run.
        if recon_level not in (1, 2, 3):
            raise ValueError(f"recon_level={recon_level}: the reference Discriminator works for levels 1, 2, 3 only "
                             "(level 0 raises a TypeError there, levels > 3 return None; models/vae_gan.py:164-173)")
        self.level = recon_level
        self.cfg = cfg
        self.group = FlatGroup(discriminator_spec(cfg), device)
        g = self.group
        d = cfg.discrim_channels
        self.c0 = ConvLayer(g, "conv.0.0.weight", "conv.0.0.bias", "conv", 3, d[0], 5, cfg.stride_gan, 2)
        self.blocks = []                    # blocks[i] = the reference's conv.{i + 1}
        cin = d[0]
        for i in (1, 2, 3):
            self.blocks.append(ConvBlock(ConvLayer(g, f"conv.{i}.conv.weight", None, "conv", cin, d[i], cfg.kernel_size,
                                                   cfg.stride, cfg.padding), BatchNorm(g, f"conv.{i}.bn.", d[i])))
            cin = d[i]
        hw = cfg.fc_input_gan * cfg.fc_input_gan
        self.fc0 = DenseLayer(g, "fc.0.weight", None, hw * cin, cfg.fc_output_gan, in_perm=(cin, hw))
        self.fc_bn = BatchNorm(g, "fc.1.", cfg.fc_output_gan)
        self.fc3 = DenseLayer(g, "fc.3.weight", "fc.3.bias", cfg.fc_output_gan, 1)

    def all_bns(self):
        return [blk.bn for blk in self.blocks] + [self.fc_bn]

    def reads_zero_tail(self) -> bool:
        """Whether the two-stream ``backward`` reads the ``zero_tail`` rows of stream B's starting cotangent (the sampled
        images' rows), i.e. whether the caller has to write those zeros: the join layer's data gradient skips them
        unless it runs with the BatchNorm-backward epilogue (ops._EPI_BWD; block 1's data gradient has none above it)."""
        return self.level > 1 and ops._EPI_BWD

    def forward(self, x16: torch.Tensor, train_stats: bool = True, conv_updates: int = 2, fc_updates: int = 1,
                head: bool = True):
        """x16 [3B,H,W,8] = cat(orig, predicted, sampled).  One pass produces both reference outputs:
        the raw conv-3 features ('REC', models/vae_gan.py:166-173) and the class logits ('GAN', :176-183).
        Conv BN layers receive the reference's two running-stat updates per step in the fused
        step; the per-mode API calls pass conv_updates=1 and head=False for 'REC'."""
        a0 = self.c0.forward(x16, ACT_RELU)
        acts, raws, svs = [a0], [], []
        h = a0
        lv = self.level
        for li, blk in enumerate(self.blocks):
            if not head and li >= lv:
                break                     # a 'REC' call ends at block ``recon_level`` (models/vae_gan.py:166-173)
            raw, done = blk.conv_forward(h, keep_raw=li == lv - 1)   # (block ``recon_level``'s RAW output is 'REC')
            if done:
                h, raw, sv = raw, None, None
            else:
                # one pass standing for the reference's REC + GAN passes (conv_updates = 2): the REC pass never reaches
                # the blocks above ``recon_level``, they take the GAN pass's update only
                upd = conv_updates if li < lv else min(conv_updates, 1)
                h, sv = blk.bn.forward(raw, relu=True, updates=upd if train_stats else 0, stat_acc=blk.conv.take_stats())
            raws.append(raw)
            svs.append(sv)
            acts.append(h)
        ctx = dict(x=x16, acts=acts, raws=raws, svs=svs)
        if not head:
            return raws[lv - 1], None, ctx
        return raws[lv - 1], self.forward_head(ctx, train_stats, fc_updates), ctx

    def forward_head(self, ctx, train_stats: bool = True, fc_updates: int = 1):
        """The 'GAN' head (flatten -> fc.0 -> BN1d -> ReLU -> fc.3, models/vae_gan.py:176-183) on the conv activations of
        an earlier ``forward(..., head=False)`` (``ctx``, completed in place): class logits [3B, 1] fp32."""
        h = ctx["acts"][3]
        flat = h.reshape(h.shape[0], -1)
        raw_fc, _ = self.fc0.forward(flat)
        hfc, svfc = self.fc_bn.forward(raw_fc, relu=True, updates=fc_updates if train_stats else 0)
        _, logit32 = self.fc3.forward(hfc, ACT_NONE, want16=False, want32=True)
        ctx.update(flat=flat, raw_fc=raw_fc, hfc=hfc, svfc=svfc)
        return logit32

    def conv_running_again(self, ctx, updates: int = 1):
        """Apply the conv blocks' BatchNorm running-statistics update once more with the batch statistics saved in ``ctx``
        (a repeated forward call on the same input, see BatchNorm.update_running_again)."""
        for blk, sv in zip(self.blocks, ctx["svs"]):
            if sv is not None:
                blk.bn.update_running_again(sv, updates)

    def _backward(self, ctx, dlogit16: Optional[torch.Tensor], scale_a: float, dfeat16: Optional[torch.Tensor],
                 scale_b: float, train: bool, img_rows: Optional[slice], img_streams=(True, True),
                 train_b: bool = False, stack: Optional[torch.Tensor] = None, zero_tail: int = 0):
        """Two cotangent streams through one saved forward:
             A: d(sum bce)/d logit  (dlogit16 [3B,8], scale_a) -- accumulates discriminator grads if ``train``
             B: d(sum mse)/d raw features of block ``recon_level`` (dfeat16 [3B,h,w,c], scale_b) -- data gradient only
           ``stack`` [6B,h,w,c]: the buffer ``dfeat16`` is the second half of; ``zero_tail``: that many last rows of
           ``dfeat16`` are exact zeros (both from steps._start_cotangents).
           With both streams and ``recon_level`` L < 3, A runs alone through the head and blocks 3 .. L+1 (one-stream
           BatchNorm backward, its weight gradients) and B joins at the BatchNorm backward into block L's raw output:
           that pass writes A's rows into the first half of ``stack``; from block L down both streams run together.
           Returns (dimg_A, dimg_B): cotangents w.r.t. input images ``img_rows`` (None if not requested)."""
        n3 = ctx["x"].shape[0]
        join = self.level - 1               # block whose raw output stream B enters at (index into blocks / raws)
        both = dlogit16 is not None and dfeat16 is not None
        # caller-provided stack [A rows | B rows] with B already in place (steps._start_cotangents): A goes into its
        # first half and the two-stream batch needs no concatenation copy
        if stack is not None and (not both or stack.shape[0] != 2 * n3):
            stack = None
        sa = Cot(0, scale_a, train, img_streams[0])
        sb = Cot(0, scale_b, train_b, img_streams[1])
        streams, d, late = [], None, None
        if dlogit16 is not None:
            half = stack[:n3].reshape(ctx["raws"][2].shape) if (stack is not None and join == 2) else None
            d = self._backward_head(ctx, dlogit16, sa, half)
            streams.append(sa)
        if dfeat16 is not None:
            db = dfeat16.reshape(ctx["raws"][join].shape)
            if both and join < 2:
                late = (sb, db)              # stream B while stream A is still alone above the join
            else:
                streams.append(sb)
                if both:
                    d = stack.reshape((2 * n3,) + tuple(db.shape[1:])) if stack is not None else torch.cat([d, db], 0)
                else:
                    d = db
        # the first cotangent enters at block 3's raw output; a 'REC' call alone at block ``recon_level``'s
        top = 2 if dlogit16 is not None else join
        d, streams = self._backward_blocks(ctx, d, streams, late, top, stack, zero_tail)
        outs = self._backward_images(ctx, d, streams, img_rows, zero_tail)
        return (outs[0] if dlogit16 is not None else None), (outs[-1] if dfeat16 is not None else None)

    def _backward_head(self, ctx, dlogit16, sa: Cot, out: Optional[torch.Tensor]):
        """Stage 1 of ``_backward``: stream A through fc.3, the BatchNorm1d, fc.0 and block 3's BatchNorm.  Returns the
        cotangent of block 3's raw output, written into ``out`` (the first half of the caller's stack) where given."""
        pscale = sa.scale if sa.train else None
        if sa.train:
            self.fc3.wgrad(ctx["hfc"], dlogit16, sa.scale)
            self.fc3.bias_grad(dlogit16, sa.scale)
        dh, _ = self.fc3.dgrad(dlogit16)
        draw_fc, _ = self.fc_bn.backward(ctx["raw_fc"], dh, ctx["svfc"], True, pscale)
        if sa.train:
            self.fc0.wgrad(ctx["flat"], draw_fc, sa.scale)
        dflat, _ = self.fc0.dgrad(draw_fc)
        d3 = dflat.reshape(ctx["acts"][3].shape)
        if out is None:
            out = torch.empty_like(d3)
        _bn_backward_blocks(self.blocks[2].bn, ctx["raws"][2], [ctx["svs"][2]], (sa,), d3.shape[0], d3, out, None)
        return out

    def _backward_blocks(self, ctx, d, streams, late, top: int, stack, zero_tail: int):
        """Stage 2 of ``_backward``: from block ``top`` down to block 1 (``blocks[top] .. blocks[0]``), per block its data
        gradient, its weight gradients and the BatchNorm backward of the block below.  ``late`` = (stream B, its
        cotangent) while A is alone above the join.  Returns (cotangent of block 1's raw output [S*3B, ...], streams)."""
        n3 = ctx["x"].shape[0]
        join = self.level - 1
        acts, raws, svs = ctx["acts"], ctx["raws"], ctx["svs"]
        runs = _wgrad_runs(streams)
        for li in range(top, 0, -1):
            blk, below = self.blocks[li], self.blocks[li - 1]
            S = len(streams)
            _, hi, wi, _ = acts[li].shape
            if li == join and S > 1 and zero_tail and not ops._EPI_BWD:
                # stream B entered at block ``recon_level``'s raw output with exact zeros on the sampled images' rows
                # -- the last rows of the stack: that block's data gradient skips them
                dact, stat = _dgrad_live(blk.conv, d, d.shape[0] - zero_tail, hi, wi), None
            else:
                # one statistics group per cotangent stream (all read the same saved forward tensor)
                dact, stat = blk.dgrad_below(d, below, raws[li - 1], [(0, svs[li - 1])] * S, hi, wi)
            _wgrad_blocks(blk.conv, acts[li], d, runs, n3)      # (after the data gradient: see EncoderNet._backward)
            joining = late is not None and li - 1 == join
            # stream B joins here: A's BatchNorm backward into block ``recon_level``'s raw output writes the first half of
            # the caller's stack, whose second half already holds B (no concatenation copy)
            dn = stack[:n3].reshape(dact.shape) if (joining and stack is not None) else torch.empty_like(dact)
            _bn_backward_blocks(below.bn, raws[li - 1], [svs[li - 1]], streams, n3, dact, dn, stat)
            d = dn
            if joining:
                d = stack.reshape((2 * n3,) + tuple(dn.shape[1:])) if stack is not None else torch.cat([dn, late[1]], 0)
                streams, late = streams + [late[0]], None
                runs = _wgrad_runs(streams)
        # block 1's weight gradients are issued here, BEFORE conv.1's data gradient (the image side's first launch)
        _wgrad_blocks(self.blocks[0].conv, acts[0], d, runs, n3)
        return d, streams

    def _backward_images(self, ctx, d, streams, img_rows: Optional[slice], zero_tail: int):
        """Stage 3 of ``_backward``: conv.1's data gradient, conv.0 (bias + ReLU).  Returns per stream the cotangent
        w.r.t. the input images ``img_rows``, or None."""
        n3 = ctx["x"].shape[0]
        S = len(streams)
        rows = lambda t, i: t[i * n3:(i + 1) * n3]
        conv1 = self.blocks[0].conv
        # Below the last BatchNorm the images are independent, so a stream that does not train the discriminator only
        # needs the rows whose image gradient is wanted.
        a0 = ctx["acts"][0]
        _, hi, wi, _ = a0.shape
        full = slice(0, n3)
        need = [full if s.train else (img_rows if (img_rows is not None and s.img) else None) for s in streams]
        # conv0's ReLU backward rides in the epilogue of conv1's data gradient where its kernel has one (act_applied),
        # and the bias gradient comes out of the weight-gradient kernel: no pass over the 64 x 64 x 32 cotangent
        masked = [False] * S
        if all(nd == full for nd in need):
            dact = conv1.dgrad(d, hi, wi)
            dacts = [rows(dact, si) for si in range(S)]
        else:
            dacts = []
            for si, nd in enumerate(need):
                if nd is None:
                    dacts.append(None)
                    continue
                ds = rows(d, si)[nd]
                live = ds.shape[0] - zero_tail
                if self.level == 1 and si == 1 and nd.stop == n3 and 0 < live < ds.shape[0]:
                    # recon_level 1: stream B entered at block 1's raw output, this is the join layer's data gradient --
                    # the sampled images' rows (the last of the stack) are exact zeros and are skipped
                    dacts.append(_dgrad_live(conv1, ds, live, hi, wi, relu_y=a0[nd][:live]))
                else:
                    dacts.append(conv1.dgrad(ds, hi, wi, relu_y=a0[nd]))
                masked[si] = conv1.act_applied
        outs = []
        for si, s in enumerate(streams):
            if need[si] is None:
                outs.append(None)
                continue
            if masked[si]:
                dpre = dacts[si]
                if s.train:
                    self.c0.wgrad(ctx["x"], dpre, s.scale, bias_too=True)
            else:
                colsum = None
                if s.train:
                    colsum = torch.empty(2 * self.c0.coutp, dtype=torch.float32, device=d.device)
                dpre = act_backward(a0[need[si]], dacts[si], ACT_RELU, colsum,
                                    dbias=self.c0.bg if s.train else None, dbias_scale=1.0 / s.scale)
                if s.train:
                    self.c0.wgrad(ctx["x"], dpre, s.scale)
            if img_rows is not None and s.img:
                _, xh, xw, _ = ctx["x"].shape
                sub = dpre[img_rows] if need[si] == full else dpre
                outs.append(self.c0.dgrad(sub.contiguous(), xh, xw))
            else:
                outs.append(None)
        return outs


# ------------------------------------------------------------------------------------------------
class WaeDiscriminatorNet(_JoinedBackward):
    """Latent-space discriminator MLP z -> 512 -> 512 -> 512 -> 512 -> 1 (models/vae_gan.py:499-529)."""

    def __init__(self, cfg: ArchConfig, device, dim_h: int = 512):
        self.cfg = cfg
        self.group = FlatGroup(wae_discriminator_spec(cfg, dim_h), device)
        dims = [cfg.latent_dim, dim_h, dim_h, dim_h, dim_h, 1]
        self.layers = [DenseLayer(self.group, f"main.{idx}.weight", f"main.{idx}.bias", dims[j], dims[j + 1])
                       for j, idx in enumerate((0, 2, 4, 6, 8))]

    def all_bns(self):
        return []

    # The fused kernels (csrc/mlp.hip: one launch forward, one for the backward data path) take this network's own
    # packed weights; FMRI_MLP=off (or a width they do not cover) keeps the layer-by-layer path below.
    def _fused_ok(self, z16) -> bool:
        dims = [l.n_out for l in self.layers]
        return (_MLP_ON and len(self.layers) == 5 and dims[:4] == [512] * 4 and dims[4] == 1
                and z16.shape[1] % 64 == 0 and 64 <= z16.shape[1] <= 256)

    @staticmethod
    def _ptrs(tensors):
        arr = (ctypes.c_void_p * len(tensors))()
        for i, t in enumerate(tensors):
            arr[i] = None if t is None else t.data_ptr()
        return arr

    def forward(self, z16: torch.Tensor):
        if self._fused_ok(z16):
            M, Zp = z16.shape
            dev = z16.device
            ws = [l.pw_f.get() for l in self.layers]
            kps = (ctypes.c_int * 5)(*[l.pw_f.kpads[0] for l in self.layers])
            hbuf = torch.empty(4, M, 512, dtype=torch.float16, device=dev)
            logit32 = torch.empty(M, 1, dtype=torch.float32, device=dev)
            lib.call("fmri_mlp_fwd", _P(z16), M, Zp, 512, self._ptrs(ws), kps, self._ptrs([l.b for l in self.layers]),
                     self._ptrs([hbuf[i] for i in range(4)]), _P(logit32))
            return logit32, dict(hs=[z16] + [hbuf[i] for i in range(4)], fused=True)
        hs = [z16]
        h = z16
        for l in self.layers[:-1]:
            h, _ = l.forward(h, ACT_RELU)
            hs.append(h)
        _, logit32 = self.layers[-1].forward(h, ACT_NONE, want16=False, want32=True)
        return logit32, dict(hs=hs)

    def _backward(self, ctx, dlogit16, scale, train: bool, need_dz: bool):
        if ctx.get("fused"):
            return self._backward_fused(ctx, dlogit16, scale, train, need_dz)
        d = dlogit16
        hs = ctx["hs"]
        for j in range(4, -1, -1):
            l = self.layers[j]
            if train:
                l.wgrad(hs[j], d, scale)
                l.bias_grad(d, scale)
            if j == 0 and not need_dz:
                return None
            if j == 0:
                _, dz32 = l.dgrad(d, want32=True)
                return dz32 * (1.0 / scale)
            dn, _ = l.dgrad(d)
            d = act_backward(hs[j], dn, ACT_RELU)
        return None

    def _backward_fused(self, ctx, dlogit16, scale, train: bool, need_dz: bool):
        """One launch for the data path (cotangents of the four hidden pre-activations, bias gradients, dz); the five
        weight gradients -- reductions over all rows -- are fmri_wgrad launches on the side stream."""
        hs = ctx["hs"]
        z16 = hs[0]
        M, Zp = z16.shape
        dev = z16.device
        Z = self.layers[0].k_in
        dbuf = torch.empty(4, M, 512, dtype=torch.float16, device=dev)
        dz32 = torch.empty(M, Z, dtype=torch.float32, device=dev) if need_dz else None
        wds = [(self.layers[i].pw_d.get() if (i > 0 or need_dz) else None) for i in range(4)]
        kpd = (ctypes.c_int * 4)(*[self.layers[i].pw_d.kpads[0] for i in range(4)])
        det = ops.deterministic()        # bias gradients as fixed-order column sums instead of the kernel's atomics
        dbias = self._ptrs([l.bg for l in self.layers]) if (train and not det) else None
        lib.call("fmri_mlp_bwd", _P(dlogit16), dlogit16.shape[1], M, Zp, Z, 512, self._ptrs(hs[1:5]),
                 _P(self.layers[4].pw_f.get()), self._ptrs(wds), kpd, self._ptrs([dbuf[i] for i in range(4)]), dbias,
                 _P(dz32), 1.0 / scale)
        if train:
            deltas = [dbuf[0], dbuf[1], dbuf[2], dbuf[3], dlogit16]
            for j in range(5):
                self.layers[j].wgrad(hs[j], deltas[j], scale)
                if det:
                    self.layers[j].bias_grad(deltas[j], scale)
        return dz32
