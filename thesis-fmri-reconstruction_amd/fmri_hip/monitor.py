"""Opt-in numerics monitor of the fused training steps (``monitor=True`` of Stage1Step, CognitiveStep, WaeStep,
DualStage1Step).

Everything is computed on the device, inside the step, in whatever launch mode the step runs (eager ``step()``,
``capture()``, ``capture_forward()``, the two-stream backward):

  * the optimizer of every sub-network writes the statistics of the gradient it consumed (true scale: the device
    normalisation factor divided out, before the clamp) and of the weights it wrote -- fmri_apply_batch_stats +
    fmri_stat_fold on the fused path, fmri_tensor_stats around fmri_rmsprop_dev / fmri_adam_dev otherwise;
  * every BatchNorm backward counts the dx values its saturating fp16 store clipped and the NaNs it stored
    (fmri_bn_*_cnt, one integer atomic per wave);
  * the step's tail takes the encoder head (mu | logvar), the loss slots and the latent range scales ``zs``.

The device block is allocated once, at construction, so that a recorded step writes the same memory at every replay;
``zero()`` clears it at the start of the step's forward pass, where the step clears its scalar block.  ``decode`` turns a
host copy of the block into the dict of ``numerics()``; it is pure host code.

Data parallel: the gradient statistics are taken after the SUM all-reduce, so every rank reports the same values; the
BatchNorm counts and the latent statistics are those of the rank's own rows.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib

_P = lib.ptr

# one fmri_stat record (include/fmri_hip.h)
STAT_DTYPE = np.dtype([("sumsq", "<f8"), ("max", "<f4"), ("min", "<f4"), ("max_abs", "<f4"), ("nonfinite", "<i4"),
                       ("clamped", "<i4"), ("written", "<i4")])
assert STAT_DTYPE.itemsize == lib.STAT_BYTES
N_ZS = 4            # latent range scales: one per decoder call group (steps.S_ZMAX)


@dataclass(frozen=True)
class Layout:
    """Byte layout of the device block: [net records: (gradient, weights) per sub-network | latent records: mu, logvar |
    one record per loss-slot segment | zs: N_ZS fp32 | BatchNorm counters: (saturated, NaN) int32 per layer]."""
    nets: Tuple[str, ...]
    bns: Tuple[str, ...]
    n_loss: int

    @property
    def n_rec(self) -> int:
        return 2 * len(self.nets) + 2 + self.n_loss

    def net_off(self, i: int) -> int:
        return 2 * i * lib.STAT_BYTES

    @property
    def latent_off(self) -> int:
        return 2 * len(self.nets) * lib.STAT_BYTES

    @property
    def loss_off(self) -> int:
        return self.latent_off + 2 * lib.STAT_BYTES

    @property
    def zs_off(self) -> int:
        return self.n_rec * lib.STAT_BYTES

    @property
    def bn_off(self) -> int:
        return self.zs_off + 4 * N_ZS

    @property
    def nbytes(self) -> int:
        return self.bn_off + 8 * len(self.bns)


def _f(v) -> float:
    return float(v)


def decode(buf, layout: Layout) -> Dict[str, object]:
    """Host copy of the device block (bytes / uint8 array) -> the dict of ``numerics()``."""
    raw = np.frombuffer(bytes(np.asarray(buf, dtype=np.uint8).tobytes()), dtype=np.uint8)
    if raw.size != layout.nbytes:
        raise ValueError(f"monitor block: {raw.size} bytes, layout wants {layout.nbytes}")
    rec = np.frombuffer(raw[:layout.zs_off].tobytes(), dtype=STAT_DTYPE)
    zs = np.frombuffer(raw[layout.zs_off:layout.bn_off].tobytes(), dtype="<f4")
    bn = np.frombuffer(raw[layout.bn_off:].tobytes(), dtype="<i4").reshape(-1, 2)
    grad, param = {}, {}
    for i, name in enumerate(layout.nets):
        g, p = rec[2 * i], rec[2 * i + 1]
        up = bool(g["written"])
        grad[name] = dict(updated=up,
                          norm=math.sqrt(float(g["sumsq"])) if up else None,
                          max_abs=_f(g["max_abs"]) if up else None,
                          nonfinite=int(g["nonfinite"]) if up else None,
                          clamped=int(g["clamped"]) if up else None)
        pw = bool(p["written"])
        param[name] = dict(max_abs=_f(p["max_abs"]) if pw else None, nonfinite=int(p["nonfinite"]) if pw else None)
    k = 2 * len(layout.nets)
    mu, lv = rec[k], rec[k + 1]
    lat_ok = bool(mu["written"]) and bool(lv["written"])
    latent = dict(logvar_max=_f(lv["max"]) if lat_ok else None, logvar_min=_f(lv["min"]) if lat_ok else None,
                  mu_max_abs=_f(mu["max_abs"]) if lat_ok else None,
                  nonfinite=int(mu["nonfinite"]) + int(lv["nonfinite"]) if lat_ok else None,
                  # -log2 of the power-of-two scale each decoder call group's latent rows were stored at (0: healthy)
                  range_exp=[(-math.log2(float(z)) + 0.0) if z > 0 else 0.0 for z in zs])
    losses = rec[k + 2:k + 2 + layout.n_loss]
    losses_finite = bool(all(r["written"] and r["nonfinite"] == 0 for r in losses))
    bn_backward = {name: dict(saturated=int(bn[i, 0]), nonfinite=int(bn[i, 1])) for i, name in enumerate(layout.bns)}
    return dict(grad=grad, param=param, bn_backward=bn_backward, latent=latent, losses_finite=losses_finite)


def tensor_stats(segs: Sequence[dict], ws: torch.Tensor):
    """fmri_tensor_stats over up to 8 segments, each a dict of lib.StatSeg fields (x / div / gate / out: pointers)."""
    n = len(segs)
    if n < 1 or n > lib.STAT_MAX_SEGS:
        raise ValueError("tensor_stats: 1 to 8 segments")
    arr = (lib.StatSeg * n)()
    for a, s in zip(arr, segs):
        a.x, a.rows, a.cols = s["x"], int(s["rows"]), int(s["cols"])
        a.ld = int(s.get("ld", s["cols"]))
        a.div, a.gate, a.out = s.get("div"), s.get("gate"), s["out"]
        a.scale, a.clamp = float(s.get("scale", 1.0)), float(s.get("clamp", 0.0))
    lib.call("fmri_tensor_stats", arr, n, _P(ws))


class Monitor:
    """The device block of one step object, its hooks and its decoder."""

    def __init__(self, device, nets: Sequence[Tuple[str, object]], bns: Sequence[Tuple[str, object]], n_loss: int):
        """``nets``: (name, _Optim) of every sub-network the step may update; ``bns``: (name, ops.BatchNorm) of every
        BatchNorm layer the step back-propagates through; ``n_loss``: loss-slot segments passed to ``tail``."""
        L = lib.load()
        self.layout = Layout(tuple(n for n, _ in nets), tuple(n for n, _ in bns), int(n_loss))
        self.device = torch.device(device)
        self.blk = torch.zeros(self.layout.nbytes, dtype=torch.uint8, device=self.device)
        # workspaces of the optimizers' statistics (which may run on the side stream) and of the tail
        self.ws = torch.empty(L.fmri_tensor_stats_ws_bytes(lib.STAT_MAX_SEGS), dtype=torch.uint8, device=self.device)
        self.ws_tail = torch.empty_like(self.ws)
        self.zs = self.blk[self.layout.zs_off:self.layout.bn_off].view(torch.float32)
        base = self.blk.data_ptr()
        for i, (_, opt) in enumerate(nets):
            opt.stats = (self, base + self.layout.net_off(i))
        for i, (_, bn) in enumerate(bns):
            bn.mon_cnt = base + self.layout.bn_off + 8 * i

    def zero(self):
        self.blk.zero_()

    def grad_stats(self, g: torch.Tensor, gdev, clamp: float, flag, out: int):
        """Before a non-fused optimizer update: the true-scale gradient g / *gdev it is about to consume."""
        tensor_stats([dict(x=_P(g), rows=1, cols=g.numel(), div=_P(gdev), gate=_P(flag), out=out, clamp=clamp)],
                     self.ws)

    def param_stats(self, w: torch.Tensor, flag, out: int):
        """After a non-fused optimizer update: the weights it wrote (record ``out`` + 1)."""
        tensor_stats([dict(x=_P(w), rows=1, cols=w.numel(), gate=_P(flag), out=out + lib.STAT_BYTES)], self.ws)

    def tail(self, head32: Optional[torch.Tensor], Z: int, losses: List[torch.Tensor], zs: Optional[torch.Tensor]):
        """The step's encoder head [B, 2Z] fp32 (mu | logvar), its loss slots and latent range scales."""
        base = self.blk.data_ptr()
        lay = self.layout
        segs = []
        if head32 is not None:
            B = head32.shape[0]
            for j in range(2):
                segs.append(dict(x=head32.data_ptr() + 4 * j * Z, rows=B, cols=Z, ld=head32.shape[1],
                                 out=base + lay.latent_off + j * lib.STAT_BYTES))
        for j, t in enumerate(losses):
            segs.append(dict(x=_P(t), rows=1, cols=t.numel(), out=base + lay.loss_off + j * lib.STAT_BYTES))
        tensor_stats(segs, self.ws_tail)
        if zs is not None:
            self.zs.copy_(zs)

    def numerics(self) -> Dict[str, object]:
        torch.cuda.synchronize(self.device)
        return decode(self.blk.cpu().numpy(), self.layout)


class Monitored:
    """Mixin of the step classes: ``numerics()`` / ``numerics_block()`` and the construction of the monitor."""

    mon: Optional[Monitor] = None

    def _init_monitor(self, on: bool, nets, n_loss: int):
        """``nets``: (state-dict prefix, _Optim, network or None) per sub-network."""
        if not on:
            self.mon = None
            return
        bns = []
        for pre, _, net in nets:
            if net is not None and hasattr(net, "all_bns"):
                bns += [(f"{pre}.{bn.prefix.rstrip('.')}", bn) for bn in net.all_bns()]
        self.mon = Monitor(self.device, [(pre, opt) for pre, opt, _ in nets], bns, n_loss)

    def numerics(self) -> Dict[str, object]:
        """Statistics of the most recent step (syncs).  ``grad[net]``: norm (double-precision sum of squares of the finite
        elements), max_abs (finite elements), nonfinite, clamped (elements the +-clamp bound changed) of the true-scale
        gradient the optimizer consumed, after the data-parallel all-reduce (identical on every rank); ``updated`` False
        and None fields for a sub-network the gate / the mode did not update.  ``param[net]``: max_abs, nonfinite of the
        new weights (None when not updated).  ``bn_backward[layer]``: dx values the saturating fp16 store clipped /
        NaNs it stored, this rank.  ``latent``: logvar max / min, max |mu|, non-finite count of this rank's encoder head
        and range_exp[g] = -log2 of decoder group g's latent range scale (0: healthy).  ``losses_finite``: every loss slot
        of the step is finite."""
        if self.mon is None:
            raise RuntimeError("numerics(): the step was constructed with monitor=False")
        return self.mon.numerics()

    def numerics_block(self) -> torch.Tensor:
        """The raw device block (no sync); ``monitor.decode(block.cpu().numpy(), step.mon.layout)`` reads it."""
        if self.mon is None:
            raise RuntimeError("numerics_block(): the step was constructed with monitor=False")
        return self.mon.blk
