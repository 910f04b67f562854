"""Exponential moving average of the weights of a fused step, kept on the device (csrc/ema.hip; include/fmri_hip.h
fmri_ema_update).

    ema = WeightEma(decay=0.999)                     # warmup=True, start=0, nets=None: what the eval forward uses
    step = Stage1Step(cfg, dev, rng=g, feed=feed, ema=ema)
    replay = step.capture()
    for _ in range(steps): replay()                  # the averages follow inside the graph
    ev = Evaluator(step, val, 64, rng=g_eval, weights="ema");  ev.run()
    torch.save(step.ema_state_dict(), path)          # the reference's keys: loads into the drop-in modules and the steps

Per step and element, in fp32: ``e = e + (1 - d) * (w - e)`` with ``d = decay_at(t)``: 0 while ``t < start`` (the shadow is
a copy), else ``min(decay, (1 + s) / (10 + s))`` with ``s = t - start`` under ``warmup``, else ``decay``.  ``t`` counts the
steps on the device.

What is averaged: of every chosen network the flat fp32 masters and the BatchNorm ``running_mean`` / ``running_var`` (of a
lazy BatchNorm the engine-order vectors, which are the live ones); ``num_batches_tracked`` is not.  The masters of a
network are updated right behind its optimizer update, on that update's stream (``_Optim.step``: whether or not the gate
let the update happen), the BatchNorm buffers of all networks in one launch at the end of the step, then the counter.

The shadows of a network start as a copy of its live values, and are copied again when the network is loaded from outside
(``load_state_dict`` / ``load_recipe``): an average continues from the checkpoint, not from the initialisation before it.

Nothing here synchronises with the host.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import struct
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import lib, ops
from .nets import refresh_net

_P = lib.ptr

EVAL_NETS = ("encoder", "decoder")       # what the eval-mode forward of every step class runs (fmri_hip/evaluate.py)


def decay_at(t: int, start: int, decay: float, warmup: bool) -> float:
    """The decay of step ``t`` as the kernel derives it (fmri_ema_decay_at: host code, no GPU)."""
    return float(lib.load().fmri_ema_decay_at(int(t), int(start), float(decay), 1 if warmup else 0))


class _Table:
    """(live, shadow) pairs one launch covers: the host table fmri_ema_update checks on every call and its device copy."""

    def __init__(self, pairs, device):
        self.pairs = list(pairs)
        self.host = (lib.EmaSeg * max(len(self.pairs), 1))()
        chunks = 0
        for row, (live, shadow) in zip(self.host, self.pairs):
            row.live, row.shadow, row.n, row.chunk0 = live.data_ptr(), shadow.data_ptr(), live.numel(), chunks
            chunks += -(-live.numel() // lib.EMA_CHUNK)
        self.n = sum(live.numel() for live, _ in self.pairs)
        self.dev = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).to(device)

    def update(self, state: torch.Tensor):
        lib.note(bytes=12.0 * self.n)            # read w, e; write e
        lib.call("fmri_ema_update", C.addressof(self.host), _P(self.dev), len(self.pairs), _P(state))

    def swap(self):
        lib.note(bytes=16.0 * self.n)
        lib.call("fmri_ema_swap", C.addressof(self.host), _P(self.dev), len(self.pairs))


def _decode(flat, off: int, shape, perm):
    """One state-dict entry out of a flat segment (a torch tensor or numpy array): the inverse of what
    ``_StepBase._group_segments`` lists -- an engine-order (HW, C0) vector goes back to the reference's (C0, HW)."""
    n = int(np.prod(shape)) if len(shape) else 1
    v = flat[off:off + n]
    if perm is not None:
        c0, hw = perm
        v = v.reshape(hw, c0).T
    return v.reshape(tuple(shape))


class WeightEma:
    """``decay`` in [0, 1); ``warmup``: ``min(decay, (1 + s) / (10 + s))`` over the first steps; ``start``: steps before it
    copy; ``nets``: names out of ``OPTIM_NAMES`` the step trains, default the trained ones among ``EVAL_NETS``.  One object
    belongs to one step (``ema=`` of the step classes)."""

    def __init__(self, decay: float = 0.999, warmup: bool = True, start: int = 0, nets: Optional[Sequence[str]] = None):
        from .step_base import OPTIM_NAMES
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"WeightEma: decay must be a number in [0, 1), got {decay!r}")
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or start < 0:
            raise ValueError(f"WeightEma: start must be an integer >= 0, got {start!r}")
        if nets is not None:
            nets = (nets,) if isinstance(nets, str) else tuple(nets)
            bad = [n for n in nets if n not in OPTIM_NAMES]
            if bad or len(set(nets)) != len(nets):
                raise ValueError(f"WeightEma: nets must be distinct names out of {OPTIM_NAMES}, got {nets!r}")
            nets = tuple(n for n in OPTIM_NAMES if n in nets)
        self.decay, self.warmup, self.start, self._asked = float(decay), bool(warmup), int(start), nets
        self.step = None

    # ---- construction (the step's ``_init_ema``) -----------------------------------------------------------------------
    def attach(self, step):
        from .step_base import OPTIM_NAMES
        if self.step is not None:
            raise ValueError("WeightEma: already attached to a step (an average belongs to one step)")
        optims = dict(zip(OPTIM_NAMES, step.optims))
        trained = [n for n in step._trained() if n in optims]
        nets = tuple(n for n in EVAL_NETS if n in trained) if self._asked is None else self._asked
        missing = [n for n in nets if n not in trained]
        if missing:
            raise ValueError(f"WeightEma: {type(step).__name__} does not train {missing} (it trains {trained}): a frozen "
                             "network has no average")
        if not nets:
            raise ValueError(f"WeightEma: {type(step).__name__} trains none of {EVAL_NETS}: name the networks with nets=")
        dev = step.device
        by_group = {id(n.group): n for n in step._state_nets()}
        prefix = {}
        for pre, n in step._state_groups():
            prefix.setdefault(id(n.group), pre)
        self.step, self.nets = step, nets
        self._net = {name: by_group[id(optims[name].g)] for name in nets}
        names = {prefix[id(self._net[name].group)]: name for name in nets}
        # (segment name, live, shadow, entries of the state dict it carries, network name), in _group_segments() order
        self._segs = []
        for seg, t, entries in step._group_segments():
            kind, _, rest = seg.partition(":")
            name = next((nm for pre, nm in names.items() if rest.startswith(pre)), None)
            if name is None or t.dtype != torch.float32:
                continue                         # another network's, or num_batches_tracked
            self._segs.append((seg, t, torch.empty_like(t), entries, name, kind == "group"))
        # [t, start, decay, warmup]: the fmri_ema_state block (decay as its fp32 bits)
        bits = struct.unpack("<i", struct.pack("<f", self.decay))[0]
        self.state = torch.tensor([0, self.start, bits, 1 if self.warmup else 0], dtype=torch.int32, device=dev)
        self._group_table = {name: _Table([(t, e) for _, t, e, _, nm, grp in self._segs if grp and nm == name], dev)
                             for name in nets}
        self._bn_table = _Table([(t, e) for _, t, e, _, _, grp in self._segs if not grp], dev)
        self._all_table = _Table([(t, e) for _, t, e, _, _, _ in self._segs], dev)
        self._seen: Dict[str, int] = {}
        self.prime()
        for name in nets:
            table = self._group_table[name]
            optims[name].ema = lambda table=table: table.update(self.state)

    def prime(self):
        """Host check at the start of every step: a network loaded from outside since the last look (FlatGroup.buf_version)
        gets its shadows copied from the loaded values."""
        for name, net in self._net.items():
            g = net.group
            if self._seen.get(name) == g.buf_version:
                continue
            for bn in net.all_bns():
                if bn._lazy:
                    bn._running_in()             # the engine-order vectors are the live ones: load them first
            for _, t, e, _, nm, _ in self._segs:
                if nm == name:
                    e.copy_(t)
            self._seen[name] = g.buf_version

    def mark_loaded(self):
        """``restore()``: the shadows are about to be overwritten with a state's -- nothing is pending any more."""
        for name, net in self._net.items():
            self._seen[name] = net.group.buf_version

    # ---- the step's launches ---------------------------------------------------------------------------------------------
    def finish(self):
        """End of a step, main stream: the BatchNorm buffers of all shadowed networks in one launch, then the counter."""
        self._bn_table.update(self.state)
        lib.call("fmri_counter_inc", _P(self.state))

    # ---- state ring ------------------------------------------------------------------------------------------------------
    def state_tensors(self) -> Dict[str, torch.Tensor]:
        out = {f"ema:{seg}": e for seg, _, e, _, _, _ in self._segs}
        out["ema:state"] = self.state
        return out

    def signature(self) -> str:
        return f"ema={self.decay!r},{self.warmup},{self.start},{'+'.join(self.nets)}"

    def layout(self) -> dict:
        """segment name -> [state-dict key, element offset, shape, (C0, HW) or None] per entry: what ``state_dict_of``
        needs to read the shadows of a TrainState (kept in its ``meta["host"]``)."""
        return {seg: [[key, int(off), list(shape), None if perm is None else list(perm)]
                      for key, off, shape, perm in entries] for seg, _, _, entries, _, _ in self._segs}

    # ---- reading ---------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The step's ``state_dict()`` with every shadowed entry taken from its shadow (device tensors, no sync)."""
        ops.join_side()
        self.prime()
        sd = self.step.state_dict()
        for _, _, e, entries, _, _ in self._segs:
            for key, off, shape, perm in entries:
                sd[key] = _decode(e, off, shape, perm).clone()
        return sd

    @staticmethod
    def state_dict_of(state) -> Dict[str, torch.Tensor]:
        """The same dict from a TrainState taken from a step with ``ema=`` (host tensors; no GPU)."""
        lay = state.meta["host"].get("ema")
        if lay is None:
            raise ValueError("WeightEma.state_dict_of: the state was taken from a step without ema=")
        sd = {k: v.clone() for k, v in state.model.items()}
        for seg, entries in lay.items():
            flat = state.engine[f"ema:{seg}"].numpy().reshape(-1)
            for key, off, shape, perm in entries:
                sd[key] = torch.from_numpy(np.ascontiguousarray(_decode(flat, off, shape, perm)).copy())
        return sd

    # ---- evaluation with the averaged weights ----------------------------------------------------------------------------
    def _swap(self):
        ops.join_side()
        self.prime()
        for net in self._net.values():
            if net.group.gq.pending or net.group.gq.materialized:
                raise RuntimeError("swapped() between backward() and apply(): weight gradients are still queued")
        self._all_table.swap()
        for net in self._net.values():
            net.group.version += 1
            refresh_net(net)

    @contextlib.contextmanager
    def swapped(self):
        """Inside: the shadowed networks run on their averaged weights and BatchNorm statistics (and the shadows hold the
        live ones).  Enqueues only: one exchange launch and the refresh of everything derived from the masters on entry, the
        same on exit -- which leaves masters, BatchNorm vectors and every packed fp16 copy bit for bit what they were."""
        self._swap()
        try:
            yield self
        finally:
            self._swap()
