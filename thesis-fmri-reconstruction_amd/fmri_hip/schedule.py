"""Device-side epoch-end schedules and the per-step training log of the fused steps (csrc/schedule.hip;
include/fmri_hip.h fmri_schedule for the arithmetic).

What the reference's loops do on the host around every step, moved to where the epoch of a fed step lives:

    sched = EpochSchedule(lr_gamma=0.98, decay_margin=1.0, decay_equilibrium=1.0, decay_mse=1.0)
    step = Stage1Step(cfg, dev, rng=g, feed=feed, schedule=sched, log=TrainLog(capacity=4096))
    replay = step.capture()
    for _ in range(steps):
        replay()                        # epoch boundaries included: no host work between replays
    h = step.history()                  # ONE sync: the last min(steps, capacity) steps, oldest first

``EpochSchedule``: the epoch-end block of the scripts (train/train_vgan_stage1.py:447-458 and its copies; ``StepLR`` of the
WAE scripts) as ONE launch of one thread in front of the feed's draws of every step.  The values a step uses are a pure
function of (base values at construction, decays, epoch of the batch the step draws): ``epoch`` iterations of that block in
float64, rounded to fp32 once, when written to ``_Optim.lr_dev`` / ``hp_dev[0:3]`` -- bit for bit what a host loop of Python
floats hands to ``set_hyper``.  The state lives in device memory, so the launch sits inside a recorded graph and follows
``DeviceFeed.set_position`` in either direction.

``TrainLog``: one launch at the very end of every step copies what ``logs()`` would have returned -- plus the epoch of the
batch and the learning rates -- into a device ring; ``history()`` reads it with one synchronisation.

Nothing here synchronises with the host except ``EpochSchedule.values`` and ``TrainLog.history`` / ``steps_logged``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib

_P = lib.ptr

KIND_F32, KIND_I32, KIND_I64 = 0, 1, 2              # fmri_trainlog_append's source kinds
_KIND = {torch.float32: KIND_F32, torch.int32: KIND_I32, torch.int64: KIND_I64}
MAX_COLUMNS = 64


class EpochSchedule:
    """``lr_gamma`` / ``lr_step``: torch's StepLR in its chainable form -- ``lr *= lr_gamma`` at every epoch end where the
    new epoch index is a multiple of ``lr_step`` (a repeated product, not ``gamma ** k``); ``lr_step=1`` is ExponentialLR.
    ``decay_margin`` / ``decay_equilibrium`` / ``decay_mse``: the factors of the VAE/GAN scripts, with their two clamps
    (``equilibrium = max(equilibrium, margin)`` after the decays, ``lambda_mse <= 1``); the WAE steps have none of the
    three and refuse a factor other than 1.  ``lr_mask``: one bool per entry of ``step.optims`` -- which follow the lr
    schedule; default: the optimizers ``set_hyper(lr=)`` touches (all of a WaeStep's).  ``beta`` is not scheduled.

    A schedule belongs to one step (``schedule=`` of the step classes) and needs that step's ``feed``.  While attached it
    owns the scheduled values: ``set_hyper`` of them and ``set_lr`` of a scheduled optimizer raise."""

    def __init__(self, lr_gamma: float = 1.0, lr_step: int = 1, decay_margin: float = 1.0,
                 decay_equilibrium: float = 1.0, decay_mse: float = 1.0, lr_mask: Optional[Sequence[bool]] = None):
        if int(lr_step) != lr_step or lr_step < 1:
            raise ValueError("EpochSchedule: lr_step must be an integer >= 1")
        self.lr_gamma, self.lr_step = float(lr_gamma), int(lr_step)
        self.decay_margin, self.decay_equilibrium, self.decay_mse = (float(decay_margin), float(decay_equilibrium),
                                                                     float(decay_mse))
        self.lr_mask = None if lr_mask is None else tuple(bool(m) for m in lr_mask)
        self.state: Optional[torch.Tensor] = None       # the device fmri_schedule, once attached
        self._base: Optional[lib.Schedule] = None

    def attach(self, feed, optims, default_mask: Sequence[bool], hp=None, hp_dev: Optional[torch.Tensor] = None):
        """(the step's ``_init_schedule``)  ``hp``: an object with margin / equilibrium / lambda_mse (the base values) and
        ``hp_dev`` the device block [lambda_mse, equilibrium, margin, beta] of a VAE/GAN step; None for a WAE step."""
        if self.state is not None:
            raise ValueError("EpochSchedule: already attached to a step (a schedule holds one step's state)")
        if len(optims) > lib.SCHED_MAX_LR:
            raise ValueError(f"EpochSchedule: at most {lib.SCHED_MAX_LR} optimizers")
        mask = tuple(default_mask) if self.lr_mask is None else self.lr_mask
        if len(mask) != len(optims):
            raise ValueError(f"EpochSchedule: lr_mask has {len(mask)} entries, the step has {len(optims)} optimizers")
        if hp is None and (self.decay_margin, self.decay_equilibrium, self.decay_mse) != (1.0, 1.0, 1.0):
            raise ValueError("EpochSchedule: this step has no margin / equilibrium / lambda_mse -- decay_margin, "
                             "decay_equilibrium and decay_mse must stay 1.0")
        s = lib.Schedule()
        for i, o in enumerate(optims):
            s.lr_base[i] = s.lr[i] = o.lr
        if hp is not None:
            s.margin_base = s.margin = float(hp.margin)
            s.equilibrium_base = s.equilibrium = float(hp.equilibrium)
            s.lambda_mse_base = s.lambda_mse = float(hp.lambda_mse)
        s.lr_gamma, s.lr_step = self.lr_gamma, self.lr_step
        s.decay_margin, s.decay_equilibrium, s.decay_mse = self.decay_margin, self.decay_equilibrium, self.decay_mse
        s.applied_epoch = 0
        self._base = s
        self.mask = mask
        self.state = torch.frombuffer(bytearray(bytes(s)), dtype=torch.uint8).to(feed.device)
        self._feed_state = feed._state
        self._lr_out = [o.lr_dev if m else None for o, m in zip(optims, mask)]
        self._lr_out += [None] * (lib.SCHED_MAX_LR - len(optims))
        self._hp_dev = hp_dev
        for o, m in zip(optims, mask):
            o.scheduled = m

    def launch(self, epoch_out: Optional[torch.Tensor] = None):
        """Enqueue the update for the batch the feed is about to draw (``epoch_out``: device int64 that receives its epoch)."""
        lib.call("fmri_epoch_begin", _P(self._feed_state), _P(self.state), *[_P(t) for t in self._lr_out],
                 _P(self._hp_dev), _P(epoch_out))

    def _decode(self, s: lib.Schedule) -> Dict[str, object]:
        n = len(self.mask)
        out = dict(lr=[s.lr[i] if self.mask[i] else None for i in range(n)], applied_epoch=int(s.applied_epoch))
        if self._hp_dev is not None:
            out.update(margin=s.margin, equilibrium=s.equilibrium, lambda_mse=s.lambda_mse)
        return out

    def values(self) -> Dict[str, object]:
        """The device state (syncs): ``lr`` (one double per optimizer, None where the mask is off), ``margin`` /
        ``equilibrium`` / ``lambda_mse`` (doubles; VAE/GAN steps only) and ``applied_epoch``, the epoch they belong to --
        the epoch of the batch the last step drew."""
        if self.state is None:
            raise RuntimeError("EpochSchedule.values(): not attached to a step")
        return self._decode(lib.Schedule.from_buffer_copy(self.state.cpu().numpy().tobytes()))

    def at(self, epoch: int) -> Dict[str, object]:
        """The doubles of ``epoch`` evaluated on the host by the code the kernel runs (fmri_schedule_seek_host); no GPU."""
        if self._base is None:
            raise RuntimeError("EpochSchedule.at(): not attached to a step")
        s = lib.Schedule.from_buffer_copy(bytes(self._base))
        lib.check(lib.load().fmri_schedule_seek_host(C.byref(s), int(epoch), None), "fmri_schedule_seek_host")
        return self._decode(s)


class TrainLog:
    """A device ring of the last ``capacity`` steps' log rows (``log=`` of the step classes; ``step.history()``)."""

    def __init__(self, capacity: int = 4096):
        if int(capacity) != capacity or capacity < 1:
            raise ValueError("TrainLog: capacity must be an integer >= 1")
        self.capacity = int(capacity)
        self.names: Optional[Tuple[str, ...]] = None

    def attach(self, device, columns: Sequence[Tuple[str, torch.Tensor, int]], losses: Sequence[str]):
        """(the step's ``_init_log``)  ``columns``: (name, persistent device tensor, element index) per column of a row, in
        row order; fp32 elements are copied, int32 elements (flags) come back as bools, int64 ones as int64.  ``losses``:
        the columns ``epoch_means`` averages."""
        if self.names is not None:
            raise ValueError("TrainLog: already attached to a step")
        K = len(columns)
        if not 1 <= K <= MAX_COLUMNS:
            raise ValueError(f"TrainLog: 1 to {MAX_COLUMNS} columns")
        self.names = tuple(n for n, _, _ in columns)
        self.kinds = tuple(_KIND[t.dtype] for _, t, _ in columns)
        self.losses = tuple(losses)
        self._keep = [t for _, t, _ in columns]          # the ring's sources must outlive it
        addr = [t.data_ptr() + i * t.element_size() for _, t, i in columns]
        self._src = torch.tensor(addr, dtype=torch.int64).to(device)
        self._kind = torch.tensor(self.kinds, dtype=torch.int32).to(device)
        # [counter: int64 in the first two words | ring: capacity x K fp32]: one block, one copy in history()
        self.blk = torch.zeros(2 + self.capacity * K, dtype=torch.float32, device=device)
        self.counter = self.blk[:2].view(torch.int64)
        self.ring = self.blk[2:].view(self.capacity, K)

    def append(self):
        lib.call("fmri_trainlog_append", _P(self._src), _P(self._kind), len(self.names), _P(self.ring), self.capacity,
                 _P(self.counter))

    def history(self) -> Dict[str, np.ndarray]:
        """One synchronising copy: column name -> numpy array over the last min(steps, capacity) steps, oldest first, and
        ``"step"``, their absolute step numbers (0 = the first step the log saw)."""
        if self.names is None:
            raise RuntimeError("TrainLog.history(): not attached to a step")
        raw = self.blk.cpu().numpy()
        n = int(raw[:2].view(np.int64)[0])
        steps = np.arange(max(0, n - self.capacity), n, dtype=np.int64)
        rows = raw[2:].reshape(self.capacity, len(self.names))[steps % self.capacity]
        out: Dict[str, np.ndarray] = {"step": steps}
        for k, (name, kind) in enumerate(zip(self.names, self.kinds)):
            col = rows[:, k]
            out[name] = col.copy() if kind == KIND_F32 else col != 0 if kind == KIND_I32 else col.astype(np.int64)
        return out

    def epoch_means(self) -> Dict[str, np.ndarray]:
        """Host arithmetic on ``history()``: ``"epoch"``, the epochs present in the ring in ascending order, ``"steps"``, how
        many of their steps it holds, and per loss column the float64 mean over those steps."""
        h = self.history()
        epochs = np.unique(h["epoch"])
        out: Dict[str, np.ndarray] = {"epoch": epochs,
                                      "steps": np.array([(h["epoch"] == e).sum() for e in epochs], dtype=np.int64)}
        for name in self.losses:
            v = h[name].astype(np.float64)
            out[name] = np.array([v[h["epoch"] == e].mean() for e in epochs], dtype=np.float64)
        return out


LR_NAMES = ("lr_encoder", "lr_decoder", "lr_discriminator", "lr_wae_discriminator")     # columns, in ``optims`` order


def lr_columns(optims) -> List[Tuple[str, torch.Tensor, int]]:
    return [(LR_NAMES[i], o.lr_dev, 0) for i, o in enumerate(optims)]
