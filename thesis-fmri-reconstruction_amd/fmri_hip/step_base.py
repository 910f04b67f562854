"""What every fused step is built on (steps.py, wae_steps.py): the fused optimizers, the data-parallel glue with its
graph-segment recorder, and ``_StepBase`` -- scalar block, device RNG and feed, the ledger of a step's draws, the unit-RMS
re-normalisation of the encoder cotangent, HIP-graph capture and replay.  Nothing here knows a loss."""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import torch

from . import lib, ops
from .augment import _check_table, blocks as aug_blocks
from .voxaug import _check_table as _check_vox_table, blocks as vox_blocks
from .monitor import Monitored
from .nets import refresh_net
from .rng import DeviceRng, StepDraws
from .schedule import EpochSchedule, TrainLog, lr_columns
from .state import StateRing, TrainState, _Segment

_P = lib.ptr

# slots of the fp32 scalar block (csrc/loss.hip enum Slot)
(S_BCE_O, S_BCE_P, S_BCE_S, S_KL, S_MSE, S_NLE, S_LENC, S_LDIS, S_LDEC, S_DL2, S_NA, S_NB, S_RATIO,
 S_ONE, S_ESQ, S_NE, S_NP, S_C1, S_C2, S_C3, S_GDEC, S_KLW) = range(22)
OPTIM_NAMES = ("encoder", "decoder", "discriminator", "wae_discriminator")      # entries of ``optims``, in their order
S_ZMAX = 22         # slots [22, 26): max |z| of the latent batch of decoder group 0..3 (ops.latent_ranged; zero at step start)


class _Optim:
    """Fused RMSprop / Adam over a FlatGroup, optionally gated by a device flag; ``gdev`` is the device
    normalisation factor still carried by the gradients (divided out inside the kernel).  The learning rate (and
    Adam's step count) live in device memory: ``set_lr`` -- the per-epoch ExponentialLR / StepLR of the scripts
    (train_vgan_stage1.py:448-450) -- reaches a step that was recorded into a HIP graph."""

    def __init__(self, group, kind="rmsprop", lr=1e-4, alpha=0.9, eps=1e-8, betas=(0.5, 0.999)):
        self.g, self.kind, self.alpha, self.eps, self.betas = group, kind, alpha, eps, betas
        self.s1 = torch.zeros_like(group.data)
        self.s2 = torch.zeros_like(group.data) if kind == "adam" else None
        self.t = 0
        self._lr = float(lr)
        self.lr_dev = torch.full((1,), float(lr), dtype=torch.float32, device=group.device)
        self.t_dev = torch.zeros(1, dtype=torch.int32, device=group.device) if kind == "adam" else None
        self.stats = None        # (monitor.Monitor, device address of its record pair): set by a monitored step
        self.ema = None          # zero-argument launch of the group's weight average (ema.WeightEma.attach), or None
        self.scheduled = False   # an attached schedule.EpochSchedule writes lr_dev (set_lr then raises)

    @property
    def lr(self) -> float:
        return self._lr

    def set_lr(self, lr: float):
        if self.scheduled:
            raise RuntimeError("set_lr: this optimizer's learning rate is owned by the step's EpochSchedule")
        self._lr = float(lr)
        self.lr_dev.fill_(float(lr))

    def step(self, flag: Optional[torch.Tensor] = None, clamp: float = 0.0, gdev: Optional[torch.Tensor] = None):
        """The update, and directly behind it on the same stream -- whether or not ``flag`` let the update happen -- the
        group's weight average (``ema=`` of the step classes)."""
        self._update(flag, clamp, gdev)
        if self.ema is not None:
            self.ema()

    def _update(self, flag, clamp, gdev):
        g = self.g
        mon, rec = self.stats if self.stats is not None else (None, None)
        if self.kind == "rmsprop" and ops.apply_group(g, self.s1, self.lr_dev, self.alpha, self.eps, flag, gdev, clamp,
                                                      stats=rec):
            return                               # deferred gradients: update + fp16 copies in one launch (ops.begin_grads)
        if self.kind != "rmsprop":
            ops.flush_pending(g)                 # (Adam has no fused form: deferred gradients -> reference layout)
        if mon is not None:
            mon.grad_stats(g.grad, gdev, clamp, flag, rec)
        if self.kind == "rmsprop":
            lib.note(bytes=20.0 * g.numel)       # read p, g, v; write p, v
            lib.call("fmri_rmsprop_dev", _P(g.data), _P(g.grad), _P(self.s1), g.numel, _P(self.lr_dev), self.alpha,
                     self.eps, 1.0, _P(gdev), clamp, _P(flag))
        else:
            self.t += 1
            b1, b2 = self.betas
            lib.call("fmri_counter_inc", _P(self.t_dev))
            lib.note(bytes=28.0 * g.numel)       # read p, g, m, v; write p, m, v
            lib.call("fmri_adam_dev", _P(g.data), _P(g.grad), _P(self.s1), _P(self.s2), g.numel, _P(self.lr_dev), b1, b2,
                     self.eps, _P(self.t_dev), 1.0, _P(gdev), clamp, _P(flag))
        if mon is not None:
            mon.param_stats(g.data, flag, rec)
        g.version += 1


def _host_copy(host: float, dev: float) -> float:
    """The host's double of a restored fp32 device value: the one it has when that already rounds to the device value
    (1e-4 stays 1e-4, not 9.99999974e-05), else the device value."""
    return host if torch.tensor(host, dtype=torch.float32).item() == dev else float(dev)


class _SegmentRecorder:
    """Records a step as an alternating list of HIP graphs and eagerly issued collectives.

    Collectives stay outside the graphs (they are issued exactly as in the eager step, RCCL sees nothing new); every
    run of kernel launches between two collectives becomes one graph.  A data-parallel step is then ~37 graph launches
    + 36 collective calls on the host instead of ~400 kernel launches."""

    def __init__(self):
        self.pool = torch.cuda.graph_pool_handle()
        self.items = []          # torch.cuda.CUDAGraph or a zero-argument callable
        self.cur = None
        # The collectives run on a stream of their own, never on the one being recorded: the backend records its work
        # events on the stream a blocking collective is issued from, its watchdog THREAD polls them, and HIP refuses to
        # query an event whose stream has meanwhile entered capture (hipErrorCapturedEvent) -- the watchdog then
        # takes the process down (seen once in ~6 runs of the one-rank RCCL test, at the capture that follows a
        # SyncBN exchange).
        self.comm = torch.cuda.Stream()

    def _on_comm(self, fn):
        cur = torch.cuda.current_stream()
        self.comm.wait_stream(cur)
        with torch.cuda.stream(self.comm):
            fn()
        cur.wait_stream(self.comm)

    def begin(self):
        self.cur = torch.cuda.CUDAGraph()
        self.cur.capture_begin(pool=self.pool, capture_error_mode="thread_local")

    def end(self):
        ops.join_side()          # a capture cannot end with forked side-stream work (weight gradients) un-joined
        self.cur.capture_end()
        self.items.append(self.cur)
        self.cur = None

    def collective(self, fn):
        self.end()
        run = lambda: self._on_comm(fn)
        run()                    # communicator warm, same call order as at replay; operates on not-yet-computed data
        self.items.append(run)
        self.begin()

    def replay(self):
        for it in self.items:
            if isinstance(it, torch.cuda.CUDAGraph):
                it.replay()
            else:
                it()


_SMALL_GROUP = {}


def _small_group(dist):
    """The second communicator (small messages), created once per process and default group -- not once per step object."""
    key = id(dist.group.WORLD)
    if key not in _SMALL_GROUP:
        _SMALL_GROUP.clear()
        _SMALL_GROUP[key] = dist.new_group()
    return _SMALL_GROUP[key]


class _Dist:
    """Data-parallel glue (one process per GPU, RCCL): SUM all-reduce of flat gradients / loss scalars and
    the SyncBN statistic exchange.  Inactive (world size 1) unless torch.distributed is initialised."""

    def __init__(self, enabled: bool, sync_bn: bool = True):
        import torch.distributed as dist
        self.dist = dist
        # FMRI_FORCE_DIST=1: take the collective path even with one rank (single-GPU rehearsal of the RCCL calls)
        force = os.environ.get("FMRI_FORCE_DIST") == "1"
        self.on = enabled and dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or force)
        self.world = dist.get_world_size() if self.on else 1
        self.rank = dist.get_rank() if self.on else 0
        self.sync_bn = sync_bn
        self.pending = []
        # A communicator of its own for the SMALL collectives of the main stream (loss scalars, the stream-norm scalar,
        # SyncBN sums).  Collectives of one communicator run in issue order on its stream: behind a 44 MB gradient
        # all-reduce that is itself waiting for the side stream's weight gradients, a 40-byte all-reduce of the main
        # stream would stall the whole backward pass (head-of-line blocking); on a second communicator it does not.
        # FMRI_SMALL_COMM=off: everything on the default communicator (collectives then run in issue order, the order of
        # the program on every rank) -- the fallback should two communicators driven from two streams ever misbehave on a
        # real multi-GPU node; costs the head-of-line blocking described above
        self.small = _small_group(dist) if (self.on and os.environ.get("FMRI_SMALL_COMM") != "off") else None
        self.recorder: Optional[_SegmentRecorder] = None     # set while a step is recorded into graph segments

    SMALL = 1 << 16          # elements: at most this many go through the small-message communicator

    def all_reduce(self, t: torch.Tensor):
        """Blocking SUM all-reduce on the CURRENT stream (the host does not wait): scalars / statistics on the
        small-message communicator, gradient buffers on the default one."""
        if not self.on:
            return
        grp = self.small if t.numel() <= self.SMALL else None
        if self.recorder is not None:
            self.recorder.collective(lambda: self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=grp))
        else:
            self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=grp)

    def all_reduce_max(self, t: torch.Tensor):
        """Blocking MAX all-reduce of a few scalars on the current stream (the latent range of a SyncBN step)."""
        if not self.on:
            return
        fn = lambda: self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX, group=self.small)
        if self.recorder is not None:
            self.recorder.collective(fn)
        else:
            fn()

    def all_reduce_async(self, t: torch.Tensor):
        """Start a SUM all-reduce (same communicator, so it queues behind / ahead of the blocking ones in program
        order on every rank) and return immediately; `wait_all` joins it with the compute stream."""
        if not self.on:
            return

        def issue():
            self.pending.append(self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, async_op=True))
        if self.recorder is not None:
            self.recorder.collective(issue)
        else:
            issue()

    def wait_all(self):
        if not self.on:
            return

        def join():
            for h in self.pending:
                h.wait()
            self.pending.clear()
        if self.recorder is not None:
            self.recorder.collective(join)
        else:
            join()

    def bn_reducer(self):
        if not (self.on and self.sync_bn):
            return None

        def red(sums):
            self.all_reduce(sums)
            return self.world
        return red


def _attach_reducers(nets, d: _Dist):
    r = d.bn_reducer()
    for n in nets:
        for bn in n.all_bns():
            bn.reducer = r


class _StepBase(Monitored):
    """What every step uses; a subclass sets ``cfg``, builds its networks, calls ``_init_step`` and ``_init_rng``
    (``_init_augment`` / ``_init_fmri_augment`` where it has the keyword), registers its optimizers in ``optims``, ends its
    constructor with ``_init_extras`` and defines ``step`` (which starts with ``_fed`` and ends with ``_log_append``).

    Whatever a step draws from its generator goes through ``self.draws`` (rng.StepDraws): the draw is issued where the
    step wants it and noted with its block count -- ``_fed`` does so for a feed on the step's generator, ``_aug_table``
    and ``_fmri_rows`` for the augmentations, ``_noise`` for the latent noise -- inside ONE ``with self.draws:`` per step,
    whose end is the generator's one advance.  Nothing else in the step classes advances the generator."""

    schedule: Optional[EpochSchedule] = None
    log: Optional[TrainLog] = None
    checkpoints: Optional[StateRing] = None
    ema = None                                   # fmri_hip.ema.WeightEma or None
    _epoch_dev: Optional[torch.Tensor] = None

    def _init_step(self, device, nets, distributed: bool, sync_bn: bool):
        self.device = torch.device(device)
        self.scal = torch.zeros(32, dtype=torch.float32, device=device)
        self.esq64 = torch.zeros(1, dtype=torch.float64, device=device)      # sum of squares of _renorm
        self.dd = _Dist(distributed, sync_bn)
        _attach_reducers(nets, self.dd)
        self.fw: Dict[str, object] = {}
        self.optims: List[_Optim] = []       # in the order encoder, decoder, discriminator(, latent discriminator)
        self._pre_replay = []                # zero-argument hooks run before every replay of a recorded step

    def _init_rng(self, rng: Optional[DeviceRng], feed=None):
        self.rng = rng
        self.draws = StepDraws(rng, type(self).__name__)
        self.feed = feed             # fmri_hip.feed.DeviceFeed or None

    def _noise(self, B: int, *wanted):
        """``wanted``: (argument name, stream id, the caller's tensor or None) of every noise input of the step, each
        fp32 [B, latent_dim]: as passed, or drawn by the step's generator (StepDraws.noise)."""
        return self.draws.noise(B, self.cfg.latent_dim, self.dd.rank, self.dd.world, *wanted)

    def last_noise(self) -> Dict[str, torch.Tensor]:
        """The noise tensors the last step used, by argument name in the order ``step`` takes them (the step's own
        buffers where it drew them: clone what has to outlive the next step)."""
        return dict(self.draws.last)

    # ---- differentiable augmentation of the discriminator's inputs (fmri_hip/augment.py) ------------------------------
    augment = None                               # fmri_hip.augment.DiffAugment or None
    _aug_buf: Optional[torch.Tensor] = None      # the persistent table a step draws into
    _last_aug: Optional[torch.Tensor] = None

    def _init_augment(self, augment):
        """``augment=`` of the step classes that have an image discriminator.  None: nothing is added -- the step issues
        the launches it always did."""
        self.augment = augment

    def _aug_table(self, aug, B: int, H: int):
        """The table of the forward pass about to be issued: ``aug`` as it is, or, left out, a draw by the step's
        generator into the step's own buffer, noted in ``draws``; None for a step without ``augment=``."""
        if self.augment is None:
            if aug is not None:
                raise ValueError(f"{type(self).__name__}: aug= given, but the step was constructed without "
                                 "augment=DiffAugment(...)")
            return None
        if aug is not None:
            _check_table(aug, B)
        elif self.rng is None:
            raise ValueError(f"{type(self).__name__}: aug not given and the step has no rng (pass the table, or "
                             "construct the step with rng=DeviceRng(seed, device))")
        else:
            if self._aug_buf is None or self._aug_buf.shape[0] != 2 * B:
                self._aug_buf = torch.empty(2 * B, 8, dtype=torch.float32, device=self.device)
            aug = self.augment.table(self.rng, B, H, row0=self.dd.rank * B, out=self._aug_buf)
            self.draws.note(aug_blocks(B * self.dd.world))
        self._last_aug = aug
        return aug

    def last_augment(self) -> Optional[torch.Tensor]:
        """The fp32 [2B, 8] augmentation table the last step used (the step's own buffer where it drew it: clone what
        has to outlive the next step); None for a step without ``augment=``."""
        return self._last_aug

    def _aug_adjoint(self, dimg_a, dimg_b, rows: slice):
        """The image cotangents ``DiscriminatorNet.backward`` returned for images ``rows`` of the 3B layout, taken back
        through the transform of the last forward pass -- both streams in one launch; as they are without ``augment=``."""
        if self.augment is None or (dimg_a is None and dimg_b is None):
            return dimg_a, dimg_b
        return self.augment.adjoint((dimg_a, dimg_b), self.fw["aug"], self.fw["B"], rows)

    # ---- augmentation of the fMRI rows (fmri_hip/voxaug.py) -----------------------------------------------------------
    fmri_augment = None                          # fmri_hip.voxaug.VoxelAugment or None
    _vox_tab: Optional[torch.Tensor] = None      # the persistent table a step draws into
    _vox16: Optional[torch.Tensor] = None        # the persistent fp16 rows the encoder reads
    _last_vox: Optional[torch.Tensor] = None
    _last_fmri16: Optional[torch.Tensor] = None

    def _init_fmri_augment(self, fmri_augment):
        """``fmri_augment=`` of the step classes that have a cognitive encoder, after ``_init_rng``.  None: nothing is
        added -- the step issues the launches it always did."""
        if fmri_augment is not None and self.rng is None:
            raise ValueError(f"{type(self).__name__}: fmri_augment= needs rng=DeviceRng(seed, device): noise and dropout "
                             "are drawn per element by the step's generator, under a table the caller passes too")
        self.fmri_augment = fmri_augment

    def _fmri_rows(self, fmri_aug, fmri: torch.Tensor):
        """The rows the encoder of the step about to be issued reads: ``fmri`` (fp32 [B, V]) under the table ``fmri_aug``
        or, left out, under a draw by the step's generator -- the table's launch (unless passed) and the transform's, noted
        in ``draws``.  Returns (table, fp16 [B, pad8(V)] rows), the step's own buffers; (None, None) for a step without
        ``fmri_augment=``."""
        if self.fmri_augment is None:
            if fmri_aug is not None:
                raise ValueError(f"{type(self).__name__}: fmri_aug= given, but the step was constructed without "
                                 "fmri_augment=VoxelAugment(...)")
            return None, None
        table, fmri = fmri_aug, fmri.contiguous().float()
        B, V = fmri.shape
        row0 = self.dd.rank * B
        if table is None:
            if self._vox_tab is None or self._vox_tab.shape[0] != B:
                self._vox_tab = torch.empty(B, 8, dtype=torch.float32, device=self.device)
            table = self.fmri_augment.table(self.rng, B, V, row0=row0, out=self._vox_tab)
        else:
            _check_vox_table(table, B)
        if self._vox16 is None or self._vox16.shape[0] != B:
            self._vox16 = torch.empty(B, ops.pad8(V), dtype=torch.float16, device=self.device)
        self._last_vox = table
        self._last_fmri16 = self.fmri_augment.apply(fmri, table, self.rng, row0=row0, out16=self._vox16)
        self.draws.note(vox_blocks(B * self.dd.world, V))
        return table, self._last_fmri16

    def last_fmri_augment(self) -> Optional[torch.Tensor]:
        """The fp32 [B, 8] table of the fMRI rows' augmentation the last step used (the step's own buffer where it drew
        it: clone what has to outlive the next step); None for a step without ``fmri_augment=``."""
        return self._last_vox

    def last_fmri16(self) -> Optional[torch.Tensor]:
        """The fp16 [B, pad8(V)] rows the cognitive encoder read in the last step (the step's own buffer); None for a step
        without ``fmri_augment=``."""
        return self._last_fmri16

    def _init_schedule(self, schedule: Optional[EpochSchedule], default_mask=None, hp=None, hp_dev=None):
        """``schedule=`` of the step classes (fmri_hip/schedule.py), after ``optims`` is complete.  ``default_mask``: which
        optimizers follow the lr schedule unless the schedule says otherwise (default: all); ``hp`` / ``hp_dev``: the
        VAE/GAN hyper-parameters and their device block, None for a step that has none."""
        self.schedule = schedule
        if schedule is None:
            return
        if self.feed is None:
            raise ValueError(f"{type(self).__name__}: schedule= needs feed=DeviceFeed(...): the feed is where the epoch "
                             "lives")
        mask = [True] * len(self.optims) if default_mask is None else default_mask
        schedule.attach(self.feed, self.optims, mask, hp, hp_dev)

    def _log_columns(self):
        """(column name, persistent device tensor, element index) of everything ``logs()`` returns, in its order -- each
        step class states its layout once, here -- and the names among them that are losses."""
        raise NotImplementedError

    def _init_log(self, log: Optional[TrainLog]):
        """``log=`` of the step classes, after ``optims`` is complete: the class's ``_log_columns`` + ``epoch`` (of the
        batch the step drew; -1 without a feed) + the learning rate of every entry of ``optims``."""
        self.log = log
        if log is None:
            return
        cols, losses = self._log_columns()
        self._epoch_dev = torch.full((1,), -1, dtype=torch.int64, device=self.device)
        log.attach(self.device, list(cols) + [("epoch", self._epoch_dev, 0)] + lr_columns(self.optims), losses)

    # ---- weight average (fmri_hip/ema.py) ------------------------------------------------------------------------------
    def _trained(self) -> List[str]:
        """Names (``OPTIM_NAMES``) of the optimizers the step runs every batch -- the networks that can have an average;
        a subclass with frozen networks says which."""
        return [n for n, _ in zip(OPTIM_NAMES, self.optims)]

    def _init_ema(self, ema):
        """``ema=`` of the step classes, after ``optims`` is complete and before ``_init_checkpoints`` (the ring sees the
        shadows).  None: nothing is added -- the step issues the launches it always did."""
        self.ema = ema
        if ema is not None:
            ema.attach(self)
            self._pre_replay.append(ema.prime)

    def ema_state_dict(self):
        """``state_dict()`` with the averaged weights and BatchNorm statistics of the shadowed networks in place of the live
        ones (everything else -- ``num_batches_tracked``, the other networks -- is the live value): loadable wherever
        ``state_dict()`` is.  Device tensors, no sync."""
        if self.ema is None:
            raise RuntimeError("ema_state_dict(): the step was constructed without ema=WeightEma(...)")
        return self.ema.state_dict()

    def _epoch_begin(self):
        """The launch in FRONT of the feed's draws: the feed's state still holds the epoch of the batch about to be drawn.
        Moves the schedule there and / or notes the epoch for the log; nothing for a step with neither.  Behind it, the
        predicated snapshot launch of a ``checkpoints=StateRing(every=...)``."""
        self._epoch_note()
        if self.checkpoints is not None and self.checkpoints.every is not None:
            self._state_ready()
            self.checkpoints.launch()

    def _epoch_note(self):
        noted = self._epoch_dev if self.feed is not None else None
        if self.schedule is not None:
            self.schedule.launch(noted)
        elif noted is not None:
            lib.call("fmri_epoch_begin", _P(self.feed._state), None, None, None, None, None, None, _P(noted))

    # ---- training state: snapshot and bit-exact resume (fmri_hip/state.py) ---------------------------------------------
    def _state_groups(self):
        """(state-dict prefix, network) in ``state_dict()`` order -- a network listed twice appears under both prefixes
        (Stage II's ``teacher_net.decoder.`` aliases ``decoder.``).  Each step class states its networks once, here."""
        raise NotImplementedError

    def state_dict(self):
        sd = {}
        for pre, n in self._state_groups():
            sd.update(n.group.state_dict(pre))
        return sd

    def _state_nets(self):
        nets = []
        for _, n in self._state_groups():
            if all(n is not m for m in nets):
                nets.append(n)
        return nets

    def _lazy_bns(self):
        return [bn for n in self._state_nets() for bn in n.all_bns() if bn._lazy]

    def _group_segments(self):
        """(segment name, live tensor, its entries of ``TrainState.model``) of every network: the fp32 masters as one
        segment per group, and the BatchNorm buffers -- of a lazy BatchNorm the engine-order copies, which are the live
        ones (ops.BatchNorm.enable_lazy_running)."""
        owner, entries = {}, {}
        for pre, n in self._state_groups():
            g = n.group
            first = owner.setdefault(id(g), pre)
            live = {}
            for bn in n.all_bns():
                if bn._lazy:
                    live[bn.prefix + "running_mean"] = (bn.rm_e, bn.perm)
                    live[bn.prefix + "running_var"] = (bn.rv_e, bn.perm)
            for k, shape, _ in g.spec:
                if k in g.views:
                    seg, t, off, perm = f"group:{first}data", g.data, g.offsets[k], None
                else:
                    t, perm = live.get(k, (g.bufs[k], None))
                    seg, off = f"buf:{first}{k}", 0
                entries.setdefault(seg, (t, []))[1].append((pre + k, off, tuple(shape), perm))
        return [(seg, t, model) for seg, (t, model) in entries.items()]

    def _state_tensors(self) -> Dict[str, torch.Tensor]:
        """name -> persistent device tensor of everything a run needs to continue bit for bit; the subclasses add theirs.
        Out: gradients, activations, the packed fp16 weights (derived), the schedule's struct (it re-seeks from the epoch),
        the monitor, the evaluator, and the scratch every step rewrites before it reads it."""
        out = {seg: t for seg, t, _ in self._group_segments()}
        for name, o in zip(OPTIM_NAMES, self.optims):
            out[f"opt:{name}.s1"] = o.s1
            if o.s2 is not None:
                out[f"opt:{name}.s2"] = o.s2
            out[f"opt:{name}.lr"] = o.lr_dev
            if o.t_dev is not None:
                out[f"opt:{name}.t"] = o.t_dev
        if self.rng is not None:
            out["rng"] = self.rng._state
        if self.feed is not None:
            out["feed"] = self.feed._state
            if self.feed.rng is not None and self.feed.rng is not self.rng:
                out["feed_rng"] = self.feed.rng._state
        if self.log is not None:
            out["log"] = self.log.blk
            out["log_epoch"] = self._epoch_dev
        if self.ema is not None:
            out.update(self.ema.state_tensors())
        return out

    def _state_signature(self) -> List[str]:
        """What a state must agree in before it is restored into this step, one line each (the segment list follows)."""
        sig = [f"class={type(self).__name__}", f"config={self.cfg!r}"]
        for a in ("mode", "stage", "penalty", "n_voxels"):
            if hasattr(self, a):
                sig.append(f"{a}={getattr(self, a)}")
        if hasattr(getattr(self, "dis", None), "level"):
            sig.append(f"recon_level={self.dis.level}")
        sig.append("optims=" + ",".join(f"{n}:{o.kind}" for n, o in zip(OPTIM_NAMES, self.optims)))
        sig.append("log=" + ("none" if self.log is None else ",".join(self.log.names) + f"@{self.log.capacity}"))
        if self.ema is not None:
            sig.append(self.ema.signature())
        if self.augment is not None:
            sig.append(f"augment={self.augment!r}")
        if self.fmri_augment is not None:
            sig.append(f"fmri_augment={self.fmri_augment!r}")
        return sig

    def _host_state(self) -> dict:
        """Host-side counters a resumed run needs (TrainState.meta["host"]); none here."""
        return {}

    def _host_meta(self) -> dict:
        """``_host_state()`` and, with ``ema=``, where the state-dict entries sit in the shadows (WeightEma.state_dict_of
        reads a saved state without a step)."""
        host = dict(self._host_state())
        if self.ema is not None:
            host["ema"] = self.ema.layout()
        return host

    def _restored(self, host: dict):
        """Host copies of restored device values (``restore`` has synchronised): learning rates, Adam's step count, the
        feed's seed; the subclasses add theirs.  A scheduled optimizer keeps the BASE rate its schedule started from."""
        for o in self.optims:
            if not o.scheduled:
                o._lr = _host_copy(o._lr, o.lr_dev.item())
            if o.t_dev is not None:
                o.t = int(o.t_dev.item())        # replays never advance ``t``: the device counter is the truth
        if self.feed is not None:
            self.feed._seed = int(self.feed._state[0].item())

    def _init_checkpoints(self, ring: Optional[StateRing]):
        """``checkpoints=`` of the step classes, after ``_init_log``."""
        self.checkpoints = ring
        if ring is None:
            return
        if ring.every is not None and self.feed is None:
            raise ValueError(f"{type(self).__name__}: checkpoints=StateRing(every=...) needs feed=DeviceFeed(...): the "
                             "feed is where the epoch lives (every=None takes manual snapshots only)")
        model = {seg: m for seg, _, m in self._group_segments()}
        segs = [_Segment(name, t, model.get(name)) for name, t in self._state_tensors().items()]
        keys = [pre + k for pre, n in self._state_groups() for k, _, _ in n.group.spec]
        ring.attach(self.device, segs, self._state_signature(), keys,
                    self.feed._state if self.feed is not None else None,
                    self.log.counter if self.log is not None else None,
                    self._host_state if self.ema is None else self._host_meta)

    def _init_extras(self, schedule, log, checkpoints=None, ema=None, lr_mask=None, hp=None, hp_dev=None):
        """The tail of every constructor -- ``schedule=`` / ``log=`` / ``ema=`` / ``checkpoints=``, in the order they depend
        on each other -- once ``optims`` is complete; ``lr_mask`` / ``hp`` / ``hp_dev``: see ``_init_schedule``."""
        self._init_schedule(schedule, lr_mask, hp, hp_dev)
        self._init_log(log)
        self._init_ema(ema)
        self._init_checkpoints(checkpoints)

    def _state_ready(self, between_steps: bool = False):
        """In front of a snapshot launch: the optimizer updates of the eager two-stream mode run on the side stream, so the
        step must have joined; the engine-order BatchNorm statistics must be the loaded ones (a host check; they are after
        the first step).  ``between_steps`` (a manual snapshot): no weight gradient may be waiting for its update -- a
        snapshot between ``backward()`` and ``apply()`` would hold half a step."""
        ops.join_side()
        if between_steps:
            for n in self._state_nets():
                if n.group.gq.pending or n.group.gq.materialized:
                    raise RuntimeError("snapshot between backward() and apply(): weight gradients are still queued")
        for bn in self._lazy_bns():
            bn._running_in()

    def snapshot(self):
        """The state now, into the manual slot of the step's ``checkpoints=StateRing(...)``: enqueue-only, between eager
        steps or replays (``ring.states()`` reads it).  A fed step takes it where its own launch would: behind the
        ``fmri_epoch_begin`` of the batch about to be drawn -- at an epoch boundary the learning rates and the gate's
        parameters are the new epoch's already, which the next step would have written first thing anyway -- so a manual
        snapshot at a boundary is bit for bit the slot the ring keeps there."""
        if self.checkpoints is None:
            raise RuntimeError("snapshot(): the step was constructed without checkpoints=StateRing(...)")
        self._state_ready(between_steps=True)
        if self.feed is not None:
            self._epoch_note()
        self.checkpoints.snapshot()

    def restore(self, state: TrainState):
        """Continue the run ``state`` was taken from: every tensor of ``_state_tensors()`` is overwritten (one host-to-device
        copy, one launch), everything derived from the weights is refreshed NOW -- a recorded step updates its packed fp16
        weights inside the graph and never looks at a version counter --, queued weight gradients are dropped and the
        host's copies of device values follow.  A state of another class, config, mode, optimizer kind or log layout is
        a ValueError naming the first difference, raised before any device byte changes.  Synchronises."""
        ring = self.checkpoints
        if ring is None:
            raise RuntimeError("restore(): the step was constructed without checkpoints=StateRing(...)")
        ring.check(state)
        blob = ring.encode(state)
        ops.join_side()
        for bn in self._lazy_bns():
            bn._running_in()                     # a pending reload from the reference-order buffers would undo the restore
        if self.ema is not None:
            self.ema.mark_loaded()               # as would a pending copy of loaded weights into the shadows
        ring.scatter(blob)
        for n in self._state_nets():
            n.group.drop_pending()
            n.group.version += 1
        self._restored(dict(state.meta["host"]))
        for n in self._state_nets():
            refresh_net(n)
        torch.cuda.current_stream().synchronize()

    def _log_append(self):
        """The last launch of a step: behind the gate, the loss all-reduce and every kernel that writes a logged value.  In
        front of it, with ``ema=``, the tail of the weight average: the BatchNorm buffers' launch and the step counter."""
        if self.ema is not None:
            self.ema.finish()
        if self.log is not None:
            self.log.append()

    def history(self):
        """``log=TrainLog(...)``: the logged steps (ONE sync): name -> numpy array, oldest first, the last
        min(steps, capacity) steps -- per step exactly what ``logs()`` would have returned after it, ``epoch`` (of the
        batch it drew, -1 without a feed), the learning rates of ``optims`` (``lr_encoder`` ...) and ``step``, the
        absolute step numbers."""
        if self.log is None:
            raise RuntimeError("history(): the step was constructed without log=TrainLog(...)")
        return self.log.history()

    def epoch_means(self):
        """Per epoch present in the log's ring: the mean of every loss over the steps held (TrainLog.epoch_means)."""
        if self.log is None:
            raise RuntimeError("epoch_means(): the step was constructed without log=TrainLog(...)")
        return self.log.epoch_means()

    def _fed(self, *given):
        """The batch of a step.  Without a feed: ``given`` (the caller's batch tensors) must all be there; returns None.
        With a feed: none may be; the feed enqueues its next batch (fmri_hip/feed.py) -- the first launches of the step,
        so they sit in the one graph of a recording, or in the first segment of a data-parallel one -- and its buffers
        (x fp32 NCHW, fmri fp32 [B,V] or None, the same rows as zero-padded fp16 or None) are returned.  A feed that
        draws its augmentation from the step's own generator leaves the advance to the step: its blocks are noted in
        ``draws``, whose one advance at the end of the step's round covers them.  A schedule / log puts ONE launch in front of the feed's (``_epoch_begin``)."""
        if self.ema is not None:
            self.ema.prime()                     # host check: weights loaded from outside since the last step
        feed = self.feed
        if feed is None:
            if any(g is None for g in given):
                raise ValueError(f"{type(self).__name__}: no batch given and the step has no feed (pass the batch, or "
                                 "construct the step with feed=DeviceFeed(...))")
            return None
        if any(g is not None for g in given):
            raise ValueError(f"{type(self).__name__}: the step has a feed and draws its own batch: step() takes no "
                             "batch arguments")
        shared = feed.rng is not None and feed.rng is self.rng
        self._epoch_begin()
        x, fm, _ = feed.next(advance_rng=not shared)
        if shared:
            self.draws.note(feed.rng_blocks())
        return x, fm, feed.fmri16

    def _reduce_async(self, group, part=None):
        """Data parallel: the sub-network's deferred weight gradients -> reference layout (one launch), then the
        asynchronous SUM all-reduce of the gradient buffer (or of ``part`` of it).  Nothing on one GPU: the gradients
        stay deferred until the update (ops.apply_group)."""
        if self.dd.on:
            ops.materialize_grads(group)
            self.dd.all_reduce_async(group.grad if part is None else part)

    def _slot(self, i):
        return self.scal[i:i + 1]

    def _renorm(self, x32: torch.Tensor, scale: float, factor_in, rows_global: int):
        """fp32 cotangent -> unit-RMS fp16 (times ``scale``); S_NE <- (*factor_in) / rms (``factor_in`` None: 1 / rms).
        The sum of squares is all-reduced so that every data-parallel rank applies the same factor."""
        n = x32.numel()
        # the sum of squares in double precision (the KL term's 0.5 * (exp(logvar) - 1), squared, leaves fp32 at
        # logvar > 44), cleared by the launch itself: a second backward() after one gate() starts from zero as well
        esq = self.esq64
        lib.call("fmri_sumsq_f64", _P(x32), n, _P(esq), 1)
        self.dd.all_reduce(esq)
        out = torch.empty(x32.shape, dtype=torch.float16, device=x32.device)
        count = float(rows_global) * (n // x32.shape[0])
        lib.call("fmri_renorm_f64", _P(x32), _P(out), n, float(scale), _P(esq), count, _P(factor_in),
                 _P(self._slot(S_NE)))
        return out

    def capture(self, *static_inputs, warmup: int = 2):
        """Record one ``step(*static_inputs)`` into a HIP graph and return a zero-argument callable that replays it.

        Every launch of a step is enqueue-only and nothing inside a step synchronises with the host (the equilibrium
        gate, the stream normalisation and the optimizer gating all live on the device), so the ~370 launches of a
        step can be replayed as one graph: the step time then no longer depends on how fast the host can issue them.
        Inputs are read from ``static_inputs`` at every replay -- copy each new batch into those tensors.  Learning
        rates, lambda, margin, equilibrium and beta are device-resident (``set_lr`` / ``set_hyper``, or a ``schedule=`` that
        applies the epoch-end block on the device, fmri_hip/schedule.py): a replayed step follows
        their schedules (Adam's step count of the WAE steps lives on the device too, ``wae_steps``).  In a data-parallel run the collectives
        are kept out of the graphs (see _SegmentRecorder)."""
        # The weight-gradient side stream (ops.side_run) is switched off while recording: a replayed HIP graph runs
        # its parallel branches no faster than a chain (measured 8.8 ms chained, 9.0-9.5 ms with the fork/join
        # branches, 8.4 ms eager with two streams), so the recorded step keeps everything on one stream.
        side_was = ops._SIDE["on"]
        ops.join_side()
        ops._SIDE["on"] = False
        try:
            return self._capture(static_inputs, warmup)
        finally:
            ops._SIDE["on"] = side_was

    def _capture(self, static_inputs, warmup):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self.step(*static_inputs)
        torch.cuda.current_stream().wait_stream(side)
        if self.dd.on:
            # data-parallel: the collectives stay eager, the launches between them become graphs
            rec = _SegmentRecorder()
            self.dd.recorder = rec
            try:
                with torch.cuda.stream(side):
                    rec.begin()
                    self.step(*static_inputs)
                    rec.end()
            except BaseException:
                if rec.cur is not None:          # leave no stream capture open behind a failed recording
                    try:
                        rec.cur.capture_end()
                    except Exception:
                        pass
                raise
            finally:
                self.dd.recorder = None
            torch.cuda.current_stream().wait_stream(side)
            self._graph = rec
            return self._versioned(rec.replay)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self.step(*static_inputs)
        self._graph = graph
        return self._versioned(graph.replay)

    def _versioned(self, replay):
        """A replay updates the master weights without passing through ``_Optim.step``: bump the groups' version
        counters so that the first eager step afterwards re-packs its fp16 weights."""
        groups = [o.g for o in self.optims]

        def run():
            for h in self._pre_replay:
                h()
            replay()
            for g in groups:
                g.version += 1
        return run
