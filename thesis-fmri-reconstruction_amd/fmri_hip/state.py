"""Device-side training-state ring of the fused steps (csrc/state.hip; include/fmri_hip.h fmri_state_copy).

What ``if not idx_epoch % 5: torch.save(model.state_dict(), ...)`` of the scripts' epoch loops does on the host
(train/train_vgan_stage1.py:596; every 10 epochs in the WAE scripts), for a step that runs whole trainings from one recorded
graph -- and the other half of a checkpoint, the state a run needs to CONTINUE bit for bit:

    ring = StateRing(capacity=2, every=5)           # every=None: manual slot only, no launch in the step, no feed needed
    step = Stage1Step(cfg, dev, rng=g, feed=feed, schedule=sched, log=log, checkpoints=ring)
    replay = step.capture()
    for _ in range(epochs * steps_per_epoch): replay()
    step.snapshot()                                  # enqueue-only: the state now, into the manual slot
    states = ring.states()                           # the ONE sync: TrainState list, oldest epoch first, manual last
    states[-1].save(path);  st = TrainState.load(path)
    fresh = Stage1Step(cfg, dev, rng=g2, feed=feed2, schedule=sched2, log=log2, checkpoints=StateRing(every=None))
    fresh.restore(st)                                # then step()/capture()/replay continue the run bit for bit

``StateRing``: with ``every`` set, ONE launch in front of the feed's draws of every step (behind ``fmri_epoch_begin``)
gathers every tensor of ``step._state_tensors()`` into a slot of a device ring -- when, and only when, the batch about to be
drawn opens epoch ``e`` with ``(e - 1) % every == 0``: the state at the end of epoch ``e - 1``, the epochs the scripts
save.  Slot and decision are read on the device from the feed's state, so the launch sits inside a recorded graph.  The
final epoch has no successor step: ``step.snapshot()`` takes its state (any state) into the ring's extra, manual slot.

``TrainState``: one snapshot on the host.  ``model`` is bitwise what ``step.state_dict()`` returned at that point -- the
reference's keys, shapes and dtypes --, ``engine`` holds the rest by name: optimizer state, learning rates, Adam's step
count, the hyper-parameter block, generator and feed state, the log.  ``save`` / ``load`` never touch a GPU.

Nothing here synchronises with the host except ``StateRing.states`` and ``restore`` (step_base._StepBase.restore).
"""
from __future__ import annotations

import ctypes as C
import hashlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib

_P = lib.ptr

FORMAT = "fmri_hip.train_state/1"
_DTYPES = {torch.float32: "float32", torch.int32: "int32", torch.int64: "int64", torch.float64: "float64"}
_META_KEYS = ("epoch", "cursor", "step", "fingerprint", "signature", "host")


# ---- host arithmetic (no GPU) ------------------------------------------------------------------------------------------
def layout(nbytes: Sequence[int]) -> Tuple[int, List[int]]:
    """(slot size, per-segment offsets) of segments of ``nbytes[i]`` bytes each: fmri_state_layout."""
    n = len(nbytes)
    arr = (C.c_int64 * max(n, 1))(*[int(b) for b in nbytes])
    offs = (C.c_int64 * max(n, 1))()
    size = lib.load().fmri_state_layout(arr, n, offs)
    if size < 0:
        raise ValueError("fmri_state_layout: byte counts must be non-negative multiples of 4")
    return int(size), [int(offs[i]) for i in range(n)]


def segment_lines(entries: Sequence[Tuple[str, str, int]]) -> List[str]:
    """The signature lines of a segment list: (name, dtype name, bytes) per segment."""
    return [f"seg {name} {dtype} {int(nbytes)}" for name, dtype, nbytes in entries]


def fingerprint(lines: Sequence[str]) -> int:
    """64-bit hash of a layout signature (a list of lines: what the step is and what its segments are)."""
    return int.from_bytes(hashlib.blake2b("\n".join(lines).encode(), digest_size=8).digest(), "little")


def slot_of(epoch: int, cursor: int, every: int, capacity: int) -> Optional[int]:
    """The firing predicate of fmri_state_copy on the host: the ring slot a step about to draw (epoch, cursor) writes, or
    None when it writes none."""
    if cursor != 0 or epoch < 1 or (epoch - 1) % every != 0:
        return None
    return ((epoch - 1) // every) % capacity


def _first_difference(mine: Sequence[str], theirs: Sequence[str]) -> str:
    for a, b in zip(mine, theirs):
        if a != b:
            return f"this step has '{a}', the state '{b}'"
    if len(mine) != len(theirs):
        longer, who = (mine, "this step") if len(mine) > len(theirs) else (theirs, "the state")
        return f"{who} also has '{longer[min(len(mine), len(theirs))]}'"
    return "the fingerprints differ"


# ---- one snapshot on the host --------------------------------------------------------------------------------------------
class TrainState:
    """``epoch`` / ``cursor``: the feed position the run continues from (-1 without a feed); ``step``: the log's step
    counter (-1 without a log); ``fingerprint``: the 64-bit hash of ``meta["signature"]``, what the step was and how its
    state is laid out."""

    def __init__(self, model: Dict[str, torch.Tensor], engine: Dict[str, torch.Tensor], meta: dict):
        missing = [k for k in _META_KEYS if k not in meta]
        if missing:
            raise ValueError(f"TrainState: meta misses {missing}")
        self.model, self.engine, self.meta = model, engine, meta
        self.epoch, self.cursor, self.step = int(meta["epoch"]), int(meta["cursor"]), int(meta["step"])
        self.fingerprint = int(meta["fingerprint"])

    def save(self, path):
        torch.save({"format": FORMAT, "model": self.model, "engine": self.engine, "meta": self.meta}, path)

    @staticmethod
    def load(path) -> "TrainState":
        blob = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(blob, dict) or blob.get("format") != FORMAT:
            fmt = blob.get("format") if isinstance(blob, dict) else type(blob).__name__
            raise ValueError(f"TrainState.load: {path} is not a '{FORMAT}' file (format: {fmt!r})")
        missing = [k for k in ("model", "engine", "meta") if k not in blob]
        if missing:
            raise ValueError(f"TrainState.load: {path} misses {missing}")
        return TrainState(blob["model"], blob["engine"], blob["meta"])


class _Segment:
    """One tensor of the state: where it lives, where it sits in a slot, and where its values go in a TrainState --
    ``model``: (state-dict key, element offset, shape, (C0, HW) or None) per entry of ``TrainState.model`` it carries (an
    engine-order BatchNorm vector is permuted to the reference's (C0, HW) order on the host), or None: ``engine[name]``."""
    __slots__ = ("name", "tensor", "dtype", "numel", "nbytes", "offset", "model")

    def __init__(self, name, tensor, model=None):
        if tensor.dtype not in _DTYPES or not tensor.is_contiguous():
            raise ValueError(f"state tensor {name}: contiguous float32 / float64 / int32 / int64 only")
        self.name, self.tensor, self.model = name, tensor, model
        self.dtype, self.numel = _DTYPES[tensor.dtype], tensor.numel()
        self.nbytes = tensor.numel() * tensor.element_size()
        self.offset = 0


class StateRing:
    """``capacity`` slots written round-robin by the step's own launch (``every``: the scripts' save period in epochs)
    plus the manual slot ``step.snapshot()`` writes.  ``every=None``: the manual slot only -- nothing is added to the
    step, no feed is needed.  A ring belongs to one step (``checkpoints=`` of the step classes)."""

    def __init__(self, capacity: int = 2, every: Optional[int] = 5):
        if every is not None and (int(every) != every or every < 1):
            raise ValueError("StateRing: every must be an integer >= 1 (or None: manual snapshots only)")
        if int(capacity) != capacity or capacity < (0 if every is None else 1):
            raise ValueError("StateRing: capacity must be an integer >= 1")
        self.every = None if every is None else int(every)
        self.capacity = int(capacity) if every is not None else 0
        self.segments: Optional[List[_Segment]] = None

    # ---- construction (the step's ``_init_checkpoints``) --------------------------------------------------------------
    def attach(self, device, segments: List[_Segment], signature: List[str], model_keys: List[str],
               feed_state: Optional[torch.Tensor], log_counter: Optional[torch.Tensor], host_state):
        if self.segments is not None:
            raise ValueError("StateRing: already attached to a step (a ring holds one step's state)")
        self.slot_bytes, offs = layout([s.nbytes for s in segments])
        table = (lib.StateSeg * max(len(segments), 1))()
        chunks = 0
        for row, s, off in zip(table, segments, offs):
            s.offset = off
            row.live, row.offset, row.bytes, row.chunk0 = s.tensor.data_ptr(), off, s.nbytes, chunks
            chunks += -(-s.nbytes // lib.STATE_CHUNK)
        self.segments, self.device, self.model_keys = segments, torch.device(device), list(model_keys)
        self.signature = list(signature) + segment_lines([(s.name, s.dtype, s.nbytes) for s in segments])
        self.fingerprint = fingerprint(self.signature)
        self.payload_bytes = sum(s.nbytes for s in segments)
        self._table = table                              # the host copy fmri_state_copy checks on every call
        self._table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(device)
        self.buf = torch.zeros((self.capacity + 1) * self.slot_bytes, dtype=torch.uint8, device=device)
        self._staging: Optional[torch.Tensor] = None     # one slot, allocated by the first restore
        self._feed_state, self._log_counter, self._host_state = feed_state, log_counter, host_state

    def _copy(self, ring: torch.Tensor, direction: int, feed_state, every: int, capacity: int):
        lib.note(bytes=2.0 * self.payload_bytes)
        lib.call("fmri_state_copy", C.addressof(self._table), _P(self._table_dev), len(self.segments), _P(ring),
                 ring.numel(), self.slot_bytes, direction, _P(feed_state), every, capacity, self.fingerprint,
                 _P(self._log_counter) if direction == 0 else None)

    def launch(self):
        """The step's own launch, in front of the feed's draws: copies when the epoch that just ended is one to keep."""
        self._copy(self.buf, 0, self._feed_state, self.every, self.capacity)

    def snapshot(self):
        """The state now, into the manual slot (enqueue-only)."""
        self._copy(self.buf, 0, self._feed_state, 0, self.capacity)

    def scatter(self, blob: np.ndarray):
        """One host-to-device copy of a slot image into the staging slot, one launch that scatters it to the live tensors."""
        if self._staging is None:
            self._staging = torch.empty(self.slot_bytes, dtype=torch.uint8, device=self.device)
        self._staging.copy_(torch.from_numpy(blob))
        self._copy(self._staging, 1, None, 0, 0)

    # ---- host side ----------------------------------------------------------------------------------------------------
    def states(self) -> List[TrainState]:
        """The ONE sync: every slot that holds a snapshot, the ring's by resume epoch (oldest first), the manual one last."""
        if self.segments is None:
            raise RuntimeError("StateRing.states(): not attached to a step")
        raw = self.buf.cpu().numpy().reshape(self.capacity + 1, self.slot_bytes)
        host = self._host_state()
        found = []
        for i, slot in enumerate(raw):
            h = slot[:lib.STATE_HEADER].view(np.int64)
            if int(h[0]) != lib.STATE_MAGIC:
                continue                                 # never written
            if int(h[1]) & (2 ** 64 - 1) != self.fingerprint or int(h[5]) != self.slot_bytes - lib.STATE_HEADER:
                raise RuntimeError("StateRing.states(): a slot carries another layout's fingerprint")
            found.append((i == self.capacity, int(h[2]), i, self._decode(slot, h, host)))
        return [st for _, _, _, st in sorted(found, key=lambda f: f[:3])]

    def _decode(self, slot: np.ndarray, h: np.ndarray, host: dict) -> TrainState:
        model, engine = {}, {}
        for s in self.segments:
            arr = slot[s.offset:s.offset + s.nbytes].view(s.dtype)
            if s.model is None:
                engine[s.name] = torch.from_numpy(arr.copy()).reshape(tuple(s.tensor.shape))
                continue
            for key, off, shape, perm in s.model:
                n = int(np.prod(shape)) if len(shape) else 1
                v = arr[off:off + n]
                if perm is not None:
                    c0, hw = perm
                    v = v.reshape(hw, c0).T                   # engine order (HW, C0) -> the reference's (C0, HW)
                model[key] = torch.from_numpy(np.ascontiguousarray(v).reshape(shape).copy())
        meta = dict(epoch=int(h[2]), cursor=int(h[3]), step=int(h[4]), fingerprint=self.fingerprint,
                    signature=list(self.signature), host=dict(host))
        return TrainState({k: model[k] for k in self.model_keys}, engine, meta)      # state_dict() order

    def check(self, state: TrainState):
        """ValueError naming the first difference when ``state`` was taken from a step of another make."""
        if state.fingerprint != self.fingerprint or list(state.meta["signature"]) != self.signature:
            raise ValueError("restore: the state does not fit this step: "
                             + _first_difference(self.signature, list(state.meta["signature"])))

    def encode(self, state: TrainState) -> np.ndarray:
        """The slot image of ``state`` (the inverse of ``_decode``); ValueError for a missing or misshapen tensor."""
        blob = np.zeros(self.slot_bytes, dtype=np.uint8)

        def take(d, key, shape, dtype):
            if key not in d:
                raise ValueError(f"restore: the state misses '{key}'")
            v = d[key].detach().cpu().numpy()
            if tuple(v.shape) != tuple(shape) or v.dtype != np.dtype(dtype):
                raise ValueError(f"restore: '{key}' is {v.dtype}{tuple(v.shape)}, the step has {dtype}{tuple(shape)}")
            return v
        for s in self.segments:
            arr = blob[s.offset:s.offset + s.nbytes].view(s.dtype)
            if s.model is None:
                arr[:] = take(state.engine, s.name, s.tensor.shape, s.dtype).reshape(-1)
                continue
            for key, off, shape, perm in s.model:
                v = take(state.model, key, shape, s.dtype)
                if perm is not None:
                    c0, hw = perm
                    v = v.reshape(c0, hw).T
                arr[off:off + v.size] = np.ascontiguousarray(v).reshape(-1)
        return blob
