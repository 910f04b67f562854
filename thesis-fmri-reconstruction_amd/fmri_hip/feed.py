"""Device-resident dataset and the feed of the fused steps (csrc/rng.hip sampler kernels, csrc/ingest.hip gathering
kernels; include/fmri_hip.h fmri_sampler_indices for the permutation and its state machine).

What the reference keeps behind ``DataLoader(dataset, batch_size, shuffle=True)`` -- a few ten thousand 64 x 64 uint8
stimuli and their fMRI rows, a few hundred MB at most -- lives on the device, and every step draws its shuffled,
augmented batch itself: indices of a counter-based permutation -> one gathering ingest pass (flip / shift / /255 / grey ->
RGB / normalise, straight out of the pool) -> a row gather of the fMRI -> the sampler's advance.  All of it is
enqueue-only with its position in device memory, so a step recorded with ``capture()`` replays whole epochs with no host
work between replays.  The batches are drop-last: an epoch has ``N // (batch * world)`` of them (the reference's loader
runs a short last batch instead; a recorded step has one batch size).

    ds = DeviceDataset(images_u8, fmri)                  # uint8 [N,H,W,C] (ops.crop_resize_u8 / HostStager make them)
    g = DeviceRng(seed, dev)
    step = Stage1Step(cfg, dev, rng=g, feed=DeviceFeed(ds, 256, seed, rng=g, flip=True, max_shift=5))
    replay = step.capture()

Nothing here synchronises with the host except ``last_indices``, ``position``, ``set_position`` and the diagnostic
``clamped``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import lib
from .ops import pad8, require_gpu
from .rng import DeviceRng, _wrap64, blocks

_P = lib.ptr


class DeviceDataset:
    """``images_u8``: uint8 [N,H,W,C], C = 1 or 3, on the device and contiguous; ``fmri``: fp32 [N,V] (optional).  Holds
    references to the caller's tensors: no copy."""

    def __init__(self, images_u8: torch.Tensor, fmri: Optional[torch.Tensor] = None):
        require_gpu(images_u8)
        if (images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] not in (1, 3)
                or not images_u8.is_contiguous() or images_u8.shape[0] < 1):
            raise ValueError("DeviceDataset: images_u8 must be a contiguous uint8 [N,H,W,C] device tensor with C = 1 or 3")
        if images_u8.shape[0] >= 2 ** 31:
            raise ValueError("DeviceDataset: at most 2^31 - 1 samples (int32 indices)")
        if fmri is not None:
            if (fmri.dtype != torch.float32 or fmri.dim() != 2 or fmri.shape[0] != images_u8.shape[0]
                    or not fmri.is_contiguous() or fmri.device != images_u8.device):
                raise ValueError("DeviceDataset: fmri must be a contiguous fp32 [N,V] tensor on the images' device")
        self.images, self.fmri = images_u8, fmri

    def __len__(self) -> int:
        return self.images.shape[0]


class DeviceFeed:
    """Draws batch after batch of a DeviceDataset on the device.

    ``seed`` keys the epoch permutation.  ``rng``: the DeviceRng the flips (``flip=True``) and shifts (``max_shift`` > 0)
    are drawn from, at its current offset, at elements ``rank * batch ..`` of the streams SID_FLIP / SID_SHIFT -- rank k
    of ``world`` gets rows k * batch .. of the one-rank batch at ``batch * world``, samples and augmentation alike.
    ``rank`` / ``world`` default to the process group's when one is initialised, else 0 / 1.

    A step that shares ``rng`` advances it (one advance per step covers the noise and the augmentation draws, which
    differ in stream id); used alone, ``next()`` advances it by ``blocks(2 * batch * world)``."""

    def __init__(self, dataset: DeviceDataset, batch: int, seed: int, rng: Optional[DeviceRng] = None,
                 max_shift: int = 0, flip: bool = False, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5),
                 rank: Optional[int] = None, world: Optional[int] = None):
        if (flip or max_shift > 0) and rng is None:
            raise ValueError("DeviceFeed: flip / max_shift need rng=DeviceRng(seed, device) to draw them from")
        if rank is None or world is None:
            import torch.distributed as dist
            on = dist.is_available() and dist.is_initialized()
            rank = (dist.get_rank() if on else 0) if rank is None else rank
            world = (dist.get_world_size() if on else 1) if world is None else world
        self.ds, self.B, self.rank, self.world = dataset, int(batch), int(rank), int(world)
        self.N = len(dataset)
        if self.B < 1 or not 0 <= self.rank < self.world:
            raise ValueError("DeviceFeed: batch >= 1 and 0 <= rank < world")
        if self.N < self.B * self.world:
            raise ValueError(f"DeviceFeed: the dataset ({self.N} samples) is smaller than the global batch "
                             f"({self.B} x {self.world})")
        self.rng, self.do_flip, self.max_shift = rng, bool(flip), int(max_shift)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        dev = dataset.images.device
        if rng is not None and rng.device != dev:
            raise ValueError("DeviceFeed: rng lives on another device than the dataset")
        self.device = dev
        _, H, W, _ = dataset.images.shape
        B = self.B
        self._state = torch.zeros(3, dtype=torch.int64, device=dev)             # [seed, epoch, cursor]
        self._seed = _wrap64(int(seed))
        self.set_position(0, 0)
        # persistent outputs: a recorded step reads the same memory at every replay
        self.x = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
        self.fmri = (torch.empty(B, dataset.fmri.shape[1], dtype=torch.float32, device=dev)
                     if dataset.fmri is not None else None)
        # the same rows as the engine's fp16 input (zero-padded to 8 columns), written by the same gather pass: a fed
        # Stage II / III step reads them instead of converting ``fmri`` in a pass of its own
        self.fmri16 = (torch.empty(B, pad8(dataset.fmri.shape[1]), dtype=torch.float16, device=dev)
                       if dataset.fmri is not None else None)
        self.idx = torch.zeros(B, dtype=torch.int32, device=dev)
        self.flip = torch.zeros(B, dtype=torch.int32, device=dev) if self.do_flip else None
        self.shift = torch.zeros(B, 2, dtype=torch.int32, device=dev) if self.max_shift > 0 else None
        self._err = torch.zeros(1, dtype=torch.int32, device=dev)

    # ---- the draws ---------------------------------------------------------------------------------------------------
    @property
    def augments(self) -> bool:
        return self.do_flip or self.max_shift > 0

    def rng_blocks(self) -> int:
        """Philox blocks of ``rng`` one batch consumes (the shifts, two per image of the global batch, are the larger
        draw); 0 without augmentation."""
        return blocks(2 * self.B * self.world) if self.augments else 0

    def next(self, advance_rng: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
        """Enqueue the next batch: (x fp32 NCHW, fmri fp32 [B,V] or None, idx int32 [B]) -- the feed's own buffers,
        rewritten by the next call.  ``advance_rng=False``: the caller advances the shared generator itself."""
        ds, B, r0 = self.ds, self.B, self.rank * self.B
        N, H, W, C = ds.images.shape
        lib.call("fmri_sampler_indices", _P(self._state), N, B, r0, _P(self.idx))
        if self.do_flip:
            self.rng.flips(B, start=r0, out=self.flip)
        if self.max_shift > 0:
            self.rng.shifts(B, self.max_shift, start=r0, out=self.shift)
        m, s = self.mean, self.std
        lib.note(bytes=float(B * H * W * (C + 12)))
        lib.call("fmri_ingest_u8_gather", _P(ds.images), _P(self.idx), N, B, H, W, C, _P(self.flip), _P(self.shift),
                 m[0], m[1], m[2], s[0], s[1], s[2], None, _P(self.x), _P(self._err))
        if self.fmri is not None:
            lib.call("fmri_gather_rows_f32", _P(ds.fmri), N, ds.fmri.shape[1], _P(self.idx), B, _P(self.fmri),
                     _P(self.fmri16), _P(self._err))
        lib.call("fmri_sampler_advance", _P(self._state), N, B * self.world)
        if advance_rng and self.augments:
            self.rng.advance(self.rng_blocks())
        return self.x, self.fmri, self.idx

    # ---- the calls that synchronise ------------------------------------------------------------------------------------
    def last_indices(self) -> torch.Tensor:
        """int32 [B] (host): the dataset rows of the batch last drawn."""
        return self.idx.cpu()

    def position(self) -> Tuple[int, int]:
        """(epoch, cursor) of the NEXT batch; with the seed it reproduces the run from here."""
        _, e, c = self._state.tolist()
        return e, c

    def set_position(self, epoch: int, cursor: int):
        if epoch < 0 or cursor < 0 or cursor + self.B * self.world > self.N:
            raise ValueError("DeviceFeed.set_position: epoch >= 0 and a whole global batch between cursor and the end")
        self._state.copy_(torch.tensor([self._seed, int(epoch), int(cursor)], dtype=torch.int64))

    def clamped(self) -> int:
        """Indices the gathering kernels had to clamp so far (always 0 with the sampler's own indices)."""
        return int(self._err.item())
