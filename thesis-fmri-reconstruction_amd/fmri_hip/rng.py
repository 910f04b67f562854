"""Device-side random numbers for the fused steps (csrc/rng.hip; include/fmri_hip.h fmri_rng_normal).

A counter-based generator (Philox4x32-10) whose state -- ``[seed, offset]``, int64 -- lives in device memory: the same
(seed, offset, global row, column, stream id) gives the same number on any launch shape, on any rank and in any replay of
a recorded step.  Draws never move the offset; ``advance`` does, as a launch of its own behind the draws that share it.
Draws made at one offset must use different stream ids (the ``SID_*`` constants below are the ones the steps use).

Nothing here synchronises with the host except ``offset()`` / ``state()``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import lib

_P = lib.ptr

# stream ids: third counter word of the Philox block
SID_EPS = 0            # reparameterisation noise of the trained encoder
SID_ZP = 1             # prior sample z_p
SID_EPS_TEACHER = 2    # reparameterisation noise of the Stage-II teacher
SID_ZFAKE = 3          # WAE prior sample (before the factor 0.5)
SID_FLIP = 8           # per-image horizontal flip
SID_SHIFT = 9          # per-image (rows, cols) shift
SID_DISTRACT = 10      # distractors of n-way identification (fmri_nway_scores)
SID_GENERATE = 11      # decoder input of the evaluator's `random` grid (fmri_hip/evaluate.py generate=)
SID_DAUG = 12          # DiffAugment rows of the [orig | pred] images (fmri_hip/augment.py)
SID_DAUG_P = 13        # DiffAugment rows of the sampled images
SID_VNOISE = 14        # VoxelAugment trial noise, one normal per (global row, voxel) (fmri_hip/voxaug.py)
SID_VDROP = 15         # VoxelAugment voxel dropout, one raw word per (global row, voxel)
SID_PERM = 16          # the epoch sampler's round function (fmri_sampler_indices; a counter layout of its own)
SID_VROW = 17          # VoxelAugment row parameters, one Philox block per global row

_I64 = (1 << 64) - 1


def _wrap64(v: int) -> int:
    """Python int -> the int64 with the same low 64 bits."""
    v &= _I64
    return v - (1 << 64) if v >> 63 else v


def blocks(n: int) -> int:
    """Philox blocks a draw of ``n`` elements from global row 0 consumes."""
    return (int(n) + 3) // 4


class DeviceRng:
    def __init__(self, seed: int, device):
        self.device = torch.device(device)
        self._state = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.seed(seed)

    # ---- state -------------------------------------------------------------------------------------------------------
    def seed(self, seed: int, offset: int = 0):
        self._state.copy_(torch.tensor([_wrap64(seed), _wrap64(offset)], dtype=torch.int64))

    def state(self) -> Tuple[int, int]:
        """(seed, offset) as unsigned Python ints -- syncs."""
        s, o = self._state.tolist()
        return s & _I64, o & _I64

    def set_state(self, state):
        self.seed(int(state[0]), int(state[1]))

    def offset(self) -> int:
        """Philox blocks consumed so far -- the only call of the draw interface that syncs."""
        return self._state[1].item() & _I64

    def advance(self, nblocks: int):
        lib.call("fmri_rng_advance", _P(self._state), int(nblocks))

    # ---- draws -------------------------------------------------------------------------------------------------------
    def normal(self, rows: int, cols: int, sid: int, row0: int = 0, scale: float = 1.0,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 [rows, cols] of scale * N(0, 1): global rows row0 .. row0 + rows of stream ``sid`` at the current offset.
        ``out``: a 2-D fp32 device tensor with unit column stride whose row stride may exceed ``cols`` (the columns
        behind ``cols`` are left as they are)."""
        if out is None:
            out = torch.empty(rows, cols, dtype=torch.float32, device=self.device)
        if (out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != rows or out.shape[1] < cols
                or out.stride(1) != 1 or out.device != self._state.device):
            raise ValueError("DeviceRng.normal: out must be fp32 [rows, >= cols] with unit column stride on the "
                             "generator's device")
        ld = out.stride(0) if rows > 1 else max(out.stride(0), cols)
        lib.call("fmri_rng_normal", _P(self._state), _P(out), rows, cols, ld, int(row0), sid, float(scale))
        return out

    def integers(self, n: int, lo: int, hi: int, sid: int, out: Optional[torch.Tensor] = None,
                 start: int = 0) -> torch.Tensor:
        """int32 [n] in [lo, hi] (both inclusive): elements start .. start + n of stream ``sid`` at the current offset
        (``start``: a rank's slice of a draw made at the global batch)."""
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=self.device)
        if (out.dtype != torch.int32 or out.numel() != n or not out.is_contiguous()
                or out.device != self._state.device):
            raise ValueError("DeviceRng.integers: out must be a contiguous int32 tensor of n elements on the "
                             "generator's device")
        if start:
            lib.call("fmri_rng_u32_at", _P(self._state), _P(out), n, int(start), sid, int(lo), int(hi))
        else:
            lib.call("fmri_rng_u32", _P(self._state), _P(out), n, sid, int(lo), int(hi))
        return out

    def flips(self, n: int, start: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int32 [n] of 0 / 1: the ``flip`` argument of ``ops.ingest_u8``, for images start .. start + n of the draw."""
        return self.integers(n, 0, 1, SID_FLIP, out=out, start=start)

    def shifts(self, n: int, max_shift: int, start: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int32 [n, 2] (rows, cols) in [-max_shift, max_shift]: the ``shift`` argument of ``ops.ingest_u8``, for images
        start .. start + n of the draw (elements 2 * start .. of the stream)."""
        return self.integers(2 * n, -int(max_shift), int(max_shift), SID_SHIFT, out=out, start=2 * start).view(n, 2)


class StepDraws:
    """The ledger of what a fused step draws from its generator, and the only place a step advances it.  The rule:
    draws never move the offset, so everything a step draws -- a shared feed's flips and shifts, the augmentation tables,
    the fMRI rows' element draws, the latent noise -- is drawn at ONE offset under different stream ids; every draw is
    noted here with the Philox blocks it consumes at the global batch, and ``close`` issues ONE advance, behind the last
    draw, by the largest.  A recorded step then draws fresh numbers at every replay and a restored one the same again.

        with step.draws:                       # leaving it closes the round; an exception drops it unadvanced
            ...draw with step.rng...; step.draws.note(blocks)
            eps, z_p = step.draws.noise(B, Z, rank, world, ("eps", SID_EPS, eps), ("z_p", SID_ZP, z_p))

    ``rng`` None (a step that is handed everything): nothing can be noted and ``close`` does nothing."""

    def __init__(self, rng: Optional[DeviceRng], owner: str = "step"):
        self.rng, self.owner = rng, owner
        self.bufs = {}           # argument name -> persistent fp32 [B, Z]: a recorded step rewrites the same memory
        self.last = {}           # argument name -> the tensor the last round used, in argument order (last_noise())
        self.noted = 0           # blocks of the largest draw of the round in progress

    def note(self, nblocks: int):
        """A draw of ``nblocks`` Philox blocks was made at the current offset."""
        if nblocks > self.noted:
            self.noted = int(nblocks)

    def noise(self, B: int, Z: int, rank: int, world: int, *wanted):
        """``wanted``: (argument name, stream id, the caller's tensor or None) of every noise input of the step.  A tensor
        the caller passed is used as it is; a missing one is drawn into the persistent [B, Z] buffer of its name at
        global rows rank * B .. and noted as a [B * world, Z] draw.  Returns the tensors in the order asked for."""
        last = self.last = {}
        for name, sid, t in wanted:
            if t is None:
                if self.rng is None:
                    missing = ", ".join(n for n, _, g in wanted if g is None)
                    raise ValueError(f"{self.owner}: {missing} not given and the step has no rng "
                                     "(pass the noise, or construct the step with rng=DeviceRng(seed, device))")
                t = self.bufs.get(name)
                if t is None or t.shape != (B, Z):
                    t = self.bufs[name] = torch.empty(B, Z, dtype=torch.float32, device=self.rng.device)
                self.rng.normal(B, Z, sid, row0=rank * B, out=t)
                self.note(blocks(B * world * Z))
            last[name] = t
        return last.values()

    def close(self):
        """The round's one advance, by the largest draw noted; nothing where nothing was."""
        n, self.noted = self.noted, 0
        if n:
            self.rng.advance(n)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self.noted = 0       # a step that failed half-way leaves nothing for the next one to advance by
        return False
