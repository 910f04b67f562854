"""Augmentation of the fMRI rows of the Stage-II / Stage-III steps (csrc/voxaug.hip; include/fmri_hip.h fmri_voxaug_apply).

The fMRI side is the scarce one -- a few thousand trials of several thousand voxels, the same rows every epoch -- and the
standard augmentations of fMRI decoding are cheap: trial noise, voxel dropout, a masked span of voxels (an "ROI"), gain
jitter.  ``fmri_augment=VoxelAugment(...)`` on ``CognitiveStep`` / ``WaeStep(stage=2|3)`` puts them in front of the
cognitive encoder, on the device and inside a recorded step.  The reference has no counterpart, so this is opt-in and
pinned against the stated formula (tests/voxaug_oracle.py), not against a script.

A row's parameters are 8 fp32 values ``[g, sigma, p, k, s, L, 0, 0]`` (gain, noise sigma, dropout probability, rescale
factor, span start, span length); a step's table has B rows.  The element draws (noise, dropout) come from the step's
generator at its current offset whatever the table says.  Nothing here synchronises with the host.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .rng import SID_VDROP, SID_VNOISE, SID_VROW, DeviceRng, blocks as rng_blocks

NEUTRAL = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0)
V_MAX = 1 << 24        # span start and length are exact in fp32 below it


def blocks(B_global: int, V: int) -> int:
    """Philox blocks one step's element draws consume at the global batch, the noise and the dropout stream alike (the
    row stream's ``B_global`` blocks are fewer)."""
    return max(rng_blocks(int(B_global) * int(V)), int(B_global))


class VoxelAugment:
    def __init__(self, noise: float = 0.1, dropout: float = 0.1, span: float = 0.0, gain: float = 0.0, prob: float = 1.0,
                 rescale: bool = True):
        """``noise``: sigma of the additive N(0, 1) trial noise; ``dropout``: probability that a voxel is zeroed, the
        others multiplied by 1 / (1 - dropout) with ``rescale`` (inverted dropout); ``span``: fraction of the V voxels
        zeroed as one contiguous run at a random start; ``gain``: sigma of the per-row gain 1 + gain * N(0, 1);
        ``prob``: probability that a row is augmented at all."""
        if not 0.0 <= dropout < 1.0:
            raise ValueError("VoxelAugment: dropout must lie in [0, 1)")
        if not 0.0 <= span <= 1.0:
            raise ValueError("VoxelAugment: span is a fraction of the voxels in [0, 1]")
        if not 0.0 <= prob <= 1.0:
            raise ValueError("VoxelAugment: prob must lie in [0, 1]")
        if not noise >= 0.0 or not gain >= 0.0:
            raise ValueError("VoxelAugment: noise and gain are standard deviations >= 0")
        self.noise, self.dropout, self.span, self.gain = float(noise), float(dropout), float(span), float(gain)
        self.prob, self.rescale = float(prob), bool(rescale)

    def __repr__(self):
        return (f"VoxelAugment(noise={self.noise!r}, dropout={self.dropout!r}, span={self.span!r}, gain={self.gain!r}, "
                f"prob={self.prob!r}, rescale={self.rescale!r})")

    def span_len(self, V: int) -> int:
        """Voxels of the masked span at V voxels: round half up."""
        return int(V * self.span + 0.5)

    def table(self, rng: DeviceRng, B: int, V: int, row0: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 [B, 8]: rows row0 .. row0 + B of stream SID_VROW at the generator's current offset, which is NOT moved.
        Rank k of a data-parallel run passes ``row0 = k * B``."""
        _check_voxels(V)
        if out is None:
            out = torch.empty(B, 8, dtype=torch.float32, device=rng.device)
        _check_table(out, B)
        return ops.voxaug_params(rng._state, out, row0, SID_VROW, V, self.gain, self.noise, self.dropout, self.rescale,
                                 self.span_len(V), self.prob)

    @staticmethod
    def neutral(B: int, device=None) -> torch.Tensor:
        """The table under which the rows come out as ``ops.rows_to_f16`` gives them, bit for bit."""
        return torch.tensor(NEUTRAL, dtype=torch.float32, device=device).repeat(B, 1)

    @staticmethod
    def apply(fmri32: torch.Tensor, table: torch.Tensor, rng: DeviceRng, row0: int = 0,
              out16: Optional[torch.Tensor] = None, out32: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The fp16 [B, pad8(V)] rows the encoder reads: ``fmri32`` (contiguous fp32 [B, V]) under ``table``, noise and
        dropout drawn for global rows row0 .. at the generator's current offset, which is NOT moved (``blocks(B_global,
        V)`` is what an advance has to cover).  ``out32``: also the fp32 result."""
        if fmri32.dim() != 2:
            raise ValueError("VoxelAugment.apply: fmri32 must be [B, V]")
        _check_voxels(fmri32.shape[1])
        _check_table(table, fmri32.shape[0])
        return ops.voxaug_apply(fmri32, table, rng._state, row0, SID_VNOISE, SID_VDROP, out16, out32)


def _check_voxels(V: int):
    if not 1 <= V < V_MAX:
        raise ValueError(f"VoxelAugment: V = {V} voxels; 1 <= V < 2^24 is needed (span start and length are stored as "
                         "fp32)")


def _check_table(table: torch.Tensor, B: int):
    if (not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or tuple(table.shape) != (B, 8)
            or not table.is_contiguous() or not table.is_cuda):
        raise ValueError(f"VoxelAugment: the table must be a contiguous fp32 [{B}, 8] device tensor")
