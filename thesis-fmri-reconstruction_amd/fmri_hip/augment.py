"""Differentiable augmentation of the discriminator's inputs (csrc/diffaug.hip; include/fmri_hip.h fmri_diffaug_fwd).

Zhao et al., "Differentiable Augmentation for Data-Efficient GAN Training" (NeurIPS 2020): every image the discriminator
sees -- real and generated alike -- goes through one random colour / translation / cutout transform, and the generator's
gradient is taken through that transform.  The regulariser of choice when a GAN is trained on a few thousand images, which
is what Stage II / III do; the reference has no counterpart, so this is opt-in (``augment=DiffAugment()`` on the fused
steps) and pinned against the stated formula (tests/diffaug_oracle.py), not against a script.

A transform is a row of 8 fp32 values ``[b, s, c, ty, tx, cy, cx, cut]`` per image; a step's table has 2B rows for its 3B
images ``[orig | pred | sampled]``: orig b and pred b share row b (the ``mse`` term compares them feature by feature),
sampled b has row B + b.  Nothing here synchronises with the host.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops
from .rng import SID_DAUG, SID_DAUG_P, DeviceRng

POLICIES = {"color": 1, "translation": 2, "cutout": 4}
NEUTRAL = (0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def blocks(B_global: int) -> int:
    """Philox blocks the draw of one stream's rows consumes at the global batch: 8 words = 2 blocks per row."""
    return 2 * int(B_global)


class DiffAugment:
    def __init__(self, policy: Sequence[str] = ("color", "translation", "cutout"), translation: float = 0.125,
                 cutout: float = 0.5):
        """``policy``: any of 'color' (brightness +-0.5, saturation x [0, 2), contrast x [0.5, 1.5)), 'translation'
        (integer shift of up to ``translation`` * H pixels each way, zero fill) and 'cutout' (a zeroed square of
        ``cutout`` * H pixels at a random centre); the defaults are the paper's."""
        policy = tuple(policy)
        unknown = [p for p in policy if p not in POLICIES]
        if unknown:
            raise ValueError(f"DiffAugment: unknown policy {unknown}; known: {sorted(POLICIES)}")
        if not (0.0 <= translation <= 1.0 and 0.0 <= cutout <= 1.0):
            raise ValueError("DiffAugment: translation and cutout are fractions of the image size in [0, 1]")
        self.policy, self.translation, self.cutout = policy, float(translation), float(cutout)
        self.mask = 0
        for p in policy:
            self.mask |= POLICIES[p]

    def __repr__(self):
        return f"DiffAugment(policy={self.policy!r}, translation={self.translation!r}, cutout={self.cutout!r})"

    def sizes(self, H: int):
        """(largest shift, cutout edge) in pixels at image size H: round half up."""
        return int(H * self.translation + 0.5), int(H * self.cutout + 0.5)

    def table(self, rng: DeviceRng, B: int, H: int, row0: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 [2B, 8]: rows row0 .. row0 + B of stream SID_DAUG ([orig | pred]) and of stream SID_DAUG_P (sampled) at
        the generator's current offset, which is NOT moved (``blocks(B_global)`` is what an advance has to cover).  Rank
        k of a data-parallel run passes ``row0 = k * B``."""
        if out is None:
            out = torch.empty(2 * B, 8, dtype=torch.float32, device=rng.device)
        sh, cut = self.sizes(H)
        ops.diffaug_params(rng._state, out[:B], row0, SID_DAUG, H, sh, cut, self.mask)
        ops.diffaug_params(rng._state, out[B:], row0, SID_DAUG_P, H, sh, cut, self.mask)
        return out

    @staticmethod
    def neutral(B: int, device=None) -> torch.Tensor:
        """The table under which the transform is the identity (and its adjoint too)."""
        return torch.tensor(NEUTRAL, dtype=torch.float32, device=device).repeat(2 * B, 1)

    @staticmethod
    def forward(x16: torch.Tensor, table: torch.Tensor, B: Optional[int] = None) -> torch.Tensor:
        """T of the 3B images ``[orig | pred | sampled]`` (fp16 [3B,H,W,8]) -> a new tensor."""
        B = x16.shape[0] // 3 if B is None else B
        _check_table(table, B)
        if x16.shape[0] != 3 * B:
            raise ValueError("DiffAugment.forward: x16 must hold the 3B images [orig | pred | sampled]")
        return ops.diffaug_fwd(x16, table, B, 0)

    @staticmethod
    def adjoint(g16, table: torch.Tensor, B: int, rows: slice):
        """The adjoint of T's linear part on a cotangent (fp16 [rows,H,W,8]) -- or on a tuple of two, either of which may
        be None, in one launch -- that covers images ``rows`` of the 3B layout (the steps ask for ``slice(B, 3B)`` or
        ``slice(B, 2B)``).  Returns new tensors."""
        _check_table(table, B)
        pair = g16 if isinstance(g16, (tuple, list)) else (g16, None)
        lo, hi, _ = rows.indices(3 * B)
        for g in pair:
            if g is not None and g.shape[0] != hi - lo:
                raise ValueError("DiffAugment.adjoint: the cotangent does not cover the images of `rows`")
        out = ops.diffaug_bwd(pair[0], pair[1], table, B, lo)
        return out if isinstance(g16, (tuple, list)) else out[0]


def _check_table(table: torch.Tensor, B: int):
    if table.dtype != torch.float32 or tuple(table.shape) != (2 * B, 8) or not table.is_contiguous() or not table.is_cuda:
        raise ValueError(f"DiffAugment: the table must be a contiguous fp32 [{2 * B}, 8] device tensor")
