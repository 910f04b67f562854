"""Contrastive latent alignment: the symmetric InfoNCE ("CLIP") loss between the cognitive encoder's means and the
teacher's means, computed by csrc/contrast.hip through the C ABI (include/fmri_hip_contrast.h fmri_latent_nce).

    LatentContrast(weight, temperature, symmetric)   the ``contrast=`` term of WaeStep (Stages II / III)
    info_nce(q, t, temperature=0.07, symmetric=True) the loss as a torch.autograd.Function; only ``q`` receives a
                                                     gradient
    latent_nce(q, t, temperature, ...)               the enqueue-only wrapper (value, in-batch top-1 rate, gradient)

GPU tensors only, like the rest of the engine: a CPU tensor is an error, there is no eager fallback.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import lib
from .ops import require_gpu

_P = lib.ptr
TAU_MIN, TAU_MAX = 0.01, 1.0
N_MAX = 4096


def _check_tau(tau: float, who: str) -> float:
    tau = float(tau)
    if not (TAU_MIN <= tau <= TAU_MAX):
        raise ValueError(f"{who}: temperature must lie in [{TAU_MIN}, {TAU_MAX}], got {tau}")
    return tau


@dataclass
class LatentContrast:
    """``contrast=`` of WaeStep: ``weight`` * InfoNCE(cognitive means, teacher means) at ``temperature``; ``symmetric``
    averages the fMRI -> image and image -> fMRI directions."""
    weight: float = 1.0
    temperature: float = 0.07
    symmetric: bool = True

    def __post_init__(self):
        self.temperature = _check_tau(self.temperature, "LatentContrast")
        self.weight = float(self.weight)
        if not (self.weight >= 0.0 and self.weight < float("inf")):
            raise ValueError(f"LatentContrast: weight must be finite and >= 0, got {self.weight}")
        self.symmetric = bool(self.symmetric)


def ws_bytes(n: int, d: int) -> int:
    b = lib.load().fmri_latent_nce_ws_bytes(n, d)
    if b < 0:
        raise RuntimeError(f"fmri_latent_nce: unsupported geometry n={n} d={d} (2 <= n <= {N_MAX}, d a multiple of 64 up "
                           "to 1024)")
    return b


def _rows(t: torch.Tensor, name: str) -> torch.Tensor:
    require_gpu(t)
    if t.dim() != 2 or t.dtype != torch.float32:
        raise RuntimeError(f"info_nce: {name} must be an fp32 matrix [n, d], got {t.dtype} {tuple(t.shape)}")
    if t.stride(1) != 1 or t.stride(0) % 4 or t.data_ptr() % 16:
        t = t.contiguous()
    return t


def latent_nce(q: torch.Tensor, t: torch.Tensor, temperature: float, symmetric: bool = True, w: float = 1.0,
               total: Optional[torch.Tensor] = None, top1: Optional[torch.Tensor] = None,
               dq: Optional[torch.Tensor] = None, gscale: float = 1.0):
    """Enqueue one fmri_latent_nce: ``total`` (fp32 device scalar, may be None) += w * L; ``top1`` (the same) += the
    in-batch top-1 retrieval rate; ``dq`` (fp32 [n, d] view with unit column stride, may be None) = gscale * w * dL/dq.
    Rows of q / t may be padded (leading dimension >= d).  Nothing is synchronised; the workspace comes from torch's
    caching allocator (graph-capturable)."""
    q, t = _rows(q, "q"), _rows(t, "t")
    n, d = q.shape
    tau = _check_tau(temperature, "info_nce")
    if n < 2:
        raise ValueError(f"info_nce: in-batch negatives need n >= 2 rows (got {n})")
    if t.shape != q.shape:
        raise ValueError(f"info_nce: q {tuple(q.shape)} and t {tuple(t.shape)} differ")
    if dq is not None and (dq.dtype != torch.float32 or dq.shape != q.shape or dq.stride(1) != 1):
        raise ValueError("info_nce: dq must be an fp32 [n, d] view with unit column stride")
    nb = ws_bytes(n, d)
    ws = torch.empty(nb, dtype=torch.uint8, device=q.device)
    lib.call("fmri_latent_nce", _P(q), q.stride(0), _P(t), t.stride(0), n, d, tau, int(bool(symmetric)), float(w),
             _P(total), _P(top1), _P(dq), dq.stride(0) if dq is not None else d, float(gscale), _P(ws), nb)


class _InfoNce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, t, tau, symmetric):
        qd = q.detach()
        total = torch.zeros(1, dtype=torch.float32, device=q.device)
        dq = torch.empty(qd.shape, dtype=torch.float32, device=q.device) if ctx.needs_input_grad[0] else None
        latent_nce(qd, t.detach(), tau, symmetric, total=total, dq=dq)
        ctx.save_for_backward(dq)
        return total.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dq,) = ctx.saved_tensors
        return (None if dq is None else dq * g), None, None, None


def info_nce(q: torch.Tensor, t: torch.Tensor, temperature: float = 0.07, symmetric: bool = True) -> torch.Tensor:
    """InfoNCE between the paired rows of ``q`` and ``t`` [n, d] (cosine logits / temperature; ``symmetric``: the mean of
    the two retrieval directions) as a 0-dim fp32 tensor (see include/fmri_hip_contrast.h fmri_latent_nce).  ``q`` receives the
    gradient, ``t`` none; n >= 2.  The forward pass also computes dL/dq, the backward pass only scales it."""
    require_gpu(q)
    require_gpu(t)
    if q.dim() != 2 or q.shape[0] < 2:
        raise ValueError(f"info_nce: q must be [n >= 2, d], got {tuple(q.shape)}")
    return _InfoNce.apply(q, t, _check_tau(temperature, "info_nce"), bool(symmetric))
