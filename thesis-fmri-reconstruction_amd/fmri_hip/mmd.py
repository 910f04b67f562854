"""MMD latent penalty with the inverse-multiquadratic kernel (Tolstikhin et al., ICLR 2018): the second WAE penalty,
computed by csrc/mmd.hip through the C ABI (include/fmri_hip.h fmri_mmd_imq).

    imq_mmd(q, p, sigma2=0.25, scales=SCALES)   unbiased statistic MMD_u(q, p) as a torch.autograd.Function;
                                                only ``q`` receives a gradient

GPU tensors only, like the rest of the engine: a CPU tensor is an error, there is no eager fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import lib
from .ops import require_gpu

_P = lib.ptr
SCALES = (0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0)


def ws_bytes(n: int, d: int) -> int:
    b = lib.load().fmri_mmd_imq_ws_bytes(n, d)
    if b < 0:
        raise RuntimeError(f"fmri_mmd_imq: unsupported geometry n={n} d={d} (n >= 2, d a multiple of 64 up to 1024)")
    return b


def _rows(t: torch.Tensor, name: str) -> torch.Tensor:
    require_gpu(t)
    if t.dim() != 2 or t.dtype != torch.float32:
        raise RuntimeError(f"imq_mmd: {name} must be an fp32 matrix [n, d], got {t.dtype} {tuple(t.shape)}")
    if t.stride(1) != 1 or t.stride(0) % 4 or t.data_ptr() % 16:
        t = t.contiguous()
    return t


def mmd_imq(q: torch.Tensor, p: torch.Tensor, sigma2: float = 0.25, scales: Sequence[float] = SCALES, w: float = 1.0,
            total: Optional[torch.Tensor] = None, dq: Optional[torch.Tensor] = None, gscale: float = 1.0):
    """Enqueue one fmri_mmd_imq: ``total`` (fp32 device scalar, may be None) += w * MMD_u(q, p); ``dq`` (fp32 [n, d] view
    with unit column stride, may be None) = gscale * w * dMMD_u/dq.  Rows of q / p may be padded (leading dimension
    >= d).  Nothing is synchronised; the workspace comes from torch's caching allocator (graph-capturable)."""
    q, p = _rows(q, "q"), _rows(p, "p")
    n, d = q.shape
    if n < 2:
        raise ValueError(f"imq_mmd: the unbiased statistic needs n >= 2 rows (got {n})")
    if p.shape != q.shape:
        raise ValueError(f"imq_mmd: q {tuple(q.shape)} and p {tuple(p.shape)} differ")
    if dq is not None and (dq.dtype != torch.float32 or dq.shape != q.shape or dq.stride(1) != 1):
        raise ValueError("imq_mmd: dq must be an fp32 [n, d] view with unit column stride")
    sc = (C.c_float * len(scales))(*[float(s) for s in scales])
    nb = ws_bytes(n, d)
    ws = torch.empty(nb, dtype=torch.uint8, device=q.device)
    lib.call("fmri_mmd_imq", _P(q), q.stride(0), _P(p), p.stride(0), n, d, float(sigma2), sc, len(scales), float(w),
             _P(total), _P(dq), dq.stride(0) if dq is not None else d, float(gscale), _P(ws), nb)


class _ImqMmd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, p, sigma2, scales):
        qd = q.detach()
        total = torch.zeros(1, dtype=torch.float32, device=q.device)
        dq = torch.empty(qd.shape, dtype=torch.float32, device=q.device) if ctx.needs_input_grad[0] else None
        mmd_imq(qd, p.detach(), sigma2, scales, total=total, dq=dq)
        ctx.save_for_backward(dq)
        return total.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dq,) = ctx.saved_tensors
        return (None if dq is None else dq * g), None, None, None


def imq_mmd(q: torch.Tensor, p: torch.Tensor, sigma2: float = 0.25, scales: Sequence[float] = SCALES) -> torch.Tensor:
    """Unbiased MMD_u(q, p) with the IMQ kernel k(a, b) = sum_s C_s / (C_s + |a - b|^2), C_s = 2 d sigma2 s, as a 0-dim
    fp32 tensor (see include/fmri_hip.h fmri_mmd_imq).  ``q`` [n, d] receives the gradient, ``p`` none; n >= 2.  The
    forward pass also computes dMMD/dq (one fused kernel), the backward pass only scales it."""
    require_gpu(q)
    require_gpu(p)
    if q.dim() != 2 or q.shape[0] < 2:
        raise ValueError(f"imq_mmd: q must be [n >= 2, d], got {tuple(q.shape)}")
    return _ImqMmd.apply(q, p, float(sigma2), tuple(float(s) for s in scales))
