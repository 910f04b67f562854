"""TEST INFRASTRUCTURE ONLY -- float64 restatement of fmri_image_metrics (csrc/evalmetrics.hip) over the engine's image
layout, fp16 [N][H][W][8] with channels 0..C-1 real: PearsonCorrelation over the whole batch, mean SSIM and MSE, on top of
ident_oracle.pcc64 / ssim64.  The optional per-channel affine v * scale[c] + shift[c] (denormalize_image) is evaluated in
numpy fp32 -- one rounding per operation, as the kernel does it -- and everything behind it in float64."""
import numpy as np
import torch

import ident_oracle as IO

DENORM = ((0.229, 0.224, 0.225), (0.485, 0.456, 0.406))      # (scale = std, shift = mean) of the GPU cases


def to_layout(x: torch.Tensor, pad_value: float = 0.0) -> torch.Tensor:
    """fp32 [N, C, H, W] -> fp16 [N, H, W, 8]: channels 0..C-1 rounded to fp16, lanes C..7 = ``pad_value``."""
    n, c, h, w = x.shape
    out = torch.full((n, h, w, 8), pad_value, dtype=torch.float16)
    out[..., :c] = x.permute(0, 2, 3, 1).half()
    return out


def from_layout(x16: torch.Tensor, C: int, scale=None, shift=None) -> torch.Tensor:
    """fp16 [N, H, W, 8] -> float64 [N, C, H, W] of v (or of fp32(fp32(v * scale[c]) + shift[c]))."""
    v = x16[..., :C].float().numpy()
    if scale is not None:
        v = v * np.asarray(scale, dtype=np.float32)[:C] + np.asarray(shift, dtype=np.float32)[:C]
        assert v.dtype == np.float32
    return torch.from_numpy(v.astype(np.float64)).permute(0, 3, 1, 2).contiguous()


def metrics64(a: torch.Tensor, b: torch.Tensor):
    """(pcc, ssim, mse) of two [N, C, H, W] batches as Python floats, every intermediate float64."""
    a, b = a.double(), b.double()
    return IO.pcc64(a, b).item(), IO.ssim64(a, b)[0].item(), ((a - b) ** 2).mean().item()


def image_metrics64(pred16: torch.Tensor, truth16: torch.Tensor, C: int = 3, scale=None, shift=None):
    """``metrics64`` of two batches in the engine layout (the restatement of fmri_image_metrics)."""
    return metrics64(from_layout(pred16, C, scale, shift), from_layout(truth16, C, scale, shift))
