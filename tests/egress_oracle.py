"""torch-CPU restatement of the pictures the scripts write, the oracle of csrc/egress.hip (torchvision is not a
dependency of the tests): torchvision 0.5.0's ``utils.make_grid`` / ``save_image`` with ``normalize=True`` and
``F.interpolate``'s default nearest mode, run on the fp32 values of the fp16 inputs.

    grid_u8(x, nrow, padding)   uint8 [Hg, Wg, 3]: make_grid(x, nrow, padding, normalize=True), then save_image's
                                mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(uint8)
    images_u8(x, resize)        uint8 [n, R, R, 3]: per image save_image(F.interpolate(im, size=resize), normalize=True)
"""
import math

import torch
import torch.nn.functional as F


def from_layout(x16: torch.Tensor, C: int = 3) -> torch.Tensor:
    """fp16 [n, H, W, 8] (the engine's image layout, any device) -> fp32 NCHW of the real channels, on the CPU."""
    return x16[..., :C].permute(0, 3, 1, 2).float().cpu().contiguous()


def norm_ip(img: torch.Tensor, lo: float, hi: float) -> None:
    img.clamp_(min=lo, max=hi)
    img.add_(-lo).div_(hi - lo + 1e-5)


def make_grid(tensor: torch.Tensor, nrow: int = 8, padding: int = 2, normalize: bool = False) -> torch.Tensor:
    """[n, 3, H, W] -> [3, Hg, Wg]; ``range=None, scale_each=False, pad_value=0``."""
    assert tensor.dim() == 4 and tensor.shape[1] == 3
    if normalize:
        tensor = tensor.clone()
        norm_ip(tensor, float(tensor.min()), float(tensor.max()))
    if tensor.size(0) == 1:
        return tensor.squeeze(0)
    nmaps = tensor.size(0)
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height, width = int(tensor.size(2) + padding), int(tensor.size(3) + padding)
    grid = tensor.new_full((3, height * ymaps + padding, width * xmaps + padding), 0)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(2, x * width + padding, width - padding).copy_(
                tensor[k])
            k += 1
    return grid


def to_u8(grid: torch.Tensor) -> torch.Tensor:
    """save_image's quantisation: [3, H, W] fp32 -> uint8 [H, W, 3]."""
    return grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).contiguous()


def grid_u8(x: torch.Tensor, nrow: int = 5, padding: int = 2) -> torch.Tensor:
    return to_u8(make_grid(x.float(), nrow=nrow, padding=padding, normalize=True))


def images_u8(x: torch.Tensor, resize=None) -> torch.Tensor:
    out = []
    for im in x.float():
        im = im[None]
        if resize is not None:
            im = F.interpolate(im, size=resize)
        out.append(to_u8(make_grid(im, normalize=True)))
    return torch.stack(out)
