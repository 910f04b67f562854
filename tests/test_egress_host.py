"""Host side of the image egress (csrc/egress.hip, fmri_hip/egress.py): the torch-CPU oracle (tests/egress_oracle.py)
against bytes worked out by hand, and the library's size functions and argument checks -- no kernel is launched."""
import ctypes

import pytest
import torch

import egress_oracle as EG


@pytest.fixture(scope="module")
def lib():
    from fmri_hip import build, lib as L
    build.build(verbose=False)
    return L.load()


def test_oracle_bytes_of_a_2x2_image_by_hand():
    """Range [0, 1]: d = fp32(1.00001), b = trunc(x / d * 255 + 0.5): 0.25 -> 63.749 + 0.5 -> 64, 0.5 -> 127.4987 + 0.5
    -> 127 (the + 1e-5 keeps it under 128), 0.75 -> 191.248 + 0.5 -> 191, 1 -> 254.997 + 0.5 -> 255."""
    x = torch.tensor([[[0.0, 0.25], [0.5, 0.75]], [[1.0, 0.5], [0.25, 0.0]], [[0.75, 0.75], [1.0, 0.5]]])[None]
    want = torch.tensor([[[0, 255, 191], [64, 127, 191]], [[127, 64, 255], [191, 0, 127]]], dtype=torch.uint8)
    assert torch.equal(EG.grid_u8(x), want)                     # n == 1: the bare image
    assert torch.equal(EG.images_u8(x)[0], want)
    # the same image moved and scaled has the same bytes up to the 1e-5: [-1, 1] -> d = 2.00001
    assert torch.equal(EG.images_u8(x * 2 - 1)[0], torch.tensor(
        [[[0, 255, 191], [64, 127, 191]], [[127, 64, 255], [191, 0, 127]]], dtype=torch.uint8))
    # nearest-neighbour 2 -> 4: every pixel twice in each direction
    up = EG.images_u8(x, resize=4)[0]
    assert up.shape == (4, 4, 3) and torch.equal(up[::2, ::2], want) and torch.equal(up[1::2, 1::2], want)


def test_oracle_grid_geometry_and_padding():
    g = torch.Generator().manual_seed(0)
    x = torch.rand(7, 3, 16, 16, generator=g) + 0.5             # strictly positive: only the minimum maps to 0
    grid = EG.grid_u8(x, nrow=5, padding=2)
    assert grid.shape == (2 * 18 + 2, 5 * 18 + 2, 3)
    mask = torch.zeros(grid.shape[:2], dtype=torch.bool)
    for k in range(7):
        r, c = (k // 5) * 18 + 2, (k % 5) * 18 + 2
        mask[r:r + 16, c:c + 16] = True
    assert int(grid[~mask].max()) == 0                          # padding and the three empty cells
    assert float((grid[mask] == 0).float().mean()) < 0.01       # only values within 1 / 510 of the range above the minimum
    lo, hi = float(x.min()), float(x.max())
    k = 6
    r, c = 18 + 2, 18 + 2
    want = ((x[k] - lo) / (hi - lo + 1e-5) * 255 + 0.5).clamp(0, 255).permute(1, 2, 0)
    assert (grid[r:r + 16, c:c + 16].float() - want).abs().max() <= 1.0
    assert EG.grid_u8(x[:1]).shape == (16, 16, 3)               # n == 1: no padding
    assert EG.grid_u8(x[:3], nrow=5, padding=2).shape == (20, 3 * 18 + 2, 3)      # xmaps = min(nrow, n)


def test_oracle_constant_image_is_black():
    x = torch.full((1, 3, 4, 4), 0.37)
    assert int(EG.images_u8(x).max()) == 0 and int(EG.grid_u8(x).max()) == 0


def test_library_sizes(lib):
    assert hasattr(lib, "fmri_images_u8") and hasattr(lib, "fmri_images_u8_open")
    assert lib.fmri_images_u8_ws_bytes(1) == 8 and lib.fmri_images_u8_ws_bytes(25) == 200
    assert lib.fmri_images_u8_ws_bytes(0) < 0
    ob = lib.fmri_images_u8_out_bytes
    assert ob(3, 16, 16, 0, 0, 1, 0) == 3 * 16 * 16 * 3 and ob(3, 16, 16, 0, 50, 1, 0) == 3 * 50 * 50 * 3
    assert ob(7, 16, 16, 1, 0, 5, 2) == 38 * 92 * 3 and ob(1, 16, 16, 1, 0, 5, 2) == 16 * 16 * 3
    assert ob(26, 64, 64, 1, 0, 5, 2) == (6 * 66 + 2) * (5 * 66 + 2) * 3
    assert ob(0, 16, 16, 0, 0, 1, 0) < 0 and ob(3, 16, 16, 2, 0, 1, 0) < 0 and ob(3, 16, 16, 1, 0, 0, 2) < 0
    from fmri_hip.egress import grid_shape
    assert grid_shape(7, 16, 16) == (38, 92) and grid_shape(1, 16, 16) == (16, 16) and grid_shape(25, 64, 64) == (332, 332)


def test_library_argument_checks_without_gpu(lib):
    """Every refusal is made before a launch: fake (aligned, non-NULL) pointers never reach a kernel."""
    P = ctypes.c_void_p
    src, ws, out = P(0x10000), P(0x20000), P(0x30000)

    def call(src=src, n=3, H=16, W=16, C=3, Cp=8, mode=0, R=0, nrow=5, padding=2, ws=ws, ws_bytes=1 << 20, out=out,
             slot=None, stride=0, mod=1, present=None):
        return lib.fmri_images_u8(src, n, H, W, C, Cp, mode, R, nrow, padding, ws, ws_bytes, out, slot, stride, mod,
                                  present, None)
    E_BADARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -4
    assert call(Cp=4) == E_UNSUPPORTED and call(C=4) == E_UNSUPPORTED and call(C=1) == E_UNSUPPORTED
    assert call(src=None) == E_BADARG and call(ws=None) == E_BADARG and call(out=None) == E_BADARG
    assert call(src=P(0x10008)) == E_BADARG                     # 16-byte loads
    assert call(out=P(0x30002)) == E_BADARG                     # dword stores
    assert call(n=0) == E_BADARG and call(H=0) == E_BADARG and call(mode=2) == E_BADARG and call(R=-1) == E_BADARG
    assert call(mode=1, nrow=0) == E_BADARG and call(mode=1, padding=-1) == E_BADARG
    assert call(slot=P(0x40000), mod=0) == E_BADARG and call(slot=P(0x40000), stride=6, mod=4) == E_BADARG
    assert call(slot=P(0x40004), stride=8, mod=4) == E_BADARG
    assert call(R=8) == E_UNSUPPORTED                           # smaller than the image: the range would change
    assert call(ws_bytes=3 * 8 - 1) == E_WORKSPACE and call(mode=1, ws_bytes=0) == E_WORKSPACE
    assert call(n=20000, R=200, ws_bytes=1 << 20) == E_UNSUPPORTED      # 2.4e9 output bytes
    assert lib.fmri_images_u8_open(None, 4, P(0x100), P(0x200), 4, 5, None) == E_BADARG
    assert lib.fmri_images_u8_open(P(0x100), 4, P(0x108), P(0x200), 3, 5, None) == E_BADARG      # stride < slots


def test_python_argument_checks():
    from fmri_hip.egress import GridSink, ImageDump, images_u8
    with pytest.raises(ValueError, match="count"):
        GridSink(count=0)
    with pytest.raises(ValueError, match="capacity"):
        GridSink(capacity=0)
    with pytest.raises(ValueError, match="resize"):
        ImageDump(resize=0)
    with pytest.raises(RuntimeError, match="attached"):
        GridSink().images()
    with pytest.raises(ValueError, match="fp16"):
        images_u8(torch.zeros(2, 16, 16, 8))
    from fmri_hip.rng import SID_DISTRACT, SID_GENERATE, SID_PERM
    assert SID_GENERATE == 11 and SID_GENERATE not in (SID_DISTRACT, SID_PERM)
