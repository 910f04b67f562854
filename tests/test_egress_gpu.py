"""The image egress kernels (csrc/egress.hip; fmri_hip/egress.py images_u8 / grid_u8) against the torch-CPU restatement
of make_grid / save_image / F.interpolate (tests/egress_oracle.py): every byte, torch.equal."""
import ctypes

import pytest
import torch

import egress_oracle as EG

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INPUTS = ("plain", "wide", "min_last", "max_last")


def _images(n, H, W, kind, seed=0):
    """fp16 [n, H, W, 8]: channels 0..2 random at scale 1.3, lanes 3..7 NaN and 65504 in turn (they must reach neither
    the range nor a byte), image 1 constant (n >= 2).  ``wide``: image 0 spans -60000 .. 60000.  ``min_last`` /
    ``max_last``: the batch's (and the last image's) minimum / maximum sits in lane 2 of the last pixel of the last image
    and nowhere else."""
    g = torch.Generator().manual_seed(seed + 1000 * n + H)
    x = (torch.randn(n, H, W, 8, generator=g) * 1.3).half()
    junk = torch.tensor([float("nan"), 65504.0, float("nan"), 65504.0, float("nan")], dtype=torch.float16)
    x[..., 3:] = junk
    x[0, 0, 0, 4], x[0, 0, 0, 3] = 65504.0, float("nan")        # ... and the other way round in one pixel
    if n >= 2:
        x[1, :, :, :3] = 0.4375
    if kind == "wide":
        x[0, H // 2, W // 3, 1] = 60000.0
        x[0, H - 1, 0, 0] = -60000.0
    elif kind == "min_last":
        x[n - 1, H - 1, W - 1, 2] = -9.5
    elif kind == "max_last":
        x[n - 1, H - 1, W - 1, 2] = 9.5
    return x


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("n,nrow,padding", [(1, 5, 2), (7, 5, 2), (25, 5, 2), (26, 5, 2), (9, 8, 0)])
def test_grid_matches_oracle(n, nrow, padding, kind):
    from fmri_hip.egress import grid_u8
    x = _images(n, 16, 16, kind)
    got = grid_u8(x.to(DEV), nrow=nrow, padding=padding).cpu()
    want = EG.grid_u8(EG.from_layout(x), nrow=nrow, padding=padding)
    assert got.shape == want.shape
    assert torch.equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("n,H,R", [(3, 16, 50), (3, 16, None), (3, 64, 200), (3, 100, 200), (33, 16, 50)],
                         ids=["16to50", "16asis", "64to200", "100to200", "n33"])
def test_images_match_oracle(n, H, R, kind):
    from fmri_hip.egress import images_u8
    x = _images(n, H, H, kind)
    got = images_u8(x.to(DEV), resize=R).cpu()
    want = EG.images_u8(EG.from_layout(x), resize=R)
    assert got.shape == want.shape == (n, R or H, R or H, 3)
    assert torch.equal(got, want), int((got != want).sum())
    if n >= 2:
        assert int(got[1].max()) == 0                           # the constant image


def test_odd_sizes_and_the_tail_dword():
    """15 x 13 images: neither the per-image nor the total byte count is a multiple of four; the wrapper's buffer is, and
    what lies behind the output is written as 0."""
    from fmri_hip import lib
    from fmri_hip.egress import grid_u8, images_u8
    x = _images(3, 15, 13, "plain")
    xd = x.to(DEV)
    assert torch.equal(grid_u8(xd, nrow=2, padding=1).cpu(), EG.grid_u8(EG.from_layout(x), nrow=2, padding=1))
    assert torch.equal(images_u8(xd).cpu(), EG.images_u8(EG.from_layout(x)))
    total = 3 * 15 * 13 * 3
    assert total % 4 == 3
    out = torch.full((total + 1 + 8,), 0xAB, dtype=torch.uint8, device=DEV)
    ws = torch.empty(6, dtype=torch.float32, device=DEV)
    lib.call("fmri_images_u8", xd.data_ptr(), 3, 15, 13, 3, 8, 0, 0, 1, 0, ws.data_ptr(), 24, out.data_ptr(), None, 0, 1,
             None)
    out = out.cpu()
    assert torch.equal(out[:total].view(3, 15, 13, 3), EG.images_u8(EG.from_layout(x)))
    assert out[total:].tolist() == [0] + [0xAB] * 8


def test_ring_addressing_follows_the_device_counter():
    """slot_dev = 0, capacity - 1 and capacity + 1 land in slots 0, capacity - 1 and 1 of a ring pre-filled with 0xAB, touch
    no other slot and set ``present`` only there.  Three 15 x 15 images, padding 1: 17 x 49 x 3 = 2499 bytes, a slot of
    2500 whose last byte is written as 0."""
    from fmri_hip import lib
    cap, n, H, nrow, pad = 4, 3, 15, 5, 1
    x = _images(n, H, H, "plain")
    xd = x.to(DEV)
    want = EG.grid_u8(EG.from_layout(x), nrow=nrow, padding=pad).reshape(-1)
    assert want.numel() == 2499
    stride = 2500
    ws = torch.empty(2 * n, dtype=torch.float32, device=DEV)
    for counter in (0, cap - 1, cap + 1):
        ring = torch.full((cap, stride), 0xAB, dtype=torch.uint8, device=DEV)
        present = torch.zeros(cap, dtype=torch.uint8, device=DEV)
        slot_dev = torch.tensor([counter], dtype=torch.int64, device=DEV)
        lib.call("fmri_images_u8", xd.data_ptr(), n, H, H, 3, 8, 1, 0, nrow, pad, ws.data_ptr(), ws.numel() * 4,
                 ring.data_ptr(), slot_dev.data_ptr(), stride, cap, present.data_ptr())
        ring, present, slot = ring.cpu(), present.cpu(), counter % cap
        assert torch.equal(ring[slot, :2499], want) and int(ring[slot, 2499]) == 0
        others = [s for s in range(cap) if s != slot]
        assert bool((ring[others] == 0xAB).all())
        assert present.tolist() == [int(s == slot) for s in range(cap)]
        assert slot_dev.item() == counter


def test_open_clears_a_slot_once_per_pass():
    from fmri_hip import lib
    cap, kinds = 3, 5
    present = torch.ones(kinds, cap, dtype=torch.uint8, device=DEV)
    counter = torch.tensor([4], dtype=torch.int64, device=DEV)          # slot 1
    opened = torch.zeros(1, dtype=torch.int64, device=DEV)
    args = (counter.data_ptr(), cap, opened.data_ptr(), present.data_ptr(), cap, kinds)
    lib.call("fmri_images_u8_open", *args)
    assert present.cpu().tolist() == [[1, 0, 1]] * kinds and opened.item() == 5
    present[2, 1] = 1                                                   # a write of the pass
    lib.call("fmri_images_u8_open", *args)                              # the same pass again: nothing
    assert present.cpu()[2].tolist() == [1, 1, 1]
    counter += 1                                                        # the next pass: slot 2
    lib.call("fmri_images_u8_open", *args)
    assert present.cpu().tolist() == [[1, 0, 0], [1, 0, 0], [1, 1, 0], [1, 0, 0], [1, 0, 0]] and opened.item() == 6


def test_bytes_do_not_depend_on_deterministic_mode():
    from fmri_hip import ops
    from fmri_hip.egress import grid_u8, images_u8
    xd = _images(26, 16, 16, "wide").to(DEV)
    was = ops.set_deterministic(True)
    try:
        a = (grid_u8(xd), images_u8(xd, resize=50))
        b = (grid_u8(xd), images_u8(xd, resize=50))
        ops.set_deterministic(False)
        c = (grid_u8(xd), images_u8(xd, resize=50))
    finally:
        ops.set_deterministic(was)
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v) and torch.equal(u, w)


def test_wrappers_refuse_what_the_kernel_does_not_take():
    from fmri_hip.egress import images_u8
    with pytest.raises(ValueError, match="smaller"):
        images_u8(_images(2, 16, 16, "plain").to(DEV), resize=8)
    with pytest.raises(RuntimeError, match="MI355X"):
        images_u8(_images(2, 16, 16, "plain"))
