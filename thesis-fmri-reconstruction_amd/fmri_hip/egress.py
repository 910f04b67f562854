"""On-device image egress of the fused steps (csrc/egress.hip; include/fmri_hip.h fmri_images_u8).

The pictures of the scripts' epoch, as uint8 pixels written on the device: the ``make_grid(x[:25], nrow=5,
normalize=True)`` of the last training batch, its reconstruction, the validation output and ``model(None, 100)``
(train/train_vgan_stage1.py:465-485, 530-560), and the per-image ``save_image(F.interpolate(im, size=200),
normalize=True)`` of ``evaluate(..., save=True, resize=200)`` (train/train_utils.py:728-735):

    sink, dump = GridSink(capacity=64), ImageDump(resize=200)
    ev = Evaluator(step, val_set, batch=64, rng=DeviceRng(seed_eval, dev), grids=sink, dump=dump, generate=100)
    for epoch in range(epochs):
        for _ in range(steps_per_epoch):
            replay()
        ev.train_batch()                # + grids train_truth / train_output
        ev.run()                        # + grids valid_truth / valid_output / random, and the dump of every image
    g = sink.images()                   # ONE sync: the grids of the last min(passes, capacity) passes
    write_png("out", dump.images())     # reconstruction and truth of every validation image of the last pass

File names, figures and TensorBoard stay with the caller; ``write_png`` is a convenience on top of the arrays.

Nothing here synchronises with the host except ``GridSink.images`` and ``ImageDump.images``.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import lib, ops

_P = lib.ptr

KINDS = ("train_truth", "train_output", "valid_truth", "valid_output", "random")


def _pad4(n: int) -> int:
    return (int(n) + 3) // 4 * 4


def _check16(images16: torch.Tensor, what: str):
    if images16.dtype != torch.float16 or images16.dim() != 4 or images16.shape[3] != 8 or not images16.is_contiguous():
        raise ValueError(f"{what}: images must be a contiguous fp16 [n, H, W, 8] tensor (channels 0..2 real)")
    if images16.shape[0] < 1:
        raise ValueError(f"{what}: no images")
    ops.require_gpu(images16)


def _workspace(n: int, device) -> torch.Tensor:
    return torch.empty(lib.load().fmri_images_u8_ws_bytes(n) // 4, dtype=torch.float32, device=device)


def grid_shape(n: int, H: int, W: int, nrow: int = 5, padding: int = 2) -> Tuple[int, int]:
    """(rows, columns) of ``make_grid`` of ``n`` images of H x W: the bare image for n == 1."""
    if n == 1:
        return H, W
    xmaps = min(nrow, n)
    ymaps = (n + xmaps - 1) // xmaps
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding


def images_u8(images16: torch.Tensor, resize: Optional[int] = None) -> torch.Tensor:
    """uint8 [n, R, R, 3] (R = H without ``resize``): every image normalised to its own range and resized with
    nearest-neighbour indices, the bytes of ``save_image(F.interpolate(im, size=resize), normalize=True)``."""
    _check16(images16, "images_u8")
    n, H, W, _ = images16.shape
    R = 0 if resize is None else int(resize)
    if resize is not None and R < max(H, W):
        raise ValueError(f"images_u8: resize = {resize} is smaller than the {H} x {W} images")
    Ho, Wo = (R, R) if R else (H, W)
    total = n * Ho * Wo * 3
    out = torch.empty(_pad4(total), dtype=torch.uint8, device=images16.device)
    ws = _workspace(n, images16.device)
    lib.call("fmri_images_u8", _P(images16), n, H, W, 3, 8, 0, R, 1, 0, _P(ws), ws.numel() * 4, _P(out), None, 0, 1, None)
    return out[:total].view(n, Ho, Wo, 3)


def grid_u8(images16: torch.Tensor, nrow: int = 5, padding: int = 2) -> torch.Tensor:
    """uint8 [Hg, Wg, 3]: ``make_grid(images, nrow, padding, normalize=True)`` as ``save_image`` quantises it."""
    _check16(images16, "grid_u8")
    if int(nrow) != nrow or nrow < 1 or int(padding) != padding or padding < 0:
        raise ValueError("grid_u8: nrow >= 1 and padding >= 0")
    n, H, W, _ = images16.shape
    Hg, Wg = grid_shape(n, H, W, nrow, padding)
    out = torch.empty(_pad4(Hg * Wg * 3), dtype=torch.uint8, device=images16.device)
    ws = _workspace(n, images16.device)
    lib.call("fmri_images_u8", _P(images16), n, H, W, 3, 8, 1, 0, int(nrow), int(padding), _P(ws), ws.numel() * 4, _P(out),
             None, 0, 1, None)
    return out[:Hg * Wg * 3].view(Hg, Wg, 3)


class GridSink:
    """A device ring of the last ``capacity`` passes' image grids (``grids=`` of ``Evaluator``): per pass one grid of the
    first ``count`` images of each kind in ``KINDS``.  The slot of a write is chosen ON THE DEVICE, from the evaluator's
    pass counter (``ev.log.counter``, what ``fmri_trainlog_append`` increments): enqueue order is the only ordering, as
    for the log ring.  A kind that holds fewer than ``count`` images (a small training batch, a short last validation
    batch) gets ``make_grid``'s geometry for that many: its grid is smaller than the slot, which is sized for ``count``.

    ``image_size``: the side of the images; None: that of the first evaluator the sink is given to.  A sink belongs to
    one evaluator."""

    def __init__(self, capacity: int = 64, count: int = 25, nrow: int = 5, padding: int = 2,
                 image_size: Optional[int] = None):
        if int(capacity) != capacity or capacity < 1:
            raise ValueError("GridSink: capacity must be an integer >= 1")
        if int(count) != count or count < 1:
            raise ValueError("GridSink: count must be an integer >= 1")
        if int(nrow) != nrow or nrow < 1 or int(padding) != padding or padding < 0:
            raise ValueError("GridSink: nrow >= 1 and padding >= 0")
        self.capacity, self.count, self.nrow, self.padding = int(capacity), int(count), int(nrow), int(padding)
        self.size = None if image_size is None else (int(image_size), int(image_size))
        self.ring: Optional[torch.Tensor] = None
        self._counter: Optional[torch.Tensor] = None
        self.shapes: Dict[str, Tuple[int, int]] = {}

    def attach(self, device, H: int, W: int, counter: torch.Tensor):
        """(the evaluator's constructor)  ``counter``: the device int64 pass counter the slots follow."""
        if self.ring is not None:
            raise ValueError("GridSink: already attached to an evaluator (a sink follows one pass counter)")
        if self.size is not None and self.size != (H, W):
            raise ValueError(f"GridSink: built for {self.size[0]} x {self.size[1]} images, the evaluator's are {H} x {W}")
        self.size = (H, W)
        Hg, Wg = grid_shape(self.count, H, W, self.nrow, self.padding)
        self.kind_stride = _pad4(Hg * Wg * 3)                # a grid is written as dwords
        K = len(KINDS)
        head = (8 + K * self.capacity + 15) // 16 * 16        # [passes: int64 | present: K x capacity], 16-byte rounded
        # one block, one copy in images(): [head | ring: capacity x K x kind_stride]
        self.blk = torch.zeros(head + self.capacity * K * self.kind_stride, dtype=torch.uint8, device=device)
        self._passes = self.blk[:8].view(torch.int64)
        self.present = self.blk[8:8 + K * self.capacity].view(K, self.capacity)
        self.ring = self.blk[head:].view(self.capacity, K, self.kind_stride)
        self._opened = torch.zeros(1, dtype=torch.int64, device=device)
        self._counter = counter
        self._ws = _workspace(self.count, device)

    def open(self):
        """Enqueue the opening of the current pass's slot: its ``present`` flags are cleared by the first call of a
        pass, on the device (a host memset would not be repeated by a replay); later calls of the pass do nothing."""
        lib.call("fmri_images_u8_open", _P(self._counter), self.capacity, _P(self._opened), _P(self.present),
                 self.capacity, len(KINDS))

    def write(self, kind: str, images16: torch.Tensor):
        """Enqueue the grid of the first ``count`` images of ``images16`` into the current pass's slot."""
        k = KINDS.index(kind)
        _check16(images16, "GridSink.write")
        n, H, W = min(self.count, images16.shape[0]), images16.shape[1], images16.shape[2]
        if (H, W) != self.size:
            raise ValueError(f"GridSink: built for {self.size[0]} x {self.size[1]} images, got {H} x {W}")
        self.shapes[kind] = grid_shape(n, H, W, self.nrow, self.padding)
        self.open()
        lib.call("fmri_images_u8", _P(images16), n, H, W, 3, 8, 1, 0, self.nrow, self.padding, _P(self._ws),
                 self._ws.numel() * 4, _P(self.ring[0, k]), _P(self._counter), len(KINDS) * self.kind_stride,
                 self.capacity, _P(self.present[k]))

    def images(self) -> Dict[str, np.ndarray]:
        """ONE sync: ``"pass"`` (int64 [rows], absolute pass numbers), per kind uint8 [rows, Hg, Wg, 3] (only the kinds
        written so far; a kind's geometry is that of the images it holds) and ``"present"`` (bool [rows, 5], in
        ``KINDS`` order: which grids the pass wrote -- the others hold bytes of an earlier pass), over the last
        min(passes, capacity) completed passes, oldest first.  Call it between passes."""
        if self.ring is None:
            raise RuntimeError("GridSink.images(): not attached to an evaluator")
        self._passes.copy_(self._counter)
        raw = self.blk.cpu().numpy()
        n = int(raw[:8].view(np.int64)[0])
        K = len(KINDS)
        passes = np.arange(max(0, n - self.capacity), n, dtype=np.int64)
        slots = passes % self.capacity
        head = raw.size - self.capacity * K * self.kind_stride
        ring = raw[head:].reshape(self.capacity, K, self.kind_stride)
        out: Dict[str, np.ndarray] = {"pass": passes}
        for kind, (Hg, Wg) in self.shapes.items():
            out[kind] = ring[slots, KINDS.index(kind), :Hg * Wg * 3].reshape(len(passes), Hg, Wg, 3).copy()
        out["present"] = raw[8:8 + K * self.capacity].reshape(K, self.capacity)[:, slots].T != 0
        return out


class ImageDump:
    """Device uint8 [2][N][R][R][3] (``dump=`` of ``Evaluator``): the reconstruction and the ground truth of every
    validation image of the last pass in dataset order, each normalised to its own range and resized to ``resize`` x
    ``resize`` with nearest-neighbour indices (None: the images' own size) -- what ``evaluate(save=True, resize=...)``
    writes as files.  Every pass overwrites it, as ``evaluate()`` overwrites its files.  The bytes of one image must be a
    multiple of four (an even side): a batch is written as dwords at its row offset."""

    def __init__(self, resize: Optional[int] = 200):
        if resize is not None and (int(resize) != resize or resize < 1):
            raise ValueError("ImageDump: resize must be None or an integer >= 1")
        self.resize = None if resize is None else int(resize)
        self.buf: Optional[torch.Tensor] = None

    def attach(self, device, N: int, H: int, W: int, batch: int):
        """(the evaluator's constructor)"""
        if self.buf is not None:
            raise ValueError("ImageDump: already attached to an evaluator")
        R = self.resize
        if R is not None and R < max(H, W):
            raise ValueError(f"ImageDump: resize = {R} is smaller than the {H} x {W} images")
        Ho, Wo = (H, W) if R is None else (R, R)
        if (Ho * Wo * 3) % 4:
            raise ValueError(f"ImageDump: {Ho} x {Wo} x 3 bytes per image are no multiple of four -- use an even size")
        self.buf = torch.zeros(2, N, Ho, Wo, 3, dtype=torch.uint8, device=device)
        self._ws = _workspace(batch, device)

    def write(self, half: int, row0: int, images16: torch.Tensor):
        """Enqueue images ``row0 ..`` of half 0 (reconstruction) or 1 (truth)."""
        n, H, W, _ = images16.shape
        lib.call("fmri_images_u8", _P(images16), n, H, W, 3, 8, 0, self.resize or 0, 1, 0, _P(self._ws),
                 self._ws.numel() * 4, _P(self.buf[half, row0]), None, 0, 1, None)

    def images(self) -> Dict[str, np.ndarray]:
        """One sync: ``"output"`` and ``"truth"``, uint8 [N, R, R, 3] each."""
        if self.buf is None:
            raise RuntimeError("ImageDump.images(): not attached to an evaluator")
        raw = self.buf.cpu().numpy()
        return {"output": raw[0], "truth": raw[1]}


def write_png(directory: str, arrays: Dict[str, np.ndarray]) -> int:
    """Host helper: every uint8 [rows, H, W, 3] (or [H, W, 3]) array of ``arrays`` as ``<directory>/<name>_<row>.png``;
    returns the number of files.  Needs PIL; nothing else here does."""
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("write_png needs PIL (pillow)") from e
    os.makedirs(directory, exist_ok=True)
    files = 0
    for name, a in arrays.items():
        a = np.asarray(a)
        if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.shape[-1] != 3:
            continue                                    # "pass", "present"
        for r, im in enumerate(a[None] if a.ndim == 3 else a):
            Image.fromarray(np.ascontiguousarray(im)).save(os.path.join(directory, f"{name}_{r:05d}.png"))
            files += 1
    return files
