"""n-way identification on the MI355X: the reference's ``objective_assessment`` (train/train_utils.py:752-816) with the
pairwise similarities computed by csrc/ident.hip through the C ABI (include/fmri_hip.h fmri_pcc_matrix, fmri_ssim_pairs).

    pcc_matrix(pred, truth)            [N, M] PCC of every reconstruction against every ground truth (fp32)
    ssim_pairs(pred, truth, pairs)     [P] mean SSIM of the listed (i, j) pairs
    ssim_matrix(pred, truth)           [N, M] mean SSIM of every pair
    n_way(pred, truth, distractors)    bool [N, 2]: ground truth strictly beats every distractor (PCC, SSIM)
    n_way_expected(pred, truth, top)   float64 [2]: the score's exact expectation over the distractor draws
    objective_assessment(model, dataloader, dataset=None, mode=None, top=5)
                                       the reference's function: same signature, same draws, same CPU result
    nway_scores16(pred16, truth16, top, rng=None, ...)
                                       one batch in the engine's fp16 [n, H, W, 8] layout, everything on the device
                                       (fmri_nway_scores, csrc/nway.hip): both matrices, the distractors drawn from a
                                       DeviceRng, the hits, the expectation and a running accumulator

Images are GPU tensors [N, C, H, W]: a CPU tensor is a RuntimeError, there is no eager fallback.  A pair's value is a
bitwise function of the two images (include/fmri_hip.h), so the strict ``>`` of the reference counts as on the host,
also for a batch that holds the same stimulus twice.  An empty batch (N = 0 or M = 0) gives empty results.

Degenerate images.  A NaN image gives NaN PCC and SSIM in its row or column, as in the reference, so it is never a hit.
A constant image has zero variance: its PCC is 0 / 0 = NaN and never a hit.  The reference agrees when the constant's
fp32 mean is exact (0.5, -1.0).  When it is not (0.1), the reference's fp32 ``torch.mean`` is off by a rounding error and
its PCC is rounding noise (|PCC| up to about 1e-7) instead of NaN; the engine's fp64 row mean of a constant row is the
constant itself, so it stays NaN.  SSIM of a constant image is finite.
"""
from __future__ import annotations

import logging
import random
from fractions import Fraction

import torch

from . import lib
from .ops import require_gpu
from .rng import SID_DISTRACT

_P = lib.ptr
_PAIR_CHUNK = 1 << 16           # pairs per fmri_ssim_pairs launch of ssim_matrix


def _images(t: torch.Tensor, name: str) -> torch.Tensor:
    require_gpu(t)
    if t.dim() != 4:
        raise ValueError(f"{name} must be an image batch [N, C, H, W], got shape {tuple(t.shape)}")
    return t.detach().contiguous().float()


def _pair_of_batches(pred, truth):
    a, b = _images(pred, "pred"), _images(truth, "truth")
    if a.shape[1:] != b.shape[1:]:
        raise ValueError(f"pred {tuple(a.shape)} and truth {tuple(b.shape)} differ in their image shape")
    if b.device != a.device:
        raise ValueError(f"pred is on {a.device}, truth on {b.device}")
    return a, b


def _workspace(nbytes: int, what: str, device) -> torch.Tensor:
    if nbytes < 0:
        raise ValueError(f"{what}: unsupported geometry")
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)


def pcc_matrix(pred: torch.Tensor, truth: torch.Tensor) -> torch.Tensor:
    """S[i, j] = PearsonCorrelation(pred[i], truth[j]) as fp32 [N, M] on the device."""
    a, b = _pair_of_batches(pred, truth)
    N, M, D = a.shape[0], b.shape[0], a.shape[1:].numel()
    S = torch.empty(N, M, dtype=torch.float32, device=a.device)
    if N == 0 or M == 0:
        return S
    nb = lib.load().fmri_pcc_matrix_ws_bytes(N, M, D)
    ws = _workspace(nb, "pcc_matrix", a.device)
    lib.call("fmri_pcc_matrix", _P(a), _P(b), N, M, D, _P(S), M, _P(ws), nb)
    return S


def _ssim_pairs(a: torch.Tensor, b: torch.Tensor, pairs: torch.Tensor, out: torch.Tensor):
    """Enqueue one fmri_ssim_pairs; ``pairs`` int32 [P, 2] on the device, in range (checked by the caller)."""
    N, C, H, W = a.shape
    M = b.shape[0]
    nb = lib.load().fmri_ssim_pairs_ws_bytes(N, M, C, H, W)
    ws = _workspace(nb, "ssim_pairs", a.device)
    lib.call("fmri_ssim_pairs", _P(a), _P(b), N, M, C, H, W, _P(pairs), pairs.shape[0], _P(out), _P(ws), nb)


def _check_ssim_geometry(a: torch.Tensor):
    H, W = a.shape[-2:]
    if H < 11 or W < 11:
        raise RuntimeError(f"ssim: images of {H} x {W} are unsupported (H and W must be >= 11, as for fmri_ssim)")


def ssim_pairs(pred: torch.Tensor, truth: torch.Tensor, pairs) -> torch.Tensor:
    """out[p] = StructuralSimilarity(pred[pairs[p, 0]], truth[pairs[p, 1]]) (mean over C, H, W) as fp32 [P]."""
    a, b = _pair_of_batches(pred, truth)
    _check_ssim_geometry(a)
    pairs = torch.as_tensor(pairs)
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype.is_floating_point or pairs.dtype == torch.bool:
        raise ValueError(f"pairs must be an integer tensor [P, 2], got {pairs.dtype} {tuple(pairs.shape)}")
    out = torch.empty(pairs.shape[0], dtype=torch.float32, device=a.device)
    if pairs.shape[0] == 0:
        return out
    lo = pairs.amin(0).tolist()
    hi = pairs.amax(0).tolist()
    if lo[0] < 0 or lo[1] < 0 or hi[0] >= a.shape[0] or hi[1] >= b.shape[0]:
        raise ValueError(f"pairs index outside pred [0, {a.shape[0]}) or truth [0, {b.shape[0]})")
    p32 = pairs.to(device=a.device, dtype=torch.int32).contiguous()
    for s in range(0, p32.shape[0], _PAIR_CHUNK):
        _ssim_pairs(a, b, p32[s:s + _PAIR_CHUNK], out[s:s + _PAIR_CHUNK])
    return out


def ssim_matrix(pred: torch.Tensor, truth: torch.Tensor) -> torch.Tensor:
    """S[i, j] = StructuralSimilarity(pred[i], truth[j]) as fp32 [N, M]: all pairs, issued in blocks of pred rows of at
    most _PAIR_CHUNK pairs each."""
    a, b = _pair_of_batches(pred, truth)
    _check_ssim_geometry(a)
    N, M = a.shape[0], b.shape[0]
    S = torch.empty(N, M, dtype=torch.float32, device=a.device)
    if N == 0 or M == 0:
        return S
    rows = max(1, _PAIR_CHUNK // M)
    for i0 in range(0, N, rows):
        r = min(rows, N - i0)
        ii = torch.arange(r, device=a.device, dtype=torch.int32).repeat_interleave(M)
        jj = torch.arange(M, device=a.device, dtype=torch.int32).repeat(r)
        _ssim_pairs(a[i0:i0 + r], b, torch.stack([ii, jj], 1).contiguous(), S[i0:i0 + r].view(-1))
    return S


def n_way(pred: torch.Tensor, truth: torch.Tensor, distractors) -> torch.Tensor:
    """bool [N, 2] on the device: row i is True where the ground truth ``truth[i]`` scores strictly higher against
    ``pred[i]`` than every ``truth[distractors[i, k]]`` -- column 0 by PCC, column 1 by SSIM.  ``distractors``: integer
    [N, top - 1] (host or device)."""
    a, b = _pair_of_batches(pred, truth)
    N = a.shape[0]
    if b.shape[0] != N:
        raise ValueError(f"n_way: {N} reconstructions against {b.shape[0]} ground-truth images")
    _check_ssim_geometry(a)
    d = torch.as_tensor(distractors)
    if d.dim() != 2 or d.shape[0] != N or d.dtype.is_floating_point or d.dtype == torch.bool:
        raise ValueError(f"distractors must be an integer tensor [N={N}, top - 1], got {d.dtype} {tuple(d.shape)}")
    k = d.shape[1]
    if k == 0 or N == 0:
        return torch.full((N, 2), k == 0, dtype=torch.bool, device=a.device)
    if d.is_cuda:
        lo, hi = d.min().item(), d.max().item()
    else:
        lo, hi = int(d.min()), int(d.max())
    if lo < 0 or hi >= N:
        raise ValueError(f"distractors outside [0, {N})")
    d = d.to(device=a.device, dtype=torch.int64)
    S = pcc_matrix(a, b)
    gt = S.diagonal()
    pcc_ok = (gt[:, None] > S.gather(1, d)).all(1)
    # SSIM of the N ground-truth pairs, then of the N (top - 1) distractor pairs: one launch
    ii = torch.arange(N, device=a.device, dtype=torch.int64)
    pairs = torch.cat([torch.stack([ii, ii], 1), torch.stack([ii.repeat_interleave(k), d.reshape(-1)], 1)])
    vals = torch.empty(pairs.shape[0], dtype=torch.float32, device=a.device)
    _ssim_pairs(a, b, pairs.to(torch.int32).contiguous(), vals)
    ssim_ok = (vals[:N, None] > vals[N:].view(N, k)).all(1)
    return torch.stack([pcc_ok, ssim_ok], 1)


def n_way_expected(pred: torch.Tensor, truth: torch.Tensor, top: int) -> torch.Tensor:
    """Exact expectation of the ``top``-way score over the reference's draws (top - 1 distractors drawn uniformly WITH
    replacement from the N - 1 other images): float64 [2] (PCC, SSIM) = mean_i q_i^(top - 1), q_i = #{j != i :
    S[i, j] < S[i, i]} / (N - 1), exactly rounded."""
    a, b = _pair_of_batches(pred, truth)
    N = a.shape[0]
    if b.shape[0] != N or N < 2:
        raise ValueError(f"n_way_expected needs N >= 2 reconstructions against as many ground truths, got {N} / "
                         f"{b.shape[0]}")
    if int(top) < 1:
        raise ValueError(f"top must be >= 1, got {top}")
    # S[i, i] < S[i, i] is False: j = i never counts.  The integer counts come back once; the mean is then formed in
    # exact rational arithmetic and rounded once, so the result does not depend on a reduction order.
    counts = torch.stack([(S < S.diagonal()[:, None]).sum(1) for S in (pcc_matrix(a, b), ssim_matrix(a, b))]).tolist()
    k = int(top) - 1
    res = [float(sum(Fraction(c, N - 1) ** k for c in col) / N) for col in counts]
    return torch.tensor(res, dtype=torch.float64, device=a.device)


def nway_scores16(pred16: torch.Tensor, truth16: torch.Tensor, top: int, rng=None, sid: int = SID_DISTRACT, acc=None,
                  acc_mode: int = 0, C: int = 3):
    """One fmri_nway_scores on a batch in the engine's image layout (fp16 [n, H, W, 8], channels 0..C-1 real); enqueues
    only.  ``rng``: a DeviceRng -- the n (top - 1) distractors are drawn at its current offset on stream ``sid`` (the
    offset is not moved); None: no draws, the sampled scores are NaN.  ``acc``: a device float64 [6] to clear and fill
    (``acc_mode`` 0) or add to (1); None: a fresh one.

    Returns ``(S_pcc, S_ssim, distractors, out8, acc6)``: fp32 [n, n] twice, int32 [n, top - 1] (None without ``rng``),
    fp32 [8] = this batch's hits / n (PCC, SSIM) and expectation / n (PCC, SSIM), then the same four over all images
    accumulated so far, and float64 [6] = hits (PCC, SSIM), expectation (PCC, SSIM), images, batches."""
    require_gpu(pred16)
    if (pred16.dim() != 4 or pred16.shape != truth16.shape or pred16.dtype != torch.float16
            or truth16.dtype != torch.float16 or truth16.device != pred16.device
            or not (pred16.is_contiguous() and truth16.is_contiguous())):
        raise ValueError("nway_scores16: pred16 and truth16 must be contiguous fp16 [n, H, W, Cp] of one shape on one "
                         "device")
    n, H, W, cp = pred16.shape
    dev = pred16.device
    nb = lib.load().fmri_nway_ws_bytes(n, H, W)
    ws = _workspace(nb, "nway_scores16", dev)
    S_pcc = torch.empty(n, n, dtype=torch.float32, device=dev)
    S_ssim = torch.empty(n, n, dtype=torch.float32, device=dev)
    d = torch.empty(n, max(int(top) - 1, 0), dtype=torch.int32, device=dev) if rng is not None else None
    out8 = torch.empty(8, dtype=torch.float32, device=dev)
    if acc is None:
        acc = torch.zeros(6, dtype=torch.float64, device=dev)
    lib.call("fmri_nway_scores", _P(pred16), _P(truth16), n, H, W, C, cp, int(top),
             None if rng is None else _P(rng._state), int(sid), _P(ws), nb, _P(S_pcc), _P(S_ssim), _P(d), _P(out8),
             _P(acc), int(acc_mode))
    return S_pcc, S_ssim, d, out8, acc


def objective_assessment(model, dataloader, dataset=None, mode=None, top=5):
    """The reference's n-way identification score (train/train_utils.py:752-816): a CPU float tensor
    [pcc_score, ssim_score], the fraction of images whose ground truth beats all ``top - 1`` random distractors.

    The distractors are drawn with ``random.choice`` in the reference's order (image-major, then the top - 1 draws) before
    the batch's GPU work, so the same ``random`` state gives the same draws and the same score.  Each batch's targets go
    to the device once, one ``n_way`` scores the batch, and only the two counts come back, once, at the end."""
    tp = None
    dataset_size = 0
    for batch_idx, data_batch in enumerate(dataloader):
        model.eval()
        with torch.no_grad():
            target = data_batch['image'] if dataset == 'bold' else data_batch
            n = len(target)
            draws = []
            for idx in range(n):
                numbers = list(range(0, n))
                numbers.remove(idx)
                for i in range(top - 1):
                    draws.append(random.choice(numbers))
            try:
                out = model(data_batch)
            except TypeError:
                if mode == 'wae-gan':
                    out = model(data_batch['fmri'])
                else:
                    logging.info('Wrong data type')
                    raise
            out = out.detach()
            if len(out) != n:
                raise ValueError(f"the model returned {len(out)} images for a batch of {n} targets")
            require_gpu(out)
            target = target.to(out.device)
            if top < 1:     # the reference's count of top - 1 wins is never reached
                hits = torch.zeros(2, dtype=torch.int64, device=out.device)
            else:
                hits = n_way(out, target, torch.tensor(draws, dtype=torch.int64).view(n, top - 1)).sum(0)
            tp = hits if tp is None else tp + hits
            dataset_size += n
    counts = tp.cpu() if tp is not None else torch.zeros(2, dtype=torch.int64)
    return counts.float() / dataset_size
