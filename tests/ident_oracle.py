"""TEST INFRASTRUCTURE ONLY -- torch-CPU restatement of n-way identification (the reference's objective_assessment,
train/train_utils.py:752-816) on top of oracle.metrics_oracle, and the seeded image batches of tests/golden/ident.npz.

  * ``pcc_matrix`` / ``ssim_matrix`` / ``ssim_pairs``: the reference's PearsonCorrelation / StructuralSimilarity of single
    image pairs.  The SSIM filters each image's x and x^2 once and the cross term x_i y_j per pair (the same convolutions
    as metrics_oracle.structural_similarity, batched).
  * ``n_way`` / ``n_way_expected`` / ``objective_assessment``: the counting of the reference on those matrices.
  * ``synth_batch``: fixed "model outputs" and targets from a numpy seed (the fixture stores the seeds, not the images);
    ``StoredModel`` replays them as a model.
"""
import random
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

from oracle import metrics_oracle as MO


def synth_batch(n, c, h, w, seed, dup=None):
    """Targets sharing a common component, and reconstructions that mix their own target with another one in a random
    proportion, plus noise: identification fails for some images, and no two similarities come close to a tie.
    ``dup = (a, b)`` makes target b a bitwise copy of target a."""
    rs = np.random.RandomState(seed)
    common = rs.uniform(-1, 1, (1, c, h, w))
    truth = 0.5 * common + 0.5 * rs.uniform(-1, 1, (n, c, h, w))
    if dup is not None:
        truth[dup[1]] = truth[dup[0]]
    other = (np.arange(n) + 1 + rs.randint(0, n - 1, n)) % n
    alpha = rs.uniform(0.15, 0.85, (n, 1, 1, 1))
    pred = alpha * truth + (1 - alpha) * truth[other] + 0.4 * rs.uniform(-1, 1, (n, c, h, w))
    return torch.from_numpy(pred.astype(np.float32)), torch.from_numpy(truth.astype(np.float32))


class StoredModel:
    """A "model" for objective_assessment: model(batch) returns the stored output of that batch (found by identity)."""

    def __init__(self, batches, outputs):
        self.batches, self.outputs = batches, outputs

    def eval(self):
        return self

    def __call__(self, batch):
        for b, o in zip(self.batches, self.outputs):
            if b is batch:
                return o
        raise KeyError("unknown batch")


def pcc_matrix(pred, truth):
    S = torch.empty(pred.shape[0], truth.shape[0], dtype=torch.float32)
    for i in range(pred.shape[0]):
        for j in range(truth.shape[0]):
            S[i, j] = MO.pearson_correlation(pred[i], truth[j])
    return S


def _filtered(x, window):
    return F.conv2d(x, window, padding=5, groups=x.shape[1])


def ssim_pairs(pred, truth, pairs, chunk=256):
    """Mean SSIM of pred[i] against truth[j] for every row (i, j) of ``pairs`` (reference :343-420, 11x11 window)."""
    C = pred.shape[1]
    window = MO.gaussian_window(11, C)
    mp, mt = _filtered(pred, window), _filtered(truth, window)
    ep, et = _filtered(pred * pred, window), _filtered(truth * truth, window)
    pairs = torch.as_tensor(pairs, dtype=torch.int64).reshape(-1, 2)
    out = torch.empty(pairs.shape[0], dtype=torch.float32)
    for s in range(0, pairs.shape[0], chunk):
        i, j = pairs[s:s + chunk, 0], pairs[s:s + chunk, 1]
        mu1, mu2 = mp[i], mt[j]
        mu1_sq, mu2_sq, mu12 = mu1 ** 2, mu2 ** 2, mu1 * mu2
        s1, s2 = ep[i] - mu1_sq, et[j] - mu2_sq
        s12 = _filtered(pred[i] * truth[j], window) - mu12
        C1, C2 = 0.01 ** 2, 0.03 ** 2
        ssim = ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
        out[s:s + chunk] = ssim.mean((1, 2, 3))
    return out


def ssim_matrix(pred, truth):
    N, M = pred.shape[0], truth.shape[0]
    ii, jj = torch.meshgrid(torch.arange(N), torch.arange(M), indexing="ij")
    return ssim_pairs(pred, truth, torch.stack([ii.reshape(-1), jj.reshape(-1)], 1)).view(N, M)


def n_way_from(S_pcc, S_ssim, distractors):
    d = torch.as_tensor(distractors, dtype=torch.int64)
    out = []
    for S in (S_pcc, S_ssim):
        gt = S.diagonal()
        out.append((gt[:, None] > S.gather(1, d)).all(1) if d.shape[1] else torch.ones(S.shape[0], dtype=torch.bool))
    return torch.stack(out, 1)


def n_way(pred, truth, distractors):
    return n_way_from(pcc_matrix(pred, truth), ssim_matrix(pred, truth), distractors)


def n_way_expected_from(S_pcc, S_ssim, top):
    N = S_pcc.shape[0]
    res = []
    for S in (S_pcc, S_ssim):
        counts = (S < S.diagonal()[:, None]).sum(1).tolist()
        res.append(float(sum(Fraction(c, N - 1) ** (top - 1) for c in counts) / N))
    return torch.tensor(res, dtype=torch.float64)


def n_way_expected(pred, truth, top):
    return n_way_expected_from(pcc_matrix(pred, truth), ssim_matrix(pred, truth), top)


def draw_distractors(n, top):
    """The reference's draws: image-major, ``random.choice`` over the other indices, top - 1 per image."""
    draws = []
    for idx in range(n):
        numbers = list(range(0, n))
        numbers.remove(idx)
        for _ in range(top - 1):
            draws.append(random.choice(numbers))
    return torch.tensor(draws, dtype=torch.int64).view(n, top - 1)


def objective_assessment(outputs, targets, top):
    """Score [pcc, ssim] (float32) of per-batch ``outputs`` against ``targets`` with the reference's draws from the
    current ``random`` state; also returns the per-batch distractors."""
    tp = torch.zeros(2, dtype=torch.int64)
    size, draws = 0, []
    for out, tgt in zip(outputs, targets):
        d = draw_distractors(len(tgt), top)
        draws.append(d)
        tp += n_way(out.float(), tgt.float(), d).sum(0)
        size += len(tgt)
    return tp.float() / size, draws
