"""TEST INFRASTRUCTURE ONLY -- torch-CPU restatement of n-way identification (the reference's objective_assessment,
train/train_utils.py:752-816) on top of oracle.metrics_oracle, and the seeded image batches of tests/golden/ident.npz.

  * ``pcc_matrix`` / ``ssim_matrix`` / ``ssim_pairs``: the reference's PearsonCorrelation / StructuralSimilarity of single
    image pairs.  The SSIM filters each image's x and x^2 once and the cross term x_i y_j per pair (the same convolutions
    as metrics_oracle.structural_similarity, batched).
  * ``n_way`` / ``n_way_expected`` / ``objective_assessment``: the counting of the reference on those matrices.
  * ``synth_batch``: fixed "model outputs" and targets from a numpy seed (the fixture stores the seeds, not the images);
    ``StoredModel`` replays them as a model.  ``edge_batch``: the same, offset per image, with saturated and flat regions.
  * ``pcc_matrix64`` / ``ssim_pairs64`` / ``ssim_matrix64`` / ``pcc64`` / ``ssim64``: the same formulas in float64 (window
    built in float64, every intermediate in float64), the anchor the HIP kernels are measured against; pinned to the
    reference's values by tests/test_ident_host.py.
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


def edge_batch(n, m, c, h, w, seed):
    """pred [n] and truth [m] (fp32, CPU) from synth_batch, each image scaled into [-1, 1] around its own offset of
    0.2..0.5 in magnitude and random sign s.  pred 1, 5, 9, ... are tanh(20 x) (saturated to exactly +-1 where
    |x| > 0.45); flat regions at exactly s (a white or black background): the top third of truth 2, 6, ..., the right
    third of truth 3, 7, ..., the bottom third of pred 2, 6, ... and the top half of pred 3, 7, ...  Across pairs, flat
    regions of equal and of opposite value overlap."""
    k = max(n, m)
    pred, truth = synth_batch(k, c, h, w, seed)
    rs = np.random.RandomState(seed + 1)

    def place(x):
        o = (rs.uniform(0.2, 0.5, k) * rs.choice([-1, 1], k))[:, None, None, None]
        amp = np.abs(x).reshape(k, -1).max(1)[:, None, None, None]
        return (1 - np.abs(o)) * x / amp + o, np.sign(o)
    (p, sp), (t, st) = place(pred.double().numpy()), place(truth.double().numpy())
    p[1::4] = np.tanh(20 * p[1::4])
    t[2::4, :, :h // 3] = st[2::4]
    t[3::4, :, :, w - w // 3:] = st[3::4]
    p[2::4, :, h - h // 3:] = sp[2::4]
    p[3::4, :, :h // 2] = sp[3::4]
    return torch.from_numpy(p[:n].astype(np.float32)), torch.from_numpy(t[:m].astype(np.float32))


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


def pcc_matrix64(pred, truth):
    """float64 [N, M]: every row centred in float64, one float64 matmul.  A zero-variance row gives 0 / 0 = NaN."""
    a = pred.reshape(pred.shape[0], -1).double()
    b = truth.reshape(truth.shape[0], -1).double()
    a = a - a.mean(1, keepdim=True)
    b = b - b.mean(1, keepdim=True)
    return (a @ b.t()) / (a.norm(dim=1)[:, None] * b.norm(dim=1)[None, :])


def gaussian64(size=11, sigma=1.5):
    """The reference's 1-D Gaussian (train/train_utils.py:313-326) in float64, normalised to sum 1."""
    x = torch.arange(size, dtype=torch.float64) - size // 2
    g = torch.exp(-x * x / (2 * sigma * sigma))
    return g / g.sum()


def _filter64(t):
    """float64 [N, C, H, W] filtered by the 11 x 11 window outer(g, g) with zero padding 5, applied as its two 1-D
    passes (the same sum; one fifth of the work of the 2-D convolution)."""
    C = t.shape[1]
    g = gaussian64()
    t = F.conv2d(t, g.view(1, 1, 1, 11).expand(C, 1, 1, 11), padding=(0, 5), groups=C)
    return F.conv2d(t, g.view(1, 1, 11, 1).expand(C, 1, 11, 1), padding=(5, 0), groups=C)


def _ssim_map64(m1, m2, e11, e22, e12):
    s1, s2, s12 = e11 - m1 * m1, e22 - m2 * m2, e12 - m1 * m2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim = ((2 * m1 * m2 + C1) * (2 * s12 + C2)) / ((m1 * m1 + m2 * m2 + C1) * (s1 + s2 + C2))
    return ssim, (2 * s12 + C2) / (s1 + s2 + C2)


def ssim_pairs64(pred, truth, pairs, chunk=1024):
    """float64 [P]: mean SSIM of pred[i] against truth[j] for every row (i, j) of ``pairs`` (the formula of
    ``ssim_pairs``), in chunks of ``chunk`` pairs."""
    a, b = pred.double(), truth.double()
    mp, mt, ep, et = _filter64(a), _filter64(b), _filter64(a * a), _filter64(b * b)
    pairs = torch.as_tensor(pairs, dtype=torch.int64).reshape(-1, 2)
    out = torch.empty(pairs.shape[0], dtype=torch.float64)
    for s in range(0, pairs.shape[0], chunk):
        i, j = pairs[s:s + chunk, 0], pairs[s:s + chunk, 1]
        ssim, _ = _ssim_map64(mp[i], mt[j], ep[i], et[j], _filter64(a[i] * b[j]))
        out[s:s + chunk] = ssim.mean((1, 2, 3))
    return out


def ssim_matrix64(pred, truth):
    N, M = pred.shape[0], truth.shape[0]
    ii, jj = torch.meshgrid(torch.arange(N), torch.arange(M), indexing="ij")
    return ssim_pairs64(pred, truth, torch.stack([ii.reshape(-1), jj.reshape(-1)], 1)).view(N, M)


def pcc64(y_pred, y_true):
    """float64 PearsonCorrelation of two whole tensors (one value over the batch, as the metric module)."""
    a, b = y_pred.double().reshape(-1), y_true.double().reshape(-1)
    a, b = a - a.mean(), b - b.mean()
    return (a @ b) / (a.norm() * b.norm())


def ssim64(img1, img2):
    """float64 (mean SSIM, mean contrast term) over a whole [N, C, H, W] or [C, H, W] batch: StructuralSimilarity's
    ``full=True`` pair."""
    a, b = img1.double(), img2.double()
    if a.dim() == 3:
        a, b = a[None], b[None]
    ssim, contrast = _ssim_map64(_filter64(a), _filter64(b), _filter64(a * a), _filter64(b * b), _filter64(a * b))
    return ssim.mean(), contrast.mean()


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
