"""Validation metrics: the oracle restatement against goldens produced by the reference's own
PearsonCorrelation / StructuralSimilarity modules (CPU), and the HIP kernels against the oracle and the goldens (GPU)."""
import os

import numpy as np
import pytest
import torch

from oracle import metrics_oracle as MO


def _inputs(shape):
    n, c, h, w, seed = [int(v) for v in shape]
    rs = np.random.RandomState(seed)
    a = torch.from_numpy(rs.uniform(-1, 1, (n, c, h, w)).astype(np.float32))
    b = 0.6 * a + 0.4 * torch.from_numpy(rs.uniform(-1, 1, (n, c, h, w)).astype(np.float32))
    return a, b


def _cases(golden_dir):
    g = np.load(os.path.join(golden_dir, "metrics.npz"))
    return g, [str(t) for t in g["meta/cases"]]


def test_metrics_oracle_matches_reference(golden_dir):
    g, tags = _cases(golden_dir)
    for tag in tags:
        a, b = _inputs(g[f"{tag}/shape"])
        s, c = MO.structural_similarity(a, b)
        assert MO.pearson_correlation(a, b).item() == pytest.approx(float(g[f"{tag}/pcc"]), rel=1e-6)
        assert s.item() == pytest.approx(float(g[f"{tag}/ssim"]), rel=1e-6)
        assert c.item() == pytest.approx(float(g[f"{tag}/contrast"]), rel=1e-6)
        assert float(g[f"{tag}/ssim_default"]) == pytest.approx(float(g[f"{tag}/ssim"]), rel=1e-7)


@pytest.mark.gpu
def test_metrics_hip_matches_oracle_and_reference(golden_dir):
    from train.train_utils import PearsonCorrelation, StructuralSimilarity
    pcc, ssim = PearsonCorrelation(), StructuralSimilarity()
    g, tags = _cases(golden_dir)
    for tag in tags:
        a, b = _inputs(g[f"{tag}/shape"])
        ad, bd = a.cuda(), b.cuda()
        s, c = ssim(ad, bd, full=True)
        so, co = MO.structural_similarity(a, b)
        # fp32 sums in a different order (separable window, fp64 global accumulation): 1e-5 relative
        assert pcc(ad, bd).item() == pytest.approx(float(g[f"{tag}/pcc"]), rel=1e-5)
        assert s.item() == pytest.approx(float(g[f"{tag}/ssim"]), rel=1e-5)
        assert c.item() == pytest.approx(float(g[f"{tag}/contrast"]), rel=1e-5)
        assert s.item() == pytest.approx(so.item(), rel=1e-5) and c.item() == pytest.approx(co.item(), rel=1e-5)
        assert ssim(ad, bd).item() == pytest.approx(s.item(), rel=1e-7)
    # identical images: SSIM = 1, PCC = 1; a 3-D input is one image
    x = torch.rand(3, 64, 64, device="cuda")
    assert ssim(x, x).item() == pytest.approx(1.0, abs=1e-6)
    assert pcc(x, x).item() == pytest.approx(1.0, abs=1e-6)
    with pytest.raises(RuntimeError):
        pcc(x.cpu(), x.cpu())


def _edge_pair(shape, seed):
    """Correlated images in [-1, 1] with per-image offsets, tanh-saturated and flat +-1 regions (ident_oracle.edge_batch);
    a 3-element shape is one [C, H, W] image."""
    import ident_oracle as IO
    n, (c, h, w) = (shape[0], shape[1:]) if len(shape) == 4 else (1, shape)
    a, b = IO.edge_batch(max(n, 2), max(n, 2), c, h, w, seed)
    return (a[:n], b[:n]) if len(shape) == 4 else (a[0], b[0])


def _against_fp64(shape, seed):
    """PearsonCorrelation and StructuralSimilarity(full=True) on the device against the float64 restatement, 2e-6
    absolute; returns the errors (pcc, ssim, contrast)."""
    import ident_oracle as IO
    from train.train_utils import PearsonCorrelation, StructuralSimilarity
    a, b = _edge_pair(shape, seed)
    ad, bd = a.cuda(), b.cuda()
    s, c = StructuralSimilarity()(ad, bd, full=True)
    s64, c64 = IO.ssim64(a, b)
    err = (abs(PearsonCorrelation()(ad, bd).item() - IO.pcc64(a, b).item()), abs(s.item() - s64.item()),
           abs(c.item() - c64.item()))
    print(f"metrics {tuple(shape)}: max |err| vs fp64 pcc {err[0]:.3g} ssim {err[1]:.3g} contrast {err[2]:.3g}")
    assert max(err) <= 2e-6, (shape, err)
    return err


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1, 11, 11), (2, 3, 11, 40), (2, 1, 17, 16), (64, 3, 100, 100), (3, 13, 29)])
def test_metrics_hip_against_fp64(shape):
    """Single-pair metrics (fmri_pcc, fmri_ssim) at the smallest SSIM geometry, H = 11 < W, one pixel past a 16-tile
    with C = 1, the reference's inference batch (469 blocks of atomics in pcc_sums_kernel) and a 3-D input."""
    _against_fp64(shape, 11 + sum(shape))


@pytest.mark.gpu
def test_metrics_hip_against_fp64_deterministic(deterministic):
    """The 64 x 3 x 100 x 100 batch in deterministic mode (one block of fixed-order sums): also within 2e-6, and two
    calls are bit-identical."""
    from train.train_utils import PearsonCorrelation, StructuralSimilarity
    _against_fp64((64, 3, 100, 100), 11 + 267)
    a, b = [t.cuda() for t in _edge_pair((64, 3, 100, 100), 11 + 267)]
    pcc, ssim = PearsonCorrelation(), StructuralSimilarity()
    assert torch.equal(pcc(a, b), pcc(a, b)) and torch.equal(ssim(a, b), ssim(a, b))
