"""CPU checks of what the evaluation-pass tests stand on: the float64 restatement of fmri_image_metrics over the engine's
image layout (tests/eval_oracle.py) against ident_oracle on NCHW copies and against the reference's own values
(tests/golden/metrics.npz), and the evaluator's batch split."""
import os

import numpy as np
import pytest
import torch

import eval_oracle as EO
import ident_oracle as IO


@pytest.mark.parametrize("shape,C", [((2, 3, 17, 16), 3), ((2, 1, 11, 40), 1), ((3, 3, 33, 31), 3)])
@pytest.mark.parametrize("affine", [False, True])
def test_layout_restatement_matches_ident_oracle(shape, C, affine):
    """The restatement over fp16 [N][H][W][8] equals pcc64 / ssim64 / the float64 MSE of NCHW copies of the same fp16
    values (affine in torch fp32, one rounding per operation) to 1e-12, whatever the pad lanes hold."""
    n, c, h, w = shape
    p, t = IO.edge_batch(n, n, c, h, w, 5 + sum(shape))
    scale, shift = EO.DENORM if affine else (None, None)
    got = EO.image_metrics64(EO.to_layout(p, float("nan")), EO.to_layout(t, 7.0), C, scale, shift)
    a, b = p.half().float(), t.half().float()
    if affine:
        sc = torch.tensor(scale[:C]).view(1, C, 1, 1)
        sf = torch.tensor(shift[:C]).view(1, C, 1, 1)
        a, b = a * sc + sf, b * sc + sf
    want = (IO.pcc64(a, b).item(), IO.ssim64(a, b)[0].item(), ((a.double() - b.double()) ** 2).mean().item())
    for g, r in zip(got, want):
        assert abs(g - r) <= 1e-12, (got, want)


def test_restatement_formulas_match_reference_golden(golden_dir):
    """``metrics64`` (the formulas behind the layout) on the inputs of tests/golden/metrics.npz against what the reference's
    PearsonCorrelation / StructuralSimilarity returned, at the tolerance of tests/test_metrics.py:30-32; the MSE against
    torch's MSELoss in fp64."""
    from test_metrics import _inputs
    g = np.load(os.path.join(golden_dir, "metrics.npz"))
    for tag in [str(t) for t in g["meta/cases"]]:
        a, b = _inputs(g[f"{tag}/shape"])
        pcc, ssim, mse = EO.metrics64(a, b)
        assert pcc == pytest.approx(float(g[f"{tag}/pcc"]), rel=1e-6)
        assert ssim == pytest.approx(float(g[f"{tag}/ssim"]), rel=1e-6)
        assert mse == pytest.approx(torch.nn.functional.mse_loss(a.double(), b.double()).item(), rel=1e-12)


def test_evaluator_batch_split():
    """Rows in order, no drop-last: N = 10, B = 4 gives 4, 4, 2; N < B gives one short batch."""
    from fmri_hip.evaluate import batch_ranges
    assert batch_ranges(10, 4) == [(0, 4), (4, 4), (8, 2)]
    assert batch_ranges(8, 4) == [(0, 4), (4, 4)]
    assert batch_ranges(3, 4) == [(0, 3)]
    assert batch_ranges(1, 1) == [(0, 1)]
    with pytest.raises(ValueError):
        batch_ranges(0, 4)
