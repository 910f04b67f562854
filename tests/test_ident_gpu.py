"""n-way identification on the MI355X (fmri_hip.ident over csrc/ident.hip): the pairwise PCC / SSIM matrices against the
reference's values (tests/golden/ident.npz) and the CPU oracle, their determinism (bitwise: repeated calls, permuted
pair lists, sliced batches, a duplicated target), the engine's objective_assessment against the reference's scores, a
real eval-mode engine model against the oracle on the same outputs and draws, and the error cases."""
import os
import random

import numpy as np
import pytest
import torch

import ident_oracle as IO
from test_ident_host import golden_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_matrices_match_reference_and_oracle(golden_dir):
    from fmri_hip import ident
    from train.train_utils import PearsonCorrelation, StructuralSimilarity
    pcc1, ssim1 = PearsonCorrelation(), StructuralSimilarity()
    g, cases = golden_cases(golden_dir)
    for name, _, batches in cases:
        for b, (pred, truth) in enumerate(batches):
            pd, td = pred.to(DEV), truth.to(DEV)
            P, S = ident.pcc_matrix(pd, td), ident.ssim_matrix(pd, td)
            assert P.shape == S.shape == (len(pred), len(truth)) and P.dtype == S.dtype == torch.float32
            # fp32 sums in another order than the reference's (fp64 row statistics, MFMA chains, separable window)
            np.testing.assert_allclose(P.double().cpu().numpy(), g[f"{name}/b{b}/pcc"], rtol=1e-5, atol=0)
            np.testing.assert_allclose(S.double().cpu().numpy(), g[f"{name}/b{b}/ssim"], rtol=1e-5, atol=0)
            np.testing.assert_allclose(P.cpu().numpy(), IO.pcc_matrix(pred, truth).numpy(), rtol=1e-5, atol=0)
            np.testing.assert_allclose(S.cpu().numpy(), IO.ssim_matrix(pred, truth).numpy(), rtol=1e-5, atol=0)
            # the diagonal against the engine's single-pair metrics of train_utils
            for i in range(len(pred)):
                assert P[i, i].item() == pytest.approx(pcc1(pd[i], td[i]).item(), rel=1e-5)
                assert S[i, i].item() == pytest.approx(ssim1(pd[i:i + 1], td[i:i + 1]).item(), rel=1e-5)
            # the exact expectation: every comparison of the full matrices has a margin > 1e-3, so it is exact
            for top in (2, 5, 10):
                want = IO.n_way_expected_from(torch.from_numpy(g[f"{name}/b{b}/pcc"]),
                                              torch.from_numpy(g[f"{name}/b{b}/ssim"]), top)
                got = ident.n_way_expected(pd, td, top)
                assert got.dtype == torch.float64 and got.shape == (2,)
                assert torch.equal(got.cpu(), want), (name, b, top, got, want)


def test_pair_values_are_bitwise_functions_of_the_two_images(golden_dir):
    from fmri_hip import ident
    _, cases = golden_cases(golden_dir)
    for name, _, batches in cases:
        pred, truth = [t.to(DEV) for t in batches[0]]
        N = len(pred)
        P, S = ident.pcc_matrix(pred, truth), ident.ssim_matrix(pred, truth)
        # two calls
        assert torch.equal(_bits(P), _bits(ident.pcc_matrix(pred, truth)))
        assert torch.equal(_bits(S), _bits(ident.ssim_matrix(pred, truth)))
        # a permuted pair list permutes the output bits
        ii, jj = torch.meshgrid(torch.arange(N), torch.arange(N), indexing="ij")
        pairs = torch.stack([ii.reshape(-1), jj.reshape(-1)], 1)
        perm = torch.randperm(len(pairs), generator=torch.Generator().manual_seed(5))
        v = ident.ssim_pairs(pred, truth, pairs)
        assert torch.equal(_bits(v), _bits(S.reshape(-1)))
        assert torch.equal(_bits(ident.ssim_pairs(pred, truth, pairs[perm].to(DEV))), _bits(v)[perm])
        # other N, M and P: a slice of the batch, a short pair list
        assert torch.equal(_bits(ident.pcc_matrix(pred[3:5], truth[1:])), _bits(P[3:5, 1:]))
        assert torch.equal(_bits(ident.ssim_pairs(pred[3:], truth[:4], torch.tensor([[0, 3], [2, 1]]))),
                           _bits(torch.stack([S[3, 3], S[5, 1]])))
        # the duplicated target: S[i, j] == S[i, i] bitwise, so the strict > counts it as a miss, as on the host
        dup = [(a, c) for a in range(N) for c in range(N) if a != c and torch.equal(truth[a], truth[c])]
        assert dup, name
        for a, c in dup:
            assert torch.equal(_bits(P[:, a]), _bits(P[:, c])) and torch.equal(_bits(S[:, a]), _bits(S[:, c]))
            d = torch.full((N, 1), (a + 1) % N, dtype=torch.int64)
            d[a, 0] = c
            assert not ident.n_way(pred, truth, d)[a].any()


def test_objective_assessment_reproduces_the_reference_scores(golden_dir):
    from fmri_hip.ident import objective_assessment
    g, cases = golden_cases(golden_dir)
    for name, dataset, batches in cases:
        outs = [p.to(DEV) for p, _ in batches]
        # the dataloader yields host batches, as a DataLoader does; the model's outputs are on the device
        loader = [{"image": t, "fmri": torch.zeros(len(t), 8)} if dataset == "bold" else t for _, t in batches]
        model = IO.StoredModel(loader, outs)
        for top in [int(t) for t in g["meta/tops"]]:
            random.seed(int(g[f"{name}/top{top}/seed"]))
            got = objective_assessment(model, loader, dataset=dataset, top=top)
            assert got.device.type == "cpu" and got.dtype == torch.float32
            assert np.array_equal(got.numpy(), g[f"{name}/top{top}/score"]), (name, top, got)
            # the next draws continue from the same random state as after the reference's call
            random.seed(int(g[f"{name}/top{top}/seed"]))
            _, draws = IO.objective_assessment([p for p, _ in batches], [t for _, t in batches], top)
            after_oracle = random.random()
            random.seed(int(g[f"{name}/top{top}/seed"]))
            objective_assessment(model, loader, dataset=dataset, top=top)
            assert random.random() == after_oracle


def test_objective_assessment_wae_gan_fallback(golden_dir):
    """mode='wae-gan': a model that rejects the batch dict with a TypeError is called with data_batch['fmri']."""
    from fmri_hip.ident import objective_assessment
    g, cases = golden_cases(golden_dir)
    name, dataset, batches = [c for c in cases if c[1] == "bold"][0]
    fmri = [torch.full((len(t), 8), float(k)) for k, (_, t) in enumerate(batches)]
    loader = [{"image": t, "fmri": f} for (_, t), f in zip(batches, fmri)]

    class WaeLike:
        def eval(self):
            return self

        def __call__(self, x):
            if isinstance(x, dict):
                raise TypeError("expects the fMRI tensor")
            return batches[int(x[0, 0])][0].to(DEV)
    top = int(g["meta/tops"][0])
    random.seed(int(g[f"{name}/top{top}/seed"]))
    got = objective_assessment(WaeLike(), loader, dataset=dataset, mode="wae-gan", top=top)
    assert np.array_equal(got.numpy(), g[f"{name}/top{top}/score"])
    with pytest.raises(TypeError):
        objective_assessment(WaeLike(), loader, dataset=dataset, mode="vae-gan", top=top)


def test_objective_assessment_of_an_engine_model_matches_the_oracle():
    """Eval-mode VaeGan (64 px, seeded weights with running statistics) on the engine: the engine's score against the
    oracle's on the same outputs and the same draws.  Counts may differ only where a comparison's margin is < 1e-5."""
    import configs.models_config as mc
    mc.use_px64()
    import models.vae_gan as vg
    from fmri_hip.ident import objective_assessment
    from oracle import vaegan_oracle as O
    from test_oracle_golden import eval_state
    cfg = O.ArchCfg.px64()
    model = vg.VaeGan(device=DEV, z_size=128).to(DEV)
    model.load_state_dict(eval_state(cfg, 11))
    loader = [IO.synth_batch(n, 3, 64, 64, 70 + n)[1].to(DEV) for n in (8, 4)]
    recorded = []

    def recording(x):
        y = model(x)
        recorded.append(y.detach().float().cpu())
        return y
    recording.eval = model.eval
    torch.manual_seed(0)
    for top in (2, 5, 10):
        recorded.clear()
        random.seed(top)
        got = objective_assessment(recording, loader, top=top)
        random.seed(top)
        tgts = [t.cpu() for t in loader]
        want, draws = IO.objective_assessment(recorded, tgts, top)
        slack = torch.zeros(2)
        for out, tgt, d in zip(recorded, tgts, draws):
            for col, S in enumerate((IO.pcc_matrix(out, tgt), IO.ssim_matrix(out, tgt))):
                near = (S.diagonal()[:, None] - S.gather(1, d)).abs() < 1e-5
                slack[col] += near.any(1).sum()
        n = sum(len(t) for t in tgts)
        assert ((got - want).abs() * n <= slack + 0.5).all(), (top, got, want, slack)


def test_ident_error_cases():
    from fmri_hip import ident
    pred, truth = IO.synth_batch(4, 3, 16, 16, 9)
    with pytest.raises(RuntimeError):
        ident.pcc_matrix(pred, truth.to(DEV))
    with pytest.raises(RuntimeError):
        ident.ssim_matrix(pred.to(DEV), truth)
    small = torch.rand(4, 3, 10, 16, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported"):
        ident.ssim_matrix(small, small)
    with pytest.raises(RuntimeError, match="unsupported"):
        ident.n_way(small, small, torch.zeros(4, 1, dtype=torch.int64))
    # the ABI itself refuses the geometry (FMRI_E_UNSUPPORTED)
    from fmri_hip import lib
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    pairs = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    out = torch.empty(1, device=DEV)
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        lib.call("fmri_ssim_pairs", small.data_ptr(), small.data_ptr(), 4, 4, 3, 10, 16, pairs.data_ptr(), 1,
                 out.data_ptr(), ws.data_ptr(), ws.numel())
    with pytest.raises(ValueError):
        ident.pcc_matrix(pred.to(DEV), truth[:, :, :8].to(DEV))
    with pytest.raises(ValueError):
        ident.ssim_pairs(pred.to(DEV), truth.to(DEV), torch.tensor([[0, 4]]))
