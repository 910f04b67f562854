"""Host-side checks of n-way identification (no GPU): the torch-CPU restatement in tests/ident_oracle.py against the
reference's own objective_assessment (tests/golden/ident.npz), the exact expectation against brute-force enumeration of
the draws, the C ABI declarations of fmri_pcc_matrix / fmri_ssim_pairs and their argument checks, and the Python
surface of fmri_hip.ident (GPU tensors only)."""
import ctypes
import itertools
import os
import random
import re

import numpy as np
import pytest
import torch

import ident_oracle as IO

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def lib():
    from fmri_hip import build, lib as L
    build.build(verbose=False)
    return L.load()


def golden_cases(golden_dir):
    g = np.load(os.path.join(golden_dir, "ident.npz"))
    cases = []
    for name in [str(c) for c in g["meta/cases"]]:
        ds = str(g[f"{name}/dataset"])
        batches = []
        for n, c, h, w, seed, da, db in g[f"{name}/batches"].tolist():
            batches.append(IO.synth_batch(n, c, h, w, seed, (da, db) if da >= 0 else None))
        cases.append((name, None if ds == "none" else ds, batches))
    return g, cases


def test_oracle_reproduces_reference_objective_assessment(golden_dir):
    g, cases = golden_cases(golden_dir)
    dup_drawn = False
    for name, _, batches in cases:
        mats = []
        for b, (pred, truth) in enumerate(batches):
            P, S = IO.pcc_matrix(pred, truth), IO.ssim_matrix(pred, truth)
            np.testing.assert_allclose(P.double().numpy(), g[f"{name}/b{b}/pcc"], rtol=1e-6, atol=0)
            np.testing.assert_allclose(S.double().numpy(), g[f"{name}/b{b}/ssim"], rtol=1e-6, atol=0)
            mats.append((P, S))
        for top in [int(t) for t in g["meta/tops"]]:
            assert g[f"{name}/top{top}/margin"].min() > 1e-4
            want = g[f"{name}/top{top}/score"]
            assert all(0.0 < v < 1.0 for v in want)
            random.seed(int(g[f"{name}/top{top}/seed"]))
            got, draws = IO.objective_assessment([p for p, _ in batches], [t for _, t in batches], top)
            assert np.array_equal(got.numpy(), want), (name, top, got, want)
            # the same counts straight from the matrices
            tp = sum(IO.n_way_from(P, S, d).sum(0) for (P, S), d in zip(mats, draws))
            assert np.array_equal((tp.float() / sum(len(t) for _, t in batches)).numpy(), want)
            for (pred, truth), d in zip(batches, draws):
                same = [[torch.equal(truth[i], truth[j]) for j in d[i].tolist()] for i in range(len(truth))]
                dup_drawn |= any(any(r) for r in same)
    assert dup_drawn, "no draw of any case picks the duplicated target: the fixture does not exercise the tie"


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_n_way_expected_equals_enumeration_of_all_draws(seed):
    """Each image's hit probability is its share of the (N - 1)^(top - 1) equally likely distractor tuples (the draws of
    different images are independent); the score's expectation is their mean.  Counted exactly, with fractions."""
    from fractions import Fraction
    N, top = 5, 3
    pred, truth = IO.synth_batch(N, 3, 16, 16, 500 + seed, dup=(1, 3) if seed == 2 else None)
    P, S = IO.pcc_matrix(pred, truth), IO.ssim_matrix(pred, truth)
    brute = []
    for col in range(2):
        acc = Fraction(0)
        for i in range(N):
            tuples = list(itertools.product([j for j in range(N) if j != i], repeat=top - 1))
            assert len(tuples) == (N - 1) ** (top - 1)
            d = torch.full((N, top - 1), (i + 1) % N, dtype=torch.int64)
            hits = 0
            for t in tuples:
                d[i] = torch.tensor(t)
                hits += int(IO.n_way_from(P, S, d)[i, col])
            acc += Fraction(hits, len(tuples))
        brute.append(acc / N)
    got = IO.n_way_expected_from(P, S, top)
    assert [float(b) for b in brute] == got.tolist(), (got, brute)
    assert 0.0 < float(min(brute)) and float(max(brute)) < 1.0
    assert torch.equal(IO.n_way_expected(pred, truth, top), got)


def test_ident_abi_is_declared_and_exported(lib):
    from fmri_hip import lib as L
    hdr = open(os.path.join(ROOT, "include", "fmri_hip.h")).read()
    for name, ret in (("fmri_pcc_matrix", "int"), ("fmri_ssim_pairs", "int"), ("fmri_pcc_matrix_ws_bytes", "int64_t"),
                      ("fmri_ssim_pairs_ws_bytes", "int64_t")):
        assert re.search(rf"\b{ret} {name}\s*\(", hdr), name
        assert hasattr(lib, name) and name in L.EXPORTS, name


def test_ident_abi_argument_checks_without_gpu(lib):
    """Rejected on the host before anything is enqueued: null pointers, empty geometry, short ldS, images below 11 px,
    a workspace below the *_ws_bytes size, a negative pair count."""
    assert lib.fmri_pcc_matrix_ws_bytes(0, 4, 100) < 0 and lib.fmri_pcc_matrix_ws_bytes(4, 4, 0) < 0
    assert lib.fmri_pcc_matrix_ws_bytes(64, 64, 30000) > 64 * 64 * 4 * 29
    assert lib.fmri_ssim_pairs_ws_bytes(4, 0, 3, 64, 64) < 0
    assert lib.fmri_ssim_pairs_ws_bytes(64, 64, 3, 100, 100) >= 2 * 128 * 3 * 100 * 100 * 4
    z = ctypes.c_void_p(256)
    big = 1 << 40

    def pcc(pred=z, truth=z, N=8, M=8, D=300, S=z, ldS=8, ws=z, nb=big):
        return lib.fmri_pcc_matrix(pred, truth, N, M, D, S, ldS, ws, nb, None)
    assert pcc(pred=None) == -1 and pcc(S=None) == -1 and pcc(ws=None) == -1
    assert pcc(N=0) == -1 and pcc(D=0) == -1 and pcc(ldS=7) == -1
    assert pcc(nb=16) == -4

    def ssim(pred=z, truth=z, N=4, M=4, C=3, H=64, W=64, pairs=z, P=16, out=z, ws=z, nb=big):
        return lib.fmri_ssim_pairs(pred, truth, N, M, C, H, W, pairs, P, out, ws, nb, None)
    assert ssim(truth=None) == -1 and ssim(pairs=None) == -1 and ssim(out=None) == -1
    assert ssim(P=-1) == -1 and ssim(C=0) == -1
    assert ssim(H=10) == -2 and ssim(W=8) == -2
    assert ssim(nb=16) == -4


def test_ident_python_surface_has_no_cpu_fallback():
    from fmri_hip import ident
    pred, truth = IO.synth_batch(4, 3, 16, 16, 7)
    for fn, args in ((ident.pcc_matrix, ()), (ident.ssim_matrix, ()), (ident.n_way_expected, (2,)),
                     (ident.ssim_pairs, (torch.zeros(1, 2, dtype=torch.int32),)),
                     (ident.n_way, (torch.zeros(4, 1, dtype=torch.int64),))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(pred, truth, *args)


def test_objective_assessment_keeps_the_reference_signature():
    import inspect
    from fmri_hip.ident import objective_assessment
    sig = inspect.signature(objective_assessment)
    assert list(sig.parameters) == ["model", "dataloader", "dataset", "mode", "top"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, None, 5]


def test_objective_assessment_batch_of_one_raises_the_reference_index_error():
    """The draws come first, on the host: one image leaves nothing to draw from (random.choice of an empty list)."""
    from fmri_hip.ident import objective_assessment

    class Model:
        def eval(self):
            return self

        def __call__(self, x):
            raise AssertionError("the model must not run before the draws")
    with pytest.raises(IndexError):
        objective_assessment(Model(), [torch.zeros(1, 3, 16, 16)], top=2)


def test_fp64_oracle_matches_reference_goldens(golden_dir):
    """The float64 restatement (ident_oracle.pcc_matrix64 / ssim_matrix64 / pcc64 / ssim64) against the reference's own
    fp32 values: tests/golden/ident.npz (every pair of every batch) and tests/golden/metrics.npz (PCC, SSIM and the
    contrast term of whole batches).  The reference's fp32 rounding is below 1e-6 here, so 2e-6 absolute ties the anchor
    of the fp64 sweeps (test_ident_edges_gpu.py, test_metrics.py) to the reference."""
    from test_metrics import _cases, _inputs
    g, cases = golden_cases(golden_dir)
    for name, _, batches in cases:
        for b, (pred, truth) in enumerate(batches):
            np.testing.assert_allclose(IO.pcc_matrix64(pred, truth).numpy(), g[f"{name}/b{b}/pcc"], rtol=0, atol=2e-6)
            np.testing.assert_allclose(IO.ssim_matrix64(pred, truth).numpy(), g[f"{name}/b{b}/ssim"], rtol=0,
                                       atol=2e-6)
    g, tags = _cases(golden_dir)
    for tag in tags:
        a, b = _inputs(g[f"{tag}/shape"])
        s, c = IO.ssim64(a, b)
        assert abs(IO.pcc64(a, b).item() - float(g[f"{tag}/pcc"])) <= 2e-6, tag
        assert abs(s.item() - float(g[f"{tag}/ssim"])) <= 2e-6, tag
        assert abs(c.item() - float(g[f"{tag}/contrast"])) <= 2e-6, tag
        # a 3-D [C, H, W] input is one image
        s0, c0 = IO.ssim64(a[0], b[0])
        s1, c1 = IO.ssim64(a[:1], b[:1])
        assert s0.item() == s1.item() and c0.item() == c1.item()


def test_fp64_oracle_is_the_exact_formula():
    """Exact cases of the float64 restatement: identical images give PCC 1 and SSIM 1; y = 2 x + 1 gives PCC 1; a
    constant image gives PCC NaN; the separable filter equals the 2-D 11 x 11 window; the pair list equals the
    matrix."""
    import torch.nn.functional as F
    pred, truth = IO.synth_batch(5, 2, 13, 17, 3)
    assert torch.allclose(IO.pcc_matrix64(pred, pred).diagonal(), torch.ones(5, dtype=torch.float64), rtol=0, atol=1e-14)
    assert torch.allclose(IO.ssim_matrix64(pred, pred).diagonal(), torch.ones(5, dtype=torch.float64), rtol=0,
                          atol=1e-14)
    assert abs(IO.pcc_matrix64(pred[:1], 2 * pred[:1] + 1).item() - 1) < 1e-14
    assert torch.isnan(IO.pcc_matrix64(torch.full((1, 2, 13, 17), 0.1), truth)).all()
    g = IO.gaussian64()
    w2 = torch.outer(g, g).expand(2, 1, 11, 11)
    x = pred.double()
    assert torch.allclose(IO._filter64(x), F.conv2d(x, w2, padding=5, groups=2), rtol=0, atol=1e-14)
    S = IO.ssim_matrix64(pred, truth)
    pairs = torch.tensor([[4, 0], [1, 3], [0, 4]])
    assert torch.equal(IO.ssim_pairs64(pred, truth, pairs, chunk=2), S[pairs[:, 0], pairs[:, 1]])
    # the fp32 oracle agrees with it to fp32 rounding
    assert (IO.pcc_matrix(pred, truth).double() - IO.pcc_matrix64(pred, truth)).abs().max() < 1e-6
    assert (IO.ssim_matrix(pred, truth).double() - S).abs().max() < 1e-6
