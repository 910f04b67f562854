"""Host-side checks of the MMD latent penalty (no GPU): the fp64 restatement in tests/mmd_oracle.py against the definition
(a naive double loop, the closed-form gradient, torch.autograd.gradcheck), the C ABI declaration and argument checks of
fmri_mmd_imq, and the Python surface (GPU tensors only, penalty="mmd")."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import mmd_oracle as M

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def lib():
    from fmri_hip import build, lib as L
    build.build(verbose=False)
    return L.load()


def _pair(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(n, d, generator=g, dtype=torch.float64) * 0.7 + 0.3
    p = torch.randn(n, d, generator=g, dtype=torch.float64) * 0.5
    return q, p


@pytest.mark.parametrize("n,d", [(2, 3), (3, 8), (7, 5), (12, 16)])
def test_mmd_u_equals_the_double_loop(n, d):
    q, p = _pair(n, d, n * 100 + d)
    for sigma2 in (0.25, 1.0):
        got = M.mmd_u(q, p, sigma2).item()
        want = M.mmd_u_loop(q, p, sigma2)
        assert abs(got - want) < 1e-12, (n, d, sigma2, got, want)
    # symmetric in the two sides
    assert abs(M.mmd_u(q, p).item() - M.mmd_u(p, q).item()) < 1e-12


def test_mmd_u_gradient_is_the_closed_form():
    """dMMD_u/dq_i = 4/(n(n-1)) sum_{j!=i} k'(r^qq_ij)(q_i-q_j) - 4/n^2 sum_j k'(r^qp_ij)(q_i-p_j),
    k'(r) = -sum_s C_s/(C_s+r)^2."""
    n, d, sigma2 = 9, 6, 0.25
    q, p = _pair(n, d, 7)
    _, g = M.mmd_u_grad(q, p, sigma2)
    cs = [2.0 * d * sigma2 * s for s in M.SCALES]

    def kp(r):
        return -sum(c / (c + r) ** 2 for c in cs)
    want = torch.zeros(n, d, dtype=torch.float64)
    for i in range(n):
        for j in range(n):
            if j != i:
                want[i] += 4.0 / (n * (n - 1)) * kp(((q[i] - q[j]) ** 2).sum()) * (q[i] - q[j])
            want[i] -= 4.0 / (n * n) * kp(((q[i] - p[j]) ** 2).sum()) * (q[i] - p[j])
    assert (g - want).abs().max().item() < 1e-14


def test_mmd_u_passes_gradcheck():
    q, p = _pair(6, 4, 3)
    q.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a: M.mmd_u(a, p), (q,), eps=1e-6, atol=1e-9)


def test_mmd_u_rejects_fewer_than_two_rows():
    q, p = _pair(1, 4, 1)
    with pytest.raises(ValueError):
        M.mmd_u(q, p)


def test_fmri_mmd_imq_is_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "fmri_hip.h")).read()
    assert re.search(r"\bint fmri_mmd_imq\s*\(", hdr)
    assert re.search(r"\bint64_t fmri_mmd_imq_ws_bytes\s*\(", hdr)
    assert hasattr(lib, "fmri_mmd_imq") and hasattr(lib, "fmri_mmd_imq_ws_bytes")


def test_fmri_mmd_imq_argument_checks_without_gpu(lib):
    """Rejected on the host before anything is enqueued: n < 2, unsupported d, short leading dimensions, misaligned rows,
    a workspace below fmri_mmd_imq_ws_bytes."""
    assert lib.fmri_mmd_imq_ws_bytes(1, 128) < 0
    assert lib.fmri_mmd_imq_ws_bytes(64, 100) < 0
    for n, d in ((2, 128), (17, 512), (1000, 1024), (64, 64)):
        assert lib.fmri_mmd_imq_ws_bytes(n, d) > 0
    z = ctypes.c_void_p(256)
    big = 1 << 40

    def call(q=z, ldq=128, p=z, ldp=128, n=8, d=128, sigma2=0.25, w=1.0, dq=z, ldd=128, ws=z, nb=big):
        return lib.fmri_mmd_imq(q, ldq, p, ldp, n, d, sigma2, None, 0, w, None, dq, ldd, 1.0, ws, nb, None)
    assert call(n=1) == -1
    assert call(ldq=64) == -1 and call(ldp=100) == -1 and call(ldd=64) == -1
    assert call(sigma2=0.0) == -1
    assert call(q=ctypes.c_void_p(260)) == -1
    assert call(ldq=130, d=128) == -1
    assert call(d=100, ldq=128, ldp=128, ldd=128) == -2
    assert call(d=2048, ldq=2048, ldp=2048, ldd=2048) == -2
    assert call(nb=16) == -4
    bad = (ctypes.c_float * 2)(1.0, -1.0)
    assert lib.fmri_mmd_imq(z, 128, z, 128, 8, 128, 0.25, bad, 2, 1.0, None, z, 128, 1.0, z, big, None) == -1


def test_imq_mmd_has_no_cpu_fallback():
    from fmri_hip.mmd import imq_mmd
    q, p = _pair(4, 64, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        imq_mmd(q.float(), p.float())


def test_wae_step_surface():
    from fmri_hip.wae_steps import WaeHyper, WaeStep
    sig = inspect.signature(WaeStep.__init__)
    assert sig.parameters["penalty"].default == "gan"
    hp = WaeHyper()
    assert hp.lam_mmd == 10.0 and hp.mmd_sigma2 == 0.25
    assert WaeHyper.stage23().lam_mmd == 10.0
    assert "DualStage1Step" in inspect.getdoc(__import__("fmri_hip.wae_steps", fromlist=["x"]))
