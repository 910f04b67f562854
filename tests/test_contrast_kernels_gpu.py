"""GPU checks of csrc/contrast.hip (fmri_latent_nce) against the float64 oracle of tests/contrast_oracle.py: value, gradient
and top-1 count under the worst-case bounds derived there (not tuned: a ratio above 1 means the kernel or the derivation
is wrong), the zero-row convention, determinism and HIP-graph capture, accumulation, the rejected geometries, and
fmri_hip.contrast.info_nce as an autograd function."""
import pytest
import torch

import contrast_oracle as CO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS, DS, TAUS = (2, 3, 17, 64, 256, 1000), (128, 512, 1024), (0.07, 0.01)
_REF = {}


def _case(n, d, tau, symmetric=True):
    """The recipe's padded device rows and the float64 reference of one case (computed once, shared, never modified)."""
    key = (n, d, tau, symmetric)
    if key not in _REF:
        if (n, d) not in _REF:
            _REF[(n, d)] = CO.recipe(n, d, pad_q=4 if n % 2 else 12, pad_t=8)
        qw, tw = _REF[(n, d)]
        ref = CO.nce64(qw[:, :d], tw[:, :d], tau, symmetric)
        _REF[key] = (ref, CO.bounds(ref, d, tau))
    qw, tw = _REF[(n, d)]
    return qw.to(DEV)[:, :d], tw.to(DEV)[:, :d], _REF[key][0], _REF[key][1]


def _kernel(q, t, tau, symmetric=True, dq_pad=0, **kw):
    from fmri_hip.contrast import latent_nce
    n, d = q.shape
    total = torch.zeros(1, dtype=torch.float32, device=DEV)
    top1 = torch.zeros(1, dtype=torch.float32, device=DEV)
    dqw = torch.full((n, d + dq_pad), float("nan"), dtype=torch.float32, device=DEV)
    dq = dqw[:, :d]
    latent_nce(q, t, tau, symmetric, total=total, top1=top1, dq=dq, **kw)
    return total, top1, dq, dqw


def _check(n, d, tau, symmetric):
    q, t, ref, b = _case(n, d, tau, symmetric)
    assert q.stride(0) > d and t.stride(0) > d                       # padded input rows
    total, top1, dq, dqw = _kernel(q, t, tau, symmetric, dq_pad=8)
    torch.cuda.synchronize()
    got = total.item()
    lerr = abs(got - float(ref["loss"]))
    rerr = (dq.double().cpu() - ref["grad"]).norm(dim=1)
    gratio = (rerr / b["grad"]).max().item()
    hits, near = CO.top1_count(ref, b["eps_s"])
    got_hits = top1.item() * n
    print(f"n {n} d {d} tau {tau} sym {int(symmetric)}: L {got:.7e} ref {float(ref['loss']):.7e} err/bound "
          f"{lerr / b['loss']:.3e}  dq row err/bound max {gratio:.3e} (|dq| {ref['grad'].norm().item():.3e})  hits "
          f"{got_hits:.2f} ref {hits} (+{int(near.sum())} near a tie)")
    assert lerr <= b["loss"], (got, float(ref["loss"]), b["loss"])
    assert gratio <= 1.0, gratio
    assert torch.isnan(dqw[:, d:]).all() and torch.isfinite(dq).all()      # nothing written past d in a padded row
    # top-1: the rows within 2 eps_s of a tie may fall either way; at most one such row per case
    k = int(near.sum())
    assert k <= 1, k
    assert abs(got_hits - round(got_hits)) < 1e-3                    # (fp32 rate: n * top1 is a count to 1e-4 at n = 1000)
    assert hits <= round(got_hits) <= hits + k, (got_hits, hits, k)


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_kernel_matches_fp64(n, d, tau):
    _check(n, d, tau, True)


@pytest.mark.parametrize("n,d,tau", [(2, 128, 0.07), (17, 512, 0.01), (256, 128, 0.07), (1000, 1024, 0.01)])
def test_kernel_matches_fp64_one_sided(n, d, tau):
    _check(n, d, tau, False)


def test_zero_rows_stay_finite():
    n, d, tau = 17, 128, 0.07
    qw, tw = CO.recipe(n, d, pad_q=4, pad_t=8)
    qw, tw = qw.clone(), tw.clone()
    qw[3, :d] = 0.0
    tw[5, :d] = 0.0
    ref = CO.nce64(qw[:, :d], tw[:, :d], tau)
    b = CO.bounds(ref, d, tau)
    total, top1, dq, _ = _kernel(qw.to(DEV)[:, :d], tw.to(DEV)[:, :d], tau)
    torch.cuda.synchronize()
    assert torch.isfinite(total).all() and torch.isfinite(top1).all() and torch.isfinite(dq).all()
    assert bool((dq[3] == 0).all())
    assert abs(total.item() - float(ref["loss"])) <= b["loss"]
    rows = [i for i in range(n) if i != 3]
    rerr = (dq.double().cpu() - ref["grad"]).norm(dim=1)
    assert (rerr[rows] / b["grad"][rows]).max().item() <= 1.0


def test_two_calls_bit_identical_and_graph_replay_equals_eager():
    from fmri_hip.contrast import latent_nce
    n, d, tau = 256, 128, 0.07
    q, t, _, _ = _case(n, d, tau)
    t1, h1, dq1, _ = _kernel(q, t, tau)
    t2, h2, dq2, _ = _kernel(q, t, tau)
    torch.cuda.synchronize()
    assert torch.equal(t1, t2) and torch.equal(h1, h2) and torch.equal(dq1, dq2)
    total = torch.zeros(1, dtype=torch.float32, device=DEV)
    top1 = torch.zeros(1, dtype=torch.float32, device=DEV)
    dq = torch.empty(n, d, dtype=torch.float32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        latent_nce(q, t, tau, total=total, top1=top1, dq=dq)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        total.zero_()
        top1.zero_()
        latent_nce(q, t, tau, total=total, top1=top1, dq=dq)
    dq.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(total, t1) and torch.equal(top1, h1) and torch.equal(dq, dq1)


@pytest.mark.selfcheck
def test_two_calls_bit_identical_in_either_deterministic_mode():
    from fmri_hip import ops
    n, d, tau = 64, 512, 0.01
    q, t, _, _ = _case(n, d, tau)
    was = ops.set_deterministic(True)
    try:
        t1, h1, dq1, _ = _kernel(q, t, tau)
        ops.set_deterministic(False)
        t2, h2, dq2, _ = _kernel(q, t, tau)
    finally:
        ops.set_deterministic(was)
    torch.cuda.synchronize()
    assert torch.equal(t1, t2) and torch.equal(h1, h2) and torch.equal(dq1, dq2)


def test_weight_gscale_value_only_and_accumulation():
    from fmri_hip.contrast import latent_nce
    n, d, tau = 64, 512, 0.07
    q, t, _, _ = _case(n, d, tau)
    t1, h1, dq1, _ = _kernel(q, t, tau)
    total = torch.full((1,), 2.0, dtype=torch.float32, device=DEV)
    top1 = torch.full((1,), 1.0, dtype=torch.float32, device=DEV)
    dq = torch.empty(n, d, dtype=torch.float32, device=DEV)
    latent_nce(q, t, tau, w=3.0, total=total, top1=top1, dq=dq, gscale=0.5)
    t0 = torch.full((1,), 2.0, dtype=torch.float32, device=DEV)
    latent_nce(q, t, tau, w=3.0, total=t0)                           # value only
    tv = torch.zeros(1, dtype=torch.float32, device=DEV)
    latent_nce(q, t, tau, total=tv)
    torch.cuda.synchronize()
    assert abs(total.item() - (2.0 + 3.0 * t1.item())) < 1e-6 * max(1.0, 3.0 * t1.item()) and torch.equal(total, t0)
    assert torch.equal(tv, t1)                                       # the value-only call: the same bits
    assert abs(top1.item() - (1.0 + h1.item())) < 1e-6              # the rate carries no weight
    assert ((dq - 1.5 * dq1).norm() / dq1.norm()).item() < 1e-6


def test_info_nce_autograd_function():
    from fmri_hip.contrast import info_nce
    n, d, tau = 17, 128, 0.07
    q, t, ref, b = _case(n, d, tau)
    qq = q.clone().requires_grad_(True)
    tt = t.clone().requires_grad_(True)
    v = info_nce(qq, tt, tau)
    (3.0 * v).backward()
    assert v.dim() == 0 and v.dtype == torch.float32 and abs(v.item() - float(ref["loss"])) <= b["loss"]
    rerr = (qq.grad.double().cpu() / 3.0 - ref["grad"]).norm(dim=1)
    assert (rerr / b["grad"]).max().item() <= 1.0
    assert tt.grad is None
    with pytest.raises(ValueError):
        info_nce(q[:1], t[:1])
    with pytest.raises(ValueError):
        info_nce(q, t, temperature=0.005)


def test_rejected_geometry_leaves_the_outputs_alone():
    from fmri_hip.contrast import latent_nce

    def attempt(n, d, tau):
        q = torch.ones(n, d, dtype=torch.float32, device=DEV)
        total = torch.full((1,), 7.0, dtype=torch.float32, device=DEV)
        top1 = torch.full((1,), 7.0, dtype=torch.float32, device=DEV)
        dq = torch.full((n, d), 7.0, dtype=torch.float32, device=DEV)
        with pytest.raises((ValueError, RuntimeError)):
            latent_nce(q, q.clone(), tau, total=total, top1=top1, dq=dq)
        torch.cuda.synchronize()
        assert total.item() == 7.0 and top1.item() == 7.0 and bool((dq == 7.0).all())
    attempt(1, 128, 0.07)
    attempt(8, 96, 0.07)
    attempt(8, 128, 0.005)
    attempt(4097, 64, 0.07)
