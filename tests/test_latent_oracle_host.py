"""CPU checks of tests/latent_oracle.py, the float64 references and bounds of tests/test_latent_path_gpu.py:

  * the references equal float64 torch autograd of the same operations;
  * a numpy emulation of the kernels' arithmetic (float32 matmul on the fp16 inputs, one rounding to fp16) stays inside
    the bounds on every element, at every shape and with the inputs the GPU tests use: the bounds are not too tight;
  * the comparison rejects subtly wrong kernels: five corruptions of the emulation's output each give err / bound > 1,
    where the whole-tensor L2 ratio of tests/test_wae_gpu.py::test_latent_discriminator_fused_kernels stays under its
    threshold.

Every check prints ``[latent] <case> | <quantity> | err/bound = r``; profiles/latent_path_parity.md records them.
"""
import numpy as np
import pytest
import torch

import latent_oracle as LO

F16, F32 = np.float16, np.float32


def _say(case, what, r, asserted=True):
    print(f"[latent] {case} | {what} | err/bound = {r:.4f}" + ("" if asserted else " (report only)"), flush=True)
    if asserted:
        assert r <= 1.0, f"{case}: {what}: err / bound = {r:.4f}"
    return r


# ---------------------------------------------------------------------------------------------------------------------
# the references against autograd
# ---------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = LO.f64(a), LO.f64(b)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


@pytest.mark.parametrize("M,Z", [(5, 64), (33, 100)])
def test_mlp_references_chain_to_autograd(M, Z):
    """With the fp16 rounding between the layers switched off (each function is fed the previous one's float64 result)
    the per-layer references are the five-layer MLP and its gradient: logit, the five bias gradients and dz against
    float64 torch autograd, 1e-12 relative."""
    rs = np.random.RandomState(M + Z)
    H, inv = 512, 0.25
    dims = [Z, H, H, H, H, 1]
    Ws = [rs.randn(dims[j + 1], dims[j]) * np.sqrt(2.0 / dims[j]) for j in range(5)]
    bs = [rs.randn(dims[j + 1]) * 0.05 for j in range(5)]
    z, dl = rs.randn(M, Z), rs.randn(M)
    hs, x = [], z
    for L in range(4):
        x, _ = LO.mlp_layer64(x, Ws[L], bs[L], True)
        hs.append(x)
    logit, _ = LO.mlp_layer64(x, Ws[4], bs[4], False)
    delta = [None] * 4
    delta[3], _ = LO.mlp_delta4_64(dl, Ws[4][0], hs[3])
    for L in (3, 2, 1):
        delta[L - 1], _ = LO.mlp_delta_64(delta[L], Ws[L].T, hs[L - 1])
    dz, _ = LO.mlp_dz64(delta[0], Ws[0].T, inv)
    dbias = [LO.mlp_dbias64(delta[i] if i < 4 else dl.reshape(M, 1), inv, np.zeros(dims[i + 1]))[0] for i in range(5)]

    zt = torch.from_numpy(z).requires_grad_(True)
    Wt = [torch.from_numpy(w) for w in Ws]
    bt = [torch.from_numpy(b).requires_grad_(True) for b in bs]
    h = zt
    for L in range(4):
        h = torch.relu(h @ Wt[L].t() + bt[L])
    lt = h @ Wt[4].t() + bt[4]
    ((lt[:, 0] * torch.from_numpy(dl)).sum() * inv).backward()
    assert _rel(logit, lt.detach().numpy()) < 1e-12
    assert _rel(dz, zt.grad.numpy()) < 1e-12
    for i in range(5):
        assert _rel(dbias[i], bt[i].grad.numpy()) < 1e-12, i
    # the sums of absolute values bound the results they belong to
    p, S = LO.mlp_layer64(z, Ws[0], bs[0], False)
    assert bool((np.abs(p) <= S * (1 + 1e-12)).all())


@pytest.mark.parametrize("sample", [0, 1])
@pytest.mark.parametrize("Z,zp,ldz", [(8, 8, 8), (100, 104, 128)])
def test_latent_references_match_autograd(Z, zp, ldz, sample):
    """latent_bwd64 is the gradient of sum(z * g) + w * sum(kl) of latent_fwd64's z and KL; z's padding columns are
    zero and kl_total is the sum of the rows."""
    B = 7
    head, eps, dz = LO.latent_inputs(B, Z, seed=Z + sample, edges=False)
    dzl = np.full((B, ldz), np.nan, F32)
    dzl[:, :Z] = dz
    dz_unscale, kl_w, kl_dev, out_scale = 0.5, 0.7, 3.0, 16.0
    z, klr, klt = LO.latent_fwd64(head, eps, Z, zp, sample)
    assert z.shape == (B, zp) and bool((z[:, Z:] == 0).all()) and abs(klt - klr.sum()) <= 1e-12 * abs(klt)
    dh, dh_s = LO.latent_bwd64(head, eps, dzl, ldz, dz_unscale, kl_w, kl_dev, out_scale, sample)
    ht = torch.from_numpy(head.astype(np.float64)).requires_grad_(True)
    mu, lv = ht[:, :Z], ht[:, Z:]
    zt = torch.from_numpy(eps.astype(np.float64)) * torch.exp(0.5 * lv) + mu if sample else mu
    kl = -0.5 * torch.sum(-lv.exp() - mu.pow(2) + lv + 1, 1)
    assert _rel(z[:, :Z], zt.detach().numpy()) < 1e-12 and _rel(klr, kl.detach().numpy()) < 1e-12
    ((zt * torch.from_numpy(dz.astype(np.float64)) * dz_unscale).sum() + kl_w * kl_dev * kl.sum()).backward()
    assert _rel(dh, ht.grad.numpy()) < 1e-12
    assert _rel(dh_s, ht.grad.numpy() * out_scale) < 1e-12
    none, _ = LO.latent_bwd64(head, eps, None, 0, 1.0, kl_w, None, 1.0, sample)      # dz = NULL, kl_dev = NULL
    ht.grad = None
    (kl_w * (-0.5 * torch.sum(-ht[:, Z:].exp() - ht[:, :Z].pow(2) + ht[:, Z:] + 1, 1)).sum()).backward()
    assert _rel(none, ht.grad.numpy()) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# a numpy emulation of the kernels' arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def _weights16(Z, Zp):
    sd = LO.mlp_params(Z)
    Wf = []
    for j, idx in enumerate((0, 2, 4, 6, 8)):
        w = sd[f"main.{idx}.weight"].astype(F16)
        if j == 0 and Zp > Z:
            w = np.concatenate([w, np.zeros((w.shape[0], Zp - Z), F16)], axis=1)
        Wf.append(w)
    return Wf, [sd[f"main.{idx}.bias"] for idx in (0, 2, 4, 6, 8)]


def _emulate(z16, Wf, bs, dl16, inv_scale, Z, priors, backward=True):
    """float32 matmul on the fp16 inputs, bias, ReLU, one rounding to fp16 -- the arithmetic of csrc/mlp.hip."""
    out = {"hs": [], "delta": None, "dz": None, "dbias": None}
    x = z16
    for L in range(4):
        f = x.astype(F32) @ Wf[L].astype(F32).T + bs[L].astype(F32)
        x = np.maximum(f, F32(0)).astype(F16)
        out["hs"].append(x)
    out["logit"] = (x.astype(F32) @ Wf[4][0].astype(F32) + bs[4].astype(F32)[0]).astype(F32)
    if not backward:
        return out
    inv = F32(inv_scale)
    delta = [None] * 4
    delta[3] = ((dl16.astype(F32)[:, None] * Wf[4][0].astype(F32)[None, :]) * (out["hs"][3] > 0)).astype(F16)
    for L in (3, 2, 1):
        delta[L - 1] = ((delta[L].astype(F32) @ Wf[L].astype(F32)) * (out["hs"][L - 1] > 0)).astype(F16)
    out["delta"] = delta
    out["dz"] = ((delta[0].astype(F32) @ Wf[0].astype(F32))[:, :Z] * inv).astype(F32)
    out["dbias"] = [(priors[i] + delta[i].astype(F32).sum(0, dtype=F32) * inv).astype(F32) for i in range(4)]
    out["dbias"].append((priors[4] + dl16.astype(F32).sum(dtype=F32) * inv).astype(F32))
    return out


def _case(M, Z, Zp, inv_scale=0.25, backward=True):
    Wf, bs = _weights16(Z, Zp)
    z16, dl16, priors = LO.mlp_inputs(M, Z, Zp, seed=1000 * Zp + M)
    out = _emulate(z16, Wf, bs, dl16, inv_scale, Z, priors, backward)
    args = (z16, Wf, bs, [w.T for w in Wf[:4]], dl16, inv_scale, Z, priors)
    return out, args


_EMU = [(M, Z, Z, True) for M, Z in LO.MLP_SHAPES] + [(77, 100, 128, True)] + [(M, Z, Z, False) for M, Z in LO.MLP_FWD_ONLY]


@pytest.mark.parametrize("M,Z,Zp,backward", _EMU, ids=[f"M{c[0]}-Z{c[1]}-Zp{c[2]}" for c in _EMU])
def test_emulation_stays_inside_the_bounds(M, Z, Zp, backward):
    """The bounds are not too tight: plain float32 arithmetic on the GPU tests' inputs gives err / bound <= 1 on every
    element of every output.  The inputs contain what the GPU tests rely on: exact zeros behind the ReLU and all-zero
    rows of z."""
    out, args = _case(M, Z, Zp, backward=backward)
    assert all(bool((h == 0).any()) and bool((h > 0).any()) for h in out["hs"]), "exact zeros behind the ReLU"
    if M > 2:
        assert bool((args[0] == 0).all(axis=1).any()), "an all-zero row of z"
    worst = 0.0
    for what, r in LO.mlp_ratios(out, *args).items():
        worst = max(worst, _say(f"emulation M={M} Z={Z} Zp={Zp}", what, r))
    print(f"[latent] emulation M={M} Z={Z} Zp={Zp} | largest | err/bound = {worst:.4f}")


@pytest.mark.parametrize("B,Z,zp", [(3, 100, 104), (259, 128, 128), (256, 8, 8)])
def test_latent_emulation_stays_inside_the_project_tolerances(B, Z, zp):
    """float32 arithmetic with an exact exponential, rounded to fp16, against latent_fwd64 / latent_bwd64 under the
    tolerances of tests/test_kernels_gpu.py::_close (2e-3 fp16, 1e-4 kl rows and fp32 gradient, 1e-3 total), with the
    edge entries of the GPU tests' inputs."""
    head, eps, dz = LO.latent_inputs(B, Z, seed=B + Z, edges=True)
    mu, lv = head[:, :Z], head[:, Z:]
    z_ref, klr_ref, klt_ref = LO.latent_fwd64(head, eps, Z, zp, 1)
    z16 = np.zeros((B, zp), F16)
    z16[:, :Z] = (eps * np.exp(F32(0.5) * lv).astype(F32) + mu).astype(F16)
    klr = (F32(-0.5) * (-np.exp(lv).astype(F32) - mu * mu + lv + F32(1))).sum(1, dtype=F32)
    case = f"emulation latent B={B} Z={Z} zp={zp}"
    _say(case, "z16", LO.close_ratio(z16, z_ref, 2e-3))
    _say(case, "kl_rows", LO.close_ratio(klr, klr_ref, 1e-4))
    _say(case, "kl_total", abs(float(klr.sum(dtype=F32)) - klt_ref) / (1e-3 * abs(klt_ref)))
    kl_w, unscale = 5e-6, 1.0 / 64
    ref, ref_s = LO.latent_bwd64(head, eps, dz, Z, unscale, kl_w, None, 16.0, 1)
    g = dz * F32(unscale)
    dmu = g + F32(kl_w) * mu
    dlv = F32(kl_w) * F32(0.5) * (np.exp(lv).astype(F32) - F32(1)) + g * eps * F32(0.5) * np.exp(F32(0.5) * lv).astype(F32)
    d32 = np.concatenate([dmu, dlv], axis=1).astype(F32)
    _say(case, "dhead32", LO.close_ratio(d32, ref, 1e-4))
    _say(case, "dhead16 (out_scale 16)", LO.close_ratio((d32 * F32(16)).astype(F16), ref_s, 2e-3))


# ---------------------------------------------------------------------------------------------------------------------
# the comparison rejects wrong kernels
# ---------------------------------------------------------------------------------------------------------------------
def _ratios(out, args):
    return LO.mlp_ratios(out, *args)


def test_lost_bias_on_one_fragment_is_rejected():
    """hs[1] without its bias on columns [16, 20) of rows [32, 64) -- one lane's 4-column fragment over one 32-row
    block.  The L2 ratio of the whole 512 x 512 activation stays under the 2e-3 of test_latent_discriminator_fused_kernels;
    the per-element comparison rejects it."""
    out, args = _case(512, 128, 128)
    z16, Wf, bs = args[0], args[1], args[2]
    good = out["hs"][1].copy()
    f = out["hs"][0].astype(F32) @ Wf[1].astype(F32).T
    out["hs"][1][32:64, 16:20] = np.maximum(f, F32(0)).astype(F16)[32:64, 16:20]
    assert bool((out["hs"][1] != good).any())
    l2 = LO.l2_ratio(out["hs"][1], good)
    r = _ratios(out, args)["hs[1]"]
    print(f"[latent] corruption lost bias | hs[1] | err/bound = {r:.1f}, whole-tensor L2 ratio {l2:.3e}")
    assert l2 < 2e-3
    assert r > 1.0


def test_relu_mask_with_greater_equal_is_rejected():
    """delta[2] masked with h >= 0 instead of h > 0 (ReLU outputs hold exact zeros, so every masked element comes
    through).  Over the whole tensor that is no subtle error -- the L2 ratio of delta[2] is of order 1, printed below --
    so the statement about the old whole-tensor measure is asserted for the same wrong mask on a few elements (one
    4-column fragment of one row): there delta[2] itself and the quantities test_latent_discriminator_fused_kernels
    compares downstream of it (the layer's weight gradient, dz) move by less than its 2e-3 in the L2 ratio, and the
    per-element comparison rejects both forms."""
    out, args = _case(512, 128, 128)
    z16, Wf, inv, Z = args[0], args[1], args[5], args[6]
    hs, delta = out["hs"], out["delta"]
    good = delta[2].copy()
    unmasked = (delta[3].astype(F32) @ Wf[3].astype(F32)).astype(F16)

    def downstream(d2):
        d1 = ((d2.astype(F32) @ Wf[2].astype(F32)) * (hs[1] > 0)).astype(F16)
        d0 = ((d1.astype(F32) @ Wf[1].astype(F32)) * (hs[0] > 0)).astype(F16)
        return d2.astype(np.float64).T @ hs[1].astype(np.float64), (d0.astype(F32) @ Wf[0].astype(F32))[:, :Z] * F32(inv)
    wg_ref, dz_ref = downstream(good)

    # the whole tensor
    delta[2] = unmasked.copy()
    r_all, l2_all = _ratios(out, args)["delta[2]"], LO.l2_ratio(unmasked, good)
    # a few elements: row 40, columns [16, 20)
    frag = good.copy()
    frag[40, 16:20] = unmasked[40, 16:20]
    assert bool((hs[2][40, 16:20] == 0).any()) and bool((frag != good).any()), "the fragment holds an exact zero of h"
    delta[2] = frag
    r_frag = _ratios(out, args)["delta[2]"]
    wg, dz = downstream(frag)
    l2_wg, l2_dz = LO.l2_ratio(wg, wg_ref), LO.l2_ratio(dz, dz_ref)
    print(f"[latent] corruption mask >= (whole tensor) | delta[2] | err/bound = {r_all:.1f}, L2 ratio of delta[2] {l2_all:.3e}")
    print(f"[latent] corruption mask >= (row 40, columns 16..19) | delta[2] | err/bound = {r_frag:.1f}, "
          f"L2 ratio of the weight gradient {l2_wg:.3e}, of dz {l2_dz:.3e}, of delta[2] {LO.l2_ratio(frag, good):.3e}")
    assert r_all > 1.0 and r_frag > 1.0
    assert LO.l2_ratio(frag, good) < 2e-3 and l2_wg < 2e-3 and l2_dz < 2e-3


def test_stale_last_row_of_dz_is_rejected():
    """Row M - 1 (M = 77, the partial block) of dz left at its previous contents (zeros)."""
    out, args = _case(77, 128, 128)
    out["dz"][76] = 0.0
    r = _ratios(out, args)["dz"]
    print(f"[latent] corruption stale last row | dz | err/bound = {r:.1f}")
    assert r > 1.0


def test_padded_row_in_the_bias_sum_is_rejected():
    """Row M's delta (a row of the padded 32-row block that does not exist) added to dbias[0]."""
    out, args = _case(77, 128, 128)
    ghost = out["delta"][0][5].astype(F32)          # any nonzero row stands in for the one behind M
    assert bool((ghost != 0).any())
    out["dbias"][0] = (out["dbias"][0] + ghost * F32(args[5])).astype(F32)
    r = _ratios(out, args)["dbias[0]"]
    print(f"[latent] corruption padded row in the sum | dbias[0] | err/bound = {r:.1f}")
    assert r > 1.0


def test_nonzero_padding_column_of_z_is_rejected():
    """A nonzero value in padding column Z of the latent z16 (Z = 100, zp = 104): the smallest positive fp16 number is
    enough, the padding is compared exactly (and the tolerance comparison sees a larger one)."""
    B, Z, zp = 3, 100, 104
    head, eps, _ = LO.latent_inputs(B, Z, seed=1, edges=False)
    ref, _, _ = LO.latent_fwd64(head, eps, Z, zp, 1)
    z16 = ref.astype(F16)
    assert LO.close_ratio(z16, ref, 2e-3) <= 1.0 and bool((z16[:, Z:] == 0).all())
    z16[1, Z] = F16(6e-8)
    assert not bool((z16[:, Z:] == 0).all())
    z16[1, Z] = F16(0.01)
    r = LO.close_ratio(z16, ref, 2e-3)
    print(f"[latent] corruption padding column | z16 | err/bound = {r:.1f}")
    assert r > 1.0
