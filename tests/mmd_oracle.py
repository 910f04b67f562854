"""CPU oracle of the MMD latent penalty (fmri_hip.mmd, WaeStep(penalty="mmd")).

The reference has no MMD step, so nothing reference-generated pins it.  Instead:
  * ``mmd_u``: an fp64 restatement of the unbiased IMQ statistic in torch (autograd gives the gradient), itself checked
    against a naive double loop over pairs (``mmd_u_loop``) and by torch.autograd.gradcheck;
  * ``wae_mmd_step``: the WAE Stage I / II / III step of oracle/vaegan_oracle.py with the latent-discriminator phase and
    penalty replaced by lam_mmd * MMD_u -- composed from the oracle's encoder / decoder / Adam pieces, which the
    reference-generated goldens pin, and never modifying them.  The forward passes (and so the BatchNorm running-stat
    updates) are those of the scripts, as in the engine.
"""
import math
from typing import Dict, Sequence

import torch
import torch.nn.functional as F

from oracle.vaegan_oracle import (_grads, cognitive_encoder_fwd, cognitive_encoder_spec, decoder_fwd, decoder_spec,
                                  encoder_fwd, encoder_spec, opt_step, param_keys)

SCALES = (0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0)


def _consts(d: int, sigma2: float, scales: Sequence[float]):
    return [2.0 * d * sigma2 * s for s in scales]


def mmd_u(q: torch.Tensor, p: torch.Tensor, sigma2: float = 0.25, scales: Sequence[float] = SCALES) -> torch.Tensor:
    """Unbiased MMD_u(q, p), IMQ kernel k(a,b) = sum_s C_s / (C_s + |a-b|^2), C_s = 2 d sigma2 s, in fp64:
    [sum_{i!=j} k(p_i,p_j) + sum_{i!=j} k(q_i,q_j)] / (n(n-1)) - 2/n^2 sum_{i,j} k(q_i,p_j).  Differentiable in q and p
    (the engine only back-propagates into q)."""
    n, d = q.shape
    if n < 2:
        raise ValueError(f"MMD_u needs n >= 2 (got {n})")
    q, p = q.double(), p.double()
    off = ~torch.eye(n, dtype=torch.bool)

    def k(a, b):
        r = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
        return sum(c / (c + r) for c in _consts(d, sigma2, scales))
    same = (k(p, p)[off].sum() + k(q, q)[off].sum()) / (n * (n - 1))
    return same - 2.0 / (n * n) * k(q, p).sum()


def mmd_u_loop(q, p, sigma2: float = 0.25, scales: Sequence[float] = SCALES) -> float:
    """The definition term by term in Python floats (a naive double loop over pairs)."""
    q, p = q.double().tolist(), p.double().tolist()
    n, d = len(q), len(q[0])
    cs = _consts(d, sigma2, scales)

    def k(a, b):
        r = math.fsum((x - y) ** 2 for x, y in zip(a, b))
        return math.fsum(c / (c + r) for c in cs)
    spp = math.fsum(k(p[i], p[j]) for i in range(n) for j in range(n) if i != j)
    sqq = math.fsum(k(q[i], q[j]) for i in range(n) for j in range(n) if i != j)
    sqp = math.fsum(k(q[i], p[j]) for i in range(n) for j in range(n))
    return (spp + sqq) / (n * (n - 1)) - 2.0 / (n * n) * sqp


def mmd_u_grad(q, p, sigma2: float = 0.25, scales: Sequence[float] = SCALES):
    """(MMD_u, dMMD_u/dq) in fp64."""
    qd = q.detach().double().requires_grad_(True)
    v = mmd_u(qd, p.detach().double(), sigma2, scales)
    (g,) = torch.autograd.grad(v, qd)
    return v.detach(), g


def _leaf(P, keys):
    for k in keys:
        P[k] = P[k].detach().requires_grad_(True)


def _done(P, keys):
    for k in keys:
        P[k] = P[k].detach()


def wae_mmd_step(P, opts: Dict, stage: int, cfg, x: torch.Tensor, z_fake_noise: torch.Tensor = None,
                 fmri: torch.Tensor = None, n_voxels: int = 0, lam_mmd: float = 10.0, sigma2: float = 0.25,
                 keep_grads: bool = False):
    """One WAE step with the MMD penalty: train_wae_stage{1,2,3}.py minus the latent-discriminator phase, with
    l_pen = lam_mmd * n * MMD_u(mu, 0.5 * z_fake_noise) (Stage I, sum convention) or lam_mmd * MMD_u(mu, mu_teacher)
    (Stages II / III, mean convention; Stage III logs it only).  The discriminator is not touched."""
    n = x.shape[0]
    if stage == 1:
        enc_k, dec_k = param_keys(encoder_spec(cfg)), param_keys(decoder_spec(cfg))
        with torch.no_grad():
            encoder_fwd(P, "encoder.", x, cfg)                                # :275 (BatchNorm side effects only)
        _leaf(P, enc_k + dec_k)
        z, _ = encoder_fwd(P, "encoder.", x, cfg)                             # :296
        x_recon = decoder_fwd(P, "decoder.", z, cfg)
        l_rec = torch.sum(torch.sum(0.5 * (x_recon - x) ** 2, 1))             # :301
        l_pen = (lam_mmd * n * mmd_u(z, 0.5 * z_fake_noise, sigma2)).float()
        g_rec = _grads(l_rec, P, enc_k + dec_k, True)
        g_pen = _grads(l_pen, P, enc_k + dec_k, False)
        g = [a if b is None else a + b for a, b in zip(g_rec, g_pen)]
        opt_step(P, enc_k, g[:len(enc_k)], opts["encoder"])
        opt_step(P, dec_k, g[len(enc_k):], opts["decoder"])
        _done(P, enc_k + dec_k)
        grads = dict(zip(enc_k + dec_k, g))
    elif stage == 2:
        enc_k = param_keys(cognitive_encoder_spec(cfg, n_voxels))
        with torch.no_grad():
            z_t, _ = encoder_fwd(P, "teacher_net.encoder.", x, cfg)         # :284
            decoder_fwd(P, "decoder.", z_t, cfg)                              # :285 x_gt: BN side effects only
            cognitive_encoder_fwd(P, "encoder.", fmri)                        # :292
            encoder_fwd(P, "teacher_net.encoder.", x, cfg)                    # :293
        _leaf(P, enc_k)
        z, _ = cognitive_encoder_fwd(P, "encoder.", fmri)                     # :314
        x_recon = decoder_fwd(P, "decoder.", z, cfg)
        l_rec = F.mse_loss(x_recon, x)                                        # :320
        l_pen = (lam_mmd * mmd_u(z, z_t, sigma2)).float()
        g_rec, g_pen = _grads(l_rec, P, enc_k, True), _grads(l_pen, P, enc_k, False)
        g = [y if a is None else (a if y is None else a + y) for a, y in zip(g_rec, g_pen)]
        opt_step(P, enc_k, g, opts["encoder"])
        _done(P, enc_k)
        grads = dict(zip(enc_k, g))
    else:
        dec_k = param_keys(decoder_spec(cfg))
        with torch.no_grad():
            cognitive_encoder_fwd(P, "encoder.", fmri)                        # :311
            z_t, _ = encoder_fwd(P, "teacher_net.encoder.", x, cfg)         # :312
            z, _ = cognitive_encoder_fwd(P, "encoder.", fmri)                 # :333
        _leaf(P, dec_k)
        x_recon = decoder_fwd(P, "decoder.", z, cfg)
        l_rec = F.mse_loss(x_recon, x)                                        # :339
        l_pen = (lam_mmd * mmd_u(z, z_t, sigma2)).float()                     # logged only (:344)
        g = _grads(l_rec, P, dec_k, False)
        opt_step(P, dec_k, g, opts["decoder"])
        _done(P, dec_k)
        grads = dict(zip(dec_k, g))
    logs = dict(loss_reconstruction=l_rec.item(), loss_penalty=l_pen.item(), loss_discriminator_fake=0.0,
                loss_discriminator_real=0.0)
    out = dict(logs=logs, fw=dict(x_recon=x_recon.detach(), z_real=z.detach()))
    if keep_grads:
        out["grads"] = grads
    return out
