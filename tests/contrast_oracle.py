"""CPU oracle of the contrastive latent alignment (fmri_hip.contrast, WaeStep(contrast=...)).

The reference has no contrastive term, so nothing reference-generated pins it.  Instead:
  * ``nce64``: the symmetric InfoNCE loss in float64, its gradient through autograd AND through the closed form the kernel
    implements (include/fmri_hip_contrast.h fmri_latent_nce), the logits, the top-1 hit flags and per-row margins;
  * ``bounds``: the worst-case fp32 error bounds of csrc/contrast.hip for one case, derived below;
  * ``wae_nce_step``: the WAE Stage II / III step of oracle/vaegan_oracle.py (penalty "gan") or of tests/mmd_oracle.py
    (penalty "mmd") with weight * L added to the encoder loss -- composed from the oracle's encoder / decoder /
    discriminator / Adam pieces, which the reference-generated goldens pin, and never modifying them.

Zero rows: a row of q (of t) whose squared norm is 0 has a_i = 0 (b_j = 0) -- its logits are 0 and its gradient 0.

Error bounds (u = 2^-24, the fp32 unit roundoff; eps_s = (d + 8) u / tau).
  Logits.  s_ij = a_i . b_j / tau from an fp32 dot product of the raw rows scaled by 1/(|q_i| |t_j|): any summation order
  of d products has error <= d u |q_i| |t_j| (Cauchy-Schwarz), the two reciprocal norms (from fp64 sums), the two scalings,
  the division by tau and tau's own rounding to fp32 add 6 u <= 8 u relative: |s - s64| <= eps_s.
  Loss.  Log-sum-exp is 1-Lipschitz in the sup norm and the diagonal adds one more eps_s:
  |L - L64| <= 2 eps_s + 16 u max(1, |L64|).
  Gradient.  dq_i = Pr_i v_i / (tau |q_i|), v_i = sum_j G_ij b_j, Pr_i = I - a_i a_i^T.  With A = (P + Q) / (2n) (P / n
  one-sided), S_i = sum_j A_ij >= 1 / (2n) and eta = e^{2 eps_s} - 1:
    (1) the softmax weights see the exponent s_ij - lse with error 2 eps_s from the logits, plus what fp32 adds to it: the
        subtraction (<= (2 / tau + log n) u), the log of an n-term sum in any order (<= (n + 3) u); under the condition
        n + 12 <= 0.6 (d + 8) / tau and d >= 128 that is <= 0.62 eps_s, so |dG_ij| <= (e^{2.62 eps_s} - 1) A_ij
        <= 1.32 eta A_ij (eps_s <= 6.2e-3);
    (2) sum_j |G_ij| <= S_i + 1/n <= 3 S_i; the n-term fp32 accumulation of v_i (any order), the roundings of G_ij and
        of b_j (|b_j| = 1) cost <= (n + 8) u . 3.1 S_i <= 1.86 eps_s S_i <= 0.93 eta S_i under the same condition;
    (3) the projection: |da_i| <= 2 u perturbs a_i a_i^T by <= 4 u, the fp32 dot product a_i . v_i by <= d u, the
        subtraction, scaling by gscale w / (tau |q_i|) by <= 6 u more: <= (d + 10) u |v_i| <= 1.02 (d + 8) u . 3.1 S_i.
  Together |dq_i - dq64_i| <= (2.25 eta + 3.2 (d + 8) u) S_i / (tau |q_i|) <= C_GRAD (eta + (d + 8) u) S_i / (tau |q_i|)
  with C_GRAD = 3.2.  ``bounds`` refuses a case outside the condition.
"""
from typing import Dict

import math

import torch
import torch.nn.functional as F

import mmd_oracle as MO
from oracle.vaegan_oracle import (_grads, _gsum, _leafify, _wae_dis_phase, cognitive_encoder_fwd, cognitive_encoder_spec,
                                  decoder_fwd, decoder_spec, encoder_fwd, opt_step, param_keys, wae_discriminator_fwd,
                                  wae_discriminator_spec)

U = 2.0 ** -24
C_GRAD = 3.2


def _unit(x: torch.Tensor) -> torch.Tensor:
    n2 = (x * x).sum(1, keepdim=True)
    ok = n2 > 0
    return x * torch.where(ok, torch.where(ok, n2, torch.ones_like(n2)).rsqrt(), torch.zeros_like(n2))


def nce_loss(q: torch.Tensor, t: torch.Tensor, tau: float, symmetric: bool = True) -> torch.Tensor:
    """L in float64, differentiable in q (and t): L_row = mean_i [lse_j s_ij - s_ii], L_col = mean_j [lse_i s_ij - s_jj],
    L = (L_row + L_col) / 2 if symmetric else L_row; s = a b^T / tau on unit rows (zero rows stay zero)."""
    s = _unit(q.double()) @ _unit(t.double()).t() / tau
    dg = s.diagonal()
    l_row = (torch.logsumexp(s, 1) - dg).mean()
    if not symmetric:
        return l_row
    return 0.5 * (l_row + (torch.logsumexp(s, 0) - dg).mean())


def nce64(q: torch.Tensor, t: torch.Tensor, tau: float, symmetric: bool = True) -> Dict:
    """Everything a test compares with, in float64: ``loss`` / ``grad`` through autograd, ``loss_cf`` / ``grad_cf`` through
    the closed form (G = ((P + Q) / 2 - I) / n, da = G b / tau, dq_i = (da_i - (a_i . da_i) a_i) / |q_i|), the logits
    ``s``, ``hit`` (s_ii >= max_j s_ij), ``margin`` (m_i = s_ii - max_{j != i} s_ij), ``arow`` (sum_j A_ij) and ``qnorm``."""
    qd = q.detach().double().requires_grad_(True)
    td = t.detach().double()
    n = qd.shape[0]
    loss = nce_loss(qd, td, tau, symmetric)
    (grad,) = torch.autograd.grad(loss, qd)
    with torch.no_grad():
        a, b = _unit(qd), _unit(td)
        s = a @ b.t() / tau
        dg = s.diagonal()
        P, Q = torch.softmax(s, 1), torch.softmax(s, 0)
        eye = torch.eye(n, dtype=torch.float64)
        if symmetric:
            loss_cf = 0.5 * ((torch.logsumexp(s, 1) - dg).mean() + (torch.logsumexp(s, 0) - dg).mean())
            A = (P + Q) / (2 * n)
        else:
            loss_cf = (torch.logsumexp(s, 1) - dg).mean()
            A = P / n
        G = A - eye / n
        da = G @ b / tau
        qn = qd.norm(dim=1, keepdim=True)
        inv = torch.where(qn > 0, 1.0 / torch.where(qn > 0, qn, torch.ones_like(qn)), torch.zeros_like(qn))
        grad_cf = (da - (a * da).sum(1, keepdim=True) * a) * inv
        off = s.masked_fill(eye.bool(), -math.inf)
        margin = dg - off.max(1).values
    return dict(loss=loss.detach(), grad=grad, loss_cf=loss_cf, grad_cf=grad_cf, s=s, hit=dg >= s.max(1).values,
                margin=margin, arow=A.sum(1), qnorm=qn.reshape(-1))


def eps_s(d: int, tau: float) -> float:
    return (d + 8) * U / tau


def bounds(ref: Dict, d: int, tau: float) -> Dict:
    """The derived bounds of the module docstring for one case: ``eps_s``, ``loss``, per-row ``grad`` (inf for a zero row of
    q, whose gradient is exactly 0 on both sides)."""
    n = ref["s"].shape[0]
    if d < 128 or n + 12 > 0.6 * (d + 8) / tau:
        raise ValueError(f"bounds: n={n} d={d} tau={tau} is outside the condition C_GRAD was derived under")
    e = eps_s(d, tau)
    eta = math.expm1(2 * e)
    qn = ref["qnorm"]
    grad = C_GRAD * (eta + (d + 8) * U) * ref["arow"] / (tau * torch.where(qn > 0, qn, torch.zeros_like(qn)))
    return dict(eps_s=e, loss=2 * e + 16 * U * max(1.0, abs(float(ref["loss"]))), grad=grad)


def top1_count(ref: Dict, e: float):
    """(hits among the rows that count, rows left out): a row whose margin is within 2 eps_s of a tie is left out."""
    near = ref["margin"].abs() < 2 * e
    return int((ref["hit"] & ~near).sum()), near


def recipe(n: int, d: int, pad_q: int = 0, pad_t: int = 0):
    """The data recipe of the kernel test (loss O(1), about half the rows hits at n = 1000): padded fp32 rows."""
    g = torch.Generator().manual_seed(7 * n + d)
    t = 0.6 * torch.randn(n, d, generator=g) + 0.1
    q = (2.5 / math.sqrt(d)) * t + 0.45 * torch.randn(n, d, generator=g) + 0.05
    qw = torch.full((n, d + pad_q), 3.0)
    tw = torch.full((n, d + pad_t), -2.0)
    qw[:, :d], tw[:, :d] = q, t
    return qw, tw


# ---- the composed oracle step ----------------------------------------------------------------------------------------
def _done(P, keys):
    for k in keys:
        P[k] = P[k].detach()


def wae_nce_step(P, opts: Dict, stage: int, cfg, x: torch.Tensor, fmri: torch.Tensor, n_voxels: int,
                 penalty: str = "gan", weight: float = 1.0, tau: float = 0.07, symmetric: bool = True,
                 lam_mmd: float = 10.0, sigma2: float = 0.25, keep_grads: bool = False):
    """One WAE Stage II / III step (train_wae_stage{2,3}.py; penalty "mmd": tests/mmd_oracle.wae_mmd_step's variant
    without the latent-discriminator phase) with l_con = weight * L(mu_cog, mu_teacher) added to the encoder loss.
    Stage III freezes the cognitive encoder: l_con is logged only, like the penalty (:344)."""
    assert stage in (2, 3) and penalty in ("gan", "mmd")
    gan = penalty == "gan"
    dis_k = param_keys(wae_discriminator_spec(cfg))
    l_fake = l_real = torch.zeros(())
    g_dis = []
    if stage == 2:
        enc_k = param_keys(cognitive_encoder_spec(cfg, n_voxels))
        with torch.no_grad():
            z_t, _ = encoder_fwd(P, "teacher_net.encoder.", x, cfg)           # :284
            decoder_fwd(P, "decoder.", z_t, cfg)                                # :285 x_gt: BN side effects only
            z_fake, _ = cognitive_encoder_fwd(P, "encoder.", fmri)              # :292
            z_real, _ = encoder_fwd(P, "teacher_net.encoder.", x, cfg)        # :293
        if gan:
            l_fake, l_real, g_dis = _wae_dis_phase(P, opts["discriminator"], z_real, z_fake, dis_k, 10.0)
        _leafify(P, enc_k)
        z, _ = cognitive_encoder_fwd(P, "encoder.", fmri)                       # :314
        x_recon = decoder_fwd(P, "decoder.", z, cfg)
        l_rec = F.mse_loss(x_recon, x)                                          # :320
        if gan:
            l_pen = -10 * torch.mean(torch.log(wae_discriminator_fwd(P, "discriminator.", z) + 1e-3))     # :321
        else:
            l_pen = (lam_mmd * MO.mmd_u(z, z_t, sigma2)).float()
        l_con = (weight * nce_loss(z, z_t, tau, symmetric)).float()
        g = _gsum(_gsum(_grads(l_rec, P, enc_k, True), _grads(l_pen, P, enc_k, True)), _grads(l_con, P, enc_k, False))
        opt_step(P, enc_k, g, opts["encoder"])
        _done(P, enc_k)
        grads = {**dict(zip(dis_k, g_dis)), **dict(zip(enc_k, g))}
    else:
        dec_k = param_keys(decoder_spec(cfg))
        with torch.no_grad():
            z_fake, _ = cognitive_encoder_fwd(P, "encoder.", fmri)              # :311
            z_t, _ = encoder_fwd(P, "teacher_net.encoder.", x, cfg)           # :312
        if gan:
            l_fake, l_real, g_dis = _wae_dis_phase(P, opts["discriminator"], z_t, z_fake, dis_k, 10.0)
        _leafify(P, dec_k)
        with torch.no_grad():
            z, _ = cognitive_encoder_fwd(P, "encoder.", fmri)                   # :333
            if gan:
                l_pen = -10 * torch.mean(torch.log(wae_discriminator_fwd(P, "discriminator.", z) + 1e-3))  # :340
            else:
                l_pen = (lam_mmd * MO.mmd_u(z, z_t, sigma2)).float()
            l_con = (weight * nce_loss(z, z_t, tau, symmetric)).float()         # logged only
        x_recon = decoder_fwd(P, "decoder.", z, cfg)
        l_rec = F.mse_loss(x_recon, x)                                          # :339
        g = _grads(l_rec, P, dec_k, False)
        opt_step(P, dec_k, g, opts["decoder"])
        _done(P, dec_k)
        grads = {**dict(zip(dis_k, g_dis)), **dict(zip(dec_k, g))}
    logs = dict(loss_reconstruction=l_rec.item(), loss_penalty=l_pen.item(), loss_discriminator_fake=l_fake.item(),
                loss_discriminator_real=l_real.item(), loss_contrast=l_con.item())
    out = dict(logs=logs, fw=dict(x_recon=x_recon.detach(), z_real=z.detach(), z_teacher=z_t.detach()))
    if keep_grads:
        out["grads"] = grads
        if gan:
            out["grad_terms"] = dict(_wae_dis_phase.last_terms)
    return out
