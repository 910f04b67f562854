"""TEST INFRASTRUCTURE ONLY -- numpy float64 restatement of the kernels between encoder and decoder and of the fused WAE
latent discriminator (csrc/loss.hip fmri_latent_fwd / fmri_latent_bwd, csrc/mlp.hip fmri_mlp_fwd / fmri_mlp_bwd), the
error bounds their outputs are held to, and the seeded inputs tests/test_latent_oracle_host.py and
tests/test_latent_path_gpu.py share.  Nothing here imports the library under test.

Latent kernels: the formulas of the comments in csrc/loss.hip
    z = eps * exp(0.5 logvar) + mu (sample) or mu, padding columns [Z, zp) zero;  kl_row = -0.5 sum(-exp(lv) - mu^2 + lv + 1)
    dhead = [ g + w mu | g eps 0.5 exp(0.5 lv) + w 0.5 (exp(lv) - 1) ],  g = dz * dz_unscale, w = kl_w * kl_dev

Fused MLP: one function per layer.  Each takes the inputs that layer of the kernel read -- the fp16 tensors the GPU
stored, widened exactly to float64 -- and returns the unrounded float64 result ``p`` and, per output element, the sum of
absolute values ``S = sum_k |w_k x_k| (+ |b|)`` of the terms it adds.  Because every layer is given the kernel's own
inputs (teacher forcing), the error of one layer never reaches the next, and the ReLU masks of the backward are the
kernel's own: no element has to be excluded from a comparison.

Bounds (u = 2^-24, K the reduction length; derived, not measured): the worst-case error of an fp32 sum of K terms in any
order is A = K u S.
    stored as fp16 (hs, delta):  |got - p| <= A + 2^-11 (|p| + A) + 2^-25      accumulation, half an fp16 ulp at the value,
                                                                               half the fp16 subnormal spacing
    stored as fp32 (logit, dz):  |got - p| <= A + u |p|
    delta4 (one product):        |got - p| <= u |p| + 2^-11 |p| + 2^-25
    dbias (M rows, atomics):     |got - p| <= (M + 1) u (inv_scale sum_rows |delta| + |prior|)
For a ReLU output p is max(p, 0): a pre-activation within A of zero may come out as 0 or as the small positive value, and
the bound covers both.
"""
import numpy as np

U = 2.0 ** -24
H16 = 2.0 ** -11            # half an fp16 ulp, relative
SUB16 = 2.0 ** -25          # half the spacing of the fp16 subnormals


def f64(x):
    """Exact widening of a numpy array / torch tensor (any device) / scalar to a float64 numpy array."""
    if hasattr(x, "detach"):
        x = x.detach().cpu()
        x = x.double().numpy() if x.is_floating_point() else x.numpy()
    return np.asarray(x, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# latent kernels
# ---------------------------------------------------------------------------------------------------------------------
def latent_fwd64(head, eps, Z, zp, sample):
    """head [B][2Z] (mu | logvar), eps [B][Z] (ignored when sample == 0) -> z [B][zp], kl_rows [B], kl_total."""
    head = f64(head)
    B = head.shape[0]
    mu, lv = head[:, :Z], head[:, Z:2 * Z]
    z = np.zeros((B, zp))
    z[:, :Z] = f64(eps) * np.exp(0.5 * lv) + mu if sample else mu
    kl_rows = -0.5 * np.sum(-np.exp(lv) - mu * mu + lv + 1.0, axis=1)
    return z, kl_rows, float(kl_rows.sum())


def latent_bwd64(head, eps, dz, ldz, dz_unscale, kl_w, kl_dev, out_scale, sample):
    """dz: [B][ldz] (columns [0, Z) are read) or None; kl_dev: a number or None (-> 1).  Returns dhead [B][2Z] and
    dhead * out_scale (what the fp16 output holds)."""
    head = f64(head)
    B, Z = head.shape[0], head.shape[1] // 2
    mu, lv = head[:, :Z], head[:, Z:]
    if dz is None:
        g = np.zeros((B, Z))
    else:
        dz = f64(dz).reshape(B, ldz)
        g = dz[:, :Z] * dz_unscale
    w = kl_w * (1.0 if kl_dev is None else float(kl_dev))
    dmu = g + w * mu
    dlv = w * 0.5 * (np.exp(lv) - 1.0)
    if sample:
        dlv = dlv + g * f64(eps) * 0.5 * np.exp(0.5 * lv)
    dhead = np.concatenate([dmu, dlv], axis=1)
    return dhead, dhead * out_scale


def close_ratio(got, ref, tol):
    """max err / bound under the project's bound for these outputs (tests/test_kernels_gpu.py::_close):
    tol * RMS(ref) + tol * |ref|."""
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), "non-finite result"
    rms = np.sqrt(np.mean(ref * ref)) + 1e-12
    return float(np.max(np.abs(got - ref) / (tol * rms + tol * np.abs(ref)))) if got.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# fused MLP, one layer at a time
# ---------------------------------------------------------------------------------------------------------------------
def mlp_layer64(x16, W16, b32, relu):
    """x [M][K], W [N][K] (row = output feature), b [N] or None -> p [M][N] (after the ReLU if ``relu``), S [M][N]."""
    x, W = f64(x16), f64(W16)
    p = x @ W.T
    S = np.abs(x) @ np.abs(W).T
    if b32 is not None:
        b = f64(b32).reshape(1, -1)
        p, S = p + b, S + np.abs(b)
    if relu:
        p = np.maximum(p, 0.0)
    return p, S


def mlp_delta4_64(dlogit16, w4row16, h4_16):
    """delta4 = dlogit * W4[0] where h4 > 0: dlogit [M], w4row [H], h4 [M][H] -> p, S (one product per element)."""
    p = f64(dlogit16).reshape(-1, 1) * f64(w4row16).reshape(1, -1) * (f64(h4_16) > 0)
    return p, np.abs(p)


def mlp_delta_64(delta_next16, Wd16, h16):
    """delta_L = (delta_{L+1} . W) where h_L > 0.  delta_next [M][N]; Wd [K][N] in the data-gradient orientation (row =
    input feature of the layer, the matrix the kernel reads); h [M][K] the kernel's stored activation."""
    d, Wd = f64(delta_next16), f64(Wd16)
    mask = f64(h16) > 0
    return (d @ Wd.T) * mask, (np.abs(d) @ np.abs(Wd).T) * mask


def mlp_dz64(delta1_16, W0_16, inv_scale):
    """dz = inv_scale * (delta1 . W0).  delta1 [M][H]; W0 [Z][H] in the data-gradient orientation (row = z feature)."""
    d, W = f64(delta1_16), f64(W0_16)
    return (d @ W.T) * inv_scale, (np.abs(d) @ np.abs(W).T) * abs(inv_scale)


def mlp_dbias64(delta16, inv_scale, prior):
    """dbias = prior + inv_scale * column sums of delta [M][N] (or [M] for the output layer) -> p [N], S [N]."""
    d = f64(delta16)
    d = d.reshape(d.shape[0], -1)
    pr = f64(prior).reshape(-1)
    return pr + inv_scale * d.sum(0), abs(inv_scale) * np.abs(d).sum(0) + np.abs(pr)


# ---- bounds ---------------------------------------------------------------------------------------------------------
def bound_f16(p, S, K):
    A = K * U * S
    return A + H16 * (np.abs(p) + A) + SUB16


def bound_f32(p, S, K):
    return K * U * S + U * np.abs(p)


def bound_delta4(p):
    return U * np.abs(p) + H16 * np.abs(p) + SUB16


def bound_dbias(S, M):
    return (M + 1) * U * S


def ratio(got, p, bound):
    """max err / bound over EVERY element (0 / 0 counts as 0, an error on a zero bound as inf)."""
    got, p, bound = f64(got), f64(p), f64(bound)
    assert got.shape == p.shape == bound.shape, (got.shape, p.shape, bound.shape)
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - p)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def l2_ratio(got, ref):
    """The whole-tensor measure of tests/test_wae_gpu.py::_terr: |got - ref|_2 / |ref|_2."""
    got, ref = f64(got).reshape(-1), f64(ref).reshape(-1)
    return float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-20))


def mlp_ratios(out, z16, Wf, bs, Wd, dl16, inv_scale, Z, priors):
    """Every output of one forward (+ backward) pass against the per-layer references, teacher-forced on ``out`` itself.
    out: dict with "hs" (4 x [M][H] fp16), "logit" [M] fp32 and optionally "delta" (4 x [M][H] fp16), "dz" ([M][Z] fp32
    or None), "dbias" (5 fp32 vectors, entries may be None).  Wf[i]: forward-orientation fp16 matrices [N][K] the kernel
    read (Wf[4]: row 0 is the output layer), bs[i]: fp32 biases or None, Wd[i]: data-gradient-orientation matrices
    [K][N] (Wd[0] may be None without dz), priors[i]: what dbias[i] held before the launch.
    Returns {quantity: max err / bound}."""
    r = {}
    M = f64(z16).shape[0]
    x = z16
    for L in range(4):
        p, S = mlp_layer64(x, Wf[L], bs[L], True)
        r[f"hs[{L}]"] = ratio(out["hs"][L], p, bound_f16(p, S, f64(x).shape[1]))
        x = out["hs"][L]
    p, S = mlp_layer64(x, f64(Wf[4])[:1], bs[4], False)
    r["logit"] = ratio(f64(out["logit"]).reshape(M, 1), p, bound_f32(p, S, f64(x).shape[1]))
    if out.get("delta") is None:
        return r
    delta = out["delta"]
    p, _ = mlp_delta4_64(dl16, f64(Wf[4])[0], out["hs"][3])
    r["delta[3]"] = ratio(delta[3], p, bound_delta4(p))
    for L in (3, 2, 1):
        p, S = mlp_delta_64(delta[L], Wd[L], out["hs"][L - 1])
        r[f"delta[{L - 1}]"] = ratio(delta[L - 1], p, bound_f16(p, S, f64(delta[L]).shape[1]))
    if out.get("dz") is not None:
        p, S = mlp_dz64(delta[0], f64(Wd[0])[:Z], inv_scale)
        r["dz"] = ratio(out["dz"], p, bound_f32(p, S, f64(delta[0]).shape[1]))
    if out.get("dbias") is not None:
        for i in range(5):
            if out["dbias"][i] is None:
                continue
            p, S = mlp_dbias64(delta[i] if i < 4 else f64(dl16).reshape(M, 1), inv_scale, priors[i])
            r[f"dbias[{i}]"] = ratio(f64(out["dbias"][i]).reshape(-1), p, bound_dbias(S, M))
    return r


# ---------------------------------------------------------------------------------------------------------------------
# seeded inputs shared by the host and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
LATENT_B = (1, 3, 256, 259)
LATENT_ZS = ((128, 128), (512, 512), (100, 104), (100, 128), (8, 8))
MLP_SHAPES = [(M, 128) for M in (1, 31, 32, 33, 77, 512)] + [(M, Z) for Z in (64, 192, 256) for M in (33, 512)]
MLP_FWD_ONLY = [(33, 320), (77, 512)]          # widths only the forward launch accepts


def latent_inputs(B, Z, seed, edges=True):
    """head [B][2Z] fp32 (mu | logvar), eps [B][Z] fp32, dz [B][Z] fp32.  mu, logvar ~ N(0, 0.5), eps ~ N(0, 1); with
    ``edges`` a few entries of mu at +-8, of logvar at -30, 0 and +20 and of eps at 0 and +-4.  Where logvar = 20,
    sigma = e^10 = 22026: eps is kept within +-2.5 and dz within +-3 there so that z and the fp16 gradient stay inside
    fp16's range (65504)."""
    rs = np.random.RandomState(seed)
    mu = rs.randn(B, Z) * 0.5
    lv = rs.randn(B, Z) * 0.5
    eps = rs.randn(B, Z)
    dz = rs.randn(B, Z)
    if edges:
        n = B * Z
        flat = lambda a: a.reshape(-1)
        flat(mu)[0::37] = 8.0
        flat(mu)[5::41] = -8.0
        flat(eps)[3::29] = 0.0
        flat(eps)[7::43] = 4.0
        flat(eps)[11::47] = -4.0
        flat(lv)[1::31] = -30.0
        flat(lv)[2::53] = 0.0
        hot = np.arange(4, n, 59)
        flat(lv)[hot] = 20.0
        flat(eps)[hot] = np.clip(flat(eps)[hot], -2.5, 2.5)
        flat(dz)[hot] = np.clip(flat(dz)[hot], -3.0, 3.0)
    head = np.concatenate([mu, lv], axis=1).astype(np.float32)
    return head, eps.astype(np.float32), dz.astype(np.float32)


def mlp_params(Z, seed=3, H=512):
    """State dict of the latent discriminator (reference key names): weights N(0, 2 / fan_in) so that activations and
    cotangents keep their magnitude through the layers (well inside fp16's normal range), biases N(0, 0.05) -- the
    reference initialises them to zero, which would leave the bias path untested."""
    rs = np.random.RandomState(seed)
    dims = [Z, H, H, H, H, 1]
    sd = {}
    for j, idx in enumerate((0, 2, 4, 6, 8)):
        sd[f"main.{idx}.weight"] = (rs.randn(dims[j + 1], dims[j]) * np.sqrt(2.0 / dims[j])).astype(np.float32)
        sd[f"main.{idx}.bias"] = (rs.randn(dims[j + 1]) * 0.05).astype(np.float32)
    return sd


def mlp_inputs(M, Z, Zp, seed):
    """z16 [M][Zp] fp16 (~ N(0, 1), columns [Z, Zp) zero, a few all-zero rows), dlogit16 [M] fp16 (~ N(0, 0.5)) and
    nonzero priors for the five bias gradients."""
    rs = np.random.RandomState(seed)
    z = np.zeros((M, Zp), np.float32)
    z[:, :Z] = rs.randn(M, Z)
    for r in (M // 2, 32):
        if 0 < r < M:
            z[r] = 0.0
    dl = (rs.randn(M) * 0.5).astype(np.float16)
    priors = [(rs.randn(512 if i < 4 else 1) * 0.3).astype(np.float32) for i in range(5)]
    return z.astype(np.float16), dl, priors
