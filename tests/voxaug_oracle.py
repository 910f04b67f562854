"""numpy float64 restatement of the fMRI-row augmentation (include/fmri_hip.h fmri_voxaug_apply; csrc/voxaug.hip), built on
the generator's restatement (tests/rng_oracle.py): the per-row table, the dropout mask, the span, the noise, y64 and the
per-element error bound of a device result against y64.  Not a test: tests/test_voxaug_oracle_host.py checks it against
itself, tests/test_voxaug_kernels_gpu.py the kernels against it.

    y[b][c] = 0                                            if s_b <= c < s_b + L_b, or dropped(b, c)
            = k_b * (sigma_b * n[r][c] + g_b * x[b][c])    otherwise                     r = row0 + b

The bound (``bound``).  Against y64 evaluated with the table's own fp32 k (computed once, by the parameter kernel), a
device value differs by
  * the normals: the device evaluates Box-Muller in fp32, within 1e-5 of the float64 map (the bound derived in
    tests/test_rng_gpu.py).  n enters as sigma * n, and g = 1 + gain * z0 as g * x:      1e-5 * (sigma + gain * |x|);
  * three fp32 roundings -- the product g x, the fma, the product with k -- of relative size 2^-24 each on a value no
    larger than |g x| + sigma |n|; 4 instead of 3 covers the second-order terms:        4 * 2^-24 * (|g x| + sigma |n|);
  * both scaled by k;
  * the ONE rounding to fp16: half an fp16 ulp of |y64| (2^-25 in the subnormal range, below 2^-14).
"""
import numpy as np

import rng_oracle as R

SID_VNOISE, SID_VDROP, SID_VROW = 14, 15, 17
NEUTRAL = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0])
NORMAL_TOL = 1e-5
TWO32 = 2.0 ** 32


def threshold(q) -> int:
    """(uint32)((double)q * 2^32) of the fp32 value q in [0, 1)."""
    return int(float(np.float32(q)) * TWO32)


def span_len(V: int, span: float) -> int:
    return int(V * span + 0.5)


def row_words(seed, offset, B, row0):
    """uint64 [B, 4]: the words of block row0 + b of the row stream."""
    w, _, _ = R.words(seed, offset, 4 * int(row0), 4 * B, SID_VROW)
    return w


def table(seed, offset, B, V, row0=0, noise=0.1, dropout=0.1, span=0.0, gain=0.0, prob=1.0, rescale=True):
    """float64 [B, 8] rows [g, sigma, p, k, s, L, 0, 0] and the bool [B] apply decisions.  sigma, p, k are the fp32
    values the kernel stores (k = fl32(1 / fl32(1 - p)): two correctly rounded fp32 operations), s and L integers; g is
    the float64 value of 1 + gain * z0."""
    w = row_words(seed, offset, B, row0)
    L = span_len(V, span)
    f32 = np.float32
    p32 = f32(dropout)
    k32 = f32(1.0) / (f32(1.0) - p32) if rescale else f32(1.0)
    applied = np.ones(B, bool) if prob >= 1.0 else w[:, 3] < np.uint64(threshold(prob))
    u = R.uniform(w)
    z0 = np.sqrt(-2.0 * np.log(u[:, 0])) * np.cos(2.0 * np.pi * u[:, 1])
    t = np.tile(NEUTRAL, (B, 1))
    rows = np.zeros((B, 8))
    rows[:, 0] = 1.0 + float(f32(gain)) * z0
    rows[:, 1] = float(f32(noise))
    rows[:, 2] = float(p32)
    rows[:, 3] = float(k32)
    rows[:, 4] = ((w[:, 2] * np.uint64(V - L + 1)) >> np.uint64(32)).astype(np.float64)
    rows[:, 5] = L
    t[applied] = rows[applied]
    return t, applied


def noise(seed, offset, B, V, row0=0):
    """float64 [B, V]: n[r][c], fmri_rng_normal's layout with cols = V."""
    return R.normal(seed, offset, B, V, row0=row0, sid=SID_VNOISE)


def drop_words(seed, offset, B, V, row0=0):
    """uint64 [B, V]: word r V + c of the dropout stream."""
    w, bi, wi = R.words(seed, offset, int(row0) * V, B * V, SID_VDROP)
    return w[bi, wi].reshape(B, V)


def drop_mask(seed, offset, B, V, row0, tab):
    """bool [B, V]: dropped(b, c) under the p column of ``tab`` -- an integer comparison."""
    thr = np.array([threshold(p) for p in tab[:, 2]], dtype=np.uint64)
    return drop_words(seed, offset, B, V, row0) < thr[:, None]


def span_mask(tab, V):
    c = np.arange(V)[None, :]
    s, L = tab[:, 4:5], tab[:, 5:6]
    return (c >= s) & (c < s + L)


def y64(x, tab, n, zero):
    """float64 [B, V] of x (float64 of the fp32 input) under the table, noise n and the zero mask (span | dropped)."""
    g, sigma, k = tab[:, 0:1], tab[:, 1:2], tab[:, 3:4]
    return np.where(zero, 0.0, k * (sigma * n + g * x))


def half_ulp16(y):
    """Half an fp16 ulp at |y|: 2^(e - 11) with e = floor(log2 |y|), at least the subnormal range's 2^-25."""
    a = np.abs(y)
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (np.maximum(e, -14.0) - 11.0)


def bound(x, tab, n, y, gain):
    """Per-element bound on |device fp16 value - y64| (module docstring)."""
    g, sigma, k = tab[:, 0:1], tab[:, 1:2], tab[:, 3:4]
    return (k * (NORMAL_TOL * (sigma + gain * np.abs(x)) + 4 * 2.0 ** -24 * (np.abs(g * x) + sigma * np.abs(n)))
            + half_ulp16(y))


def apply32(x32, tab, n, zero):
    """The formula in the kernel's own arithmetic, as far as numpy has it: fp32 product, fma (exact product and sum in
    float64 -- a 48-bit product --, rounded to fp32), fp32 product with k, the cast to fp16.  ``n`` and g are rounded to
    fp32 first."""
    f32 = np.float32
    g, sigma, k = (tab[:, i:i + 1].astype(f32) for i in (0, 1, 3))
    t = g * x32.astype(f32)
    fma = sigma.astype(np.float64) * n.astype(f32).astype(np.float64) + t.astype(np.float64)
    t = np.where(sigma != 0, fma.astype(f32), t)
    return np.where(zero, f32(0), t * k).astype(np.float16)
