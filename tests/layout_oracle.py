"""Plain numpy float64 restatement of the weight-layout maps and of the RMSprop update documented in include/fmri_hip.h
(fmri_pack_weight, fmri_unpack_grad, fmri_rmsprop_dev) -- the reference of tests/test_layout_update_gpu.py.

Nothing here calls the library under test.  A layout map is any object with the fields of ``fmri_hip.ops.PackSpec``
(sa, sta, A, TA, sb, stb, B, KW, py, px, step, TH, TW); ``Spec`` below is such an object, so the tables of the tests can
be written without importing the engine.  tests/test_layout_oracle_host.py checks these functions against torch
permute / reshape / slicing restatements of the same weights, so that they are not merely the kernels' formula again.
"""
from collections import namedtuple

import numpy as np

_Spec = namedtuple("Spec", "sa sta A TA sb stb B KW py px step TH TW")


def Spec(sa, sta, A, TA, sb, stb, B, KW=1, py=0, px=0, step=1, TH=1, TW=1):
    return _Spec(sa, sta, A, TA, sb, stb, B, KW, py, px, step, TH, TW)


def pad8(c):
    return (c + 7) // 8 * 8


def taps(spec):
    """t(tb) = (py + step * ty) * KW + (px + step * tx) for tb = ty * TW + tx."""
    ty, tx = np.divmod(np.arange(spec.TH * spec.TW, dtype=np.int64), spec.TW)
    return (spec.py + spec.step * ty) * spec.KW + (spec.px + spec.step * tx)


def ref_index(spec):
    """int64 [TA * A][taps][B]: reference-layout offset of packed element (row = ta * A + a, tap tb, channel b)."""
    ta = np.arange(spec.TA, dtype=np.int64)[:, None, None, None]
    a = np.arange(spec.A, dtype=np.int64)[None, :, None, None]
    t = taps(spec)[None, None, :, None]
    b = np.arange(spec.B, dtype=np.int64)[None, None, None, :]
    idx = a * spec.sa + ta * spec.sta + b * spec.sb + t * spec.stb
    return idx.reshape(spec.TA * spec.A, spec.TH * spec.TW, spec.B)


def extent(spec):
    """Elements of the smallest reference tensor the map stays inside."""
    return int(ref_index(spec).max()) + 1


def touched(spec, n):
    """bool [n]: the reference-layout elements the map reaches."""
    m = np.zeros(n, dtype=bool)
    m[ref_index(spec).ravel()] = True
    return m


def pack_ref(src, spec, rows_pad, kpad):
    """float64 [rows_pad][kpad]: dst[ta * A + a][tb * Bp + b] = src[a sa + ta sta + b sb + t(tb) stb], zero padded."""
    rows, nt, bp = spec.TA * spec.A, spec.TH * spec.TW, pad8(spec.B)
    assert rows_pad >= rows and kpad >= nt * bp
    vals = np.asarray(src, dtype=np.float64).ravel()[ref_index(spec)]
    out = np.zeros((rows_pad, kpad), dtype=np.float64)
    out[:rows, :nt * bp].reshape(rows, nt, bp)[:, :, :spec.B] = vals
    return out


def valid_mask(spec, rows_pad, kpad):
    """bool [rows_pad][kpad]: the packed elements that carry a weight (everything else is padding)."""
    return pack_ref(np.ones(extent(spec)), spec, rows_pad, kpad) != 0.0


def unpack_ref(slabs, spec, ld, scale, into=None):
    """The inverse map with the slab sum: flat float64 reference tensor with
    dst[a sa + ta sta + b sb + t(tb) stb] = (into or 0) + scale * sum_z slabs[z][ta * A + a][tb * Bp + b].
    ``slabs``: [nslabs][>= rows][ld] (or [rows][ld]); ``into`` (flat, any float type) also fixes the length of the
    result, ``extent(spec)`` without it.  Elements the map does not reach keep ``into``'s value (0 without it)."""
    s = np.asarray(slabs, dtype=np.float64)
    if s.ndim == 2:
        s = s[None]
    rows, nt, bp = spec.TA * spec.A, spec.TH * spec.TW, pad8(spec.B)
    assert s.shape[2] == ld and ld >= nt * bp and s.shape[1] >= rows
    total = s.sum(axis=0)[:rows, :nt * bp].reshape(rows, nt, bp)[:, :, :spec.B]
    idx = ref_index(spec)
    assert np.unique(idx).size == idx.size, "two packed elements share one reference element"
    out = np.zeros(extent(spec)) if into is None else np.asarray(into, dtype=np.float64).ravel().copy()
    out[idx.ravel()] += (float(scale) * total).ravel()
    return out


def rmsprop_ref(w, sq, g, lr, alpha, eps, gscale=1.0, gdev=1.0, clamp=0.0):
    """One step of torch.optim.RMSprop (no momentum, not centred) in float64 on the true gradient g * gscale / gdev,
    clamped to +-clamp when clamp > 0; ``lr`` and ``alpha`` are the fp32 numbers the kernel receives.
    Returns (new w, new sq)."""
    lr, alpha = float(np.float32(lr)), float(np.float32(alpha))
    w, sq = np.asarray(w, dtype=np.float64), np.asarray(sq, dtype=np.float64)
    gg = np.asarray(g, dtype=np.float64) * float(gscale) / float(gdev)
    if clamp > 0:
        gg = np.clip(gg, -clamp, clamp)
    s = alpha * sq + (1.0 - alpha) * gg * gg
    return w - lr * gg / (np.sqrt(s) + eps), s
