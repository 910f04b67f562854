"""float64 restatement of the differentiable augmentation (csrc/diffaug.hip; include/fmri_hip.h fmri_diffaug_fwd): the
transform T_p, the adjoint of its linear part, the decoding of a parameter row from Philox words, and a torch version of T
that autograd can differentiate (the step tests put it in front of the CPU oracle's discriminator).
Not a test: tests/test_diffaug_oracle_host.py checks it against itself (adjoint identity, autograd), the GPU tests check
the kernels against it.

A row is p = [b, s, c, ty, tx, cy, cx, cut]; an image here is [H, W, 3] (the real channels of the engine's NHWC8)."""
import numpy as np

import rng_oracle

SID_DAUG, SID_DAUG_P = 12, 13
NEUTRAL = np.array([0, 1, 1, 0, 0, 0, 0, 0], np.float64)
COLOR, TRANSLATION, CUTOUT = 1, 2, 4


def sizes(H, translation=0.125, cutout=0.5):
    return int(np.floor(H * translation + 0.5)), int(np.floor(H * cutout + 0.5))


def decode(w, H, sh, cut, policy=7):
    """uint64 [n, 8] Philox words -> float64 [n, 8] rows holding fp32 values.  Every value is exact in fp32 but c at
    u + 0.5 >= 1, where fp32 has 23 fraction bits for the 24 of u: c is the fp32 sum, rounded to nearest even, as the
    device adds it."""
    w = np.asarray(w, dtype=np.uint64)
    u = lambda x: (x >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    mulhi = lambda x, span: ((x * np.uint64(span)) >> np.uint64(32)).astype(np.float64)
    p = np.tile(NEUTRAL, (w.shape[0], 1))
    if policy & COLOR:
        p[:, 0] = u(w[:, 0]) - 0.5
        p[:, 1] = 2.0 * u(w[:, 1])
        p[:, 2] = (u(w[:, 2]).astype(np.float32) + np.float32(0.5)).astype(np.float64)
    if policy & TRANSLATION:
        p[:, 3] = mulhi(w[:, 3], 2 * sh + 1) - sh
        p[:, 4] = mulhi(w[:, 4], 2 * sh + 1) - sh
    if policy & CUTOUT:
        p[:, 5] = mulhi(w[:, 5], H - cut % 2 + 1)
        p[:, 6] = mulhi(w[:, 6], H - cut % 2 + 1)
        p[:, 7] = cut
    return p


def table_rows(seed, offset, rows, row0, sid, H, sh, cut, policy=7):
    """Rows row0 .. row0 + rows of stream ``sid``: row r takes elements 8 r .. 8 r + 7 of the stream."""
    w, bi, wi = rng_oracle.words(seed, offset, 8 * int(row0), 8 * int(rows), sid)
    return decode(w[bi, wi].reshape(rows, 8), H, sh, cut, policy)


def step_table(seed, offset, B, H, row0=0, translation=0.125, cutout=0.5, policy=7):
    """The [2B, 8] table of a step: SID_DAUG rows for [orig | pred], SID_DAUG_P rows for sampled."""
    sh, cut = sizes(H, translation, cutout)
    return np.concatenate([table_rows(seed, offset, B, row0, SID_DAUG, H, sh, cut, policy),
                           table_rows(seed, offset, B, row0, SID_DAUG_P, H, sh, cut, policy)])


def row_of(img, B):
    """Image ``img`` of the [orig | pred | sampled] layout -> its table row."""
    return img if img < B else img - B


def _window(c, cut, H):
    """Boolean [H]: the clamped cutout rows (or columns) around centre c."""
    m = np.zeros(H, bool)
    if cut > 0:
        m[np.clip(c - cut // 2 + np.arange(cut), 0, H - 1)] = True
    return m


def _keep(p, H):
    """float64 [H, H]: 0 inside the cutout window, 1 outside."""
    cy, cx, cut = int(p[5]), int(p[6]), int(p[7])
    return 1.0 - np.outer(_window(cy, cut, H), _window(cx, cut, H)).astype(np.float64)


def _shift(a, ty, tx, fill=0.0):
    """o[y, x] = a[y + ty, x + tx] inside the image, else ``fill``."""
    H, W = a.shape[:2]
    o = np.full_like(a, fill)
    ys, xs = np.arange(H), np.arange(W)
    vy, vx = (ys + ty >= 0) & (ys + ty < H), (xs + tx >= 0) & (xs + tx < W)
    o[np.ix_(ys[vy], xs[vx])] = a[np.ix_(ys[vy] + ty, xs[vx] + tx)]
    return o


def transform(x, p):
    """T_p of one image, float64 [H, W, 3] -> float64 (not yet rounded).  A neutral stage is skipped."""
    x = np.asarray(x, np.float64)
    b, s, c = float(p[0]), float(p[1]), float(p[2])
    ty, tx = int(p[3]), int(p[4])
    H = x.shape[0]
    v = x + b if b != 0 else x
    if s != 1:
        m = v.mean(axis=2, keepdims=True)
        v = (v - m) * s + m
    if c != 1:
        M = v.mean()
        v = (v - M) * c + M
    return _shift(v, ty, tx) * _keep(p, H)[:, :, None]


def adjoint(g, p):
    """The adjoint of T_p's linear part on one cotangent image, float64 [H, W, 3] -> float64 (not yet saturated)."""
    g = np.asarray(g, np.float64)
    s, c = float(p[1]), float(p[2])
    ty, tx = int(p[3]), int(p[4])
    H = g.shape[0]
    g1 = _shift(g * _keep(p, H)[:, :, None], -ty, -tx)
    g2 = c * g1 + (1.0 - c) * g1.mean() if c != 1 else g1
    return s * g2 + (1.0 - s) * g2.mean(axis=2, keepdims=True) if s != 1 else g2


def _batch(fn, x16, table, B, img0, post):
    x16 = np.asarray(x16)
    out = np.zeros(x16.shape, np.float16)
    for i in range(x16.shape[0]):
        r = fn(x16[i, :, :, :3].astype(np.float64), table[row_of(img0 + i, B)])
        out[i, :, :, :3] = post(r).astype(np.float16)
    return out


def forward16(x16, table, B, img0=0):
    """fp16 [N, H, W, 8] -> what fmri_diffaug_fwd must store, up to the stated ulp: the float64 result rounded to fp16,
    lanes 3..7 zero."""
    return _batch(transform, x16, table, B, img0, lambda r: r)


def adjoint16(g16, table, B, img0):
    """fp16 [N, H, W, 8] cotangent of images img0 .. -> what fmri_diffaug_bwd must store: saturated at +-65504."""
    return _batch(adjoint, g16, table, B, img0, lambda r: np.clip(r, -65504.0, 65504.0))


def ulp16(ref16):
    """Spacing of fp16 at |ref| (float64 array): 2^(e - 10) for normal values, 2^-24 below the normal range."""
    a = np.abs(np.asarray(ref16, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (np.minimum(e, 15) - 10)


# ---- torch restatement (autograd) -----------------------------------------------------------------------------------
def torch_transform(x, rows):
    """T of a batch: x torch [n, 3, H, W] (any float dtype, may require grad), rows float [n, 8] -> [n, 3, H, W]."""
    import torch
    n, _, H, W = x.shape
    outs = []
    for i in range(n):
        p = [float(v) for v in rows[i]]
        b, s, c, ty, tx = p[0], p[1], p[2], int(p[3]), int(p[4])
        v = x[i]
        if b != 0:
            v = v + b
        if s != 1:
            m = v.mean(dim=0, keepdim=True)
            v = (v - m) * s + m
        if c != 1:
            M = v.mean()
            v = (v - M) * c + M
        o = torch.zeros_like(v)
        y0, y1 = max(0, -ty), min(H, H - ty)
        x0, x1 = max(0, -tx), min(W, W - tx)
        if y1 > y0 and x1 > x0:
            o[:, y0:y1, x0:x1] = v[:, y0 + ty:y1 + ty, x0 + tx:x1 + tx]
        outs.append(o * torch.as_tensor(_keep(p, H), dtype=x.dtype)[None])
    return torch.stack(outs)


def torch_transform_3b(x_orig, x_pred, x_samp, table):
    """The three image groups of a step under its [2B, 8] table: orig and pred share rows 0 .. B-1."""
    B = x_orig.shape[0]
    return (torch_transform(x_orig, table[:B]), torch_transform(x_pred, table[:B]),
            torch_transform(x_samp, table[B:2 * B]))
