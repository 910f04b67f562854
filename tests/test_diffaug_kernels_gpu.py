"""The differentiable-augmentation kernels (csrc/diffaug.hip) against the float64 restatement (tests/diffaug_oracle.py):
N = 6 images (B = 2) at H = W in {16, 25, 64, 100, 128} -- even and odd, below and above one 64-lane row pass, one to
eight rows per wave (25 and 100: an uneven share) -- under hand-built and drawn tables.

Bounds.  With the colour stages off the kernels gather and mask: the stored values equal the oracle's.  With colour on the
kernels evaluate the stated formula in fp64 and round to fp32, then to fp16: the result is the fp16 rounding of the
float64 value or, where the two roundings straddle a tie, its neighbour -- every element within 1 fp16 ulp (the spacing
of fp16 at the reference value, 2^-24 below the normal range) of the float64 result rounded to fp16."""
import ctypes

import numpy as np
import pytest
import torch

import diffaug_oracle as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N = 2, 6
SIZES = (16, 25, 64, 100, 128)
SENTINEL = 0x7E00                # an fp16 NaN no kernel output holds


def _hand_rows(H):
    sh, cut = A.sizes(H)
    odd = cut % 2
    rows = [A.NEUTRAL.copy()]
    for ty in (-sh, sh):
        for tx in (-sh, sh):
            rows.append(np.array([0.3, 0.4, 1.4, ty, tx, H // 2, H // 3, cut]))
    for cy, cx in ((0, 0), (H - odd, H - odd), (0, H - odd), (H - odd, 0)):
        rows.append(np.array([-0.2, 1.7, 0.6, 1, -1, cy, cx, cut]))
    rows.append(np.array([0.1, 0.9, 1.1, 0, 0, H // 2, H // 2, H]))              # cut = H: everything
    rows.append(np.array([0.25, 1, 1, 0, 0, 0, 0, 0]))                            # one stage at a time
    rows.append(np.array([0, 0.5, 1, 0, 0, 0, 0, 0]))
    rows.append(np.array([0, 1, 0.75, 0, 0, 0, 0, 0]))
    rows.append(np.array([0, 1, 1, -sh, sh, 0, 0, 0]))                            # translation only
    rows.append(np.array([0, 1, 1, 0, 0, 3, H - 2, cut]))                         # cutout only
    rows.append(np.array([0, 1, 1, sh, -1, H - odd, 0, cut]))                     # gather + mask, colour off
    return [np.asarray(r, np.float64) for r in rows]


def _tables(H):
    """[2B, 8] float64 tables: the hand-built rows four at a time, then drawn ones -- all policies, and one at a time."""
    sh, cut = A.sizes(H)
    rows = _hand_rows(H)
    while len(rows) % (2 * B):
        rows.append(A.NEUTRAL.copy())
    out = [np.stack(rows[i:i + 2 * B]) for i in range(0, len(rows), 2 * B)]
    for k, pol in enumerate((7, A.COLOR, A.TRANSLATION, A.CUTOUT)):
        out.append(A.table_rows(77, 5 + k, 2 * B, 3, A.SID_DAUG, H, sh, cut, pol))
    return [_f32(t) for t in out]


def _f32(t):
    """The table the device holds: fp32 values (0.3 is not one), as float64 for the oracle."""
    return np.asarray(t, np.float64).astype(np.float32).astype(np.float64)


def _images(H, seed, scale=None):
    """fp16 [N, H, H, 8]: uniform [-1, 1] images, or unit-RMS * scale cotangents; lanes 3..7 hold junk that must not
    reach the output."""
    rs = np.random.RandomState(seed)
    x = np.empty((N, H, H, 8), np.float16)
    x[..., 3:] = rs.uniform(-4, 4, (N, H, H, 5)).astype(np.float16)
    real = rs.uniform(-1, 1, (N, H, H, 3)) if scale is None else rs.standard_normal((N, H, H, 3)) * scale
    x[..., :3] = real.astype(np.float16)
    return x


def _dev16(a):
    return torch.from_numpy(a.view(np.int16).copy()).to(DEV).view(torch.float16)


def _host16(t):
    return t.cpu().view(torch.int16).numpy().view(np.float16)


def _sentinel_like(t):
    return torch.full(t.shape, SENTINEL, dtype=torch.int16, device=DEV).view(torch.float16)


def _fwd(x, table):
    from fmri_hip import lib
    out = _sentinel_like(x)
    n, H, W, _ = x.shape
    lib.call("fmri_diffaug_fwd", lib.ptr(x), lib.ptr(out), n, H, W, lib.ptr(table), B, 0)
    return out


def _bwd(ga, gb, table, img0):
    from fmri_hip import lib
    oa, ob = _sentinel_like(ga), (None if gb is None else _sentinel_like(gb))
    n, H, W, _ = ga.shape
    lib.call("fmri_diffaug_bwd", lib.ptr(ga), lib.ptr(oa), lib.ptr(gb), lib.ptr(ob), n, H, W, lib.ptr(table), B, img0)
    return oa, ob


def _table_dev(t64):
    return torch.tensor(t64, dtype=torch.float32, device=DEV).contiguous()


def _check(got16, ref16, table, img0, what):
    """Every element: lanes 3..7 zero, colour-off images equal, colour-on images within 1 fp16 ulp; nothing left out."""
    got, ref = got16.astype(np.float64), ref16.astype(np.float64)
    assert not np.isnan(got).any(), f"{what}: elements left unwritten"
    assert not got[..., 3:].any(), f"{what}: lanes 3..7 not zero"
    worst = 0.0
    for i in range(got.shape[0]):
        p = table[A.row_of(img0 + i, B)]
        g, r = got[i, :, :, :3], ref[i, :, :, :3]
        if p[0] == 0 and p[1] == 1 and p[2] == 1:
            assert np.array_equal(g, r), f"{what}: image {i} (gather / mask only) differs from the oracle"
        else:
            err = np.abs(g - r) / A.ulp16(r)
            worst = max(worst, err.max())
            assert err.max() <= 1.0, (what, i, list(p), err.max(), np.unravel_index(err.argmax(), err.shape))
    return worst


@pytest.fixture(scope="module")
def lib():
    from fmri_hip import lib as L
    L.load()
    return L


@pytest.mark.parametrize("H", SIZES)
def test_forward_matches_the_oracle(lib, H):
    x = _images(H, 10 + H)
    xd = _dev16(x)
    worst = 0.0
    for k, t in enumerate(_tables(H)):
        got = _host16(_fwd(xd, _table_dev(t)))
        worst = max(worst, _check(got, A.forward16(x, t, B), t, 0, f"fwd H={H} table {k}"))
    assert _host16(xd).tobytes() == x.tobytes()                 # the input is not modified
    print(f"fwd H={H}: worst error {worst:.3f} fp16 ulp")


@pytest.mark.parametrize("H", SIZES)
@pytest.mark.parametrize("scale", (16.0, 512.0))
def test_adjoint_matches_the_oracle(lib, H, scale):
    """Cotangents at the magnitudes the two streams carry (unit RMS x 16 and x 512), both streams in one launch over
    images B .. 3B, and one stream over images B .. 2B."""
    ga, gb = _images(H, 20 + H, scale)[B:], _images(H, 30 + H, scale)[B:]
    gad, gbd = _dev16(ga), _dev16(gb)
    worst = 0.0
    for k, t in enumerate(_tables(H)):
        td = _table_dev(t)
        oa, ob = _bwd(gad, gbd, td, B)
        worst = max(worst, _check(_host16(oa), A.adjoint16(ga, t, B, B), t, B, f"bwd A H={H} table {k}"))
        worst = max(worst, _check(_host16(ob), A.adjoint16(gb, t, B, B), t, B, f"bwd B H={H} table {k}"))
        one, _ = _bwd(gbd[:B].contiguous(), None, td, B)
        assert torch.equal(one.view(torch.int16), ob[:B].view(torch.int16))
    assert _host16(gad).tobytes() == ga.tobytes() and _host16(gbd).tobytes() == gb.tobytes()
    print(f"bwd H={H} x{scale:g}: worst error {worst:.3f} fp16 ulp")


@pytest.mark.parametrize("H", (25, 64))
def test_adjoint_saturates(lib, H):
    """Values whose image under L^T leaves fp16's range are stored as +-65504, not inf."""
    sh, cut = A.sizes(H)
    g = _images(H, 40 + H, 512.0)[B:]
    g[0, 1:5, 1:9, :3] = np.float16(60000.0)
    g[1, 2, 3, :3] = np.float16(-65504.0)
    g[2, 4, 5, 1] = np.float16(50000.0)
    t = np.stack([np.array([0.2, 1.9, 1.45, 1, -1, H // 2, H // 2, cut], np.float64)] * (2 * B))
    t[1] = [0, 1, 1.5, 0, 0, 0, 0, 0]
    t[2] = [0, 2.0, 1, -sh, sh, 0, 0, 0]
    t = _f32(t)
    ref = A.adjoint16(g, t, B, B)
    assert (np.abs(ref[..., :3].astype(np.float64)) == 65504.0).sum() >= 40          # the case does saturate
    out, _ = _bwd(_dev16(g), None, _table_dev(t), B)
    got = _host16(out)
    assert np.isfinite(got.astype(np.float64)).all()
    _check(got, ref, t, B, f"saturating bwd H={H}")


@pytest.mark.parametrize("H", SIZES)
def test_adjoint_identity_from_the_device_outputs(lib, H):
    """<T(x) - T(x'), g> = <x - x', L^T g> in float64 on what the kernels stored; each side carries one fp16 rounding
    per element: 2^-10 of the sums of absolute products."""
    x, x2, g = _images(H, 50 + H), _images(H, 60 + H), _images(H, 70 + H, 16.0)
    xd, x2d, gd = _dev16(x), _dev16(x2), _dev16(g)
    f64 = lambda a: a[..., :3].astype(np.float64)
    for k, t in enumerate(_tables(H)):
        td = _table_dev(t)
        tx, tx2 = f64(_host16(_fwd(xd, td))), f64(_host16(_fwd(x2d, td)))
        ltg = np.zeros((N, H, H, 3))
        ltg[B:] = f64(_host16(_bwd(gd[B:].contiguous(), None, td, B)[0]))
        ltg[:B] = f64(_host16(_bwd(gd[:B].contiguous(), None, td, 0)[0]))
        for i in range(N):
            dT, dx, gi = tx[i] - tx2[i], f64(x)[i] - f64(x2)[i], f64(g)[i]
            lhs, rhs = np.sum(dT * gi), np.sum(dx * ltg[i])
            bound = 2.0 ** -10 * (np.sum(np.abs(dT) * np.abs(gi)) + np.sum(np.abs(dx) * np.abs(ltg[i])))
            assert abs(lhs - rhs) <= bound, (H, k, i, lhs, rhs, bound)


@pytest.mark.parametrize("H", (25, 128))
def test_launches_are_deterministic(lib, H):
    x, g = _dev16(_images(H, 80 + H)), _dev16(_images(H, 90 + H, 512.0)[B:])
    td = _table_dev(_tables(H)[-4])                              # drawn, every policy on
    L = lib.load()
    was = L.fmri_get_deterministic()
    bits = []
    try:
        for det in (1, 0, 1):
            L.fmri_set_deterministic(det)
            for _ in range(2):
                oa, ob = _bwd(g, g, td, B)
                bits.append((_fwd(x, td).view(torch.int16).clone(), oa.view(torch.int16).clone(),
                             ob.view(torch.int16).clone()))
    finally:
        L.fmri_set_deterministic(was)
    for b in bits[1:]:
        assert all(torch.equal(p, q) for p, q in zip(b, bits[0]))
    assert torch.equal(bits[0][1], bits[0][2])                   # the two streams of one launch run the same code


def test_parameter_draw_matches_the_philox_oracle(lib):
    from fmri_hip.augment import SID_DAUG, SID_DAUG_P, DiffAugment
    from fmri_hip.rng import DeviceRng
    assert (SID_DAUG, SID_DAUG_P) == (A.SID_DAUG, A.SID_DAUG_P) == (12, 13)
    aug = DiffAugment()
    Bg = 8
    for seed, offset in ((3, 0), (3, (1 << 32) - 5), (2 ** 63 + 11, 12345)):
        rng = DeviceRng(seed, DEV)
        rng.seed(seed, offset)
        for H in (25, 64, 128):
            t = aug.table(rng, Bg, H)
            ref = A.step_table(seed, offset, Bg, H).astype(np.float32)
            assert t.dtype == torch.float32 and tuple(t.shape) == (2 * Bg, 8)
            assert t.cpu().numpy().tobytes() == ref.tobytes(), (seed, offset, H)
            assert not np.array_equal(ref[:Bg], ref[Bg:])       # sampled rows: the other stream
            # rank k of 4 gets rows k * B .. of the draw at the global batch, for both streams
            for k in range(4):
                part = aug.table(rng, 2, H, row0=2 * k).cpu().numpy()
                assert np.array_equal(part[:2], ref[2 * k:2 * k + 2]) and np.array_equal(part[2:], ref[Bg + 2 * k:Bg + 2 * k + 2])
        assert rng.offset() == offset                           # a draw does not move the offset
    rng = DeviceRng(9, DEV)
    for pol, mask in ((("color",), 1), (("translation",), 2), (("cutout",), 4), (("color", "cutout"), 5), ((), 0)):
        t = DiffAugment(policy=pol, translation=0.25, cutout=0.3).table(rng, 4, 25)
        ref = A.step_table(9, 0, 4, 25, translation=0.25, cutout=0.3, policy=mask).astype(np.float32)
        assert t.cpu().numpy().tobytes() == ref.tobytes(), pol
    assert torch.equal(DiffAugment.neutral(3, DEV), torch.tensor(A.NEUTRAL, dtype=torch.float32, device=DEV).repeat(6, 1))


def test_unsupported_shapes_are_refused_and_nothing_is_launched(lib):
    L = lib.load()
    P = lib.ptr
    td = _table_dev(np.tile(A.NEUTRAL, (2 * B, 1)))
    x = _dev16(_images(16, 1))
    out = _sentinel_like(x)
    rect = x.view(N, 8, 32, 8)
    fwd = lambda src, dst, n, h, w, t=td, b=B, i0=0: L.fmri_diffaug_fwd(P(src), P(dst), n, h, w, P(t), b, i0, None)
    bwd = lambda ga, da, gb, db, n, h, w, i0=B: L.fmri_diffaug_bwd(P(ga), P(da), P(gb), P(db), n, h, w, P(td), B, i0,
                                                                   None)
    assert fwd(rect, out, N, 8, 32) == -2                       # H != W
    assert fwd(x, out, N, 129, 129) == -2                       # H > 128
    assert bwd(x, out, None, None, 4, 8, 32) == -2
    assert fwd(x, out, N, 16, 16, i0=1) == -1                   # images outside [0, 3B)
    assert fwd(x, out, 0, 16, 16) == -1
    assert fwd(x, x, N, 16, 16) == -1                           # in place
    assert bwd(x[:4], out[:4], x[:4], None, 4, 16, 16) == -1    # half a second stream
    assert bwd(x[:4], out[:4], x[2:], out[:4], 4, 16, 16) == -1    # two streams into one output
    assert bwd(x[:4], out[:4], None, None, 4, 16, 16, i0=3) == -1
    odd = ctypes.c_void_p(x.data_ptr() + 8)
    assert L.fmri_diffaug_fwd(odd, P(out), 1, 16, 16, P(td), B, 0, None) == -1       # misaligned pointers
    assert L.fmri_diffaug_fwd(P(x), P(out), N, 16, 16, ctypes.c_void_p(td.data_ptr() + 4), B, 0, None) == -1
    assert L.fmri_diffaug_fwd(None, P(out), N, 16, 16, P(td), B, 0, None) == -1
    st = torch.zeros(2, dtype=torch.int64, device=DEV)
    par = lambda t, rows, H, sh, cut, mask=7, row0=0: L.fmri_diffaug_params(P(st), P(t), rows, row0, 12, H, sh, cut, mask,
                                                                         None)
    tb = torch.full((4, 8), 7.0, device=DEV)
    assert par(tb, 4, 129, 16, 64) == -2
    assert par(tb, 4, 64, 65, 32) == -1 and par(tb, 4, 64, 8, 65) == -1 and par(tb, 4, 64, 8, 32, mask=8) == -1
    assert par(tb, 0, 64, 8, 32) == -1 and par(tb, 4, 64, 8, 32, row0=-1) == -1
    assert L.fmri_diffaug_params(P(st), ctypes.c_void_p(tb.data_ptr() + 4), 1, 0, 12, 64, 8, 32, 7, None) == -1
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), torch.full_like(out.view(torch.int16), SENTINEL))
    assert torch.equal(tb, torch.full((4, 8), 7.0, device=DEV))
