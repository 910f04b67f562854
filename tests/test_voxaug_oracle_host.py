"""The fMRI-augmentation oracle against itself (tests/voxaug_oracle.py) and the argument checks of ``VoxelAugment`` -- no
GPU: the neutral table is the identity, the span lies inside the row, prob = 0 leaves every row neutral, the dropout rate
is the stated probability, and the formula restated in fp32 stays inside the bound the kernel tests use."""
import numpy as np
import pytest

import voxaug_oracle as X

SEED, OFF = 9, (1 << 32) - 3


def _x(B, V, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((B, V)).astype(np.float32)
    x[x == 0] = 1.0
    return x


def test_neutral_table_is_the_identity():
    B, V = 5, 37
    x = _x(B, V)
    tab = np.tile(X.NEUTRAL, (B, 1))
    n = X.noise(SEED, OFF, B, V)
    zero = X.span_mask(tab, V) | X.drop_mask(SEED, OFF, B, V, 0, tab)
    assert not zero.any()
    assert np.array_equal(X.y64(x.astype(np.float64), tab, n, zero), x.astype(np.float64))
    assert X.apply32(x, tab, n, zero).tobytes() == x.astype(np.float16).tobytes()


@pytest.mark.parametrize("V,span", [(37, 0.3), (100, 0.25), (256, 1.0), (64, 0.0), (9, 0.06)])
def test_span_lies_inside_the_row(V, span):
    B = 64
    tab, applied = X.table(SEED, OFF, B, V, span=span)
    L = X.span_len(V, span)
    assert applied.all() and (tab[:, 5] == L).all()
    assert (tab[:, 4] >= 0).all() and (tab[:, 4] + L <= V).all() and (tab[:, 4] == np.floor(tab[:, 4])).all()
    m = X.span_mask(tab, V)
    assert (m.sum(1) == L).all()
    if 0 < L < V:
        assert len(set(tab[:, 4])) > 1                       # the start moves from row to row


def test_prob_zero_leaves_every_row_neutral_and_prob_selects_rows():
    tab, applied = X.table(SEED, OFF, 32, 100, noise=0.3, dropout=0.2, span=0.2, gain=0.1, prob=0.0)
    assert not applied.any() and np.array_equal(tab, np.tile(X.NEUTRAL, (32, 1)))
    tab, applied = X.table(SEED, OFF, 4096, 100, noise=0.3, dropout=0.2, span=0.2, gain=0.1, prob=0.25)
    sd = np.sqrt(0.25 * 0.75 / 4096)
    assert abs(applied.mean() - 0.25) < 5 * sd
    assert np.array_equal(tab[~applied], np.tile(X.NEUTRAL, ((~applied).sum(), 1)))
    assert (tab[applied, 1] == float(np.float32(0.3))).all() and (tab[applied, 5] == 20).all()
    full, _ = X.table(SEED, OFF, 4096, 100, noise=0.3, dropout=0.2, span=0.2, gain=0.1, prob=1.0)
    assert np.array_equal(full[applied], tab[applied])         # the same draws, whatever prob says


def test_rows_are_a_function_of_the_global_row():
    full, _ = X.table(SEED, OFF, 8, 100, gain=0.2, span=0.1)
    part, _ = X.table(SEED, OFF, 4, 100, row0=4, gain=0.2, span=0.1)
    assert np.array_equal(part, full[4:])
    assert np.array_equal(X.noise(SEED, OFF, 4, 37, row0=4), X.noise(SEED, OFF, 8, 37)[4:])
    assert np.array_equal(X.drop_words(SEED, OFF, 4, 37, row0=4), X.drop_words(SEED, OFF, 8, 37)[4:])


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_rate(p):
    B, V = 200, 1000                                           # 2e5 elements
    tab, _ = X.table(SEED, OFF, B, V, dropout=p)
    rate = X.drop_mask(SEED, OFF, B, V, 0, tab).mean()
    sd = np.sqrt(p * (1 - p) / (B * V))
    print(f"dropout p = {p}: rate {rate:.5f}, {abs(rate - p) / sd:.2f} standard deviations")
    assert abs(rate - p) < 5 * sd
    assert tab[0, 3] == float(np.float32(1) / (np.float32(1) - np.float32(p)))
    assert X.table(SEED, OFF, B, V, dropout=p, rescale=False)[0][0, 3] == 1.0


def test_threshold_is_an_integer_comparison():
    assert X.threshold(0.0) == 0 and X.threshold(0.5) == 1 << 31
    assert X.threshold(np.float32(0.1)) == int(float(np.float32(0.1)) * 2.0 ** 32) < 1 << 32
    assert X.threshold(np.nextafter(np.float32(1), np.float32(0))) == (1 << 32) - 256


@pytest.mark.parametrize("V", [37, 100, 256])
def test_fp32_restatement_lies_within_the_bound(V):
    """The reference alone stays inside the bound: the formula in fp32 (normals and gain rounded to fp32) against y64."""
    B, gain = 5, 0.2
    x = _x(B, V, seed=V) * 3.0
    tab, _ = X.table(SEED, OFF, B, V, row0=3, noise=0.3, dropout=0.2, span=0.2, gain=gain)
    n = X.noise(SEED, OFF, B, V, row0=3)
    zero = X.span_mask(tab, V) | X.drop_mask(SEED, OFF, B, V, 3, tab)
    assert zero.any() and not zero.all()
    y = X.y64(x.astype(np.float64), tab, n, zero)
    got = X.apply32(x, tab, n, zero).astype(np.float64)
    b = X.bound(x.astype(np.float64), tab, n, y, gain)
    err = np.abs(got - y)
    print(f"V = {V}: worst err / bound {np.max(err / b):.3f}")
    assert (err <= b).all()
    assert (got[zero] == 0).all() and (got[~zero] != 0).all()
    # the bound is not slack by orders of magnitude: the fp16 rounding alone comes near it somewhere
    assert np.max(err / b) > 0.5


def test_half_ulp16():
    assert X.half_ulp16(np.array([1.0]))[0] == 2.0 ** -11 and X.half_ulp16(np.array([1.999]))[0] == 2.0 ** -11
    assert X.half_ulp16(np.array([2.0]))[0] == 2.0 ** -10 and X.half_ulp16(np.array([-3.0]))[0] == 2.0 ** -10
    assert X.half_ulp16(np.array([0.0]))[0] == 2.0 ** -25 and X.half_ulp16(np.array([2.0 ** -15]))[0] == 2.0 ** -25
    assert X.half_ulp16(np.array([2.0 ** -14]))[0] == 2.0 ** -25 and X.half_ulp16(np.array([2.0 ** -13]))[0] == 2.0 ** -24


def test_stream_ids_and_block_counts():
    from fmri_hip import rng, voxaug
    assert (rng.SID_VNOISE, rng.SID_VDROP, rng.SID_VROW) == (X.SID_VNOISE, X.SID_VDROP, X.SID_VROW) == (14, 15, 17)
    ids = [v for k, v in vars(rng).items() if k.startswith("SID_")]
    assert len(ids) == len(set(ids))                           # no stream id is taken twice
    assert voxaug.blocks(4, 256) == 256 and voxaug.blocks(8, 37) == 74 and voxaug.blocks(256, 4096) == 262144


def test_argument_validation():
    from fmri_hip.voxaug import VoxelAugment, _check_voxels
    VoxelAugment()
    VoxelAugment(noise=0.0, dropout=0.0, span=1.0, gain=0.0, prob=0.0, rescale=False)
    for kw in (dict(dropout=1.0), dict(dropout=-0.1), dict(span=1.5), dict(span=-0.1), dict(prob=1.1), dict(prob=-1.0),
               dict(noise=-0.1), dict(gain=-1.0), dict(noise=float("nan"))):
        with pytest.raises(ValueError):
            VoxelAugment(**kw)
    assert VoxelAugment(span=0.25).span_len(100) == 25 and VoxelAugment(span=0.3).span_len(37) == X.span_len(37, 0.3)
    _check_voxels((1 << 24) - 1)
    with pytest.raises(ValueError, match="2\\^24"):
        _check_voxels(1 << 24)
    assert "dropout=0.1" in repr(VoxelAugment())


def test_c_abi_refuses_bad_arguments_before_anything_is_launched():
    """fmri_voxaug_params / fmri_voxaug_apply (include/fmri_hip.h): host-side checks only, no GPU touched."""
    import ctypes
    from fmri_hip import build, lib as L
    build.build(verbose=False)
    lib = L.load()
    P, F = ctypes.c_void_p, ctypes.c_float
    z = P(4096)

    def params(state=z, table=z, rows=4, row0=0, sid=17, V=100, gain=0.1, sigma=0.1, p=0.1, rescale=1, L=10, prob=1.0):
        return lib.fmri_voxaug_params(state, table, rows, row0, sid, V, F(gain), F(sigma), F(p), rescale, L, F(prob), None)

    def apply(src=z, V=100, B=4, table=z, state=z, row0=0, sn=14, sd=15, dst16=P(8192), dst32=None):
        return lib.fmri_voxaug_apply(src, V, B, table, state, row0, sn, sd, dst16, dst32, None)
    for kw in (dict(state=None), dict(table=None), dict(table=P(4100)), dict(state=P(4100)), dict(rows=0), dict(row0=-1),
               dict(sid=-1), dict(V=0), dict(V=1 << 24), dict(L=101), dict(L=-1), dict(gain=-0.1), dict(sigma=-1.0),
               dict(p=1.0), dict(p=-0.1), dict(prob=1.5), dict(prob=-0.5), dict(p=float("nan"))):
        assert params(**kw) == -1, kw
    for kw in (dict(src=None), dict(src=P(4098)), dict(table=P(4104)), dict(state=None), dict(dst16=None),
               dict(dst16=P(8200)), dict(dst32=P(4098)), dict(V=0), dict(V=1 << 24), dict(B=0), dict(row0=-1),
               dict(sn=-1), dict(sn=15), dict(dst32=P(4096)), dict(dst32=P(4096 + 4 * 399))):
        assert apply(**kw) == -1, kw
    assert apply(V=1 << 23, B=512) == -2
