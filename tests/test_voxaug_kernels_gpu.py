"""fmri_voxaug_params / fmri_voxaug_apply (csrc/voxaug.hip) against the float64 oracle (tests/voxaug_oracle.py), every
element compared.  B = 5 rows of V = 37 / 100 (V % 4 != 0 / V % 8 != 0: single loads, Philox blocks that straddle the
thread's 8 columns and the rows) and V = 256 (the 16-byte path), at an offset whose block counter carries out of 32 bits
inside the draw, at global row 0 and 3.

The bound of the noise > 0 comparison, per element, derived from the arithmetic and not from the kernel's output
(tests/voxaug_oracle.py ``bound``).  With y64 = k (sigma n + g x) in float64, k the fp32 value of the table:
  * the kernel's normals are within 1e-5 of the float64 Box-Muller map (tests/test_rng_gpu.py derives that bound): the
    noise term moves by at most sigma * 1e-5, the gain g = 1 + gain z0 by gain * 1e-5, which x multiplies;
  * three fp32 roundings (g x; the fma; the product with k), each 2^-24 relative on a value of at most |g x| + sigma |n|,
    counted as four for the second-order terms;
  * both scaled by k; then ONE rounding to fp16: half an fp16 ulp of |y64|, 2^-25 in the subnormal range:
      bound = k (1e-5 (sigma + gain |x|) + 4 2^-24 (|g x| + sigma |n|)) + half_ulp16(y64).
The mask, the span, s, L, p, k and the apply decision are integer or single-operation results and compared exactly."""
import numpy as np
import pytest
import torch

import voxaug_oracle as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, OFF = 11, (1 << 32) - 3
B = 5
SHAPES = [(37, 0), (37, 3), (100, 0), (100, 3), (256, 0), (256, 3)]
KW = dict(noise=0.3, dropout=0.2, span=0.2, gain=0.2)


def _rng():
    from fmri_hip.rng import DeviceRng
    g = DeviceRng(SEED, DEV)
    g.set_state((SEED, OFF))
    return g


def _x(rows, V, seed=0):
    rs = np.random.RandomState(1000 * V + seed)
    x = (3.0 * rs.standard_normal((rows, V))).astype(np.float32)
    x[x == 0] = 1.0                                            # no zeros: a zero of the output is a masked element
    return x


def _run(V, row0, rows=B, x=None, out32=False, **kw):
    from fmri_hip.voxaug import VoxelAugment
    va = VoxelAugment(**kw)
    g = _rng()
    x = _x(rows, V) if x is None else x
    xd = torch.from_numpy(x).to(DEV)
    tab = va.table(g, rows, V, row0=row0)
    o32 = torch.empty(rows, V, dtype=torch.float32, device=DEV) if out32 else None
    y16 = va.apply(xd, tab, g, row0=row0, out32=o32)
    torch.cuda.synchronize()
    assert g.state() == (SEED, OFF)                            # neither launch moves the offset
    assert y16.shape == (rows, (V + 7) // 8 * 8) and not y16[:, V:].any()
    return x, tab.cpu().numpy(), y16[:, :V].cpu().numpy(), (o32.cpu().numpy() if out32 else None)


def _zero_mask(tab, V, row0, rows=B):
    return X.span_mask(tab.astype(np.float64), V) | X.drop_mask(SEED, OFF, rows, V, row0, tab)


@pytest.mark.parametrize("V,row0", SHAPES)
@pytest.mark.parametrize("prob", [1.0, 0.5])
def test_table_matches_the_oracle(V, row0, prob):
    from fmri_hip.voxaug import VoxelAugment
    rows = 64                                                  # enough rows for both outcomes of the apply decision
    tab = VoxelAugment(prob=prob, **KW).table(_rng(), rows, V, row0=row0).cpu().numpy()
    ref, applied = X.table(SEED, OFF, rows, V, row0=row0, prob=prob, **KW)
    assert tab.dtype == np.float32 and tab.shape == (rows, 8)
    if prob < 1:
        assert applied.any() and not applied.all()
    assert np.array_equal(tab[:, 1:], ref[:, 1:].astype(np.float32))           # sigma, p, k, s, L, 0, 0: exact
    assert np.array_equal(tab[~applied], np.tile(X.NEUTRAL, ((~applied).sum(), 1)).astype(np.float32))
    err = np.abs(tab[:, 0].astype(np.float64) - ref[:, 0]).max()
    print(f"V = {V} row0 = {row0} prob = {prob}: g err {err:.3e} bound {KW['gain'] * X.NORMAL_TOL:.3e}")
    assert err <= KW["gain"] * X.NORMAL_TOL
    assert (tab[applied, 0] != 1).any()


def test_table_without_rescale_and_into_a_buffer():
    from fmri_hip.voxaug import VoxelAugment
    out = torch.full((B, 8), 7.0, device=DEV)
    tab = VoxelAugment(rescale=False, dropout=0.5, noise=0.0).table(_rng(), B, 100, out=out)
    assert tab is out
    ref, _ = X.table(SEED, OFF, B, 100, rescale=False, dropout=0.5, noise=0.0)
    assert np.array_equal(out.cpu().numpy(), ref.astype(np.float32)) and (ref[:, 3] == 1).all() and (ref[:, 0] == 1).all()


@pytest.mark.parametrize("V,row0", SHAPES)
def test_zeros_sit_where_the_oracle_masks(V, row0):
    x, tab, y, _ = _run(V, row0, **KW)
    zero = _zero_mask(tab, V, row0)
    assert zero.any() and not zero.all()
    assert np.array_equal(y.view(np.uint16) == 0, zero)        # +0 exactly there, and nowhere else


@pytest.mark.parametrize("V,row0", SHAPES)
def test_without_noise_the_rows_are_the_fp32_restatement_bit_for_bit(V, row0):
    kw = dict(KW, noise=0.0)
    x, tab, y, y32 = _run(V, row0, out32=True, **kw)
    zero = _zero_mask(tab, V, row0)
    g, k = tab[:, 0:1], tab[:, 3:4]                            # fp32, read back from the kernel's table
    ref32 = np.where(zero, np.float32(0), (g * x) * k).astype(np.float32)
    assert y32.tobytes() == ref32.tobytes()
    assert y.tobytes() == ref32.astype(np.float16).tobytes()


@pytest.mark.parametrize("V,row0", SHAPES)
def test_with_noise_the_rows_are_within_the_derived_bound(V, row0):
    x, tab, y, y32 = _run(V, row0, out32=True, **KW)
    ref_tab, _ = X.table(SEED, OFF, B, V, row0=row0, **KW)
    n = X.noise(SEED, OFF, B, V, row0=row0)
    zero = _zero_mask(tab, V, row0)
    x64 = x.astype(np.float64)
    y64 = X.y64(x64, ref_tab, n, zero)
    bound = X.bound(x64, ref_tab, n, y64, KW["gain"])
    err = np.abs(y.astype(np.float64) - y64)
    print(f"V = {V} row0 = {row0}: max err {err.max():.3e}, worst err / bound {np.max(err / bound):.3f}, "
          f"smallest bound {bound.min():.3e}")
    assert (err <= bound).all(), (np.argmax(err / bound), np.max(err / bound))
    assert y.tobytes() == y32.astype(np.float16).tobytes()     # the fp32 result is the value in front of the last rounding


@pytest.mark.parametrize("V", [37, 100, 256])
def test_neutral_table_gives_the_plain_conversion(V):
    from fmri_hip import ops
    from fmri_hip.voxaug import VoxelAugment
    x = _x(B, V)
    x[0, :4] = [0.0, -0.0, 65520.0, 1e-8]                      # zeros of both signs, an overflow, an underflow
    xd = torch.from_numpy(x).to(DEV)
    y = VoxelAugment().apply(xd, VoxelAugment.neutral(B, DEV), _rng(), row0=3)
    ref = ops.rows_to_f16(xd)
    assert torch.equal(y.view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("V", [37, 100, 256])
def test_rows_do_not_depend_on_the_world_size(V):
    x = _x(8, V)
    _, tab, y, _ = _run(V, 0, rows=8, x=x, **KW)
    for r0 in (0, 4):
        _, tab_r, y_r, _ = _run(V, r0, rows=4, x=x[r0:r0 + 4], **KW)
        assert tab_r.tobytes() == tab[r0:r0 + 4].tobytes() and y_r.tobytes() == y[r0:r0 + 4].tobytes(), (V, r0)


@pytest.mark.parametrize("V,row0", SHAPES)
def test_the_noise_is_the_generators_normal_draw(V, row0):
    """With x = 0, g = 1, k = 1 and no mask the formula is half(fl32(sigma n)): bit for bit from DeviceRng.normal's n --
    one Box-Muller definition (csrc/philox.h) behind both kernels."""
    from fmri_hip.rng import SID_VNOISE
    sigma = 0.3
    x = np.zeros((B, V), np.float32)
    _, tab, y, y32 = _run(V, row0, x=x, out32=True, noise=sigma, dropout=0.0)
    n = _rng().normal(B, V, SID_VNOISE, row0=row0).cpu().numpy()
    assert np.abs(n - X.noise(SEED, OFF, B, V, row0=row0)).max() <= X.NORMAL_TOL
    ref32 = np.float32(sigma) * n
    assert y32.tobytes() == ref32.tobytes() and y.tobytes() == ref32.astype(np.float16).tobytes()


def test_a_larger_launch_takes_the_grid_stride_loop():
    """More chunks than the launch has threads (4096 blocks of 256): rows 0 .. of a [2100, 4000] draw equal the same rows
    drawn alone -- the values do not depend on the launch shape."""
    V, rows = 4000, 2100
    x = _x(rows, V)
    _, tab, y, _ = _run(V, 0, rows=rows, x=x, **KW)
    _, tab_s, y_s, _ = _run(V, 2096, rows=4, x=x[2096:], **KW)
    assert tab_s.tobytes() == tab[2096:].tobytes() and y_s.tobytes() == y[2096:].tobytes()
    zero = _zero_mask(tab[2096:], V, 2096, rows=4)
    assert np.array_equal(y_s.view(np.uint16) == 0, zero)


def test_bad_arguments():
    from fmri_hip.voxaug import VoxelAugment
    va, g = VoxelAugment(), _rng()
    x = torch.zeros(B, 37, device=DEV)
    for bad in (torch.zeros(B + 1, 8, device=DEV), torch.zeros(B, 8, device=DEV, dtype=torch.float64),
                torch.zeros(B, 8), torch.zeros(8, B, device=DEV).t()):
        with pytest.raises(ValueError, match="table"):
            va.apply(x, bad, g)
    with pytest.raises(ValueError):
        va.apply(x.double(), VoxelAugment.neutral(B, DEV), g)
    with pytest.raises(ValueError):
        va.apply(x, VoxelAugment.neutral(B, DEV), g, out16=torch.zeros(B, 37, dtype=torch.float16, device=DEV))
    with pytest.raises(ValueError, match="2\\^24"):
        va.table(g, B, 1 << 24)
