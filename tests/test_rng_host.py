"""CPU-side checks of the device generator's definition: the numpy restatement (tests/rng_oracle.py) against the
Random123 known answers, the distribution of its normal and integer maps, and the C ABI of csrc/rng.hip (declared,
exported, bad geometry refused on the host).  No kernels are launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import rng_oracle as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("fmri_rng_normal", "fmri_rng_u32", "fmri_rng_advance")

# counter, key, output: the known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10 rounds)
KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = " ".join("%08x" % int(v) for v in R.philox4x32_10(ctr, key))
    assert got == want


def test_philox_is_vectorised_consistently():
    """Arrays of counters give what the counters give one by one (the layout functions rely on it)."""
    ctr = (np.arange(5), np.zeros(5), np.full(5, 3), np.zeros(5))
    many = np.stack(R.philox4x32_10(ctr, (7, 9)), 1)
    for i in range(5):
        one = [int(v) for v in R.philox4x32_10((i, 0, 3, 0), (7, 9))]
        assert many[i].tolist() == one


def test_counter_layout():
    """Element e = (row0 + r) * cols + c is word e % 4 of block offset + e // 4; the offset carries into the second
    counter word; the stream id is the third word; the key is (low, high) of the seed."""
    seed, off = (0x299f31d0 << 32) | 0xa4093822, 0xFFFFFFFF
    w = R.raw_words(seed, off, 9, sid=5)
    b0 = [int(v) for v in R.philox4x32_10((0xFFFFFFFF, 0, 5, 0), (0xa4093822, 0x299f31d0))]
    b1 = [int(v) for v in R.philox4x32_10((0, 1, 5, 0), (0xa4093822, 0x299f31d0))]
    b2 = [int(v) for v in R.philox4x32_10((1, 1, 5, 0), (0xa4093822, 0x299f31d0))]
    assert w.tolist() == b0 + b1 + b2[:1]
    # rows of a draw that starts at a global row equal those rows of the draw from row 0 -- at any split
    full = R.normal(3, 17, 8, 127)
    assert np.array_equal(R.normal(3, 17, 5, 127, row0=3), full[3:])
    assert np.array_equal(R.normal(3, 17, 3, 127, row0=0), full[:3])
    # other stream id, other offset, other seed: other numbers
    for other in (R.normal(3, 17, 8, 127, sid=1), R.normal(3, 18, 8, 127), R.normal(4, 17, 8, 127)):
        assert not np.any(other == full)
    assert np.array_equal(R.normal(3, 17, 8, 127, scale=0.5), 0.5 * full)


def test_normal_map_moments_and_ks():
    """2^20 normals at seed 1234, offset 0, sid 0.  Five-sigma bounds on the first moments of N(0, 1) (sd of the sample
    mean 1/sqrt(n), of the variance sqrt(2/n), of the fourth moment sqrt(96/n)) and a KS test: a wrong uniform map or
    Box-Muller pairing misses them by orders of magnitude, this seed sits at 0.14 / 0.3 / 0.1 sigma."""
    from scipy import stats
    n = 1 << 20
    z = R.normal(1234, 0, n, 1).ravel()
    mean, var, m4 = z.mean(), z.var(), (z ** 4).mean()
    p = stats.kstest(z, "norm").pvalue
    print(f"mean {mean:.3e} var {var:.5f} m4 {m4:.4f} KS p {p:.3f} max|z| {np.abs(z).max():.3f}")
    assert abs(mean) < 5 / np.sqrt(n)
    assert abs(var - 1) < 5 * np.sqrt(2 / n)
    assert abs(m4 - 3) < 5 * np.sqrt(96 / n)
    assert p > 0.01
    assert np.abs(z).max() <= np.sqrt(-2 * np.log(2.0 ** -25))       # the tail limit of 24-bit uniforms, ~5.89


def test_uniform_map_stays_inside_the_open_interval():
    u = R.uniform(np.array([0, 0xFF, 0x100, 0xFFFFFFFF], dtype=np.uint64))
    assert u[0] == u[1] == 2.0 ** -25 and u[2] == 1.5 * 2.0 ** -24 and u[3] == 1 - 2.0 ** -25


def test_integers_map():
    n = 1 << 16
    for lo, hi in ((0, 1), (-5, 5), (-1, 1), (3, 3), (-2 ** 31, 2 ** 31 - 1)):
        v = R.integers(1234, 0, n, lo, hi, 9)
        assert v.min() >= lo and v.max() <= hi, (lo, hi)
    v = R.integers(1234, 0, n, -5, 5, 9)
    assert sorted(set(v.tolist())) == list(range(-5, 6))
    # over the full int32 range the multiply-high is the identity: the words themselves, shifted by lo
    w = R.raw_words(1234, 0, 64, 9)
    assert np.array_equal(R.integers(1234, 0, 64, -2 ** 31, 2 ** 31 - 1, 9), w.astype(np.int64) - 2 ** 31)
    f = R.integers(1234, 0, n, 0, 1, 8)
    assert abs(f.mean() - 0.5) < 5 * 0.5 / np.sqrt(n)


def test_abi_declares_and_exports_the_generator():
    hdr = open(os.path.join(ROOT, "include", "fmri_hip.h")).read()
    declared = set(re.findall(r"\b(fmri_[a-z0-9_]+)\s*\(", hdr))
    from fmri_hip import build, lib as L
    build.build(verbose=False)
    lib = L.load()
    for name in SYMBOLS:
        assert name in declared, f"{name} is not declared in include/fmri_hip.h"
        assert name in L.EXPORTS and hasattr(lib, name)


def test_bad_geometry_is_refused_on_the_host():
    """Nothing is enqueued for arguments the kernels cannot serve: FMRI_E_BADARG (-1) / FMRI_E_UNSUPPORTED (-2)."""
    from fmri_hip import build, lib as L
    build.build(verbose=False)
    lib = L.load()
    z, f1 = ctypes.c_void_p(64), ctypes.c_float(1.0)
    assert lib.fmri_rng_normal(None, z, 4, 8, 8, 0, 0, f1, None) == -1            # no state
    assert lib.fmri_rng_normal(ctypes.c_void_p(68), z, 4, 8, 8, 0, 0, f1, None) == -1   # state not 8-byte aligned
    assert lib.fmri_rng_normal(z, None, 4, 8, 8, 0, 0, f1, None) == -1
    assert lib.fmri_rng_normal(z, z, 0, 8, 8, 0, 0, f1, None) == -1
    assert lib.fmri_rng_normal(z, z, 4, 8, 7, 0, 0, f1, None) == -1               # ld < cols
    assert lib.fmri_rng_normal(z, z, 4, 8, 8, -1, 0, f1, None) == -1              # negative global row
    assert lib.fmri_rng_normal(z, z, 4, 8, 8, 0, -1, f1, None) == -1              # negative stream id
    assert lib.fmri_rng_normal(z, z, 1 << 16, 1 << 15, 1 << 15, 0, 0, f1, None) == -2   # 2^31 elements
    assert lib.fmri_rng_normal(z, z, 4, 8, 8, (1 << 40) + 1, 0, f1, None) == -2
    assert lib.fmri_rng_u32(z, z, 0, 0, 0, 1, None) == -1
    assert lib.fmri_rng_u32(z, z, 4, 0, 2, 1, None) == -1                         # hi < lo
    assert lib.fmri_rng_u32(z, z, (1 << 40) + 1, 0, 0, 1, None) == -2
    assert lib.fmri_rng_advance(None, 1, None) == -1
    assert lib.fmri_rng_advance(z, -1, None) == -1


def test_step_constructors_take_an_rng_and_noise_is_optional():
    """The four fused steps gain ``rng=None`` and their noise arguments default to None (signatures only: no GPU)."""
    import inspect
    from fmri_hip import rng
    from fmri_hip.steps import CognitiveStep, Stage1Step
    from fmri_hip.wae_steps import DualStage1Step, WaeStep
    assert (rng.SID_EPS, rng.SID_ZP, rng.SID_EPS_TEACHER, rng.SID_ZFAKE, rng.SID_FLIP, rng.SID_SHIFT) == (0, 1, 2, 3, 8, 9)
    for cls, noise in ((Stage1Step, ("eps", "z_p")), (CognitiveStep, ("eps", "z_p", "eps_teacher")),
                       (WaeStep, ("z_fake_noise",)), (DualStage1Step, ("eps", "z_p", "z_fake_noise"))):
        assert inspect.signature(cls.__init__).parameters["rng"].default is None
        sp = inspect.signature(cls.step).parameters
        for n in noise:
            assert sp[n].default is None, (cls.__name__, n)
        assert callable(cls.last_noise)
