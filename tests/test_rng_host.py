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


class _RecordingRng:
    """Stands in for a DeviceRng on the host: records the draws and advances a StepDraws issues, in order."""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def normal(self, rows, cols, sid, row0=0, scale=1.0, out=None):
        self.calls.append(("normal", rows, cols, sid, row0, out.data_ptr()))
        return out

    def advance(self, nblocks):
        self.calls.append(("advance", nblocks))


def test_step_draws_given_tensors_pass_through():
    """What the caller passed comes back as the same objects, in order; nothing is drawn, nothing advanced -- with a
    generator and without one."""
    import torch
    from fmri_hip.rng import StepDraws
    a, b = torch.zeros(4, 8), torch.ones(4, 8)
    for g in (None, _RecordingRng()):
        d = StepDraws(g, "SomeStep")
        with d:
            got = list(d.noise(4, 8, 0, 1, ("eps", 0, a), ("z_p", 1, b)))
        assert got[0] is a and got[1] is b
        assert list(d.last.items()) == [("eps", a), ("z_p", b)] and d.last["eps"] is a
        d.close()
        assert d.noted == 0 and (g is None or g.calls == [])


def test_step_draws_missing_noise_without_a_generator_names_every_argument():
    import torch
    from fmri_hip.rng import StepDraws
    d = StepDraws(None, "SomeStep")
    with pytest.raises(ValueError) as e:
        d.noise(4, 8, 0, 1, ("eps", 0, None), ("z_p", 1, torch.zeros(4, 8)), ("z_fake_noise", 3, None))
    assert str(e.value) == ("SomeStep: eps, z_fake_noise not given and the step has no rng "
                            "(pass the noise, or construct the step with rng=DeviceRng(seed, device))")


@pytest.mark.parametrize("largest", ["feed", "table", "voxel", "noise"])
def test_step_draws_one_advance_by_the_largest_behind_the_last_draw(largest):
    """A round with all four consumers -- a shared feed's blocks, an augmentation table's, the fMRI rows' and two drawn
    noise tensors (B = 4 rows of a global batch of 8, Z = 8: blocks(8 * 8) = 16) -- with each of them the largest in
    turn: exactly one advance, by the maximum, after the last draw; the next round starts from zero."""
    import torch
    from fmri_hip.rng import StepDraws, blocks
    B, Z, rank, world = 4, 8, 1, 2
    noise = blocks(B * world * Z)
    assert noise == 16
    n = {"feed": 3, "table": 5, "voxel": 7, "noise": noise}
    if largest != "noise":
        n[largest] = 40
    g = _RecordingRng()
    d = StepDraws(g, "SomeStep")
    given = torch.zeros(B, Z)
    d.note(n["feed"])
    with d:
        d.note(n["table"])
        d.note(n["voxel"])
        eps, z_p, z_t = d.noise(B, Z, rank, world, ("eps", 0, None), ("z_p", 1, given), ("eps_teacher", 2, None))
        assert g.calls == [("normal", B, Z, 0, rank * B, eps.data_ptr()), ("normal", B, Z, 2, rank * B, z_t.data_ptr())]
    assert z_p is given and eps.shape == z_t.shape == (B, Z) and eps.dtype == torch.float32
    assert eps.data_ptr() != z_t.data_ptr()
    assert g.calls[2:] == [("advance", max(n.values()))] and d.noted == 0
    assert list(d.last) == ["eps", "z_p", "eps_teacher"]             # argument order, given and drawn alike
    # a second round starts from zero: the smallest draw alone is advanced by itself, into the same buffers
    del g.calls[:]
    with d:
        d.note(2)
    assert g.calls == [("advance", 2)]
    del g.calls[:]
    with d:
        eps2, = d.noise(B, Z, rank, world, ("eps", 0, None))
    assert eps2 is eps and g.calls == [("normal", B, Z, 0, rank * B, eps.data_ptr()), ("advance", noise)]
    assert list(d.last) == ["eps"]


def test_step_draws_close_with_nothing_noted_issues_nothing():
    from fmri_hip.rng import StepDraws
    g = _RecordingRng()
    d = StepDraws(g, "SomeStep")
    d.close()
    with d:
        d.note(0)
    StepDraws(None, "SomeStep").close()
    assert g.calls == []


def test_step_draws_a_failed_round_leaves_nothing_pending():
    """A step that raises between its draws and the end of the round advances nothing, then or in the next round."""
    from fmri_hip.rng import StepDraws
    g = _RecordingRng()
    d = StepDraws(g, "SomeStep")
    with pytest.raises(RuntimeError):
        with d:
            d.note(9)
            raise RuntimeError("a bad table")
    assert d.noted == 0
    d.close()
    assert g.calls == []


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
