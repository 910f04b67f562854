"""CPU-side checks of the epoch sampler's definition: the numpy restatement (tests/sampler_oracle.py) is a permutation for
every N, moves with the epoch and the seed, and its state machine visits floor(N / B) * B distinct samples per epoch and
rolls over where include/fmri_hip.h says; the C ABI of the feed (declared, exported, bad geometry refused on the host) and
the Python surface (fmri_hip.feed, ``feed=`` / ``start=``).  No kernels are launched here."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import sampler_oracle as S

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("fmri_sampler_indices", "fmri_sampler_advance", "fmri_rng_u32_at", "fmri_ingest_u8_gather",
           "fmri_gather_rows_f32")
SEED, SEED2 = 0x9E3779B97F4A7C15, 12345
SIZES = [1, 2, 3, 5, 16, 17, 255, 256, 257, 1000, 65537]


@pytest.mark.parametrize("N", SIZES)
def test_pi_is_a_permutation_that_moves_with_epoch_and_seed(N):
    """Two permutations of N >= 17 elements drawn independently coincide with probability 1 / N! < 3e-15: a keyed
    bijection that is the same for two epochs or two seeds there is not keyed by them."""
    i = np.arange(N)
    e0, e1, other = S.pi(SEED, 0, i, N), S.pi(SEED, 1, i, N), S.pi(SEED2, 0, i, N)
    for p in (e0, e1, other, S.pi(SEED, 2 ** 40 + 3, i, N)):              # (an epoch that uses the high counter word)
        assert p.dtype == np.int64 and np.array_equal(np.sort(p), i), N
    if N >= 17:
        assert not np.array_equal(e0, e1) and not np.array_equal(e0, other)
        assert not np.array_equal(e0, i)
    # a pure function of (seed, epoch, i, N): single positions and slices give what the whole table gives
    assert int(S.pi(SEED, 1, N - 1, N)[0]) == e1[-1]
    assert np.array_equal(S.pi(SEED, 1, i[N // 2:], N), e1[N // 2:])


def test_pi_spreads_the_positions():
    """Not only a bijection: over 64 epochs every position of N = 16 lands on every value about equally often
    (expectation 4 per cell of the 16 x 16 table of counts; every row and every column of the table sums to 64, which
    leaves (16 - 1)^2 = 225 degrees of freedom: chi-square mean 225, standard deviation sqrt(450) ~ 21.2 -- bound at
    mean + 5 sigma)."""
    N, E = 16, 64
    counts = np.zeros((N, N))
    for e in range(E):
        counts[np.arange(N), S.pi(SEED, e, np.arange(N), N)] += 1
    chi2 = ((counts - E / N) ** 2 / (E / N)).sum()
    print("chi2", chi2)
    assert chi2 < 225 + 5 * 21.2


@pytest.mark.parametrize("N,B", [(10, 4), (8, 4), (4, 4), (257, 256)])
def test_state_machine_drops_the_tail_and_rolls_over(N, B):
    s = S.Sampler(SEED, N)
    per_epoch = N // B
    for epoch in range(3):
        seen = []
        for b in range(per_epoch):
            assert (s.epoch, s.cursor) == (epoch, b * B)
            idx = s.next(B)
            assert np.array_equal(idx, S.pi(SEED, epoch, np.arange(b * B, (b + 1) * B), N))
            seen.append(idx)
        seen = np.concatenate(seen)
        assert len(seen) == per_epoch * B == len(set(seen.tolist())) and seen.min() >= 0 and seen.max() < N
        assert (s.epoch, s.cursor) == (epoch + 1, 0)                     # rolled over: fewer than B positions were left
    # ranks read slices of the one-rank batch
    s = S.Sampler(SEED, N, epoch=1)
    if B % 2 == 0:
        assert np.array_equal(np.concatenate([s.indices(B // 2), s.indices(B // 2, row0=B // 2)]), s.indices(B))


def test_the_feed_symbols_are_declared_and_exported():
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
    z, odd = ctypes.c_void_p(64), ctypes.c_void_p(68)
    f = [ctypes.c_float(v) for v in (0.5, 0.5, 0.5, 0.5, 0.5, 0.5)]
    assert lib.fmri_sampler_indices(None, 10, 4, 0, z, None) == -1
    assert lib.fmri_sampler_indices(odd, 10, 4, 0, z, None) == -1                 # state not 8-byte aligned
    assert lib.fmri_sampler_indices(z, 10, 4, 0, None, None) == -1
    assert lib.fmri_sampler_indices(z, 0, 4, 0, z, None) == -1
    assert lib.fmri_sampler_indices(z, 10, 0, 0, z, None) == -1
    assert lib.fmri_sampler_indices(z, 10, 4, -1, z, None) == -1
    assert lib.fmri_sampler_indices(z, 10, 4, 8, z, None) == -2                   # rows 8 .. 11 of 10
    assert lib.fmri_sampler_advance(None, 10, 4, None) == -1
    assert lib.fmri_sampler_advance(z, 10, 0, None) == -1
    assert lib.fmri_sampler_advance(z, 3, 4, None) == -2                          # N < B_global
    assert lib.fmri_rng_u32_at(z, z, 4, -1, 0, 0, 1, None) == -1                  # negative start
    assert lib.fmri_rng_u32_at(z, z, 0, 0, 0, 0, 1, None) == -1
    assert lib.fmri_rng_u32_at(z, z, 4, 0, 0, 2, 1, None) == -1                   # hi < lo
    assert lib.fmri_rng_u32_at(z, z, 4, (1 << 40) + 1, 0, 0, 1, None) == -2
    assert lib.fmri_ingest_u8_gather(z, None, 11, 4, 8, 8, 3, None, None, *f, z, None, None, None) == -1     # no indices
    assert lib.fmri_ingest_u8_gather(z, z, 0, 4, 8, 8, 3, None, None, *f, z, None, None, None) == -1         # empty pool
    assert lib.fmri_ingest_u8_gather(z, z, 11, 4, 8, 8, 2, None, None, *f, z, None, None, None) == -1        # C = 2
    assert lib.fmri_ingest_u8_gather(z, z, 11, 4, 8, 8, 3, None, None, *f, None, None, None, None) == -1     # no output
    assert lib.fmri_ingest_u8_gather(z, z, 11, 4, 8, 8, 3, None, None, *f, ctypes.c_void_p(72), None, None, None) == -1
    assert lib.fmri_gather_rows_f32(z, 11, 7, None, 4, z, None, None, None) == -1
    assert lib.fmri_gather_rows_f32(z, 11, 0, z, 4, z, None, None, None) == -1
    assert lib.fmri_gather_rows_f32(z, 11, 7, z, 4, None, None, None, None) == -1                            # no output
    assert lib.fmri_gather_rows_f32(z, 11, 7, z, 4, None, ctypes.c_void_p(72), None, None) == -1             # fp16 rows unaligned


def test_python_surface():
    """The four fused steps gain ``feed=None`` and their batch arguments default to None; the draws gain ``start=0``
    (signatures only: no GPU)."""
    from fmri_hip import feed, rng
    from fmri_hip.steps import CognitiveStep, Stage1Step
    from fmri_hip.wae_steps import DualStage1Step, WaeStep
    assert rng.SID_PERM == S.SID_PERM == 16
    for cls, batch in ((Stage1Step, ("x",)), (CognitiveStep, ("fmri", "image")), (WaeStep, ("image", "fmri")),
                       (DualStage1Step, ("x",))):
        assert inspect.signature(cls.__init__).parameters["feed"].default is None
        sp = inspect.signature(cls.step).parameters
        for n in batch:
            assert sp[n].default is None, (cls.__name__, n)
    for fn in (rng.DeviceRng.integers, rng.DeviceRng.flips, rng.DeviceRng.shifts):
        assert inspect.signature(fn).parameters["start"].default == 0
    fp = inspect.signature(feed.DeviceFeed.__init__).parameters
    assert [fp[k].default for k in ("rng", "max_shift", "flip", "rank", "world")] == [None, 0, False, None, None]
    for name in ("next", "last_indices", "position", "set_position"):
        assert callable(getattr(feed.DeviceFeed, name))
    assert callable(feed.DeviceDataset)
