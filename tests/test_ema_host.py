"""Host side of the weight average (csrc/ema.hip, fmri_hip/ema.py): the decay schedule against the oracle, the argument
checks of the two entry points -- nothing is enqueued, no GPU is touched -- and every ValueError of WeightEma."""
import ctypes as C

import numpy as np
import pytest

import ema_oracle as EO


@pytest.fixture(scope="module")
def L():
    from fmri_hip import build, lib
    build.build(verbose=False)
    return lib.load()


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.999, 0.9999])
@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("start", [0, 3])
def test_decay_schedule_is_the_oracles(L, decay, warmup, start):
    for t in range(41):
        got = L.fmri_ema_decay_at(t, start, decay, 1 if warmup else 0)
        want = EO.decay_at(t, start, decay, warmup)
        assert np.float32(got).tobytes() == np.float32(want).tobytes(), (t, start, decay, warmup, got, want)
        assert 0.0 <= got <= np.float32(decay)
        if t < start:
            assert got == 0.0
    from fmri_hip.ema import decay_at
    assert decay_at(5, start, decay, warmup) == float(EO.decay_at(5, start, decay, warmup))


def _table(rows):
    from fmri_hip import lib
    t = (lib.EmaSeg * max(len(rows), 1))()
    for r, (live, shadow, n, chunk0) in zip(t, rows):
        r.live, r.shadow, r.n, r.chunk0 = live, shadow, n, chunk0
    return t


def test_bad_tables_are_refused_before_anything_is_enqueued(L):
    from fmri_hip import lib
    assert C.sizeof(lib.EmaSeg) == 32
    BAD = -1
    dev, state = C.c_void_p(0x1000), C.c_void_p(0x2000)          # never dereferenced: every call below returns on the host
    good = _table([(0x10000, 0x20000, 5000, 0), (0, 0, 0, 2), (0x30000, 0x40000, 1, 2)])
    h = lambda t: C.cast(t, C.c_void_p)

    def both(table, table_dev, nseg, st=state):
        return (L.fmri_ema_update(table, table_dev, nseg, st, None), L.fmri_ema_swap(table, table_dev, nseg, None))
    assert both(None, dev, 3) == (BAD, BAD)                      # a null host table
    assert both(h(good), None, 3) == (BAD, BAD)                  # a null device table
    assert both(h(good), dev, -1) == (BAD, BAD)                  # nseg < 0
    assert L.fmri_ema_update(h(good), dev, 3, None, None) == BAD                     # a null state block
    assert L.fmri_ema_update(h(good), dev, 3, C.c_void_p(0x2002), None) == BAD       # ... or a misaligned one
    cases = {
        "negative n": [(0x10000, 0x20000, -4, 0)],
        "chunk0 behind the running count": [(0x10000, 0x20000, 5000, 0), (0x30000, 0x40000, 8, 1)],
        "chunk0 ahead of the running count": [(0x10000, 0x20000, 4096, 0), (0x30000, 0x40000, 8, 2)],
        "first chunk0 not 0": [(0x10000, 0x20000, 16, 1)],
        "null live": [(0, 0x20000, 16, 0)],
        "null shadow": [(0x10000, 0, 16, 0)],
        "live not a multiple of 4": [(0x10002, 0x20000, 16, 0)],
        "shadow not a multiple of 4": [(0x10000, 0x20001, 16, 0)],
    }
    for what, rows in cases.items():
        assert both(h(_table(rows)), dev, len(rows)) == (BAD, BAD), what
    # legal and launching nothing: no segment, and segments of no floats (their pointers are not looked at)
    assert both(None, None, 0) == (0, 0)
    assert both(h(_table([(0, 0, 0, 0), (0, 0, 0, 0)])), dev, 2) == (0, 0)


def test_weight_ema_argument_checks():
    from fmri_hip.ema import WeightEma
    for decay in (-0.1, 1.0, 1.5, float("nan"), "0.9", None, True):
        with pytest.raises(ValueError, match="decay"):
            WeightEma(decay=decay)
    for start in (-1, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="start"):
            WeightEma(start=start)
    for nets in (("generator",), ("encoder", "critic"), ("encoder", "encoder"), "dec"):
        with pytest.raises(ValueError, match="nets"):
            WeightEma(nets=nets)
    e = WeightEma(decay=0, warmup=False, start=2, nets=("discriminator", "encoder"))
    assert (e.decay, e.warmup, e.start, e._asked) == (0.0, False, 2, ("encoder", "discriminator"))
    assert WeightEma(nets="decoder")._asked == ("decoder",) and WeightEma()._asked is None
    # an object belongs to one step: attach() looks at that before it looks at the step
    e.step = object()
    with pytest.raises(ValueError, match="already attached"):
        e.attach(None)
