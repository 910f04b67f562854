"""Numerics monitor, host side (no GPU): the new C entry points are declared and exported and check their arguments
before anything is enqueued; ``monitor.decode`` turns a hand-built device block into the documented dict."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

NEW = ("fmri_tensor_stats", "fmri_tensor_stats_ws_bytes", "fmri_apply_batch_stats", "fmri_stat_fold",
       "fmri_bn_bwd_apply_cnt", "fmri_bn_bwd_apply2_cnt", "fmri_bn_cols_bwd_cnt")


@pytest.fixture(scope="module")
def lib():
    from fmri_hip import lib as L
    return L.load()


def test_new_symbols_are_declared_and_exported(lib):
    from fmri_hip import lib as L
    hdr = open(os.path.join(ROOT, "include", "fmri_hip.h")).read()
    declared = set(re.findall(r"\b(fmri_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in L.EXPORTS, name
    assert "typedef struct fmri_stat {" in hdr and "typedef struct fmri_stat_seg {" in hdr


def test_bindings_pass_every_declared_parameter():
    """The ctypes argument lists of the new entry points have as many entries as the header's declarations."""
    from fmri_hip import lib as L
    hdr = open(os.path.join(ROOT, "include", "fmri_hip.h")).read()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)      # the declaration, not a mention in a comment
        assert m, name
        assert m.group(1).rstrip().endswith("void* stream") or name == "fmri_tensor_stats_ws_bytes", name   # host only
        assert len(L._SIGS[name]) == m.group(1).count(",") + 1, name


def test_struct_layouts_match_the_header(lib):
    from fmri_hip import lib as L
    from fmri_hip import monitor
    assert ctypes.sizeof(L.StatSeg) == 64
    assert monitor.STAT_DTYPE.itemsize == L.STAT_BYTES == 32
    assert lib.fmri_tensor_stats_ws_bytes(8) == 8 * 256 * 32
    assert lib.fmri_tensor_stats_ws_bytes(0) == 0 and lib.fmri_tensor_stats_ws_bytes(9) == 0


def test_argument_checks_return_badarg(lib):
    from fmri_hip import lib as L
    z = ctypes.c_void_p(16)
    odd = ctypes.c_void_p(20)                          # not 8-byte aligned
    segs = (L.StatSeg * 2)()
    for s in segs:
        s.x, s.rows, s.cols, s.ld, s.out = 16, 4, 4, 4, 32
    assert lib.fmri_tensor_stats(None, 1, z, None) == -1
    assert lib.fmri_tensor_stats(segs, 0, z, None) == -1
    assert lib.fmri_tensor_stats(segs, 9, z, None) == -1
    assert lib.fmri_tensor_stats(segs, 1, None, None) == -1
    assert lib.fmri_tensor_stats(segs, 1, odd, None) == -1
    segs[1].ld = 3                                     # ld < cols
    assert lib.fmri_tensor_stats(segs, 2, z, None) == -1
    segs[1].ld, segs[1].out = 4, None                  # no output record
    assert lib.fmri_tensor_stats(segs, 2, z, None) == -1
    segs[1].out, segs[1].x = 32, None
    assert lib.fmri_tensor_stats(segs, 2, z, None) == -1
    # apply_batch_stats: modes 1 / 3 only, a learning rate and an aligned record buffer
    assert lib.fmri_apply_batch_stats(z, 1, 1, 0, z, 0.9, 1e-8, 1.0, None, 0.0, None, 0, z, None) == -1
    assert lib.fmri_apply_batch_stats(z, 1, 1, 2, z, 0.9, 1e-8, 1.0, None, 0.0, None, 0, z, None) == -1
    assert lib.fmri_apply_batch_stats(z, 1, 1, 1, None, 0.9, 1e-8, 1.0, None, 0.0, None, 0, z, None) == -1
    assert lib.fmri_apply_batch_stats(z, 1, 1, 1, z, 0.9, 1e-8, 1.0, None, 0.0, None, 0, None, None) == -1
    assert lib.fmri_apply_batch_stats(z, 1, 1, 3, z, 0.9, 1e-8, 1.0, None, 0.0, None, 0, odd, None) == -1
    assert lib.fmri_stat_fold(None, 1, None, z, None) == -1
    assert lib.fmri_stat_fold(z, 1, None, None, None) == -1
    assert lib.fmri_stat_fold(z, -1, None, z, None) == -1
    # counted BatchNorm backward: the counter pointer is required, the other checks are the uncounted entries'
    assert lib.fmri_bn_bwd_apply_cnt(z, z, z, 4, 8, 4.0, z, z, z, z, 0, z, None, None) == -1
    assert lib.fmri_bn_bwd_apply_cnt(z, z, z, 4, 12, 4.0, z, z, z, z, 0, z, z, None) == -1
    assert lib.fmri_bn_bwd_apply2_cnt(z, z, z, 4, 8, 4.0, z, z, z, z, 0, z, None, None) == -1
    assert lib.fmri_bn_bwd_apply2_cnt(z, z, z, 0, 8, 4.0, z, z, z, z, 0, z, z, None) == -1
    assert lib.fmri_bn_cols_bwd_cnt(z, z, z, 4, 8, 1, 4.0, z, z, z, z, 0, z, None, None, 1.0, 0, None, None) == -1
    assert lib.fmri_bn_cols_bwd_cnt(z, z, z, 4, 8, 1, 4.0, z, z, z, z, 0, z, None, None, 1.0, 1, z, None) == -1


def _rec(sumsq=0.0, mx=-np.inf, mn=np.inf, max_abs=0.0, nonfinite=0, clamped=0, written=1):
    from fmri_hip import monitor
    return np.array([(sumsq, mx, mn, max_abs, nonfinite, clamped, written)], dtype=monitor.STAT_DTYPE)


def test_decode_of_a_hand_built_block():
    from fmri_hip import monitor
    lay = monitor.Layout(nets=("encoder", "decoder", "discriminator"), bns=("decoder.fc.1", "encoder.conv.0.bn"),
                         n_loss=1)
    recs = [
        _rec(sumsq=9.0, mx=2.0, mn=-2.5, max_abs=2.5, nonfinite=1, clamped=3),     # encoder gradient
        _rec(max_abs=0.75, mx=0.75, mn=-0.5),                                         # encoder weights
        _rec(written=0), _rec(written=0),                                             # decoder: gated off
        _rec(sumsq=16.0, max_abs=1.5, mx=1.5, mn=0.0),                                # discriminator gradient
        _rec(max_abs=3.0, nonfinite=2, mx=3.0, mn=-1.0),                              # discriminator weights
        _rec(sumsq=1.0, mx=0.5, mn=-4.0, max_abs=4.0),                                # mu
        _rec(sumsq=1.0, mx=25.5, mn=-3.0, max_abs=25.5, nonfinite=1),                 # logvar
        _rec(sumsq=1.0, mx=1.0, mn=0.0, max_abs=1.0),                                 # losses: finite
    ]
    raw = b"".join(r.tobytes() for r in recs)
    raw += np.array([2.0 ** -5, 1.0, 1.0, 1.0], dtype="<f4").tobytes()
    raw += np.array([[3, 0], [0, 7]], dtype="<i4").tobytes()
    assert len(raw) == lay.nbytes
    d = monitor.decode(np.frombuffer(raw, dtype=np.uint8), lay)
    assert set(d) == {"grad", "param", "bn_backward", "latent", "losses_finite"}
    assert d["grad"]["encoder"] == dict(updated=True, norm=3.0, max_abs=2.5, nonfinite=1, clamped=3)
    assert d["grad"]["decoder"] == dict(updated=False, norm=None, max_abs=None, nonfinite=None, clamped=None)
    assert d["grad"]["discriminator"]["norm"] == 4.0
    assert d["param"]["encoder"] == dict(max_abs=0.75, nonfinite=0)
    assert d["param"]["decoder"] == dict(max_abs=None, nonfinite=None)
    assert d["param"]["discriminator"] == dict(max_abs=3.0, nonfinite=2)
    assert d["bn_backward"] == {"decoder.fc.1": dict(saturated=3, nonfinite=0),
                                "encoder.conv.0.bn": dict(saturated=0, nonfinite=7)}
    lat = d["latent"]
    assert lat["logvar_max"] == 25.5 and lat["logvar_min"] == -3.0 and lat["mu_max_abs"] == 4.0
    assert lat["nonfinite"] == 1
    assert lat["range_exp"] == [5.0, 0.0, 0.0, 0.0]
    assert d["losses_finite"] is True
    # a non-finite loss slot, or one never written, makes losses_finite False
    bad = raw[:8 * 32] + _rec(nonfinite=1).tobytes() + raw[9 * 32:]
    assert monitor.decode(np.frombuffer(bad, dtype=np.uint8), lay)["losses_finite"] is False
    unwritten = raw[:8 * 32] + _rec(written=0).tobytes() + raw[9 * 32:]
    assert monitor.decode(np.frombuffer(unwritten, dtype=np.uint8), lay)["losses_finite"] is False
    with pytest.raises(ValueError):
        monitor.decode(np.zeros(lay.nbytes - 1, dtype=np.uint8), lay)
    assert math.isclose(d["grad"]["encoder"]["norm"], 3.0)


def test_steps_take_a_monitor_argument_defaulting_to_off():
    import inspect
    from fmri_hip.steps import CognitiveStep, Stage1Step
    from fmri_hip.wae_steps import DualStage1Step, WaeStep
    for cls in (Stage1Step, CognitiveStep, WaeStep, DualStage1Step):
        p = inspect.signature(cls.__init__).parameters
        assert "monitor" in p and p["monitor"].default is False, cls
        assert callable(getattr(cls, "numerics")) and callable(getattr(cls, "numerics_block"))
