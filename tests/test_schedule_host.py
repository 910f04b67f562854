"""CPU-side checks of the device-side epoch-end schedule's arithmetic: the inline code of include/fmri_hip.h that the
kernel runs, reached through the host entry point fmri_schedule_seek_host, against the reference's epoch-end block
written out in Python floats (tests/schedule_oracle.py).  Doubles are compared with ``==``, and so are their fp32
roundings: both sides form the same IEEE products in the same order.  No kernels are launched here."""
import ctypes as C
import inspect

import numpy as np
import pytest

import schedule_oracle as O


@pytest.fixture(scope="module")
def L():
    from fmri_hip import build, lib
    build.build(verbose=False)
    return lib.load()


def _sched(base, lr_gamma=1.0, lr_step=1, decay_margin=1.0, decay_equilibrium=1.0, decay_mse=1.0):
    from fmri_hip import lib
    s = lib.Schedule()
    assert C.sizeof(s) == 160
    for i, v in enumerate(base["lr"]):
        s.lr_base[i] = s.lr[i] = v
    s.margin_base = s.margin = base["margin"]
    s.equilibrium_base = s.equilibrium = base["equilibrium"]
    s.lambda_mse_base = s.lambda_mse = base["lambda_mse"]
    s.lr_gamma, s.lr_step = lr_gamma, lr_step
    s.decay_margin, s.decay_equilibrium, s.decay_mse = decay_margin, decay_equilibrium, decay_mse
    return s


def _seek(L, s, epoch):
    out = (C.c_float * 7)()
    assert L.fmri_schedule_seek_host(C.byref(s), epoch, out) == 0
    assert s.applied_epoch == epoch
    return np.array(out, dtype=np.float32)


def _check(s, out7, want, n_lr, what):
    for i in range(n_lr):
        assert s.lr[i] == want["lr"][i], (what, i, s.lr[i], want["lr"][i])
        assert out7[i] == O.f32(want["lr"][i]), (what, i)
    for k, name in ((4, "lambda_mse"), (5, "equilibrium"), (6, "margin")):
        assert getattr(s, name) == want[name], (what, name, getattr(s, name), want[name])
        assert out7[k] == O.f32(want[name]), (what, name)


CASES = {
    "stage1": (O.GAN_BASE, O.STAGE1_DECAYS),
    "steplr30": (O.GAN_BASE, dict(lr_gamma=0.5, lr_step=30)),
    # margin decays more slowly than equilibrium: 0.35 * 0.99^e overtakes 0.68 * 0.9^e at e = 7
    "margin_clamp": (O.GAN_BASE, dict(lr_gamma=0.98, decay_margin=0.99, decay_equilibrium=0.9)),
    # 0.5 * 1.1^e passes 1 at e = 8
    "mse_cap": (dict(O.GAN_BASE, lambda_mse=0.5), dict(lr_gamma=0.98, decay_mse=1.1)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_header_arithmetic_equals_the_python_float_loop(L, case):
    base, dec = CASES[case]
    s = _sched(base, **dec)
    v = dict(base, lr=list(base["lr"]))
    for e in range(0, 201):
        if e:
            v = O.epoch_end(v, e, **dec)                 # the running loop: epoch after epoch, as the script does
        _check(s, _seek(L, s, e), v, 3, (case, e))
    assert v == O.at(base, 200, **dec)


def test_both_clamps_fire_in_the_reference_loop_alone(L):
    """The inputs of the two clamp cases reach the clamps in the Python loop itself (checked here without the library),
    and the lr of the StepLR case moves at multiples of 30 only."""
    base, dec = CASES["margin_clamp"]
    free_m = [base["margin"] * dec["decay_margin"] ** e for e in range(201)]
    free_e = [base["equilibrium"] * dec["decay_equilibrium"] ** e for e in range(201)]
    first = next(e for e in range(201) if free_m[e] > free_e[e])
    assert 0 < first < 200
    v = O.at(base, first, **dec)
    assert v["equilibrium"] == v["margin"] and O.at(base, first - 1, **dec)["equilibrium"] > O.at(base, first - 1, **dec)["margin"]
    assert O.at(base, 200, **dec)["equilibrium"] == O.at(base, 200, **dec)["margin"]
    base, dec = CASES["mse_cap"]
    vals = [O.at(base, e, **dec)["lambda_mse"] for e in range(201)]
    assert vals[0] == 0.5 and max(vals) == 1 and vals[200] == 1 and 0.5 * 1.1 ** 8 > 1 > vals[7]
    base, dec = CASES["steplr30"]
    lrs = [O.at(base, e, **dec)["lr"][0] for e in range(201)]
    assert lrs[29] == 1e-4 and lrs[30] == 0.5e-4 == lrs[59] and lrs[60] == 0.25e-4 and lrs[200] == 1e-4 * 0.5 ** 6


@pytest.mark.parametrize("case", sorted(CASES))
def test_restart_path(L, case):
    """Forward to 50, back to 7 (a restart from the base values), forward to 20: each equals the direct evaluation."""
    base, dec = CASES[case]
    s = _sched(base, **dec)
    for e in (50, 7, 20, 20, 0, 3):
        _check(s, _seek(L, s, e), O.at(base, e, **dec), 3, (case, e))
        d = _sched(base, **dec)
        _seek(L, d, e)
        assert bytes(d) == bytes(s), (case, e)


def test_bad_arguments_are_refused(L):
    s = _sched(O.GAN_BASE)
    assert L.fmri_schedule_seek_host(None, 3, None) == -1
    assert L.fmri_schedule_seek_host(C.byref(s), -1, None) == -1
    s.lr_step = 0
    assert L.fmri_schedule_seek_host(C.byref(s), 3, None) == -1
    z, odd = C.c_void_p(64), C.c_void_p(68)
    assert L.fmri_epoch_begin(None, z, None, None, None, None, None, None, None) == -1
    assert L.fmri_epoch_begin(z, None, None, None, None, None, None, None, None) == -1       # nothing to do
    assert L.fmri_epoch_begin(odd, z, None, None, None, None, None, None, None) == -1        # state not 8-byte aligned
    assert L.fmri_epoch_begin(z, odd, None, None, None, None, None, None, None) == -1
    assert L.fmri_epoch_begin(z, z, C.c_void_p(66), None, None, None, None, None, None) == -1
    assert L.fmri_trainlog_append(None, z, 4, z, 8, z, None) == -1
    assert L.fmri_trainlog_append(z, z, 0, z, 8, z, None) == -1
    assert L.fmri_trainlog_append(z, z, 65, z, 8, z, None) == -1                             # one wave of columns
    assert L.fmri_trainlog_append(z, z, 4, z, 0, z, None) == -1
    assert L.fmri_trainlog_append(z, z, 4, z, 8, odd, None) == -1                            # counter not 8-byte aligned


def test_python_surface():
    """The four fused steps gain ``schedule=None`` / ``log=None``; the schedule validates its own arguments (no GPU)."""
    from fmri_hip.schedule import EpochSchedule, TrainLog
    from fmri_hip.steps import CognitiveStep, Stage1Step
    from fmri_hip.wae_steps import DualStage1Step, WaeStep
    for cls in (Stage1Step, CognitiveStep, WaeStep, DualStage1Step):
        p = inspect.signature(cls.__init__).parameters
        assert p["schedule"].default is None and p["log"].default is None, cls.__name__
        for name in ("history", "epoch_means"):
            assert callable(getattr(cls, name))
    d = inspect.signature(EpochSchedule.__init__).parameters
    assert [d[k].default for k in ("lr_gamma", "lr_step", "decay_margin", "decay_equilibrium", "decay_mse", "lr_mask")] \
        == [1.0, 1, 1.0, 1.0, 1.0, None]
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            EpochSchedule(lr_step=bad)
    with pytest.raises(ValueError):
        TrainLog(capacity=0)
    with pytest.raises(RuntimeError):
        EpochSchedule().values()
