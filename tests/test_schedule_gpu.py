"""GPU checks of the device-side epoch-end schedule (csrc/schedule.hip, fmri_hip/schedule.py, ``schedule=`` of the fused
steps) against the host path it replaces: the same fed step with the host calling ``set_hyper`` / ``set_lr`` at every epoch
boundary with Python-double decays (tests/schedule_oracle.py).  Everything is compared bit for bit (``torch.equal``): both
paths hand the kernels the fp32 rounding of the same doubles, and deterministic mode fixes every summation order.

A pool of 12 images in batches of 4 is three steps per epoch."""
import numpy as np
import pytest
import torch

import schedule_oracle as O
from schedule_cases import DECAYS, DEV, PER_EPOCH, _base, _fed, _finish, _make

pytestmark = pytest.mark.gpu


def _host_epoch_end(st, v, mask, gan):
    """What a port of the script does between two epochs: the oracle's doubles through the host interface."""
    for o, m, lr in zip(st.optims, mask, v["lr"]):
        if m:
            o.set_lr(lr)
    if gan:
        st.set_hyper(lambda_mse=v["lambda_mse"], equilibrium=v["equilibrium"], margin=v["margin"])


def _run_host(st, steps, decays, mask, gan=True, apply=True):
    base = _base(st, gan)
    for i in range(steps):
        e = i // PER_EPOCH
        if apply and i % PER_EPOCH == 0 and e > 0:
            _host_epoch_end(st, O.at(base, e, **decays), mask, gan)
        st.step()
    _finish()


def _same_state(a, b, what, gan=True):
    for i, (oa, ob) in enumerate(zip(a.optims, b.optims)):
        assert torch.equal(oa.lr_dev, ob.lr_dev), (what, "lr_dev", i, oa.lr_dev.item(), ob.lr_dev.item())
    if gan:
        assert torch.equal(a.hp_dev, b.hp_dev), (what, a.hp_dev.tolist(), b.hp_dev.tolist())
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (what, k)
        assert bool(torch.isfinite(sa[k]).all()), (what, k)


def _differs(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return [k for k in sa if not torch.equal(sa[k], sb[k])]


def _expect_dev(st, v, mask, gan=True):
    """The device values the kernels read equal the fp32 roundings of the oracle's doubles ``v``."""
    base = _base(st, gan)
    for i, (o, m) in enumerate(zip(st.optims, mask)):
        assert o.lr_dev.item() == O.f32(v["lr"][i] if m else base["lr"][i]), (i, o.lr_dev.item())
    if gan:
        got = st.hp_dev.cpu().numpy()
        want = np.array([v["lambda_mse"], v["equilibrium"], v["margin"], st.hp.beta], dtype=np.float32)
        assert np.array_equal(got, want), (got, want)


def test_recorded_stage1_schedule_equals_the_host_path(deterministic):
    """Run A: 8 eager steps, the host applying the epoch-end block in front of steps 3 and 6.  Run B: ``schedule=``,
    recorded with ``capture()`` (its two warm-up steps are steps 0 and 1) and replayed six times -- both boundaries fall
    into replays.  Run C: run A without the epoch-end block, which must differ (the decays matter at this size)."""
    from fmri_hip.schedule import EpochSchedule
    mask = (True, True, True)
    a = _make("stage1")
    _run_host(a, 8, DECAYS, mask)
    sched = EpochSchedule(**DECAYS)
    b = _make("stage1", sched)
    replay = b.capture()
    for _ in range(6):
        replay()
    _finish()
    assert b.feed.position() == (2, 8) and a.feed.position() == (2, 8)
    _same_state(a, b, "host path against the recorded schedule")
    want = O.at(_base(b), 2, **DECAYS)
    _expect_dev(b, want, mask)
    got = sched.values()
    assert got == dict(lr=want["lr"], margin=want["margin"], equilibrium=want["equilibrium"],
                       lambda_mse=want["lambda_mse"], applied_epoch=2), got
    assert got == sched.at(2)
    assert b.hp.lr == 1e-4 and b.hp.margin == 0.35                   # step.hp keeps the base values
    c = _make("stage1")
    _run_host(c, 8, DECAYS, mask, apply=False)
    assert _differs(a, c)                                           # without the block the weights are others


@pytest.mark.parametrize("kind,decays,mask", [
    ("stage2", DECAYS, None),
    ("wae1", dict(lr_gamma=0.5, lr_step=2), None),
    ("dual1", DECAYS, None),
    ("dual1", DECAYS, (True, True, False, True)),        # the script's literal behaviour (wae_vgan_stage1.py:246-250)
])
def test_schedule_equals_the_host_path_on_the_other_steps(deterministic, kind, decays, mask):
    """Eager steps over the first boundary -- for the WAE step with ``lr_step=2`` over two, since its rates move at the
    second only (7 steps: epochs 0 0 0 1 1 1 2)."""
    from fmri_hip.schedule import EpochSchedule
    gan = kind != "wae1"
    steps = 7 if kind == "wae1" else 4
    default = {"stage2": (True,) * 3, "wae1": (True,) * 3, "dual1": (True, True, True, False)}[kind]
    eff = default if mask is None else mask
    a = _make(kind)
    _run_host(a, steps, decays, eff, gan)
    b = _make(kind, EpochSchedule(lr_mask=mask, **decays))
    for _ in range(steps):
        b.step()
    _finish()
    _same_state(a, b, (kind, mask), gan)
    last = (steps - 1) // PER_EPOCH
    _expect_dev(b, O.at(_base(b, gan), last, **decays), eff, gan)
    if kind == "wae1":
        assert b.optims[0].lr_dev.item() == O.f32(0.5e-4) and b.optims[2].lr_dev.item() == O.f32(0.25e-4)
    assert b.schedule.values()["applied_epoch"] == last
    c = _make(kind)
    _run_host(c, steps, decays, eff, gan, apply=False)
    assert _differs(a, c)


def test_resume_puts_the_rates_where_the_epoch_has_them():
    from fmri_hip.schedule import EpochSchedule
    mask = (True,) * 3
    sched = EpochSchedule(**DECAYS)
    st = _make("stage1", sched)
    base = _base(st)
    st.step()
    _finish()
    _expect_dev(st, O.at(base, 0, **DECAYS), mask)
    for epoch, cursor in ((5, 0), (2, 4), (2, 8), (3, 0)):           # forward, back (a restart from the base), on
        st.feed.set_position(epoch, cursor)
        st.step()
        _finish()
        _expect_dev(st, O.at(base, epoch, **DECAYS), mask)
        want = O.at(base, epoch, **DECAYS)
        assert sched.values() == dict(want, applied_epoch=epoch), (epoch, sched.values())
    assert st.feed.position() == (3, 4)


def test_ownership_and_argument_errors():
    from fmri_hip.params import ArchConfig
    from fmri_hip.schedule import EpochSchedule
    from fmri_hip.steps import Stage1Step
    from fmri_hip.wae_steps import WaeStep
    cfg = ArchConfig.px64()
    st = _make("stage1", EpochSchedule(**DECAYS))
    for kw in (dict(lr=1e-3), dict(lambda_mse=1e-3), dict(equilibrium=0.5), dict(margin=0.1), dict(lr=1e-3, beta=2.0)):
        with pytest.raises(RuntimeError, match="EpochSchedule"):
            st.set_hyper(**kw)
    with pytest.raises(RuntimeError, match="EpochSchedule"):
        st.opt_enc.set_lr(1e-3)
    st.set_hyper(beta=2.0)                                          # not scheduled: works as ever
    assert st.hp.beta == 2.0 and st.hp_dev.tolist() == [O.f32(1e-6), O.f32(0.68), O.f32(0.35), 2.0]
    with pytest.raises(ValueError, match="feed"):
        Stage1Step(cfg, DEV, schedule=EpochSchedule(lr_gamma=0.98))
    g, feed = _fed()
    with pytest.raises(ValueError, match="margin"):
        WaeStep(cfg, DEV, 1, rng=g, feed=feed, schedule=EpochSchedule(lr_gamma=0.5, decay_margin=0.9))
    with pytest.raises(ValueError, match="lr_mask"):
        Stage1Step(cfg, DEV, rng=g, feed=feed, schedule=EpochSchedule(lr_mask=(True, True)))
    used = st.schedule
    with pytest.raises(ValueError, match="attached"):
        Stage1Step(cfg, DEV, rng=g, feed=feed, schedule=used)
    # the latent discriminator of the Dual step keeps its rate under the default mask and may still be set by hand
    d = _make("dual1", EpochSchedule(**DECAYS))
    d.opt_wd.set_lr(2e-4)
    assert d.opt_wd.lr_dev.item() == O.f32(2e-4)


def _names(monkeypatch, st, steps=2, **step_kw):
    """Entry-point names of the LAST of ``steps`` eager steps (the first one also packs weights)."""
    from fmri_hip import lib
    rec = []
    real = lib.call

    def spy(name, *args):
        rec.append(name)
        return real(name, *args)
    for i in range(steps):
        _finish()
        if i == steps - 1:
            monkeypatch.setattr(lib, "call", spy)
        st.step(**step_kw)
    _finish()
    monkeypatch.setattr(lib, "call", real)
    return rec


def test_off_means_off(monkeypatch):
    """A step built without the keywords, and one handed ``schedule=None, log=None``, issue the same launches, none of
    them new; with both on the sequence is the same with exactly one launch in front and one behind."""
    from fmri_hip.schedule import EpochSchedule, TrainLog
    new = {"fmri_epoch_begin", "fmri_trainlog_append"}
    plain = _names(monkeypatch, _make("stage1"))
    explicit = _names(monkeypatch, _make("stage1", None, log=None))
    assert plain == explicit and len(plain) > 100 and not new & set(plain)
    assert plain[0] == "fmri_sampler_indices"
    on = _names(monkeypatch, _make("stage1", EpochSchedule(**DECAYS), log=TrainLog(8)))
    assert on == ["fmri_epoch_begin"] + plain + ["fmri_trainlog_append"]
    logged = _names(monkeypatch, _make("stage1", None, log=TrainLog(8)))
    assert logged == on                                             # the log alone notes the epoch in the same launch
    scheduled = _names(monkeypatch, _make("stage1", EpochSchedule(**DECAYS)))
    assert scheduled == ["fmri_epoch_begin"] + plain
    for kind in ("stage2", "wae1", "dual1"):
        names = _names(monkeypatch, _make(kind))
        assert not new & set(names) and names == _names(monkeypatch, _make(kind, None, log=None)), kind
