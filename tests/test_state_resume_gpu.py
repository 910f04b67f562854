"""Snapshot and bit-exact resume of the fused steps (fmri_hip/state.py, ``checkpoints=`` / ``snapshot()`` / ``restore()``).

The steps are the fed steps of tests/schedule_cases.py -- a pool of 12 images in batches of 4, three steps per epoch, the
strong decays of DECAYS, ``log=TrainLog(64)`` -- under deterministic reductions; everything is compared bit for bit.

    A   straight: 9 steps
    B   5 steps (mid-epoch: the next batch is (epoch 1, cursor 8)), snapshot() -> states() -> save -> load
    C   another step of the same kind with other weights, generator and feed seeds, restore(), 4 steps

A and C must agree in every piece of state a tenth step would read."""
import numpy as np
import pytest
import torch

from schedule_cases import DECAYS, DEV, PER_EPOCH, _finish, _make

pytestmark = pytest.mark.gpu

KINDS = ("stage1", "stage2", "wae1", "dual1")
GAN = {"stage1", "stage2", "dual1"}
HEAD, TAIL = 5, 4


def _step(kind, ring="manual", **kw):
    from fmri_hip.schedule import EpochSchedule, TrainLog
    from fmri_hip.state import StateRing
    decays = DECAYS if kind in GAN else dict(lr_gamma=DECAYS["lr_gamma"])       # a WAE step has only rates to decay
    if isinstance(ring, str):
        ring = StateRing(every=None)
    kw.setdefault("log", TrainLog(64))
    return _make(kind, EpochSchedule(**decays), checkpoints=ring, **kw)


def _other_seeds(st):
    """Other weights, another generator seed and offset, another permutation key and position: nothing of the run to be
    restored is there by construction -- and one step from there, so that the optimizers, the BatchNorm statistics and the
    log hold another run's values."""
    st.load_recipe(41, True)
    st.rng.seed(1001, 55)
    st.feed._seed = 77
    st.feed.set_position(3, 4)
    st.step()
    _finish()
    return st


def _run(st, n, fn=None):
    for _ in range(n):
        (fn or st.step)()
    _finish()
    return st


_STRAIGHT, _SAVED = {}, {}


def _straight(kind):
    """Run A, once per kind (callers hold the ``deterministic`` fixture)."""
    if kind not in _STRAIGHT:
        _STRAIGHT[kind] = _run(_step(kind), HEAD + TAIL)
    return _STRAIGHT[kind]


def _saved(kind, tmp_path_factory):
    """Run B's state through a file, once per kind, and B's own ``state_dict()`` at that point."""
    if kind not in _SAVED:
        from fmri_hip.state import TrainState
        b = _run(_step(kind), HEAD)
        b.snapshot()
        states = b.checkpoints.states()
        assert len(states) == 1
        path = tmp_path_factory.mktemp("state") / f"{kind}.pt"
        states[-1].save(path)
        _SAVED[kind] = (TrainState.load(path), {k: v.cpu() for k, v in b.state_dict().items()})
    return _SAVED[kind]


def _assert_same_run(a, c, what):
    sa, sc = a.state_dict(), c.state_dict()
    assert list(sa) == list(sc)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), (what, k)
    for i, (oa, oc) in enumerate(zip(a.optims, c.optims)):
        for name in ("s1", "s2", "lr_dev", "t_dev"):
            ta, tc = getattr(oa, name), getattr(oc, name)
            assert (ta is None) == (tc is None) and (ta is None or torch.equal(ta, tc)), (what, i, name)
        assert oa.lr == oc.lr and (oa.t_dev is None or oc.t == int(oc.t_dev.item())), (what, i)
    if hasattr(a, "hp_dev"):
        assert torch.equal(a.hp_dev, c.hp_dev), (what, a.hp_dev.tolist(), c.hp_dev.tolist())
    assert a.rng.state() == c.rng.state(), what
    assert a.feed.position() == c.feed.position() == (3, 0), what
    assert torch.equal(a.feed.last_indices(), c.feed.last_indices()), what
    ha, hc = a.history(), c.history()
    assert list(ha) == list(hc) and len(ha["step"]) == HEAD + TAIL
    for k in ha:
        np.testing.assert_array_equal(ha[k], hc[k], err_msg=f"{what}: history column {k}")


def _differs(a, c):
    sa, sc = a.state_dict(), c.state_dict()
    return [k for k in sa if not torch.equal(sa[k], sc[k])]


@pytest.mark.parametrize("kind", KINDS)
def test_a_restored_run_continues_bit_for_bit(deterministic, tmp_path_factory, kind):
    a = _straight(kind)
    st, b_model = _saved(kind, tmp_path_factory)
    assert (st.epoch, st.cursor, st.step) == (HEAD // PER_EPOCH, (HEAD % PER_EPOCH) * 4, HEAD) == (1, 8, 5)
    # .model: bitwise what state_dict() returned there, the reference's keys in its order
    assert list(st.model) == list(b_model)
    for k, v in b_model.items():
        assert st.model[k].dtype == v.dtype and st.model[k].shape == v.shape and torch.equal(st.model[k], v), k
    c = _other_seeds(_step(kind))
    c.restore(st)
    _assert_same_run(a, _run(c, TAIL), kind)
    # the control: the same resume with cold optimizers is another run -- at these sizes the state matters
    c.restore(st)
    for o in c.optims:
        o.s1.zero_()
    assert _differs(a, _run(c, TAIL)), kind


def test_restore_into_a_recorded_step(deterministic, tmp_path_factory):
    """capture() first, then restore(): the graph updates its packed fp16 weights and the decoder's engine-order BatchNorm
    statistics itself and looks at no version counter -- restore() has to leave both current."""
    a = _straight("stage1")
    st, _ = _saved("stage1", tmp_path_factory)
    c = _other_seeds(_step("stage1"))
    replay = c.capture()
    c.restore(st)
    _assert_same_run(a, _run(c, TAIL, replay), "recorded C")


def test_snapshot_between_replays(deterministic):
    """Run B recorded (two warm-up steps + three replays), snapshot() between replays; an eager step continues it."""
    a = _straight("stage1")
    b = _step("stage1")
    replay = b.capture()
    _run(b, HEAD - 2, replay)
    b.snapshot()
    replay()                                                         # the snapshot is enqueue-only: the run goes on
    st = b.checkpoints.states()[-1]
    assert (st.epoch, st.cursor, st.step) == (1, 8, 5)
    c = _step("stage1")
    c.restore(st)
    _assert_same_run(a, _run(c, TAIL), "snapshot between replays")
    _assert_same_run(a, _run(b, TAIL - 1, replay), "recorded straight")


def test_the_ring_inside_a_recorded_step(deterministic):
    """every = 2, capacity = 2, replayed through the first step of epoch 5: the ends of epochs 0, 2, 4 fired (slots 0, 1,
    0), epochs 1 and 3 never did -- the ring holds resume epochs 3 and 5, each bitwise the manual snapshot of an eager
    twin at that boundary."""
    from fmri_hip.state import StateRing
    st = _step("stage1", StateRing(capacity=2, every=2))
    replay = st.capture()
    _run(st, 5 * PER_EPOCH + 1 - 2, replay)
    got = st.checkpoints.states()
    assert [(s.epoch, s.cursor, s.step) for s in got] == [(3, 0, 9), (5, 0, 15)]
    twin = _step("stage1")
    done = 0
    for s in got:
        _run(twin, s.step - done)
        done = s.step
        sd = {k: v.cpu() for k, v in twin.state_dict().items()}
        twin.snapshot()
        t = twin.checkpoints.states()[-1]
        assert (t.epoch, t.cursor, t.step, t.fingerprint) == (s.epoch, s.cursor, s.step, s.fingerprint)
        assert list(s.model) == list(t.model) == list(sd) and list(s.engine) == list(t.engine)
        for k in sd:
            assert torch.equal(s.model[k], t.model[k]) and torch.equal(s.model[k], sd[k]), (s.epoch, k)
        for k in t.engine:
            assert torch.equal(s.engine[k], t.engine[k]), (s.epoch, k)
    assert {"opt:encoder.s1", "opt:discriminator.lr", "hp", "rng", "feed", "log", "log_epoch"} <= set(got[0].engine)


def _names(monkeypatch, st, steps=2):
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
        st.step()
    _finish()
    monkeypatch.setattr(lib, "call", real)
    return rec


def test_off_means_off(monkeypatch):
    from fmri_hip.schedule import TrainLog
    from fmri_hip.state import StateRing
    plain = _names(monkeypatch, _make("stage1"))
    assert _names(monkeypatch, _make("stage1", checkpoints=None)) == plain
    assert len(plain) > 100 and "fmri_state_copy" not in plain and plain[0] == "fmri_sampler_indices"
    assert _names(monkeypatch, _make("stage1", checkpoints=StateRing(every=None))) == plain
    assert _names(monkeypatch, _make("stage1", checkpoints=StateRing(2, every=2))) == ["fmri_state_copy"] + plain
    logged = _names(monkeypatch, _make("stage1", log=TrainLog(8), checkpoints=StateRing(2, every=2)))
    assert logged == ["fmri_epoch_begin", "fmri_state_copy"] + plain + ["fmri_trainlog_append"]
    for kind in ("stage2", "wae1", "dual1"):
        names = _names(monkeypatch, _make(kind))
        assert "fmri_state_copy" not in names and names == _names(monkeypatch, _make(kind, checkpoints=None)), kind
        assert _names(monkeypatch, _make(kind, checkpoints=StateRing(2, every=2))) == ["fmri_state_copy"] + names, kind


def test_errors_change_no_device_byte():
    from fmri_hip.params import ArchConfig
    from fmri_hip.schedule import TrainLog
    from fmri_hip.state import StateRing
    from fmri_hip.steps import Stage1Step
    with pytest.raises(ValueError, match="feed"):
        Stage1Step(ArchConfig.px64(), DEV, checkpoints=StateRing(capacity=2, every=5))
    src = _step("stage1")
    with pytest.raises(ValueError, match="attached"):
        _step("stage1", src.checkpoints)
    src.snapshot()
    st = src.checkpoints.states()[-1]
    assert (st.epoch, st.cursor, st.step) == (0, 0, 0)
    with pytest.raises(RuntimeError, match="checkpoints"):
        _make("stage1").restore(st)
    # half a step is no state: between backward() and apply() the encoder's weight gradients wait in their queue
    fw = src.forward(src._fed(None)[0])
    src.gate(fw["B"])
    src.backward(early_apply=True)
    with pytest.raises(RuntimeError, match="apply"):
        src.snapshot()
    src.apply()
    src.snapshot()
    _finish()
    for what, dst in (("class=", _step("dual1")), ("mode=", _step("stage1", mode="beta-vae")),
                      ("recon_level=", _step("stage1", recon_level=2)), ("log=", _step("stage1", log=TrainLog(32)))):
        _run(dst, 1)
        before = {k: v.clone() for k, v in dst._state_tensors().items()}
        with pytest.raises(ValueError, match=what):
            dst.restore(st)
        _finish()
        for k, v in dst._state_tensors().items():
            assert torch.equal(v, before[k]), (what, k)
    # a state with a tensor of another shape is refused as well, before anything is copied
    dst = _step("stage1")
    bad = type(st)(dict(st.model), dict(st.engine), st.meta)
    bad.engine["hp"] = torch.zeros(5)
    before = {k: v.clone() for k, v in dst._state_tensors().items()}
    with pytest.raises(ValueError, match="hp"):
        dst.restore(bad)
    for k, v in dst._state_tensors().items():
        assert torch.equal(v, before[k]), k
