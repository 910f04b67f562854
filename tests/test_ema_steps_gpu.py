"""The weight average through the fused steps (fmri_hip/ema.py, ``ema=`` / ``ema_state_dict()`` / ``swapped()``,
``Evaluator(weights="ema")``): px64, B = 4, recipe weights with ``perturb=True``, a DeviceRng -- the fed steps of
tests/schedule_cases.py (a pool of 12 images) plus Stage III.  Everything is compared bit for bit: against the numpy fp32
oracle (tests/ema_oracle.py) where the formula is checked, engine against engine (``selfcheck``) elsewhere."""
import numpy as np
import pytest
import torch

import ema_oracle as EO
from schedule_cases import DEV, V, _fed, _finish, _fmri

pytestmark = pytest.mark.gpu

STEPS = 3


def _make(kind, ema=None, fed=True, **kw):
    from fmri_hip.params import ArchConfig
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import CognitiveStep, Stage1Step
    from fmri_hip.wae_steps import DualStage1Step, WaeStep
    cfg = ArchConfig.px64()
    if fed:
        kw["rng"], kw["feed"] = _fed(_fmri() if kind in ("stage2", "stage3") else None)
    else:
        kw["rng"] = DeviceRng(7, DEV)
    if ema is not None:
        kw["ema"] = ema
    if kind == "stage1":
        st, seed = Stage1Step(cfg, DEV, **kw), 0
    elif kind in ("stage2", "stage3"):
        st, seed = CognitiveStep(cfg, V, DEV, int(kind[-1]), **kw), 3
    elif kind == "wae1":
        st, seed = WaeStep(cfg, DEV, 1, **kw), 5
    else:
        st, seed = DualStage1Step(cfg, DEV, **kw), 8
    st.load_recipe(seed, True)
    return st


def _cpu(sd):
    return {k: v.detach().cpu() for k, v in sd.items()}


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _shadowed_keys(st):
    return {key for entries in st.ema.layout().values() for key, _, _, _ in entries}


def _recurrence(st, steps=STEPS, t0=0):
    """After every step: every shadowed entry of ``ema_state_dict()`` is the oracle's update of the previous one with the
    live ``state_dict()`` and ``decay_at(t)``, bit for bit; every other entry is the live one."""
    ema, keys = st.ema, _shadowed_keys(st)
    prev = _cpu(st.ema_state_dict())
    for t in range(t0, t0 + steps):
        st.step()
        _finish()
        live, cur = _cpu(st.state_dict()), _cpu(st.ema_state_dict())
        assert list(live) == list(cur)
        d = EO.decay_at(t, ema.start, ema.decay, ema.warmup)
        moved = 0
        for k in live:
            assert cur[k].dtype == live[k].dtype and cur[k].shape == live[k].shape, k
            if k in keys:
                want = torch.from_numpy(EO.update(prev[k].numpy(), live[k].numpy(), d))
                assert torch.equal(_bits(cur[k]), _bits(want)), (t, k)
                moved += int(not torch.equal(cur[k], live[k]))
            else:
                assert torch.equal(cur[k], live[k]), (t, k)
        assert moved > 0 or float(d) == 0, (t, moved)                    # an average, not a copy
        prev = cur
    assert st.ema.state.tolist()[0] == t0 + steps
    return keys


def _prefixes(keys):
    return sorted({k.split(".")[0] for k in keys})


CASES = [("stage1", {}, ["decoder", "encoder"]), ("stage2", {}, ["encoder"]), ("stage3", {}, ["decoder"]),
         ("wae1", {}, ["decoder", "encoder"]), ("dual1", {}, ["decoder", "encoder"]),
         ("stage1", dict(start=1), ["decoder", "encoder"]),
         ("stage1", dict(nets=("encoder", "decoder", "discriminator")), ["decoder", "discriminator", "encoder"]),
         ("dual1", dict(nets=("wae_discriminator",), decay=0.5, warmup=False), ["wae_discriminator"])]


@pytest.mark.parametrize("kind,kw,nets", CASES, ids=[f"{k}-{'-'.join(kw) or 'default'}" for k, kw, _ in CASES])
def test_shadows_follow_the_recurrence(deterministic, kind, kw, nets):
    from fmri_hip.ema import WeightEma
    st = _make(kind, WeightEma(**kw))
    keys = _recurrence(st)
    assert _prefixes(keys) == nets
    assert not any(k.endswith("num_batches_tracked") for k in keys)
    if nets != ["wae_discriminator"]:
        assert any(k.endswith("running_mean") for k in keys) and any(k.endswith("running_var") for k in keys)
    if "decoder" in nets:
        assert "decoder.fc.1.running_mean" in keys                      # the lazy, engine-order BatchNorm
    with pytest.raises(ValueError, match="already attached"):
        _make(kind, st.ema)


def test_a_frozen_network_has_no_average():
    from fmri_hip.ema import WeightEma
    with pytest.raises(ValueError, match="does not train"):
        _make("stage2", WeightEma(nets=("decoder",)))
    with pytest.raises(ValueError, match="does not train"):
        _make("stage1", WeightEma(nets=("wae_discriminator",)))


def test_the_average_runs_whether_or_not_the_gate_lets_the_update_happen(deterministic):
    """equilibrium = 100 with the margin it has: every BCE term is below equilibrium - margin, the gate switches the
    discriminator off (and, both being off otherwise, leaves the decoder on) -- its masters stand still, its shadows
    still move towards them."""
    from fmri_hip.ema import WeightEma
    st = _make("stage1", WeightEma(decay=0.5, warmup=False, nets=("encoder", "decoder", "discriminator")))
    _recurrence(st, 1)
    st.set_hyper(equilibrium=100.0)
    before = _cpu(st.state_dict())
    _recurrence(st, 2, t0=1)
    logs, after = st.logs(), _cpu(st.state_dict())
    assert logs["train_dis"] is False and logs["train_dec"] is True
    assert all(torch.equal(before[k], after[k]) for k in before if k.startswith("discriminator.") and "running" not in k
               and "num_batches" not in k)
    ema_sd = _cpu(st.ema_state_dict())
    assert any(not torch.equal(ema_sd[k], after[k]) for k in after if k.startswith("discriminator.conv"))


def _training(st):
    out = _cpu(st.state_dict())
    for i, o in enumerate(st.optims):
        for name in ("s1", "s2", "lr_dev", "t_dev"):
            t = getattr(o, name)
            if t is not None:
                out[f"optim{i}.{name}"] = t.detach().cpu()
    out["rng"], out["feed"], out["scal"] = st.rng._state.cpu(), st.feed._state.cpu(), st.scal.cpu()
    return out


@pytest.mark.selfcheck
@pytest.mark.parametrize("kind", ["stage1", "wae1"])
def test_the_average_is_read_only_on_training(deterministic, kind):
    from fmri_hip.ema import WeightEma
    runs = []
    for ema in (WeightEma(nets=("encoder", "decoder", "discriminator")), None):
        st = _make(kind, ema)
        for _ in range(STEPS):
            st.step()
        _finish()
        runs.append((_training(st), st.logs()))
    (a, la), (b, lb) = runs
    assert a.keys() == b.keys() and la == lb
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.selfcheck
def test_launch_modes_give_the_same_shadows(deterministic):
    """Four steps on one static batch -- eager, capture_forward (two warm-up steps + two runs) and capture() (two warm-up
    steps + two replays): shadows and the state block are bit-identical."""
    from fmri_hip.ema import WeightEma
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(DEV)
    got = {}
    for mode in ("eager", "capture_forward", "capture"):
        st = _make("stage1", WeightEma(decay=0.9, nets=("encoder", "decoder", "discriminator")), fed=False)
        if mode == "eager":
            for _ in range(4):
                st.step(x)
        else:
            run = st.capture_forward(x) if mode == "capture_forward" else st.capture(x)
            run()
            run()
        _finish()
        got[mode] = {k: v.cpu() for k, v in st.ema.state_tensors().items()}
        assert got[mode]["ema:state"].tolist()[0] == 4
    for mode in ("capture_forward", "capture"):
        assert got[mode].keys() == got["eager"].keys()
        for k, v in got["eager"].items():
            assert torch.equal(_bits(v), _bits(got[mode][k])), (mode, k)


def _val():
    from fmri_hip.feed import DeviceDataset
    u8 = torch.randint(0, 256, (8, 64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    return DeviceDataset(u8.to(DEV))


def _packed(st):
    return [pw.buf.cpu() for n in st._state_nets() for pw in n.group.packed]


@pytest.mark.selfcheck
def test_an_ema_pass_is_a_live_pass_of_the_averaged_weights_and_leaves_training_alone(deterministic):
    """A (``ema=``, recorded: two warm-up steps and one replay) evaluates with ``weights="ema"``; B, without, is loaded
    with ``A.ema_state_dict()`` and evaluates live from the same generator seed: the same row and last output.
    Afterwards A's state, packed fp16 copies and three further replays are bit for bit those of a twin that never
    evaluated -- a recorded step looks at no version counter, so the exit of ``swapped()`` has to restore them."""
    from fmri_hip.ema import WeightEma
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.params import ArchConfig
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import Stage1Step
    va = _val()
    a, twin = (_make("stage1", WeightEma(decay=0.5, warmup=False)) for _ in range(2))
    ra, rt = a.capture(), twin.capture()
    ra()
    rt()
    b = Stage1Step(ArchConfig.px64(), DEV)
    b.load_state_dict(a.ema_state_dict())
    ev_a = Evaluator(a, va, batch=4, rng=DeviceRng(31, DEV), weights="ema")
    ev_b = Evaluator(b, va, batch=4, rng=DeviceRng(31, DEV))
    ev_live = Evaluator(a, va, batch=4, rng=DeviceRng(31, DEV))
    ev_a.run()
    ev_b.run()
    ev_live.run()
    ha, hb, hl = ev_a.history(), ev_b.history(), ev_live.history()
    assert list(ha) == ["epoch"] + list(hb)
    for k in hb:
        assert np.array_equal(ha[k], hb[k], equal_nan=True), (k, ha[k], hb[k])
    assert torch.equal(ev_a.last_output(), ev_b.last_output())
    assert not torch.equal(ev_a.last_output(), ev_live.last_output()) and ha["mean_MSE"] != hl["mean_MSE"]
    _finish()
    sa, stw = _cpu(a.state_dict()), _cpu(twin.state_dict())
    for k in sa:
        assert torch.equal(sa[k], stw[k]), k
    pa, pt = _packed(a), _packed(twin)
    assert len(pa) == len(pt) > 10 and all(torch.equal(u, v) for u, v in zip(pa, pt))
    for _ in range(3):
        ra()
        rt()
    _finish()
    ta, tt = _training(a), _training(twin)
    for k in ta:
        assert torch.equal(ta[k], tt[k]), k
    for (k, u), v in zip(a.ema.state_tensors().items(), twin.ema.state_tensors().values()):
        assert torch.equal(_bits(u), _bits(v)), k
    assert all(torch.equal(u, v) for u, v in zip(_packed(a), _packed(twin)))


def test_the_state_ring_carries_the_shadows(deterministic, tmp_path):
    from fmri_hip.ema import WeightEma
    from fmri_hip.state import StateRing, TrainState
    mk = lambda: _make("stage1", WeightEma(decay=0.9, start=1), checkpoints=StateRing(every=None))
    a = mk()
    for _ in range(2):
        a.step()
    a.snapshot()
    at_snapshot = _cpu(a.ema_state_dict())
    for _ in range(2):
        a.step()
    _finish()
    want = {k: v.cpu() for k, v in a.ema.state_tensors().items()}
    want_sd = _cpu(a.ema_state_dict())
    state = a.checkpoints.states()[-1]
    assert any(line.startswith("ema=0.9,True,1,encoder+decoder") for line in state.meta["signature"])
    assert {"ema:state", "ema:group:encoder.data", "ema:buf:decoder.fc.1.running_mean"} <= set(state.engine)
    path = tmp_path / "state.pt"
    state.save(path)
    loaded = TrainState.load(path)
    assert loaded.engine["ema:state"].tolist() == [2, 1, state.engine["ema:state"].tolist()[2], 1]
    # a saved snapshot exports its averaged weights without a GPU
    exported = WeightEma.state_dict_of(loaded)
    assert list(exported) == list(at_snapshot)
    for k, v in at_snapshot.items():
        assert exported[k].dtype == v.dtype and exported[k].shape == v.shape and torch.equal(_bits(exported[k]), _bits(v)), k
    # the same step, and a fresh one with other weights: restore, the same two steps again
    for c in (a, mk()):
        if c is not a:
            c.load_recipe(41, True)
            c.step()
        c.restore(loaded)
        for _ in range(2):
            c.step()
        _finish()
        for k, v in c.ema.state_tensors().items():
            assert torch.equal(_bits(v.cpu()), _bits(want[k])), k
        got_sd = _cpu(c.ema_state_dict())
        for k, v in want_sd.items():
            assert torch.equal(_bits(got_sd[k]), _bits(v)), k
    # with and without ema= are different makes of step: the first difference names the ema= line
    plain = _make("stage1", checkpoints=StateRing(every=None))
    with pytest.raises(ValueError, match="ema="):
        plain.restore(loaded)
    plain.snapshot()
    with pytest.raises(ValueError, match="ema="):
        a.restore(plain.checkpoints.states()[-1])
    with pytest.raises(ValueError, match="without ema="):
        WeightEma.state_dict_of(plain.checkpoints.states()[-1])


def test_error_paths():
    from fmri_hip.ema import WeightEma
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.rng import DeviceRng
    plain = _make("stage1")
    with pytest.raises(ValueError, match="ema="):
        Evaluator(plain, _val(), batch=4, rng=DeviceRng(1, DEV), weights="ema")
    with pytest.raises(ValueError, match="weights"):
        Evaluator(plain, _val(), batch=4, rng=DeviceRng(1, DEV), weights="average")
    with pytest.raises(RuntimeError, match="ema="):
        plain.ema_state_dict()
    st = _make("stage1", WeightEma())
    fw = st.forward(st._fed(None)[0])
    st.gate(fw["B"])
    st.backward(early_apply=True)
    before = {k: v.clone() for k, v in st.ema.state_tensors().items()}
    with pytest.raises(RuntimeError, match="apply"):
        with st.ema.swapped():
            pass
    st.apply()
    _finish()
    for k, v in st.ema.state_tensors().items():
        if k.startswith("ema:group:decoder") or k == "ema:state":
            assert torch.equal(v, before[k]), k              # the refused swap moved nothing
