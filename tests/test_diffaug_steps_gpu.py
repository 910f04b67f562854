"""``augment=DiffAugment(...)`` on the fused steps (fmri_hip/augment.py; px64, B = 4, deterministic reductions):
  * under the neutral table a step built with the keyword is bit for bit the step built without it -- the plumbing changes
    nothing but the transform;
  * with all three policies on, the Stage-I step and the Stage-III step agree with the CPU oracle whose discriminator
    sees the torch restatement of T (tests/diffaug_oracle.py) under the same table: the procedure and the bounds of
    tests/test_stage1_gpu.py / tests/test_stage23_gpu.py;
  * tables the step draws itself follow the noise convention: fresh per step and per replay, reproducible from the seed,
    restored with the generator, one advance per step."""
import numpy as np
import pytest
import torch

import diffaug_oracle as A
import gradcheck

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, V, H = 4, 256, 64
LOSS_RTOL = 1e-3
LOSS_KEYS = ("loss_encoder", "loss_decoder", "loss_discriminator", "nle", "kl", "mse", "bce_orig", "bce_pred",
             "bce_samp")


def _cfgs():
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    return O, O.ArchCfg.px64(), ArchConfig.px64()


_DATA = {}


def _data():
    if not _DATA:
        O, cfg_o, _ = _cfgs()
        d = O.synth_batch(B, cfg_o, n_voxels=V, seed=1234, steps=2)
        _DATA.update(x=d["x"], fmri=d["fmri"], noise=d["noise"], xd=d["x"].to(DEV), fd=d["fmri"].to(DEV),
                     nd=d["noise"].to(DEV))
    return _DATA


def _make(kind, **kw):
    from fmri_hip.steps import CognitiveStep, Stage1Step
    from fmri_hip.wae_steps import DualStage1Step
    _, _, cfg = _cfgs()
    if kind in ("vae-gan", "dcgan"):
        st = Stage1Step(cfg, DEV, mode=kind, **kw)
    elif kind == "dual1":
        st = DualStage1Step(cfg, DEV, **kw)
    else:
        st = CognitiveStep(cfg, V, DEV, 2 if kind == "stage2" else 3, **kw)
    st.load_recipe(3, True)
    return st


def _args(kind, s):
    d = _data()
    nz = d["nd"][s]
    if kind in ("vae-gan", "dcgan"):
        return (d["xd"], nz[0], nz[1])
    if kind == "dual1":
        return (d["xd"], nz[0], nz[1], nz[2])
    return (d["fd"], d["xd"], nz[0], nz[1], nz[2])


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-12)


@pytest.mark.parametrize("kind", ["vae-gan", "dcgan", "dual1", "stage2", "stage3"])
def test_neutral_table_changes_nothing(deterministic, kind):
    from fmri_hip.augment import DiffAugment
    plain, aug = _make(kind), _make(kind, augment=DiffAugment())
    neutral = DiffAugment.neutral(B, DEV)
    assert plain.last_augment() is None
    for s in range(2):
        plain.step(*_args(kind, s))
        aug.step(*_args(kind, s), aug=neutral)
        torch.cuda.synchronize()
        assert torch.equal(plain.scal, aug.scal), (kind, s, plain.logs(), aug.logs())
        assert torch.equal(plain.flags, aug.flags), (kind, s)
        assert aug.last_augment() is neutral
        # the discriminator saw a copy: the same real channels, zero pad lanes
        assert torch.equal(aug.fw["disc_aug"][..., :3], aug.fw["disc_in"][..., :3])
        assert not aug.fw["disc_aug"][..., 3:].any()
    sa, sb = plain.state_dict(), aug.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (kind, k)
    for oa, ob in zip(plain.optims, aug.optims):
        assert torch.equal(oa.s1, ob.s1)


def _patch_oracle(monkeypatch, O, table):
    """The oracle's discriminator sees T of its three inputs (rounded where the engine stores them, under the 16-bit
    storage model) under ``table``; nothing under oracle/ changes."""
    orig = O.discriminator_fwd

    def wrapped(P, pre, x_orig, x_pred, x_samp, *a, **k):
        q = lambda t: O._q(t, "images")
        return orig(P, pre, *A.torch_transform_3b(q(x_orig), q(x_pred), q(x_samp), table), *a, **k)
    monkeypatch.setattr(O, "discriminator_fwd", wrapped)


def _drawn_table(seed):
    t = A.step_table(seed, 0, B, H)
    assert (t[:, 7] == 32).all() and (t[:, :3] != A.NEUTRAL[:3]).all()          # every policy is on
    return t


def _stage1_case(table):
    """One Stage-I step of the engine (``table`` None: built without the keyword) and of the oracle as it stands -- fp32,
    and under its 16-bit storage model with the engine's ReLU masks pinned -> (engine logs, engine gradients, fp32 run,
    16-bit run)."""
    from fmri_hip.augment import DiffAugment
    O, cfg_o, _ = _cfgs()
    d = _data()
    if table is None:
        st = _make("vae-gan")
        st.forward(d["xd"], d["nd"][0, 0], d["nd"][0, 1])
    else:
        st = _make("vae-gan", augment=DiffAugment())
        st.forward(d["xd"], d["nd"][0, 0], d["nd"][0, 1], aug=torch.tensor(table, dtype=torch.float32, device=DEV))
        assert not torch.equal(st.fw["disc_aug"], st.fw["disc_in"])
    masks = gradcheck._engine_relu_masks(st)
    st.gate(B)
    st.backward()
    grads = {k: v.detach().cpu().clone() for k, v in st.named_grads().items()}
    st.apply()
    logs = st.logs()
    new_opts = lambda: {n: O.OptState(kind="rmsprop", lr=1e-4) for n in ("encoder", "decoder", "discriminator")}
    ref = O.stage1_step(O.fill_state(O.vaegan_spec(cfg_o), 3, True), new_opts(), d["x"], d["noise"][0, 0],
                        d["noise"][0, 1], cfg_o, keep_grads=True)
    with gradcheck.pinned(O, masks):
        ref16 = O.stage1_step(O.fill_state(O.vaegan_spec(cfg_o), 3, True), new_opts(), d["x"], d["noise"][0, 0],
                              d["noise"][0, 1], cfg_o, keep_grads=True)
    return logs, grads, ref, ref16


def test_stage1_step_with_augmentation_matches_the_oracle(deterministic, monkeypatch):
    """test_stage1_step_matches_oracle's procedure (tests/test_stage1_gpu.py) with all three policies on: logged losses
    to 1e-3, the same gate flags, gradients under gradcheck's bounds with the engine's ReLU masks pinned.

    The 16-bit bound.  gradcheck's TOL16 = 1e-2 was set on the un-augmented step; with the transform in front of the
    discriminator the encoder's gradients -- the end of the longest fp16 chain, now one stored cotangent longer and with a
    quarter of every image cut out of the signal -- read 0.96e-2 .. 1.04e-2 against it, uniformly over the encoder's
    tensors (profiles/diffaug.md).  As stated for this case, the un-augmented step of the same inputs is measured in the
    same call and TWICE its worst 16-bit error is the bound here; the cosine and projection bounds stay gradcheck's."""
    O, _, _ = _cfgs()
    p_logs, p_grads, p_ref, p_ref16 = _stage1_case(None)
    plain = gradcheck.check(p_grads, p_ref["grads"], p_ref16["grads"], "stage1 px64, same inputs, no augmentation")
    plain16 = max(r[1] for r in plain if r[4] >= 64)
    table = _drawn_table(21)
    _patch_oracle(monkeypatch, O, table)
    logs, grads, ref, ref16 = _stage1_case(table)
    for k in LOSS_KEYS:
        print("stage1+aug", k, logs[k], ref["logs"][k], _rel(logs[k], ref["logs"][k]))
    print(f"stage1+aug 16-bit bound: 2 x {plain16:.3e} (un-augmented worst) = {2 * plain16:.3e}")
    assert logs["train_dis"] == ref["logs"]["train_dis"] and logs["train_dec"] == ref["logs"]["train_dec"]
    for k in LOSS_KEYS:
        assert _rel(logs[k], ref["logs"][k]) < LOSS_RTOL, (k, logs[k], ref["logs"][k])
    gradcheck.check(grads, ref["grads"], ref16["grads"], "stage1 px64 + diffaug", tol16=2 * plain16)


def test_stage3_step_with_augmentation_matches_the_oracle(deterministic, monkeypatch):
    """The Stage-III procedure of tests/test_stage23_gpu.py with all three policies on."""
    import test_stage23_gpu as S23
    from fmri_hip.augment import DiffAugment
    O, cfg_o, _ = _cfgs()
    d = _data()
    table = _drawn_table(22)
    st = _make("stage3", augment=DiffAugment())
    rec = gradcheck.Recorder(st)
    nz = d["nd"][0]
    st.forward(d["fd"], d["xd"], nz[0], nz[1], nz[2], aug=torch.tensor(table, dtype=torch.float32, device=DEV))
    masks = gradcheck.cognitive_masks(rec, B, False)       # (the discriminator's are those of the transformed images)
    st.gate(B)
    st.backward()
    grads = {k: v.cpu() for k, v in st.named_grads().items()}
    st.apply()
    logs = st.logs()
    _patch_oracle(monkeypatch, O, table)
    new_opts = lambda: {n: O.OptState(kind="rmsprop", lr=1e-4) for n in ("encoder", "decoder", "discriminator")}
    P, _ = S23._oracle_state(O, cfg_o, V, 3, True, 3)
    ref = O.stage3_step(P, new_opts(), d["fmri"], d["x"], d["noise"][0], cfg_o, V, keep_grads=True)
    for k in LOSS_KEYS:
        print("stage3+aug", k, logs[k], ref["logs"][k], _rel(logs[k], ref["logs"][k]))
    P16, _ = S23._oracle_state(O, cfg_o, V, 3, True, 3)
    with gradcheck.pinned(O, masks):
        ref16 = O.stage3_step(P16, new_opts(), d["fmri"], d["x"], d["noise"][0], cfg_o, V, keep_grads=True)
    assert logs["train_dis"] == ref["logs"]["train_dis"] and logs["train_dec"] == ref["logs"]["train_dec"]
    for k in LOSS_KEYS:
        assert _rel(logs[k], ref["logs"][k]) < LOSS_RTOL, (k, logs[k], ref["logs"][k])
    gradcheck.check(grads, ref["grads"], ref16["grads"], "stage3 + diffaug")


def _drawing_step(seed=5, **kw):
    from fmri_hip.augment import DiffAugment
    from fmri_hip.rng import DeviceRng
    return _make("vae-gan", augment=DiffAugment(), rng=DeviceRng(seed, DEV), **kw)


def _run_drawn(st, n, fn=None):
    x = _data()["xd"]
    tables, scals = [], []
    for _ in range(n):
        fn() if fn is not None else st.step(x)
        tables.append(st.last_augment().clone())
        scals.append(st.scal.clone())
    torch.cuda.synchronize()
    return tables, scals


def test_drawn_tables_follow_the_noise_convention(deterministic):
    _, _, cfg = _cfgs()
    Z = cfg.latent_dim
    a = _drawing_step()
    ta, sa = _run_drawn(a, 3)
    assert not torch.equal(ta[0], ta[1]) and not torch.equal(ta[1], ta[2])
    # ONE advance per step, by the larger of the noise draw's blocks and the table's: the tables are the oracle's at those offsets
    per_step = max(B * Z // 4, 2 * B)
    assert a.rng.offset() == 3 * per_step
    for s, t in enumerate(ta):
        assert t.cpu().numpy().tobytes() == A.step_table(5, s * per_step, B, H).astype(np.float32).tobytes(), s
    # a second object from the same seed reproduces tables and losses bit for bit
    tb, sb = _run_drawn(_drawing_step(), 3)
    for s in range(3):
        assert torch.equal(ta[s], tb[s]) and torch.equal(sa[s], sb[s]), s
    # handed all its noise, the step still draws its table -- and still advances, by the table's blocks
    d = _data()
    c = _drawing_step()
    c.step(d["xd"], d["nd"][0, 0], d["nd"][0, 1])
    assert torch.equal(c.last_augment(), ta[0]) and c.rng.offset() == 2 * B
    c.step(d["xd"], d["nd"][0, 0], d["nd"][0, 1], aug=ta[1])                  # a table passed in: used as it is, no advance
    assert c.last_augment() is ta[1] and c.rng.offset() == 2 * B


def test_recorded_step_draws_a_fresh_table_at_every_replay(deterministic):
    eager_t, eager_s = _run_drawn(_drawing_step(), 5)
    rec = _drawing_step()
    replay = rec.capture(_data()["xd"])               # two eager warm-up steps, then the recording
    got_t, got_s = _run_drawn(rec, 3, replay)
    for i in range(3):
        assert torch.equal(got_t[i], eager_t[2 + i]), i
        assert torch.equal(got_s[i], eager_s[2 + i]), i


def test_restored_step_redraws_the_same_tables(deterministic):
    from fmri_hip.state import StateRing
    a = _drawing_step(checkpoints=StateRing(every=None))
    _run_drawn(a, 1)
    a.snapshot()
    t1, s1 = _run_drawn(a, 2)
    sd1 = {k: v.clone() for k, v in a.state_dict().items()}
    a.restore(a.checkpoints.states()[-1])
    t2, s2 = _run_drawn(a, 2)
    for i in range(2):
        assert torch.equal(t1[i], t2[i]) and torch.equal(s1[i], s2[i]), i
    for k, v in a.state_dict().items():
        assert torch.equal(v, sd1[k]), k


def test_a_table_is_needed():
    from fmri_hip.augment import DiffAugment
    d = _data()
    st = _make("vae-gan", augment=DiffAugment())
    with pytest.raises(ValueError, match="aug not given"):
        st.step(d["xd"], d["nd"][0, 0], d["nd"][0, 1])
    with pytest.raises(ValueError, match="without augment"):
        _make("vae-gan").step(d["xd"], d["nd"][0, 0], d["nd"][0, 1], aug=DiffAugment.neutral(B, DEV))
    with pytest.raises(ValueError):
        st.step(d["xd"], d["nd"][0, 0], d["nd"][0, 1], aug=DiffAugment.neutral(B + 1, DEV))
    from fmri_hip.wae_steps import WaeStep
    import inspect
    assert "augment" not in inspect.signature(WaeStep.__init__).parameters
