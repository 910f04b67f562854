"""The fused Stage-I and Dual steps at ``recon_level`` 1 and 2 on the GPU: against the CPU oracle composed at that level
(tests/recon_oracle.py) and against golden vectors the real reference produced with ``VaeGan(recon_level=level)``
(tests/golden/make_golden_recon.py), at the bars tests/test_stage1_gpu.py and tests/test_wae_gpu.py hold level 3 to:
first-step losses 1e-3 relative, equal gate flags, gradients through tests/gradcheck.py, post-update parameter norms 2e-3.
B = 4 at 64 px (the fixtures), B = 5 once for a ragged batch.  Launch-mode comparisons run in deterministic mode and are
exact."""
import math
import os

import numpy as np
import pytest
import torch

import gradcheck
import recon_oracle as RO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_RTOL = 1e-3
GAN_KEYS = ("loss_encoder", "loss_decoder", "loss_discriminator", "nle", "kl", "mse", "bce_orig", "bce_pred", "bce_samp")
WAE_KEYS = ("loss_penalty", "loss_discriminator_fake", "loss_discriminator_real")
FEAT_SHAPE = {1: (32, 32, 128), 2: (16, 16, 256), 3: (8, 8, 256)}        # block ``level``'s raw output at 64 px (h, w, c)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-12)


def _terr(got, ref):
    got, ref = got.detach().float().cpu().reshape(-1), ref.detach().float().cpu().reshape(-1)
    return ((got - ref).norm() / (ref.norm() + 1e-20)).item()


def _opts(*names):
    from oracle import vaegan_oracle as O
    return {n: O.OptState(kind="rmsprop", lr=1e-4) for n in names}


def _check_state_against_golden(sd, g, level, tag="step0"):
    """Post-update parameter norms (2e-3) and BatchNorm counters of the reference's state after the step."""
    skeys = [str(k) for k in g[f"{tag}/state_keys"]]
    summ = g[f"{tag}/state_sum"]
    seen = 0
    for i, k in enumerate(skeys):
        if "num_batches" in k:
            assert float(sd[k]) == summ[i][1], (k, float(sd[k]), summ[i][1])
            seen += 1
        elif "running" not in k:
            got = sd[k].double().norm().item()
            assert _rel(got, summ[i][0]) < 2e-3, (k, got, summ[i][0])
    assert seen > 0
    # the 'REC' pass of the reference ends at block ``level``: two running-statistics updates up to it, one above
    for i in (1, 2, 3):
        assert int(sd[f"discriminator.conv.{i}.bn.num_batches_tracked"]) == (2 if i <= level else 1), (i, level)
    assert int(sd["discriminator.fc.1.num_batches_tracked"]) == 1


def test_level_below_three_constructs_and_steps():
    """Without the feature: ``recon_level`` is a TypeError of the constructor, and the two-stream backward of a
    discriminator at level < 3 a NotImplementedError."""
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import CognitiveStep, Stage1Step
    from fmri_hip.wae_steps import DualStage1Step
    B = 4
    data = O.synth_batch(B, O.ArchCfg.px64(), seed=1234, steps=1)
    st = Stage1Step(ArchConfig.px64(), DEV, recon_level=1)
    st.load_recipe(0, True)
    assert st.dis.level == 1
    st.step(data["x"].to(DEV), data["noise"][0, 0].to(DEV), data["noise"][0, 1].to(DEV))
    torch.cuda.synchronize()
    assert tuple(st.fw["feat"].shape) == (3 * B,) + FEAT_SHAPE[1] and st.fw["F"] == 131072
    assert all(math.isfinite(float(v)) for v in st.logs().values())
    assert st.outputs()["disc_layer"].shape == (3 * B, 131072)
    for lv in (0, 4):
        with pytest.raises(ValueError):
            Stage1Step(ArchConfig.px64(), DEV, recon_level=lv)
    assert DualStage1Step(ArchConfig.px64(), DEV, recon_level=2).dis.level == 2
    # the Stage-II / III scripts build their discriminator with the default level
    assert CognitiveStep(ArchConfig.px64(), 64, DEV, 3).dis.level == 3
    with pytest.raises(TypeError):
        CognitiveStep(ArchConfig.px64(), 64, DEV, 3, recon_level=2)
    # the parameters are the same at every level
    assert Stage1Step(ArchConfig.px64(), DEV).state_dict().keys() == st.state_dict().keys()


@pytest.mark.parametrize("name,level,mode,beta", [("stage1_rl1_b4", 1, "vae-gan", 1.0), ("stage1_rl2_b4", 2, "vae-gan", 1.0),
                                                  ("stage1_rl2_betavae_b4", 2, "beta-vae", 4.0)])
def test_stage1_levels_match_oracle_and_golden(golden_dir, name, level, mode, beta):
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import GanHyper, Stage1Step
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    B, seed, perturb = int(g["meta/B"]), int(g["meta/seed"]), bool(g["meta/perturb"])
    assert int(g["meta/recon_level"]) == level and str(g["meta/mode"]) == mode and float(g["meta/beta"]) == beta
    cfg_o = O.ArchCfg.px64()
    data = O.synth_batch(B, cfg_o, seed=1234, steps=int(g["meta/steps"]))
    st = Stage1Step(ArchConfig.px64(), DEV, hp=GanHyper(beta=beta), mode=mode, recon_level=level)
    st.load_recipe(seed, perturb)
    st.forward(data["x"].to(DEV), data["noise"][0, 0].to(DEV), data["noise"][0, 1].to(DEV))
    assert tuple(st.fw["feat"].shape) == (3 * B,) + FEAT_SHAPE[level]
    masks = gradcheck._engine_relu_masks(st)           # (17 + level: the 'REC' pass ends at block ``level``)
    st.gate(B)
    st.backward()
    grads = {k: v.detach().cpu().clone() for k, v in st.named_grads().items()}
    st.apply()
    logs = st.logs()
    P = O.fill_state(O.vaegan_spec(cfg_o), seed, perturb)
    ref = RO.stage1_step_level(level, P, _opts("encoder", "decoder", "discriminator"), data["x"], data["noise"][0, 0],
                               data["noise"][0, 1], cfg_o, keep_grads=True, mode=mode, beta=beta)
    assert logs["train_dis"] == ref["logs"]["train_dis"] and logs["train_dec"] == ref["logs"]["train_dec"]
    assert logs["train_dis"] == bool(g["step0/logs/train_dis"]) and logs["train_dec"] == bool(g["step0/logs/train_dec"])
    for k in GAN_KEYS:
        print(name, k, logs[k], ref["logs"][k], _rel(logs[k], ref["logs"][k]), _rel(logs[k], float(g[f"step0/logs/{k}"])))
    assert _terr(st.outputs()["disc_layer"], ref["fw"]["disc_layer"]) < 1e-2
    for k in GAN_KEYS:
        assert _rel(logs[k], ref["logs"][k]) < LOSS_RTOL, (k, logs[k], ref["logs"][k])
        assert _rel(logs[k], float(g[f"step0/logs/{k}"])) < LOSS_RTOL, (k, "golden")
    with gradcheck.pinned(O, masks):
        ref16 = RO.stage1_step_level(level, O.fill_state(O.vaegan_spec(cfg_o), seed, perturb),
                                     _opts("encoder", "decoder", "discriminator"), data["x"], data["noise"][0, 0],
                                     data["noise"][0, 1], cfg_o, keep_grads=True, mode=mode, beta=beta)
    gradcheck.check(grads, ref["grads"], ref16["grads"], f"stage1 level {level} {mode}")
    _check_state_against_golden({k: v.cpu() for k, v in st.state_dict().items()}, g, level)


def test_stage1_level2_ragged_batch_matches_oracle():
    """B = 5: not a multiple of the four-image tiles of the narrow layers, 15 / 30 rows in the stacked cotangent."""
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import Stage1Step
    B, level, seed = 5, 2, 1
    cfg_o = O.ArchCfg.px64()
    data = O.synth_batch(B, cfg_o, seed=1234, steps=1)
    st = Stage1Step(ArchConfig.px64(), DEV, recon_level=level)
    st.load_recipe(seed, True)
    st.forward(data["x"].to(DEV), data["noise"][0, 0].to(DEV), data["noise"][0, 1].to(DEV))
    masks = gradcheck._engine_relu_masks(st)
    st.gate(B)
    st.backward()
    grads = {k: v.detach().cpu().clone() for k, v in st.named_grads().items()}
    st.apply()
    logs = st.logs()
    P = O.fill_state(O.vaegan_spec(cfg_o), seed, True)
    ref = RO.stage1_step_level(level, P, _opts("encoder", "decoder", "discriminator"), data["x"], data["noise"][0, 0],
                               data["noise"][0, 1], cfg_o, keep_grads=True)
    assert logs["train_dis"] == ref["logs"]["train_dis"] and logs["train_dec"] == ref["logs"]["train_dec"]
    for k in GAN_KEYS:
        print("B=5", k, logs[k], ref["logs"][k], _rel(logs[k], ref["logs"][k]))
        assert _rel(logs[k], ref["logs"][k]) < LOSS_RTOL, (k, logs[k], ref["logs"][k])
    with gradcheck.pinned(O, masks):
        ref16 = RO.stage1_step_level(level, O.fill_state(O.vaegan_spec(cfg_o), seed, True),
                                     _opts("encoder", "decoder", "discriminator"), data["x"], data["noise"][0, 0],
                                     data["noise"][0, 1], cfg_o, keep_grads=True)
    gradcheck.check(grads, ref["grads"], ref16["grads"], "stage1 level 2 B=5")


def test_dual_stage1_level2_matches_oracle_and_golden(golden_dir):
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    from fmri_hip.wae_steps import DualStage1Step
    level = 2
    g = np.load(os.path.join(golden_dir, "dual1_rl2_b4.npz"))
    B, seed, perturb, lam = int(g["meta/B"]), int(g["meta/seed"]), bool(g["meta/perturb"]), float(g["meta/lam"])
    assert int(g["meta/recon_level"]) == level
    cfg_o = O.ArchCfg.px64()
    data = O.synth_batch(B, cfg_o, seed=1234, steps=int(g["meta/steps"]))
    st = DualStage1Step(ArchConfig.px64(), DEV, lam=lam, recon_level=level)
    st.load_recipe(seed, perturb)
    rec = gradcheck.Recorder(st)
    nz = data["noise"][0]
    st.step(data["x"].to(DEV), nz[0].to(DEV), nz[1].to(DEV), nz[2].to(DEV))
    logs = st.logs()
    grads = st.named_grads()

    def state():
        P = O.fill_state(O.vaegan_spec(cfg_o), seed, perturb)
        P.update(O.fill_state(O.wae_discriminator_spec(cfg_o, pre="wae_discriminator."), seed + 200, perturb))
        return P, _opts("encoder", "decoder", "discriminator", "wae_discriminator")
    P, opts = state()
    ref = RO.dual_stage1_step_level(level, P, opts, data["x"], nz, cfg_o, lam=lam, keep_grads=True)
    assert logs["train_dis"] == ref["logs"]["train_dis"] and logs["train_dec"] == ref["logs"]["train_dec"]
    assert logs["train_dis"] == bool(g["step0/logs/train_dis"]) and logs["train_dec"] == bool(g["step0/logs/train_dec"])
    for k in GAN_KEYS + WAE_KEYS:
        print("dual level 2", k, logs[k], ref["logs"][k], _rel(logs[k], ref["logs"][k]))
        assert _rel(logs[k], ref["logs"][k]) < LOSS_RTOL, (k, logs[k], ref["logs"][k])
        assert _rel(logs[k], float(g[f"step0/logs/{k}"])) < LOSS_RTOL, (k, "golden")
    P16, o16 = state()
    with gradcheck.pinned(O, gradcheck.dual_masks(rec, B, level)):
        ref16 = RO.dual_stage1_step_level(level, P16, o16, data["x"], nz, cfg_o, lam=lam, keep_grads=True)
    # (the latent discriminator's two passes cancel, tests/test_wae_gpu.py: plain bound)
    latent_d = [k for k in ref["grads"] if k.startswith("wae_discriminator.")]
    gradcheck.check(grads, ref["grads"], ref16["grads"], "dual1 level 2", skip=latent_d)
    for k in latent_d:
        assert _terr(grads[k], ref["grads"][k]) < 0.1, k
    _check_state_against_golden({k: v.cpu() for k, v in st.state_dict().items()}, g, level)


@pytest.mark.parametrize("mode", ["dcgan", "vae"])
def test_pixel_modes_at_level1_log_the_level1_feature_term(mode):
    """'dcgan' / 'vae': the reconstruction term of the losses is the pixel nle and no feature cotangent is
    back-propagated; the logged ``mse`` is still the feature term at the step's level."""
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import Stage1Step
    B, level = 4, 1
    cfg_o = O.ArchCfg.px64()
    data = O.synth_batch(B, cfg_o, seed=1234, steps=1)
    st = Stage1Step(ArchConfig.px64(), DEV, mode=mode, recon_level=level)
    st.load_recipe(0, True)
    st.step(data["x"].to(DEV), data["noise"][0, 0].to(DEV), data["noise"][0, 1].to(DEV))
    logs = st.logs()
    P = O.fill_state(O.vaegan_spec(cfg_o), 0, True)
    ref = RO.stage1_step_level(level, P, _opts("encoder", "decoder", "discriminator"), data["x"], data["noise"][0, 0],
                               data["noise"][0, 1], cfg_o, mode=mode)
    assert logs["train_dis"] == ref["logs"]["train_dis"] and logs["train_dec"] == ref["logs"]["train_dec"]
    for k in GAN_KEYS:
        print(mode, k, logs[k], ref["logs"][k], _rel(logs[k], ref["logs"][k]))
        assert _rel(logs[k], ref["logs"][k]) < LOSS_RTOL, (k, logs[k], ref["logs"][k])
    sd = st.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())


# ---- the engine against itself (deterministic mode: exact) -------------------------------------------------------
def _pair(B, **kw):
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import Stage1Step
    data = O.synth_batch(B, O.ArchCfg.px64(), seed=1234, steps=1)
    args = (data["x"].to(DEV), data["noise"][0, 0].to(DEV), data["noise"][0, 1].to(DEV))
    a = Stage1Step(ArchConfig.px64(), DEV, **kw)
    a.load_recipe(0, True)
    return a, args


def _finish():
    from fmri_hip import ops
    ops.join_side()
    torch.cuda.synchronize()


def _everything(st):
    out = {k: v.clone() for k, v in st.state_dict().items()}
    for n in ("opt_enc", "opt_dec", "opt_dis"):
        out["optimizer." + n] = getattr(st, n).s1.clone()
    out["losses"] = st.scal[:len(GAN_KEYS)].clone()
    out["flags"] = st.flags.clone()
    return out


def _same_bits(sa, sb, what):
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (what, k)


def _three_steps(mode, level=1, B=8):
    """Three steps of a fresh engine in one launch mode: 'step' (two streams), 'one-stream', 'replay' (one warm-up step,
    the recording, two replays)."""
    from fmri_hip import ops
    st, args = _pair(B, recon_level=level)
    side_was = ops._SIDE["on"]
    try:
        if mode == "replay":
            run = st.capture(*args, warmup=1)
            run()
            run()
        else:
            ops._SIDE["on"] = mode == "step"
            for _ in range(3):
                st.step(*args)
        _finish()
    finally:
        ops._SIDE["on"] = side_was
    return _everything(st)


@pytest.mark.selfcheck
def test_level1_runs_are_bit_identical_in_every_launch_mode(deterministic):
    first = {}
    for mode in ("step", "one-stream", "replay"):
        first[mode] = _three_steps(mode)
        _same_bits(first[mode], _three_steps(mode), f"two runs, {mode}")
        assert all(bool(torch.isfinite(v).all()) for v in first[mode].values() if v.is_floating_point())
    # ... and the launch modes agree with each other, as they do at level 3 (tests/test_zz_selfcheck_gpu.py)
    _same_bits(first["step"], first["one-stream"], "two streams vs one")
    _same_bits(first["replay"], first["one-stream"], "replay vs eager")


@pytest.mark.selfcheck
def test_level3_argument_is_the_default_step(deterministic):
    a, args = _pair(8)
    b, _ = _pair(8, recon_level=3)
    for _ in range(3):
        a.step(*args)
        b.step(*args)
    _finish()
    _same_bits(_everything(a), _everything(b), "recon_level=3 vs default")


def test_level1_long_run_stays_finite_with_the_monitor_on():
    """150 steps at B = 8 with fresh device noise per step; the BatchNorm-backward clip counts of the last step are
    reported, not asserted (a saturating store is a legitimate event the monitor exists to show)."""
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import Stage1Step
    B = 8
    x = O.synth_batch(B, O.ArchCfg.px64(), seed=1234, steps=1)["x"].to(DEV)
    st = Stage1Step(ArchConfig.px64(), DEV, monitor=True, rng=DeviceRng(11, DEV), recon_level=1)
    st.load_recipe(0, True)
    clipped = 0
    for it in range(150):
        st.step(x)
        if it % 50 == 49:
            num = st.numerics()
            logs = st.logs()
            assert all(math.isfinite(float(v)) for v in logs.values()), (it, logs)
            assert num["losses_finite"], (it, num)
            assert all(v["nonfinite"] in (0, None) for v in num["grad"].values()), (it, num["grad"])
            assert all(v["nonfinite"] == 0 for v in num["bn_backward"].values()), (it, num["bn_backward"])
            dis = {k: v for k, v in num["bn_backward"].items() if k.startswith("discriminator")}
            assert len(dis) == 4, dis                      # every BatchNorm of the discriminator reports
            clipped += sum(v["saturated"] for v in num["bn_backward"].values())
            print(f"level 1 step {it}: loss_encoder {logs['loss_encoder']:.5g} mse {logs['mse']:.5g} "
                  f"bn_backward saturated {({k: v['saturated'] for k, v in num['bn_backward'].items() if v['saturated']})}")
    print("level 1, 150 steps: clipped dx values seen at the three probes:", clipped)
    sd = st.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
