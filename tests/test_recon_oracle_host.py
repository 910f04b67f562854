"""tests/recon_oracle.py (the CPU oracle's Stage-I / Dual steps at ``--recon_level`` 1 / 2) against golden vectors the real
reference produced (tests/golden/make_golden_recon.py: ``VaeGan(recon_level=level)``, literal three ``backward()`` calls,
real ``torch.optim``).  No GPU, no reference tree.

Bars and procedure are those of tests/test_oracle_golden.py, whose helpers and two-pass ``precision`` fixture are used as
they are: every test runs in float64 against <case>_f64.npz at 1e-9 per entry (the exact pin of the restatement) and in
fp32 against <case>.npz at that file's fp32 bars (thread-count noise floor of the CPU convolutions)."""
import pytest
import torch

import recon_oracle as RO
from oracle import vaegan_oracle as O
from test_oracle_golden import precision  # noqa: F401  (autouse, parametrised: f64 / f32 pass of every test below)
from test_oracle_golden import _check_step, _load, _rms_opts, dual_state

STAGE1_CASES = {"stage1_rl1_b4": 1, "stage1_rl2_b4": 2, "stage1_rl2_betavae_b4": 2}


@pytest.mark.parametrize("name", sorted(STAGE1_CASES))
def test_stage1_levels_match_reference(golden_dir, name):
    cfg = O.ArchCfg.px64()
    g = _load(golden_dir, name)
    level = int(g["meta/recon_level"])
    assert level == STAGE1_CASES[name]
    B, seed, perturb, steps = int(g["meta/B"]), int(g["meta/seed"]), bool(g["meta/perturb"]), int(g["meta/steps"])
    mode, beta = str(g["meta/mode"]), float(g["meta/beta"])
    P = O.fill_state(O.vaegan_spec(cfg), seed, perturb)
    data = O.synth_batch(B, cfg, seed=1234, steps=steps)
    opts = _rms_opts("encoder", "decoder", "discriminator")
    for s in range(steps):
        out = RO.stage1_step_level(level, P, opts, data["x"], data["noise"][s, 0], data["noise"][s, 1], cfg,
                                   keep_grads=True, mode=mode, beta=beta)
        assert out["logs"].pop("train_dis") == bool(g[f"step{s}/logs/train_dis"])
        assert out["logs"].pop("train_dec") == bool(g[f"step{s}/logs/train_dec"])
        # the feature tensor is block ``level``'s raw output: 128 x 32 x 32 / 256 x 16 x 16 per image at 64 px
        assert out["fw"]["disc_layer"].shape[1] == {1: 131072, 2: 65536}[level]
        _check_step(g, f"step{s}", out, P)
        # BatchNorm counters: the REC pass ends at block ``level`` -> two updates per step up to it, one above
        for i in (1, 2, 3):
            assert int(P[f"discriminator.conv.{i}.bn.num_batches_tracked"]) == (s + 1) * (2 if i <= level else 1)


def test_dual_stage1_level2_matches_reference(golden_dir):
    cfg = O.ArchCfg.px64()
    g = _load(golden_dir, "dual1_rl2_b4")
    level = int(g["meta/recon_level"])
    assert level == 2
    B, seed, perturb, steps = int(g["meta/B"]), int(g["meta/seed"]), bool(g["meta/perturb"]), int(g["meta/steps"])
    P = dual_state(cfg, seed, perturb)
    data = O.synth_batch(B, cfg, seed=1234, steps=steps)
    opts = _rms_opts("encoder", "decoder", "discriminator", "wae_discriminator")
    for s in range(steps):
        out = RO.dual_stage1_step_level(level, P, opts, data["x"], data["noise"][s], cfg, lam=float(g["meta/lam"]),
                                        keep_grads=True)
        assert out["logs"].pop("train_dis") == bool(g[f"step{s}/logs/train_dis"])
        assert out["logs"].pop("train_dec") == bool(g[f"step{s}/logs/train_dec"])
        _check_step(g, f"step{s}", out, P)


def test_feature_width_follows_the_level():
    """'REC' output of block 1 / 2 / 3 at 64 px: 128 x 32 x 32, 256 x 16 x 16, 256 x 8 x 8 values per image."""
    cfg = O.ArchCfg.px64()
    data = O.synth_batch(2, cfg, seed=1234)
    for level, width in ((1, 131072), (2, 65536), (3, 16384)):
        P = O.fill_state(O.vaegan_spec(cfg), 0, True)
        with RO.at_level(level), torch.no_grad():
            fw = O.vaegan_forward(P, data["x"], data["noise"][0, 0], data["noise"][0, 1], cfg)
        assert tuple(fw["disc_layer"].shape) == (6, width)


def test_level3_is_the_plain_oracle_step():
    cfg = O.ArchCfg.px64()
    data = O.synth_batch(2, cfg, seed=1234)
    res = []
    for leveled in (False, True):
        P = O.fill_state(O.vaegan_spec(cfg), 0, True)
        opts = _rms_opts("encoder", "decoder", "discriminator")
        args = (P, opts, data["x"], data["noise"][0, 0], data["noise"][0, 1], cfg)
        out = RO.stage1_step_level(3, *args, keep_grads=True) if leveled else O.stage1_step(*args, keep_grads=True)
        res.append((out, P))
    assert res[0][0]["logs"] == res[1][0]["logs"]
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k
    for k, v in res[0][0]["grads"].items():
        assert torch.equal(v, res[1][0]["grads"][k]), k


def test_discriminator_fwd_is_restored():
    orig = O.discriminator_fwd
    with RO.at_level(2):
        assert O.discriminator_fwd is not orig
        with RO.at_level(1):                      # nested: each exit puts back what it found
            pass
        assert O.discriminator_fwd is not orig
    assert O.discriminator_fwd is orig
    with pytest.raises(RuntimeError):
        with RO.at_level(1):
            raise RuntimeError("inside")
    assert O.discriminator_fwd is orig
    with pytest.raises(ValueError):
        with RO.at_level(0):
            pass
    assert O.discriminator_fwd is orig
    cfg = O.ArchCfg.px64()
    data = O.synth_batch(2, cfg, seed=1234)
    P = O.fill_state(O.vaegan_spec(cfg), 0, True)
    RO.stage1_step_level(1, P, _rms_opts("encoder", "decoder", "discriminator"), data["x"], data["noise"][0, 0],
                         data["noise"][0, 1], cfg)
    assert O.discriminator_fwd is orig
