"""The oracle's ReLU-mask hooks (oracle/vaegan_oracle.py: RELU_MASKS with ``None`` entries, RELU_RECORD) and what pinning
the masks buys the step-level gradient tests (tests/gradcheck.py) -- CPU only, B = 4 at 64 px.

  * every step function: the masks of a 16-bit-storage run, recorded and replayed, reproduce its gradients and losses bit
    for bit with the list fully consumed; so does the replay with every other entry ``None``; the number of ReLU calls
    is the documented one (CALLS below: the call order the ordering functions of tests/gradcheck.py build);
  * one mask too few or too many fails loudly;
  * sensitivity: an "engine" whose KL cotangent is weighted 3 % too much fails ``gradcheck.check`` at its default bound and
    passes the bound the un-pinned regime had.
"""
import pytest
import torch

import gradcheck
import mmd_oracle as M
import recon_oracle as RO
from oracle import vaegan_oracle as O

B, V = 4, 256
CFG = O.ArchCfg.px64()

# ReLU calls per step function at 64 px, in call order (E = image encoder: 3 conv blocks + fc = 4, C = cognitive encoder 1,
# G = decoder: fc + 3 deconv blocks = 4, REC = discriminator up to block ``recon_level``: 3 at level 3, GAN = conv0 +
# 3 blocks + fc = 5, W = latent discriminator 4):
CALLS = {
    "stage1": 20,           # E G(z) G(z_p) REC GAN                                            -- in any mode
    "stage1 beta-vae": 20,
    "stage1 level 1": 18,   # REC ends at block 1: conv0 only
    "stage1 level 2": 19,
    "stage2": 25,           # C G(z) E_teacher G(z_teacher) G(z_p) REC GAN
    "stage2 vae": 17,       # C G(z) G(z_p) REC GAN
    "stage3": 17,           # C G(z) G(z_p) REC GAN
    "wae1": 24,             # E | W(real) W(fake) | E G W
    "wae2": 30,             # E_t G(z_t) C E_t | W(real) W(fake) | C G W
    "wae3": 22,             # C E_t | W(real) W(fake) | C W G
    "dual1": 44,            # stage1, E | W(real) W(fake) | E G(z_real2) W
    "wae1 mmd": 12,         # E E G
    "wae2 mmd": 18,         # E_t G(z_t) C E_t C G
    "wae3 mmd": 10,         # C E_t C G
}

_DATA = {}


def _data():
    if not _DATA:
        _DATA.update(O.synth_batch(B, CFG, n_voxels=V, seed=1234, steps=1))
    return _DATA


def _rms(*names):
    return {n: O.OptState(kind="rmsprop", lr=1e-4) for n in names}


def _cog_state(stage, teacher):
    t = O.fill_state(O.vaegan_spec(CFG), 0, True)
    P = dict(O.fill_state(O.cognitive_encoder_spec(CFG, V), 100, True))
    P.update({k: v for k, v in t.items() if k.startswith(("decoder.", "discriminator."))})
    if teacher:
        P.update({"teacher_net." + k: v for k, v in t.items() if k.startswith("encoder.")})
    return P


def _wae_state(stage):
    spec = O.encoder_spec(CFG) + O.decoder_spec(CFG) + O.wae_discriminator_spec(CFG)
    if stage == 1:
        return O.fill_state(spec, 0, False)
    t = O.fill_state(spec, 0, True)
    P = dict(O.fill_state(O.cognitive_encoder_spec(CFG, V), 100, True))
    P.update({k: v for k, v in t.items() if k.startswith("decoder.")})
    P.update(O.fill_state(O.wae_discriminator_spec(CFG), 200, True))
    P.update({"teacher_net." + k: v for k, v in t.items() if k.startswith("encoder.")})
    return P


def _adam(stage):
    lr = 1e-4 if stage == 1 else 1e-3
    return {n: O.OptState(kind="adam", lr=lr) for n in ("encoder", "decoder", "discriminator")}


def _run(name, beta=None):
    """One step of the step function ``name`` on fresh seeded state; -> its result dict (gradients kept)."""
    d = _data()
    x, fmri, nz = d["x"], d["fmri"], d["noise"][0]
    kind, _, opt = name.partition(" ")
    if kind == "stage1":
        P = O.fill_state(O.vaegan_spec(CFG), 0, True)
        o = _rms("encoder", "decoder", "discriminator")
        if opt.startswith("level"):
            return RO.stage1_step_level(int(opt[-1]), P, o, x, nz[0], nz[1], CFG, keep_grads=True)
        kw = dict(mode="beta-vae", beta=4.0 if beta is None else beta) if opt == "beta-vae" else {}
        return O.stage1_step(P, o, x, nz[0], nz[1], CFG, keep_grads=True, **kw)
    if kind in ("stage2", "stage3"):
        mode = opt or "vae-gan"
        fn = O.stage2_step if kind == "stage2" else O.stage3_step
        P = _cog_state(int(kind[-1]), kind == "stage2" and mode == "vae-gan")
        return fn(P, _rms("encoder", "decoder", "discriminator"), fmri, x, nz, CFG, V, keep_grads=True, mode=mode)
    if kind == "dual1":
        P = O.fill_state(O.vaegan_spec(CFG), 0, True)
        P.update(O.fill_state(O.wae_discriminator_spec(CFG, pre="wae_discriminator."), 200, True))
        return O.dual_stage1_step(P, _rms("encoder", "decoder", "discriminator", "wae_discriminator"), x, nz, CFG,
                                  keep_grads=True)
    stage = int(kind[-1])
    P = _wae_state(stage)
    if opt == "mmd":
        return M.wae_mmd_step(P, _adam(stage), stage, CFG, x, nz[2], fmri if stage > 1 else None, V, keep_grads=True)
    if stage == 1:
        return O.wae_stage1_step(P, _adam(1), x, nz[2], CFG, keep_grads=True)
    fn = O.wae_stage2_step if stage == 2 else O.wae_stage3_step
    return fn(P, _adam(stage), fmri, x, CFG, V, keep_grads=True)


def _same(a, b, what):
    assert a["logs"] == b["logs"], what
    assert a["grads"].keys() == b["grads"].keys()
    for k, v in a["grads"].items():
        assert (v is None) == (b["grads"][k] is None), (what, k)
        if v is not None:
            assert torch.equal(v, b["grads"][k]), (what, k)


_RECORDED = {}


def _recorded(name):
    """(masks, result) of the recording 16-bit-storage run of ``name``: made once, shared, never modified."""
    if name not in _RECORDED:
        masks = []
        with gradcheck.storage16(O), gradcheck.recording(O, masks):
            res = _run(name)
        _RECORDED[name] = (tuple(masks), res)
    return _RECORDED[name]


@pytest.mark.parametrize("name", sorted(CALLS))
def test_recorded_masks_replay_bit_for_bit(name):
    masks, first = _recorded(name)
    assert len(masks) == CALLS[name], (name, len(masks))
    assert O.RELU_RECORD is None and O.RELU_MASKS is None and not O.STORAGE16
    with gradcheck.pinned(O, masks):
        again = _run(name)
    _same(first, again, f"{name}: replay")
    with gradcheck.pinned(O, [None if i % 2 else m for i, m in enumerate(masks)]):
        own = _run(name)
    _same(first, own, f"{name}: replay with None entries")
    assert O.RELU_MASKS is None and not O.STORAGE16


def test_recording_is_off_by_default_and_while_masks_are_pinned():
    masks, first = _recorded("stage3")
    seen = []
    with gradcheck.recording(O, seen), gradcheck.pinned(O, masks):
        _run("stage3")
    assert seen == []
    plain = _run("stage3")                       # nothing set: the fp32 oracle, recording nothing
    assert O.RELU_RECORD is None
    assert any(not torch.equal(v, first["grads"][k]) for k, v in plain["grads"].items() if v is not None)


def test_one_mask_too_few_or_too_many_fails_loudly():
    masks, _ = _recorded("stage3")
    with pytest.raises(IndexError):
        with gradcheck.pinned(O, masks[:-1]):
            _run("stage3")
    assert O.RELU_MASKS is None and not O.STORAGE16
    with pytest.raises(AssertionError, match="1 of 18 pinned ReLU masks"):
        with gradcheck.pinned(O, masks + masks[-1:]):
            _run("stage3")
    assert O.RELU_MASKS is None and not O.STORAGE16
    # masks of the wrong call (two decoder passes swapped for one of another shape): the shape assert of the oracle
    with pytest.raises(AssertionError):
        with gradcheck.pinned(O, masks[1:2] + masks[:1] + masks[2:]):
            _run("stage3")
    assert O.RELU_MASKS is None and not O.STORAGE16


def test_pinned_masks_see_a_three_percent_misweighted_kl_term():
    """Stage I 'beta-vae', B = 4, seed 0.  "The engine": the oracle under its 16-bit storage model with beta = 4.12 in place
    of 4.0 -- the KL cotangent 3 % too heavy, everything else exact.  The references: the fp32 oracle and the 16-bit run
    with that engine's ReLU masks pinned, both at beta = 4.0.  ``check`` at its default bound (TOL16) sees it
    (encoder.l_mu.bias: err16 3e-2, projection 1.03); the bound the un-pinned regime had (LOOSE16 = 0.15 relative L2,
    cosine 0.95, length within 8 %) does not."""
    name = "stage1 beta-vae"
    masks = []
    with gradcheck.storage16(O), gradcheck.recording(O, masks):
        engine = _run(name, beta=4.0 * 1.03)
    ref32 = _run(name)
    with gradcheck.pinned(O, masks):
        ref16 = _run(name)
    with pytest.raises(AssertionError) as err:
        gradcheck.check(engine["grads"], ref32["grads"], ref16["grads"], "beta x 1.03")
    assert "encoder.l_mu.bias" in str(err.value)
    gradcheck.check(engine["grads"], ref32["grads"], ref16["grads"], "beta x 1.03, un-pinned bounds",
                    tol16=gradcheck.LOOSE16)
    # ... and the exact engine passes the default bound with room: what is left is nothing at all here
    with gradcheck.storage16(O), gradcheck.recording(O, []):
        exact = _run(name)
    rows = gradcheck.check(exact["grads"], ref32["grads"], ref16["grads"], "beta x 1.00")
    assert max(r[1] for r in rows) == 0.0
