"""The on-device validation pass of the fused steps (fmri_hip/evaluate.py): its eval-mode forward against the oracle, its
metrics plumbing against the float64 restatement (tests/eval_oracle.py), and that a pass leaves training exactly where it
was.  px64, B = 4, a 16-image training set and a 10-image validation set (batches 4, 4, 2), V = 4096, deterministic mode."""
import numpy as np
import pytest
import torch

import eval_oracle as EO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, V, N_TRAIN, N_VAL = 4, 4096, 16, 10
BAR_ABS = 2e-6                  # PCC / SSIM against float64 (tests/test_metrics.py:81)
BAR_MSE_REL = 2.0 ** -22        # one fp32 rounding of an fp64 result


@pytest.fixture(autouse=True)
def _deterministic(deterministic):
    yield


def _u8(n, seed):
    return torch.randint(0, 256, (n, 64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _fmri(n, seed):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((n, V)).astype(np.float32))


def _datasets(fmri=False):
    from fmri_hip.feed import DeviceDataset
    tr = DeviceDataset(_u8(N_TRAIN, 1).to(DEV), _fmri(N_TRAIN, 2).to(DEV) if fmri else None)
    va = DeviceDataset(_u8(N_VAL, 3).to(DEV), _fmri(N_VAL, 4).to(DEV) if fmri else None)
    return tr, va


def _cfgs():
    from fmri_hip.params import ArchConfig
    from oracle import vaegan_oracle as O
    return ArchConfig.px64(), O.ArchCfg.px64()


def _engine_sd(P):
    """An oracle state as the engine's ``load_state_dict`` takes it (its ``num_batches_tracked`` are 0-d, as torch's)."""
    return {k: (v.reshape(()) if k.endswith("num_batches_tracked") else v.clone()) for k, v in P.items()}


def _summary_close(got, ref, tag):
    """The comparison of tests/test_api.py:174-175: L2 norm within 2e-3, head / tail elements within 5e-3."""
    from oracle import vaegan_oracle as O
    g, r = O.tensor_summary(got.float().cpu()), O.tensor_summary(ref.float())
    e_l2, e_el = abs(g[0] - r[0]) / abs(r[0]), np.abs(g[2:] - r[2:]).max() / max(np.abs(r[2:]).max(), 1e-3)
    print(f"evaluator forward {tag}: L2 err/bound {e_l2:.3g}/2e-3, elements err/bound {e_el:.3g}/5e-3, "
          f"max |diff| over all elements {(got.float().cpu() - ref.float()).abs().max().item():.3g}")
    assert e_l2 < 2e-3 and e_el < 5e-3, (tag, e_l2, e_el)


# ---- forward parity -----------------------------------------------------------------------------------------------------
def test_eval_forward_stage1_matches_oracle():
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.feed import DeviceDataset
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import Stage1Step
    from oracle import vaegan_oracle as O
    from test_oracle_golden import eval_state
    cfg_e, cfg_o = _cfgs()
    P = eval_state(cfg_o, 0)
    step = Stage1Step(cfg_e, DEV)
    step.load_state_dict(_engine_sd(P))
    ev = Evaluator(step, DeviceDataset(_u8(B, 5).to(DEV)), batch=B, rng=DeviceRng(21, DEV))
    ev.run()
    x, eps = ev.last_truth().cpu(), ev.last_noise().cpu()
    with torch.no_grad():
        mu, lv = O.encoder_fwd(P, "encoder.", x, cfg_o, train=False)
        ref = O.decoder_fwd(P, "decoder.", O.reparameterize(mu, lv, eps), cfg_o, train=False)
    assert eps.shape == (B, cfg_e.latent_dim) and float(eps.std()) > 0.5
    _summary_close(ev.last_output(), ref, "Stage1Step")


def _cognitive_state(cfg_o, seed):
    from oracle import vaegan_oracle as O
    from test_oracle_golden import eval_state
    sd = {k: v for k, v in eval_state(cfg_o, seed).items() if k.startswith(("decoder.", "discriminator."))}
    sd.update(O.fill_state(O.cognitive_encoder_spec(cfg_o, V), seed + 100, True))
    return sd


def test_eval_forward_cognitive_matches_oracle():
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.feed import DeviceDataset
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import CognitiveStep
    from oracle import vaegan_oracle as O
    cfg_e, cfg_o = _cfgs()
    P = _cognitive_state(cfg_o, 0)
    step = CognitiveStep(cfg_e, V, DEV, stage=3)
    step.load_state_dict(_engine_sd(P))
    fm = _fmri(B, 6)
    ev = Evaluator(step, DeviceDataset(_u8(B, 5).to(DEV), fm.to(DEV)), batch=B, rng=DeviceRng(22, DEV))
    ev.run()
    with torch.no_grad():
        mu, lv = O.cognitive_encoder_fwd(P, "encoder.", fm, train=False)
        ref = O.decoder_fwd(P, "decoder.", O.reparameterize(mu, lv, ev.last_noise().cpu()), cfg_o, train=False)
    _summary_close(ev.last_output(), ref, "CognitiveStep")


def test_eval_forward_wae_stage2_matches_oracle():
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.feed import DeviceDataset
    from fmri_hip.wae_steps import WaeStep
    from oracle import vaegan_oracle as O
    cfg_e, cfg_o = _cfgs()
    P = _cognitive_state(cfg_o, 0)
    step = WaeStep(cfg_e, DEV, stage=2, n_voxels=V)
    step.cog.group.load_state_dict(_engine_sd(P), "encoder.")
    step.dec.group.load_state_dict(_engine_sd(P), "decoder.")
    fm = _fmri(B, 6)
    ev = Evaluator(step, DeviceDataset(_u8(B, 5).to(DEV), fm.to(DEV)), batch=B)
    ev.run()
    assert ev.last_noise() is None
    with torch.no_grad():
        ref = O.wae_cognitive_eval(P, fm, cfg_o)
    _summary_close(ev.last_output(), ref, "WaeStep stage 2")


# ---- metrics plumbing ---------------------------------------------------------------------------------------------------
def _bars(tag, got, want):
    errs = [abs(float(got[0]) - want[0]), abs(float(got[1]) - want[1]), abs(float(got[2]) - want[2]) / want[2]]
    for name, e, b in zip(("PCC", "SSIM", "MSE(rel)"), errs, (BAR_ABS, BAR_ABS, BAR_MSE_REL)):
        print(f"evaluator {tag} {name}: err/bound {e:.3g}/{b:.3g} = {e / b:.3f}")
    assert errs[0] <= BAR_ABS and errs[1] <= BAR_ABS and errs[2] <= BAR_MSE_REL, (tag, errs)


@pytest.mark.parametrize("denorm", [False, True], ids=["raw", "denorm"])
def test_pass_metrics_against_fp64(denorm):
    """valid_* = the last (ragged, 2-image) batch against the float64 restatement on ``last_output()`` and the ingested
    truth; mean_* = the float64 mean of ``batch_metrics()`` to one fp32 ulp; batches = 3."""
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import Stage1Step
    cfg_e, _ = _cfgs()
    _, va = _datasets()
    step = Stage1Step(cfg_e, DEV)
    step.load_recipe(0, True)
    ev = Evaluator(step, va, batch=B, rng=DeviceRng(23, DEV), denorm=denorm)
    assert ev.ranges == [(0, 4), (4, 4), (8, 2)]
    ev.run()
    h = ev.history()
    assert "epoch" not in h and h["pass"].tolist() == [0] and h["batches"].tolist() == [3]
    out, truth = ev.last_output().cpu(), ev.last_truth().cpu()
    assert out.shape == (2, 3, 64, 64)
    aff = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)) if denorm else (None, None)
    want = EO.image_metrics64(EO.to_layout(out), EO.to_layout(truth), 3, *aff)
    _bars("valid", [h[f"valid_{m}"][0] for m in ("PCC", "SSIM", "MSE")], want)
    bm = ev.batch_metrics().cpu().numpy()
    assert bm.shape == (3, 3) and [h[f"valid_{m}"][0] for m in ("PCC", "SSIM", "MSE")] == bm[2].tolist()
    mean64 = bm.astype(np.float64).mean(0)
    for j, m in enumerate(("PCC", "SSIM", "MSE")):
        err, ulp = abs(float(h[f"mean_{m}"][0]) - mean64[j]), float(np.spacing(np.float32(abs(mean64[j]))))
        print(f"evaluator mean_{m}: err/bound {err:.3g}/{ulp:.3g}")
        assert err <= ulp
        assert np.isnan(h[f"train_{m}"][0])


def test_train_batch_metrics_against_fp64():
    """train_* of the row after a step: the step's train-mode x_tilde against its x, and NaN again in the row after."""
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.ops import nhwc_to_images
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import Stage1Step
    from oracle import vaegan_oracle as O
    cfg_e, cfg_o = _cfgs()
    _, va = _datasets()
    step = Stage1Step(cfg_e, DEV)
    step.load_recipe(0, True)
    ev = Evaluator(step, va, batch=B, rng=DeviceRng(23, DEV))
    with pytest.raises(RuntimeError):
        ev.train_batch()
    data = O.synth_batch(B, cfg_o, seed=1234, steps=1)
    step.step(data["x"].to(DEV), data["noise"][0, 0].to(DEV), data["noise"][0, 1].to(DEV))
    ev.train_batch()
    xt = step.outputs()["x_tilde"].cpu()
    x = nhwc_to_images(step.fw["disc_in"][:B], 3).cpu()
    ev.run()
    ev.run()
    h = ev.history()
    _bars("train", [h[f"train_{m}"][0] for m in ("PCC", "SSIM", "MSE")],
          EO.image_metrics64(EO.to_layout(xt), EO.to_layout(x)))
    assert all(np.isnan(h[f"train_{m}"][1]) for m in ("PCC", "SSIM", "MSE"))


# ---- training is untouched ----------------------------------------------------------------------------------------------
def _make(kind, with_log=True):
    from fmri_hip.feed import DeviceFeed
    from fmri_hip.rng import DeviceRng
    from fmri_hip.schedule import TrainLog
    from fmri_hip.steps import Stage1Step
    from fmri_hip.wae_steps import WaeStep
    cfg_e, _ = _cfgs()
    tr, va = _datasets()
    g = DeviceRng(7, DEV)
    feed = DeviceFeed(tr, B, 11, rng=g, flip=True, max_shift=2)
    log = TrainLog(64) if with_log else None
    if kind == "stage1":
        step = Stage1Step(cfg_e, DEV, rng=g, feed=feed, log=log)
        step.load_recipe(0, True)
    else:
        step = WaeStep(cfg_e, DEV, stage=1, rng=g, feed=feed, log=log)
        step.load_recipe(0, True)
    return step, va


def _training_state(step):
    out = dict(step.state_dict())
    for i, o in enumerate(step.optims):
        for name in ("s1", "s2", "lr_dev", "t_dev"):
            t = getattr(o, name)
            if t is not None:
                out[f"optim{i}.{name}"] = t.clone()
    out["rng"] = step.rng._state.clone()
    out["feed"] = step.feed._state.clone()
    out["scal"] = step.scal.clone()
    return out


def _six_steps(kind, captured, with_eval):
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.rng import DeviceRng
    step, va = _make(kind)
    ev = Evaluator(step, va, batch=B, rng=DeviceRng(31, DEV) if kind == "stage1" else None) if with_eval else None
    run = step.capture() if captured else step.step
    for s in range(6):
        run()
        if ev is not None and s in (1, 3):
            ev.train_batch()
            ev.run()
    torch.cuda.synchronize()
    return _training_state(step), step.history(), (ev.history() if ev is not None else None)


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "replayed"])
@pytest.mark.parametrize("kind", ["stage1", "wae1"])
def test_training_is_untouched_by_passes(kind, captured):
    """Six steps plain, and six steps with train_batch() + run() after steps 2 and 4: parameters, BatchNorm buffers,
    optimizer state, generator / feed state and the training log are bitwise the same."""
    plain, log_p, _ = _six_steps(kind, captured, False)
    mixed, log_m, eh = _six_steps(kind, captured, True)
    assert plain.keys() == mixed.keys()
    for k in plain:
        assert torch.equal(plain[k], mixed[k]), k
    assert log_p.keys() == log_m.keys()
    for k in log_p:
        assert np.array_equal(log_p[k], log_m[k], equal_nan=True), k
    assert eh["pass"].tolist() == [0, 1] and eh["batches"].tolist() == [3, 3]
    assert np.isfinite(np.stack([eh[f"{p}_{m}"] for p in ("valid", "mean", "train") for m in ("PCC", "SSIM", "MSE")])).all()


def test_run_moves_no_batchnorm_buffer():
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.rng import DeviceRng
    step, va = _make("stage1", with_log=False)
    for _ in range(2):
        step.step()
    before = step.state_dict()
    modes = [bn.eval_mode for n in (step.enc, step.dec, step.dis) for bn in n.all_bns()]
    Evaluator(step, va, batch=B, rng=DeviceRng(31, DEV)).run()
    after = step.state_dict()
    assert modes == [bn.eval_mode for n in (step.enc, step.dec, step.dis) for bn in n.all_bns()] and not any(modes)
    keys = [k for k in before if "running_" in k or "num_batches_tracked" in k]
    assert len(keys) >= 30
    for k in before:
        assert torch.equal(before[k], after[k]), k


@pytest.mark.selfcheck
def test_pass_sees_the_state_of_the_last_replay():
    """After four replays the pass's row and last output are those of a fresh step loaded from ``state_dict()``, with a
    fresh evaluator at the same generator state."""
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import Stage1Step
    step, va = _make("stage1", with_log=False)
    ev = Evaluator(step, va, batch=B, rng=DeviceRng(31, DEV))
    replay = step.capture()
    for _ in range(4):
        replay()
    ev.run()
    fresh = Stage1Step(step.cfg, DEV)
    fresh.load_state_dict(step.state_dict())
    ev2 = Evaluator(fresh, va, batch=B, rng=DeviceRng(31, DEV))
    ev2.run()
    assert torch.equal(ev.last_output(), ev2.last_output())
    assert torch.equal(ev.batch_metrics(), ev2.batch_metrics())
    h, h2 = ev.history(), ev2.history()
    for k in h2:
        assert np.array_equal(h[k], h2[k], equal_nan=True), k
    # ... and not those of the weights the step started from
    start = Stage1Step(step.cfg, DEV)
    start.load_recipe(0, True)
    ev3 = Evaluator(start, va, batch=B, rng=DeviceRng(31, DEV))
    ev3.run()
    assert not torch.equal(ev.last_output(), ev3.last_output())


# ---- ring, epoch column, argument errors --------------------------------------------------------------------------------
def test_ring_keeps_the_last_rows_and_epoch_follows_the_feed():
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.rng import DeviceRng
    step, va = _make("stage1", with_log=False)
    ev = Evaluator(step, va, batch=B, rng=DeviceRng(31, DEV), capacity=2)
    epochs = []
    for n_steps in (1, 3, 4):               # 16 training images, batches of 4: four steps per epoch
        for _ in range(n_steps):
            step.step()
        ev.run()
        epochs.append(step.feed.position()[0])
    h = ev.history()
    assert h["pass"].tolist() == [1, 2] and h["epoch"].tolist() == epochs[1:] and h["epoch"].dtype == np.int64
    assert epochs[2] > epochs[0]
    assert all(len(v) == 2 for v in h.values())


def test_argument_errors():
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.feed import DeviceDataset
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import CognitiveStep, Stage1Step
    from fmri_hip.wae_steps import WaeStep
    cfg_e, _ = _cfgs()
    _, va = _datasets()
    s1 = Stage1Step(cfg_e, DEV)
    with pytest.raises(ValueError, match="rng"):
        Evaluator(s1, va, batch=B)
    with pytest.raises(ValueError, match="fMRI"):
        Evaluator(CognitiveStep(cfg_e, V, DEV, stage=3), va, batch=B, rng=DeviceRng(1, DEV))
    with pytest.raises(ValueError, match="fMRI"):
        Evaluator(WaeStep(cfg_e, DEV, stage=2, n_voxels=V), va, batch=B)
    small = DeviceDataset(torch.zeros(4, 32, 32, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="32 x 32"):
        Evaluator(s1, small, batch=B, rng=DeviceRng(1, DEV))
    with pytest.raises(TypeError):
        Evaluator(object(), va, batch=B)
    Evaluator(WaeStep(cfg_e, DEV, stage=1), va, batch=B)          # a WAE step samples nothing: no rng needed
