"""n-way identification inside the on-device validation pass (fmri_hip/evaluate.py ``Evaluator(identify=top)``): the columns
every evaluator has keep their bits, the four new columns are the accumulator's, the accumulator is the host's counting on
the matrices and draws of each batch, and training stays where it was.  The px64 configuration and the tiny datasets of
tests/test_evaluator_gpu.py: 10 validation images in batches of 4, 4, 2."""
import numpy as np
import pytest
import torch

import ident_oracle as IO
from test_evaluator_gpu import B, DEV, N_VAL, _cfgs, _datasets, _make, _training_state, _u8

pytestmark = pytest.mark.gpu

TOP = 5
BAR = 2e-6
NWAY = ("nway_PCC", "nway_SSIM", "nway_exp_PCC", "nway_exp_SSIM")


@pytest.fixture(autouse=True)
def _deterministic(deterministic):
    yield


def _step(kind):
    from fmri_hip.steps import Stage1Step
    from fmri_hip.wae_steps import WaeStep
    cfg_e, _ = _cfgs()
    step = Stage1Step(cfg_e, DEV) if kind == "stage1" else WaeStep(cfg_e, DEV, stage=1)
    step.load_recipe(0, True)
    return step


def _evaluator(step, ds, seed=23, **kw):
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.rng import DeviceRng
    return Evaluator(step, ds, batch=B, rng=DeviceRng(seed, DEV) if seed is not None else None, **kw)


def _prefix(ds, n):
    from fmri_hip.feed import DeviceDataset
    return DeviceDataset(ds.images[:n].contiguous())


@pytest.mark.parametrize("kind", ["stage1", "wae1"])
def test_shared_columns_keep_their_bits_and_new_columns_are_the_host_counting(kind):
    step = _step(kind)
    _, va = _datasets()
    plain, ident = _evaluator(step, va), _evaluator(step, va, identify=TOP)
    plain.run()
    ident.run()
    hp, hi = plain.history(), ident.history()
    assert set(hi) == set(hp) | set(NWAY)
    for k in hp:
        assert np.array_equal(hp[k], hi[k], equal_nan=True), k
    assert torch.equal(plain.last_output(), ident.last_output())
    assert torch.equal(plain.batch_metrics(), ident.batch_metrics())
    if kind == "stage1":
        assert torch.equal(plain.last_noise(), ident.last_noise())
        assert plain.rng.state() == ident.rng.state()          # the advance per batch is unchanged

    # the four columns are the accumulator's, to one fp32 rounding
    acc = ident.identification().cpu()
    assert acc[4:].tolist() == [N_VAL, 3]
    for k, name in enumerate(NWAY):
        want = acc[k].item() / acc[4].item()
        err = abs(float(hi[name][0]) - want)
        print(f"evaluator {kind} {name} = {hi[name][0]:.6f}: err/bound {err:.3g}/{abs(want) * 2.0 ** -24:.3g}")
        assert err <= abs(want) * 2.0 ** -24

    # the accumulator is the host counting over the three batches: passes over the 4-, 8- and 10-image prefixes of the
    # set end on batch 0, 1 and 2 (same generator seed, so the same eps and the same draws for the batches they share)
    hits, exp = np.zeros(2), np.zeros(2)
    rows = ident.batch_identification().cpu().double()
    for k, n_rows in enumerate((4, 8, N_VAL)):
        ev = _evaluator(step, _prefix(va, n_rows), identify=TOP)
        ev.run()
        torch.cuda.synchronize()
        S_pcc, S_ssim = (t.cpu() for t in ev.last_similarity())
        d = ev.last_distractors().cpu()
        b = S_pcc.shape[0]
        assert b == (4, 4, 2)[k] and d.shape == (b, TOP - 1)
        h = IO.n_way_from(S_pcc, S_ssim, d).sum(0).numpy()
        e = IO.n_way_expected_from(S_pcc, S_ssim, TOP).numpy() * b
        assert rows[k, :2].tolist() == (h / b).astype(np.float32).tolist()
        assert np.abs(rows[k, 2:4].numpy() - e / b).max() <= 2.0 ** -24
        hits += h
        exp += e
        if k == 2:
            assert torch.equal(ev.last_output(), ident.last_output())
            assert all(torch.equal(a, b_) for a, b_ in zip(ev.last_similarity(), ident.last_similarity()))
            assert torch.equal(ev.last_distractors(), ident.last_distractors())
            out, truth = ev.last_output().cpu(), ev.last_truth().cpu()
            for tag, got, want in (("PCC", S_pcc, IO.pcc_matrix64(out, truth)), ("SSIM", S_ssim, IO.ssim_matrix64(out, truth))):
                err = (got.double() - want).abs().max().item()
                print(f"evaluator {kind} last batch {tag} matrix: err/bound {err:.3g}/{BAR:.3g}")
                assert err <= BAR
    assert acc[:2].tolist() == hits.tolist()
    rel = np.abs(acc[2:4].numpy() - exp) / exp
    print(f"evaluator {kind} expectation: err/bound {rel.max():.3g}/{(N_VAL + TOP + 3) * 2.0 ** -52:.3g}")
    assert rel.max() <= (N_VAL + TOP + 3) * 2.0 ** -52


def test_wae_without_rng_gives_nan_sampled_columns():
    step = _step("wae1")
    _, va = _datasets()
    ev = _evaluator(step, va, seed=None, identify=TOP)
    ev.run()
    h = ev.history()
    assert np.isnan(h["nway_PCC"][0]) and np.isnan(h["nway_SSIM"][0])
    assert 0.0 <= h["nway_exp_PCC"][0] <= 1.0 and 0.0 <= h["nway_exp_SSIM"][0] <= 1.0
    assert ev.last_distractors() is None
    with_rng = _evaluator(step, va, identify=TOP)
    with_rng.run()
    h2 = with_rng.history()
    assert h2["nway_exp_PCC"][0] == h["nway_exp_PCC"][0] and h2["nway_exp_SSIM"][0] == h["nway_exp_SSIM"][0]
    # a non-sampling step advances by the draws it made: blocks(b * (top - 1)) per batch
    assert with_rng._id_rng.state()[1] == 4 + 4 + 2


def _six_steps(kind, captured, with_eval):
    step, va = _make(kind)
    run = step.capture() if captured else step.step          # captured BEFORE the evaluator is built
    ev = _evaluator(step, va, seed=31, identify=TOP) if with_eval else None
    for s in range(6):
        run()
        if ev is not None and s in (1, 3):
            ev.train_batch()
            ev.run()
    torch.cuda.synchronize()
    return _training_state(step), step.history(), (ev.history() if ev is not None else None)


@pytest.mark.selfcheck
@pytest.mark.parametrize("captured", [False, True], ids=["eager", "replayed"])
@pytest.mark.parametrize("kind", ["stage1", "wae1"])
def test_training_is_untouched_by_identifying_passes(kind, captured):
    plain, log_p, _ = _six_steps(kind, captured, False)
    mixed, log_m, eh = _six_steps(kind, captured, True)
    assert plain.keys() == mixed.keys()
    for k in plain:
        assert torch.equal(plain[k], mixed[k]), k
    assert log_p.keys() == log_m.keys()
    for k in log_p:
        assert np.array_equal(log_p[k], log_m[k], equal_nan=True), k
    assert eh["pass"].tolist() == [0, 1] and eh["batches"].tolist() == [3, 3]
    assert np.isfinite(np.stack([eh[k] for k in NWAY])).all()


def test_argument_errors():
    from fmri_hip.feed import DeviceDataset
    cfg_e, _ = _cfgs()
    s1 = _step("stage1")
    _, va = _datasets()
    with pytest.raises(ValueError, match="last batch"):
        _evaluator(s1, DeviceDataset(_u8(9, 3).to(DEV)), identify=TOP)
    with pytest.raises(ValueError, match="last batch"):
        _evaluator(s1, DeviceDataset(_u8(1, 3).to(DEV)), identify=TOP)
    with pytest.raises(ValueError, match="identify"):
        _evaluator(s1, va, identify=0)
    with pytest.raises(ValueError, match="latent_dim"):
        _evaluator(s1, va, identify=cfg_e.latent_dim + 2)
    _evaluator(s1, va, identify=cfg_e.latent_dim + 1)
    _evaluator(_step("wae1"), va, identify=cfg_e.latent_dim + 2)        # nothing sampled: no such limit
    with pytest.raises(RuntimeError, match="identify"):
        _evaluator(s1, va).identification()
