"""GPU checks of the per-step training log (csrc/schedule.hip fmri_trainlog_append, fmri_hip/schedule.py TrainLog,
``log=`` of the fused steps): a row of the device ring holds exactly what ``logs()`` returns after that step -- the same
fp32 values, compared with ``==`` -- plus the epoch of the batch and the learning rates, in every launch mode, and the ring
wraps.  Deterministic mode makes two runs of the same steps bit-identical, so a run that syncs after every step to call
``logs()`` is the reference of a run that is read once at the end."""
import numpy as np
import pytest
import torch

import schedule_oracle as O
from schedule_cases import DECAYS, DEV, PER_EPOCH, _base, _finish, _make

pytestmark = pytest.mark.gpu
STEPS, CAP = 7, 4


def _reference(kind, schedule_kw=None, steps=STEPS):
    """``logs()`` after each of ``steps`` eager steps of a fresh fed step."""
    from fmri_hip.schedule import EpochSchedule
    st = _make(kind, EpochSchedule(**schedule_kw) if schedule_kw else None)
    out = []
    for _ in range(steps):
        st.step()
        _finish()
        out.append(st.logs())
    return out, _base(st, kind != "wae1")


def _check_rows(h, ref, first, names_lr, base=None, decays=None, masked=()):
    n = len(h["step"])
    assert h["step"].tolist() == list(range(first, first + n))
    for r, i in enumerate(range(first, first + n)):
        for k, v in ref[i].items():
            got = h[k][r]
            if isinstance(v, bool):
                assert got.dtype == np.bool_ and bool(got) == v, (i, k, got, v)
            else:
                assert got.dtype == np.float32 and got == np.float32(v), (i, k, got, v)     # logs() floats are fp32 values
                assert np.isfinite(got), (i, k)
    assert set(h) == set(ref[first]) | {"step", "epoch"} | set(names_lr)
    if base is not None:
        epochs = [i // PER_EPOCH for i in range(first, first + n)]
        assert h["epoch"].dtype == np.int64 and h["epoch"].tolist() == epochs
        for j, name in enumerate(names_lr):
            want = [O.f32(base["lr"][j] if j in masked else O.at(base, e, **decays)["lr"][j]) for e in epochs]
            assert h[name].tolist() == want, (name, h[name], want)


@pytest.mark.parametrize("mode", ["eager", "capture"])
def test_stage1_rows_equal_logs_of_every_step(deterministic, mode):
    """Two identical runs of 7 steps under a schedule; ``capacity=4`` keeps steps 3 .. 6 (epochs 1 1 1 2)."""
    from fmri_hip.schedule import EpochSchedule, TrainLog
    ref, base = _reference("stage1", DECAYS)
    st = _make("stage1", EpochSchedule(**DECAYS), log=TrainLog(capacity=CAP))
    if mode == "eager":
        for _ in range(STEPS):
            st.step()
    else:
        replay = st.capture()                                       # two warm-up steps, logged like any other
        for _ in range(STEPS - 2):
            replay()
    h = st.history()                                                # the one sync
    names_lr = ("lr_encoder", "lr_decoder", "lr_discriminator")
    _check_rows(h, ref, STEPS - CAP, names_lr, base, DECAYS)
    assert h["step"].tolist() == [3, 4, 5, 6] and h["epoch"].tolist() == [1, 1, 1, 2]
    m = st.epoch_means()
    assert m["epoch"].tolist() == [1, 2] and m["steps"].tolist() == [3, 1]
    for k in ("loss_encoder", "loss_decoder", "loss_discriminator", "nle", "kl", "mse"):
        assert m[k][0] == h[k][:3].astype(np.float64).mean() and m[k][1] == float(h[k][3]), k
    assert "train_dis" not in m and "lr_encoder" not in m


def test_ring_before_it_wraps_and_without_feed_or_schedule(deterministic):
    """A WaeStep handed its batch: no feed, no schedule -- ``epoch`` is -1 and the rates are the base rates; 7 steps in a
    ring of 16 come back whole, and the same 7 in a ring of 4 are its last four."""
    from fmri_hip.params import ArchConfig
    from fmri_hip.schedule import TrainLog
    from fmri_hip.wae_steps import W_LOG_KEYS, WaeStep
    cfg = ArchConfig.px64()
    gen = torch.Generator().manual_seed(5)
    xs = [torch.rand(4, 3, 64, 64, generator=gen).mul(2).sub(1).to(DEV) for _ in range(STEPS)]
    zs = [torch.randn(4, cfg.latent_dim, generator=gen).to(DEV) for _ in range(STEPS)]

    def run(log):
        st = WaeStep(cfg, DEV, 1, log=log)
        st.load_recipe(5, False)
        out = []
        for x, z in zip(xs, zs):
            st.step(x, z)
            if log is None:
                _finish()
                out.append(st.logs())
        return st, out
    _, ref = run(None)
    names_lr = ("lr_encoder", "lr_decoder", "lr_discriminator")
    for cap in (16, CAP):
        st, _ = run(TrainLog(capacity=cap))
        h = st.history()
        _check_rows(h, ref, max(0, STEPS - cap), names_lr)
        n = min(cap, STEPS)
        assert len(h["step"]) == n and h["epoch"].tolist() == [-1] * n
        assert h["lr_encoder"].tolist() == [O.f32(1e-4)] * n and h["lr_discriminator"].tolist() == [O.f32(0.5e-4)] * n
        assert tuple(k for k in W_LOG_KEYS) == st.log.losses
        m = st.epoch_means()
        assert m["epoch"].tolist() == [-1] and m["steps"].tolist() == [n]
    with pytest.raises(RuntimeError, match="log="):
        WaeStep(cfg, DEV, 1).history()


def test_dual_step_rows_hold_both_scalar_blocks(deterministic):
    """The Dual step's ``logs()`` merges two device blocks and has four optimizers: a fed run of 4 steps, default mask
    (the latent discriminator keeps its rate)."""
    from fmri_hip.schedule import EpochSchedule, TrainLog
    ref, base = _reference("dual1", DECAYS, steps=4)
    st = _make("dual1", EpochSchedule(**DECAYS), log=TrainLog(capacity=16))
    for _ in range(4):
        st.step()
    names_lr = ("lr_encoder", "lr_decoder", "lr_discriminator", "lr_wae_discriminator")
    _check_rows(st.history(), ref, 0, names_lr, base, DECAYS, masked=(3,))


def test_capture_forward_rows_equal_logs(deterministic):
    """The hybrid launch mode (recorded forward, eager backward) appends behind its updates as well: every row equals the
    ``logs()`` read right after that step in the same run."""
    from fmri_hip.params import ArchConfig
    from fmri_hip.schedule import TrainLog
    from fmri_hip.steps import Stage1Step
    cfg = ArchConfig.px64()
    gen = torch.Generator().manual_seed(2)
    x = torch.rand(4, 3, 64, 64, generator=gen).mul(2).sub(1).to(DEV)
    eps, z_p = (torch.randn(4, cfg.latent_dim, generator=gen).to(DEV) for _ in range(2))
    st = Stage1Step(cfg, DEV, log=TrainLog(capacity=16))
    st.load_recipe(0, True)
    run = st.capture_forward(x, eps, z_p)                           # two warm-up steps: rows 0 and 1
    ref = [None, None]
    for _ in range(3):
        run()
        _finish()
        ref.append(st.logs())
    h = st.history()
    assert h["step"].tolist() == [0, 1, 2, 3, 4] and h["epoch"].tolist() == [-1] * 5
    sel = {k: v[2:] for k, v in h.items()}
    sel["step"] = h["step"][2:]
    _check_rows(sel, ref, 2, ("lr_encoder", "lr_decoder", "lr_discriminator"))
