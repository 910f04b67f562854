"""The pictures of a validation pass (fmri_hip/evaluate.py grids= / dump= / generate=; fmri_hip/egress.py) against the
torch-CPU restatement of make_grid / save_image (tests/egress_oracle.py), and that a pass which writes them leaves
training and every existing column exactly where they were.  Configurations, N_VAL = 10 and B = 4 (batches 4, 4, 2) as
tests/test_evaluator_gpu.py; deterministic mode."""
import numpy as np
import pytest
import torch

import egress_oracle as EG
from test_evaluator_gpu import B, DEV, N_VAL, _cfgs, _datasets, _make, _training_state

pytestmark = pytest.mark.gpu

SEED = 31


@pytest.fixture(autouse=True)
def _deterministic(deterministic):
    yield


def _grid(x_nchw, count=25):
    return EG.grid_u8(x_nchw[:count].cpu(), nrow=5, padding=2).numpy()


def _evaluator(step, va, **kw):
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.rng import DeviceRng
    return Evaluator(step, va, batch=B, rng=DeviceRng(SEED, DEV), **kw)


def test_grids_match_oracle():
    """valid_* = the oracle's grid of last_output() / last_truth() (the short last batch: two images, a 68 x 134 grid),
    train_* that of the step's training block and its train-mode x_tilde (B = 4 images)."""
    from fmri_hip.egress import GridSink
    from fmri_hip.ops import nhwc_to_images
    step, va = _make("stage1", with_log=False)
    sink = GridSink(capacity=4, count=25)
    ev = _evaluator(step, va, grids=sink)
    step.step()
    ev.train_batch()
    ev.run()
    g = sink.images()
    assert g["pass"].tolist() == [0] and g["present"].tolist() == [[True, True, True, True, False]]
    assert "random" not in g
    assert g["valid_output"].shape == (1, 68, 134, 3) and g["train_truth"].shape == (1, 68, 4 * 66 + 2, 3)
    assert np.array_equal(g["valid_output"][0], _grid(ev.last_output()))
    assert np.array_equal(g["valid_truth"][0], _grid(ev.last_truth()))
    d = step.fw["disc_in"]
    assert np.array_equal(g["train_truth"][0], _grid(nhwc_to_images(d[:B], 3)))
    assert np.array_equal(g["train_output"][0], _grid(nhwc_to_images(d[B:2 * B], 3)))
    assert g["valid_output"].std() > 10 and g["train_output"].std() > 10          # pictures, not a flat field


def test_count_limits_the_grid():
    from fmri_hip.egress import GridSink
    step, va = _make("wae1", with_log=False)
    sink = GridSink(capacity=2, count=3, nrow=2, padding=1)
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.feed import DeviceDataset
    ev = Evaluator(step, DeviceDataset(va.images[:8]), batch=B, grids=sink)      # last batch: 4 images, 3 in the grid
    ev.run()
    g = sink.images()
    assert g["valid_output"].shape == (1, 2 * 65 + 1, 2 * 65 + 1, 3)
    assert np.array_equal(g["valid_output"][0], EG.grid_u8(ev.last_output()[:3].cpu(), nrow=2, padding=1).numpy())


@pytest.mark.parametrize("resize", [200, None], ids=["to200", "asis"])
def test_dump_matches_oracle(resize):
    """Every image of every batch: the reconstructions of a batch are collected by re-running it alone -- an evaluator
    over that batch's rows whose generator starts at the offset the pass had reached -- and the truth half is the oracle
    on the ingested images."""
    from fmri_hip.egress import ImageDump
    from fmri_hip.evaluate import Evaluator, batch_ranges
    from fmri_hip.feed import DeviceDataset
    from fmri_hip.rng import DeviceRng, blocks
    step, va = _make("stage1", with_log=False)
    step.step()
    dump = ImageDump(resize=resize)
    ev = _evaluator(step, va, dump=dump)
    ev.run()
    got = dump.images()
    R = resize or 64
    assert got["output"].shape == got["truth"].shape == (N_VAL, R, R, 3) and got["output"].dtype == np.uint8
    offset, Z = 0, step.cfg.latent_dim
    for r0, b in batch_ranges(N_VAL, B):
        g = DeviceRng(SEED, DEV)
        g.seed(SEED, offset)
        one = Evaluator(step, DeviceDataset(va.images[r0:r0 + b]), batch=b, rng=g)
        one.run()
        offset += blocks(b * Z)
        assert np.array_equal(got["output"][r0:r0 + b], EG.images_u8(one.last_output().cpu(), resize=resize).numpy()), r0
        assert np.array_equal(got["truth"][r0:r0 + b], EG.images_u8(one.last_truth().cpu(), resize=resize).numpy()), r0
    assert ev.rng.offset() == offset
    assert got["output"].std() > 10


@pytest.mark.parametrize("kind", ["stage1", "wae1"])
def test_random_grid_and_untouched_columns(kind):
    """generate = 30, count = 25: the `random` grid is the oracle's grid of an eval-mode decoder forward of
    DeviceRng.normal(30, Z, SID_GENERATE) at the offset the pass ends on (Stage-I WAE: times 0.5), the same for the same
    (seed, offset), and history() / last_noise() / the outputs have the bits of a pass without grids, dump and generate."""
    from fmri_hip import lib
    from fmri_hip.egress import GridSink, ImageDump
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.ops import nhwc_to_images, rows_to_f16
    from fmri_hip.rng import SID_GENERATE, DeviceRng

    def one_pass(**kw):
        step, va = _make(kind, with_log=False)
        step.step()
        ev = _evaluator(step, va, **kw)
        ev.train_batch()
        ev.run()
        return step, ev

    sink = GridSink(capacity=2, count=25)
    step, ev = one_pass(grids=sink, dump=ImageDump(resize=None), generate=30)
    rnd = sink.images()
    assert rnd["present"].tolist() == [[True] * 5] and rnd["random"].shape == (1, 332, 332, 3)
    # the oracle: the engine's own decoder in eval mode on the same draw
    seed, offset = ev._gen_rng.state()
    g = DeviceRng(seed, DEV)
    g.seed(seed, offset)
    z = g.normal(30, step.cfg.latent_dim, SID_GENERATE, scale=0.5 if kind == "wae1" else 1.0)
    bns = step.dec.all_bns()
    for bn in bns:
        bn.eval_mode = True
    try:
        y, _ = step.dec.forward(rows_to_f16(z), 1)
    finally:
        for bn in bns:
            bn.eval_mode = False
    assert np.array_equal(rnd["random"][0], _grid(nhwc_to_images(y, 3)))
    assert rnd["random"].std() > 10
    # reproducible, and a plain pass has the same columns, noise and outputs
    sink2 = GridSink(capacity=2, count=25)
    _, ev2 = one_pass(grids=sink2, generate=30)
    assert np.array_equal(sink2.images()["random"], rnd["random"])
    _, plain = one_pass()
    h, hp = ev.history(), plain.history()
    assert h.keys() == hp.keys()
    for k in hp:
        assert np.array_equal(h[k], hp[k], equal_nan=True), k
    assert torch.equal(ev.last_output(), plain.last_output()) and torch.equal(ev.batch_metrics(), plain.batch_metrics())
    if kind == "stage1":
        assert torch.equal(ev.last_noise(), plain.last_noise())
        assert ev.rng.state() == plain.rng.state()
    assert not any(bn.eval_mode for n in (step.enc if kind == "stage1" else step.img_enc, step.dec) for bn in n.all_bns())


def _six_steps(kind, captured, with_images):
    from fmri_hip.egress import GridSink, ImageDump
    step, va = _make(kind)
    ev = _evaluator(step, va, grids=GridSink(capacity=2), dump=ImageDump(resize=None), generate=30) if with_images else None
    run = step.capture() if captured else step.step
    for s in range(6):
        run()
        if ev is not None and s in (1, 3):
            ev.train_batch()
            ev.run()
    torch.cuda.synchronize()
    return _training_state(step), step.history(), ev


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "replayed"])
@pytest.mark.parametrize("kind", ["stage1", "wae1"])
def test_training_is_untouched_by_image_passes(kind, captured):
    """Six steps plain, and six steps with train_batch() + run() with grids, dump and generate after steps 2 and 4:
    parameters, BatchNorm buffers, optimizer state, generator / feed state and the training log are bitwise the same."""
    plain, log_p, _ = _six_steps(kind, captured, False)
    mixed, log_m, ev = _six_steps(kind, captured, True)
    assert plain.keys() == mixed.keys()
    for k in plain:
        assert torch.equal(plain[k], mixed[k]), k
    assert log_p.keys() == log_m.keys()
    for k in log_p:
        assert np.array_equal(log_p[k], log_m[k], equal_nan=True), k
    g = ev.grids.images()
    assert g["pass"].tolist() == [0, 1] and g["present"].all()


def test_ring_keeps_the_last_passes_and_clears_present():
    """capacity = 2, three passes: passes 1 and 2 remain.  Pass 2 re-uses the slot of pass 0, which had training grids;
    pass 2 has none: its ``present`` flags are cleared on the device and its valid_* grids are its own."""
    from fmri_hip.egress import GridSink
    step, va = _make("stage1", with_log=False)
    sink = GridSink(capacity=2)
    ev = _evaluator(step, va, grids=sink)
    valid = []
    for p in range(3):
        step.step()
        if p < 2:
            ev.train_batch()
        ev.run()
        valid.append(_grid(ev.last_output()))
    g = sink.images()
    assert g["pass"].tolist() == [1, 2]
    assert g["present"].tolist() == [[True, True, True, True, False], [False, False, True, True, False]]
    assert np.array_equal(g["valid_output"][0], valid[1]) and np.array_equal(g["valid_output"][1], valid[2])
    assert not np.array_equal(valid[1], valid[2])
    assert ev.history()["pass"].tolist() == [0, 1, 2]


def test_argument_errors():
    from fmri_hip.egress import GridSink, ImageDump
    from fmri_hip.evaluate import Evaluator
    from fmri_hip.rng import DeviceRng
    from fmri_hip.wae_steps import WaeStep
    cfg_e, _ = _cfgs()
    _, va = _datasets()
    wae = WaeStep(cfg_e, DEV, stage=1)
    with pytest.raises(ValueError, match="rng"):
        Evaluator(wae, va, batch=B, grids=GridSink(), generate=30)
    with pytest.raises(ValueError, match="grids"):
        Evaluator(wae, va, batch=B, rng=DeviceRng(1, DEV), generate=30)
    with pytest.raises(ValueError, match="generate"):
        Evaluator(wae, va, batch=B, generate=-1)
    with pytest.raises(ValueError, match="count"):
        GridSink(count=0)
    with pytest.raises(ValueError, match="32 x 32"):
        Evaluator(wae, va, batch=B, grids=GridSink(image_size=32))
    with pytest.raises(ValueError, match="smaller"):
        Evaluator(wae, va, batch=B, dump=ImageDump(resize=32))
    sink = GridSink()
    Evaluator(wae, va, batch=B, grids=sink)
    with pytest.raises(ValueError, match="already attached"):
        Evaluator(wae, va, batch=B, grids=sink)
