"""``fmri_augment=VoxelAugment(...)`` on the Stage-II / Stage-III steps (fmri_hip/voxaug.py; px64, B = 4, V = 256,
deterministic reductions; CognitiveStep stage 2 / 3 and WaeStep stage 2 / 3):
  * under the neutral table a step built with the keyword is bit for bit the step built without it;
  * with a drawn table the step is bit for bit the plain step that is handed ``VoxelAugment.apply``'s rows (fp16 -> fp32
    -> fp16 is exact) and the noise ``DeviceRng.normal`` draws at that offset: the kernels are pinned against the oracle
    in tests/test_voxaug_kernels_gpu.py, here only the plumbing is;
  * the draws follow the noise convention: one advance per step, fresh rows per step and per replay of a recorded step,
    reproducible from the seed, restored with the generator; a feed's buffers keep the clean rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, V, H = 4, 256, 64
KINDS = ["stage2", "stage3", "wae2", "wae3"]
SEED = 5


def _cfgs():
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    return O, O.ArchCfg.px64(), ArchConfig.px64()


_DATA = {}


def _data():
    if not _DATA:
        O, cfg_o, _ = _cfgs()
        d = O.synth_batch(B, cfg_o, n_voxels=V, seed=1234, steps=2)
        _DATA.update(xd=d["x"].to(DEV), fd=d["fmri"].to(DEV).contiguous(), nd=d["noise"].to(DEV))
    return _DATA


def _va():
    from fmri_hip.voxaug import VoxelAugment
    return VoxelAugment(noise=0.2, dropout=0.2, span=0.1, gain=0.1)


def _make(kind, augmented=False, seed=SEED, **kw):
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import CognitiveStep
    from fmri_hip.wae_steps import WaeStep
    _, _, cfg = _cfgs()
    if augmented:
        kw.update(fmri_augment=_va())
        kw.setdefault("rng", DeviceRng(seed, DEV))
    stage = int(kind[-1])
    if kind.startswith("stage"):
        st = CognitiveStep(cfg, V, DEV, stage, **kw)
        st.load_recipe(3, True)
    else:
        st = WaeStep(cfg, DEV, stage, V, **kw)
        st.load_recipe(5)
    return st


def _step(kind, st, fmri, noise=None, **kw):
    """One step on the fixture's images with the fMRI rows ``fmri``; ``noise``: the latent noise tensors of a
    CognitiveStep (None: the step draws them; a WaeStep of stage 2 / 3 takes none)."""
    x = _data()["xd"]
    if kind.startswith("stage"):
        return st.step(fmri, x, *(noise if noise is not None else ()), **kw)
    return st.step(x, None, fmri, **kw)


def _finish():
    from fmri_hip import ops
    ops.join_side()
    torch.cuda.synchronize()


def _same_state(a, b, what):
    _finish()
    assert torch.equal(a.scal, b.scal), (what, a.logs(), b.logs())
    if hasattr(a, "flags"):
        assert torch.equal(a.flags, b.flags), what
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (what, k)
    for oa, ob in zip(a.optims, b.optims):
        assert torch.equal(oa.s1, ob.s1), what
        if oa.s2 is not None:
            assert torch.equal(oa.s2, ob.s2), what


def _latent_blocks(kind):
    _, _, cfg = _cfgs()
    return B * cfg.latent_dim // 4 if kind.startswith("stage") else 0


def _per_step(kind):
    from fmri_hip.voxaug import blocks
    assert blocks(B, V) == B * V // 4
    return max(_latent_blocks(kind), B * V // 4)


@pytest.mark.parametrize("kind", KINDS)
def test_neutral_table_changes_nothing(deterministic, kind):
    from fmri_hip import ops
    from fmri_hip.voxaug import VoxelAugment
    d = _data()
    plain, aug = _make(kind), _make(kind, augmented=True)
    neutral = VoxelAugment.neutral(B, DEV)
    assert plain.last_fmri_augment() is None and plain.last_fmri16() is None
    for s in range(2):
        noise = tuple(d["nd"][s][:3])          # eps, z_p, eps_teacher
        _step(kind, plain, d["fd"], noise)
        _step(kind, aug, d["fd"], noise, fmri_aug=neutral)
        _same_state(plain, aug, (kind, s))
        assert aug.last_fmri_augment() is neutral
        assert torch.equal(aug.last_fmri16(), ops.rows_to_f16(d["fd"]))


def _noise_sids(kind, st):
    from fmri_hip.rng import SID_EPS, SID_EPS_TEACHER, SID_ZP
    if not kind.startswith("stage"):
        return None
    return (SID_EPS, SID_ZP, SID_EPS_TEACHER) if st.teacher_enc is not None else (SID_EPS, SID_ZP)


@pytest.mark.parametrize("kind", KINDS)
def test_drawn_augmentation_is_the_plain_step_on_the_augmented_rows(deterministic, kind):
    from fmri_hip.rng import DeviceRng
    _, _, cfg = _cfgs()
    d = _data()
    va = _va()
    aug, plain = _make(kind, augmented=True), _make(kind)
    g = DeviceRng(SEED, DEV)                       # hands the plain step what the augmented one draws
    sids = _noise_sids(kind, aug)
    rows = []
    for s in range(2):
        assert aug.rng.offset() == g.offset() == s * _per_step(kind)
        table = va.table(g, B, V)
        rows16 = va.apply(d["fd"], table, g)
        noise = None if sids is None else [g.normal(B, cfg.latent_dim, sid) for sid in sids]
        g.advance(_per_step(kind))
        _step(kind, aug, d["fd"])
        assert rows16.shape == (B, V)                  # V is a multiple of 8: no pad columns to cut
        _step(kind, plain, rows16.float(), noise)
        _same_state(aug, plain, (kind, s))
        assert torch.equal(aug.last_fmri_augment(), table)
        assert torch.equal(aug.last_fmri16().view(torch.int16), rows16.view(torch.int16))
        assert (table[:, 0] != 1).all() and (table[:, 5] == 26).all()          # the augmentation is on
        rows.append(rows16.clone())
    assert not torch.equal(rows[0], rows[1])           # two steps draw different rows


@pytest.mark.parametrize("kind", ["stage2", "wae3"])
def test_offset_and_reproducibility(deterministic, kind):
    d = _data()

    def run(st, n, **kw):
        out = []
        for _ in range(n):
            _step(kind, st, d["fd"], **kw)
            out.append((st.last_fmri16().clone(), st.last_fmri_augment().clone(), st.scal.clone()))
        _finish()
        return out
    a = _make(kind, augmented=True)
    ra = run(a, 3)
    assert a.rng.offset() == 3 * _per_step(kind)
    assert not torch.equal(ra[0][0], ra[1][0]) and not torch.equal(ra[1][0], ra[2][0])
    assert not torch.equal(ra[0][1], ra[1][1])
    rb = run(_make(kind, augmented=True), 3)
    for s in range(3):
        for ta, tb in zip(ra[s], rb[s]):
            assert torch.equal(ta, tb), (kind, s)
    assert not torch.equal(run(_make(kind, augmented=True, seed=SEED + 1), 1)[0][0], ra[0][0])
    # a handed table pins the row parameters; the element draws still come from the generator, which still advances
    c = _make(kind, augmented=True)
    noise = tuple(d["nd"][0][:3]) if kind.startswith("stage") else None
    _step(kind, c, d["fd"], noise, fmri_aug=ra[0][1])
    assert c.last_fmri_augment() is ra[0][1] and torch.equal(c.last_fmri16(), ra[0][0])
    assert c.rng.offset() == B * V // 4


def test_every_consumer_of_the_generator_in_one_step(deterministic, golden_dir):
    """Stage II with all four things a step draws from its generator at once -- a feed that flips and shifts on it,
    ``augment=``, ``fmri_augment=`` and drawn noise (V of the ``stage2_b4`` golden): after one ``step()`` the offset has
    moved once, by the largest of the four draws, and every draw is bit for bit the lone draw a second generator with
    the same seed makes at the offset the step started from."""
    import os
    from fmri_hip import augment, rng as R, voxaug
    from fmri_hip.augment import DiffAugment
    from fmri_hip.feed import DeviceDataset, DeviceFeed
    from fmri_hip.steps import CognitiveStep
    _, _, cfg = _cfgs()
    Vg, Z, start = int(np.load(os.path.join(golden_dir, "stage2_b4.npz"))["meta/V"]), cfg.latent_dim, 1000
    rs = np.random.RandomState(7)
    pool = torch.from_numpy(rs.randint(0, 256, (16, H, H, 3), dtype=np.uint8)).to(DEV)
    fmri = torch.from_numpy(rs.standard_normal((16, Vg)).astype(np.float32)).to(DEV)
    g, lone = R.DeviceRng(SEED, DEV), R.DeviceRng(SEED, DEV)
    g.seed(SEED, start)
    lone.seed(SEED, start)
    feed = DeviceFeed(DeviceDataset(pool, fmri), B, 77, rng=g, flip=True, max_shift=2)
    da, va = DiffAugment(), _va()
    st = CognitiveStep(cfg, Vg, DEV, 2, rng=g, feed=feed, augment=da, fmri_augment=va)
    st.load_recipe(3, True)
    st.step()
    _finish()
    moved = [R.blocks(B * Z), R.blocks(2 * B), augment.blocks(B), voxaug.blocks(B, Vg)]
    print("blocks: noise, feed, augment, voxaug =", moved)
    assert g.offset() == start + max(moved)
    assert lone.offset() == start
    noise = st.last_noise()
    assert list(noise) == ["eps", "z_p", "eps_teacher"]
    for name, sid in (("eps", R.SID_EPS), ("z_p", R.SID_ZP), ("eps_teacher", R.SID_EPS_TEACHER)):
        assert torch.equal(noise[name], lone.normal(B, Z, sid)), name
    assert torch.equal(st.last_augment(), da.table(lone, B, H))
    table = va.table(lone, B, Vg)
    assert torch.equal(st.last_fmri_augment(), table)
    assert torch.equal(feed.flip, lone.flips(B)) and torch.equal(feed.shift, lone.shifts(B, 2))
    # (and the rows the encoder read are the feed's clean rows under that table and the generator's element draws)
    assert torch.equal(feed.fmri, fmri[feed.last_indices().long()])
    assert torch.equal(st.last_fmri16().view(torch.int16), va.apply(feed.fmri, table, lone).view(torch.int16))


def _fed(seed=SEED):
    from fmri_hip.feed import DeviceDataset, DeviceFeed
    from fmri_hip.rng import DeviceRng
    rs = np.random.RandomState(7)
    pool = torch.from_numpy(rs.randint(0, 256, (16, H, H, 3), dtype=np.uint8)).to(DEV)
    fmri = torch.from_numpy(rs.standard_normal((16, V)).astype(np.float32)).to(DEV)
    g = DeviceRng(seed, DEV)
    return g, DeviceFeed(DeviceDataset(pool, fmri), B, 77, rng=g, flip=True, max_shift=2), fmri


def _run_fed(st, n, fn=None):
    out = []
    for _ in range(n):
        fn() if fn is not None else st.step()
        out.append((st.last_fmri16().clone(), st.last_fmri_augment().clone(), st.scal.clone()))
    _finish()
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_recorded_step_draws_fresh_rows_at_every_replay(deterministic, kind):
    from fmri_hip import ops
    g, feed, _ = _fed()
    eager = _run_fed(_make(kind, augmented=True, rng=g, feed=feed), 5)
    g, feed, fmri = _fed()
    rec = _make(kind, augmented=True, rng=g, feed=feed)
    replay = rec.capture()                             # two eager warm-up steps, then the recording
    got = _run_fed(rec, 3, replay)
    for i in range(3):
        for te, tg in zip(eager[2 + i], got[i]):
            assert torch.equal(te, tg), (kind, i)
    assert not torch.equal(got[0][1], got[1][1]) and not torch.equal(got[1][1], got[2][1])
    # the feed's buffers keep the clean rows of the batch; the encoder read something else
    idx = feed.last_indices().long()
    assert torch.equal(feed.fmri, fmri[idx])
    assert torch.equal(feed.fmri16, ops.rows_to_f16(fmri[idx]))
    assert not torch.equal(rec.last_fmri16(), feed.fmri16)
    assert rec.last_fmri16().data_ptr() != feed.fmri16.data_ptr()


@pytest.mark.parametrize("kind", ["stage2", "wae2"])
def test_restored_step_redraws_the_same_rows(deterministic, kind):
    from fmri_hip.state import StateRing
    d = _data()
    a = _make(kind, augmented=True, checkpoints=StateRing(every=None))

    def run(n):
        out = []
        for _ in range(n):
            _step(kind, a, d["fd"])
            out.append((a.last_fmri16().clone(), a.scal.clone()))
        _finish()
        return out
    run(1)
    a.snapshot()
    first = run(2)
    a.restore(a.checkpoints.states()[-1])
    again = run(2)
    for i in range(2):
        assert torch.equal(first[i][0], again[i][0]) and torch.equal(first[i][1], again[i][1]), (kind, i)


def test_errors():
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import CognitiveStep
    from fmri_hip.voxaug import VoxelAugment
    from fmri_hip.wae_steps import WaeStep
    _, _, cfg = _cfgs()
    d = _data()
    noise = tuple(d["nd"][0][:3])
    with pytest.raises(ValueError, match="rng"):
        CognitiveStep(cfg, V, DEV, 2, fmri_augment=_va())
    with pytest.raises(ValueError, match="rng"):
        WaeStep(cfg, DEV, 2, V, fmri_augment=_va())
    with pytest.raises(ValueError, match="stage"):
        WaeStep(cfg, DEV, 1, fmri_augment=_va(), rng=DeviceRng(1, DEV))
    with pytest.raises(ValueError, match="without"):
        _step("stage2", _make("stage2"), d["fd"], noise, fmri_aug=VoxelAugment.neutral(B, DEV))
    with pytest.raises(ValueError, match="without"):
        _step("wae2", _make("wae2"), d["fd"], fmri_aug=VoxelAugment.neutral(B, DEV))
    st = _make("stage2", augmented=True)
    for bad in (VoxelAugment.neutral(B + 1, DEV), VoxelAugment.neutral(B, DEV).double(), VoxelAugment.neutral(B, "cpu"),
                torch.zeros(B, 7, device=DEV)):
        with pytest.raises(ValueError, match="table"):
            _step("stage2", st, d["fd"], noise, fmri_aug=bad)
