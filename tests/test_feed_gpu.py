"""GPU checks of the device-resident dataset feed (csrc/rng.hip sampler kernels, csrc/ingest.hip gathering kernels,
fmri_hip/feed.py, ``feed=`` of the fused steps): the sampler against the numpy restatement tests/sampler_oracle.py, the
draws with a start index against the whole draw, the gathering kernels bit for bit against the kernels they fuse, and a
fed step -- eager and recorded -- bit for bit against a step that is handed the batches and the noise the oracles predict.
Every comparison is exact (integers, or the same fp32 / fp16 arithmetic on the same inputs)."""
import numpy as np
import pytest
import torch

import rng_oracle as R
import sampler_oracle as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x9E3779B97F4A7C15          # both key words in use
TOL = 1e-5                         # normals against the float64 map (tests/test_rng_gpu.py for where it comes from)


def _lib():
    from fmri_hip import lib
    return lib, lib.ptr


def _state(seed, epoch=0, cursor=0):
    from fmri_hip.rng import _wrap64
    return torch.tensor([_wrap64(seed), epoch, cursor], dtype=torch.int64).to(DEV)


def _i32(a):
    return torch.from_numpy(np.asarray(a).astype(np.int32))


def _pool(N, H=64, W=64, C=3, seed=0):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (N, H, W, C), dtype=np.uint8)).to(DEV)


# ---- indices ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B", [(10, 4), (8, 4), (4, 4), (257, 256)])
def test_sampler_indices_equal_the_oracle_over_two_epochs(N, B):
    lib, P = _lib()
    st = _state(SEED)
    smp = S.Sampler(SEED, N)
    steps = 2 * (N // B) + 1                            # two full epochs and the first batch of the third
    got = torch.empty(steps, B, dtype=torch.int32, device=DEV)
    states = torch.empty(steps, 3, dtype=torch.int64, device=DEV)
    ref = []
    for s in range(steps):
        lib.call("fmri_sampler_indices", P(st), N, B, 0, P(got[s]))
        lib.call("fmri_sampler_advance", P(st), N, B)
        states[s].copy_(st)
        ref.append(smp.next(B))
        ref_state = (smp.epoch, smp.cursor)
        assert states[s, 1:].tolist() == list(ref_state), (s, states[s].tolist(), ref_state)
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), _i32(np.stack(ref)))
    assert smp.epoch >= 2 and int(got.min()) >= 0 and int(got.max()) < N


@pytest.mark.parametrize("N", [1, 2, 3, 5, 16, 17, 255, 1000, 65537])
def test_whole_permutation_tables(N):
    """One launch over a whole epoch (several thread blocks, every length of the cycle walk), epochs 0 and 2^40 + 3."""
    lib, P = _lib()
    for epoch in (0, 2 ** 40 + 3):
        st = _state(SEED, epoch)
        got = torch.full((N + 1,), -7, dtype=torch.int32, device=DEV)
        lib.call("fmri_sampler_indices", P(st), N, N, 0, P(got))
        assert torch.equal(got[:N].cpu(), _i32(S.pi(SEED, epoch, np.arange(N), N))), (N, epoch)
        assert int(got[N]) == -7                        # nothing written behind B entries
        assert st.tolist()[1:] == [epoch, 0]            # reading does not move the state


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("N", [29, 257])
def test_ranks_read_slices_of_the_one_rank_batch(N, W):
    from fmri_hip.feed import DeviceDataset, DeviceFeed
    ds = DeviceDataset(_pool(N, 8, 8))
    one = DeviceFeed(ds, W * 4, SEED, rank=0, world=1)
    ranks = [DeviceFeed(ds, 4, SEED, rank=k, world=W) for k in range(W)]
    smp = S.Sampler(SEED, N)
    for _ in range(N // (W * 4) + 2):                   # across an epoch boundary
        whole = one.next()[2].clone()
        parts = torch.cat([f.next()[2] for f in ranks])
        assert torch.equal(parts, whole) and torch.equal(whole.cpu(), _i32(smp.next(W * 4)))
    assert one.position() == ranks[-1].position() == (smp.epoch, smp.cursor) and smp.epoch >= 1


def test_set_position_resumes_the_sequence_and_a_lone_feed_advances_its_generator():
    from fmri_hip.feed import DeviceDataset, DeviceFeed
    from fmri_hip.rng import DeviceRng
    N, B = 29, 4
    ds = DeviceDataset(_pool(N, 8, 8))
    g = DeviceRng(7, DEV)
    f = DeviceFeed(ds, B, SEED, rng=g, flip=True, max_shift=3)
    seq, flips = [], []
    for _ in range(9):                                  # 7 batches per epoch
        seq.append((f.position(), f.next()[2].clone()))
        flips.append((f.flip.clone(), f.shift.clone()))
    assert g.offset() == 9 * 2                          # the feed advanced its generator: blocks(2 * B) per batch
    assert f.clamped() == 0
    h = DeviceFeed(ds, B, SEED)
    h.set_position(0, 12)
    for k in (3, 4):
        assert h.position() == seq[k][0] == (0, 4 * k)
        assert torch.equal(h.next()[2], seq[k][1])
    h.set_position(1, 4)
    assert torch.equal(h.next()[2], seq[8][1]) and h.position() == (1, 8)
    assert torch.equal(h.last_indices(), seq[8][1].cpu())
    with pytest.raises(ValueError):
        h.set_position(0, 26)                           # no whole batch left
    # the augmentation draws are the oracle's, at the offsets the feed moved through
    for k in (0, 8):
        assert torch.equal(flips[k][0].cpu(), _i32(R.integers(7, 2 * k, B, 0, 1, 8)))
        assert torch.equal(flips[k][1].cpu(), _i32(R.integers(7, 2 * k, 2 * B, -3, 3, 9)).view(B, 2))
    with pytest.raises(ValueError, match="rng"):
        DeviceFeed(ds, B, SEED, flip=True)
    with pytest.raises(ValueError, match="rng"):
        DeviceFeed(ds, B, SEED, max_shift=1)
    with pytest.raises(ValueError):
        DeviceFeed(ds, 30, SEED)                        # dataset smaller than the batch


# ---- draws with a start index ----------------------------------------------------------------------------------------
def test_integer_draws_with_a_start_index():
    from fmri_hip.rng import SID_FLIP, SID_SHIFT, DeviceRng
    lib, P = _lib()
    off = 2 ** 32 - 2
    g = DeviceRng(SEED, DEV)
    g.set_state((SEED, off))
    for n in (1, 3, 4, 5, 1023):
        a = g.integers(n, -5, 5, SID_SHIFT)
        b = torch.empty(n, dtype=torch.int32, device=DEV)
        lib.call("fmri_rng_u32_at", P(g._state), P(b), n, 0, SID_SHIFT, -5, 5)
        assert torch.equal(a, b), n                     # start = 0 is fmri_rng_u32
    whole = g.integers(12, -5, 5, SID_SHIFT)
    assert torch.equal(g.integers(7, -5, 5, SID_SHIFT, start=5), whole[5:12])
    big = g.integers(4100, -2 ** 31, 2 ** 31 - 1, 3)
    for start, n in ((1, 4099), (2, 1), (3, 4), (4, 4096), (4097, 3)):
        buf = torch.full((n + 9,), -7, dtype=torch.int32, device=DEV)
        for shift_out in (0, 1):                        # aligned and unaligned destination
            out = buf[4 + shift_out:4 + shift_out + n]
            g.integers(n, -2 ** 31, 2 ** 31 - 1, 3, out=out, start=start)
            assert torch.equal(out, big[start:start + n]), (start, n, shift_out)
            assert int(buf[3 + shift_out]) == -7 and int(buf[4 + shift_out + n]) == -7
            buf.fill_(-7)
    ref = R.raw_words(SEED, off, 4100, 3).astype(np.int64) - 2 ** 31
    assert torch.equal(big.cpu().long(), torch.from_numpy(ref))
    assert torch.equal(g.flips(4, start=4), g.flips(8)[4:])
    assert torch.equal(g.shifts(4, 3, start=4), g.shifts(8, 3)[4:])
    assert torch.equal(g.shifts(3, 3, start=5), g.shifts(8, 3)[5:])
    assert g.state() == (SEED, off)


# ---- gathering ingest ------------------------------------------------------------------------------------------------
IDX = {1: [10], 3: [10, 0, 10], 8: [0, 10, 3, 3, 7, 0, 10, 5]}     # repeats, first and last row of the pool of 11


def _gather(pool, idx, flip=None, shift=None, want16=True, want32=True, err=None, mean=(0.5,) * 3, std=(0.5,) * 3):
    lib, P = _lib()
    N, H, W, C = pool.shape
    B = idx.numel()
    o16 = torch.full((B, H, W, 8), 7.0, dtype=torch.float16, device=DEV) if want16 else None
    o32 = torch.full((B, 3, H, W), 7.0, dtype=torch.float32, device=DEV) if want32 else None
    lib.call("fmri_ingest_u8_gather", P(pool), P(idx), N, B, H, W, C, P(flip), P(shift), *mean, *std, P(o16), P(o32),
             P(err))
    return o16, o32


@pytest.mark.parametrize("flips", [False, True])
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", [(8, 8), (5, 7), (64, 64)])
def test_gathering_ingest_equals_ingest_of_the_gathered_images(H, W, C, B, flips):
    from fmri_hip import ops
    rs = np.random.RandomState(H * 100 + W * 10 + C + B)
    pool = _pool(11, H, W, C, seed=H + C)
    idx = torch.tensor(IDX[B], dtype=torch.int32, device=DEV)
    shift = _i32(rs.randint(-3, 4, (B, 2))).to(DEV)     # [-3, 3]: more than half of H = 5
    flip = _i32(rs.randint(0, 2, B)).to(DEV) if flips else None
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    got16, got32 = _gather(pool, idx, flip, shift, err=err, mean=mean, std=std)
    ref16, ref32 = ops.ingest_u8(pool[idx.long()].contiguous(), mean, std, flip=flip, shift=shift, want32=True)
    assert torch.equal(got16, ref16) and torch.equal(got32, ref32) and int(err) == 0
    # one output only, no augmentation: the other paths of the kernel
    only16, _ = _gather(pool, idx, want32=False)
    _, only32 = _gather(pool, idx, want16=False)
    p16, p32 = ops.ingest_u8(pool[idx.long()].contiguous(), want32=True)
    assert torch.equal(only16, p16) and torch.equal(only32, p32)


def test_an_index_outside_the_pool_is_clamped_and_counted():
    """The kernels clamp before they form an address: what comes out is the batch of the clamped indices, and the
    counter says how many were moved (once per image / row)."""
    from fmri_hip import ops
    lib, P = _lib()
    pool = _pool(11, 8, 8, 3)
    bad = torch.tensor([-1, 11, 5, 2 ** 31 - 1, -2 ** 31, 10], dtype=torch.int32, device=DEV)
    good = torch.tensor([0, 10, 5, 10, 0, 10], dtype=torch.int64, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    got16, got32 = _gather(pool, bad, err=err)
    ref16, ref32 = ops.ingest_u8(pool[good].contiguous(), want32=True)
    assert torch.equal(got16, ref16) and torch.equal(got32, ref32) and int(err) == 4
    _gather(pool, bad)                                  # the counter is optional
    rows = torch.randn(11, 12, device=DEV)
    out = torch.empty(6, 12, device=DEV)
    lib.call("fmri_gather_rows_f32", P(rows), 11, 12, P(bad), 6, P(out), None, P(err))
    assert torch.equal(out, rows[good]) and int(err) == 8


# ---- row gather ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("V", [1, 7, 8, 12, 3620])
def test_row_gather_equals_index_select(V, B):
    from fmri_hip import ops
    lib, P = _lib()
    g = torch.Generator().manual_seed(V + B)
    src = (torch.randn(11, V, generator=g) * 3).to(DEV)
    idx = torch.tensor(([10, 0, 10, 4, 4])[:B], dtype=torch.int32, device=DEV)
    vp = ops.pad8(V)
    d32 = torch.full((B, V), 7.0, device=DEV)
    d16 = torch.full((B, vp), 7.0, dtype=torch.float16, device=DEV)
    lib.call("fmri_gather_rows_f32", P(src), 11, V, P(idx), B, P(d32), P(d16), None)
    ref = src.index_select(0, idx.long())
    assert torch.equal(d32, ref)
    assert torch.equal(d16, ops.rows_to_f16(ref)) and bool((d16[:, V:] == 0).all())
    only16 = torch.full((B, vp), 7.0, dtype=torch.float16, device=DEV)
    lib.call("fmri_gather_rows_f32", P(src), 11, V, P(idx), B, None, P(only16), None)
    only32 = torch.full((B, V), 7.0, device=DEV)
    lib.call("fmri_gather_rows_f32", P(src), 11, V, P(idx), B, P(only32), None, None)
    assert torch.equal(only16, d16) and torch.equal(only32, ref)
    # rows that do not start on 16 bytes (a view one float into the allocation): the single-load path
    flat = torch.zeros(11 * V + 1, device=DEV)
    flat[1:] = src.reshape(-1)
    off32 = torch.full((B, V), 7.0, device=DEV)
    lib.call("fmri_gather_rows_f32", P(flat[1:]), 11, V, P(idx), B, P(off32), P(only16), None)
    assert torch.equal(off32, ref) and torch.equal(only16, d16)


# ---- the fed steps ---------------------------------------------------------------------------------------------------
def _finish():
    from fmri_hip import ops
    ops.join_side()
    torch.cuda.synchronize()


def _same(a, b, what):
    _finish()
    la, lb = a.logs(), b.logs()
    assert la.keys() == lb.keys()
    for k in la:
        assert la[k] == lb[k], (what, k, la[k], lb[k])
        assert np.isfinite(float(la[k])), (what, k, la[k])
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (what, k)


NPOOL, BATCH, MAX_SHIFT, RNG_SEED, FEED_SEED = 10, 4, 2, 7, 11


class _Expect:
    """What the oracles say a fed step reads, step after step: the sampler's indices, the flips and shifts at the shared
    generator's offset, and that offset -- one advance per step by the larger of blocks(B * Z) and blocks(2 * B)."""

    def __init__(self, pool, Z, fmri=None):
        self.pool, self.fmri, self.Z = pool, fmri, Z
        self.smp = S.Sampler(FEED_SEED, NPOOL)
        self.off = 0

    def next(self):
        """(x fp32 NCHW, fmri rows or None, indices, generator offset of the step) of the next step."""
        from fmri_hip import ops
        from fmri_hip.rng import SID_FLIP, SID_SHIFT
        idx = self.smp.next(BATCH)
        flip = _i32(R.integers(RNG_SEED, self.off, BATCH, 0, 1, SID_FLIP))
        shift = _i32(R.integers(RNG_SEED, self.off, 2 * BATCH, -MAX_SHIFT, MAX_SHIFT, SID_SHIFT)).view(BATCH, 2)
        sel = torch.from_numpy(idx).to(DEV)
        x = ops.ingest_u8(self.pool[sel].contiguous(), flip=flip, shift=shift, want16=False, want32=True)[1]
        off = self.off
        self.off += max(BATCH * self.Z // 4, (2 * BATCH + 3) // 4)
        return x, (self.fmri[sel] if self.fmri is not None else None), _i32(idx), off


def _fed(pool, fmri=None):
    from fmri_hip.feed import DeviceDataset, DeviceFeed
    from fmri_hip.rng import DeviceRng
    g = DeviceRng(RNG_SEED, DEV)
    return g, DeviceFeed(DeviceDataset(pool, fmri), BATCH, FEED_SEED, rng=g, flip=True, max_shift=MAX_SHIFT)


def _recorded_against_handed(make, sids, pool, fmri=None):
    """Engine A: rng + feed, capture(), three replays.  Engine B: no feed, no rng, handed the batch and the noise of the
    same steps.  capture() RUNS its two warm-up steps; the recording itself executes nothing (stream capture), so five
    steps have run after three replays: with 10 samples and batches of 4 an epoch is two batches, the first replay is
    batch 0 of epoch 1 and the third is batch 0 of epoch 2."""
    from fmri_hip import ops
    from fmri_hip.params import ArchConfig
    from fmri_hip.rng import DeviceRng
    cfg = ArchConfig.px64()
    Z = cfg.latent_dim
    g, feed = _fed(pool, fmri)
    a = make(cfg, g, feed)
    b = make(cfg, None, None)
    h = DeviceRng(RNG_SEED, DEV)                        # hands B the noise of A's layout, checked against the oracle below
    exp = _Expect(pool, Z, fmri)

    def hand():
        x, fm, idx, off = exp.next()
        h.set_state((RNG_SEED, off))
        noise = [h.normal(BATCH, Z, sid) for sid in sids]
        b.step(*((fm, x) if fmri is not None else (x,)), *noise)
        return x, fm, idx, off, noise
    replay = a.capture()
    hand()
    hand()
    _finish()
    assert feed.position() == (exp.smp.epoch, exp.smp.cursor) == (1, 0) and g.offset() == exp.off
    for r in range(3):
        replay()
        x, fm, idx, off, noise = hand()
        _finish()
        assert torch.equal(feed.last_indices(), idx), r
        assert feed.position() == (exp.smp.epoch, exp.smp.cursor) and g.offset() == exp.off
        assert torch.equal(feed.x, x)
        if fmri is not None:
            assert torch.equal(feed.fmri, fm)           # image and fMRI row of a sample carry the same index
            assert torch.equal(feed.fmri16, ops.rows_to_f16(fm))        # what the fed step's encoder read
        drawn = list(a.last_noise().values())
        for sid, t, n in zip(sids, drawn, noise):
            assert torch.equal(t, n)
            err = float(np.abs(t.double().cpu().numpy() - R.normal(RNG_SEED, off, BATCH, Z, sid=sid)).max())
            assert err <= TOL, (r, sid, err)
    assert feed.position() == (2, 4) and feed.clamped() == 0
    _same(a, b, "two warm-up + three replayed fed steps against five handed ones")


def test_a_recorded_fed_stage1_step_replays_epochs(deterministic):
    from fmri_hip.rng import SID_EPS, SID_ZP
    from fmri_hip.steps import Stage1Step

    def make(cfg, g, feed):
        st = Stage1Step(cfg, DEV, rng=g, feed=feed)
        st.load_recipe(0, True)
        return st
    _recorded_against_handed(make, (SID_EPS, SID_ZP), _pool(NPOOL))


def test_a_recorded_fed_stage2_step_draws_image_and_fmri_of_the_same_samples(deterministic):
    from fmri_hip.rng import SID_EPS, SID_EPS_TEACHER, SID_ZP
    from fmri_hip.steps import CognitiveStep
    V = 37
    fmri = torch.randn(NPOOL, V, generator=torch.Generator().manual_seed(3)).to(DEV)

    def make(cfg, g, feed):
        st = CognitiveStep(cfg, V, DEV, 2, rng=g, feed=feed)
        st.load_recipe(3, True)
        return st
    _recorded_against_handed(make, (SID_EPS, SID_ZP, SID_EPS_TEACHER), _pool(NPOOL), fmri)


@pytest.mark.parametrize("kind", ["wae1", "dual1"])
def test_other_fed_steps_equal_the_handed_step(deterministic, kind):
    from fmri_hip.params import ArchConfig
    from fmri_hip.wae_steps import DualStage1Step, WaeStep
    cfg = ArchConfig.px64()
    pool = _pool(NPOOL)

    def make(g, feed):
        if kind == "wae1":
            st = WaeStep(cfg, DEV, 1, rng=g, feed=feed)
            st.load_recipe(5, False)
        else:
            st = DualStage1Step(cfg, DEV, rng=g, feed=feed)
            st.load_recipe(8, True)
        return st
    g, feed = _fed(pool)
    a, b = make(g, feed), make(None, None)
    exp = _Expect(pool, cfg.latent_dim)
    a.step()
    x, _, idx, _ = exp.next()
    assert torch.equal(feed.last_indices(), idx) and torch.equal(feed.x, x)
    assert g.offset() == exp.off == BATCH * cfg.latent_dim // 4 and feed.position() == (0, 4)
    b.step(x, *a.last_noise().values())
    _same(a, b, kind)


def test_a_fed_step_takes_no_batch_and_an_unfed_step_needs_one():
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import CognitiveStep, Stage1Step
    cfg = ArchConfig.px64()
    g, feed = _fed(_pool(NPOOL))
    x = torch.zeros(BATCH, 3, 64, 64, device=DEV)
    fed = Stage1Step(cfg, DEV, rng=g, feed=feed)
    with pytest.raises(ValueError, match="feed"):
        fed.step(x)
    assert feed.position() == (0, 0)                    # refused before anything was drawn
    plain = Stage1Step(cfg, DEV, rng=g)
    with pytest.raises(ValueError, match="feed"):
        plain.step()
    with pytest.raises(ValueError, match="fMRI"):
        CognitiveStep(cfg, 37, DEV, 2, rng=g, feed=feed)        # the feed's dataset has no fMRI rows
