"""GPU checks of the device generator (csrc/rng.hip, fmri_hip/rng.py) against the numpy restatement tests/rng_oracle.py,
and of the fused steps drawing their own noise: a step that draws equals, bit for bit, a step that is handed the same
numbers, and a step recorded into a HIP graph draws fresh, oracle-exact noise at every replay.

Bound on the normals, |kernel - float64 map| <= 1e-5 * scale, from the arithmetic (not from the kernel's output): the
argument 2 pi u carries up to 2 pi 2^-24 ~ 3.7e-7 of rounding, times r <= 5.89; logf, sqrtf, sincosf and the products add
a few fp32 ulp of a value <= 5.89 (~5e-7 each): ~4e-6 in total, a 2.5 x margin.  Every element is compared."""
import numpy as np
import pytest
import torch

import rng_oracle as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
SEED = 0x9E3779B97F4A7C15          # both key words in use


def _rng(seed=SEED, offset=0):
    from fmri_hip.rng import DeviceRng
    g = DeviceRng(seed, DEV)
    if offset:
        g.set_state((seed, offset))
    return g


def _max_err(got: torch.Tensor, ref: np.ndarray) -> float:
    assert tuple(got.shape) == ref.shape
    err = float(np.abs(got.double().cpu().numpy() - ref).max())
    print("max abs error", err)
    return err


# ---- kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", [0, 9])
@pytest.mark.parametrize("offset", [0, 2 ** 32 - 1])
def test_raw_words_equal_the_oracle(offset, sid):
    """lo = -2^31, hi = 2^31 - 1: the multiply-high is the identity, the output the Philox words themselves (plus lo)."""
    g = _rng(offset=offset)
    for n in (1, 3, 4, 5, 1023, 4097):
        got = g.integers(n, -2 ** 31, 2 ** 31 - 1, sid)
        ref = torch.from_numpy(R.raw_words(SEED, offset, n, sid).astype(np.int64))
        assert got.dtype == torch.int32 and torch.equal(got.cpu().long() + 2 ** 31, ref), (n, offset, sid)
    assert g.state() == (SEED, offset)                  # draws do not move the offset


@pytest.mark.parametrize("rows,cols,ld", [(4, 128, 128), (5, 127, 127), (1, 1, 1), (256, 128, 128), (4, 128, 136)])
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_normals_match_the_float64_map(rows, cols, ld, scale):
    g = _rng(offset=5)
    buf = torch.full((rows, ld), -777.0, dtype=torch.float32, device=DEV)
    out = g.normal(rows, cols, 1, scale=scale, out=buf[:, :cols])
    ref = R.normal(SEED, 5, rows, cols, sid=1, scale=scale)
    assert _max_err(out, ref) <= TOL * scale
    if ld > cols:                                       # the tail columns of a wider buffer stay untouched
        assert torch.all(buf[:, cols:] == -777.0)
    assert torch.equal(g.normal(rows, cols, 1, scale=scale), out.contiguous())       # fresh buffer, same numbers


def test_normals_at_an_unaligned_global_row_and_offset_carry():
    """row0 * cols no multiple of 4 (first and last Philox block shared with rows outside the draw), 64-bit offset."""
    off = 2 ** 32 - 3
    g = _rng(offset=off)
    for rows, cols, row0 in ((3, 127, 5), (2, 1, 7), (6, 130, 1)):
        out = g.normal(rows, cols, 0, row0=row0)
        assert _max_err(out, R.normal(SEED, off, rows, cols, row0=row0)) <= TOL


def test_draws_are_invariant_to_the_world_size():
    g = _rng()
    full = g.normal(8, 128, 0)
    for first in (4, 3):                                # 4 + 4 and 3 + 5
        g.set_state((SEED, 0))
        lo, hi = g.normal(first, 128, 0), g.normal(8 - first, 128, 0, row0=first)
        assert torch.equal(lo, full[:first]) and torch.equal(hi, full[first:])
    odd = g.normal(8, 127, 0)
    assert torch.equal(g.normal(5, 127, 0, row0=3), odd[3:])                          # block-unaligned split


def test_advance_moves_the_offset_and_the_numbers():
    g = _rng(offset=2 ** 32 - 2)
    a, b = g.normal(4, 128, 0), g.normal(4, 128, 0)
    assert torch.equal(a, b)                            # no advance: the same draw
    g.advance(128)
    assert g.offset() == 2 ** 32 - 2 + 128
    c = g.normal(4, 128, 0)
    assert not torch.equal(a, c)
    assert _max_err(c, R.normal(SEED, 2 ** 32 - 2 + 128, 4, 128)) <= TOL
    g.advance(0)
    assert g.offset() == 2 ** 32 - 2 + 128
    g.seed(5)
    assert g.state() == (5, 0)


def test_flips_and_shifts_feed_the_ingest_kernel():
    from fmri_hip import ops
    from fmri_hip.rng import SID_FLIP, SID_SHIFT
    g = _rng(offset=3)
    flip, shift = g.flips(7), g.shifts(7, 5)
    assert flip.dtype == torch.int32 and tuple(flip.shape) == (7,)
    assert shift.dtype == torch.int32 and tuple(shift.shape) == (7, 2)
    assert torch.equal(flip.cpu(), torch.from_numpy(R.integers(SEED, 3, 7, 0, 1, SID_FLIP).astype(np.int32)))
    assert torch.equal(shift.cpu(), torch.from_numpy(R.integers(SEED, 3, 14, -5, 5, SID_SHIFT).astype(np.int32)).view(7, 2))
    assert int(flip.min()) >= 0 and int(flip.max()) <= 1 and int(shift.abs().max()) <= 5
    big = g.integers(1 << 16, -5, 5, SID_SHIFT)
    assert torch.equal(big.cpu(), torch.from_numpy(R.integers(SEED, 3, 1 << 16, -5, 5, SID_SHIFT).astype(np.int32)))
    img = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (7, 16, 16, 3), dtype=np.uint8)).to(DEV)
    got16, got32 = ops.ingest_u8(img, flip=flip, shift=shift, want32=True)
    ref16, ref32 = ops.ingest_u8(img, flip=torch.tensor(flip.tolist(), dtype=torch.int32),
                                 shift=torch.tensor(shift.tolist(), dtype=torch.int32), want32=True)
    assert torch.equal(got16, ref16) and torch.equal(got32, ref32) and bool(torch.isfinite(got32).all())
    plain = ops.ingest_u8(img, want32=True)[1]
    assert not torch.equal(got32, plain)                # the draws did something


# ---- the steps -------------------------------------------------------------------------------------------------------
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


def _batch(B, V=0, seed=1234):
    from oracle import vaegan_oracle as O
    data = O.synth_batch(B, O.ArchCfg.px64(), n_voxels=V, seed=seed, steps=1) if V else \
        O.synth_batch(B, O.ArchCfg.px64(), seed=seed, steps=1)
    return data


def _check_noise(noise, names, offset, B, Z, seed=7):
    from fmri_hip import rng as G
    sids = dict(eps=G.SID_EPS, z_p=G.SID_ZP, eps_teacher=G.SID_EPS_TEACHER, z_fake_noise=G.SID_ZFAKE)
    assert list(noise) == list(names)
    for k in names:
        assert noise[k].dtype == torch.float32 and tuple(noise[k].shape) == (B, Z)
        assert _max_err(noise[k], R.normal(seed, offset, B, Z, sid=sids[k])) <= TOL, k


def test_stage1_step_draws_what_it_would_have_been_handed(deterministic):
    from fmri_hip.params import ArchConfig
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import Stage1Step
    cfg, B = ArchConfig.px64(), 4
    x = _batch(B)["x"].to(DEV)
    g = DeviceRng(7, DEV)
    a = Stage1Step(cfg, DEV, rng=g)
    a.load_recipe(0, True)
    a.step(x)
    noise = a.last_noise()
    _check_noise(noise, ("eps", "z_p"), 0, B, cfg.latent_dim)
    assert g.offset() == B * cfg.latent_dim // 4        # one advance, by the blocks of a [B, Z] draw
    b = Stage1Step(cfg, DEV)
    b.load_recipe(0, True)
    b.step(x, *noise.values())
    _same(a, b, "stage 1")
    assert list(b.last_noise()) == ["eps", "z_p"]
    # a second step draws other numbers, at the advanced offset; a handed tensor is used as it is
    first = {k: v.clone() for k, v in noise.items()}
    a.step(x)
    _check_noise(a.last_noise(), ("eps", "z_p"), B * cfg.latent_dim // 4, B, cfg.latent_dim)
    assert not torch.equal(a.last_noise()["eps"], first["eps"])
    a.step(x, z_p=first["z_p"])
    assert a.last_noise()["z_p"] is first["z_p"] and g.offset() == 3 * B * cfg.latent_dim // 4
    _finish()


def test_a_step_without_rng_and_without_noise_is_an_error():
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import Stage1Step
    st = Stage1Step(ArchConfig.px64(), DEV)
    x = _batch(4)["x"].to(DEV)
    with pytest.raises(ValueError, match="rng"):
        st.step(x)
    with pytest.raises(ValueError, match="z_p"):
        st.step(x, torch.zeros(4, 128, device=DEV))


@pytest.mark.parametrize("kind", ["stage2", "wae1", "dual1"])
def test_other_steps_draw_what_they_would_have_been_handed(deterministic, kind):
    """CognitiveStep stage 2 (eps, z_p and the teacher's eps), WaeStep stage I (z_fake_noise) and DualStage1Step (all of
    Stage I's and z_fake_noise): one step each, drawn against handed."""
    from fmri_hip.params import ArchConfig
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import CognitiveStep
    from fmri_hip.wae_steps import DualStage1Step, WaeStep
    cfg, B, V = ArchConfig.px64(), 4, 64
    data = _batch(B, V if kind == "stage2" else 0)
    x = data["x"].to(DEV)

    def make(rng):
        if kind == "stage2":
            st = CognitiveStep(cfg, V, DEV, 2, rng=rng)
            st.load_recipe(3, True)
            fm = data["fmri"].to(DEV)
            return st, (lambda *nz: st.step(fm, x, *nz)), ("eps", "z_p", "eps_teacher")
        if kind == "wae1":
            st = WaeStep(cfg, DEV, 1, rng=rng)
            st.load_recipe(5, False)
            return st, (lambda *nz: st.step(x, *nz)), ("z_fake_noise",)
        st = DualStage1Step(cfg, DEV, rng=rng)
        st.load_recipe(8, True)
        return st, (lambda *nz: st.step(x, *nz)), ("eps", "z_p", "z_fake_noise")
    g = DeviceRng(7, DEV)
    a, run_a, names = make(g)
    b, run_b, _ = make(None)
    run_a()
    noise = a.last_noise()
    _check_noise(noise, names, 0, B, cfg.latent_dim)
    assert g.offset() == B * cfg.latent_dim // 4
    run_b(*noise.values())
    _same(a, b, kind)
    with pytest.raises(ValueError):
        run_b()


def test_a_recorded_step_draws_fresh_noise_at_every_replay(deterministic):
    from fmri_hip.params import ArchConfig
    from fmri_hip.rng import DeviceRng
    from fmri_hip.steps import Stage1Step
    cfg, B = ArchConfig.px64(), 4
    Z = cfg.latent_dim
    x = _batch(B)["x"].to(DEV)
    g = DeviceRng(7, DEV)
    a = Stage1Step(cfg, DEV, rng=g)
    a.load_recipe(0, True)
    replay = a.capture(x)
    off0 = g.offset()
    replay()
    _finish()
    n1 = {k: v.clone() for k, v in a.last_noise().items()}
    off1 = g.offset()
    replay()
    _finish()
    n2 = a.last_noise()
    off2 = g.offset()
    assert off1 - off0 == off2 - off1 == B * Z // 4
    assert not torch.equal(n1["eps"], n2["eps"]) and not torch.equal(n1["z_p"], n2["z_p"])
    _check_noise(n1, ("eps", "z_p"), off0, B, Z)
    _check_noise(n2, ("eps", "z_p"), off1, B, Z)
    logs = a.logs()
    for k in ("loss_encoder", "loss_decoder", "loss_discriminator", "kl", "mse"):
        assert np.isfinite(logs[k]), (k, logs[k])
    # the replayed step is the eager step: a second engine handed the two noise sets in turn, from the same start
    # (capture() runs two warm-up steps first: it is handed their noise as well, from the oracle-checked layout)
    b = Stage1Step(cfg, DEV)
    b.load_recipe(0, True)
    h = DeviceRng(7, DEV)
    for _ in range(2):
        b.step(x, h.normal(B, Z, 0), h.normal(B, Z, 1))
        h.advance(B * Z // 4)
    b.step(x, n1["eps"], n1["z_p"])
    b.step(x, n2["eps"], n2["z_p"])
    _same(a, b, "two warm-up + two replayed steps against four eager ones")
