"""fmri_nway_scores (csrc/nway.hip) through ident.nway_scores16: both similarity matrices against the float64 oracle of
tests/ident_oracle.py, the counting against the host counting on the returned matrices (exactly) and on the float64
matrices (end to end), the draws against the Philox oracle, and the bitwise invariants of include/fmri_hip.h.

Inputs are synth_batch / edge_batch rounded to fp16 and packed with eval_oracle.to_layout; the oracle sees the same fp16
values.  Shapes (n, C, H, W) are the smallest that reach each path: (2, 3, 11, 11) minimum n, the window spans the image;
(19, 3, 24, 20) partial 16-tiles in n, H and W, D = 1440 (two K chunks); (33, 3, 16, 16) three tile groups and an exact
tie; (17, 1, 13, 37) C = 1, three tiles wide; (16, 1, 25, 41) D = 1025, a last K chunk of one element."""
import functools

import numpy as np
import pytest
import torch

import eval_oracle as EO
import ident_oracle as IO
import rng_oracle as RO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 2e-6                      # the project's bar for every metric kernel against float64
SEED, RNG_SEED, RNG_OFFSET = 3, 0x5EED1234, 41
SHAPES = {"n2": (2, 3, 11, 11), "n19": (19, 3, 24, 20), "n33dup": (33, 3, 16, 16), "c1wide": (17, 1, 13, 37),
          "k1025": (16, 1, 25, 41)}
DUP = (4, 9)
# float64 margins |S_ij - S_ii|, j != i, of the three synth batches below at SEED (checked on the CPU): 600 x the bar
MARGIN_PCC, MARGIN_SSIM = 8e-3, 1.2e-3


def _fp16(x):
    return x.half().float()


@functools.lru_cache(maxsize=None)
def batch(name, kind="synth"):
    """(pred, truth) fp32 CPU holding fp16 values, their layouts on the device, and the float64 matrices."""
    n, c, h, w = SHAPES[name]
    if kind == "edge":
        p, t = IO.edge_batch(n, n, c, h, w, SEED)
    else:
        p, t = IO.synth_batch(n, c, h, w, SEED, dup=DUP if name == "n33dup" else None)
    p, t = _fp16(p), _fp16(t)
    return dict(pred=p, truth=t, p16=EO.to_layout(p).to(DEV), t16=EO.to_layout(t).to(DEV), C=c,
                pcc64=IO.pcc_matrix64(p, t), ssim64=IO.ssim_matrix64(p, t))


def _rng(offset=RNG_OFFSET):
    from fmri_hip.rng import DeviceRng
    g = DeviceRng(RNG_SEED, DEV)
    g.seed(RNG_SEED, offset)
    return g


def run(b, top=5, rng=True, **kw):
    from fmri_hip import ident
    out = ident.nway_scores16(kw.pop("p16", b["p16"]), kw.pop("t16", b["t16"]), top, rng=_rng() if rng is True else rng,
                              C=b["C"], **kw)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def engine(name, kind="synth"):
    return run(batch(name, kind))


def host_draws(n, top, offset=RNG_OFFSET, sid=10):
    u = RO.integers(RNG_SEED, offset, n * (top - 1), 0, n - 2, sid).reshape(n, top - 1)
    return u + (u >= np.arange(n)[:, None])


def host_counts(S_pcc, S_ssim, d, top):
    """(hits [2], expectation * n [2]) as the reference counts them on the given matrices."""
    n = S_pcc.shape[0]
    hits = IO.n_way_from(S_pcc, S_ssim, d).sum(0).tolist() if d is not None else [float("nan")] * 2
    return hits, (IO.n_way_expected_from(S_pcc, S_ssim, top) * n).tolist()


def check_counts(tag, out8, acc6, hits, exp, n, top):
    out8, acc6 = out8.cpu().double(), acc6.cpu()
    bound = (n + top) * 2.0 ** -52
    for k in range(2):
        assert acc6[k].item() == hits[k], (tag, k, acc6.tolist(), hits)
        rel = abs(acc6[2 + k].item() - exp[k]) / max(abs(exp[k]), 1e-300) if exp[k] else abs(acc6[2 + k].item())
        print(f"nway {tag} expectation[{k}]: err/bound {rel:.3g}/{bound:.3g}")
        assert rel <= bound, (tag, k, acc6.tolist(), exp)
        assert out8[k].item() == np.float32(hits[k] / n) and out8[2 + k].item() == np.float32(acc6[2 + k].item() / n)
    assert acc6[4:].tolist() == [n, 1]
    assert torch.equal(out8[:4], out8[4:])          # one batch: the running score is the batch's


# ---- matrices -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", [("synth", k) for k in SHAPES] + [("edge", "n19"), ("edge", "c1wide")])
def test_matrices_against_fp64(kind, name):
    b = batch(name, kind)
    S_pcc, S_ssim = (t.cpu().double() for t in engine(name, kind)[:2])
    for tag, got, want in (("PCC", S_pcc, b["pcc64"]), ("SSIM", S_ssim, b["ssim64"])):
        err = (got - want).abs().max().item()
        print(f"nway {kind} {name} {SHAPES[name]} {tag}: err/bound {err:.3g}/{BAR:.3g} = {err / BAR:.3f}")
        assert err <= BAR, (kind, name, tag, err)


def test_duplicate_truth_gives_an_exact_tie():
    S_pcc, S_ssim = engine("n33dup")[:2]
    for S in (S_pcc, S_ssim):
        assert torch.equal(S[:, DUP[1]], S[:, DUP[0]])
        assert not torch.equal(S[:, DUP[1]], S[:, DUP[0] + 1])


# ---- counting -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,top", [("n19", 1), ("n19", 2), ("n19", 5), ("n33dup", 5), ("n2", 5), ("n2", 1)])
def test_counting_is_exact_on_the_returned_matrices(name, top):
    b = batch(name)
    n = SHAPES[name][0]
    S_pcc, S_ssim, d, out8, acc6 = run(b, top=top)
    assert d.shape == (n, top - 1)
    if name == "n2" and top == 5:
        assert d.cpu().tolist() == [[1] * 4, [0] * 4]       # all four draws are the other image
    hits, exp = host_counts(S_pcc.cpu(), S_ssim.cpu(), d.cpu(), top)
    if top == 1:
        assert hits == [n, n] and exp == [n, n]
    check_counts(f"{name} top={top}", out8, acc6, hits, exp, n, top)


@pytest.mark.parametrize("name", ["n19", "c1wide", "k1025"])
def test_counts_hits_and_expectation_equal_those_of_the_fp64_matrices(name):
    """The float64 margins are hundreds of bars wide, so the engine's strict comparisons must all fall as in float64:
    counts, hits and expectation are those of the oracle's matrices, no row excluded."""
    b = batch(name)
    n, top = SHAPES[name][0], 5
    off = ~torch.eye(n, dtype=torch.bool)
    for S, m in ((b["pcc64"], MARGIN_PCC), (b["ssim64"], MARGIN_SSIM)):
        margin = (S - S.diagonal()[:, None]).abs()[off].min().item()
        print(f"nway {name} fp64 margin {margin:.3g} >= {m:.3g}")
        assert margin >= m
        short = int(((S < S.diagonal()[:, None]).sum(1) < n - 1).sum())
        assert 0 < short < n                                # the counts are not trivial
    S_pcc, S_ssim, d, out8, acc6 = engine(name)
    for got, want in ((S_pcc, b["pcc64"]), (S_ssim, b["ssim64"])):
        got = got.cpu()
        assert torch.equal((got < got.diagonal()[:, None]).sum(1), (want < want.diagonal()[:, None]).sum(1))
    hits, exp = host_counts(b["pcc64"], b["ssim64"], d.cpu(), top)
    check_counts(f"{name} vs fp64", out8, acc6, hits, exp, n, top)


# ---- draws --------------------------------------------------------------------------------------------------------------
def test_distractors_are_the_philox_stream_at_the_generators_offset():
    from fmri_hip.rng import SID_DISTRACT, blocks
    b = batch("n19")
    n, top = 19, 5
    g = _rng()
    d1 = run(b, rng=g)[2].cpu()
    assert d1.dtype == torch.int32 and np.array_equal(d1.numpy(), host_draws(n, top, sid=SID_DISTRACT))
    assert torch.equal(run(b, rng=g)[2].cpu(), d1)          # a call does not move the offset
    assert g.state() == (RNG_SEED, RNG_OFFSET)
    g.advance(blocks(n * (top - 1)))
    d2 = run(b, rng=g)[2].cpu()
    assert np.array_equal(d2.numpy(), host_draws(n, top, offset=RNG_OFFSET + 19, sid=SID_DISTRACT))
    assert not torch.equal(d1, d2)
    d3 = run(b, rng=_rng(), sid=9)[2].cpu()
    assert np.array_equal(d3.numpy(), host_draws(n, top, sid=9)) and not torch.equal(d3, d1)
    # a long row of draws: more than one thread's worth and a ragged last Philox block
    d4 = run(b, top=300, rng=_rng())[2].cpu()
    assert np.array_equal(d4.numpy(), host_draws(n, 300))


def test_no_rng_gives_nan_hits_and_a_valid_expectation():
    b = batch("n19")
    ref = engine("n19")
    S_pcc, S_ssim, d, out8, acc6 = run(b, rng=None)
    assert d is None and torch.equal(S_pcc, ref[0]) and torch.equal(S_ssim, ref[1])
    assert torch.isnan(out8[[0, 1, 4, 5]]).all() and torch.isnan(acc6[:2]).all()
    assert torch.equal(out8[[2, 3, 6, 7]], ref[3][[2, 3, 6, 7]]) and torch.equal(acc6[2:], ref[4][2:])


# ---- invariants ---------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))         # (no NaN in these outputs)


def test_outputs_do_not_depend_on_dead_lanes_pointer_offset_mode_or_call():
    from fmri_hip import ops
    b = batch("n19")
    ref = engine("n19")
    assert _same(run(b), ref)                                                       # two calls
    nan_p, nan_t = (EO.to_layout(b[k], float("nan")).to(DEV) for k in ("pred", "truth"))
    assert torch.isnan(nan_p[..., 3:]).all()
    assert _same(run(b, p16=nan_p, t16=nan_t), ref)                                 # NaN in lanes 3..7
    views = []
    for t in (nan_p, nan_t):
        big = torch.full((t.numel() + 64,), 7.0, dtype=torch.float16, device=DEV)
        v = big[8:8 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 32 == 16 and v.is_contiguous()
        views.append(v)
    assert _same(run(b, p16=views[0], t16=views[1]), ref)                           # 16-byte offset into a buffer
    was = ops.set_deterministic(True)
    try:
        on = run(b)
        ops.set_deterministic(False)
        off = run(b)
    finally:
        ops.set_deterministic(was)
    assert _same(on, ref) and _same(off, ref)


def test_a_pairs_value_does_not_depend_on_the_batch_it_sits_in():
    b = batch("n19")
    ref = engine("n19")
    S_pcc, S_ssim = run(b, p16=b["p16"][:5].contiguous(), t16=b["t16"][:5].contiguous())[:2]
    assert torch.equal(S_pcc, ref[0][:5, :5]) and torch.equal(S_ssim, ref[1][:5, :5])
    # ... nor on its place: the batch reversed gives the matrices reversed
    S_pcc, S_ssim = run(b, p16=b["p16"].flip(0).contiguous(), t16=b["t16"].flip(0).contiguous())[:2]
    assert torch.equal(S_pcc.flip(0, 1), ref[0]) and torch.equal(S_ssim.flip(0, 1), ref[1])


# ---- degenerate images --------------------------------------------------------------------------------------------------
def test_nan_and_constant_images():
    b = batch("n19")
    n, top = 19, 5
    p = b["pred"].clone()
    p[3, 1, 7, 5] = float("nan")            # one NaN pixel: the whole row of both matrices
    p[6] = 0.5                              # constant: zero variance
    S_pcc, S_ssim, d, out8, acc6 = run(b, p16=EO.to_layout(p).to(DEV))
    S_pcc, S_ssim, d = S_pcc.cpu(), S_ssim.cpu(), d.cpu()
    assert torch.isnan(S_pcc[3]).all() and torch.isnan(S_ssim[3]).all()
    assert torch.isnan(S_pcc[6]).all() and torch.isfinite(S_ssim[6]).all()
    rest = [i for i in range(n) if i not in (3, 6)]
    assert torch.isfinite(S_pcc[rest]).all() and torch.isfinite(S_ssim[rest]).all()
    ref = engine("n19")
    assert torch.equal(S_pcc[rest], ref[0].cpu()[rest]) and torch.equal(S_ssim[rest], ref[1].cpu()[rest])
    hit = IO.n_way_from(S_pcc, S_ssim, d)
    assert not hit[3].any() and not hit[6, 0]           # NaN compares false: never a hit, count 0, term 0
    hits, exp = host_counts(S_pcc, S_ssim, d, top)
    check_counts("degenerate", out8, acc6, hits, exp, n, top)
    # top = 1: every image is a hit and the expectation is n, NaN rows included
    out8, acc6 = run(b, top=1, p16=EO.to_layout(p).to(DEV))[3:]
    assert acc6.cpu().tolist() == [n, n, n, n, n, 1]


# ---- accumulator --------------------------------------------------------------------------------------------------------
def test_accumulator_over_three_batches():
    a, c = batch("n19"), batch("n2")
    top = 5
    acc = torch.full((6,), 123.0, dtype=torch.float64, device=DEV)       # acc_mode 0 clears whatever is there
    outs = []
    for k, b in enumerate((a, a, c)):
        S_pcc, S_ssim, d, out8, acc6 = run(b, rng=_rng(RNG_OFFSET + 100 * k), acc=acc, acc_mode=0 if k == 0 else 1)
        assert acc6 is acc
        outs.append((out8.cpu(),) + host_counts(S_pcc.cpu(), S_ssim.cpu(), d.cpu(), top))
    acc = acc.cpu()
    assert acc[4:].tolist() == [40, 3]
    want_hits = sum(np.array(o[1]) for o in outs)
    want_exp = sum(np.array(o[2]) for o in outs)
    assert acc[:2].tolist() == want_hits.tolist()
    for m in range(2):
        rel = abs(acc[2 + m].item() - want_exp[m]) / want_exp[m]
        print(f"nway accumulator expectation[{m}]: err/bound {rel:.3g}/{(40 + top + 3) * 2.0 ** -52:.3g}")
        assert rel <= (40 + top + 3) * 2.0 ** -52
    last = outs[-1][0].double()
    for m in range(4):
        assert last[4 + m].item() == np.float32(acc[m].item() / 40.0)
    assert last[0].item() == np.float32(outs[-1][1][0] / 2)
