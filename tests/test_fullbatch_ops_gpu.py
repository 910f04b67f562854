"""The dense, BatchNorm and loss / optimizer kernels at the row counts of the B = 256 step, each against a plain torch
float64 restatement of the same operation on the same fp16-rounded inputs.

tests/test_kernels_gpu.py pins these operators at a handful of rows (M <= 12 for the dense layers and the one-launch
BatchNorm, B = 5 for the losses); behind that only the fused-step tests stand, and they compare losses.  Here:

  A. DenseLayer.forward / dgrad / wgrad / bias_grad at M = 256 / 512 / 768 (and 1536, where run_wgrad first splits a
     dense reduction), a row sweep over the 128-row tile edge, both split-K routes, both reduction modes;
  B. ops.BatchNorm on the one-launch column path and on the streaming path at 131 072 ... 2 097 152 rows, the switch
     between the two, and channels that are off-centre, all zero, constant or far off-centre;
  C. the loss / optimizer entry points the steps call (``*_parts``, ``*_dev``, ``*_f64``, fmri_pixel_sq, ...), B = 256.

The references never call the library under test and read nothing outside this file.  Every check prints one line
``[fullbatch] <case> | <quantity> | err/bound = r``; profiles/fullbatch_ops_parity.md records those of one GPU run.
"""
import math
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24          # unit roundoff of fp32


def _h(t):
    return t.half().float()


class _G:
    """Minimal FlatGroup stand-in for single-layer tests (as in tests/test_kernels_gpu.py)."""

    def __init__(self, tensors):
        self.views = {k: v.to(DEV).contiguous() for k, v in tensors.items()}
        self.grads = {k: torch.zeros_like(v) for k, v in self.views.items()}
        self.version = 0
        self.device = torch.device(DEV)


def _ratio(got, ref, tol):
    """max err / bound with the bound of tests/test_kernels_gpu.py::_close (tol * RMS of the reference + tol * |ref|),
    evaluated in float64 on the device the result lives on."""
    got = got.detach().double()
    ref = ref.detach().double().to(got.device)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "non-finite result"
    rms = ref.pow(2).mean().sqrt().item() + 1e-12
    return float(((got - ref).abs() / (tol * rms + tol * ref.abs())).max())


def _say(case, what, r, asserted=True):
    print(f"[fullbatch] {case} | {what} | err/bound = {r:.4f}" + ("" if asserted else " (report only)"), flush=True)
    if asserted:
        assert r <= 1.0, f"{case}: {what}: err / bound = {r:.4f}"
    return r


def _check(case, what, got, ref, tol, asserted=True):
    return _say(case, what, _ratio(got, ref, tol), asserted)


def _bounded(case, what, err, bound, asserted=True):
    """max err / bound for an explicit per-element bound (0 / 0 counts as 0, err > 0 on a zero bound as a miss)."""
    err, bound = err.double(), bound.double().to(err.device)
    assert bool(torch.isfinite(err).all()), f"{case}: {what}: non-finite"
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return _say(case, what, float(r.max()), asserted)


class _Spy:
    """Records (entry point, arguments) of every library call made inside the ``with`` block."""

    def __enter__(self):
        from fmri_hip import lib
        self.lib, self.orig, self.calls = lib, lib.call, []

        def call(name, *args):
            self.calls.append((name, args))
            return self.orig(name, *args)
        lib.call = call
        return self

    def __exit__(self, *exc):
        self.lib.call = self.orig

    def names(self):
        return [n for n, _ in self.calls]

    def args_of(self, name):
        return [a for n, a in self.calls if n == name]


def _join():
    from fmri_hip.ops import join_side
    join_side()


# =====================================================================================================================
# A. dense layers
# =====================================================================================================================
RELU, NONE = 1, 0
SWEEP = (1, 63, 64, 127, 128, 129, 200, 257)

# name, K, N, in_perm, out_perm, bias, activation, rows M, then the route this case takes, stated from
# ops._choose_splits (forward, data gradient: 1 = one pass with the bias / activation / fp16 store in the contraction's
# epilogue, > 1 = fp32 slabs + fmri_reduce_slabs) and from the generic branch of the library's weight-gradient plan (ops.wgrad_plan:
# splits > 1 needs tiles < 512 and ceil(M / 64) >= 16 K steps), and the K steps of the weight gradient.
DENSE_TABLE = [
    # name                      K      N      in_perm    out_perm   bias   act   M     fwd dgrad wgrad ksteps
    ("encoder.fc.0",            16384, 1024,  (256, 64), None,      True,  NONE, 256,  16, 1,  1,  4),
    ("discriminator.fc.0",      16384, 512,   (256, 64), None,      True,  NONE, 768,  11, 1,  1,  12),
    ("decoder.fc.0",            128,   16384, None,      (256, 64), False, NONE, 512,  1,  64, 1,  8),
    ("fused heads",             1024,  256,   None,      None,      True,  NONE, 256,  4,  1,  1,  4),
    ("discriminator.fc.3",      512,   1,     None,      None,      True,  NONE, 768,  2,  1,  1,  12),
    ("cognitive.fc1",           4096,  1024,  None,      None,      True,  NONE, 256,  16, 4,  1,  4),
    ("cognitive.fc1",           4096,  1024,  None,      None,      True,  NONE, 128,  16, 4,  1,  2),
    ("cognitive.fc1 (3620)",    3620,  1024,  None,      None,      True,  NONE, 256,  12, 4,  1,  4),
    ("cognitive.fc1 (3620)",    3620,  1024,  None,      None,      True,  NONE, 128,  12, 4,  1,  2),
    ("latent-disc 128->512",    128,   512,   None,      None,      True,  RELU, 77,   1,  2,  1,  2),
    ("latent-disc 128->512",    128,   512,   None,      None,      True,  RELU, 512,  1,  2,  1,  8),
    ("latent-disc 512->512",    512,   512,   None,      None,      True,  RELU, 77,   2,  2,  1,  2),
    ("latent-disc 512->512",    512,   512,   None,      None,      True,  RELU, 512,  2,  2,  1,  8),
    # the smallest real row count at which run_wgrad splits the reduction of a dense layer (per-GPU batch 512):
    # fc.3 has 4 output tiles and 24 K steps -> 3 splits; fc.0 has exactly 512 tiles, which is not < 512 -> one pass
    ("discriminator.fc.0",      16384, 512,   (256, 64), None,      True,  NONE, 1536, 6,  1,  1,  24),
    ("discriminator.fc.3",      512,   1,     None,      None,      True,  NONE, 1536, 2,  1,  3,  24),
    # the dense layers of the 100-px step (ArchConfig.px100: 13 x 13 and 7 x 7 feature planes, HW = 169 and 49 in the
    # (C, HW) <-> (HW, C) permutation) at the reference's shipped batch of 64, M = 64 / 128 / 192: 31 and 62 splits over
    # 676 K steps (no even division), 49 splits over 196 K steps
    ("encoder.fc.0 @100",       43264, 1024,  (256, 169), None,     True,  NONE, 64,   31, 1,  1,  1),
    ("decoder.fc.0 @100",       512,   43264, None,     (256, 169), False, NONE, 128,  1,  62, 1,  2),
    ("discriminator.fc.0 @100", 12544, 256,   (256, 49), None,      True,  NONE, 192,  49, 1,  1,  3),
    ("fused heads @100",        1024,  1024,  None,      None,      True,  NONE, 64,   4,  4,  1,  1),
    ("discriminator.fc.3 @100", 256,   1,     None,      None,      True,  NONE, 192,  1,  1,  1,  3),
    # ... and at the remainder batch of 5 (M = 5 / 10 / 15): the same splits over one partial row tile
    ("encoder.fc.0 @100",       43264, 1024,  (256, 169), None,     True,  NONE, 5,    31, 1,  1,  1),
    ("decoder.fc.0 @100",       512,   43264, None,     (256, 169), False, NONE, 10,   1,  62, 1,  1),
    ("discriminator.fc.0 @100", 12544, 256,   (256, 49), None,      True,  NONE, 15,   49, 1,  1,  1),
]


def _k_steps(case):
    """(forward, data-gradient) K steps of 64 of a DENSE_TABLE row: the reduction lengths _dense_route hands to
    ops._choose_splits."""
    from fmri_hip.ops import ceil_to, pad8
    return ceil_to(pad8(case[1]), 64) // 64, ceil_to(pad8(case[2]), 64) // 64
# row sweep over the 128-row tile edge on one split-K layer (fused heads) and one single-pass layer (128 -> 512)
DENSE_TABLE += [("fused heads", 1024, 256, None, None, True, NONE, m, 4, 1, 1, (m + 63) // 64) for m in SWEEP]
DENSE_TABLE += [("latent-disc 128->512", 128, 512, None, None, True, RELU, m, 1, 2, 1, (m + 63) // 64) for m in SWEEP]


def _dense_route(M, K, N):
    """(forward splits, data-gradient splits, weight-gradient splits, weight-gradient K steps) from ops._choose_splits
    with DenseLayer._gemm's block / K-step counts, and from ops.wgrad_plan for the geometry DenseLayer._wgrad hands to
    run_wgrad (a 1 x 1 plane per row, one tap)."""
    from fmri_hip.ops import _choose_splits, ceil_to, pad8, tile_for, wgrad_plan
    kp, np_ = pad8(K), pad8(N)
    t_out, t_in = min(64, tile_for(N)), min(64, tile_for(K))
    rows = (M + 127) // 128
    fwd = _choose_splits(rows * (ceil_to(N, t_out) // t_out), ceil_to(kp, 64) // 64)
    dgr = _choose_splits(rows * (ceil_to(K, t_in) // t_in), ceil_to(np_, 64) // 64)
    wgr = wgrad_plan(M, 1, 1, np_, 1, 1, kp, 1, 1, 0).splits
    return fwd, dgr, wgr, (M + 63) // 64


def test_dense_table_states_its_routes_and_covers_both():
    """The routes written into DENSE_TABLE are what ops._choose_splits / ops.wgrad_plan give today, and the
    table as a whole holds every route: forward and data gradient in one pass and through fmri_reduce_slabs (the
    latter with bias + activation over two or more 128-row tiles), weight gradient in one pass over several K steps
    and split.  A routing change that moves a case fails here (and in the case itself, which observes the launch)."""
    for name, K, N, _, _, _, _, M, fwd, dgr, wgr, steps in DENSE_TABLE:
        assert _dense_route(M, K, N) == (fwd, dgr, wgr, steps), (name, M, _dense_route(M, K, N))
    rows = [(f"{c[0]} M={c[7]}", c[8], c[9], c[10]) for c in DENSE_TABLE]
    for r in rows:
        print("[fullbatch] route %-32s forward splits %3d  dgrad splits %3d  wgrad splits %3d" % r)
    for col, what in ((8, "forward"), (9, "dgrad"), (10, "wgrad")):
        vals = {c[col] for c in DENSE_TABLE}
        assert 1 in vals and max(vals) > 1, (what, vals)
    assert any(c[8] == 1 and c[5] and c[6] == RELU for c in DENSE_TABLE), "fused bias + activation, fp16 store"
    assert any(c[8] > 1 and c[5] and c[6] == RELU and c[7] > 128 for c in DENSE_TABLE), \
        "fmri_reduce_slabs with bias + activation over two or more row tiles"
    assert any(c[10] == 1 and c[11] >= 4 for c in DENSE_TABLE), "one-pass weight gradient over several K steps"
    assert any(c[10] > 1 for c in DENSE_TABLE), "split weight gradient"
    # a split count that does not divide the K steps (the splits then cover unequal K ranges), in either direction
    assert any(c[8] > 1 and _k_steps(c)[0] % c[8] for c in DENSE_TABLE), "forward splits that do not divide the K steps"
    assert any(c[9] > 1 and _k_steps(c)[1] % c[9] for c in DENSE_TABLE), "dgrad splits that do not divide the K steps"
    assert (676 % 31, 676 % 62) == (25, 56) and any(c[8] == 31 for c in DENSE_TABLE) and any(c[9] == 62 for c in DENSE_TABLE)
    # the feature permutation at plane sizes other than 64
    assert {p[1] for c in DENSE_TABLE for p in (c[3], c[4]) if p} >= {64, 169, 49}


def _perms(K, N, in_perm, out_perm):
    def to_engine_in(t):          # reference (C,HW) feature order -> engine (HW,C)
        if in_perm:
            C, HW = in_perm
            return t.reshape(-1, C, HW).transpose(1, 2).reshape(-1, K)
        return t

    def from_engine_in(t):
        if in_perm:
            C, HW = in_perm
            return t.reshape(-1, HW, C).transpose(1, 2).reshape(-1, K)
        return t

    def to_engine_out(t):
        if out_perm:
            C, HW = out_perm
            return t.reshape(-1, C, HW).transpose(1, 2).reshape(-1, N)
        return t

    def from_engine_out(t):
        if out_perm:
            C, HW = out_perm
            return t.reshape(-1, HW, C).transpose(1, 2).reshape(-1, N)
        return t
    return to_engine_in, from_engine_in, to_engine_out, from_engine_out


@pytest.mark.parametrize("name,K,N,in_perm,out_perm,bias,act,M,fwd,dgr,wgr,steps", DENSE_TABLE,
                         ids=[f"{c[0]}-M{c[7]}".replace(" ", "_").replace("->", "to") for c in DENSE_TABLE])
def test_dense_at_engine_rows(name, K, N, in_perm, out_perm, bias, act, M, fwd, dgr, wgr, steps):
    """DenseLayer against float64 F.linear (+ relu) and its autograd, on the CPU.  The fp16 outputs' padding columns
    [N, pad8(N)) must be zero.  DenseLayer allocates its own outputs, so the rows-behind-M half of the padding contract
    is checked where the caller owns the buffer: test_dense_caller_owned_buffers_keep_the_rows_behind_m."""
    from fmri_hip import ops
    from fmri_hip.ops import DenseLayer, pad8, rows_to_f16
    case = f"A {name} {K}->{N} M={M}"
    t_start = time.time()
    torch.manual_seed(M * 7 + K + N)
    w = _h(torch.randn(N, K) / np.sqrt(K))
    b = torch.randn(N) * 0.1 if bias else None
    x = _h(torch.randn(M, K))
    dy = _h(torch.randn(M, N))
    g = _G({"w": w, "b": b} if bias else {"w": w})
    layer = DenseLayer(g, "w", "b" if bias else None, K, N, in_perm=in_perm, out_perm=out_perm)
    to_in, from_in, to_out, from_out = _perms(K, N, in_perm, out_perm)

    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    lin = F.linear(xr, wr, None)
    ref = lin.detach() + (b.double() if bias else 0.0)
    if act == RELU:
        ref = torch.relu(ref)
    lin.backward(dy.double())

    x16 = rows_to_f16(to_in(x).contiguous().to(DEV))
    dy16 = rows_to_f16(to_out(dy).contiguous().to(DEV))
    o16, o32 = layer.forward(x16, act, want16=True, want32=True)
    with _Spy() as spy:
        o16b, none32 = layer.forward(x16, act)                   # the call the networks make: fp16 only
    # argument 19 of fmri_igemm_ep is the split count the launch was given
    assert spy.args_of("fmri_igemm_ep")[0][19] == fwd and none32 is None, (case, spy.args_of("fmri_igemm_ep")[0][19], fwd)
    assert ("fmri_reduce_slabs" in spy.names()) == (fwd > 1), spy.names()
    np_ = pad8(N)
    _check(case, "forward fp32", from_out(o32.cpu()), ref, 1e-3)
    _check(case, "forward fp16 (with fp32)", from_out(o16[:, :N].float().cpu()), ref, 2e-3)
    _check(case, f"forward fp16 (splits {fwd})", from_out(o16b[:, :N].float().cpu()), ref, 2e-3)
    assert o16b.shape == (M, np_) and bool((o16b[:, N:] == 0).all()) and bool((o16[:, N:] == 0).all()), "padding columns"

    with _Spy() as spy:
        dx16, _ = layer.dgrad(dy16)
    assert spy.args_of("fmri_igemm_ep")[0][19] == dgr, (case, spy.args_of("fmri_igemm_ep")[0][19], dgr)
    assert ("fmri_reduce_slabs" in spy.names()) == (dgr > 1), spy.names()
    _, dx32 = layer.dgrad(dy16, want32=True)
    _check(case, f"dgrad fp16 (splits {dgr})", from_in(dx16[:, :K].float().cpu()), xr.grad, 2e-3)
    _check(case, "dgrad fp32", from_in(dx32.cpu()), xr.grad, 1e-3)
    assert dx16.shape == (M, pad8(K)) and bool((dx16[:, K:] == 0).all()), "padding columns of dx"

    was = ops.deterministic()
    try:
        for det in (False, True):
            ops.set_deterministic(det)
            runs = []
            for rep in range(2 if det else 1):
                for v in g.grads.values():
                    v.zero_()
                with _Spy() as spy:
                    layer.wgrad(x16, dy16, 2.0)
                    _join()
                    if bias:
                        layer.bias_grad(dy16, 2.0)
                torch.cuda.synchronize()
                a = spy.args_of("fmri_wgrad_if")[0]
                assert a[-2] == wgr and a[-1] == ((4 if det else 1) if wgr > 1 else 0), (case, a[-2:], wgr)
                runs.append({k: v.clone() for k, v in g.grads.items()})
            mode = "deterministic" if det else "default"
            _check(case, f"wgrad ({mode}, splits {wgr}, {steps} K steps)", runs[0]["w"].cpu() * 2.0, wr.grad, 3e-3)
            if bias:
                _check(case, f"bias grad ({mode})", runs[0]["b"].cpu() * 2.0, dy.double().sum(0), 3e-3)
            if det:
                assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0]), "deterministic mode: two runs differ"
    finally:
        ops.set_deterministic(was)
    torch.cuda.synchronize()
    print(f"[fullbatch] {case} | wall {time.time() - t_start:.1f} s", flush=True)


@pytest.mark.parametrize("K,N,M,act", [(128, 512, 77, RELU), (512, 1, 768, NONE), (1024, 256, 129, NONE)])
def test_dense_caller_owned_buffers_keep_the_rows_behind_m(K, N, M, act):
    """The launches behind DenseLayer._gemm with buffers of M + 3 rows filled with a sentinel: the one-pass contraction
    (fp16 store), the split contraction's slabs and fmri_reduce_slabs' two outputs write rows [0, M) only."""
    from fmri_hip import lib, ops
    from fmri_hip.ops import DenseLayer, pad8, rows_to_f16
    case = f"A rows behind M, {K}->{N} M={M}"
    torch.manual_seed(K + N + M)
    w = _h(torch.randn(N, K) / np.sqrt(K))
    b = torch.randn(N) * 0.1
    x = _h(torch.randn(M, K))
    g = _G({"w": w, "b": b})
    layer = DenseLayer(g, "w", "b", K, N)
    ref = F.linear(x.double(), w.double(), b.double())
    ref = torch.relu(ref) if act == RELU else ref
    x16 = rows_to_f16(x.to(DEV))
    kp, np_ = pad8(K), pad8(N)
    out = torch.full((M + 3, np_), 7.0, dtype=torch.float16, device=DEV)
    ops.run_igemm(x16, layer.pw_f, out, layer.b, M, 1, 1, kp, 1, 1, np_, N, 1, 1, 0, ops.MODE_CONV, act, False, 1, 0,
                  layer.t_out)
    torch.cuda.synchronize()
    assert bool((out[M:] == 7.0).all()), "one-pass store wrote behind row M"
    assert bool((out[:M, N:] == 0).all()), "padding columns"
    _check(case, "one pass", out[:M, :N].float().cpu(), ref, 2e-3)
    splits = 2
    stride = (M + 3) * np_
    slabs = torch.full((splits, M + 3, np_), 7.0, dtype=torch.float32, device=DEV)
    ops.run_igemm(x16, layer.pw_f, slabs, None, M, 1, 1, kp, 1, 1, np_, N, 1, 1, 0, ops.MODE_CONV, NONE, True, splits,
                  stride, layer.t_out)
    o16 = torch.full((M + 3, np_), 7.0, dtype=torch.float16, device=DEV)
    o32 = torch.full((M + 3, N), 7.0, dtype=torch.float32, device=DEV)
    lib.call("fmri_reduce_slabs", slabs.data_ptr(), splits, stride, M, N, np_, layer.b.data_ptr(), act, o32.data_ptr(), N,
             o16.data_ptr(), np_)
    torch.cuda.synchronize()
    assert bool((slabs[:, M:] == 7.0).all()), "slab store wrote behind row M"
    assert bool((o16[M:] == 7.0).all()) and bool((o32[M:] == 7.0).all()), "fmri_reduce_slabs wrote behind row M"
    assert bool((o16[:M, N:] == 0).all()), "padding columns"
    _check(case, "two slabs fp16", o16[:M, :N].float().cpu(), ref, 2e-3)
    _check(case, "two slabs fp32", o32[:M].cpu(), ref, 1e-3)


# =====================================================================================================================
# B. BatchNorm
# =====================================================================================================================
EPS = 1e-5


def _bn_chain(M, C, cols):
    """Number of sequential fp32 additions on the longest path of the BatchNorm sums, from the geometry documented at
    the top of csrc/norm.hip: rows per thread + the in-block fold over the row lanes + the number of partial rows.
    Column path (bn_cols_*): 64 row lanes per block, one block per channel group, no partial rows.  Streaming path
    (row_geometry): CX = min(256, pow2 >= C / 8) chunk columns, RY = 256 / CX row lanes, gy = min(ceil(M / 16 RY),
    768 / gx) blocks along the rows, each writing one partial row."""
    if cols:
        return (M + 63) // 64 + 64, 0
    nch = C // 8
    lg = 0
    while (1 << lg) < nch and lg < 8:
        lg += 1
    CX, RY = 1 << lg, 256 >> lg
    gx = (nch + CX - 1) // CX
    gy = max(1, min((M + RY * 16 - 1) // (RY * 16), max(768 // gx, 1)))
    return (M + gy * RY - 1) // (gy * RY) + RY + gy, gy


# hard channels (section B of the module docstring): channel -> (kind, mean, std)
HARD = {1: ("off-centre 2", 2.0, 1.0), 2: ("off-centre 4", 2.0, 0.5), 3: ("off-centre 8", 2.0, 0.25),
        4: ("all zero", 0.0, 0.0), 5: ("constant", 3.0, 0.0), 6: ("mean/std 64", 8.0, 0.125)}
REPORT_ONLY = (5, 6)     # the one-pass variance is not expected to be accurate there: finite, var >= 0, printed


def _bn_input(M, C, seed, hard):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    x = torch.randn(M, C, device=DEV, generator=gen) * 1.5 + 0.3
    if hard:
        for c, (_, mu, sd) in HARD.items():
            x[:, c] = torch.randn(M, device=DEV, generator=gen) * sd + mu
    return x.half()


def _bn_cotangents(x16, seed):
    """Two cotangents dy = s randn + a_c + b_c z, z = the input standardised per channel, with |a_c|, |b_c| in [0.5, 1.5]
    of either sign.  The two mean terms of the data gradient, sum(g) / count and xhat sum(g xhat) / count, are then of
    the order of dx itself, so the 3e-3 bound on dx checks how the apply kernels use the reduced sums and the count at
    every row count (with zero-mean cotangents those terms are ~ 0.7 / sqrt(M) of dx and a wrong count, a factor on
    them or the sums of a neighbouring channel would hide inside the bound)."""
    M, C = x16.shape
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    xf = x16.float()
    z = (xf - xf.mean(0)) / xf.std(0).clamp_min(1e-3)
    out = []
    for s_ in (1.0, 0.5):
        ab = (torch.rand(2, C, device=DEV, generator=gen) + 0.5) * \
            (torch.randint(0, 2, (2, C), device=DEV, generator=gen) * 2 - 1)
        out.append((torch.randn(M, C, device=DEV, generator=gen) * s_ + ab[0] + ab[1] * z).half())
    return out


def _dx_ratio(dx, ref, other, flip, edge, tol):
    """err / bound of a BatchNorm data gradient.  ReLU's derivative jumps at 0, and the kernel takes the side its own
    (verified) fp32 statistics put an element on: where the float64 reference lands on the other side (``flip``) the
    reference is the other one-sided derivative (``other`` = reference -+ gamma rstd dy), and where the kernel's own
    pre-activation is within fp32 rounding of 0 (``edge``) either side is accepted.  No element is left out."""
    rms = ref.pow(2).mean().sqrt().item() + 1e-12
    e_ref = (dx - ref).abs() / (tol * rms + tol * ref.abs())
    e_oth = (dx - other).abs() / (tol * rms + tol * other.abs())
    r = torch.where(edge, torch.minimum(e_ref, e_oth), torch.where(flip, e_oth, e_ref))
    assert bool(torch.isfinite(dx).all())
    return float(r.max())


def _run_bn_case(M, C, perm=None, hard=False, updates=1, x16=None, seed=None):
    """One BatchNorm layer end to end against float64 torch ON THE DEVICE (ATen's batch_norm / relu / autograd, no
    kernel of this project): forward (+ running statistics), forward_eval, backward, backward2 with either parameter
    stream.  Host memory: a few hundred bytes per channel -- inputs are drawn on the device and compared there; the
    largest case (786 432 x 128, 100 M elements) peaks at about 11 GiB of DEVICE memory, most of it float64
    temporaries (each case prints its peak).  The cotangents carry a per-channel offset and a component along xhat
    (``_bn_cotangents``), so that the mean terms of dx are of the order of dx."""
    from fmri_hip import lib, ops
    from fmri_hip.ops import BatchNorm
    cols = M <= ops._BN_COLS_ROWS
    case = f"B ({M}, {C})" + (" perm" if perm else "") + (" hard" if hard else "") + (" cols" if cols else " stream")
    torch.cuda.reset_peak_memory_stats()
    t_start = time.time()
    if x16 is None:
        x16 = _bn_input(M, C, seed if seed is not None else M + C, hard)
    dya, dyb = _bn_cotangents(x16, 3 * M + C)
    torch.manual_seed(C)
    gamma = 1 + 0.2 * torch.randn(C)
    beta = 0.1 * torch.randn(C)
    if hard:
        beta[4] = 0.25                       # the all-zero channel: y = relu(beta) > 0, so dx is exercised too
    g = _G({"bn.weight": gamma, "bn.bias": beta})
    g.bufs = {"bn.running_mean": torch.zeros(C, device=DEV), "bn.running_var": torch.ones(C, device=DEV),
              "bn.num_batches_tracked": torch.zeros((), dtype=torch.int64, device=DEV)}
    bn = BatchNorm(g, "bn.", C, perm=perm)

    def eng(v):                              # per-feature vector, reference (C0, HW) order -> engine (HW, C0) order
        if perm:
            return v.reshape(perm[0], perm[1]).t().reshape(-1)
        return v

    # ---- the layer
    with _Spy() as spy:
        y16, sv = bn.forward(x16, relu=True, updates=updates)
        rm_k, rv_k = eng(g.bufs["bn.running_mean"]).double(), eng(g.bufs["bn.running_var"]).double()
        ye16 = bn.forward_eval(x16, relu=True)
        dx16, _ = bn.backward(x16, dya, sv, relu=True, param_scale=8.0)
        ga_k, gb_k = eng(g.grads["bn.weight"]).double() * 8.0, eng(g.grads["bn.bias"]).double() * 8.0
        dy2 = torch.cat([dya, dyb], 0)
        two = []
        for ps in (0, 1):
            for v in g.grads.values():
                v.zero_()
            dx2, sums2 = bn.backward2(x16, dy2, sv, relu=True, param_scale=4.0, param_stream=ps)
            assert sums2.shape == (4, C)
            two.append((dx2, eng(g.grads["bn.weight"]).double() * 4.0, eng(g.grads["bn.bias"]).double() * 4.0))
    torch.cuda.synchronize()
    names = set(spy.names())
    col_k = {"fmri_bn_cols_fwd_s", "fmri_bn_cols_bwd"}
    str_k = {"fmri_bn_stats_finalize", "fmri_bn_bwd_reduce", "fmri_bn_bwd_apply", "fmri_bn_bwd_reduce2",
             "fmri_bn_bwd_apply2"}
    assert (col_k <= names and not (str_k & names)) if cols else (str_k <= names and not (col_k & names)), names
    assert int(g.bufs["bn.num_batches_tracked"]) == updates

    # ---- float64 reference (engine feature order throughout)
    ge, be = eng(gamma.double().to(DEV)), eng(beta.double().to(DEV))
    x64 = x16.double().requires_grad_(True)
    gr, br = ge.clone().requires_grad_(True), be.clone().requires_grad_(True)
    rm, rv = torch.zeros(C, dtype=torch.float64, device=DEV), torch.ones(C, dtype=torch.float64, device=DEV)
    yr = F.relu(F.batch_norm(x64, rm, rv, gr, br, True, 0.9, EPS))
    with torch.no_grad():
        for _ in range(updates - 1):
            F.batch_norm(x64, rm, rv, ge, be, True, 0.9, EPS)
        xd = x64.detach()
        mean64, ex2, eabs = xd.mean(0), (xd * xd).mean(0), xd.abs().mean(0)
        var64 = ((xd - mean64) ** 2).mean(0)
        rstd64 = (var64 + EPS).rsqrt()
        yev = F.relu(F.batch_norm(xd, rm, rv, ge, be, False, 0.9, EPS))
    refs = [torch.autograd.grad(yr, (x64, gr, br), dy.double(), retain_graph=True) for dy in (dya, dyb)]

    # ---- statistics, bounded by the worst-case rounding of the summation (not by what the kernel gives)
    d, gy = _bn_chain(M, C, cols)
    assert cols or gy == lib.load().fmri_bn_ws_floats(M, C) // (2 * C), "the geometry restated in _bn_chain is stale"
    ok = torch.ones(C, dtype=torch.bool, device=DEV)
    if hard:
        ok[list(REPORT_ONLY)] = False
        # the inputs keep rstd within the project's 2e-3 under that bound: 0.5 (d + 4) u E[x^2] / (var + eps) <= 2e-3
        worst = float((0.5 * (d + 4) * U * ex2 / (var64 + EPS))[ok].max())
        print(f"[fullbatch] {case} | d = {d}, worst-case relative rstd error of the asserted channels = {worst:.2e}")
        assert worst <= 2e-3, (d, worst)
    sx, sxx = sv.sums[0].double(), sv.sums[1].double()
    mean_k, rstd_k = sv.mean.double(), sv.rstd.double()
    var_k = sxx / M - (sx / M) ** 2
    w_run = 1.0 - 0.1 ** updates
    unb = M / (M - 1.0)
    stat = [("mean", (mean_k - mean64).abs(), d * U * eabs + U * mean64.abs()),
            ("var from the sums", (var_k - var64).abs(), d * U * ex2),
            ("rstd", (rstd_k / rstd64 - 1).abs(), torch.full_like(ex2, 2e-3)),
            # + 16 u of the value: per momentum update three roundings and the fp32 constant 1 - 0.9f (4 u off 0.1), the
            # unbiasing factor, the division by the count
            ("running_mean", (rm_k - rm).abs(), w_run * (d * U * eabs + U * mean64.abs()) + 16 * U * rm.abs()),
            ("running_var", (rv_k - rv).abs(), w_run * unb * (d + 4) * U * ex2 + 16 * U * rv.abs())]
    for what, err, bound in stat:
        _bounded(case, what, err[ok], bound[ok])
    assert bool(torch.isfinite(rstd_k).all()) and bool((rv_k >= 0).all()) and bool(torch.isfinite(rm_k).all())
    if hard:
        for c in REPORT_ONLY:
            for what, err, bound in stat:
                _bounded(case, f"{what}, channel '{HARD[c][0]}'", err[c:c + 1], bound[c:c + 1],
                         asserted=what.startswith("running"))
        z = 4                                # the all-zero channel
        assert abs(float(rstd_k[z]) * math.sqrt(EPS) - 1) < 1e-6, float(rstd_k[z])
        assert float(mean_k[z]) == 0.0 and float(var_k[z]) == 0.0
        assert bool((y16[:, z] == torch.relu(be[z]).half()).all()), "all-zero channel: y != relu(beta)"

    # ---- outputs
    def split(what, got, ref, tol):
        _check(case, what, got[..., ok], ref[..., ok], tol)
        if hard:
            for c in REPORT_ONLY:
                _check(case, f"{what}, channel '{HARD[c][0]}'", got[..., c:c + 1], ref[..., c:c + 1], tol, asserted=False)

    split("y", y16, yr.detach(), 2e-3)
    split("y (eval)", ye16, yev, 2e-3)
    with torch.no_grad():
        pre64 = (xd - mean64) * rstd64 * ge + be
        xh_k = (xd - mean_k) * rstd_k
        pre_k = xh_k * ge + be
        flip = (pre64 > 0) != (pre_k > 0)
        edge = pre_k.abs() <= 8 * U * ((xh_k * ge).abs() + be.abs())
        print(f"[fullbatch] {case} | ReLU side: {int(flip.sum())} elements flipped by the fp32 statistics, "
              f"{int(edge.sum())} within fp32 rounding of 0, of {flip.numel()}")
        plain = not bool((flip | edge).any())          # the usual case: every element on the reference's side of 0
        sign = None if plain else torch.where(pre64 > 0, -1.0, 1.0).double()
        del pre64, xh_k, pre_k

        def dx_check(what, dx, ref, dy):
            if plain:
                return split(what, dx, ref, 3e-3)
            other = ref + sign * ge * rstd64 * dy.double()
            r = _dx_ratio(dx.double()[:, ok], ref[:, ok], other[:, ok], flip[:, ok], edge[:, ok], 3e-3)
            _say(case, what, r)
            if hard:
                for c in REPORT_ONLY:
                    s = slice(c, c + 1)
                    _say(case, f"{what}, channel '{HARD[c][0]}'",
                         _dx_ratio(dx.double()[:, s], ref[:, s], other[:, s], flip[:, s], edge[:, s], 3e-3), False)

        dx_check("dx", dx16, refs[0][0], dya)
        split("dgamma", ga_k, refs[0][1], 3e-3)
        split("dbeta", gb_k, refs[0][2], 3e-3)
        for ps in (0, 1):
            dx2, ga2, gb2 = two[ps]
            dx_check(f"backward2 dx stream A (param_stream {ps})", dx2[:M], refs[0][0], dya)
            dx_check(f"backward2 dx stream B (param_stream {ps})", dx2[M:], refs[1][0], dyb)
            split(f"backward2 dgamma (param_stream {ps})", ga2, refs[ps][1], 3e-3)
            split(f"backward2 dbeta (param_stream {ps})", gb2, refs[ps][2], 3e-3)
        if hard:
            z = 4
            dz, rz = dx16[:, z].double(), refs[0][0][:, z]
            lim = 3e-3 * rz.pow(2).mean().sqrt() + 3e-3 * rz.abs()
            assert bool((dz == 0).all()) or bool(((dz - rz).abs() <= lim).all()), "all-zero channel: dx"
    torch.cuda.synchronize()
    print(f"[fullbatch] {case} | wall {time.time() - t_start:.1f} s, peak device memory "
          f"{torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")


BN_COLS = [(256, 1024, None), (512, 16384, (256, 64)), (768, 512, None), (2048, 64, None),
           # the 100-px step at batch 64: encoder.fc.0, decoder.fc.0 (13 x 13 planes: HW = 169), discriminator.fc.0
           (64, 1024, None), (128, 43264, (256, 169)), (192, 256, None)]
BN_STREAM = [(256 * 32 * 32, 64), (768 * 32 * 32, 128), (512 * 16 * 16, 256), (512 * 64 * 64, 32),
             (512 * 64 * 64 - 5, 32),
             # the row counts N H W of the 100-px planes at batch 64, none a power of two: 64 x 50 x 50, 64 x 25 x 25,
             # 64 x 13 x 13, 192 x 7 x 7, 128 x 100 x 100
             (160000, 64), (40000, 128), (10816, 256), (9408, 256), (1280000, 64)]


@pytest.mark.parametrize("M,C,perm", BN_COLS)
def test_batchnorm_column_path_at_engine_rows(M, C, perm):
    _run_bn_case(M, C, perm=perm, updates=1 + (M // 256) % 2)


@pytest.mark.parametrize("M,C", BN_STREAM)
def test_batchnorm_streaming_path_at_engine_rows(M, C):
    _run_bn_case(M, C, updates=1 + (C // 32) % 2)


def test_batchnorm_path_switch_at_2048_rows():
    """The same input cut to 2048 rows (bn_cols_*) and to 2049 rows (streaming kernels): _run_bn_case asserts which
    entry points ran, and each cut must match float64."""
    from fmri_hip import ops
    assert ops._BN_COLS_ROWS == 2048
    x16 = _bn_input(2049, 64, 11, False)
    _run_bn_case(2048, 64, x16=x16[:2048].contiguous(), updates=2)
    _run_bn_case(2049, 64, x16=x16.contiguous(), updates=2)


@pytest.mark.parametrize("M,C", [(768, 512), (512 * 64 * 64, 32)])
def test_batchnorm_hard_channels(M, C):
    """Off-centre channels (mean / std 2, 4, 8), an all-zero channel, and -- report only, apart from finiteness,
    var >= 0 and the running statistics -- a constant channel and one with mean / std = 64, among normal ones."""
    _run_bn_case(M, C, hard=True, updates=2, seed=5 * M + C)


# =====================================================================================================================
# C. loss / optimizer entry points
# =====================================================================================================================
@pytest.fixture(params=[False, True], ids=["default", "deterministic"])
def reduction_mode(request):
    from fmri_hip import ops
    was = ops.set_deterministic(request.param)
    try:
        yield request.param
    finally:
        ops.set_deterministic(was)


def _logits(n, seed):
    torch.manual_seed(seed)
    l = torch.randn(n) * 2
    l[::37] = 30.0
    l[5::41] = -30.0
    l[11::43] = 0.0
    l[17::47] = 10.0
    return l


@pytest.mark.parametrize("npix", [256 * 64 * 64, 256 * 64 * 64 - 37])
def test_pixel_sq_at_full_batch(npix, reduction_mode):
    """total = sum 0.5 (x - xt)^2 over the 3 real channels; dxt = -(x - xt) * gscale with zero padding channels; garbage
    in the padding channels of the inputs changes neither: dxt is bit-identical in both reduction modes, the total is
    bit-identical in deterministic mode (fixed order) -- in default mode the blocks meet in atomics, two launches of the
    SAME input may differ in the last bits, and each total is bounded against float64 on its own.  The total over 3 M terms has no precedent in
    test_loss_kernels: it is bounded by d u sum|terms|, d = the longest addition chain (per thread: pixels per thread x 3
    channels; 9 for the block's fold; then one atomic add per block -- 1024 blocks, or 1 in deterministic mode) + 2 for
    the roundings of one term."""
    from fmri_hip import lib
    P = lib.ptr
    case = f"C pixel_sq npix={npix} {'det' if reduction_mode else 'default'}"
    gen = torch.Generator(device=DEV)
    gen.manual_seed(npix)
    x = torch.randn(npix, 8, device=DEV, generator=gen).half()
    xt = (x.float() + 0.3 * torch.randn(npix, 8, device=DEV, generator=gen)).half()
    xz, xtz = x.clone(), xt.clone()
    xz[:, 3:] = 0
    xtz[:, 3:] = 0
    df = xz[:, :3].double() - xtz[:, :3].double()
    terms = 0.5 * df * df
    blocks = 1 if reduction_mode else min((npix + 255) // 256, 1024)
    per_thread = (npix + blocks * 256 - 1) // (blocks * 256)
    d = 3 * per_thread + 9 + blocks + 2
    tots, dxts = [], []
    for variant, a, b in (("padding garbage", x, xt), ("padding zero", xz, xtz)):
        tot = torch.zeros(1, device=DEV)
        dxt = torch.full((npix + 2, 8), 7.0, dtype=torch.float16, device=DEV)
        lib.call("fmri_pixel_sq", P(a), P(b), npix, 3, 8, P(tot), P(dxt), 0.37)
        torch.cuda.synchronize()
        tots.append(tot.clone())
        dxts.append(dxt)
        _bounded(case, f"total, {variant} (d = {d})", (tot.double() - terms.sum()).abs(),
                 d * U * terms.sum().reshape(1))
        _check(case, f"dxt, {variant}", dxt[:npix, :3], -df * 0.37, 2e-3)
        assert bool((dxt[:npix, 3:] == 0).all()), "padding channels of dxt"
        assert bool((dxt[npix:] == 7.0).all()), "dxt written behind the last pixel"
    assert torch.equal(dxts[0], dxts[1]), "padding garbage changed dxt"
    if reduction_mode:
        assert torch.equal(tots[0], tots[1]), "padding garbage changed the total"


def test_feat_mse_at_full_batch(reduction_mode):
    """Rows: the 1e-4 of test_loss_kernels.  Total (no precedent): d u sum|terms| with d = 64 elements per thread + 9
    (block fold) + 256 rows met in atomics (default) or summed by one block (deterministic) + 2."""
    from fmri_hip import lib
    P = lib.ptr
    case = f"C feat_mse {'det' if reduction_mode else 'default'}"
    B, Fd = 256, 16384
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    feat = torch.randn(3 * B, Fd, device=DEV, generator=gen).half()
    dif = feat[:B].double() - feat[B:2 * B].double()
    rows_ref = (0.5 * dif * dif).sum(1)
    rows = torch.zeros(B, device=DEV)
    tot = torch.zeros(1, device=DEV)
    lib.call("fmri_feat_mse", P(feat), B, Fd, P(rows), P(tot))
    _check(case, "rows", rows, rows_ref, 1e-4)
    d = Fd // 256 + 9 + B + 2
    _bounded(case, f"total (d = {d})", (tot.double() - rows_ref.sum()).abs(), d * U * rows_ref.sum().reshape(1))
    nrm = torch.tensor([2.0], device=DEV)
    dfeat = torch.full((3 * B + 1, Fd), 7.0, dtype=torch.float16, device=DEV)
    lib.call("fmri_feat_mse_bwd", P(feat), B, Fd, P(dfeat), 4.0, P(nrm))
    torch.cuda.synchronize()
    _check(case, "dfeat, original rows", dfeat[:B], dif * 8.0, 2e-3)
    _check(case, "dfeat, predicted rows", dfeat[B:2 * B], -dif * 8.0, 2e-3)
    assert bool((dfeat[2 * B:3 * B] == 0).all()) and bool((dfeat[3 * B:] == 7.0).all())


def _gan_ref(logit, B, parts):
    l = logit.double()
    p = torch.sigmoid(l)
    part = torch.arange(3 * B) // B
    bce = torch.where(part == 0, -torch.log(p + 1e-3), -torch.log(1 - p + 1e-3))
    dl = torch.where(part == 0, -p * (1 - p) / (p + 1e-3), p * (1 - p) / (1 - p + 1e-3))
    sel = torch.tensor([bool((parts >> k) & 1) for k in range(3)])[part]
    dl = torch.where(sel, dl, torch.zeros_like(dl))
    return p, torch.stack([bce[:B].sum(), bce[B:2 * B].sum(), bce[2 * B:].sum()]), dl


@pytest.mark.parametrize("parts", [0b111, 0b101])
def test_gan_head_parts_at_full_batch(parts, reduction_mode):
    """Bounds of test_loss_kernels: 1e-5 prob / bce sums, 1e-4 relative for the squared-cotangent sum, 2e-3 dlogit."""
    from fmri_hip import lib
    P = lib.ptr
    case = f"C gan_head parts={parts:03b} {'det' if reduction_mode else 'default'}"
    B = 256
    logit = _logits(3 * B, 7)
    p_ref, bce_ref, dl_ref = _gan_ref(logit, B, parts)
    assert bool(torch.isfinite(bce_ref).all())
    lgd = logit.to(DEV)
    scal = torch.zeros(24, device=DEV)
    prob = torch.empty(3 * B, device=DEV)
    lib.call("fmri_gan_head_parts", P(lgd), 1, B, P(prob), P(scal), parts)
    _check(case, "prob", prob, p_ref, 1e-5)
    _check(case, "bce sums", scal[:3], bce_ref, 1e-5)
    dl2 = dl_ref.pow(2).sum().item()
    _say(case, "sum dl^2 over the selected parts", abs(scal[9].item() - dl2) / (1e-4 * dl2))
    rest = torch.ones(24, dtype=torch.bool)
    rest[[0, 1, 2, 9]] = False
    assert bool((scal.cpu()[rest] == 0).all()), "a slot outside bce / dl2 was written"
    nrm = torch.tensor([0.5], device=DEV)
    dl16 = torch.full((3 * B + 2, 8), 7.0, dtype=torch.float16, device=DEV)
    lib.call("fmri_gan_head_bwd_parts", P(lgd), 1, B, P(dl16), 8, 32.0, P(nrm), parts)
    torch.cuda.synchronize()
    _check(case, "dlogit", dl16[:3 * B, 0], dl_ref * 16.0, 2e-3)
    assert bool((dl16[:3 * B, 1:] == 0).all()) and bool((dl16[3 * B:] == 7.0).all())
    if parts == 0b101:
        assert bool((dl16[B:2 * B, 0] == 0).all()), "the unselected part has a cotangent"


@pytest.mark.parametrize("n", [256, 512, 77])
@pytest.mark.parametrize("one_minus", [0, 1])
def test_wae_logloss_at_full_batch(n, one_minus, reduction_mode):
    from fmri_hip import lib
    P = lib.ptr
    case = f"C wae_logloss n={n} one_minus={one_minus} {'det' if reduction_mode else 'default'}"
    w, gs = 0.7, 16.0
    logit = _logits(n, n + one_minus)
    p = torch.sigmoid(logit.double())
    if one_minus:
        tot_ref, dl_ref = (-w * torch.log(1 - p + 1e-3)).sum(), w * p * (1 - p) / (1 - p + 1e-3)
    else:
        tot_ref, dl_ref = (-w * torch.log(p + 1e-3)).sum(), -w * p * (1 - p) / (p + 1e-3)
    lgd = logit.to(DEV)
    tot = torch.zeros(1, device=DEV)
    prob = torch.empty(n, device=DEV)
    dl16 = torch.full((n + 2, 8), 7.0, dtype=torch.float16, device=DEV)
    lib.call("fmri_wae_logloss", P(lgd), 1, n, one_minus, w, P(tot), P(prob), P(dl16), 8, gs)
    torch.cuda.synchronize()
    _check(case, "total", tot, tot_ref.reshape(1), 1e-5)
    _check(case, "prob", prob, p, 1e-5)
    _check(case, "dlogit", dl16[:n, 0], dl_ref * gs, 2e-3)
    assert bool((dl16[:n, 1:] == 0).all()) and bool((dl16[n:] == 7.0).all())


def _compose_ref(s, batch, nfeat, npix, hp, mode, gate_on, force_dis, force_dec):
    """The documented formulas of compose_gate_kernel (csrc/loss.hip) in Python floats.  Returns {slot: (value, sum of
    the magnitudes of the terms it is made of)} and the two flags."""
    lam, eq, margin, beta = hp
    bo, bp, bs, kl, mse, nle, dl2 = s[0], s[1], s[2], s[3], s[4], s[5], s[9]
    pix = mode in (2, 3)
    rec = nle if pix else mse
    l_dis = bo + bs if pix else bo + bp + bs
    klw = beta / batch if mode == 1 else 1.0
    na = 1 / max(math.sqrt(dl2 / (3 * batch)), 1e-20)
    nb = 1 / max(math.sqrt(2 * mse / (batch * nfeat)), 1e-20)
    npx = 1 / max(math.sqrt(2 * nle / (batch * max(npix, 1.0))), 1e-20)
    ldec = lam * rec if mode == 3 else lam * rec - (1 - lam) * l_dis
    out = {21: (klw, klw), 6: (klw * kl + rec, abs(klw * kl) + rec), 7: (l_dis, l_dis),
           8: (ldec, lam * rec + (0 if mode == 3 else (1 - lam) * l_dis)),
           10: (na, na), 11: (nb, nb), 16: (npx, npx), 12: (na / nb, na / nb), 13: (1.0, 0.0), 14: (0.0, 0.0),
           17: (lam * na / nb, lam * na / nb), 18: (1 - lam, 1.0), 19: (lam * na, lam * na),
           20: (npx / max(lam, 1e-30) if mode == 3 else na,) * 2}
    dis, dec = (0 if mode == 3 else 1), 1
    if gate_on:
        mo, mp = bo / batch, bp / batch
        if mo < eq - margin or mp < eq - margin:
            dis = 0
        if mo > eq + margin or mp > eq + margin:
            dec = 0
        if not dis and not dec:
            dis = dec = 1
    if force_dis >= 0:
        dis = force_dis
    if force_dec >= 0:
        dec = force_dec
    return out, [dis, dec]


def test_compose_gate_dev_every_mode_gate_and_flag():
    """All four loss compositions x gate on / off x forced flags x four gate situations (balanced, discriminator paused,
    decoder paused, both paused -> both train), hyper-parameters from the device vector.  Bounds: test_loss_kernels
    allows 1e-5 absolute on losses of size <= 18, i.e. 9 u relative; at B = 256 the losses are hundreds, so the same
    bound is stated relative to the terms: 8 u sum|terms| (a slot is at most 8 roundings deep), not wider than the
    precedent at its sizes.  The normalisation factors keep their 1e-4 relative."""
    from fmri_hip import lib
    P = lib.ptr
    B, nfeat, npix = 256.0, 16384.0, 3.0 * 64 * 64
    hp = [0.3, 0.68, 0.35, 4.0]
    # rounded to fp32 first: the restatement then starts from the numbers the kernel reads
    hp = [float(np.float32(v)) for v in hp]
    hp_dev = torch.tensor(hp, device=DEV)
    # mean bce_orig, mean bce_pred:          balanced      dis paused    dec paused   both paused
    situations = {"balanced": (0.6, 0.7), "dis paused": (0.2, 0.5), "dec paused": (0.6, 1.2), "both": (0.2, 1.2)}
    worst = {"loss slots": 0.0, "norm factors": 0.0}
    n = 0
    for sit, (mo, mp) in situations.items():
        base = [mo * B, mp * B, 0.5 * B, 1234.5, 5678.25, 91011.5, 0.0, 0.0, 0.0, 12.0 * B / 5] + [0.0] * 14
        base = [float(np.float32(v)) for v in base]
        for mode in range(4):
            for gate_on in (0, 1):
                for fd, fc in ((-1, -1), (0, 1), (1, 0)):
                    scal = torch.tensor(base, device=DEV)
                    scal[15] = 7.0                                    # not a slot of this kernel
                    flags = torch.full((2,), -9, dtype=torch.int32, device=DEV)
                    lib.call("fmri_compose_gate_dev", P(scal), P(flags), B, nfeat, npix, P(hp_dev), mode, gate_on, fd, fc)
                    s = scal.cpu().double().tolist()
                    ref, fl = _compose_ref(base, B, nfeat, npix, hp, mode, gate_on, fd, fc)
                    assert flags.tolist() == fl, (sit, mode, gate_on, fd, fc, flags.tolist(), fl)
                    for slot in (0, 1, 2, 3, 4, 5, 9):
                        assert s[slot] == base[slot], ("input slot changed", slot)
                    assert s[15] == 7.0
                    for slot, (v, mag) in ref.items():
                        err = abs(s[slot] - v)
                        if slot in (10, 11, 12, 16, 17, 19, 20):
                            r, key = err / (1e-4 * abs(v)), "norm factors"
                        else:
                            r, key = (0.0 if err == 0 else err / max(8 * U * mag, 1e-300)), "loss slots"
                        worst[key] = max(worst[key], r)
                        assert r <= 1.0, (sit, mode, gate_on, fd, fc, slot, s[slot], v, r)
                    n += 1
    assert n == 96
    # the rule itself, spelled out once: gate on, both sides outside the margin -> both train; 'vae' trains no
    # discriminator unless that rule re-arms it
    assert _compose_ref([0.2 * B, 1.2 * B] + [1.0] * 8, B, nfeat, npix, hp, 0, 1, -1, -1)[1] == [1, 1]
    assert _compose_ref([0.6 * B, 0.7 * B] + [1.0] * 8, B, nfeat, npix, hp, 3, 1, -1, -1)[1] == [0, 1]
    assert _compose_ref([0.2 * B, 1.2 * B] + [1.0] * 8, B, nfeat, npix, hp, 3, 1, -1, -1)[1] == [1, 1]
    for k, v in worst.items():
        _say("C compose_gate_dev (96 launches)", k, v)


def test_device_rate_optimizers_match_float64_torch():
    """fmri_rmsprop_dev / fmri_adam_dev: learning rate and step counter on the device (the rate changes every step, the
    counter goes through fmri_counter_inc), device gradient factor 4, clamp 0.5, flag gating, three steps, against
    torch.optim in float64 on the clamped true gradients; rtol 1e-6 / 2e-6 of test_optimizers_match_torch."""
    from fmri_hip import lib
    P = lib.ptr
    torch.manual_seed(3)
    n = 10007
    p0 = torch.randn(n)
    grads = [torch.randn(n) * (10.0 ** np.random.RandomState(i).uniform(-6, 0)) for i in range(3)]
    grads[1] = grads[1] * 3.0 / grads[1].abs().max() * 0.5          # some |g| above the clamp
    lrs = [1e-4, 5e-5, 2e-4]
    clamp = 0.5
    four = torch.tensor([4.0], device=DEV)
    on = torch.ones(1, dtype=torch.int32, device=DEV)
    off = torch.zeros(1, dtype=torch.int32, device=DEV)
    lr_dev = torch.zeros(1, device=DEV)
    assert any(float(g.abs().max()) > clamp for g in grads)

    pt = p0.double().clone().requires_grad_(True)
    opt = torch.optim.RMSprop([pt], lr=lrs[0], alpha=0.9, eps=1e-8)
    pd, sq = p0.to(DEV).clone(), torch.zeros(n, device=DEV)
    for lr, gr in zip(lrs, grads):
        opt.param_groups[0]["lr"] = float(np.float32(lr))
        pt.grad = gr.double().clamp(-clamp, clamp)
        opt.step()
        lr_dev.fill_(lr)
        g4 = (gr * 4.0).to(DEV)
        before = (pd.clone(), sq.clone())
        lib.call("fmri_rmsprop_dev", P(pd), P(g4), P(sq), n, P(lr_dev), 0.9, 1e-8, 1.0, P(four), clamp, P(off))
        assert torch.equal(pd, before[0]) and torch.equal(sq, before[1]), "flag = 0 updated"
        lib.call("fmri_rmsprop_dev", P(pd), P(g4), P(sq), n, P(lr_dev), 0.9, 1e-8, 1.0, P(four), clamp, P(on))
    ref = pt.detach().float()
    err = (pd.cpu() - ref).abs() / (1e-7 + 1e-6 * ref.abs())
    _say("C rmsprop_dev n=10007, 3 steps", "parameters (atol 1e-7 + rtol 1e-6)", float(err.max()))

    pt = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=lrs[0], betas=(0.5, 0.999), eps=1e-8)
    pd, m, v = p0.to(DEV).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    t_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    for lr, gr in zip(lrs, grads):
        opt.param_groups[0]["lr"] = float(np.float32(lr))
        pt.grad = gr.double().clamp(-clamp, clamp)
        opt.step()
        lr_dev.fill_(lr)
        g4 = (gr * 4.0).to(DEV)
        lib.call("fmri_counter_inc", P(t_dev))
        before = (pd.clone(), m.clone(), v.clone())
        lib.call("fmri_adam_dev", P(pd), P(g4), P(m), P(v), n, P(lr_dev), 0.5, 0.999, 1e-8, P(t_dev), 1.0, P(four), clamp,
                 P(off))
        assert all(torch.equal(a, b) for a, b in zip((pd, m, v), before)), "flag = 0 updated"
        lib.call("fmri_adam_dev", P(pd), P(g4), P(m), P(v), n, P(lr_dev), 0.5, 0.999, 1e-8, P(t_dev), 1.0, P(four), clamp,
                 P(on))
    assert int(t_dev) == 3
    ref = pt.detach().float()
    err = (pd.cpu() - ref).abs() / (1e-7 + 2e-6 * ref.abs())
    _say("C adam_dev n=10007, 3 steps", "parameters (atol 1e-7 + rtol 2e-6)", float(err.max()))


def test_renorm_f64_survives_squares_beyond_fp32(reduction_mode):
    """B x 2z = 256 x 256 cotangent values with entries of 1e20: their squares leave fp32, the double sum does not.
    Bounds: the double sum within n 2^-53 sum x^2 (worst case of any summation order); the factor within 4 u (a square
    root in double, one cast, one reciprocal, one product); the fp16 output within one fp16 unit of float64's (the fp32
    product can move a value across a rounding boundary: 2^-10 relative, 2^-24 in the subnormal range)."""
    from fmri_hip import lib
    P = lib.ptr
    case = f"C sumsq_f64 / renorm_f64 {'det' if reduction_mode else 'default'}"
    torch.manual_seed(9)
    n = 256 * 256
    x = torch.randn(n)
    big = [5, 4099, 30011, 65535]
    x[big] = torch.tensor([1e20, -1e20, 1e20, -1e20])
    xd = x.to(DEV)
    acc = torch.full((1,), 123.0, dtype=torch.float64, device=DEV)            # zero_first clears it
    lib.call("fmri_sumsq_f64", P(xd), n, P(acc), 1)
    ss = x.double().pow(2).sum()
    assert not math.isfinite(float(x.pow(2).sum())), "the case the f64 form exists for"
    _bounded(case, "sum of squares", (acc.cpu() - ss).abs(), (n * 2.0 ** -53 * ss).reshape(1))
    fin = torch.tensor([3.0], device=DEV)
    fout = torch.zeros(1, device=DEV)
    out = torch.full((n + 8,), 7.0, dtype=torch.float16, device=DEV)
    count, scale = float(n), 0.5
    lib.call("fmri_renorm_f64", P(xd), P(out), n, scale, P(acc), count, P(fin), P(fout))
    torch.cuda.synchronize()
    f = 1.0 / math.sqrt(float(ss) / count)
    assert math.isfinite(float(fout)) and float(fout) > 0
    _say(case, "factor_out = factor_in * f", abs(float(fout) - 3.0 * f) / (4 * U * 3.0 * f))
    ref = (x.double() * f * scale)
    got = out[:n].cpu().double()
    assert bool(torch.isfinite(got).all()) and bool((out[n:] == 7.0).all())
    _bounded(case, "fp16 rows", (got - ref).abs(), 2.0 ** -10 * ref.abs() + 2.0 ** -24)
    assert float(got[big[0]]) > 10.0                                          # the large entries carry the signal


def test_axpby2_f16_with_device_factors():
    from fmri_hip import lib
    P = lib.ptr
    case = "C axpby2_f16 n=256*16384"
    n = 256 * 16384
    gen = torch.Generator(device=DEV)
    gen.manual_seed(4)
    x = torch.randn(n, device=DEV, generator=gen).half()
    y = torch.randn(n, device=DEV, generator=gen).half()
    pa, pb = torch.tensor([3.0], device=DEV), torch.tensor([0.25], device=DEV)
    out = torch.full((n + 8,), 7.0, dtype=torch.float16, device=DEV)
    lib.call("fmri_axpby2_f16", P(x), P(y), P(out), n, 0.5, -1.5, P(pa), P(pb))
    _check(case, "a pa x + b pb y", out[:n], 1.5 * x.double() - 0.375 * y.double(), 2e-3)
    assert bool((out[n:] == 7.0).all())
    lib.call("fmri_axpby2_f16", P(x), None, P(out), n, 0.5, -1.5, P(pa), P(pb))
    _check(case, "a pa x (no y)", out[:n], 1.5 * x.double(), 2e-3)
    lib.call("fmri_axpby2_f16", P(x), P(y), P(out), n, 0.5, -1.5, None, None)
    _check(case, "a x + b y (no device factors)", out[:n], 0.5 * x.double() - 1.5 * y.double(), 2e-3)
    assert bool((out[n:] == 7.0).all())
