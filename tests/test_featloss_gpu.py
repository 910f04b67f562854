"""The feature-loss head for wide rows (csrc/featloss.hip: fmri_feat_mse_wide / fmri_feat_mse_bwd_wide) on the GPU against
float64 and against the per-sample kernels it stands next to (fmri_feat_mse / fmri_feat_mse_bwd).

Shapes: B in {1, 3, 5}; F in {8, chunk - 8, chunk, chunk + 8, 43 264 (recon_level 3 at 100 px: 13 * 13 * 256), 131 072
(recon_level 1 at 64 px)}, chunk = fmri_feat_mse_wide_chunk() halves per (row, chunk) task -- one lane group, a ragged last
chunk, exactly one chunk, one chunk plus one lane group, many chunks with a ragged one, many full chunks.

Forward, exact grid.  Inputs k / 2 with |k| <= 4.  Then df = f_o - f_p is a multiple of 1/2 with |df| <= 4 and every term
0.5 df^2 is a multiple of 1/8 and <= 8, i.e. an integer <= 64 in units of 1/8.  The sum of ALL terms of a call is at most
64 B F units, which is <= 2^24 while B F <= 262 144 (= 2^24 / 64): every partial sum, in any order, is an integer <= 2^24
in units and exactly representable in fp32.  B is chosen per F so that this holds (B = 2 at 131 072, B = 5 at 43 264) and
the kernel's row sums and total must EQUAL the float64 sums in every bit.

Forward, random fp16 inputs.  u = 2^-24.  A term carries three roundings (df, df * df; 0.5 * is exact; hipcc may contract
nothing here, the library is built with -ffp-contract=off): relative error 3u.  A term's path to its row sum has
D_row = 15 (a lane adds its 16 terms of a chunk in sequence) + 6 (wave butterfly) + 2 (four waves) + nch (the fold adds
the nch chunk partials of a row in sequence) additions, to the total 1 + 6 + 2 + 1 more (rows of a lane, butterfly, waves,
the add onto *mse_total).  All terms are >= 0, so first order in u:
        |row   - row64|   <= (D_row + 3) u row64
        |total - total64| <= (D_row + 10 + 3) u total64
One err/bound line per check is printed (pytest -s).

Backward.  Rows [0, 2B) are bit-identical to fmri_feat_mse_bwd's; rows [2B, 3B) are zeros with the flag on and keep a
sentinel with the flag off.  Against float64: with inputs on a 2^-10 grid (|x| <= 8: f_o - f_p has 15 significant bits,
exact in fp32) and a power-of-two scale the fp16 store is the only rounding, so the result equals the float64 product
rounded to fp16 bit for bit; with random fp16 inputs and an arbitrary scale the fp32 product adds u |p| in front of the
fp16 store (tests/glue_oracle.py: bound_store16).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import glue_oracle as GO
from glue_oracle import F16, F32
from latent_oracle import U, f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

F_NAMES = ["8", "chunk-8", "chunk", "chunk+8", "43264", "131072"]
BATCHES = [1, 3, 5]


def _L():
    from fmri_hip import lib
    return lib


def _chunk():
    return int(_L().load().fmri_feat_mse_wide_chunk())


def _F(name):
    c = _chunk()
    return {"8": 8, "chunk-8": c - 8, "chunk": c, "chunk+8": c + 8, "43264": 43264, "131072": 131072}[name]


def _nch(F):
    return (F + _chunk() - 1) // _chunk()


@functools.lru_cache(maxsize=None)
def _inputs(kind, B, F):
    """(feat fp16 [3B][F] numpy, float64 row sums [B]) -- made once per shape and shared, never written."""
    rs = np.random.RandomState(1000 * B + F % 997 + {"grid": 0, "real": 1, "grid10": 2}[kind])
    if kind == "grid":
        x = (rs.randint(-4, 5, size=(3 * B, F)) / 2.0).astype(F16)
    elif kind == "grid10":
        x = (rs.randint(-8192, 8193, size=(3 * B, F)) / 1024.0).astype(F16)
    else:
        x = rs.standard_normal((3 * B, F)).astype(F16)
    x.setflags(write=False)
    d = f64(x[:B]) - f64(x[B:2 * B])
    rows = (0.5 * d * d).sum(1)
    rows.setflags(write=False)
    return x, rows


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _fwd_wide(feat, B, F, total0=0.0, want_rows=True):
    L = _L()
    n = int(L.load().fmri_feat_mse_wide_ws_floats(B, F))
    assert n == B * _nch(F)
    ws = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    rows = torch.full((B,), float("nan"), dtype=torch.float32, device=DEV) if want_rows else None
    total = torch.full((1,), total0, dtype=torch.float32, device=DEV)
    L.call("fmri_feat_mse_wide", L.ptr(feat), B, F, L.ptr(rows), L.ptr(total), L.ptr(ws), n)
    torch.cuda.synchronize()
    return rows, total


def _bwd(name, feat, B, F, gscale, norm, flag=None, fill=1234.0):
    L = _L()
    out = torch.full((3 * B, F), fill, dtype=torch.float16, device=DEV)
    if flag is None:
        L.call(name, L.ptr(feat), B, F, L.ptr(out), gscale, L.ptr(norm))
    else:
        L.call(name, L.ptr(feat), B, F, L.ptr(out), gscale, L.ptr(norm), flag)
    torch.cuda.synchronize()
    return out


def _say(results, case):
    for line in GO.lines(case, results):
        print(line, flush=True)
    assert GO.passed(results), (case, results)


@pytest.mark.parametrize("fname", F_NAMES)
def test_forward_exact_grid_equals_float64(fname):
    F = _F(fname)
    for B in ({"131072": [2], "43264": [5]}.get(fname, BATCHES)):
        assert B * F <= 262144                      # 64 B F units of 1/8 <= 2^24: every partial sum is exact in fp32
        x, rows64 = _inputs("grid", B, F)
        t = 0.5 * (f64(x[:B]) - f64(x[B:2 * B])) ** 2
        assert np.array_equal(t * 8, np.rint(t * 8)) and t.max() <= 8.0 and t.sum() * 8 <= 2.0 ** 24
        rows, total = _fwd_wide(_dev(x), B, F)
        res = [GO.bits("mse_rows", rows.cpu().numpy(), rows64.astype(F32)),
               GO.bits("mse_total", total.cpu().numpy(), np.array([rows64.sum()], dtype=F32))]
        assert f64(rows64.astype(F32)).tolist() == rows64.tolist()          # (the float64 sums are fp32 numbers)
        _say(res, f"feat_mse_wide grid B={B} F={F}")


@pytest.mark.parametrize("fname", F_NAMES)
@pytest.mark.parametrize("B", BATCHES)
def test_forward_random_inputs_within_the_summation_bound(B, fname):
    F = _F(fname)
    x, rows64 = _inputs("real", B, F)
    feat = _dev(x)
    rows, total = _fwd_wide(feat, B, F)
    d_row = 15 + 6 + 2 + _nch(F)
    res = [GO.rat("mse_rows", rows.cpu().numpy(), rows64, (d_row + 3) * U * rows64),
           GO.rat("mse_total", total.cpu().numpy(), np.array([rows64.sum()]),
                  np.array([(d_row + 10 + 3) * U * rows64.sum()]))]
    _say(res, f"feat_mse_wide real B={B} F={F}")
    # mse_rows is optional, and the total is ADDED onto *mse_total
    _, total_only = _fwd_wide(feat, B, F, want_rows=False)
    assert torch.equal(total_only, total)
    _, onto = _fwd_wide(feat, B, F, total0=1.5)
    assert onto.item() == float(F32(F32(1.5) + F32(total.item())))
    # the per-sample kernel computes the same quantity
    L = _L()
    rows_old = torch.empty(B, dtype=torch.float32, device=DEV)
    L.call("fmri_feat_mse", L.ptr(feat), B, F, L.ptr(rows_old), None)
    torch.cuda.synchronize()
    d_old = (F + 2047) // 2048 * 8 + 6 + 2             # a lane's sequential terms, butterfly, waves
    _say([GO.rat("mse_rows (fmri_feat_mse)", rows_old.cpu().numpy(), rows64, (d_old + 3) * U * rows64)],
         f"feat_mse per-sample kernel B={B} F={F}")


@pytest.mark.parametrize("fname", F_NAMES)
@pytest.mark.parametrize("B", BATCHES)
def test_forward_bits_do_not_depend_on_the_deterministic_switch(B, fname):
    from fmri_hip import ops
    F = _F(fname)
    feat = _dev(_inputs("real", B, F)[0])
    was = ops.set_deterministic(False)
    try:
        r0, t0 = _fwd_wide(feat, B, F)
        r1, t1 = _fwd_wide(feat, B, F)
        ops.set_deterministic(True)
        r2, t2 = _fwd_wide(feat, B, F)
        r3, t3 = _fwd_wide(feat, B, F)
    finally:
        ops.set_deterministic(was)
    for r, t in ((r1, t1), (r2, t2), (r3, t3)):
        assert torch.equal(r, r0) and torch.equal(t, t0)


@pytest.mark.parametrize("fname", F_NAMES)
@pytest.mark.parametrize("B", BATCHES)
def test_backward_equals_the_per_sample_kernel_and_float64(B, fname):
    F = _F(fname)
    for kind, gscale, nrm in (("grid10", 16.0, 0.5), ("real", 16.0, 0.37)):
        x, _ = _inputs(kind, B, F)
        feat = _dev(x)
        norm = torch.tensor([nrm], dtype=torch.float32, device=DEV)
        old = _bwd("fmri_feat_mse_bwd", feat, B, F, gscale, norm)
        on = _bwd("fmri_feat_mse_bwd_wide", feat, B, F, gscale, norm, flag=1)
        off = _bwd("fmri_feat_mse_bwd_wide", feat, B, F, gscale, norm, flag=0)
        again = _bwd("fmri_feat_mse_bwd_wide", feat, B, F, gscale, norm, flag=1)
        assert torch.equal(again.view(torch.int16), on.view(torch.int16))
        on_n, off_n, old_n = on.cpu().numpy(), off.cpu().numpy(), old.cpu().numpy()
        sc = float(F32(gscale) * F32(nrm))
        p = (f64(x[:B]) - f64(x[B:2 * B])) * sc
        res = [GO.bits("orig | pred rows vs fmri_feat_mse_bwd", on_n[:2 * B], old_n[:2 * B]),
               GO.bits("orig | pred rows, flag off", off_n[:2 * B], old_n[:2 * B]),
               GO.bits("sampled rows, flag on: zeros", on_n[2 * B:], np.zeros((B, F), dtype=F16)),
               GO.bits("sampled rows, flag off: untouched", off_n[2 * B:], np.full((B, F), 1234.0, dtype=F16))]
        if kind == "grid10":
            # f_o - f_p exact in fp32, power-of-two scale: one rounding, the fp16 store
            res += [GO.bits("+d vs fp16(float64)", on_n[:B], p.astype(F16)),
                    GO.bits("-d vs fp16(float64)", on_n[B:2 * B], (-p).astype(F16))]
        else:
            # df (u), df * sc (u) in fp32, then the fp16 store
            bound = GO.bound_store16(p, 2 * U * np.abs(p))
            res += [GO.rat("+d vs float64", on_n[:B], p, bound), GO.rat("-d vs float64", on_n[B:2 * B], -p, bound)]
        _say(res, f"feat_mse_bwd_wide {kind} B={B} F={F}")


def test_norm_pointer_is_optional_and_arguments_are_checked():
    L = _L()
    B, F = 3, _chunk() + 8
    feat = _dev(_inputs("real", B, F)[0])
    one = torch.ones(1, dtype=torch.float32, device=DEV)
    a = _bwd("fmri_feat_mse_bwd_wide", feat, B, F, 4.0, None, flag=1)
    b = _bwd("fmri_feat_mse_bwd_wide", feat, B, F, 4.0, one, flag=1)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    lib = L.load()
    p = ctypes.c_void_p(feat.data_ptr())
    n = int(lib.fmri_feat_mse_wide_ws_floats(B, F))
    assert lib.fmri_feat_mse_wide(p, B, F + 4, None, None, p, n, None) == -1          # F not a multiple of 8
    assert lib.fmri_feat_mse_wide(p, B, F, None, None, None, n, None) == -1           # no workspace
    assert lib.fmri_feat_mse_wide(p, B, F, None, None, p, n - 1, None) == -4          # workspace too small
    assert lib.fmri_feat_mse_bwd_wide(p, B, F, None, 1.0, None, 1, None) == -1
    assert lib.fmri_feat_mse_bwd_wide(p, 0, F, p, 1.0, None, 1, None) == -1
