"""fmri_apply_batch's 16-byte path and the whole-line transposes (csrc/layout.hip), at the smallest shapes at which each
vector path and each fallback can go wrong.

A row of the update table takes the 16-byte path in mode 1 when its strides and base pointers allow it
(apply_entry_tiles records the decision in the last word of the row); every other row, and modes 0 / 3, keep the scalar
path.  ONE table holds all of it, vector and scalar rows next to each other, over one flat w / sq / grad buffer:

  kind 0, dense map (run = 64): 3 rows x B in {64, 72, 8} (one full tile, full + ragged, only ragged), 8 columns behind
      the taps, nslabs in {1, 2, 5, 6} (every remainder of the four-in-flight slab loop), clear in {0, 1}, with and
      without the fp16 copy, kpad 64 beyond run * Bp;
  kind 0, conv maps: run in {25, 9, 6, 4} x B in {40, 32, 8, 3} (bt = 32 full + ragged, and the 3-channel image layer
      whose row stride 3 * run is no multiple of 4 for the odd runs: scalar), A = 2; one role-exchanged map (sb != run);
  kind 1: 7 rows x B in {5, 128, 129}, and an out_perm map with TA > 1;
  kind 2: n in {1, 3, 4, 1023, 1024, 1025} at element offsets = 0, 1, 2, 3 (mod 4);
  forced fallbacks: a tensor of kinds 0 and 1 at an odd element offset of w / sq / grad, and one of each whose slab
      stride is = 2 (mod 4).

Sentinels sit in every gap, pad column, row without a copy and between the slabs (the helpers of
tests/test_layout_update_gpu.py, whose table-building code this module reuses).  The tolerances are that module's.

The library's blocks do not loop over tiles (one block per logical tile, as before), so there is no block cap to test.
The per-block records of fmri_apply_batch_stats carry ``written`` = 0 by design (fmri_stat_fold sets the flag), so the
stats test counts elements through the records' sums instead: a sum of squares over every updated element that agrees
with the downloaded buffers to the rounding of its double additions, and the integer count of clamped gradients.
"""
import ctypes
import functools
from collections import namedtuple

import numpy as np
import pytest

import test_layout_update_gpu as T
from layout_oracle import Spec, pad8, rmsprop_ref, touched, unpack_ref, valid_mask

pytestmark = pytest.mark.gpu

GUARD, SENT16, SENT32, U = T.GUARD, T.SENT16, T.SENT32, T.U
ALPHA, EPS, GDEV, CLAMP, LRS = T.ALPHA, T.EPS, T.GDEV, T.CLAMP, T.LRS
APPLY_CHUNK = T.APPLY_CHUNK
_exact, _bounded, _dev, _host, _bits, _call, _L, _torch = T._exact, T._bounded, T._dev, T._host, T._bits, T._call, T._L, T._torch

# r.case / r.nslabs / r.clear / r.has_pk / r.ld / r.scale as tests/test_layout_update_gpu.ApplyRow, plus: element offset
# of the tensor mod 4, what is added to the slab stride, what is added to kpad
VRow = namedtuple("VRow", "case nslabs clear has_pk ld scale w_mis stride_mis kpad_extra")
Flat = namedtuple("Flat", "n mis")


def _conv_rect(cout, cin, th, tw):
    """Conv2d weight [cout][cin][th][tw], rows co, reduce (tap, ci)."""
    kk = th * tw
    return Spec(sa=cin * kk, sta=0, A=cout, TA=1, sb=kk, stb=1, B=cin, KW=tw, TH=th, TW=tw), cout * cin * kk


def _items():
    """The table, in buffer order."""
    out, j = [], 0

    def row(name, spec_numel, kind, nslabs, clear, has_pk, extra=0, w_mis=0, stride_mis=0, kpad_extra=0):
        nonlocal j
        sp, numel = spec_numel
        case = T.Case(name, sp, numel, None, None, kind)
        out.append(VRow(case, nslabs, bool(clear), bool(has_pk), sp.TH * sp.TW * pad8(sp.B) + extra, 2.0 ** -(9 + j % 3),
                        w_mis, stride_mis, kpad_extra))
        j += 1

    def dense64(n, c):
        f, _, numel = T._dense(n, c * 64, in_perm=(c, 64))
        return f, numel

    flats = [Flat(n, mis) for n in (1, 3, 4, 1023, 1024, 1025) for mis in (0, 1, 2, 3)]
    for B in (64, 72, 8):
        for nslabs in (1, 2, 5, 6):
            for clear in (0, 1):
                for has_pk in (1, 0):
                    row(f"dense run 64 A=3 B={B}", dense64(3, B), 0, nslabs, clear, has_pk, extra=8, kpad_extra=64)
            out.append(flats.pop())
    for (th, tw) in ((5, 5), (3, 3), (2, 3), (2, 2)):
        for i, B in enumerate((40, 32, 8, 3)):
            row(f"conv run {th * tw} A=2 B={B}", _conv_rect(2, B, th, tw), 0, (2, 5, 1, 6)[i], (i + th) % 2, i != 2,
                extra=(0, 8, 24)[i % 3])
        out.append(flats.pop())
    row("conv5 d 40x5 (sb != run)", T._conv_d(40, 5, 5), 0, 2, 1, 1)
    for i, B in enumerate((5, 128, 129)):
        f, _, numel = T._dense(7, B)
        for nslabs in (1, 5):
            row(f"dense kind 1 7x{B}", (f, numel), 1, nslabs, (i + nslabs) % 2, nslabs == 1)
        out.append(flats.pop())
    f, _, numel = T._dense(8 * 16, 40, out_perm=(8, 16))
    row("out_perm kind 1 (TA=16) K=40", (f, numel), 1, 6, 1, 1)
    # forced fallbacks
    row("dense run 64 B=64 at an odd offset", dense64(3, 64), 0, 2, 1, 1, extra=8, w_mis=1)
    row("dense run 64 B=72 slab stride = 2 mod 4", dense64(3, 72), 0, 5, 1, 1, extra=8, stride_mis=2)
    f, _, numel = T._dense(7, 128)
    row("dense kind 1 7x128 at an odd offset", (f, numel), 1, 2, 1, 1, w_mis=3)
    row("dense kind 1 7x128 slab stride = 2 mod 4", (f, numel), 1, 6, 0, 1, stride_mis=2)
    row("dense run 64 B=72 (vector, behind the fallbacks)", dense64(3, 72), 0, 6, 1, 1, extra=8)
    return out + flats


def _expect_vec(r, off, stride, kpad):
    """The conditions of apply_entry_vec (csrc/layout.hip) restated; the buffers themselves are 16-byte aligned."""
    sp = r.case.spec
    if off % 4 or sp.sa % 4 or sp.sta % 4 or r.ld % 4 or stride % 4 or (r.has_pk and kpad % 4):
        return False
    return sp.sb == sp.TH * sp.TW if r.case.apply == 0 else sp.B % 4 == 0


class _VWorld(T._World):
    """tests/test_layout_update_gpu._World over this module's table: the same attributes, so its methods (make_slabs,
    make_grad, cleared, upload, download, apply, separate, pk_of) are used as they are."""

    def __init__(self, seed):
        torch = _torch()
        items = _items()
        self.rows = [it for it in items if isinstance(it, VRow)]
        rs = np.random.RandomState(seed)
        at, self.off, self.flat, order = GUARD, [], [], []
        for it in items:
            at = (at + 1 + 3) // 4 * 4 + (it.w_mis if isinstance(it, VRow) else it.mis)      # a gap of 1 .. 7 elements
            if isinstance(it, VRow):
                order.append((at, len(self.off)))
                self.off.append(at)
                at += it.case.numel
            else:
                order.append((at, -1 - len(self.flat)))
                self.flat.append((at, it.n))
                at += it.n
        self.n = at + GUARD
        self.covered = np.zeros(self.n, dtype=bool)
        self.is_flat = np.zeros(self.n, dtype=bool)
        for j, r in enumerate(self.rows):
            assert touched(r.case.spec, r.case.numel).all()
            self.covered[self.off[j]:self.off[j] + r.case.numel] = True
        for o, n in self.flat:
            assert not self.covered[o:o + n].any()
            self.covered[o:o + n] = True
            self.is_flat[o:o + n] = True
        self.w0 = np.where(self.covered, rs.uniform(0.05, 2.0, self.n) * rs.choice([-1.0, 1.0], self.n), SENT32).astype(np.float32)
        self.sq0 = np.where(self.covered, rs.uniform(0.0, 1.0, self.n) * (rs.uniform(size=self.n) > 0.1), SENT32).astype(np.float32)
        self.gs_off, self.pk_off, self.geo = [], [], []
        ga, pa = GUARD, GUARD
        for r in self.rows:
            rows, rows_pad, kpad = T.geometry(r.case.spec)
            kpad += r.kpad_extra
            stride = rows * r.ld + 40 + r.stride_mis
            self.geo.append((rows, rows_pad, kpad, stride))
            ga = (ga + 3) // 4 * 4
            self.gs_off.append(ga)
            ga += r.nslabs * stride + GUARD
            self.pk_off.append(pa if r.has_pk else None)
            if r.has_pk:
                pa += rows_pad * kpad + GUARD
        self.gs_n, self.pk_n = ga, pa
        self.pk0 = np.full(self.pk_n, SENT16, dtype=np.float16)
        self.pk_valid = np.zeros(self.pk_n, dtype=bool)
        for j, r in enumerate(self.rows):
            if r.has_pk:
                rows, rows_pad, kpad, _ = self.geo[j]
                self.pk_valid[self.pk_off[j]:self.pk_off[j] + rows_pad * kpad] = valid_mask(r.case.spec, rows_pad, kpad).ravel()
        self.w, self.sq = _dev(self.w0), _dev(self.sq0)
        self.grad = torch.empty(self.n, dtype=torch.float32, device=T.DEV)
        self.gs = torch.empty(self.gs_n, dtype=torch.float32, device=T.DEV)
        self.pk = _dev(self.pk0)
        self.lr = torch.zeros(1, dtype=torch.float32, device=T.DEV)
        self.gdev = torch.full((1,), GDEV, dtype=torch.float32, device=T.DEV)
        self.flags = {None: None, 1: torch.ones(1, dtype=torch.int32, device=T.DEV),
                      0: torch.zeros(1, dtype=torch.int32, device=T.DEV)}
        for t in (self.w, self.sq, self.grad, self.gs, self.pk):
            assert t.data_ptr() % 16 == 0
        L = _L().load()
        nbytes = L.fmri_apply_entry_bytes()
        tab, self.tiles, self.vec, self.vec_want = [], 0, [], []
        for o, j in order:
            host = ctypes.create_string_buffer(nbytes)
            wp, sp_, gp = (t.data_ptr() + 4 * o for t in (self.w, self.sq, self.grad))
            if j >= 0:
                r, sp = self.rows[j], self.rows[j].case.spec
                rows, rows_pad, kpad, stride = self.geo[j]
                pk = self.pk.data_ptr() + 2 * self.pk_off[j] if r.has_pk else None
                n = L.fmri_apply_entry_fill(host, self.gs.data_ptr() + 4 * self.gs_off[j], wp, sp_, gp, pk, *T.spec_args(sp),
                                            r.ld, kpad if r.has_pk else 0, r.nslabs, stride, 1 if r.clear else 0,
                                            float(r.scale), 0, self.tiles)
                assert n == T.expected_apply_blocks(sp, r.case.apply), (r.case.name, n)
                self.vec_want.append(_expect_vec(r, o, stride, kpad))
            else:
                flat_n = self.flat[-1 - j][1]
                n = L.fmri_apply_entry_fill(host, None, wp, sp_, gp, None, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 1, 0,
                                            0, 1.0, flat_n, self.tiles)
                assert n == (flat_n + APPLY_CHUNK - 1) // APPLY_CHUNK
                self.vec_want.append(False)
            self.vec.append(bool(int.from_bytes(host.raw[-4:], "little") & 1))
            tab.append(host.raw)
            self.tiles += n
        self.ntab = len(tab)
        self.order = order
        self.table = torch.frombuffer(bytearray(b"".join(tab)), dtype=torch.uint8).to(T.DEV)


@functools.lru_cache(maxsize=None)
def _world(k):
    return _VWorld(91)


def test_the_table_mixes_vector_and_scalar_rows_as_stated():
    """The decision the entry-fill function records per row (last word of the row) is the one the strides and base
    offsets give, the tile counts are the documented ones (asserted while the table is built), and the table holds every
    case of the module's docstring: vector and scalar rows of kinds 0 and 1 adjacent, every forced fallback scalar."""
    W = _world(0)
    assert W.vec == W.vec_want, [(W.rows[j].case.name if j >= 0 else "flat") for k, (o, j) in enumerate(W.order)
                                 if W.vec[k] != W.vec_want[k]]
    by_name = {W.rows[j].case.name: W.vec[k] for k, (o, j) in enumerate(W.order) if j >= 0}
    for name, v in by_name.items():
        print(f"[vector] row {name:52s} {'16-byte' if v else 'scalar'}")
    for name in ("dense run 64 B=64 at an odd offset", "dense run 64 B=72 slab stride = 2 mod 4", "conv5 d 40x5 (sb != run)",
                 "dense kind 1 7x128 at an odd offset", "dense kind 1 7x128 slab stride = 2 mod 4", "dense kind 1 7x129",
                 "dense kind 1 7x5", "conv run 25 A=2 B=3", "conv run 9 A=2 B=3"):
        assert by_name[name] is False, name
    for name in ("dense run 64 A=3 B=64", "dense run 64 A=3 B=72", "dense run 64 A=3 B=8", "conv run 25 A=2 B=40",
                 "conv run 25 A=2 B=32", "conv run 9 A=2 B=8", "conv run 6 A=2 B=40", "conv run 4 A=2 B=3",
                 "dense kind 1 7x128", "out_perm kind 1 (TA=16) K=40", "dense run 64 B=72 (vector, behind the fallbacks)"):
        assert by_name[name] is True, name
    pairs = list(zip(W.vec[:-1], W.vec[1:]))
    assert (True, False) in pairs and (False, True) in pairs
    assert {(o - 0) % 4 for o, n in W.flat} == {0, 1, 2, 3} and sorted({n for o, n in W.flat}) == [1, 3, 4, 1023, 1024, 1025]
    for n in (1, 3, 4, 1023, 1024, 1025):
        assert {o % 4 for o, m in W.flat if m == n} == {0, 1, 2, 3}, n


def test_mode1_three_steps_bits_of_the_separate_launches_and_float64():
    """Mode 1 for three steps on the mixed table: after every step the same BITS in w, sq and the fp16 copies as
    fmri_unpack_grad onto zeros + fmri_rmsprop_dev + fmri_pack_weight, w and sq inside the existing tolerances of the
    float64 trajectory, ``clear`` rows handed back as ``_World.cleared`` states (pad-channel garbage surviving), and
    every gap, guard, padding and row without a copy untouched."""
    A, B = _world(0), _world(1)
    assert A is not B
    for X in (A, B):
        X.upload(w=X.w0, sq=X.sq0, pk=X.pk0)
    w_ref, sq_ref = A.w0.astype(np.float64), A.sq0.astype(np.float64)
    beyond = 0
    for step, lr in enumerate(LRS):
        gs, gref = A.make_slabs(5300 + step)
        g0 = A.make_grad(5310 + step)
        g_all = np.where(A.is_flat, g0.astype(np.float64), gref)
        beyond += int(np.count_nonzero(np.abs(g_all[A.covered]) / GDEV > CLAMP))
        with np.errstate(invalid="ignore"):
            nw, ns = rmsprop_ref(w_ref, sq_ref, g_all, lr, ALPHA, EPS, 1.0, GDEV, CLAMP)
        w_ref, sq_ref = np.where(A.covered, nw, w_ref), np.where(A.covered, ns, sq_ref)
        for X in (A, B):
            X.upload(grad=g0, gs=gs)
        A.apply(1, lr)
        B.separate(lr)
        a, b = A.download(), B.download()
        case = f"vector apply mode 1 step {step + 1} ({A.ntab} rows, {A.tiles} blocks)"
        T._check_update(case, A, a, w_ref, sq_ref, step + 1, a["w"])
        _exact(case, "grad untouched", a["grad"], g0)
        _exact(case, "packed gradients: clear rows zeroed, pad channels / slab gaps / guards unchanged", a["gs"], A.cleared(gs))
        _exact(case, "w, sq = fmri_unpack_grad + fmri_rmsprop_dev (bits)", np.stack([a["w"], a["sq"]]),
               np.stack([b["w"], b["sq"]]))
        _exact(case, "fp16 copies = fmri_pack_weight of the separately updated w (valid regions)",
               np.where(A.pk_valid, a["pk"], SENT16), np.where(A.pk_valid, b["pk"], SENT16))
    assert beyond > 100


def test_mode0_and_mode3_on_the_mixed_table():
    """Modes 0 and 3 (scalar on every row) on the table whose rows carry the vector mark: exact, as the existing mode
    tests."""
    A, B = _world(0), _world(1)
    gs, gref = A.make_slabs(5400)
    g0 = A.make_grad(5401)
    A.upload(w=A.w0, sq=A.sq0, grad=g0, gs=gs, pk=A.pk0)
    A.apply(0)
    got = A.download()
    tensors = A.covered & ~A.is_flat
    want = np.where(tensors, gref.astype(np.float32), g0)
    assert (want.astype(np.float64)[tensors] == gref[tensors]).all()
    _exact("vector table mode 0", "grad = mapped slab sums; flat segments, gaps, guards unchanged", got["grad"], want)
    _exact("vector table mode 0", "w, sq unchanged", np.stack([got["w"], got["sq"]]), np.stack([A.w0, A.sq0]))
    _exact("vector table mode 0", "fp16 copies unchanged", got["pk"], A.pk0)
    _exact("vector table mode 0", "packed gradients: clear rows zeroed, the rest unchanged", got["gs"], A.cleared(gs))
    gs, _ = A.make_slabs(5410, nan=True)
    for X in (A, B):
        X.upload(w=X.w0, sq=X.sq0, grad=g0, gs=gs, pk=X.pk0)
    lr = LRS[0]
    with np.errstate(invalid="ignore"):
        w_ref, sq_ref = rmsprop_ref(A.w0, A.sq0, g0, lr, ALPHA, EPS, 1.0, GDEV, CLAMP)
    w_ref, sq_ref = np.where(A.covered, w_ref, A.w0), np.where(A.covered, sq_ref, A.sq0)
    A.apply(3, lr)
    B.separate(lr, from_slabs=False)
    a, b = A.download(), B.download()
    T._check_update("vector table mode 3", A, a, w_ref, sq_ref, 1, a["w"])
    _exact("vector table mode 3", "grad unchanged", a["grad"], g0)
    _exact("vector table mode 3", "packed gradients (NaN) not read, not cleared", a["gs"], gs)
    _exact("vector table mode 3", "w, sq = fmri_rmsprop_dev on the same gradient (bits)", np.stack([a["w"], a["sq"]]),
           np.stack([b["w"], b["sq"]]))
    _exact("vector table mode 3", "fp16 copies = fmri_pack_weight (valid regions)", np.where(A.pk_valid, a["pk"], SENT16),
           np.where(A.pk_valid, b["pk"], SENT16))


def test_gate_matrix_on_the_mixed_table():
    """flag in {NULL, 1, 0} x gated in {0, 1} in mode 1: a live launch gives the bits of the ungated one; with flag = 0
    nothing in w, sq or the fp16 copies changes and the ``clear`` pass runs iff gated == 0."""
    W = _world(0)
    gs, _ = W.make_slabs(5500)
    g0 = W.make_grad(5501)
    lr = LRS[2]
    live = None
    for flag in (None, 1, 0):
        for gated in (0, 1):
            W.upload(w=W.w0, sq=W.sq0, grad=g0, gs=gs, pk=W.pk0)
            W.apply(1, lr, flag, gated)
            got = W.download()
            case = f"vector table gate flag {'NULL' if flag is None else flag} gated {gated}"
            clears = flag != 0 or gated == 0
            _exact(case, "packed gradients " + ("cleared on the clear rows" if clears else "unchanged"), got["gs"],
                   W.cleared(gs) if clears else gs)
            _exact(case, "grad unchanged", got["grad"], g0)
            if flag == 0:
                _exact(case, "w, sq unchanged", np.stack([got["w"], got["sq"]]), np.stack([W.w0, W.sq0]))
                _exact(case, "fp16 copies unchanged", got["pk"], W.pk0)
            elif live is None:
                live = got
                assert np.count_nonzero(_bits(got["w"]) != _bits(W.w0)) > 0.3 * np.count_nonzero(W.covered)
            else:
                _exact(case, "w, sq = the ungated launch (bits)", np.stack([got["w"], got["sq"]]),
                       np.stack([live["w"], live["sq"]]))
                _exact(case, "fp16 copies = the ungated launch (bits)", got["pk"], live["pk"])


STAT = np.dtype([("sumsq", "<f8"), ("max", "<f4"), ("min", "<f4"), ("max_abs", "<f4"), ("nonfinite", "<i4"),
                 ("clamped", "<i4"), ("written", "<i4")])


def test_apply_batch_stats_records_every_updated_element_once():
    """fmri_apply_batch_stats on the mixed table: the same bits in w, sq and the copies as fmri_apply_batch, and the
    per-block records (gradient, weights) together hold every updated element exactly once -- max, min and max |.| equal
    those of the true-scale gradients (exact here: integer slab sums, power-of-two scales, gdev 4) and of the downloaded
    new weights; the sums of squares agree to n * 2^-53 relative (n double additions of non-negative terms, any order);
    the clamped count is the number of true-scale gradients beyond the clamp; nothing non-finite."""
    torch = _torch()
    A, B = _world(0), _world(1)
    gs, gref = A.make_slabs(5600)
    g0 = A.make_grad(5601)
    lr = LRS[1]
    for X in (A, B):
        X.upload(w=X.w0, sq=X.sq0, grad=g0, gs=gs, pk=X.pk0)
    assert STAT.itemsize == _L().STAT_BYTES
    part = torch.full((2 * A.tiles * STAT.itemsize,), 0xEE, dtype=torch.uint8, device=T.DEV)
    A.lr.fill_(lr)
    _call("fmri_apply_batch_stats", A.table.data_ptr(), A.ntab, A.tiles, 1, A.lr.data_ptr(), ALPHA, EPS, 1.0,
          A.gdev.data_ptr(), CLAMP, None, 0, part.data_ptr())
    B.apply(1, lr)
    a, b = A.download(), B.download()
    case = "vector table stats"
    _exact(case, "w, sq = fmri_apply_batch (bits)", np.stack([a["w"], a["sq"]]), np.stack([b["w"], b["sq"]]))
    _exact(case, "fp16 copies = fmri_apply_batch (bits)", a["pk"], b["pk"])
    rec = _host(part).view(STAT).reshape(A.tiles, 2)
    g_true = (np.where(A.is_flat, g0.astype(np.float64), gref) / GDEV)[A.covered]
    assert (g_true.astype(np.float32).astype(np.float64) == g_true).all(), "the true-scale gradients are exact in fp32"
    n = g_true.size
    for k, (what, v) in enumerate((("gradient", g_true), ("weights", a["w"][A.covered].astype(np.float64)))):
        r = rec[:, k]
        assert int(r["nonfinite"].sum()) == 0
        _exact(case, f"{what}: max, min, max |.| over the records",
               np.array([r["max"].max(), r["min"].min(), r["max_abs"].max()], dtype=np.float32),
               np.array([v.max(), v.min(), np.abs(v).max()], dtype=np.float32))
        ss = float(np.sum(v * v))
        _bounded(case, f"{what}: sum of squares over the records vs the downloaded buffers ({n} elements, n * 2^-53 relative)",
                 abs(float(r["sumsq"].sum()) - ss), 2.0 * n * 2.0 ** -53 * ss)
    want = int(np.count_nonzero(np.abs(g_true) > CLAMP))
    got = int(rec[:, 0]["clamped"].sum())
    print(f"[vector] {case} | clamped gradients | {got} of {n}, expected {want}", flush=True)
    assert got == want and want > 100


# ---------------------------------------------------------------------------------------------------------------------
# transposes
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 8), (8, 1), (63, 65), (64, 64), (65, 127), (200, 24)]


def _transpose_job(rs, R, C, taps=1):
    """(source [rbuf][lds] with zero padding, expected destination with guards, cip, cop, lds, ldd) of ``taps`` slices."""
    cip, cop = pad8(C), pad8(R)
    lds, ldd = taps * cip + 8, taps * cop + 8                      # ldd larger than R rounded up to 8
    rbuf = (R + 31) // 32 * 32
    src = np.zeros((rbuf, lds), dtype=np.float16)
    src[:R, :taps * cip].reshape(R, taps, cip)[:, :, :C] = rs.standard_normal((R, taps, C)).astype(np.float16)
    want = np.full((GUARD + cip * ldd + GUARD,), SENT16, dtype=np.float16)
    return src, want, cip, cop, lds, ldd, rbuf


@pytest.mark.parametrize("R,C", SHAPES)
def test_transpose_f16_exact_with_canaries(R, C):
    """fmri_transpose_f16: numpy's transpose bit for bit, zeros from R up to R rounded up to 8 (whole 16-byte items),
    sentinels everywhere else: columns from there to ld_dst, rows from C on, the guards."""
    rs = np.random.RandomState(6000 + R)
    src, want, cip, cop, lds, ldd, rbuf = _transpose_job(rs, R, C)
    body = want[GUARD:-GUARD].reshape(cip, ldd)
    body[:C, :cop] = 0
    body[:C, :R] = src[:R, :C].T
    s_dev, d_dev = _dev(src), _dev(np.full_like(want, SENT16))
    _call("fmri_transpose_f16", s_dev.data_ptr(), d_dev.data_ptr() + 2 * GUARD, R, C, rbuf, lds, ldd)
    _exact(f"transpose R={R} C={C}", "transpose, zero fill to 8, sentinel padding and guards", _host(d_dev), want)


def test_transpose_f16_batch_exact_with_canaries():
    """fmri_transpose_f16_batch: the six shapes as whole-matrix rows and one per-tap source (slice t at column t * Cip,
    written at column t' * Cop, taps in reverse order) in one table."""
    torch = _torch()
    L = _L().load()
    nbytes = L.fmri_transpose_entry_bytes()
    rs = np.random.RandomState(6100)
    tab, tiles, keep, checks = [], 0, [], []
    for R, C, taps in [(R, C, 1) for R, C in SHAPES] + [(13, 5, 9), (70, 72, 4)]:
        src, want, cip, cop, lds, ldd, rbuf = _transpose_job(rs, R, C, taps)
        body = want[GUARD:-GUARD].reshape(cip, ldd)
        s_dev, d_dev = _dev(src), _dev(np.full_like(want, SENT16))
        for t in range(taps):
            t2 = taps - 1 - t
            host = ctypes.create_string_buffer(nbytes)
            n = L.fmri_transpose_entry_fill(host, s_dev.data_ptr() + 2 * t * cip, d_dev.data_ptr() + 2 * (GUARD + t2 * cop), R, C,
                                            rbuf, lds - t * cip, lds, ldd, tiles)
            assert n == ((R + 63) // 64) * ((C + 63) // 64), (R, C, t, n)
            tab.append(host.raw)
            tiles += n
            body[:C, t2 * cop:t2 * cop + cop] = 0
            body[:C, t2 * cop:t2 * cop + R] = src[:R, t * cip:t * cip + C].T
        keep.append(s_dev)
        checks.append(((R, C, taps), d_dev, want))
    table = torch.frombuffer(bytearray(b"".join(tab)), dtype=torch.uint8).to(T.DEV)
    _call("fmri_transpose_f16_batch", table.data_ptr(), len(tab), tiles)
    for (R, C, taps), d_dev, want in checks:
        _exact(f"transpose batch R={R} C={C} taps={taps}", "transposed slices, zero fill to 8, sentinel padding and guards",
               _host(d_dev), want)
