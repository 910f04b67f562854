"""The weight-layout and one-launch update kernels of csrc/layout.hip against float64 / numpy, every element.

Every training step ends here: fmri_apply_batch sums the packed weight gradients over their slabs, maps them to the
reference layout, runs RMSprop and casts the new weights into the fp16 GEMM copies; fmri_pack_weight(_batch) and
fmri_transpose_f16_batch make the other copies.  A wrong element does not crash and gives no NaN.  The other tests reach
these kernels through whole layers (tolerances of fp16 GEMMs) or compare fmri_apply_batch with the separate launches it
shares its code with; here each kernel is compared with tests/layout_oracle.py, which calls nothing of the library:

  A. fmri_pack_weight / fmri_pack_weight_batch: all five routes, bit for bit with one round-to-nearest-even cast;
  B. fmri_unpack_grad: all three routes, slab counts on both sides of the four-way unrolled sum, bit for bit on
     integer-valued data (sums of integers are exact in any order), one case with the worst-case summation bound;
  C. fmri_apply_batch: one table of 100+ rows of all three kinds over one flat buffer, modes 0 - 3 and the gate matrix;
  D. fmri_transpose_f16_batch on per-tap slices and fmri_permute_chw.

One table of small shapes (rows <= 130, B <= 130, k <= 5, one 100-position flatten for the tap runs above 64) states,
per layout map, the route each entry point takes; test_table_states_its_routes_and_covers_all checks those statements
and that every route is there.  tests/test_layout_oracle_host.py checks the oracle and the block counts without a GPU.

Every check prints one line ``[layout] <case> | <quantity> | ...``: the number of differing elements for an exact
check (0 or the test fails), err/bound for a bounded one.
"""
import ctypes
import functools
from collections import namedtuple

import numpy as np
import pytest

from layout_oracle import Spec, extent, pack_ref, pad8, rmsprop_ref, touched, unpack_ref, valid_mask

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24                      # unit roundoff of fp32
GUARD = 64                          # sentinel elements in front of and behind every buffer
SENT16 = np.float16(-1234.0)
SENT32 = np.float32(-4321.5)
NSLABS = (1, 2, 4, 5, 8, 9)         # both sides of slab_sum's four-way unrolled loop (z = 1; z + 3 < nslabs; z += 4)
FLAT_LENGTHS = (1, 1023, 1025, 3000)   # around APPLY_CHUNK = 1024, the elements a block of kinds 1 / 2 takes
APPLY_CHUNK = 1024

# Geometry of the four output-parity classes fmri_tconv_class gives for k = 5, pad = 2: (cy, cx) -> (py, px, TH, TW)
# (the host test compares this with the library's answer)
CLASSES_K5P2 = {(0, 0): (0, 0, 3, 3), (0, 1): (0, 1, 3, 2), (1, 0): (1, 0, 2, 3), (1, 1): (1, 1, 2, 2)}

Case = namedtuple("Case", "name spec numel pack unpack apply")


def _conv_f(cout, cin, k):
    """Conv2d weight [cout][cin][k][k], rows co, reduce (tap, ci): ops.ConvLayer's forward copy and gradient map."""
    kk = k * k
    return Spec(sa=cin * kk, sta=0, A=cout, TA=1, sb=kk, stb=1, B=cin, KW=k, TH=k, TW=k), cout * cin * kk


def _conv_d(cout, cin, k):
    """The same weight, rows ci, reduce (tap, co): the stride-1 data-gradient copy / the role-exchanged gradient map."""
    kk = k * k
    return Spec(sa=kk, sta=0, A=cin, TA=1, sb=cin * kk, stb=1, B=cout, KW=k, TH=k, TW=k), cout * cin * kk


def _conv_class(cout, cin, cy, cx):
    """Parity class (cy, cx) of the stride-2 data gradient of a 5x5, pad-2 Conv2d weight (ops._tconv)."""
    py, px, th, tw = CLASSES_K5P2[(cy, cx)]
    return Spec(sa=25, sta=0, A=cin, TA=1, sb=cin * 25, stb=1, B=cout, KW=5, py=py, px=px, step=2, TH=th, TW=tw), \
        cout * cin * 25


def _dense(n, k, in_perm=None, out_perm=None):
    """(forward map, data-gradient map, elements) of ops.DenseLayer's weight [n][k]."""
    if in_perm:
        c, hw = in_perm
        return (Spec(sa=k, sta=0, A=n, TA=1, sb=hw, stb=1, B=c, KW=hw, TH=1, TW=hw),
                Spec(sa=hw, sta=1, A=c, TA=hw, sb=k, stb=0, B=n), n * k)
    if out_perm:
        c, hw = out_perm
        return (Spec(sa=hw * k, sta=k, A=c, TA=hw, sb=1, stb=0, B=k),
                Spec(sa=1, sta=0, A=k, TA=1, sb=hw * k, stb=k, B=c, KW=hw, TH=1, TW=hw), n * k)
    return Spec(sa=k, sta=0, A=n, TA=1, sb=1, stb=0, B=k), Spec(sa=1, sta=0, A=k, TA=1, sb=k, stb=0, B=n), n * k


def _table():
    t = []

    def add(name, spec_numel, pack, unpack, apply):
        t.append(Case(name, spec_numel[0], spec_numel[1], pack, unpack, apply))
    # name                                     map                      fmri_pack_weight  fmri_unpack_grad  apply kind
    add("conv5 f 5x3 (B=3)",                   _conv_f(5, 3, 5),        "tile",           "tile",           0)
    add("conv5 f 3x40 (B=40)",                 _conv_f(3, 40, 5),       "tile",           "tile",           0)
    add("conv5 f 2x64 (B=64)",                 _conv_f(2, 64, 5),       "tile",           "tile",           0)
    add("conv5 f 2x72 (B=72)",                 _conv_f(2, 72, 5),       "tile",           "tile",           0)
    add("conv5 f 2x130 (B=130)",               _conv_f(2, 130, 5),      "tile",           "tile",           0)
    add("conv3 f 7x3 (B=3)",                   _conv_f(7, 3, 3),        "tile",           "tile",           0)
    add("conv3 f 3x72 (B=72)",                 _conv_f(3, 72, 3),       "tile",           "tile",           0)
    add("conv5 d 40x5 (rows ci, B=40)",        _conv_d(40, 5, 5),       "tile",           "tile",           0)
    add("conv3 d 130x3 (rows ci, B=130)",      _conv_d(130, 3, 3),      "tile",           "tile",           0)
    for cy, cx in sorted(CLASSES_K5P2):
        add(f"tconv class ({cy},{cx}) 40x6",   _conv_class(40, 6, cy, cx), "tile",        "tapinner",       None)
    f, d, n = _dense(5, 8 * 16, in_perm=(8, 16))
    add("in_perm f HW=16 C=8 N=5",             (f, n),                  "tile",           "tile",           0)
    f, d, n = _dense(40, 8 * 16, in_perm=(8, 16))
    add("in_perm d HW=16 C=8 N=40 (sta=1)",    (d, n),                  "transpose_ta",   "generic",        None)
    f, d, n = _dense(3, 40 * 16, in_perm=(40, 16))
    add("in_perm f HW=16 C=40 N=3",            (f, n),                  "tile",           "tile",           0)
    f, d, n = _dense(2, 8 * 64, in_perm=(8, 64))
    add("in_perm f HW=64 C=8 N=2 (run 64)",    (f, n),                  "tile",           "tile",           0)
    f, d, n = _dense(3, 72 * 64, in_perm=(72, 64))
    add("in_perm f HW=64 C=72 N=3 (run 64)",   (f, n),                  "tile",           "tile",           0)
    f, d, n = _dense(3, 8 * 100, in_perm=(8, 100))
    add("in_perm f HW=100 C=8 N=3 (run 100)",  (f, n),                  "tapinner",       "tapinner",       None)
    f, d, n = _dense(8 * 16, 40, out_perm=(8, 16))
    add("out_perm f C=8 HW=16 K=40 (TA=16)",   (f, n),                  "generic",        "generic",        1)
    add("out_perm d C=8 HW=16 K=40 (tapped)",  (d, n),                  "transpose_a",    "generic",        None)
    f, d, n = _dense(40 * 3, 33, out_perm=(40, 3))
    add("out_perm f C=40 HW=3 K=33 (TA=3)",    (f, n),                  "generic",        "generic",        1)
    add("out_perm d C=40 HW=3 K=33 (tapped)",  (d, n),                  "transpose_a",    "generic",        None)
    f, d, n = _dense(7, 130)
    add("dense f 7x130",                       (f, n),                  "generic",        "generic",        1)
    add("dense d 7x130",                       (d, n),                  "transpose_a",    "generic",        None)
    f, d, n = _dense(130, 3)
    add("dense f 130x3",                       (f, n),                  "generic",        "generic",        1)
    add("dense d 130x3",                       (d, n),                  "transpose_a",    "generic",        None)
    return t


CASES = _table()
IDS = [c.name for c in CASES]


def run_of(sp):
    """Source taps a packed row touches: 1 + the last tap index."""
    return (sp.py + sp.step * (sp.TH - 1)) * sp.KW + (sp.px + sp.step * (sp.TW - 1)) + 1


def routes(sp):
    """(fmri_pack_weight route, fmri_unpack_grad route, fmri_apply_batch kind or None) restated from the conditions of
    pack_weight_launch / unpack_grad_launch / apply_entry_tiles (csrc/layout.hip): the library has no function to ask
    which kernel a single launch takes.  What CAN be observed is: fmri_pack_entry_fill returns blocks for exactly the
    'tile' maps and fmri_apply_entry_fill for exactly the kinds 0 / 1 (asserted here and in the host test); the generic
    pack kernel is the only one that zeroes the padding (asserted in section A)."""
    nt = sp.TH * sp.TW
    full = sp.py == 0 and sp.px == 0 and sp.step == 1 and sp.TW == sp.KW
    if nt > 1 and sp.stb == 1:
        pack = "tile" if run_of(sp) <= 64 else "tapinner"
    elif sp.TA == 1 and sp.sa == 1 and (nt == 1 or full):
        pack = "transpose_a"
    elif nt == 1 and sp.sta == 1 and sp.TA > 1:
        pack = "transpose_ta"
    else:
        pack = "generic"
    if 1 < nt <= 64 and sp.stb == 1 and full:
        unpack = "tile"
    elif nt > 1 and sp.stb == 1:
        unpack = "tapinner"
    else:
        unpack = "generic"
    kind = 0 if unpack == "tile" else (1 if (nt == 1 and sp.sb == 1) else None)
    return pack, unpack, kind


def geometry(sp):
    """(rows, rows_pad, kpad) the way ops._single sizes a packed buffer (32-row tiles)."""
    rows = sp.TA * sp.A
    return rows, (rows + 31) // 32 * 32, (sp.TH * sp.TW * pad8(sp.B) + 63) // 64 * 64


def spec_args(sp):
    return (sp.sa, sp.sta, sp.sb, sp.stb, sp.A, sp.TA, sp.B, sp.KW, sp.py, sp.px, sp.step, sp.TH, sp.TW)


def expected_pack_blocks(sp):
    return sp.TA * sp.A * ((sp.B + 31) // 32)


def expected_apply_blocks(sp, kind):
    rows = sp.TA * sp.A
    if kind == 0:
        bt = 64 if sp.B >= 64 else 32
        return rows * ((sp.B + bt - 1) // bt)
    return (rows * sp.B + APPLY_CHUNK - 1) // APPLY_CHUNK


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _L():
    from fmri_hip import lib
    return lib


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    _torch().cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _exact(case, what, got, ref):
    """Bit-for-bit comparison of two arrays of one dtype; prints and asserts the number of differing elements."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (case, what, got.dtype, ref.dtype, got.shape, ref.shape)
    bad = _bits(got) != _bits(ref)
    n = int(np.count_nonzero(bad))
    print(f"[layout] {case} | {what} | differing elements = {n} of {got.size}", flush=True)
    if n:
        where = np.argwhere(bad)[:8]
        shown = [(tuple(int(v) for v in i), got[tuple(i)], ref[tuple(i)]) for i in where]
        raise AssertionError(f"{case}: {what}: {n} of {got.size} elements differ; first (index, got, ref): {shown}")
    return n


def _bounded(case, what, err, bound):
    """max err / bound over the elements (0 / 0 counts as 0, err > 0 on a zero bound as a miss)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.isfinite(err).all(), f"{case}: {what}: non-finite"
    r = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    r = float(r.max()) if r.size else 0.0
    print(f"[layout] {case} | {what} | err/bound = {r:.4f}", flush=True)
    assert r <= 1.0, f"{case}: {what}: err / bound = {r:.4f}"
    return r


def _fp16_range_values(n, seed):
    """fp32 values over fp16's NORMAL range (|v| >= 2^-13.9: nothing the cast would make subnormal), every fifth an
    exact tie between two neighbouring fp16 numbers ((1 + (2m + 1) / 2048) 2^e: twelve significant bits), every eleventh
    at or above the largest fp16 number: 65504, 65512 (rounds down to 65504), the last fp32 below 65520, 65520 (the tie
    that rounds to infinity), 65536, 1e5, 3e38."""
    rs = np.random.RandomState(seed)
    sign = rs.choice([-1.0, 1.0], n)
    v = 2.0 ** rs.uniform(-13.9, 15.9, n) * sign
    i = np.arange(n)
    m, e = rs.randint(0, 1024, n), rs.randint(-14, 16, n)
    tie = (1.0 + (2 * m + 1) / 2048.0) * 2.0 ** e * sign
    v = np.where(i % 5 == 1, tie, v)
    big = np.array([65504.0, 65512.0, float(np.nextafter(np.float32(65520.0), np.float32(0.0))), 65520.0, 65536.0, 1e5,
                    3e38])
    v = np.where(i % 11 == 3, big[rs.randint(0, len(big), n)] * sign, v)
    return v.astype(np.float32)                 # (3e38 rounds to fp32: whatever fp32 holds is the input)


def _f16(x):
    """The one round-to-nearest-even cast float64 (holding fp32 values) -> fp16; values beyond 65520 become inf."""
    with np.errstate(over="ignore"):
        return np.asarray(x).astype(np.float16)


def _call(name, *args):
    _L().call(name, *args)


# ---------------------------------------------------------------------------------------------------------------------
# the table itself
# ---------------------------------------------------------------------------------------------------------------------
def test_table_states_its_routes_and_covers_all():
    """The routes written into the table are what the launch conditions give, the library's own block counts agree with
    them (blocks from fmri_pack_entry_fill for exactly the 'tile' maps, from fmri_apply_entry_fill for exactly kinds
    0 / 1, with the counts the header documents), and the table as a whole reaches every pack route, every unpack route,
    every apply kind and every edge the module's docstring names."""
    L = _L().load()
    pe, ae = ctypes.create_string_buffer(L.fmri_pack_entry_bytes()), ctypes.create_string_buffer(L.fmri_apply_entry_bytes())
    fake = ctypes.c_void_p(0x10000)
    for c in CASES:
        sp = c.spec
        assert routes(sp) == (c.pack, c.unpack, c.apply), (c.name, routes(sp))
        assert extent(sp) <= c.numel, c.name
        rows, rows_pad, kpad = geometry(sp)
        assert rows <= 130 and sp.B <= 130, c.name
        n = L.fmri_pack_entry_fill(pe, fake, fake, *spec_args(sp), rows_pad, kpad, 0)
        assert n == (expected_pack_blocks(sp) if c.pack == "tile" else 0), (c.name, n)
        n = L.fmri_apply_entry_fill(ae, fake, fake, fake, fake, fake, *spec_args(sp), kpad, kpad, 1, rows * kpad, 0, 1.0, 0, 0)
        assert n == (expected_apply_blocks(sp, c.apply) if c.apply is not None else 0), (c.name, n)
        print("[layout] route %-40s pack %-12s unpack %-8s apply kind %s" % (c.name, c.pack, c.unpack, c.apply))
    for flat in FLAT_LENGTHS:
        n = L.fmri_apply_entry_fill(ae, None, fake, fake, fake, None, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 1, 0, 0, 1.0,
                                    flat, 0)
        assert n == (flat + APPLY_CHUNK - 1) // APPLY_CHUNK, (flat, n)
    assert {c.pack for c in CASES} == {"tile", "tapinner", "transpose_a", "transpose_ta", "generic"}
    assert {c.unpack for c in CASES} == {"tile", "tapinner", "generic"}
    assert {c.apply for c in CASES} == {0, 1, None}               # kind 2: the flat segments of section C
    k0 = [c.spec for c in CASES if c.apply == 0]
    for k in (5, 3):                                              # the b tile: 32 wide below 64, 64 wide from 64 on, ragged
        assert {3, 72} <= {s.B for s in k0 if s.KW == k and s.TH == k}, k
    assert {3, 40, 64, 72, 130} <= {s.B for s in k0 if s.TH == 5}
    assert any(s.TH * s.TW == 64 for s in k0), "run = 64: LDS stride 65"
    assert any(run_of(c.spec) > 64 and c.pack == "tapinner" and c.unpack == "tapinner" for c in CASES)
    assert any(c.apply == 1 and c.spec.TA > 1 for c in CASES), "kind-1 rows with TA > 1 (out_perm dense)"
    assert any(c.apply == 1 and (c.spec.TA * c.spec.A * c.spec.B) % APPLY_CHUNK for c in CASES)
    assert sum(c.spec.step == 2 for c in CASES) == 4, "the four parity classes"
    assert any(c.pack == "transpose_a" and c.spec.TH * c.spec.TW > 1 for c in CASES), "tapped transpose"
    assert any(c.pack == "transpose_a" and c.spec.TH * c.spec.TW == 1 for c in CASES)
    assert len(_apply_rows()) + len(FLAT_LENGTHS) > 64 and 64 < PACK_REPEAT * sum(c.pack == "tile" for c in CASES)


# =====================================================================================================================
# A. fmri_pack_weight, fmri_pack_weight_batch
# =====================================================================================================================
PACK_REPEAT = 4


@functools.lru_cache(maxsize=None)
def _pack_source(i):
    return _fp16_range_values(CASES[i].numel, 1000 + i)


@functools.lru_cache(maxsize=None)
def _pack_single(i):
    """The whole destination buffer (guards included) after ONE fmri_pack_weight launch onto sentinels."""
    torch = _torch()
    c = CASES[i]
    rows, rows_pad, kpad = geometry(c.spec)
    src = _dev(_pack_source(i))
    dst = torch.full((GUARD + rows_pad * kpad + GUARD,), float(SENT16), dtype=torch.float16, device=DEV)
    _call("fmri_pack_weight", src.data_ptr(), dst.data_ptr() + 2 * GUARD, *spec_args(c.spec), rows_pad, kpad)
    return _host(dst)


def _pack_expected(i):
    """(expected buffer for a fast path, valid mask) of case i: reference bits inside the valid region, sentinel elsewhere."""
    c = CASES[i]
    rows, rows_pad, kpad = geometry(c.spec)
    ref = _f16(pack_ref(_pack_source(i), c.spec, rows_pad, kpad))
    valid = valid_mask(c.spec, rows_pad, kpad)
    body = np.where(valid, ref, SENT16 if c.pack != "generic" else np.float16(0.0))
    guard = np.full(GUARD, SENT16, dtype=np.float16)
    return np.concatenate([guard, body.ravel(), guard]), valid


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_pack_weight_is_one_rne_cast_of_the_documented_map(i):
    """Inside the valid region every packed element is the round-to-nearest-even fp16 cast of its source element (ties,
    the values around 65504 and the overflow to infinity included); outside it the fast paths leave the destination
    alone (sentinel intact: the caller zeroed the padding once) and the generic kernel, which owns the padding, writes
    zeros; nothing is written in front of or behind the buffer."""
    c = CASES[i]
    got = _pack_single(i)
    want, valid = _pack_expected(i)
    ref_valid = want[GUARD:-GUARD][valid.ravel()]
    assert np.isinf(ref_valid).any() and (np.abs(ref_valid.astype(np.float64)) < 1e-3).any(), "the value set spans the range"
    case = f"A pack {c.name} [{c.pack}]"
    _exact(case, "valid region (fp16 bits)", got[GUARD:-GUARD][valid.ravel()], ref_valid)
    _exact(case, "padding (%s) and guards" % ("zero" if c.pack == "generic" else "sentinel"),
           np.where(np.concatenate([np.zeros(GUARD, bool), valid.ravel(), np.zeros(GUARD, bool)]), SENT16, got),
           np.where(np.concatenate([np.zeros(GUARD, bool), valid.ravel(), np.zeros(GUARD, bool)]), SENT16, want))


def test_pack_weight_batch_equals_the_single_launches():
    """One table of every eligible map, repeated to more than 64 rows (the entry search strides over the table), every
    row with its own destination: the same bits as the single launches, guards and padding included."""
    torch = _torch()
    L = _L().load()
    nbytes = L.fmri_pack_entry_bytes()
    elig = [i for i, c in enumerate(CASES) if c.pack == "tile"]
    rows_tab, dsts, keep, tiles = [], [], [], 0
    for rep in range(PACK_REPEAT):
        for i in elig:
            c = CASES[i]
            rows, rows_pad, kpad = geometry(c.spec)
            src = _dev(_pack_source(i))
            dst = torch.full((GUARD + rows_pad * kpad + GUARD,), float(SENT16), dtype=torch.float16, device=DEV)
            host = ctypes.create_string_buffer(nbytes)
            n = L.fmri_pack_entry_fill(host, src.data_ptr(), dst.data_ptr() + 2 * GUARD, *spec_args(c.spec), rows_pad, kpad,
                                       tiles)
            assert n == expected_pack_blocks(c.spec), (c.name, n)
            rows_tab.append(host.raw)
            tiles += n
            dsts.append((i, dst))
            keep.append(src)
    assert len(rows_tab) > 64
    table = torch.frombuffer(bytearray(b"".join(rows_tab)), dtype=torch.uint8).to(DEV)
    _call("fmri_pack_weight_batch", table.data_ptr(), len(rows_tab), tiles)
    bad = 0
    for j, (i, dst) in enumerate(dsts):
        got, single = _host(dst), _pack_single(i)
        n = int(np.count_nonzero(_bits(got) != _bits(single)))
        assert n == 0, f"table row {j} ({CASES[i].name}): {n} elements differ from the single launch"
        bad += n
    print(f"[layout] A pack batch {len(rows_tab)} rows, {tiles} blocks | all buffers vs single launches | "
          f"differing elements = {bad} of {sum(d.numel() for _, d in dsts)}", flush=True)


# =====================================================================================================================
# B. fmri_unpack_grad
# =====================================================================================================================
def _unpack_launch(sp, slabs_dev, dst_dev, ld, scale, accumulate, nslabs, slab_stride):
    _call("fmri_unpack_grad", slabs_dev.data_ptr(), dst_dev.data_ptr() + 4 * GUARD, *spec_args(sp), ld, float(scale),
          accumulate, nslabs, slab_stride)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_unpack_grad_sums_the_slabs_exactly(i):
    """Integer-valued slabs (|v| <= 1024, the padding columns and a spare row behind every slab filled too: they must not
    be read), scale 1/8: every sum and product is exact in fp32 in any order, so the result is compared bit for bit, with
    ``accumulate`` = 0 onto garbage (stored, elements the map does not reach left alone) and = 1 onto integers."""
    c = CASES[i]
    sp = c.spec
    rows, rows_pad, kpad = geometry(sp)
    ld, scale = kpad + 8, 0.125
    rs = np.random.RandomState(2000 + i)
    mask = touched(sp, c.numel)
    guard = np.full(GUARD, SENT32, dtype=np.float32)
    for accumulate in (0, 1):
        diff = 0
        for nslabs in NSLABS:
            slabs = rs.randint(-1024, 1025, (nslabs, rows + 1, ld)).astype(np.float32)
            before = (rs.standard_normal(c.numel) * 100.0 if accumulate == 0 else
                      rs.randint(-1024, 1025, c.numel)).astype(np.float32)
            dst = _dev(np.concatenate([guard, before, guard]))
            _unpack_launch(sp, _dev(slabs), dst, ld, scale, accumulate, nslabs, (rows + 1) * ld)
            if accumulate:
                ref = unpack_ref(slabs, sp, ld, scale, into=before)
            else:
                ref = np.where(mask, unpack_ref(slabs, sp, ld, scale, into=np.zeros(c.numel)), before)
            want = np.concatenate([guard, ref.astype(np.float32), guard])
            assert (want[GUARD:-GUARD].astype(np.float64) == ref).all(), "the reference is exact in fp32"
            got = _host(dst)
            n = int(np.count_nonzero(_bits(got) != _bits(want)))
            assert n == 0, (f"B unpack {c.name} [{c.unpack}] nslabs {nslabs} accumulate {accumulate}: {n} elements differ; "
                            f"first at {np.flatnonzero(_bits(got) != _bits(want))[:8] - GUARD}")
            diff += n
        print(f"[layout] B unpack {c.name} [{c.unpack}] | accumulate = {accumulate}, nslabs {NSLABS}, guards | "
              f"differing elements = {diff} of {len(NSLABS) * (c.numel + 2 * GUARD)}", flush=True)


@pytest.mark.parametrize("route", ["tile", "tapinner", "generic"])
def test_unpack_grad_rounding_stays_inside_the_summation_bound(route):
    """Non-integer slabs and scale 0.37: per element within nslabs * 2^-24 * sum_z |slab value| * |scale| of float64 --
    the first-order worst case of ANY order of nslabs - 1 additions plus the product with the scale."""
    i = next(j for j, c in enumerate(CASES) if c.unpack == route)
    c = CASES[i]
    sp = c.spec
    rows, rows_pad, kpad = geometry(sp)
    ld = kpad
    scale = float(np.float32(0.37))
    rs = np.random.RandomState(2500 + i)
    mask = touched(sp, c.numel)
    guard = np.full(GUARD, SENT32, dtype=np.float32)
    for nslabs in (5, 9):
        slabs = (rs.standard_normal((nslabs, rows, ld)) * 10.0 ** rs.uniform(-3, 2, (nslabs, rows, ld))).astype(np.float32)
        before = rs.standard_normal(c.numel).astype(np.float32)
        dst = _dev(np.concatenate([guard, before, guard]))
        _unpack_launch(sp, _dev(slabs), dst, ld, scale, 0, nslabs, rows * ld)
        got = _host(dst)
        ref = unpack_ref(slabs, sp, ld, scale, into=np.zeros(c.numel))
        bound = nslabs * U * unpack_ref(np.abs(slabs), sp, ld, abs(scale), into=np.zeros(c.numel))
        case = f"B unpack {c.name} [{route}] nslabs {nslabs}, scale 0.37"
        _bounded(case, "gradient vs float64", np.abs(got[GUARD:-GUARD].astype(np.float64) - ref)[mask], bound[mask])
        _exact(case, "untouched elements and guards", np.where(mask, np.float32(0), got[GUARD:-GUARD]),
               np.where(mask, np.float32(0), before))
        _exact(case, "guards", np.concatenate([got[:GUARD], got[-GUARD:]]), np.concatenate([guard, guard]))


# =====================================================================================================================
# C. fmri_apply_batch
# =====================================================================================================================
ApplyRow = namedtuple("ApplyRow", "case nslabs clear has_pk ld scale")
ALPHA, EPS, GDEV, CLAMP = 0.9, 1e-8, 4.0, 0.5
LRS = (1e-4, 5e-5, 2e-4)


def _apply_rows():
    """Every eligible map of the table with every slab count: ``clear`` on every second row, no fp16 copy on every
    third, and (kind 0) 0 / 8 / 24 columns behind the taps up to ``ld``."""
    out, j = [], 0
    for c in CASES:
        if c.apply is None:
            continue
        for nslabs in NSLABS:
            rows, rows_pad, kpad = geometry(c.spec)
            extra = (0, 8, 24)[j % 3] if c.apply == 0 else 0
            out.append(ApplyRow(c, nslabs, j % 2 == 0, j % 3 != 1, c.spec.TH * c.spec.TW * pad8(c.spec.B) + extra,
                                2.0 ** -(9 + j % 3)))
            j += 1
    return out


class _World:
    """One flat w / sq / grad buffer laid out the way ops._plan_apply sees a sub-network -- tensors with gaps between them,
    flat segments of 1-D parameters in between -- one buffer of all packed gradients and one of all fp16 copies, each part
    between sentinel guards, and the device table over them (kind-0, kind-1 and kind-2 rows mixed, more than 64)."""

    SLAB_PAD = 40          # floats between two slabs of one row that belong to nobody

    def __init__(self, seed):
        torch = _torch()
        self.rows = _apply_rows()
        rs = np.random.RandomState(seed)
        # --- flat layout -------------------------------------------------------------------------------------------
        flats = dict(zip((9, 39, 69, 99), FLAT_LENGTHS))       # a flat segment behind these rows
        at, self.off, self.flat = GUARD, [], []
        for j, r in enumerate(self.rows):
            self.off.append(at)
            at += r.case.numel + 1 + 3 * (j % 4)                # a gap of 1 / 4 / 7 / 10 elements
            if j in flats:
                self.flat.append((at, flats[j]))
                at += flats[j] + 5
        assert len(self.flat) == len(FLAT_LENGTHS)
        self.n = at + GUARD
        self.covered = np.zeros(self.n, dtype=bool)
        self.is_flat = np.zeros(self.n, dtype=bool)
        for j, r in enumerate(self.rows):
            self.covered[self.off[j]:self.off[j] + r.case.numel] |= touched(r.case.spec, r.case.numel)
            assert touched(r.case.spec, r.case.numel).all()    # (every eligible map reaches its whole tensor)
        for o, n in self.flat:
            self.covered[o:o + n] = True
            self.is_flat[o:o + n] = True
        # weights in [0.05, 2): nothing the three steps could move into fp16's subnormal range
        self.w0 = np.where(self.covered, rs.uniform(0.05, 2.0, self.n) * rs.choice([-1.0, 1.0], self.n), SENT32).astype(np.float32)
        self.sq0 = np.where(self.covered, rs.uniform(0.0, 1.0, self.n) * (rs.uniform(size=self.n) > 0.1), SENT32).astype(np.float32)
        # --- packed gradients and fp16 copies ----------------------------------------------------------------------------
        self.gs_off, self.pk_off, self.geo = [], [], []
        ga, pa = GUARD, GUARD
        for r in self.rows:
            rows, rows_pad, kpad = geometry(r.case.spec)
            stride = rows * r.ld + self.SLAB_PAD
            self.geo.append((rows, rows_pad, kpad, stride))
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
        # --- device side ---------------------------------------------------------------------------------------------------
        self.w, self.sq = _dev(self.w0), _dev(self.sq0)
        self.grad = torch.empty(self.n, dtype=torch.float32, device=DEV)
        self.gs = torch.empty(self.gs_n, dtype=torch.float32, device=DEV)
        self.pk = _dev(self.pk0)
        self.lr = torch.zeros(1, dtype=torch.float32, device=DEV)
        self.gdev = torch.full((1,), GDEV, dtype=torch.float32, device=DEV)
        self.flags = {None: None, 1: torch.ones(1, dtype=torch.int32, device=DEV),
                      0: torch.zeros(1, dtype=torch.int32, device=DEV)}
        L = _L().load()
        nbytes = L.fmri_apply_entry_bytes()
        tab, self.tiles = [], 0
        entries = [(self.off[j], j) for j in range(len(self.rows))] + [(o, -1 - k) for k, (o, n) in enumerate(self.flat)]
        for o, j in sorted(entries):                                # table in buffer order, flat segments in between
            host = ctypes.create_string_buffer(nbytes)
            wp, sp_, gp = (t.data_ptr() + 4 * o for t in (self.w, self.sq, self.grad))
            if j >= 0:
                r, sp = self.rows[j], self.rows[j].case.spec
                rows, rows_pad, kpad, stride = self.geo[j]
                pk = self.pk.data_ptr() + 2 * self.pk_off[j] if r.has_pk else None
                n = L.fmri_apply_entry_fill(host, self.gs.data_ptr() + 4 * self.gs_off[j], wp, sp_, gp, pk, *spec_args(sp),
                                            r.ld, kpad if r.has_pk else 0, r.nslabs, stride, 1 if r.clear else 0,
                                            float(r.scale), 0, self.tiles)
                assert n == expected_apply_blocks(sp, r.case.apply), (r.case.name, n)
            else:
                flat_n = self.flat[-1 - j][1]
                n = L.fmri_apply_entry_fill(host, None, wp, sp_, gp, None, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 1, 0,
                                            0, 1.0, flat_n, self.tiles)
                assert n == (flat_n + APPLY_CHUNK - 1) // APPLY_CHUNK
            tab.append(host.raw)
            self.tiles += n
        self.ntab = len(tab)
        assert self.ntab > 64
        self.table = torch.frombuffer(bytearray(b"".join(tab)), dtype=torch.uint8).to(DEV)

    # ---- host-side inputs of one step ------------------------------------------------------------------------------------
    def make_slabs(self, seed, nan=False):
        """(host image of the packed-gradient buffer, float64 reference-layout gradient of every kind-0 / kind-1 tensor).
        Integer data |v| <= 1024 in every column, power-of-two scales: the gradients are exact.  The pad-channel columns
        (b in [B, Bp) of every tap), the columns behind the taps and the floats between two slabs hold such garbage too:
        none of it may be read into a gradient."""
        rs = np.random.RandomState(seed)
        gs = np.full(self.gs_n, SENT32, dtype=np.float32)
        gref = np.zeros(self.n)
        for j, r in enumerate(self.rows):
            rows, rows_pad, kpad, stride = self.geo[j]
            sp = r.case.spec
            nt, bp = sp.TH * sp.TW, pad8(sp.B)
            block = rs.randint(-1024, 1025, (r.nslabs, stride)).astype(np.float32)
            slabs = block[:, :rows * r.ld].reshape(r.nslabs, rows, r.ld)
            if nan:
                block[:] = np.nan
            else:
                gref[self.off[j]:self.off[j] + r.case.numel] = unpack_ref(slabs, sp, r.ld, r.scale, into=np.zeros(r.case.numel))
            gs[self.gs_off[j]:self.gs_off[j] + r.nslabs * stride] = block.ravel()
        return gs, gref

    def make_grad(self, seed):
        """Reference-layout gradient buffer: values of every size up to 4 (true gradient up to 1: some beyond the clamp) on
        every tensor and flat segment (garbage to the modes that store gradients there), sentinels in the gaps."""
        rs = np.random.RandomState(seed)
        g = (rs.standard_normal(self.n) * 10.0 ** rs.uniform(-5, 0.3, self.n)).astype(np.float32)
        g = np.clip(g, -4.0, 4.0)
        return np.where(self.covered, g, SENT32).astype(np.float32)

    def cleared(self, gs):
        """``gs`` after the ``clear`` pass: in every slab of every ``clear`` row, zeros in the columns the kernel sums
        (b < B of every tap) and, for kind 0, in the columns behind the taps up to ``ld`` (the weight-gradient kernels add
        there too: the narrow one keeps a bias gradient in the first of them).  The pad-channel columns b in [B, Bp) are
        NOT handed back: a weight-gradient GEMM only ever adds zeros there (the pad channels of its activations are zero),
        so the kernel leaves them alone -- the garbage put there here has to survive.  So do the floats between two slabs."""
        out = gs.copy()
        for j, r in enumerate(self.rows):
            if r.clear:
                rows, rows_pad, kpad, stride = self.geo[j]
                sp = r.case.spec
                nt, bp = sp.TH * sp.TW, pad8(sp.B)
                cols = np.arange(r.ld)
                zero = np.where(cols < nt * bp, cols % bp < sp.B, r.case.apply == 0)
                for z in range(r.nslabs):
                    o = self.gs_off[j] + z * stride
                    out[o:o + rows * r.ld].reshape(rows, r.ld)[:, zero] = 0.0
        return out

    def upload(self, w=None, sq=None, grad=None, gs=None, pk=None):
        for t, a in ((self.w, w), (self.sq, sq), (self.grad, grad), (self.gs, gs), (self.pk, pk)):
            if a is not None:
                t.copy_(_torch().from_numpy(a))

    def download(self):
        return {k: _host(t) for k, t in (("w", self.w), ("sq", self.sq), ("grad", self.grad), ("gs", self.gs),
                                         ("pk", self.pk))}

    def apply(self, mode, lr=0.0, flag=None, gated=0):
        self.lr.fill_(lr)
        if mode in (1, 3):
            _call("fmri_apply_batch", self.table.data_ptr(), self.ntab, self.tiles, mode, self.lr.data_ptr(), ALPHA, EPS, 1.0,
                  self.gdev.data_ptr(), CLAMP, _L().ptr(self.flags[flag]), gated)
        else:
            _call("fmri_apply_batch", self.table.data_ptr(), self.ntab, self.tiles, mode, None, 0.0, 0.0, 1.0, None, 0.0, None, 0)

    def separate(self, lr, from_slabs=True):
        """The launches the header promises the same bits as: fmri_unpack_grad onto zeros, fmri_rmsprop_dev,
        fmri_pack_weight, tensor by tensor (flat segments: fmri_rmsprop_dev on the gradient that is there)."""
        self.lr.fill_(lr)
        P = lambda t, o: t.data_ptr() + 4 * o
        for j, r in enumerate(self.rows):
            rows, rows_pad, kpad, stride = self.geo[j]
            o, n, sp = self.off[j], r.case.numel, r.case.spec
            if from_slabs:
                self.grad[o:o + n].zero_()
                _call("fmri_unpack_grad", P(self.gs, self.gs_off[j]), P(self.grad, o), *spec_args(sp), r.ld, float(r.scale), 1,
                      r.nslabs, stride)
            _call("fmri_rmsprop_dev", P(self.w, o), P(self.grad, o), P(self.sq, o), n, self.lr.data_ptr(), ALPHA, EPS, 1.0,
                  self.gdev.data_ptr(), CLAMP, None)
            if r.has_pk:
                _call("fmri_pack_weight", P(self.w, o), self.pk.data_ptr() + 2 * self.pk_off[j], *spec_args(sp), rows_pad, kpad)
        for o, n in self.flat:
            _call("fmri_rmsprop_dev", P(self.w, o), P(self.grad, o), P(self.sq, o), n, self.lr.data_ptr(), ALPHA, EPS, 1.0,
                  self.gdev.data_ptr(), CLAMP, None)

    def pk_of(self, w):
        """The fp16 copies a host image ``w`` of the weights casts to: sentinel outside the valid regions."""
        out = self.pk0.copy()
        for j, r in enumerate(self.rows):
            if r.has_pk:
                rows, rows_pad, kpad, _ = self.geo[j]
                o = self.off[j]
                ref = _f16(pack_ref(w[o:o + r.case.numel], r.case.spec, rows_pad, kpad)).ravel()
                seg = slice(self.pk_off[j], self.pk_off[j] + rows_pad * kpad)
                out[seg] = np.where(self.pk_valid[seg], ref, SENT16)
        return out


@functools.lru_cache(maxsize=None)
def _world(k):
    return _World(77)


def _check_update(case, W, got, w_ref, sq_ref, steps, pk_from):
    """w / sq against the float64 trajectory, the fp16 copies against the cast of the weights the launch wrote, and
    everything outside the tensors (gaps, guards, padding of the copies) untouched."""
    cov = W.covered
    _bounded(case, "w vs float64 RMSprop (atol 1e-7 + rtol 1e-6)", np.abs(got["w"].astype(np.float64) - w_ref)[cov],
             (1e-7 + 1e-6 * np.abs(w_ref))[cov])
    _bounded(case, f"sq vs float64 (8 * 2^-24 relative per step, {steps} steps)",
             np.abs(got["sq"].astype(np.float64) - sq_ref)[cov], (steps * 8 * U * np.abs(sq_ref))[cov])
    _exact(case, "w, sq outside the tensors (gaps, guards)",
           np.stack([np.where(cov, np.float32(0), got["w"]), np.where(cov, np.float32(0), got["sq"])]),
           np.stack([np.where(cov, np.float32(0), W.w0), np.where(cov, np.float32(0), W.sq0)]))
    _exact(case, "fp16 copies = RNE cast of the written w; padding, guards, rows without a copy", got["pk"], W.pk_of(pk_from))


def test_apply_batch_mode0_stores_the_mapped_slab_sums():
    """Mode 0: ``grad`` (garbage before) holds exactly scale * slab sum in the reference layout on every kind-0 / kind-1
    tensor -- stored, not added -- and is left alone on the flat segments and in the gaps; w, sq and the fp16 copies are
    unchanged; slabs with ``clear`` come back zero in every column a weight-gradient kernel adds into (``_World.cleared``:
    the summed columns and those behind the taps up to ``ld``), the others unchanged."""
    W = _world(0)
    gs, gref = W.make_slabs(3100)
    g0 = W.make_grad(3101)
    W.upload(w=W.w0, sq=W.sq0, grad=g0, gs=gs, pk=W.pk0)
    W.apply(0)
    got = W.download()
    case = f"C apply mode 0 ({W.ntab} rows, {W.tiles} blocks)"
    tensors = W.covered & ~W.is_flat
    want = np.where(tensors, gref.astype(np.float32), g0)
    assert (want.astype(np.float64)[tensors] == gref[tensors]).all(), "the reference is exact in fp32"
    _exact(case, "grad: tensors = mapped slab sums, flat segments / gaps / guards unchanged", got["grad"], want)
    _exact(case, "w, sq unchanged", np.stack([got["w"], got["sq"]]), np.stack([W.w0, W.sq0]))
    _exact(case, "fp16 copies unchanged", got["pk"], W.pk0)
    _exact(case, "packed gradients: clear rows zeroed (summed columns, columns behind the taps), the rest unchanged", got["gs"], W.cleared(gs))


def test_apply_batch_mode2_zeroes_only_the_flat_segments():
    """Mode 2 over the WHOLE table: the flat segments (1, 1023, 1025 and 3000 elements) of ``grad`` are zero, nothing else
    anywhere has changed."""
    W = _world(0)
    gs, _ = W.make_slabs(3200)
    g0 = W.make_grad(3201)
    W.upload(w=W.w0, sq=W.sq0, grad=g0, gs=gs, pk=W.pk0)
    W.apply(2)
    got = W.download()
    case = f"C apply mode 2 (flat segments {FLAT_LENGTHS})"
    assert [n for _, n in W.flat] == list(FLAT_LENGTHS)
    _exact(case, "grad: flat segments zero, the rest unchanged", got["grad"], np.where(W.is_flat, np.float32(0), g0))
    _exact(case, "w, sq unchanged", np.stack([got["w"], got["sq"]]), np.stack([W.w0, W.sq0]))
    _exact(case, "fp16 copies unchanged", got["pk"], W.pk0)
    _exact(case, "packed gradients unchanged", got["gs"], gs)


def test_apply_batch_mode1_three_steps_against_float64_and_the_separate_launches():
    """Mode 1, three steps with a device learning rate that changes every step, device gradient factor 4, clamp 0.5 (some
    true gradients beyond it): w and sq against the float64 trajectory, the fp16 copies against the cast of the written
    weights, cleared / untouched slabs, and after every step the same BITS as fmri_unpack_grad onto zeros +
    fmri_rmsprop_dev + fmri_pack_weight on a second copy of the buffers."""
    A, B = _world(0), _world(1)
    assert A is not B
    for X in (A, B):
        X.upload(w=X.w0, sq=X.sq0, pk=X.pk0)
    w_ref, sq_ref = A.w0.astype(np.float64), A.sq0.astype(np.float64)
    beyond = 0
    for step, lr in enumerate(LRS):
        gs, gref = A.make_slabs(3300 + step)
        g0 = A.make_grad(3310 + step)
        g_all = np.where(A.is_flat, g0.astype(np.float64), gref)
        beyond += int(np.count_nonzero(np.abs(g_all[A.covered]) / GDEV > CLAMP))
        with np.errstate(invalid="ignore"):                        # (the sentinels in the gaps: discarded below)
            nw, ns = rmsprop_ref(w_ref, sq_ref, g_all, lr, ALPHA, EPS, 1.0, GDEV, CLAMP)
        w_ref, sq_ref = np.where(A.covered, nw, w_ref), np.where(A.covered, ns, sq_ref)
        for X in (A, B):
            X.upload(grad=g0, gs=gs)
        A.apply(1, lr)
        B.separate(lr)
        a, b = A.download(), B.download()
        case = f"C apply mode 1 step {step + 1}"
        _check_update(case, A, a, w_ref, sq_ref, step + 1, a["w"])
        _exact(case, "grad untouched (the gradients never reach the reference layout)", a["grad"], g0)
        _exact(case, "packed gradients: clear rows zeroed (summed columns, columns behind the taps), the rest unchanged", a["gs"], A.cleared(gs))
        _exact(case, "w, sq = fmri_unpack_grad + fmri_rmsprop_dev (bits)", np.stack([a["w"], a["sq"]]),
               np.stack([b["w"], b["sq"]]))
        _exact(case, "fp16 copies = fmri_pack_weight of the separately updated w (valid regions: its generic route also "
               "zeroes the padding)", np.where(A.pk_valid, a["pk"], SENT16), np.where(A.pk_valid, b["pk"], SENT16))
    assert beyond > 100, "some true gradients beyond the clamp"
    print(f"[layout] C apply mode 1 | true gradients beyond the clamp over three steps = {beyond}", flush=True)


def test_apply_batch_mode3_reads_the_reference_layout_and_leaves_the_slabs_alone():
    """Mode 3: the same update from ``grad`` in the reference layout; the packed gradients hold NaN (read, they would reach
    w) and keep their bits -- ``clear`` rows included."""
    A, B = _world(0), _world(1)
    gs, _ = A.make_slabs(3400, nan=True)
    g0 = A.make_grad(3401)
    for X in (A, B):
        X.upload(w=X.w0, sq=X.sq0, grad=g0, gs=gs, pk=X.pk0)
    lr = LRS[0]
    with np.errstate(invalid="ignore"):                            # (the sentinels in the gaps: discarded below)
        w_ref, sq_ref = rmsprop_ref(A.w0, A.sq0, g0, lr, ALPHA, EPS, 1.0, GDEV, CLAMP)
    w_ref, sq_ref = np.where(A.covered, w_ref, A.w0), np.where(A.covered, sq_ref, A.sq0)
    assert np.count_nonzero(np.abs(g0[A.covered]) / GDEV > CLAMP) > 100
    A.apply(3, lr)
    B.separate(lr, from_slabs=False)
    a, b = A.download(), B.download()
    case = "C apply mode 3"
    _check_update(case, A, a, w_ref, sq_ref, 1, a["w"])
    _exact(case, "grad unchanged", a["grad"], g0)
    _exact(case, "packed gradients (NaN) not read, not cleared", a["gs"], gs)
    _exact(case, "w, sq = fmri_rmsprop_dev on the same gradient (bits)", np.stack([a["w"], a["sq"]]), np.stack([b["w"], b["sq"]]))
    _exact(case, "fp16 copies = fmri_pack_weight of the separately updated w (valid regions: its generic route also "
               "zeroes the padding)", np.where(A.pk_valid, a["pk"], SENT16), np.where(A.pk_valid, b["pk"], SENT16))


@pytest.mark.parametrize("mode", [1, 3])
def test_apply_batch_gate_matrix(mode):
    """flag in {NULL, 1, 0} x gated in {0, 1} (x clear, which alternates over the rows): a live launch gives the bits of the
    ungated one whatever ``gated`` says; with flag = 0 nothing in w, sq or the fp16 copies changes, and the ``clear`` pass
    over the packed gradients runs iff gated == 0 and the mode is 1 (never on a flat segment: ``grad`` keeps its bits)."""
    W = _world(0)
    gs, _ = W.make_slabs(3500 + mode)
    g0 = W.make_grad(3510 + mode)
    lr = LRS[2]
    live = None
    for flag in (None, 1, 0):
        for gated in (0, 1):
            W.upload(w=W.w0, sq=W.sq0, grad=g0, gs=gs, pk=W.pk0)
            W.apply(mode, lr, flag, gated)
            got = W.download()
            case = f"C gate mode {mode} flag {'NULL' if flag is None else flag} gated {gated}"
            clears = mode == 1 and (flag != 0 or gated == 0)
            _exact(case, "packed gradients " + ("cleared on the clear rows" if clears else "unchanged"), got["gs"],
                   W.cleared(gs) if clears else gs)
            _exact(case, "grad unchanged", got["grad"], g0)
            if flag == 0:
                _exact(case, "w, sq unchanged", np.stack([got["w"], got["sq"]]), np.stack([W.w0, W.sq0]))
                _exact(case, "fp16 copies unchanged", got["pk"], W.pk0)
            elif live is None:
                live = got
                assert np.count_nonzero(_bits(got["w"]) != _bits(W.w0)) > 0.3 * np.count_nonzero(W.covered), "the update ran"
                assert (got["pk"] != W.pk0).any()
            else:
                _exact(case, "w, sq = the ungated launch (bits)", np.stack([got["w"], got["sq"]]),
                       np.stack([live["w"], live["sq"]]))
                _exact(case, "fp16 copies = the ungated launch (bits)", got["pk"], live["pk"])


# =====================================================================================================================
# D. fmri_transpose_f16_batch, fmri_permute_chw
# =====================================================================================================================
# (rows R of the source = output channels, channels C of one tap, taps): per-tap slices of a forward copy
# [R][tap * Cip + ci] -> one block [ci][tap' * Cop + co]; R is no multiple of 8, C no multiple of 64, and every slice
# but the first has width < ld_src
TRANSPOSE_SOURCES = [(13, 5, 25), (70, 72, 25), (33, 130, 9), (13, 5, 9)]
TRANSPOSE_DENSE = [(70, 130), (5, 40)]                 # whole-matrix rows (a dense layer's second orientation)


def test_transpose_f16_batch_per_tap_slices():
    """More than 64 table rows: every tap of three forward copies as its own 2-D transpose (source slice narrower than
    ld_src, taps written in reverse order) plus two whole matrices.  Destination = numpy's transpose bit for bit; the
    columns from R up to R rounded up to 8 are written as zeros (16-byte stores: the header asks for ld_dst >= that),
    everything else of the destination keeps its sentinel."""
    torch = _torch()
    L = _L().load()
    nbytes = L.fmri_transpose_entry_bytes()
    rs = np.random.RandomState(4000)
    tab, tiles, keep, checks = [], 0, [], []
    jobs = [(R, C, T) for R, C, T in TRANSPOSE_SOURCES] + [(R, C, 1) for R, C in TRANSPOSE_DENSE]
    for R, C, T in jobs:
        assert R % 8 and C % 64
        cip, cop = pad8(C), pad8(R)
        lds, ldd = (T * cip + 63) // 64 * 64, (T * cop + 63) // 64 * 64
        rbuf = (R + 31) // 32 * 32
        src = np.zeros((rbuf, lds), dtype=np.float16)                     # rows from R on and columns behind the taps: zero
        src[:R, :T * cip].reshape(R, T, cip)[:, :, :C] = rs.standard_normal((R, T, C)).astype(np.float16)
        want = np.full((GUARD + cip * ldd + GUARD,), SENT16, dtype=np.float16)
        body = want[GUARD:-GUARD].reshape(cip, ldd)
        s_dev = _dev(src)
        d_dev = _dev(want)                                                  # (all sentinel so far)
        for t in range(T):
            t2 = T - 1 - t
            host = ctypes.create_string_buffer(nbytes)
            n = L.fmri_transpose_entry_fill(host, s_dev.data_ptr() + 2 * t * cip, d_dev.data_ptr() + 2 * (GUARD + t2 * cop), R, C,
                                            rbuf, lds - t * cip, lds, ldd, tiles)
            assert n == ((R + 63) // 64) * ((C + 63) // 64), (R, C, t, n)
            assert T == 1 or t == 0 or lds - t * cip < lds
            tab.append(host.raw)
            tiles += n
            body[:C, t2 * cop:t2 * cop + cop] = 0
            body[:C, t2 * cop:t2 * cop + R] = src[:R, t * cip:t * cip + C].T
        keep.append(s_dev)
        checks.append(((R, C, T), d_dev, want))
    assert len(tab) > 64
    table = torch.frombuffer(bytearray(b"".join(tab)), dtype=torch.uint8).to(DEV)
    _call("fmri_transpose_f16_batch", table.data_ptr(), len(tab), tiles)
    for (R, C, T), d_dev, want in checks:
        _exact(f"D transpose batch R={R} C={C} taps={T} ({len(tab)} rows in the table)",
               "transposed slices, zero fill to 8, sentinel padding and guards", _host(d_dev), want)


@pytest.mark.parametrize("C,HW", [(24, 100), (5, 7)])
def test_permute_chw_both_directions(C, HW):
    """(C, HW) <-> (HW, C) order of a per-feature vector, with a power-of-two scale and with ``accumulate``: exact."""
    rs = np.random.RandomState(4100 + C)
    n = C * HW
    guard = np.full(GUARD, SENT32, dtype=np.float32)
    src = rs.standard_normal(n).astype(np.float32)
    before = rs.randint(-64, 65, n).astype(np.float32)
    case = f"D permute_chw C={C} HW={HW}"
    for to_engine, accumulate, scale in ((1, 0, 1.0), (1, 0, 0.25), (0, 0, 1.0), (0, 0, 0.25), (0, 1, 0.25), (0, 1, 1.0)):
        s = src if not accumulate else rs.randint(-64, 65, n).astype(np.float32)      # (integers: the sum is exact)
        dst, s_dev = _dev(np.concatenate([guard, before, guard])), _dev(s)
        _call("fmri_permute_chw", s_dev.data_ptr(), dst.data_ptr() + 4 * GUARD, C, HW, to_engine, scale, accumulate)
        s64 = s.astype(np.float64) * scale
        if to_engine:
            ref = s64.reshape(C, HW).T.ravel()                             # dst[hw * C + c] = src[c * HW + hw]
        else:
            ref = s64.reshape(HW, C).T.ravel() + (before if accumulate else 0.0)
        want = np.concatenate([guard, ref.astype(np.float32), guard])
        assert (want[GUARD:-GUARD].astype(np.float64) == ref).all()
        _exact(case, f"to_engine {to_engine} accumulate {accumulate} scale {scale}", _host(dst), want)
