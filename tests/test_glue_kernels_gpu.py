"""The small kernels every step runs between its contractions, each by itself and over EVERY element against the float64
references of tests/glue_oracle.py (no sampling, no skipped case):

  A. fmri_nchw_to_nhwc / fmri_nhwc_to_nchw / fmri_rows_f32_to_f16 / fmri_rows_f16_to_f32: bitwise, with fp16 subnormals, rounding
     ties, +-65504 and its neighbours, overflowing values, +-0, inf and NaN among the data; padded lanes exactly zero; a canary
     behind every destination; one case per kernel past the launcher's 4096 x 256 item cap (a second grid-stride sweep);
  B. fmri_act_bwd: none / ReLU / tanh, without colsum, with colsum, with the dbias fold (dbias_n = 3 < C, gscale != 1, a non-zero
     dbias on entry), at the edges of row_geometry;
  C. fmri_colsum_acc (fp16 / fp32, strided as ConvLayer._wgrad reads the narrow slabs' spare column), fmri_colsum_rows (both
     halves of [sum x | sum x^2]) and the route switch of ops.colsum_acc at 2048 rows;
  D. fmri_bn_apply at the edges of stream_geometry, with zero, negative and overflowing channel scales;
  E. fmri_ingest_u8: every shift / flip combination on five image shapes, and a batch past the 4096-block cap;
  F. fmri_rows_absmax, fmri_sumsq / fmri_renorm (fp32), fmri_axpby_f16 and ops.axpby(y=None).

Exact-grid inputs must come out EQUAL to the float64 result in every bit; real-valued inputs are held to bounds derived from
the number formats (see the oracle's docstring).  tests/test_glue_oracle_host.py shows on the CPU that these checks accept
float32 arithmetic and reject eleven wrong kernels.  Every check prints one ``[glue] <case> | <quantity> | ...`` line;
profiles/glue_kernels_parity.md records those of one GPU run.

Reduction modes: fmri_act_bwd, fmri_colsum_rows (reduce_launch in csrc/norm.hip: per-block partials and a fold, no atomics) and
fmri_colsum_acc never consult the deterministic switch, and rows_absmax meets in an integer atomicMax: their results cannot
depend on the mode.  fmri_sumsq does (one block instead of up to 256 meeting in a float atomicAdd) and runs under both.
"""
import numpy as np
import pytest
import torch

import glue_oracle as GO
from glue_oracle import F16, F32

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S16, S32 = 0x5A5A, 0x5A5A5A5A            # sentinel bit patterns (fp16 207.25, fp32 1.5e16)
TAIL = 64                                # canary elements behind every destination


def _say(case, results):
    for ln in GO.lines(case, results):
        print(ln, flush=True)
    assert GO.passed(results), (case, results)


def _sent(n, dtype):
    if dtype == torch.float16:
        return torch.full((n + TAIL,), S16, dtype=torch.int16, device=DEV).view(torch.float16)
    return torch.full((n + TAIL,), S32, dtype=torch.int32, device=DEV).view(torch.float32)


def _take(buf, n, what="destination"):
    """The first n elements of a sentinel buffer as numpy, after checking that nothing behind them was written."""
    torch.cuda.synchronize()
    tail = buf[n:]
    ok = (tail.view(torch.int16) == S16).all() if buf.dtype == torch.float16 else (tail.view(torch.int32) == S32).all()
    assert bool(ok), f"{what}: written behind its end"
    return buf[:n].cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(params=[False, True], ids=["default", "deterministic"])
def reduction_mode(request):
    from fmri_hip import ops
    was = ops.set_deterministic(request.param)
    try:
        yield request.param
    finally:
        ops.set_deterministic(was)


# =====================================================================================================================
# A. conversions
# =====================================================================================================================
def _nchw_to_nhwc(x):
    from fmri_hip import lib
    N, C, HW = x.shape
    Cp = GO.pad8(C)
    xd, buf = _dev(x), _sent(N * HW * Cp, torch.float16)
    lib.call("fmri_nchw_to_nhwc", lib.ptr(xd), lib.ptr(buf), N, C, HW, Cp)
    return _take(buf, N * HW * Cp).reshape(N, HW, Cp)


def _nhwc_to_nchw(h, C, scale):
    from fmri_hip import lib
    N, HW, Cp = h.shape
    hd, buf = _dev(h), _sent(N * C * HW, torch.float32)
    lib.call("fmri_nhwc_to_nchw", lib.ptr(hd), lib.ptr(buf), N, C, HW, Cp, scale)
    return _take(buf, N * C * HW).reshape(N, C, HW)


def _rows_f32_to_f16(x, scale):
    from fmri_hip import lib
    M, C = x.shape
    Cp = GO.pad8(C)
    xd, buf = _dev(x), _sent(M * Cp, torch.float16)
    lib.call("fmri_rows_f32_to_f16", lib.ptr(xd), lib.ptr(buf), M, C, Cp, scale)
    return _take(buf, M * Cp).reshape(M, Cp)


def _rows_f16_to_f32(h, C, scale):
    from fmri_hip import lib
    M, Cp = h.shape
    hd, buf = _dev(h), _sent(M * C, torch.float32)
    lib.call("fmri_rows_f16_to_f32", lib.ptr(hd), lib.ptr(buf), M, C, Cp, scale)
    return _take(buf, M * C).reshape(M, C)


@pytest.mark.parametrize("C", (1, 3, 8, 9, 20, 64))
def test_image_conversions(C):
    """fmri_nchw_to_nhwc (its ABI has no scale: the cast alone) and fmri_nhwc_to_nchw at scale 1, 0.5 and 1/3, every element
    bitwise.  The cast of a value past fp16's range is a plain round-to-nearest conversion: from 65520 on it gives inf, as
    numpy's astype(float16) does (65519.99 -> 65504); both are among the data."""
    for i, (N, Cc, HW) in enumerate(GO.IMG_SHAPES):
        if Cc != C:
            continue
        Cp = GO.pad8(C)
        x = GO.conv_values(N * C * HW, i, as16=False).reshape(N, C, HW)
        _say(f"A nchw_to_nhwc N={N} C={C} HW={HW}", GO.cmp_conv(_nchw_to_nhwc(x), GO.nchw_to_nhwc_ref(x, Cp), C))
        h = GO.conv_values(N * HW * Cp, i + 100, as16=True).reshape(N, HW, Cp)
        for s in GO.SCALES:
            _say(f"A nhwc_to_nchw N={N} C={C} HW={HW} scale={s:.4g}", GO.cmp_conv(_nhwc_to_nchw(h, C, s), GO.nhwc_to_nchw_ref(h, C, s)))


@pytest.mark.parametrize("C", (1, 7, 8, 12, 3620))
def test_row_conversions(C):
    for i, (M, Cc) in enumerate(GO.ROW_SHAPES):
        if Cc != C:
            continue
        Cp = GO.pad8(C)
        x = GO.conv_values(M * C, i + 200, as16=False).reshape(M, C)
        h = GO.conv_values(M * Cp, i + 300, as16=True).reshape(M, Cp)
        for s in GO.SCALES:
            _say(f"A rows_f32_to_f16 M={M} C={C} scale={s:.4g}", GO.cmp_conv(_rows_f32_to_f16(x, s), GO.rows_f32_to_f16_ref(x, Cp, s), C))
            _say(f"A rows_f16_to_f32 M={M} C={C} scale={s:.4g}", GO.cmp_conv(_rows_f16_to_f32(h, C, s), GO.rows_f16_to_f32_ref(h, C, s)))


def test_conversions_past_the_block_cap():
    """nblocks() of csrc/layout.hip caps the grid at 4096 blocks of 256 items: the smallest shapes past it, so that the
    second sweep of each grid-stride loop runs (every element compared, the last ones are those only it reaches)."""
    N, C, HW = GO.IMG_CAP
    Cp = GO.pad8(C)
    assert N * HW * (Cp // 8) > 4096 * 256 and N * C * HW > 4096 * 256
    x = GO.conv_values(N * C * HW, 901, as16=False).reshape(N, C, HW)
    _say(f"A second sweep nchw_to_nhwc N={N} C={C} HW={HW}", GO.cmp_conv(_nchw_to_nhwc(x), GO.nchw_to_nhwc_ref(x, Cp), C))
    h = GO.conv_values(N * HW * Cp, 902, as16=True).reshape(N, HW, Cp)
    _say(f"A second sweep nhwc_to_nchw N={N} C={C} HW={HW} scale=1/3", GO.cmp_conv(_nhwc_to_nchw(h, C, GO.THIRD), GO.nhwc_to_nchw_ref(h, C, GO.THIRD)))
    M, C = GO.ROW_CAP
    Cp = GO.pad8(C)
    assert M * Cp > 4096 * 256 and M * C > 4096 * 256
    x = GO.conv_values(M * C, 903, as16=False).reshape(M, C)
    _say(f"A second sweep rows_f32_to_f16 M={M} C={C} scale=1/3", GO.cmp_conv(_rows_f32_to_f16(x, GO.THIRD), GO.rows_f32_to_f16_ref(x, Cp, GO.THIRD), C))
    h = GO.conv_values(M * Cp, 904, as16=True).reshape(M, Cp)
    _say(f"A second sweep rows_f16_to_f32 M={M} C={C} scale=0.5", GO.cmp_conv(_rows_f16_to_f32(h, C, 0.5), GO.rows_f16_to_f32_ref(h, C, 0.5)))


def test_conversion_wrappers():
    """The ops wrappers the steps call: images_to_nhwc(out=buf[:B]) leaves the rows of ``buf`` behind B untouched;
    nhwc_to_images and rows_to_f16 give the same bits as the references."""
    from fmri_hip import ops
    B, H, W = 3, 5, 7
    x = GO.conv_values(B * 3 * H * W, 911, as16=False).reshape(B, 3, H * W)
    buf = torch.full((B + 2, H, W, 8), S16, dtype=torch.int16, device=DEV).view(torch.float16)
    out = ops.images_to_nhwc(_dev(x).reshape(B, 3, H, W), out=buf[:B])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr() and bool((buf[B:].view(torch.int16) == S16).all()), "rows behind B"
    _say("A images_to_nhwc(out=buf[:3]) 5x7", GO.cmp_conv(buf[:B].cpu().numpy().reshape(B, H * W, 8), GO.nchw_to_nhwc_ref(x, 8), 3))
    h = GO.conv_values(B * H * W * 8, 912, as16=True).reshape(B, H * W, 8)
    got = ops.nhwc_to_images(_dev(h).reshape(B, H, W, 8), 3, 0.5).cpu().numpy().reshape(B, 3, H * W)
    _say("A nhwc_to_images scale=0.5", GO.cmp_conv(got, GO.nhwc_to_nchw_ref(h, 3, 0.5)))
    r = GO.conv_values(5 * 12, 913, as16=False).reshape(5, 12)
    _say("A rows_to_f16 scale=1/3", GO.cmp_conv(ops.rows_to_f16(_dev(r), GO.THIRD).cpu().numpy(), GO.rows_f32_to_f16_ref(r, 16, GO.THIRD), 12))


# =====================================================================================================================
# B. fmri_act_bwd
# =====================================================================================================================
def _act_bwd(y, dy, act, variant, prior=None, n=0, gscale=1.0):
    """variant 0: no colsum; 1: colsum; 2: colsum and dbias.  Returns dpre16, colsum[:C] (or None), dbias buffer (or None)."""
    from fmri_hip import lib
    P = lib.ptr
    M, C = y.shape
    yd, dyd = _dev(y), _dev(dy)
    dpre = _sent(M * C, torch.float16)
    if variant == 0:
        lib.call("fmri_act_bwd", P(yd), P(dyd), P(dpre), M, C, act, None, None, 0, None, 0, 0.0)
        return _take(dpre, M * C, "dpre").reshape(M, C), None, None
    nws = lib.load().fmri_bn_ws_floats(M, C)
    ws = torch.empty(nws, dtype=torch.float32, device=DEV)
    cs = _sent(2 * C, torch.float32)
    db = None
    if variant == 2:
        db = _sent(C, torch.float32)
        db[:C] = _dev(prior)
    lib.call("fmri_act_bwd", P(yd), P(dyd), P(dpre), M, C, act, P(cs), P(ws), nws, P(db), n if db is not None else 0, gscale)
    return (_take(dpre, M * C, "dpre").reshape(M, C), _take(cs, 2 * C, "colsum")[:C],
            _take(db, C, "dbias") if db is not None else None)


@pytest.mark.parametrize("act", (GO.ACT_NONE, GO.ACT_RELU, GO.ACT_TANH), ids=("none", "relu", "tanh"))
@pytest.mark.parametrize("C", GO.ACT_C)
def test_act_bwd(C, act):
    """dpre: ReLU / none bitwise (dy where y > 0 -- +-0 and a subnormal y among the data -- else +0), tanh bitwise on the grid
    and inside 2 roundings + the fp16 store on real inputs.  colsum (the first C floats) and dbias[:3] += gscale * colsum:
    bitwise on the grid, the sum bound on real inputs; dbias behind dbias_n keeps its entry value; dpre is the same whichever
    of colsum / dbias is NULL."""
    for M in GO.act_rows(C):
        for fam in ("grid", "real"):
            y, dy = GO.act_inputs(M, C, act, fam, 1000 * act + M % 997 + C)
            gs = 0.5 if fam == "grid" else GO.THIRD
            prior = GO.colsum_prior(C, fam, M + C)
            case = f"B act_bwd {GO.ACT_NAME[act]} {fam} M={M} C={C}"
            d0, _, _ = _act_bwd(y, dy, act, 0)
            _say(case + " no colsum", GO.cmp_act(y, dy, act, fam, d0))
            d1, s1, _ = _act_bwd(y, dy, act, 1)
            _say(case + " colsum", GO.cmp_act(y, dy, act, fam, d1, s1))
            d2, s2, db = _act_bwd(y, dy, act, 2, prior, 3, gs)
            _say(case + f" colsum+dbias[:3] gscale={gs:.3g}", GO.cmp_act(y, dy, act, fam, d2, s2, (db, 3), prior, gs))
            assert GO.mismatches(d0, d1) == 0 and GO.mismatches(d0, d2) == 0 and GO.mismatches(s1, s2) == 0, case


@pytest.mark.parametrize("fam", ("grid", "real"))
@pytest.mark.parametrize("act", (GO.ACT_NONE, GO.ACT_RELU, GO.ACT_TANH), ids=("none", "relu", "tanh"))
def test_act_bwd_decoder_output_rows(act, fam):
    """2^20 rows of 8 channels (the B = 256 decoder output, 256 block rows): dpre, colsum and dbias[:3] of one launch; on
    the grid a single dropped, doubled or misplaced row of the 2^20 changes a bit of the sums."""
    M, C = GO.BIG
    y, dy = GO.act_inputs(M, C, act, fam, 1000 * act + M % 997 + C)
    gs = 0.5 if fam == "grid" else GO.THIRD
    prior = GO.colsum_prior(C, fam, M + C)
    d2, s2, db = _act_bwd(y, dy, act, 2, prior, 3, gs)
    _say(f"B act_bwd {GO.ACT_NAME[act]} {fam} M={M} C={C} colsum+dbias[:3] gscale={gs:.3g}",
         GO.cmp_act(y, dy, act, fam, d2, s2, (db, 3), prior, gs))
    d0, _, _ = _act_bwd(y, dy, act, 0)
    assert GO.mismatches(d0, d2) == 0, "dpre depends on colsum being NULL"


def test_act_backward_wrapper():
    """ops.act_backward as DecoderNet calls it (tanh, colsum, the conv bias gradient's 3 of 8 columns)."""
    from fmri_hip import ops
    M, C = 1025, 8
    for fam, gs in (("grid", 0.5), ("real", GO.THIRD)):
        y, dy = GO.act_inputs(M, C, GO.ACT_TANH, fam, 77)
        prior = GO.colsum_prior(3, fam, 5)
        cs = torch.zeros(2 * C, dtype=torch.float32, device=DEV)
        db = _dev(prior)
        out = ops.act_backward(_dev(y), _dev(dy), ops.ACT_TANH, colsum=cs, dbias=db, dbias_scale=gs)
        torch.cuda.synchronize()
        _say(f"B ops.act_backward tanh {fam} M={M} C={C}",
             GO.cmp_act(y, dy, GO.ACT_TANH, fam, out.cpu().numpy(), cs[:C].cpu().numpy(), (db.cpu().numpy(), 3), prior, gs))


# =====================================================================================================================
# C. column sums
# =====================================================================================================================
@pytest.mark.parametrize("f16", (True, False), ids=("f16", "f32"))
def test_colsum_acc(f16):
    """dst[c] += scale * sum_m src[m * ld_row + c * ld_col]: rows of ld_row = C + 3 elements (the three behind C hold junk), a
    non-zero dst on entry, three entries of dst behind C untouched."""
    from fmri_hip import lib
    rs = np.random.RandomState(4)
    for C in GO.CS_C:
        for M in GO.CS_M:
            for fam, scale in (("grid", 0.5), ("real", GO.THIRD)):
                src = GO.colsum_src(M, C, fam, f16, M * 31 + C)
                wide = (rs.randn(M, C + 3) * 100).astype(src.dtype)
                wide[:, :C] = src
                prior = GO.colsum_prior(C + 3, fam, M + C)
                dst = _sent(C + 3, torch.float32)
                dst[:C + 3] = _dev(prior)
                wd = _dev(wide)
                lib.call("fmri_colsum_acc", lib.ptr(wd), 1 if f16 else 0, M, C, C + 3, 1, scale, lib.ptr(dst))
                _say(f"C colsum_acc {fam} {'f16' if f16 else 'f32'} M={M} C={C} scale={scale:.3g}",
                     GO.cmp_colsum(src, scale, prior, C, fam, _take(dst, C + 3, "dst")))


@pytest.mark.parametrize("f16", (True, False), ids=("f16", "f32"))
def test_colsum_acc_strided(f16):
    """The form ConvLayer._wgrad uses for the narrow weight-gradient slabs' spare column: slabs [M][A][ldo], the sum over the
    slabs of element (c, k) -- ld_row = A * ldo > C * ld_col, ld_col = ldo, the source pointer k elements into the buffer."""
    from fmri_hip import lib
    rs = np.random.RandomState(5)
    ldo, k = 24, 17
    for C in (5, 9):
        A = C + 2
        for M in (1, 31, 33):
            for fam, scale in (("grid", 0.5), ("real", GO.THIRD)):
                src = GO.colsum_src(M, C, fam, f16, M * 37 + C)
                slabs = (rs.randn(M, A, ldo) * 100).astype(src.dtype)
                slabs[:, :C, k] = src
                prior = GO.colsum_prior(C + 3, fam, M + C)
                dst = _sent(C + 3, torch.float32)
                dst[:C + 3] = _dev(prior)
                sd = _dev(slabs)
                lib.call("fmri_colsum_acc", lib.ptr(sd[0, 0, k:]), 1 if f16 else 0, M, C, A * ldo, ldo, scale, lib.ptr(dst))
                _say(f"C colsum_acc strided {fam} {'f16' if f16 else 'f32'} M={M} C={C} ld_row={A * ldo} ld_col={ldo}",
                     GO.cmp_colsum(src, scale, prior, C, fam, _take(dst, C + 3, "dst")))


@pytest.mark.parametrize("fam,gs", (("grid", 0.5), ("real", GO.THIRD)), ids=("grid", "real"))
@pytest.mark.parametrize("M,C", GO.CSR_SHAPES)
def test_colsum_rows(M, C, fam, gs):
    """sums2C = [sum x | sum x^2], both halves, and dbias[:n] += gscale * sum x for n = C and n = 3."""
    from fmri_hip import lib
    P = lib.ptr
    nws = lib.load().fmri_bn_ws_floats(M, C)
    x = GO.colsum_src(M, C, fam, True, M % 1009 + C)
    xd = _dev(x)
    for n in (C, 3):
        prior = GO.colsum_prior(C, fam, M % 1009 + n)
        ws = torch.empty(nws, dtype=torch.float32, device=DEV)
        sums, db = _sent(2 * C, torch.float32), _sent(C, torch.float32)
        db[:C] = _dev(prior)
        lib.call("fmri_colsum_rows", P(xd), M, C, P(sums), P(ws), nws, P(db), n, gs)
        _say(f"C colsum_rows {fam} M={M} C={C} dbias_n={n}",
             GO.cmp_colsum_rows(x, fam, _take(sums, 2 * C, "sums").reshape(2, C), _take(db, C, "dbias"), prior, n, gs))


class _Spy:
    """Records (entry point, arguments) of every library call made inside the ``with`` block (as
    tests/test_fullbatch_ops_gpu.py does)."""

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


def test_colsum_route_switch():
    """ops.colsum_acc sends fewer than 2048 contiguous fp16 rows to fmri_colsum_acc and 2048 or more to fmri_colsum_rows;
    on exact-grid inputs both routes give the float64 sums bit for bit (so the same bits as each other)."""
    from fmri_hip import ops
    C, n = 24, 20
    for M, route in ((2047, "fmri_colsum_acc"), (2048, "fmri_colsum_rows")):
        x = GO.colsum_src(M, C, "grid", True, M)
        prior = GO.colsum_prior(C, "grid", M)
        dst = _dev(prior)
        with _Spy() as spy:
            ops.colsum_acc(_dev(x), M, n, C, 1, 0.5, dst)
        torch.cuda.synchronize()
        assert spy.names() == [route], (M, spy.names())
        print(f"[glue] C ops.colsum_acc M={M} | route | {route}", flush=True)
        _say(f"C ops.colsum_acc grid M={M} C={C} n={n} via {route}", GO.cmp_colsum(x[:, :n], 0.5, prior, n, "grid", dst.cpu().numpy()))


# =====================================================================================================================
# D. fmri_bn_apply
# =====================================================================================================================
@pytest.mark.parametrize("C", GO.BN_C)
def test_bn_apply(C):
    """y = relu?(x scale[c] + shift[c]) at 1, 7, 8 RY +- 1 rows (and 2^20 at C = 8).  bn_stream_kernel<0> stores with a plain
    cast -- it does not saturate: channels whose scale carries the result past fp16's range must come out as +-inf (0 under
    the ReLU for the negative ones), exactly as numpy's astype(float16) gives."""
    from fmri_hip import lib
    P = lib.ptr
    for M in GO.bn_rows(C):
        x, a, b = GO.bn_inputs(M, C, M % 1013 + C)
        xd, ad, bd = _dev(x), _dev(a), _dev(b)
        for relu in (0, 1):
            y = _sent(M * C, torch.float16)
            lib.call("fmri_bn_apply", P(xd), P(y), M, C, P(ad), P(bd), relu)
            _say(f"D bn_apply M={M} C={C} relu={relu}", GO.cmp_bn(x, a, b, relu, _take(y, M * C, "y").reshape(M, C)))


@pytest.mark.parametrize("relu", (0, 1))
def test_bn_apply_decoder_output_rows(relu):
    """2^20 rows of 8 channels: stream_geometry's row cap (2048 block rows of 256 lanes, two trips of the x4 unrolled loop)."""
    from fmri_hip import lib
    M, C = GO.BIG
    x, a, b = GO.bn_inputs(M, C, M % 1013 + C)
    xd, ad, bd, y = _dev(x), _dev(a), _dev(b), _sent(M * C, torch.float16)
    lib.call("fmri_bn_apply", lib.ptr(xd), lib.ptr(y), M, C, lib.ptr(ad), lib.ptr(bd), relu)
    _say(f"D bn_apply M={M} C={C} relu={relu}", GO.cmp_bn(x, a, b, relu, _take(y, M * C, "y").reshape(M, C)))


# =====================================================================================================================
# E. fmri_ingest_u8
# =====================================================================================================================
def _ingest(img, fl, sh, mean, std, want16, want32):
    from fmri_hip import lib
    P = lib.ptr
    N, H, W, C = img.shape
    o16 = _sent(N * H * W * 8, torch.float16) if want16 else None
    o32 = _sent(N * 3 * H * W, torch.float32) if want32 else None
    imd, fld, shd = _dev(img), _dev(fl), _dev(sh)          # (named: a temporary's block would be handed to the next one)
    lib.call("fmri_ingest_u8", P(imd), N, H, W, C, P(fld), P(shd), *[float(v) for v in mean],
             *[float(v) for v in std], P(o16), P(o32))
    return (_take(o16, N * H * W * 8, "dst16").reshape(N, H, W, 8) if want16 else None,
            _take(o32, N * 3 * H * W, "dst32").reshape(N, 3, H, W) if want32 else None)


@pytest.mark.parametrize("C", (1, 3))
@pytest.mark.parametrize("H,W", GO.INGEST_HW, ids=[f"{h}x{w}" for h, w in GO.INGEST_HW])
def test_ingest(H, W, C):
    """162 images per launch: every (row, column) shift pair of {0, +-1, +-(n-1), +-n, +-(n+3)}, each unflipped and flipped (no
    image is left-right symmetric, so flip-then-shift and shift-then-flip give different pictures wherever the column shift
    is not 0), three sets of per-channel statistics, fp16 only / fp32 only / both.  The reference takes its geometry from
    oracle/ingest_oracle.py and evaluates (p / 255 - m) / std in float64."""
    fl, sh = GO.ingest_shifts(H, W)
    img = GO.ingest_images(len(fl), H, W, C, H * 10 + W + C)
    pix = GO.ingest_pixels(img, fl, sh)
    for mean, std in GO.INGEST_STATS:
        case = f"E ingest {H}x{W} C={C} mean={mean} std={std}"
        o16, o32 = _ingest(img, fl, sh, mean, std, True, True)
        _say(case + " both", GO.cmp_ingest(pix, mean, std, o16, o32))
        a16, none32 = _ingest(img, fl, sh, mean, std, True, False)
        none16, b32 = _ingest(img, fl, sh, mean, std, False, True)
        _say(case + " want16 only", GO.cmp_ingest(pix, mean, std, a16, None))
        _say(case + " want32 only", GO.cmp_ingest(pix, mean, std, None, b32))
        assert GO.mismatches(a16, o16) == 0 and GO.mismatches(b32, o32) == 0, case


def test_ingest_past_the_block_cap():
    """65 images of 128 x 128: 1 064 960 pixels against 4096 blocks x 256 threads, so image 64 -- all of it -- is written by
    the second sweep of the grid-stride loop only.  Every image has its own flip and shift; every pixel of every image is
    compared."""
    from fmri_hip import ops
    N, H, W = GO.INGEST_CAP
    assert (N - 1) * H * W >= 4096 * 256
    img = GO.ingest_images(N, H, W, 3, 41)
    fl = (np.arange(N) % 2).astype(np.int32)
    sh = np.stack([(np.arange(N) * 5) % 23 - 11, (np.arange(N) * 7) % 19 - 9], 1).astype(np.int32)
    assert len({(int(f), int(a), int(b)) for f, (a, b) in zip(fl, sh)}) == N
    mean, std = GO.INGEST_STATS[1]
    o16, o32 = ops.ingest_u8(_dev(img), mean=mean, std=std, flip=_dev(fl), shift=_dev(sh), want16=True, want32=True)
    torch.cuda.synchronize()
    o16, o32 = o16.cpu().numpy(), o32.cpu().numpy()
    pix = GO.ingest_pixels(img, fl, sh)
    _say(f"E second sweep ingest {N}x{H}x{W} all images", GO.cmp_ingest(pix, mean, std, o16, o32))
    _say(f"E second sweep ingest {N}x{H}x{W} image 64 alone", GO.cmp_ingest(pix[64:], mean, std, o16[64:], o32[64:]))


# =====================================================================================================================
# F. scalars and mixing
# =====================================================================================================================
@pytest.mark.parametrize("n", GO.ABSMAX_N)
def test_rows_absmax(n):
    """*zmax = max(*zmax, max |x|), bitwise.  The kernel folds with fmaxf, which returns its other operand when one is a NaN:
    NaNs among the values are SKIPPED, the result is the largest |x| of the rest (pinned here; the ranged latent path
    relies on it, csrc/loss.hip).  -0 counts as 0, an inf wins, the maximum may sit in the last element (n = 131 077 is past
    the 256-block cap: that element is reached by the third sweep), and a larger value already in *zmax stays."""
    from fmri_hip import lib
    rs = np.random.RandomState(n)
    base = rs.randn(n).astype(F32)
    variants = {"plain": base.copy(), "max last": base.copy(), "with NaN": base.copy(), "with inf": base.copy(),
                "all -0": np.full(n, -0.0, F32), "all NaN": np.full(n, np.nan, F32)}
    variants["max last"][-1] = -77.5
    variants["with NaN"][::3] = np.nan
    variants["with NaN"][-1] = 55.0
    variants["with inf"][n // 2] = -np.inf
    for name, x in variants.items():
        for prior in (0.0, 60.0):
            z = _sent(1, torch.float32)
            z[:1] = prior
            xd = _dev(x)
            lib.call("fmri_rows_absmax", lib.ptr(xd), n, lib.ptr(z))
            _say(f"F rows_absmax n={n} {name} prior={prior}", [GO.bits("zmax", _take(z, 1, "zmax"), GO.absmax_ref(x, prior))])


@pytest.mark.parametrize("n", (1, 255, 257, 70000))
def test_sumsq_exact(n, reduction_mode):
    """*acc += sum x^2 on the grid (x = k/8, |k| <= 8), onto a non-zero accumulator: bitwise in both reduction modes (n = 70 000
    is past the 256-block cap of the default mode; the deterministic mode sweeps everything with one block)."""
    from fmri_hip import lib
    x = GO.sumsq_inputs(n, n)
    acc = _sent(1, torch.float32)
    acc[:1] = 3.25
    xd = _dev(x)
    lib.call("fmri_sumsq", lib.ptr(xd), n, lib.ptr(acc))
    _say(f"F sumsq grid n={n} {'deterministic' if reduction_mode else 'default'}", GO.cmp_sumsq(x, 3.25, _take(acc, 1, "acc")))


def test_renorm():
    """out16 = x * f * scale, f = 1 / max(sqrt(sumsq / count), 1e-20); *factor_out = *factor_in * f (1 * f without factor_in);
    the factor chained through two launches; the 1e-20 floor on an all-zero input (f = 1e20, the rows stay +0)."""
    from fmri_hip import lib
    P = lib.ptr
    rs = np.random.RandomState(8)
    for n in (1, 257, 70000):
        x = (rs.randn(n) * 3).astype(F32)
        ss = np.array([np.sum(GO.f64(x) ** 2)], F32)
        cnt, scale = 7.0, 0.25
        xd, sd = _dev(x), _dev(ss)
        out, f1, f2 = _sent(n, torch.float16), _sent(1, torch.float32), _sent(1, torch.float32)
        lib.call("fmri_renorm", P(xd), P(out), n, scale, P(sd), cnt, None, P(f1))
        o = _take(out, n, "out16")
        g1 = _take(f1, 1, "factor_out")
        _say(f"F renorm n={n} no factor_in", GO.cmp_renorm(x, scale, ss[0], cnt, None, o, g1))
        out2 = _sent(n, torch.float16)
        lib.call("fmri_renorm", P(xd), P(out2), n, scale, P(sd), cnt, P(f1), P(f2))
        _say(f"F renorm n={n} chained factor", GO.cmp_renorm(x, scale, ss[0], cnt, g1[0], _take(out2, n, "out16"), _take(f2, 1, "factor_out")))
    z = np.zeros(16, F32)
    out, f1 = _sent(16, torch.float16), _sent(1, torch.float32)
    zd, sd, fd = _dev(z), _dev(np.zeros(1, F32)), _dev(np.array([0.5], F32))
    lib.call("fmri_renorm", P(zd), P(out), 16, 0.25, P(sd), 16.0, P(fd), P(f1))
    o = _take(out, 16, "out16")
    _say("F renorm all-zero (1e-20 floor)", GO.cmp_renorm(z, 0.25, 0.0, 16.0, 0.5, o, _take(f1, 1, "factor_out")) + [GO.bits("rows +0", o, np.zeros(16, F16))])


def test_axpby():
    """fmri_axpby_f16 (one device factor) with and without y, and ops.axpby(y=None); one n past the launcher's cap of
    4096 blocks x 256 threads x 8 values.  (The two-factor form is covered by tests/test_fullbatch_ops_gpu.py.)"""
    from fmri_hip import lib, ops
    P = lib.ptr
    rs = np.random.RandomState(9)
    a, pa, b = float(F32(0.75)), float(F32(GO.THIRD)), float(F32(-1.3))
    pad = _dev(np.array([pa], F32))
    for n in (8, 2056, GO.AXPBY_CAP + 8 * 300):
        x, y = rs.randn(n).astype(F16), (rs.randn(n) * 2).astype(F16)
        xd, yd = _dev(x), _dev(y)
        out = _sent(n, torch.float16)
        lib.call("fmri_axpby_f16", P(xd), P(yd), P(out), n, a, b, P(pad))
        _say(f"F axpby_f16 n={n} a_dev", GO.cmp_axpby(x, y, a, pa, b, _take(out, n, "out")))
        out = _sent(n, torch.float16)
        lib.call("fmri_axpby_f16", P(xd), None, P(out), n, a, b, None)
        _say(f"F axpby_f16 n={n} y=NULL a_dev=NULL", GO.cmp_axpby(x, None, a, None, b, _take(out, n, "out")))
        got = ops.axpby(xd, None, a, b, a_dev=pad)
        torch.cuda.synchronize()
        _say(f"F ops.axpby(y=None) n={n}", GO.cmp_axpby(x, None, a, pa, b, got.cpu().numpy()))
