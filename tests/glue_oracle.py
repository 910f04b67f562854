"""TEST INFRASTRUCTURE ONLY -- numpy float64 restatement of the small kernels every step runs between its contractions
(csrc/layout.hip conversions and fmri_colsum_acc, csrc/norm.hip fmri_act_bwd / fmri_colsum_rows / fmri_bn_apply,
csrc/ingest.hip fmri_ingest_u8, csrc/loss.hip fmri_rows_absmax / fmri_sumsq / fmri_renorm / fmri_axpby_f16), the checks their
outputs are held to, and the seeded inputs tests/test_glue_oracle_host.py and tests/test_glue_kernels_gpu.py share.  Nothing
here imports the library under test (oracle/ingest_oracle.py, the golden-pinned restatement of the reference's transforms,
is test infrastructure as well).

Two input families:
  * exact grid: values k * 2^-3 (y of tanh in {0, +-0.5, +-1}).  Every term of every sum is a multiple of a power of two
    ``unit`` and ``assert_exact_sums`` checks sum |t| / unit < 2^24 per column: every partial sum, in any order, is then an
    integer below 2^24 in units and exactly representable in fp32.  The kernel's result must EQUAL the float64 result in
    every bit (a check kind "bits": the number of differing elements, which must be 0 -- an equality, not a ratio).
  * real: fp16-rounded normals.  Bounds from the number formats only (u = 2^-24, as tests/latent_oracle.py):
        fp32 sum of n terms, any order            n u sum|t|
        k fp32 roundings on a product chain       k u |p|
        fp16 store of p with fp32 error A         A + 2^-11 (|p| + A) + 2^-25
    (first order in u; the second-order terms are 2^-24 of these and far below the fp16 term or the slack of the worst
    case).  hipcc may contract a * b + c into one FMA; every bound below covers the contracted and the uncontracted form.
Single multiplies and pure casts (the four conversions, ReLU / none in fmri_act_bwd) must equal numpy bit for bit.

A check is a tuple (quantity, kind, value, elements): kind "bits" -> value = number of differing elements (NaN matches
NaN), kind "ratio" -> value = max err / bound over every element.  ``passed`` / ``lines`` are shared by both test files.
"""
import numpy as np

import latent_oracle as LO
from latent_oracle import H16, SUB16, U, f64

F16, F32 = np.float16, np.float32
THIRD = float(F32(1.0 / 3.0))
SCALES = (1.0, 0.5, THIRD)
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2
ACT_NAME = {0: "none", 1: "relu", 2: "tanh"}
OVER16 = 65520.0            # fp32 -> fp16 (round to nearest even): |v| >= 65520 becomes inf, below it 65504


# ---------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------
def mismatches(got, ref):
    """Number of elements whose bits differ (a NaN equals any NaN; +0 and -0 differ)."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    it = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    gn, rn = np.isnan(got), np.isnan(ref)
    return int(np.count_nonzero((gn != rn) | (~gn & ~rn & (got.view(it) != ref.view(it)))))


def first_diffs(got, ref, k=4):
    """(index, got, reference) of the first k differing elements, for a failure message."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    it = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    gn, rn = np.isnan(got), np.isnan(ref)
    idx = np.argwhere((gn != rn) | (~gn & ~rn & (got.view(it) != ref.view(it))))[:k]
    return [(tuple(int(v) for v in i), float(got[tuple(i)]), float(ref[tuple(i)])) for i in idx]


def bits(what, got, ref):
    n = mismatches(got, ref)
    if n:
        print(f"[glue]   {what}: first differences (index, got, reference): {first_diffs(got, ref)}", flush=True)
    return (what, "bits", n, int(np.asarray(ref).size))


def rat(what, got, p, bound):
    return (what, "ratio", LO.ratio(got, p, bound), int(np.asarray(p).size))


def passed(results):
    return all((v == 0) if kind == "bits" else (v <= 1.0) for _, kind, v, _ in results)


def lines(case, results):
    out = []
    for what, kind, v, n in results:
        if kind == "bits":
            out.append(f"[glue] {case} | {what} | bitwise: {v} of {n} differ")
        else:
            out.append(f"[glue] {case} | {what} | err/bound = {v:.4f}")
    return out


def bound_store16(p, A):
    return A + H16 * (np.abs(p) + A) + SUB16


def assert_exact_sums(terms, unit):
    """The exactness argument of the grid family: every term a multiple of ``unit`` and, per column, sum |t| < 2^24 units."""
    t = f64(terms) / unit
    assert np.array_equal(t, np.rint(t)), "term off the grid"
    assert float(np.abs(t).reshape(t.shape[0], -1).sum(0).max()) < 2.0 ** 24, "a partial sum could leave the exact range"


def pad8(c):
    return (c + 7) // 8 * 8


# ---------------------------------------------------------------------------------------------------------------------
# launch geometry of csrc/norm.hip (which row counts sit on an edge of the row loops)
# ---------------------------------------------------------------------------------------------------------------------
def row_lanes(C):
    """RY of row_geometry: a 256-thread block is CX chunk columns (CX = the power of two >= C/8, at most 256) x RY lanes."""
    nch, lg = C // 8, 0
    while (1 << lg) < nch and lg < 8:
        lg += 1
    return 256 >> lg


ACT_C = (8, 24, 64, 512, 2056)      # one chunk column | an idle chunk column | ... | gx = 2 with a nearly empty block
BN_C = (8, 24, 512, 2056)


def act_rows(C):
    """1, 31, the two sides of the x4 unrolled row loop at one block row (stride = RY) and two block rows.  BIG (the decoder
    output's 2^20 rows at C = 8, 256 block rows) is a case of its own in both test files."""
    ry = row_lanes(C)
    return [1, 31, 4 * ry - 1, 4 * ry + 1, 16 * ry + 1]


BIG = (2 ** 20, 8)


def act_lanes(M, C):
    """Row lanes of fmri_act_bwd / fmri_colsum_rows over all blocks (row_geometry: gy block rows of RY lanes)."""
    ry = row_lanes(C)
    gx = (C // 8 + 256 // ry - 1) // (256 // ry)
    gy = max(1, min((M + ry * 16 - 1) // (ry * 16), max(768 // gx, 1)))
    return gy * ry


def bn_rows(C):
    ry = row_lanes(C)
    return [1, 7, 8 * ry - 1, 8 * ry + 1]


# ---------------------------------------------------------------------------------------------------------------------
# A. conversions
# ---------------------------------------------------------------------------------------------------------------------
IMG_SHAPES = [(N, C, HW) for N in (1, 3) for C in (1, 3, 8, 9, 20, 64) for HW in (1, 7, 64 * 64)]
IMG_CAP = (5, 20, 75000)            # N HW Cp/8 = 1 125 000 and N C HW = 7 500 000 items > 4096 x 256
ROW_SHAPES = [(M, C) for M in (1, 5, 257) for C in (1, 7, 8, 12, 3620)]
ROW_CAP = (300, 3620)               # M Cp = 1 087 200 and M C = 1 086 000 items > 4096 x 256

_T = 2.0 ** -24                     # smallest fp16 subnormal
SPECIALS = np.array(
    [0.0, -0.0, _T, -_T, 3 * _T, 1023 * _T, 2.0 ** -14, 2.0 ** -25, -2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -10), 1.5 * _T,
     2.5 * _T, 1e-10, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -20, 2047.0, 2049.0,
     65504.0, -65504.0, 65503.0, 65519.0, 65519.99, 65520.0, -65520.0, 65536.0, 1e5, -1e5, 3 * 65504.0, 131040.0, 196559.0,
     196561.0, np.inf, -np.inf, np.nan, 32752.0, 32760.0], dtype=F32)


def conv_values(n, seed, as16):
    """n values: normals (sigma 4) with the special values spread over them, rotated by the seed so that the small
    shapes cover all of them between them.  ``as16``: an fp16 source (specials rounded to fp16: subnormals, +-65504,
    +-0, inf, NaN survive), else an fp32 source (unrounded: ties and overflowing values reach the kernel's cast)."""
    rs = np.random.RandomState(seed)
    x = (rs.randn(n) * 4.0).astype(F32)
    k = min(n, len(SPECIALS))
    idx = np.unique(np.linspace(0, n - 1, k).astype(np.int64))
    x[idx] = SPECIALS[(np.arange(len(idx)) + seed) % len(SPECIALS)]
    if as16:
        with np.errstate(over="ignore"):
            return x.astype(F16)
    return x


def _cast16(v64):
    """The kernel's two roundings: float64 value -> fp32 (the multiply's rounding) -> fp16 (the cast)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return v64.astype(F32).astype(F16)


def nchw_to_nhwc_ref(x32, Cp):
    """[N][C][HW] fp32 -> [N][HW][Cp] fp16, channels [C, Cp) zero."""
    N, C, HW = x32.shape
    out = np.zeros((N, HW, Cp), F16)
    out[:, :, :C] = _cast16(f64(x32)).transpose(0, 2, 1)
    return out


def nhwc_to_nchw_ref(x16, C, scale):
    """[N][HW][Cp] fp16 -> [N][C][HW] fp32, scaled (one fp32 multiply)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (f64(x16)[:, :, :C] * float(F32(scale))).astype(F32).transpose(0, 2, 1).copy()


def rows_f32_to_f16_ref(x32, Cp, scale):
    M, C = x32.shape
    out = np.zeros((M, Cp), F16)
    with np.errstate(over="ignore", invalid="ignore"):
        out[:, :C] = _cast16(f64(x32) * float(F32(scale)))
    return out


def rows_f16_to_f32_ref(x16, C, scale):
    with np.errstate(over="ignore", invalid="ignore"):
        return (f64(x16)[:, :C] * float(F32(scale))).astype(F32)


def cmp_conv(got, ref, C=None):
    """Every element bitwise; with ``C`` the padded lanes [C, Cp) of the last axis are also checked to be +0 by themselves."""
    res = [bits("all elements", got, ref)]
    if C is not None and C < ref.shape[-1]:
        pad = np.ascontiguousarray(np.asarray(got)[..., C:])
        res.append(("padded lanes", "bits", int(np.count_nonzero(pad.view(np.uint16))), int(pad.size)))
    return res


# ---------------------------------------------------------------------------------------------------------------------
# B. fmri_act_bwd
# ---------------------------------------------------------------------------------------------------------------------
def grid16(rs, shape, kmax):
    return (rs.randint(-kmax, kmax + 1, size=shape) * 0.125).astype(F16)


def grid_kmax(M):
    """|k| <= 32 as long as 2^15 rows of it stay exact, |k| <= 4 for the long columns (sum k^2 of 2^20 rows < 2^24)."""
    return 32 if M <= 2 ** 13 else 4


def act_inputs(M, C, act, family, seed):
    """y16, dy16 [M][C].  grid: dy = k/8; y from {+-0, +-0.5, +-1, +-2^-24} (ReLU / none: the zeros and the subnormal hold
    the mask to ``>``) or {0, +-0.5, +-1} (tanh).  real: dy ~ N(0, 1) in fp16; y = tanh(N(0, 1)) for tanh, N(0, 1) with
    +-0 and +-2^-24 entries otherwise."""
    rs = np.random.RandomState(seed)
    if family == "grid":
        dy = grid16(rs, (M, C), grid_kmax(M))
        vals = np.array([0.0, 0.5, -0.5, 1.0, -1.0] if act == ACT_TANH else [0.0, -0.0, 0.5, -0.5, 1.0, -1.0, _T, -_T], F16)
        y = vals[rs.randint(0, len(vals), size=(M, C))]
    else:
        dy = rs.randn(M, C).astype(F16)
        if act == ACT_TANH:
            y = np.tanh(rs.randn(M, C) * 1.5).astype(F16)
        else:
            y = rs.randn(M, C).astype(F16)
            f = y.reshape(-1)
            f[0::7], f[3::11], f[5::13], f[6::17] = 0.0, -0.0, _T, -_T
    return y, dy


def act_bwd64(y16, dy16, act):
    """dpre = dy * act'(y) in float64 from the activation's OUTPUT y: ReLU dy where y > 0 else +0, tanh dy (1 - y^2)."""
    y, dy = f64(y16), f64(dy16)
    if act == ACT_RELU:
        return np.where(y > 0, dy, 0.0)
    if act == ACT_TANH:
        return dy * (1.0 - y * y)
    return dy.copy()


def cmp_act(y16, dy16, act, family, dpre16, colsum=None, dbias=None, prior=None, gscale=1.0):
    """dpre16 [M][C] fp16; colsum: the first C floats of the kernel's [2][C] (the second half is documented as unused);
    dbias: all of the buffer (entries behind len(prior) = dbias_n ... must still hold ``prior``: prior covers all of it,
    dbias_n = ``n`` entries were to be updated -- passed as the tuple (buffer, n))."""
    p = act_bwd64(y16, dy16, act)
    M = p.shape[0]
    res = []
    if act == ACT_TANH and family == "real":
        # fl(1 - y^2) (y^2 is exact in fp32: 11 x 11 bits; an FMA rounds the same value once) and the product: 2 roundings
        res.append(rat("dpre", dpre16, p, bound_store16(p, 2 * U * np.abs(p))))
    else:
        # ReLU / none: a select and a cast of an fp16 value; tanh on the grid: dy (1 - y^2) is a multiple of 2^-5 below 2^3
        with np.errstate(over="ignore"):
            res.append(bits("dpre", dpre16, p.astype(F16)))
    if colsum is None:
        return res
    s = p.sum(0)
    if family == "grid":
        assert_exact_sums(p, 2.0 ** -5)
        res.append(bits("colsum", np.asarray(colsum, F32), s.astype(F32)))
    else:
        # M terms, each carrying 2 roundings of its own for tanh (0 otherwise: dy is an fp16 value)
        k = M + (2 if act == ACT_TANH else 0)
        res.append(rat("colsum", colsum, s, k * U * np.abs(p).sum(0)))
    if dbias is None:
        return res
    buf, n = dbias
    pr = f64(prior)
    want = pr.copy()
    want[:n] += gscale * s[:n]
    if family == "grid":
        res.append(bits("dbias", np.asarray(buf, F32), want.astype(F32)))
    else:
        # the sum's bound, one rounding of gscale * s and one of the add (or one FMA)
        S = abs(gscale) * np.abs(p).sum(0)
        bound = np.zeros_like(want)
        bound[:n] = (k + 1) * U * (S[:n] + np.abs(pr[:n]))
        res.append(rat("dbias", buf, want, bound))          # (entries behind n: bound 0, any change is an infinite ratio)
    return res


def emu_sum32(terms32, lanes):
    """fp32 column sums in a kernel-like order: ``lanes`` row lanes each add their rows m = lane, lane + lanes, ... in turn,
    then the lanes are added in turn."""
    t = np.asarray(terms32, F32)
    M = t.shape[0]
    steps = (M + lanes - 1) // lanes
    padded = np.zeros((steps * lanes,) + t.shape[1:], F32)
    padded[:M] = t
    padded = padded.reshape((steps, lanes) + t.shape[1:])
    acc = np.zeros((lanes,) + t.shape[1:], F32)
    for i in range(steps):
        acc += padded[i]
    if lanes > 256:                     # blocks of 256 lanes first, then the blocks
        acc = acc.reshape((lanes // 256, 256) + t.shape[1:])
        blk = np.zeros((lanes // 256,) + t.shape[1:], F32)
        for r in range(256):
            blk += acc[:, r]
        acc = blk
    s = np.zeros(t.shape[1:], F32)
    for r in range(acc.shape[0]):
        s += acc[r]
    return s


def emu_act(y16, dy16, act, lanes, prior=None, n=0, gscale=1.0, relu_ge=False, tanh_1my=False, no_gscale=False):
    """The kernel's arithmetic in float32 (uncontracted), one rounding to fp16; the keyword flags plant wrong kernels."""
    y, g = np.asarray(y16).astype(F32), np.asarray(dy16).astype(F32)
    if act == ACT_RELU:
        g = np.where((y >= 0) if relu_ge else (y > 0), g, F32(0))
    elif act == ACT_TANH:
        g = g * ((F32(1) - y) if tanh_1my else (F32(1) - y * y))
    s = emu_sum32(g, lanes)
    db = None
    if prior is not None:
        db = np.asarray(prior, F32).copy()
        db[:n] = db[:n] + (s[:n] if no_gscale else F32(gscale) * s[:n])
    return g.astype(F16), s, db


# ---------------------------------------------------------------------------------------------------------------------
# C. column sums
# ---------------------------------------------------------------------------------------------------------------------
CS_C = (1, 5, 8, 9, 513)
CS_M = (1, 31, 32, 33, 2047)
CSR_SHAPES = [(2048, 8), (2048, 24), (2049, 8), (2049, 64), (2 ** 20, 8), (3 * 2 ** 15, 64)]


def colsum_src(M, C, family, f16, seed):
    """[M][C] source of a column sum, fp16 or fp32 (grid values are the same numbers in both)."""
    rs = np.random.RandomState(seed)
    if family == "grid":
        return grid16(rs, (M, C), grid_kmax(M)).astype(F16 if f16 else F32)
    x = rs.randn(M, C)
    return x.astype(F16) if f16 else x.astype(F16).astype(F32)


def colsum_prior(n, family, seed):
    rs = np.random.RandomState(seed + 77)
    return (rs.randint(-16, 17, size=n) * 0.25).astype(F32) if family == "grid" else (rs.randn(n) * 0.3).astype(F32)


def cmp_colsum(src, scale, prior, C, family, got):
    """got = the whole dst buffer after ``dst[c] += scale * sum_m src[m][c]``, c < C; len(prior) >= C entries."""
    x = f64(src)
    M = x.shape[0]
    pr = f64(prior)
    want = pr.copy()
    want[:C] += scale * x.sum(0)
    if family == "grid":
        assert_exact_sums(x, 0.125)
        return [bits("dst", np.asarray(got, F32), want.astype(F32))]
    bound = np.zeros_like(want)
    bound[:C] = LO.bound_dbias(abs(scale) * np.abs(x).sum(0) + np.abs(pr[:C]), M)      # (M + 1) u (|scale| S + |prior|)
    return [rat("dst", got, want, bound)]


def cmp_colsum_rows(x16, family, sums, dbias=None, prior=None, n=0, gscale=1.0):
    """sums [2][C] = [sum x | sum x^2] (x^2 of an fp16 value is exact in fp32), dbias[:n] += gscale * sum x."""
    x = f64(x16)
    M = x.shape[0]
    s1, s2 = x.sum(0), (x * x).sum(0)
    res = []
    if family == "grid":
        assert_exact_sums(x, 0.125)
        assert_exact_sums(x * x, 2.0 ** -6)
        res += [bits("sum x", np.asarray(sums[0], F32), s1.astype(F32)), bits("sum x^2", np.asarray(sums[1], F32), s2.astype(F32))]
    else:
        res += [rat("sum x", sums[0], s1, M * U * np.abs(x).sum(0)), rat("sum x^2", sums[1], s2, M * U * s2)]
    if dbias is not None:
        pr = f64(prior)
        want = pr.copy()
        want[:n] += gscale * s1[:n]
        if family == "grid":
            res.append(bits("dbias", np.asarray(dbias, F32), want.astype(F32)))
        else:
            bound = np.zeros_like(want)
            bound[:n] = LO.bound_dbias(abs(gscale) * np.abs(x).sum(0)[:n] + np.abs(pr[:n]), M)
            res.append(rat("dbias", dbias, want, bound))
    return res


# ---------------------------------------------------------------------------------------------------------------------
# D. fmri_bn_apply
# ---------------------------------------------------------------------------------------------------------------------
def bn_inputs(M, C, seed):
    """x16 [M][C], scale / shift fp32 [C].  Channel c % 8: 1 -> scale 0, 2 -> negative scale, 3 -> scale 4096 and shift 0
    with x from {0, +-1/16, +-32, +-64}: results 0, +-256 or +-131072 / +-262144, far on either side of fp16's range."""
    rs = np.random.RandomState(seed)
    x = (rs.randn(M, C) * 2.0).astype(F16)
    a = (0.5 + rs.rand(C)).astype(F32)
    b = (rs.randn(C) * 0.5).astype(F32)
    a[1::8] = 0.0
    a[2::8] *= -1.0
    a[3::8], b[3::8] = 4096.0, 0.0
    hot = np.array([0.0, 0.0625, -0.0625, 32.0, -32.0, 64.0, -64.0], F16)
    x[:, 3::8] = hot[rs.randint(0, len(hot), size=x[:, 3::8].shape)]
    return x, a, b


def cmp_bn(x16, a32, b32, relu, got16):
    """y = relu?(x a + b) stored with a plain cast: bn_stream_kernel<0> does NOT saturate (only the backward kernels go
    through sat16), so a result past fp16's range must come out as +-inf, as numpy's astype(float16) gives.
    fp32 error: one FMA rounding u |p|, or u |x a| + u |p| uncontracted; then the fp16 store."""
    x, a, b = f64(x16), f64(a32).reshape(1, -1), f64(b32).reshape(1, -1)
    p = x * a + b
    A = U * (np.abs(x * a) + np.abs(p))
    if relu:
        p = np.maximum(p, 0.0)
    over = np.abs(p) >= OVER16 * (1 + 2.0 ** -10)
    near = (np.abs(p) > 65504.0 * (1 - 2.0 ** -10)) & ~over
    assert not near.any(), "an input on the edge of fp16's range: the case must keep clear of it"
    g = np.asarray(got16)
    res = []
    if over.any():
        with np.errstate(over="ignore"):
            res.append(bits("overflow -> inf", g[over], p[over].astype(F16)))
    res.append(rat("y", g[~over], p[~over], bound_store16(p, A)[~over]))
    return res


def emu_bn(x16, a32, b32, relu):
    f = np.asarray(x16).astype(F32) * np.asarray(a32, F32).reshape(1, -1) + np.asarray(b32, F32).reshape(1, -1)
    if relu:
        f = np.where(f > 0, f, F32(0))
    with np.errstate(over="ignore"):
        return f.astype(F16)


# ---------------------------------------------------------------------------------------------------------------------
# E. fmri_ingest_u8
# ---------------------------------------------------------------------------------------------------------------------
INGEST_HW = ((1, 1), (1, 9), (9, 1), (5, 7), (64, 64))
INGEST_STATS = (((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),
                ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
                ((0.1, 0.9, 0.33), (1.7, 0.05, 0.6)))
INGEST_CAP = (65, 128, 128)          # 1 064 960 pixels > 4096 x 256: image 64 is reached by the second sweep only


def ingest_shifts(H, W):
    """Every (row shift, column shift) pair of {0, +-1, +-(n-1), +-n, +-(n+3)} (n = H for rows, W for columns), each with
    and without the flip: 162 images.  Shifts of n and n + 3 are beyond the image: every pixel is then an edge pixel."""
    one = lambda n: [0, 1, -1, n - 1, -(n - 1), n, -n, n + 3, -(n + 3)]
    sh = np.array([(sy, sx) for sy in one(H) for sx in one(W)] * 2, np.int32)
    fl = np.repeat(np.array([0, 1], np.int32), len(sh) // 2)
    return fl, sh


def ingest_images(N, H, W, C, seed):
    """Random uint8 images with 0 and 255 present; no image is left-right symmetric when W > 1 (checked)."""
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, size=(N, H, W, C)).astype(np.uint8)
    img.reshape(N, -1)[:, 0] = 0
    if H * W * C > 1:
        img.reshape(N, -1)[:, -1] = 255
    if W > 1:
        assert all((im != im[:, ::-1]).any() for im in img)
    return img


def ingest_pixels(img, flip, shift):
    """The geometry of the reference, from the golden-pinned oracle itself: ingest(mean 0, std 1) * 255 is the uint8 value
    the oracle put at every output position -> float64 [N][3][H][W] of integers."""
    from oracle import ingest_oracle as IO
    v = IO.ingest(img, flip, shift, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))
    return np.rint(f64(v) * 255.0)


def ingest64(pix, mean, std):
    """(p / 255 - m) / std in float64, m and std the fp32 values the oracle and the C ABI both take; also the error bound
    of the kernel's fp32 form  (p * fl(1/255) - m) * fl(1/std):
        v = p * fl(1/255): 2 roundings (the constant, the product; an FMA with the subtraction drops the second) 2 u p/255
        d = v - m: one rounding u |d|;  r = fl(1/std): u;  d * r: u    ->    (2 u p/255 + 3 u |d|) / |std|."""
    m = f64(np.asarray(mean, F32)).reshape(1, 3, 1, 1)
    s = f64(np.asarray(std, F32)).reshape(1, 3, 1, 1)
    v = pix / 255.0
    d = v - m
    return d / s, (2 * U * v + 3 * U * np.abs(d)) / np.abs(s)


def cmp_ingest(pix, mean, std, o16=None, o32=None):
    """o32 [N][3][H][W] fp32, o16 [N][H][W][8] fp16 (lanes 3..7 exactly +0)."""
    p, b32 = ingest64(pix, mean, std)
    res = []
    if o32 is not None:
        res.append(rat("fp32", o32, p, b32))
    if o16 is not None:
        g = np.asarray(o16)
        res.append(rat("fp16", g[..., :3].transpose(0, 3, 1, 2), p, bound_store16(p, b32)))
        pad = np.ascontiguousarray(g[..., 3:])
        res.append(("padded lanes 3..7", "bits", int(np.count_nonzero(pad.view(np.uint16))), int(pad.size)))
    return res


def emu_ingest(img, flip, shift, mean, std, shift_first=False, sign=1, clamp_off=0, sweep_items=None):
    """The kernel in float32 (uncontracted).  Wrong kernels: ``shift_first`` (shift applied before the flip), ``sign`` = -1
    (shift direction reversed), ``clamp_off`` = 1 (edge clamp one pixel short), ``sweep_items`` (pixels from that flat
    index on are never written: the output keeps its fill of 1000)."""
    N, H, W, C = img.shape
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    o32 = np.empty((N, 3, H, W), F32)
    m = np.asarray(mean, F32)
    r = F32(1) / np.asarray(std, F32)
    for n in range(N):
        sy, sx = (int(shift[n][0]) * sign, int(shift[n][1]) * sign) if shift is not None else (0, 0)
        fl = bool(flip[n]) if flip is not None else False
        if shift_first:                                 # out = flip(shift(img)): un-flip the output column, then shift
            xo = (W - 1 - x) if fl else x
            yy, xx = np.clip(y - sy, 0, H - 1 - clamp_off), np.clip(xo - sx, 0, W - 1 - clamp_off)
        else:                                           # out = shift(flip(img))
            yy, xx = np.clip(y - sy, 0, max(H - 1 - clamp_off, 0)), np.clip(x - sx, 0, max(W - 1 - clamp_off, 0))
            if fl:
                xx = W - 1 - xx
        px = img[n][yy, xx].astype(F32)                 # [H][W][C]
        for c in range(3):
            v = px[..., c if C == 3 else 0] * F32(1.0 / 255.0)
            o32[n, c] = (v - m[c]) * r[c]
    o16 = np.zeros((N, H, W, 8), F16)
    o16[..., :3] = o32.transpose(0, 2, 3, 1).astype(F16)
    if sweep_items is not None:
        o16.reshape(-1, 8)[sweep_items:] = 1000.0
        f = np.moveaxis(o32, 1, -1).reshape(-1, 3).copy()
        f[sweep_items:] = 1000.0
        o32 = np.moveaxis(f.reshape(N, H, W, 3), -1, 1).copy()
    return o16, o32


# ---------------------------------------------------------------------------------------------------------------------
# F. scalars and mixing
# ---------------------------------------------------------------------------------------------------------------------
ABSMAX_CAP = 256 * 256              # rows_absmax / sumsq / renorm launch at most 256 blocks of 256 threads
ABSMAX_N = (1, 255, 257, 2 * ABSMAX_CAP + 5)
AXPBY_CAP = 4096 * 256 * 8          # fmri_axpby_f16: 4096 blocks x 256 threads x 8 values


def absmax_ref(x32, prior):
    """max(prior, max |x|) over the values that are not NaN: the kernel folds with fmaxf, which returns its other operand
    when one is a NaN, so NaNs are skipped (an all-NaN input leaves the prior)."""
    a = np.abs(np.asarray(x32, F32))
    a = a[~np.isnan(a)]
    return np.array([max(F32(prior), a.max() if a.size else F32(0))], F32)


def sumsq_inputs(n, seed):
    return grid16(np.random.RandomState(seed), (n,), 8).astype(F32)


def cmp_sumsq(x32, prior, got):
    x = f64(x32).reshape(-1, 1)
    assert_exact_sums(np.concatenate([x * x, [[float(prior)]]]), 2.0 ** -6)
    return [bits("acc", np.asarray(got, F32).reshape(1), np.array([prior + (x * x).sum()], F32))]


def renorm64(x32, scale, sumsq, count, factor_in):
    f = 1.0 / max(np.sqrt(float(sumsq) / float(count)), 1e-20)
    return f64(x32) * f * float(F32(scale)), (1.0 if factor_in is None else float(factor_in)) * f


def cmp_renorm(x32, scale, sumsq, count, factor_in, out16, factor_out):
    """f = 1 / max(sqrt(ss / count), 1e-20): roundings (float) sqrt [or the fp32 constant 1e-20f], 1 / ., then f * scale and
    x * sc for the rows (4 u |p| and the fp16 store), factor_in * f for the factor (3 u |p|)."""
    p, pf = renorm64(x32, scale, sumsq, count, factor_in)
    return [rat("out16", out16, p, bound_store16(p, 4 * U * np.abs(p))),
            rat("factor_out", np.asarray(factor_out, F32).reshape(1), np.array([pf]), np.array([3 * U * abs(pf)]))]


def cmp_axpby(x16, y16, a, pa, b, got16):
    """out = fl(a * pa) x + b y: fl(a pa) u, the products and the add u each (or one FMA): 2 u |a pa x| + u |b y| + u |p|."""
    x = f64(x16)
    ax = float(F32(a)) * (1.0 if pa is None else float(F32(pa))) * x
    if y16 is None:
        p, A = ax, 2 * U * np.abs(ax)
    else:
        by = float(F32(b)) * f64(y16)
        p = ax + by
        A = 2 * U * np.abs(ax) + U * np.abs(by) + U * np.abs(p)
    return [rat("out", got16, p, bound_store16(p, A))]
