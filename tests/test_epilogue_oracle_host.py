"""Host side of tests/test_conv_epilogues_gpu.py, no GPU needed: the kernel-name half of its route tables against the
library's own router (fmri_igemm_route is host code), the 2^24 validity of the grid inputs at small N scaled to the step's
pixel counts, and self-checks of tests/epilogue_oracle.py -- every bound is met by an fp32 emulation of the kernel's
arithmetic and missed by a planted wrong kernel (one pixel dropped, one row skipped, a biased running variance)."""

import pytest
import torch

import epilogue_oracle as EO

F32, F64 = torch.float32, torch.float64


def _layer(case):
    from fmri_hip import ops
    return ops, EO.make_layer(ops, EO.Group({"w": torch.zeros(EO.weight_shape(case))}, "cpu"), case)


# =====================================================================================================================
# route tables
# =====================================================================================================================
def test_tables_cover_the_cases():
    from test_kernels_gpu import FULL_SIZE, EPI_STAT_CASES, AFFINE_CASES
    assert set(EO.STAT_ROUTES) == set(EO.STAT_CASES)
    assert set(EO.CAP_CASES) <= set(EO.STAT_CASES) and set(EO.BN_CASES) <= set(EO.STAT_FULL)
    for case, _ in EO.STAT_FULL.values():
        assert case in FULL_SIZE or case[:6] == ("deconv", 256, 128, 2, 16, 1), case
    # every FULL_SIZE row between two BatchNorm'd maps is there (conv.0 of the discriminator and conv.3 of the decoder
    # carry a bias and an activation instead)
    want = {c for c in FULL_SIZE if not (c[1] == 3 and c[2] == 32) and c[2] != 3}
    assert want <= {case for case, _ in EO.STAT_FULL.values()}
    # the geometries of the small test that are restated as edges
    small = {(k, ci, co, s, H, op, N, g) for k, ci, co, s, H, op, N, g, _ in EPI_STAT_CASES}
    for name in ("px100 64->128 50px N=2 g=2", "px100 256->256 13px N=3 deconv", "px100 128->64 25px N=2 g=2 deconv",
                 "one tile per group conv", "one tile per group deconv", "straddle conv", "straddle deconv",
                 "solo classes deconv N=12 g=3"):
        case, groups = EO.STAT_EDGE[name]
        assert case + (groups,) in small, name
    assert {(c[0], c[1], c[2], c[4], c[5], c[6], e) for c, e in EO.AFFINE_SMALL.values()} >= set(AFFINE_CASES)
    # rows of every epilogue fit the capacity ConvLayer.forward allocates; the two-stage fold is reached
    for name, (kernel, expect, rows) in EO.STAT_ROUTES.items():
        case, groups = EO.STAT_CASES[name]
        assert (rows > 0) == expect and rows <= EO.usual_cap(case, groups), name
    assert max(r for _, _, r in EO.STAT_ROUTES.values()) > EO.FOLD_SWITCH


@pytest.mark.parametrize("name", list(EO.STAT_CASES))
def test_statistics_route_names(name):
    """Kernel name at the usual capacity; where the name shows the epilogue, ``rows`` is the smallest capacity at which the
    library still routes to that kernel."""
    case, groups = EO.STAT_CASES[name]
    kernel, expect, rows = EO.STAT_ROUTES[name]
    ops, layer = _layer(case)
    gn = case[6] // groups if groups > 1 else 0
    assert EO.route_of(ops, layer, case, EO.usual_cap(case, groups), gn) == kernel
    plain = EO.route_of(ops, layer, case)
    if expect and kernel != plain:
        assert EO.route_of(ops, layer, case, rows, gn) == kernel
        if rows > 1:
            assert EO.route_of(ops, layer, case, rows - 1, gn) != kernel
    if name in EO.CAP_CASES:
        at, below, _ = EO.CAP_CASES[name]
        assert at == kernel
        assert EO.route_of(ops, layer, case, rows - 1, gn) == below


@pytest.mark.parametrize("name", list(EO.AFFINE_FULL))
def test_affine_route_names(name):
    case, kernel, applied = EO.AFFINE_FULL[name]
    ops, layer = _layer(case)
    assert EO.route_of(ops, layer, case, affine=True) == kernel
    # the epilogue lives in the wide forms only
    assert applied == ("c5w" in kernel or "tc5w" in kernel)


# =====================================================================================================================
# grid inputs
# =====================================================================================================================
@pytest.mark.parametrize("name", list(EO.STAT_FULL))
def test_grid_inputs_stay_exact_at_the_full_pixel_count(name):
    """Two images (one per group where there are two) through the float64 convolution: integers, max |y| <= 2048, and
    sum |y| / sum y^2 per channel scaled to the step's pixels per group stay below 2^24 with a margin of 1.5 (the sums
    of 2 images of >= 64 pixels each scatter by far less)."""
    case, groups = EO.STAT_FULL[name]
    kind, cin, cout, stride, H, op, N = case
    n = 2 if groups <= 2 else groups
    small = (kind, cin, cout, stride, H, op, n)
    g = min(groups, n)
    w = EO.grid_weight(case, EO.case_seed(case, groups))
    co_axis = 0 if kind == "conv" else 1
    assert set(w.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert float(w.abs().sum([a for a in range(4) if a != co_axis]).min()) >= 1
    x = EO.make_input(small, "grid", EO.case_seed(case, groups), "cpu", groups=g)
    assert set(x.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    y = EO.conv64(x, w, small)
    assert bool((y == y.round()).all()) and float(y.abs().max()) <= 2048
    sums = EO.group_sums64(y, g)
    scale = (N // groups) / (n // g)
    assert float(sums[:, 2].max()) * scale * 1.5 < EO.LIMIT, float(sums[:, 2].max()) * scale
    assert float(sums[:, 1].max()) * scale * 1.5 < EO.LIMIT, float(sums[:, 1].max()) * scale
    if g > 1:
        # the groups are told apart: group 1 is twice group-0-like input
        assert float(sums[1, 1].sum()) > 2 * float(sums[0, 1].sum())


def test_affine_grid_map_is_exact_in_fp16():
    scale, shift = EO.affine_params(256, 3, "cpu")
    assert set(scale.abs().tolist()) <= {0.25, 0.5, 1.0, 2.0} and bool((scale < 0).any()) and bool((scale > 0).any())
    y = torch.arange(-61, 62, dtype=F64).reshape(-1, 1)
    p = EO.affine64(y, scale, shift, True)
    assert float(p.max()) < 128 and torch.equal(p.half().double(), p)
    f = torch.relu(y.float() * scale + shift)              # the kernel's fp32 arithmetic
    assert torch.equal(f.double(), p)


# =====================================================================================================================
# self-checks of the comparisons
# =====================================================================================================================
def test_bits_and_ratio():
    a = torch.tensor([1.0, float("nan"), 0.0, 3.0])
    assert EO.bits("x", a, a.clone())[2] == 0
    assert EO.bits("x", a, torch.tensor([1.0, float("nan"), -0.0, 3.0]))[2] == 1
    assert EO.bits("x", a, torch.tensor([1.0, 2.0, 0.0, 3.0]))[2] == 1
    assert EO.rat("x", torch.tensor([1.0, float("nan")]), torch.tensor([1.0, 1.0], dtype=F64), 1.0)[2] == float("inf")
    assert EO.rat("x", torch.tensor([1.5]), torch.tensor([1.0], dtype=F64), 1.0)[2] == 0.5
    assert EO.rat("x", torch.tensor([1.5]), torch.tensor([1.0], dtype=F64), 0.0)[2] == float("inf")
    assert EO.passed([("a", "bits", 0, 4), ("b", "ratio", 1.0, 4)]) and not EO.passed([("a", "bits", 1, 4)])
    with pytest.raises(AssertionError):
        EO.report("case", [("b", "ratio", 1.01, 4)])


def _emu_fold_columns(part, lo, hi, depth):
    """fold_columns of csrc/norm.hip in fp32: [rows][n] -> [n]."""
    n = part.shape[1]
    lanes = torch.zeros(32, n, dtype=F32)
    for r in range(32):
        acc = torch.zeros(depth, n, dtype=F32)
        p = lo + r
        while p + 32 * (depth - 1) < hi:
            for u in range(depth):
                acc[u] += part[p + 32 * u]
            p += 32 * depth
        while p < hi:
            acc[0] += part[p]
            p += 32
        lanes[r] = (acc[0] + acc[1]) + (acc[2] + acc[3]) if depth == 4 else acc[0] + acc[1]
    out = torch.zeros(n, dtype=F32)
    for r in range(32):
        out += lanes[r]
    return out


def _emu_fold(part, depth, skip=None):
    """The whole fold (fold_stage1 + the final pass); ``skip``: a row that is left out (a planted wrong kernel)."""
    rows = part.shape[0]
    if skip is not None:
        part = part.clone()
        part[skip] = 0
    if rows <= EO.FOLD_SWITCH:
        return _emu_fold_columns(part, 0, rows, depth)
    per = (rows + EO.FOLD_STAGE_ROWS - 1) // EO.FOLD_STAGE_ROWS
    ny = (rows + per - 1) // per
    stage = torch.stack([_emu_fold_columns(part, y * per, min(y * per + per, rows), 4) for y in range(ny)])
    return _emu_fold_columns(stage, 0, ny, depth)


@pytest.mark.parametrize("rows", [1, 33, 129, 512, 513, 1025])
@pytest.mark.parametrize("depth", [2, 4])
def test_fold_checks_accept_the_kernels_order_and_catch_a_skipped_row(rows, depth):
    for family in ("grid", "real"):
        part = EO.fold_rows_input(rows, 16, family, rows + depth, "cpu", cap=rows + 3)
        good = _emu_fold(part[0, :rows], depth).reshape(1, -1)
        assert EO.passed(EO.cmp_fold(family, part, rows, good, depth, "fold")), (family, rows)
        bad = _emu_fold(part[0, :rows], depth, skip=rows - 1).reshape(1, -1)
        assert not EO.passed(EO.cmp_fold(family, part, rows, bad, depth, "fold")), (family, rows)
    # the chain lengths: one pass of 512 rows with four accumulators = 4 + 2 + 32, two stages at 513
    assert EO.fold_chains(512, 4) == 38 and EO.fold_chains(512, 2) == 8 + 1 + 32
    assert EO.fold_chains(513, 4) == EO.fold_chain(17, 4) + EO.fold_chain(31, 4)
    assert EO.fold_chains(6152, 2) == EO.fold_chain(193, 4) + EO.fold_chain(32, 2)


def test_statistics_bounds_accept_fp32_sums_and_catch_eight_dropped_pixels():
    """discriminator.conv.1's pixel count (768 x 32 x 32 per channel, 256 rows): block sums in fp32, folded.  real: with
    eight pixels left out the project bounds still pass and the sharp bound on sum y^2 does not.  grid: ONE pixel
    left out fails the bitwise comparison."""
    M, C, rows = 768 * 32 * 32, 8, 256
    g = torch.Generator().manual_seed(1)

    def kernel_sums(v):
        blocks = v.float().reshape(rows, -1, C)
        part = torch.stack([blocks.sum(1), (blocks * blocks).sum(1)], 1).reshape(rows, 2 * C)
        return _emu_fold(part, 4).reshape(2, C)
    y = torch.randn(M, C, generator=g).half()
    sums = EO.group_sums64(y, 1)[0]
    assert EO.passed(EO.cmp_stat_sums("real", sums, kernel_sums(y), M, rows, 4, "fold"))
    miss = y.clone()
    miss[123456:123456 + 8] = 0
    by = {w: v for w, _, v, _ in EO.cmp_stat_sums("real", sums, kernel_sums(miss), M, rows, 4, "fold")}
    assert by["fold sum y | project"] <= 1.0 and by["fold sum y^2 | project"] <= 1.0, by
    assert by["fold sum y^2 | sharp"] > 2.0, by
    y = torch.randint(-3, 4, (M, C), generator=g).half()
    sums = EO.group_sums64(y, 1)[0]
    EO.assert_grid_valid(y, sums.reshape(1, 3, C))
    assert EO.passed(EO.cmp_stat_sums("grid", sums, kernel_sums(y), M, rows, 4, "fold"))
    miss = y.clone()
    miss[123456] = 0
    assert not EO.passed(EO.cmp_stat_sums("grid", sums, kernel_sums(miss), M, rows, 4, "fold"))


def _emu_finalize(sx, sxx, count, gamma, beta, updates, rm, rv, biased=False):
    """bn_finalize_channel in fp32 (uncontracted)."""
    c = torch.tensor(float(count), dtype=F32)
    mean = sx / c
    var = (sxx / c - mean * mean).clamp_min(0)
    rstd = torch.rsqrt(var + torch.tensor(1e-5, dtype=F32))
    sc = gamma * rstd
    sh = beta - mean * sc
    unb = var if (count <= 1 or biased) else var * c / (c - 1)
    m = torch.tensor(0.9, dtype=F32)
    rm, rv = rm.clone(), rv.clone()
    for _ in range(updates):
        rm = (1 - m) * rm + m * mean
        rv = (1 - m) * rv + m * unb
    return {"mean": mean, "rstd": rstd, "scale": sc, "shift": sh, "running_mean": rm, "running_var": rv}


@pytest.mark.parametrize("count", [1, 7, 65536])
@pytest.mark.parametrize("updates", [0, 1, 2])
def test_finalize_reference_and_bounds(count, updates):
    C = 40
    sx, sxx = EO.hard_sums(C, count, 11 + count, "cpu")
    g = torch.Generator().manual_seed(count)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    rm, rv = torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5
    fin = EO.finalize64(sx.double(), sxx.double(), count, gamma, beta, updates, rm, rv)
    # the float64 formula is nn.BatchNorm's: mean, biased variance for the normalisation, unbiased for the running one
    mean, var = sx.double() / count, (sxx.double() / count - (sx.double() / count) ** 2).clamp_min(0)
    assert torch.equal(fin["mean"][0], mean) and torch.equal(fin["var"][0], var)
    assert torch.allclose(fin["rstd"][0], (var + EO.EPS32).rsqrt(), rtol=1e-15)
    unb = var * count / (count - 1) if count > 1 else var
    r, s = rm.double(), rv.double()
    for _ in range(updates):
        r, s = (1 - EO.MOM32) * r + EO.MOM32 * mean, (1 - EO.MOM32) * s + EO.MOM32 * unb
    assert torch.allclose(fin["running_mean"][0], r, rtol=1e-15) and torch.allclose(fin["running_var"][0], s, rtol=1e-15)
    emu = _emu_finalize(sx, sxx, count, gamma, beta, updates, rm, rv)
    for k, v in emu.items():
        assert EO.rat(k, v, fin[k][0], fin[k][1])[2] <= 1.0, (k, count, updates)
    if updates and count > 1 and count < 1000:
        wrong = _emu_finalize(sx, sxx, count, gamma, beta, updates, rm, rv, biased=True)
        assert EO.rat("rv", wrong["running_var"], *fin["running_var"])[2] > 1.0
    # the constant channel: var is exactly 0 in float64, the kernel may see cancellation noise -- the interval holds it
    assert float(fin["var"][0][6]) == 0.0 and float(fin["rstd"][1][6]) >= 0.0


def test_batchnorm_apply_bound_accepts_fp32_and_catches_a_second_rounding_of_the_shift():
    M, C = 4096, 16
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(M, C, generator=g) * 1.5 + 0.3).half()
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    s = EO.group_sums64(x, 1)[0]
    fin = EO.finalize64(s[0], s[1], M, gamma, beta)
    emu = _emu_finalize(s[0].float(), s[1].float(), M, gamma, beta, 0, torch.zeros(C), torch.ones(C))
    y = torch.relu(x.float() * emu["scale"] + emu["shift"]).half()
    assert EO.passed(EO.cmp_bn_apply("y", x, y, fin))
    y2 = torch.relu(x.float() * emu["scale"] + emu["shift"].half().float()).half()      # shift through fp16
    assert not EO.passed(EO.cmp_bn_apply("y", x, y2, fin))


def test_affine_real_bound_catches_the_two_rounding_chain():
    """conv -> fp16 -> affine -> fp16 (the unfused chain) leaves the one-rounding bound; the fused form meets it."""
    g = torch.Generator().manual_seed(9)
    conv = torch.randn(4, 8, 8, 128, generator=g, dtype=F64)
    scale, shift = torch.rand(128, generator=g) * 3 + 0.5, torch.randn(128, generator=g) * 0.2
    fused = torch.relu(conv.float() * scale + shift).half()
    assert EO.passed(EO.cmp_affine_real("y", fused, conv, scale, shift, True, 25 * 128))
    twice = torch.relu(conv.half().float() * scale + shift).half()
    assert not EO.passed(EO.cmp_affine_real("y", twice, conv, scale, shift, True, 25 * 128))
