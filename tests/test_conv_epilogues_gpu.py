"""The statistics and affine epilogues of the contraction kernels at the sizes of the fused steps, the folds of the
statistics rows, and BatchNorm from those rows, against float64 (tests/epilogue_oracle.py has the cases, the route table,
the two input families and the derivation of every bound; tests/test_epilogue_oracle_host.py is the CPU half).

Every convolution that feeds a train-mode BatchNorm runs the ``<..,1>`` instantiation of its kernel in the steps
(``ConvLayer.forward(bn_groups=g)``), every one in the eval pass the affine epilogue of the ``<..,0>`` instantiation;
tests/test_fullbatch_conv_gpu.py covers neither at these sizes, and tests/test_kernels_gpu.py folds small cases on the
host with tolerances that hide tens of pixels.  Here the rows are folded by the library (fmri_bn_fold,
fmri_bn_fold_finalize), the reference is the float64 column sum of the tensor the kernel itself stored, and on the grid
family every comparison is bitwise: one miscounted pixel fails.

Unwritten memory: output buffers, row buffers, fold scratch and result vectors are NaN-filled before every launch, and
every convolution output is followed by a 64 KiB NaN guard band in the same allocation that must still be NaN afterwards
(the kernels address the output through a buffer descriptor plus a scalar row offset).
One line ``[epilogue] <case> | <quantity> | ...`` per check; profiles/epilogue_parity.md records one run.
"""
import math
import time

import pytest
import torch

import epilogue_oracle as EO
from test_fullbatch_conv_gpu import _Spy, _nan16

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
_id = lambda n: n.replace(" ", "_").replace("->", "to")


def _nan32(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


GUARD = 1 << 15          # fp16 elements behind every convolution output


def _out16(*shape):
    """NaN-filled fp16 output buffer and the NaN guard band behind it (one allocation)."""
    n = math.prod(shape)
    big = torch.full((n + GUARD,), NAN, dtype=torch.float16, device=DEV)
    return big[:n].view(shape), big[n:]


def _untouched(what, guard):
    return (what + ": guard band behind the output", "bits", int((~torch.isnan(guard)).sum()), int(guard.numel()))


def _P(t):
    return None if t is None else t.data_ptr()


def _setup(case, family, groups, with_bn=False):
    """ops, parameter group, layer, the fp32 weight and the case's seed."""
    from fmri_hip import ops
    seed = EO.case_seed(case, groups)
    w = EO.grid_weight(case, seed) if family == "grid" else EO.real_weight(case, seed)
    g = EO.bn_group({"w": w}, EO.pad8(case[2]), DEV, seed) if with_bn else EO.Group({"w": w}, DEV)
    return ops, g, EO.make_layer(ops, g, case), w, seed


def _check_launch_args(ops, layer, case, a):
    """The recorded fmri_igemm_ep call is the one EO.route_of asks the router about."""
    kind, cin, cout, stride, H, op, N = case
    Ho = EO.out_hw(kind, H, stride, op)
    mode = ops.MODE_CONV if kind == "conv" else ops.MODE_TCONV2
    assert tuple(a[5:23]) == (N, H, H, layer.cinp, Ho, Ho, layer.coutp, layer.cout, 5, stride, 2, mode, ops.ACT_NONE, 0, 1, 0,
                              layer.t_out, layer.pw_f.buf.numel()), a[5:23]


def _fold(rows_t, rows, C):
    """[2][C] through fmri_bn_fold and through fmri_bn_fold_finalize (gamma 1, beta 0, no running statistics)."""
    from fmri_hip import lib
    nscr = lib.load().fmri_bn_fold_scratch_floats(C)
    a, b = _nan32(2, C), _nan32(2, C)
    lib.call("fmri_bn_fold", _P(rows_t), rows, C, _P(_nan32(nscr)), _P(a))
    one, zero, junk = torch.ones(C, device=DEV), torch.zeros(C, device=DEV), _nan32(4, C)
    lib.call("fmri_bn_fold_finalize", _P(rows_t), rows, C, _P(_nan32(nscr)), _P(b), 1.0, _P(one), _P(zero), 1e-5, 0.9, 0,
             None, None, _P(junk[0]), _P(junk[1]), _P(junk[2]), _P(junk[3]), None)
    return a, b


# =====================================================================================================================
# 1. statistics epilogue
# =====================================================================================================================
@pytest.mark.parametrize("family", ["grid", "real"])
@pytest.mark.parametrize("name", list(EO.STAT_CASES), ids=_id)
def test_statistics_epilogue(name, family):
    """Route, stored output, unwritten / overwritten rows, group isolation, folded sums, determinism (module docstring);
    a declined request leaves every row untouched and BatchNorm to its own pass."""
    from fmri_hip.ops import BatchNorm
    t0 = time.time()
    case, groups = EO.STAT_CASES[name]
    kernel, expect, rows = EO.STAT_ROUTES[name]
    kind, cin, cout, stride, H, op, N = case
    label = f"{name} {kind} {cin}->{cout} {H}px N={N} g={groups} {family}"
    ops, g, layer, w, seed = _setup(case, family, groups, with_bn=True)
    C, Ho, B = layer.coutp, EO.out_hw(kind, H, stride, op), N // groups
    cap, gn = EO.usual_cap(case, groups), (N // groups if groups > 1 else 0)
    pixels = B * Ho * Ho
    assert EO.route_of(ops, layer, case, cap, gn) == kernel
    res = []
    for zero_group in ([None] + ([0] if groups > 1 else [])):
        tag = "" if zero_group is None else "group 0 zero: "
        x16 = EO.make_input(case, family, seed, DEV, groups, zero_group)
        plain, guard0 = _out16(N, Ho, Ho, C)
        layer.forward(x16, out=plain)
        part = layer._stat_part = _nan32(groups, cap, 2, C)
        y16, guard1 = _out16(N, Ho, Ho, C)
        with _Spy() as spy:
            layer.forward(x16, out=y16, bn_groups=groups)
        torch.cuda.synchronize()
        res += [_untouched(tag + "plain", guard0), _untouched(tag + "statistics", guard1)]
        _check_launch_args(ops, layer, case, spy.args_of("fmri_igemm_ep")[0])
        assert layer._stat_part is part, "the layer replaced a row buffer of the usual capacity"
        assert layer._stat_rows == rows, (label, layer._stat_rows, rows)
        assert (layer.take_stats(0) is not None) == expect
        # stored output
        assert bool(torch.isfinite(plain).all()) and bool(torch.isfinite(y16).all()), "an output element was never written"
        res.append(EO.bits(tag + "stored output vs the plain instantiation", y16, plain))
        assert bool((y16[..., cout:] == 0).all()), "padded output channels"
        if family == "grid" and zero_group is None:
            pick = EO.sample_images(N)
            res.append(EO.bits("stored output vs float64 convolution, sampled images", y16[pick][..., :cout],
                               EO.conv64(x16, w, case, pick).half()))
        # rows
        res += [(tag + "rows [0, ep_done): elements not written", "bits", int((~torch.isfinite(part[:, :rows])).sum()),
                 groups * rows * 2 * C),
                (tag + "rows [ep_done, cap): elements written", "bits", int((~torch.isnan(part[:, rows:])).sum()),
                 groups * (cap - rows) * 2 * C)]
        sums = EO.group_sums64(y16, groups)
        if family == "grid":
            EO.assert_grid_valid(y16, sums)
        if zero_group is not None:
            assert float(sums[zero_group].abs().max()) == 0.0
        if not expect:
            with _Spy() as spy:
                BatchNorm(g, "bn.", C).forward(y16[:B], True, 0, stat_acc=layer.take_stats(0))
            names = [n for n, _ in spy.calls]          # its own pass: the streaming reduction, or the one-launch form of few rows
            assert names[0] in ("fmri_bn_stats_finalize", "fmri_bn_cols_fwd_s") and "fmri_bn_fold_finalize" not in names, names
            continue
        for gi in range(groups):
            a, b = _fold(part[gi], rows, C)
            res += EO.cmp_stat_sums(family, sums[gi], a, pixels, rows, 4, f"{tag}group {gi} fmri_bn_fold")
            res += EO.cmp_stat_sums(family, sums[gi], b, pixels, rows, 2, f"{tag}group {gi} fmri_bn_fold_finalize")
        # a second launch writes bit-identical rows
        first = part[:, :rows].clone()
        layer.forward(x16, out=y16, bn_groups=groups)
        torch.cuda.synchronize()
        res.append(EO.bits(tag + "rows of a second launch", part[:, :rows], first))
        del x16, plain, y16
    torch.cuda.synchronize()
    print(f"[epilogue] {label} | kernel {kernel}, ep_done = {rows} rows per group of {cap} | wall {time.time() - t0:.2f} s",
          flush=True)
    EO.report(label, res)


@pytest.mark.parametrize("name", list(EO.CAP_CASES), ids=_id)
def test_row_capacity_exact_and_one_row_short(name):
    """fmri_igemm_ep with rows_cap exactly the rows a group needs, and with one row fewer: the second comes back with
    *ep_done = 0, every row untouched and the plain output -- or, where a narrower form needs fewer rows, with that
    form's rows (EO.CAP_CASES)."""
    case, groups = EO.STAT_CASES[name]
    at, below, below_rows = EO.CAP_CASES[name]
    rows = EO.STAT_ROUTES[name][2]
    kind, cin, cout, stride, H, op, N = case
    ops, g, layer, w, seed = _setup(case, "grid", groups)
    C, Ho, B = layer.coutp, EO.out_hw(kind, H, stride, op), N // groups
    gn = B if groups > 1 else 0
    x16 = EO.make_input(case, "grid", seed, DEV, groups)
    plain = layer.forward(x16, out=_out16(N, Ho, Ho, C)[0])
    torch.cuda.synchronize()
    sums = EO.group_sums64(plain, groups)
    EO.assert_grid_valid(plain, sums)
    mode = ops.MODE_CONV if kind == "conv" else ops.MODE_TCONV2
    res = []
    for cap, want_kernel, want_rows in ((rows, at, rows), (rows - 1, below, below_rows)):
        assert EO.route_of(ops, layer, case, cap, gn) == want_kernel
        part, (out, guard) = _nan32(groups, cap, 2, C), _out16(N, Ho, Ho, C)
        r = ops.run_igemm(x16, layer.pw_f, out, None, N, H, H, layer.cinp, Ho, Ho, C, cout, 5, stride, 2, mode, ops.ACT_NONE,
                          False, 1, 0, layer.t_out, stats=(part, cap, gn))
        torch.cuda.synchronize()
        assert r == want_rows, (name, cap, r, want_rows)
        res += [EO.bits(f"cap {cap}: output vs plain", out, plain), _untouched(f"cap {cap}", guard)]
        assert bool(torch.isfinite(part[:, :want_rows]).all()) and bool(torch.isnan(part[:, want_rows:]).all())
        for gi in range(groups if want_rows else 0):
            a, b = _fold(part[gi], want_rows, C)
            res += EO.cmp_stat_sums("grid", sums[gi], a, 0, want_rows, 4, f"cap {cap}: group {gi} fmri_bn_fold")
            res += EO.cmp_stat_sums("grid", sums[gi], b, 0, want_rows, 2, f"cap {cap}: group {gi} fmri_bn_fold_finalize")
    EO.report(f"{name} rows_cap {rows} / {rows - 1}", res)


def test_statistics_and_affine_together_give_statistics():
    """ConvLayer.forward drops the affine request when statistics are asked for (the C ABI rejects the pair:
    tests/test_routing_host.py): rows are written, the output is the plain one, aff_applied is clear."""
    name = "px100 128->256 25px N=3"
    case, groups = EO.STAT_CASES[name]
    kind, cin, cout, stride, H, op, N = case
    ops, g, layer, w, seed = _setup(case, "grid", groups)
    Ho = EO.out_hw(kind, H, stride, op)
    x16 = EO.make_input(case, "grid", seed, DEV)
    plain = layer.forward(x16, out=_out16(N, Ho, Ho, layer.coutp)[0])
    scale, shift = EO.affine_params(layer.coutp, seed, DEV)
    both = layer.forward(x16, out=_out16(N, Ho, Ho, layer.coutp)[0], bn_groups=1, affine=(scale, shift, True))
    torch.cuda.synchronize()
    assert not layer.aff_applied and layer._stat_rows == EO.STAT_ROUTES[name][2] and layer.take_stats(0) is not None
    sums = EO.group_sums64(plain, 1)
    a, _ = _fold(layer.take_stats(0), layer._stat_rows, layer.coutp)
    EO.report(name + " statistics + affine", [EO.bits("output vs plain", both, plain)] +
              EO.cmp_stat_sums("grid", sums[0], a, 0, layer._stat_rows, 4, "fmri_bn_fold"))


# =====================================================================================================================
# 2. the fold kernels on synthetic row matrices
# =====================================================================================================================
def _merge(results):
    """One entry per quantity over the row counts of a loop: differing elements added, ratios maximised."""
    out = {}
    for what, kind, v, n in results:
        k0, v0, n0 = out.get(what, (kind, 0, 0))
        out[what] = (kind, v0 + v if kind == "bits" else max(v0, v), n0 + n)
    return [(what, k, v, n) for what, (k, v, n) in out.items()]


@pytest.mark.parametrize("family", ["grid", "real"])
@pytest.mark.parametrize("C", EO.FOLD_C)
def test_fold_kernels_on_synthetic_rows(C, family):
    """fmri_bn_fold, the sums of fmri_bn_fold_finalize and fmri_bn_bwd_fold over EO.FOLD_ROWS row counts against float64
    column sums (grid: bitwise; real: u D sum |p|).  fmri_bn_bwd_fold: 1 - 4 groups by turns, a capacity of rows + 3 with NaN
    in the rows beyond ``rows``, parameter gradients += gscale x the sums of ``param_group`` on a non-zero prior, and NULL
    gradient pointers."""
    from fmri_hip import lib
    n = 2 * C
    nscr = lib.load().fmri_bn_fold_scratch_floats(C)
    res = []
    for i, rows in enumerate(EO.FOLD_ROWS):
        seed = 1000 * C + rows
        part = EO.fold_rows_input(rows, n, family, seed, DEV)
        a, b = _fold(part[0], rows, C)
        res += EO.cmp_fold(family, part, rows, a.view(1, n), 4, "fmri_bn_fold")
        res += EO.cmp_fold(family, part, rows, b.view(1, n), 2, "fmri_bn_fold_finalize sums")
        G = 1 + i % 4
        pg = (i // 4) % G
        partg = EO.fold_rows_input(rows, n, family, seed + 1, DEV, groups=G, cap=rows + 3)
        gen = torch.Generator().manual_seed(seed)
        prior = (torch.randint(-64, 65, (2, C), generator=gen).float() if family == "grid"
                 else torch.randn(2, C, generator=gen)).to(DEV)
        grads, sums = prior.clone(), _nan32(G, n)
        lib.call("fmri_bn_bwd_fold", _P(partg), rows, rows + 3, C, G, _P(_nan32(G * nscr)), _P(sums), _P(grads[0]),
                 _P(grads[1]), 0.25, pg)
        res += EO.cmp_fold(family, partg, rows, sums, 4, "fmri_bn_bwd_fold sums")
        res += EO.cmp_param_grad(family, sums[pg, :C], prior[0], 0.25, grads[0], "fmri_bn_bwd_fold dbeta")
        res += EO.cmp_param_grad(family, sums[pg, C:], prior[1], 0.25, grads[1], "fmri_bn_bwd_fold dgamma")
        again = _nan32(G, n)
        lib.call("fmri_bn_bwd_fold", _P(partg), rows, rows + 3, C, G, _P(_nan32(G * nscr)), _P(again), None, None, 0.25,
                 pg)
        res.append(EO.bits("fmri_bn_bwd_fold sums, NULL gradient pointers", again, sums))
        torch.cuda.synchronize()
        if not EO.passed(res):
            print(f"[epilogue]   first failure at rows = {rows}: {[r for r in res if not EO.passed([r])]}", flush=True)
            break
    EO.report(f"folds C={C} rows {EO.FOLD_ROWS[0]}..{EO.FOLD_ROWS[-1]} {family}", _merge(res))


@pytest.mark.parametrize("updates", [0, 1, 2])
@pytest.mark.parametrize("count", [1, 7, 65536])
@pytest.mark.parametrize("C,rows", [(8, 1), (40, 33), (1024, 513)])
def test_fold_finalize_outputs(C, rows, count, updates):
    """Everything fmri_bn_fold_finalize derives from the sums -- mean, rstd, scale, shift, running_mean, running_var after
    ``updates`` momentum updates, num_batches_tracked += updates -- against the float64 formula applied to the kernel's OWN
    fp32 sums (EO.finalize64 has the derivation of each bound).  Channels with |mean| up to 1000 std, a zero and a
    constant channel (EO.hard_sums); count = 1 takes the biased variance for the running one."""
    from fmri_hip import lib
    sx, sxx = EO.hard_sums(C, count, 17 * C + count, DEV)
    gen = torch.Generator().manual_seed(C + count)
    share = torch.rand(rows, 1, generator=gen).to(DEV) + 0.5
    part = (torch.cat([sx, sxx]).view(1, 2 * C) * (share / share.sum())).contiguous()
    gamma = (torch.rand(C, generator=gen) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=gen) * 0.2).to(DEV)
    rm0, rv0 = (torch.randn(C, generator=gen) * 0.3).to(DEV), (torch.rand(C, generator=gen) + 0.5).to(DEV)
    rm, rv = rm0.clone(), rv0.clone()
    nbt = torch.full((), 3, dtype=torch.int64, device=DEV)
    sums, out = _nan32(2, C), _nan32(4, C)
    lib.call("fmri_bn_fold_finalize", _P(part), rows, C, _P(_nan32(lib.load().fmri_bn_fold_scratch_floats(C))), _P(sums),
             float(count), _P(gamma), _P(beta), 1e-5, 0.9, updates, _P(rm), _P(rv), _P(out[0]), _P(out[1]), _P(out[2]),
             _P(out[3]), _P(nbt))
    torch.cuda.synchronize()
    assert int(nbt) == 3 + updates
    assert bool(torch.isfinite(sums).all())
    fin = EO.finalize64(sums[0].double(), sums[1].double(), float(count), gamma, beta, updates, rm0, rv0)
    res = [EO.rat(k, out[i], *fin[k]) for i, k in enumerate(("mean", "rstd", "scale", "shift"))]
    if updates:
        res += [EO.rat("running_mean", rm, *fin["running_mean"]), EO.rat("running_var", rv, *fin["running_var"])]
    else:
        res += [EO.bits("running_mean untouched", rm, rm0), EO.bits("running_var untouched", rv, rv0)]
    EO.report(f"fmri_bn_fold_finalize C={C} rows={rows} count={count} updates={updates}", res)


# =====================================================================================================================
# 3. BatchNorm from the rows, end to end
# =====================================================================================================================
@pytest.mark.parametrize("name", EO.BN_CASES, ids=_id)
def test_batchnorm_from_the_rows(name):
    """BatchNorm.forward(raw, stat_acc = take_stats(g)) and forward_groups with a reducer of world size 1 (fmri_bn_fold +
    finalize) against float64 BatchNorm + ReLU of the stored output, every element: one fp16 rounding on top of the
    propagated bound of the statistics (EO.cmp_bn_apply, EO.finalize64).  Running statistics in the given order."""
    from fmri_hip.ops import BatchNorm
    t0 = time.time()
    case, groups = EO.STAT_CASES[name]
    rows = EO.STAT_ROUTES[name][2]
    kind, cin, cout, stride, H, op, N = case
    label = f"{name} BatchNorm from the rows"
    ops, g, layer, w, seed = _setup(case, "real", groups, with_bn=True)
    C, Ho, B = layer.coutp, EO.out_hw(kind, H, stride, op), N // groups
    assert C == cout
    count = B * Ho * Ho
    x16 = EO.make_input(case, "real", seed, DEV, groups)
    raw = layer.forward(x16, out=_out16(N, Ho, Ho, C)[0], bn_groups=groups)
    torch.cuda.synchronize()
    assert layer._stat_rows == rows
    accs = [layer.take_stats(gi) for gi in range(groups)]
    sums = EO.group_sums64(raw, groups)
    bn = BatchNorm(g, "bn.", C)
    rm0, rv0 = g.bufs["bn.running_mean"].clone(), g.bufs["bn.running_var"].clone()
    res = []

    def reference(gi, depth, updates, rm, rv, Brm=0.0, Brv=0.0):
        Bsx, Bsxx = EO.stat_sum_bounds(sums[gi], count, rows, depth)
        return EO.finalize64(sums[gi, 0], sums[gi, 1], float(count), bn.gamma, bn.beta, updates, rm, rv, Bsx, Bsxx, Brm, Brv)

    # (a) forward, one call per group, two momentum updates each from the same start
    for gi in range(groups):
        g.bufs["bn.running_mean"].copy_(rm0)
        g.bufs["bn.running_var"].copy_(rv0)
        with _Spy() as spy:
            y, sv = bn.forward(raw[gi * B:(gi + 1) * B], True, 2, out=_nan16(B, Ho, Ho, C), stat_acc=accs[gi])
        torch.cuda.synchronize()
        assert [n for n, _ in spy.calls] == ["fmri_bn_fold_finalize", "fmri_bn_apply"]
        fin = reference(gi, 2, 2, rm0, rv0)
        res += EO.cmp_bn_apply(f"forward group {gi}: y", raw[gi * B:(gi + 1) * B], y, fin)
        res += [EO.rat(f"forward group {gi}: mean", sv.mean, *fin["mean"]),
                EO.rat(f"forward group {gi}: rstd", sv.rstd, *fin["rstd"]),
                EO.rat(f"forward group {gi}: running_mean", g.bufs["bn.running_mean"], *fin["running_mean"]),
                EO.rat(f"forward group {gi}: running_var", g.bufs["bn.running_var"], *fin["running_var"])]
    # (b) forward_groups behind a reducer (world size 1), running statistics in reversed order
    g.bufs["bn.running_mean"].copy_(rm0)
    g.bufs["bn.running_var"].copy_(rv0)
    nbt0 = int(g.bufs["bn.num_batches_tracked"])
    order = tuple(reversed(range(groups)))
    bn.reducer = lambda t: 1
    outs = [_nan16(B, Ho, Ho, C) for _ in range(groups)]
    with _Spy() as spy:
        svs = bn.forward_groups([raw[gi * B:(gi + 1) * B] for gi in range(groups)], True, 1, outs, accs, order)
    torch.cuda.synchronize()
    names = [n for n, _ in spy.calls]
    assert names.count("fmri_bn_fold") == groups and "fmri_bn_stats" not in names, names
    assert int(g.bufs["bn.num_batches_tracked"]) == nbt0 + groups
    r, Br, s, Bs = rm0, 0.0, rv0, 0.0
    for gi in order:
        fin = reference(gi, 4, 1, r, s, Br, Bs)
        (r, Br), (s, Bs) = fin["running_mean"], fin["running_var"]
        res += EO.cmp_bn_apply(f"forward_groups group {gi}: y", raw[gi * B:(gi + 1) * B], outs[gi], fin)
        res += [EO.rat(f"forward_groups group {gi}: mean", svs[gi].mean, *fin["mean"]),
                EO.rat(f"forward_groups group {gi}: rstd", svs[gi].rstd, *fin["rstd"])]
    res += [EO.rat(f"forward_groups running_mean, order {order}", g.bufs["bn.running_mean"], r, Br),
            EO.rat(f"forward_groups running_var, order {order}", g.bufs["bn.running_var"], s, Bs)]
    print(f"[epilogue] {label} | wall {time.time() - t0:.2f} s", flush=True)
    EO.report(label, res)


# =====================================================================================================================
# 4. eval-mode affine epilogue
# =====================================================================================================================
@pytest.mark.parametrize("name", list(EO.AFFINE_FULL), ids=_id)
def test_affine_epilogue_grid_full_size(name):
    """The eval pass's launches at the step's sizes, grid family: the fused output equals relu?(y scale + shift) of the exact
    plain output bit for bit (scale +-2^k, shift j / 16: exact in fp32 and fp16); kernels without the epilogue say so and
    leave the plain output."""
    t0 = time.time()
    case, kernel, applied = EO.AFFINE_FULL[name]
    kind, cin, cout, stride, H, op, N = case
    label = f"{name} {kind} {cin}->{cout} {H}px N={N} affine grid"
    ops, g, layer, w, seed = _setup(case, "grid", 1)
    C, Ho = layer.coutp, EO.out_hw(kind, H, stride, op)
    assert EO.route_of(ops, layer, case, affine=True) == kernel
    x16 = EO.make_input(case, "grid", seed, DEV)
    plain = layer.forward(x16, out=_out16(N, Ho, Ho, C)[0])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(plain).all()) and bool((plain == plain.round()).all())
    assert 2 * float(plain.abs().max()) + 4 < 128, "grid output too large for an exact affine map"
    pick = EO.sample_images(N)
    res = [EO.bits("plain output vs float64 convolution, sampled images", plain[pick][..., :cout],
                   EO.conv64(x16, w, case, pick).half())]
    scale, shift = EO.affine_params(C, seed, DEV)
    for relu in (True, False):
        fused, guard = _out16(N, Ho, Ho, C)
        with _Spy() as spy:
            layer.forward(x16, out=fused, affine=(scale, shift, relu))
        torch.cuda.synchronize()
        res.append(_untouched(f"relu={relu}", guard))
        _check_launch_args(ops, layer, case, spy.args_of("fmri_igemm_ep")[0])
        assert layer.aff_applied == applied, (label, layer.aff_applied)
        assert bool(torch.isfinite(fused).all())
        assert bool((fused[..., cout:] == 0).all()), "padded output channels"
        want = plain
        if applied:
            want = torch.empty_like(plain)
            for a in range(0, N, 64):
                want[a:a + 64] = EO.affine64(plain[a:a + 64].double(), scale, shift, relu).half()
        res.append(EO.bits(f"fused output, relu={relu}" if applied else f"declined: plain output, relu={relu}", fused, want))
    print(f"[epilogue] {label} | kernel {kernel}, aff_applied = {applied} | wall {time.time() - t0:.2f} s", flush=True)
    EO.report(label, res)


@pytest.mark.parametrize("name", list(EO.AFFINE_SMALL), ids=_id)
def test_affine_epilogue_real_small(name):
    """Real family at the small AFFINE_CASES and partial-tile / odd-N edges against the float64 convolution followed by the
    affine map: ONE fp16 rounding (EO.cmp_affine_real)."""
    case, applied = EO.AFFINE_SMALL[name]
    kind, cin, cout, stride, H, op, N = case
    ops, g, layer, w, seed = _setup(case, "real", 1)
    C, Ho = layer.coutp, EO.out_hw(kind, H, stride, op)
    x16 = EO.make_input(case, "real", seed, DEV)
    gen = torch.Generator().manual_seed(seed)
    scale = ((torch.rand(C, generator=gen) + 0.5) * (torch.randint(0, 4, (C,), generator=gen) > 0).float().mul(2).sub(1)).to(DEV)
    shift = (torch.randn(C, generator=gen) * 0.3).to(DEV)
    plain = layer.forward(x16, out=_out16(N, Ho, Ho, C)[0])
    ref = EO.conv64(x16, w, case) if applied else None
    res = []
    for relu in (True, False):
        fused, guard = _out16(N, Ho, Ho, C)
        layer.forward(x16, out=fused, affine=(scale, shift, relu))
        torch.cuda.synchronize()
        res.append(_untouched(f"relu={relu}", guard))
        assert layer.aff_applied == applied
        assert bool(torch.isfinite(fused).all()) and bool((fused[..., cout:] == 0).all())
        if not applied:
            res.append(EO.bits(f"declined: plain output, relu={relu}", fused, plain))
            continue
        res += EO.cmp_affine_real(f"fused output, relu={relu}", fused[..., :cout], ref, scale[:cout], shift[:cout], relu,
                                  25 * cin)
    EO.report(f"{name} affine real", res)
