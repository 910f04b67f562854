"""CPU checks of tests/glue_oracle.py, the float64 references and bounds of tests/test_glue_kernels_gpu.py:

  * the exactness argument of the grid inputs: numpy float32 sums in forward, reverse and shuffled order all equal the
    float64 sum, at 2^20 rows;
  * the references equal plain float64 numpy / torch of the same operation (fmri_act_bwd: float64 autograd of relu / tanh;
    ingest: the golden-pinned oracle's own float32 result lies inside the fp32 bound of the float64 evaluation);
  * a numpy emulation of each kernel's arithmetic (float32 operations in a kernel-like order, one rounding to fp16) passes
    every check at the shapes and with the inputs the GPU tests use: the bounds are not too tight;
  * the checks reject wrong kernels: eleven corruptions planted in the emulation's output each break a bitwise equality or
    give err / bound > 1.

Every check prints one ``[glue] <case> | <quantity> | ...`` line; profiles/glue_kernels_parity.md records them.
"""
import numpy as np
import pytest
import torch

import glue_oracle as GO
from glue_oracle import F16, F32, f64


def _say(case, results, expect=True):
    for ln in GO.lines(case, results):
        print(ln + ("" if expect else "   (planted fault: must fail)"), flush=True)
    ok = GO.passed(results)
    assert ok == expect, (case, results)
    return results


# ---------------------------------------------------------------------------------------------------------------------
# the exactness argument
# ---------------------------------------------------------------------------------------------------------------------
def test_grid_sums_are_exact_in_any_order():
    """k/8 (|k| <= 4), its square and the tanh terms dy (1 - y^2) of 2^20 rows: float32 sums forward, backward, shuffled
    and in the lane order of the kernels all equal the float64 sum (as do |k| <= 32 at 2047 rows)."""
    for M, C in ((2 ** 20, 8), (2047, 9)):
        y, dy = GO.act_inputs(M, C, GO.ACT_TANH, "grid", 5)
        x = f64(dy)
        for name, t, unit in (("x", x, 0.125), ("x^2", x * x, 2.0 ** -6), ("tanh terms", GO.act_bwd64(y, dy, GO.ACT_TANH), 2.0 ** -5)):
            GO.assert_exact_sums(t, unit)
            want = t.sum(0)
            t32 = t.astype(F32)
            assert np.array_equal(f64(t32), t)
            perm = np.random.RandomState(1).permutation(M)
            for order, v in (("forward", t32), ("reverse", t32[::-1]), ("shuffled", t32[perm])):
                got = np.add.accumulate(v, axis=0, dtype=F32)[-1]            # a strictly sequential float32 sum
                assert np.array_equal(f64(got), want), (M, name, order)
            assert np.array_equal(f64(GO.emu_sum32(t32, GO.act_lanes(M, 8) if C == 8 else 32)), want), (M, name, "lanes")
    with pytest.raises(AssertionError):                                       # the guard itself: |k| <= 32 at 2^20 rows
        GO.assert_exact_sums(np.full((2 ** 20, 1), 4.0), 0.125)


# ---------------------------------------------------------------------------------------------------------------------
# references against plain numpy / torch
# ---------------------------------------------------------------------------------------------------------------------
def test_conversion_references_equal_torch():
    x = GO.conv_values(3 * 9 * 7, 2, as16=False).reshape(3, 9, 7)
    ref = GO.nchw_to_nhwc_ref(x, 16)
    t = torch.zeros(3, 7, 16, dtype=torch.float16)
    t[:, :, :9] = torch.from_numpy(x).permute(0, 2, 1).half()
    assert GO.mismatches(ref, t.numpy()) == 0
    h = GO.conv_values(3 * 7 * 16, 3, as16=True).reshape(3, 7, 16)
    for s in GO.SCALES:
        want = (torch.from_numpy(h)[:, :, :9].float() * torch.tensor(s, dtype=torch.float32)).permute(0, 2, 1).contiguous()
        assert GO.mismatches(GO.nhwc_to_nchw_ref(h, 9, s), want.numpy()) == 0
        r = GO.conv_values(5 * 12, 4, as16=False).reshape(5, 12)
        want = torch.zeros(5, 16, dtype=torch.float16)
        want[:, :12] = (torch.from_numpy(r) * torch.tensor(s, dtype=torch.float32)).half()
        assert GO.mismatches(GO.rows_f32_to_f16_ref(r, 16, s), want.numpy()) == 0
        want = torch.from_numpy(h.reshape(21, 16))[:, :12].float() * torch.tensor(s, dtype=torch.float32)
        assert GO.mismatches(GO.rows_f16_to_f32_ref(h.reshape(21, 16), 12, s), want.numpy()) == 0
    # the cast's overflow rule the GPU test pins: below 65520 -> 65504, from 65520 on -> inf
    with np.errstate(over="ignore"):
        assert F32(65519.99).astype(F16) == F16(65504) and np.isinf(F32(65520.0).astype(F16))


@pytest.mark.parametrize("act", [GO.ACT_NONE, GO.ACT_RELU, GO.ACT_TANH])
def test_act_reference_matches_autograd(act):
    """act_bwd64 takes the activation's OUTPUT y: against float64 autograd of relu / tanh / identity at the pre-activation."""
    rs = np.random.RandomState(act)
    pre = torch.from_numpy(rs.randn(33, 24)).requires_grad_(True)
    dy = rs.randn(33, 24)
    y = {GO.ACT_NONE: lambda t: t * 1.0, GO.ACT_RELU: torch.relu, GO.ACT_TANH: torch.tanh}[act](pre)
    (y * torch.from_numpy(dy)).sum().backward()
    got = GO.act_bwd64(y.detach().numpy(), dy, act)
    assert np.abs(got - pre.grad.numpy()).max() < 1e-14
    assert np.abs(got.sum(0) - pre.grad.sum(0).numpy()).max() < 1e-12


def test_ingest_reference_is_the_golden_oracle():
    """ingest_pixels takes its geometry from oracle/ingest_oracle.py; the oracle's own float32 output lies inside the fp32
    bound around the float64 evaluation (two divisions there, two multiplications by reciprocals in the kernel)."""
    from oracle import ingest_oracle as IO
    for (H, W), C in (((5, 7), 3), ((9, 1), 1), ((64, 64), 3)):
        fl, sh = GO.ingest_shifts(H, W)
        img = GO.ingest_images(len(fl), H, W, C, 3)
        pix = GO.ingest_pixels(img, fl, sh)
        assert pix.min() >= 0 and pix.max() <= 255 and pix.shape == (len(fl), 3, H, W)
        for mean, std in GO.INGEST_STATS:
            p, b = GO.ingest64(pix, mean, std)
            _say(f"host ingest oracle fp32 {H}x{W} C={C} mean={mean}", [GO.rat("oracle fp32", IO.ingest(img, fl, sh, mean, std), p, b)])
    # an unshifted, unflipped image is its own pixels
    img = GO.ingest_images(2, 5, 7, 3, 9)
    assert np.array_equal(GO.ingest_pixels(img, None, None), img.transpose(0, 3, 1, 2))


# ---------------------------------------------------------------------------------------------------------------------
# the emulation stays inside the bounds, at the GPU tests' shapes and inputs
# ---------------------------------------------------------------------------------------------------------------------
def _emu_conv(kind, src, C, Cp, scale):
    s = F32(scale)
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == "nchw_to_nhwc":
            out = np.zeros((src.shape[0], src.shape[2], Cp), F16)
            out[:, :, :C] = src.astype(F16).transpose(0, 2, 1)
            return out
        if kind == "nhwc_to_nchw":
            return (src[:, :, :C].astype(F32) * s).transpose(0, 2, 1).copy()
        if kind == "rows_f32_to_f16":
            out = np.zeros((src.shape[0], Cp), F16)
            out[:, :C] = (src * s).astype(F16)
            return out
        return src[:, :C].astype(F32) * s


def test_emulated_conversions_pass():
    for i, (N, C, HW) in enumerate(GO.IMG_SHAPES + [GO.IMG_CAP]):
        Cp = GO.pad8(C)
        x = GO.conv_values(N * C * HW, i, as16=False).reshape(N, C, HW)
        _say(f"host nchw_to_nhwc N={N} C={C} HW={HW}", GO.cmp_conv(_emu_conv("nchw_to_nhwc", x, C, Cp, 1.0), GO.nchw_to_nhwc_ref(x, Cp), C))
        if (N, C, HW) == GO.IMG_CAP:
            continue
        h = GO.conv_values(N * HW * Cp, i + 100, as16=True).reshape(N, HW, Cp)
        for s in GO.SCALES:
            _say(f"host nhwc_to_nchw N={N} C={C} HW={HW} scale={s:.4g}", GO.cmp_conv(_emu_conv("nhwc_to_nchw", h, C, Cp, s), GO.nhwc_to_nchw_ref(h, C, s)))
    for i, (M, C) in enumerate(GO.ROW_SHAPES + [GO.ROW_CAP]):
        Cp = GO.pad8(C)
        x = GO.conv_values(M * C, i + 200, as16=False).reshape(M, C)
        h = GO.conv_values(M * Cp, i + 300, as16=True).reshape(M, Cp)
        for s in GO.SCALES:
            _say(f"host rows_f32_to_f16 M={M} C={C} scale={s:.4g}", GO.cmp_conv(_emu_conv("rows_f32_to_f16", x, C, Cp, s), GO.rows_f32_to_f16_ref(x, Cp, s), C))
            _say(f"host rows_f16_to_f32 M={M} C={C} scale={s:.4g}", GO.cmp_conv(_emu_conv("rows_f16_to_f32", h, C, Cp, s), GO.rows_f16_to_f32_ref(h, C, s)))


@pytest.mark.parametrize("C", GO.ACT_C + ("big",))
def test_emulated_act_bwd_passes(C):
    rows, C = ([GO.BIG[0]], GO.BIG[1]) if C == "big" else (GO.act_rows(C), C)
    for M in rows:
        for act in (GO.ACT_NONE, GO.ACT_RELU, GO.ACT_TANH):
            if M == GO.BIG[0] and act == GO.ACT_NONE:
                continue                                     # (two activations at the largest shape keep the CPU half short)
            for fam in ("grid", "real"):
                y, dy = GO.act_inputs(M, C, act, fam, 1000 * act + M % 997 + C)
                n = min(3, C)
                gs = 0.5 if fam == "grid" else GO.THIRD
                prior = GO.colsum_prior(C, fam, M + C)
                d16, s, db = GO.emu_act(y, dy, act, GO.act_lanes(M, C), prior, n, gs)
                _say(f"host act_bwd {GO.ACT_NAME[act]} {fam} M={M} C={C}",
                     GO.cmp_act(y, dy, act, fam, d16, s, (db, n), prior, gs))


def test_emulated_colsums_pass():
    for C in GO.CS_C:
        for M in GO.CS_M:
            for fam, scale in (("grid", 0.5), ("real", GO.THIRD)):
                for f16 in (True, False):
                    src = GO.colsum_src(M, C, fam, f16, M * 31 + C)
                    prior = GO.colsum_prior(C + 3, fam, M + C)
                    got = prior.copy()
                    got[:C] = got[:C] + F32(scale) * GO.emu_sum32(src.astype(F32), 32)
                    _say(f"host colsum_acc {fam} {'f16' if f16 else 'f32'} M={M} C={C}", GO.cmp_colsum(src, scale, prior, C, fam, got))
    for M, C in GO.CSR_SHAPES:
        for fam, gs in (("grid", 0.5), ("real", GO.THIRD)):
            x = GO.colsum_src(M, C, fam, True, M % 1009 + C)
            x32 = x.astype(F32)
            lanes = GO.act_lanes(M, C)
            sums = np.stack([GO.emu_sum32(x32, lanes), GO.emu_sum32(x32 * x32, lanes)])
            prior = GO.colsum_prior(C, fam, M % 1009)
            db = prior.copy()
            db[:3] = db[:3] + F32(gs) * sums[0][:3]
            _say(f"host colsum_rows {fam} M={M} C={C}", GO.cmp_colsum_rows(x, fam, sums, db, prior, 3, gs))


def test_emulated_bn_apply_passes():
    for C in GO.BN_C:
        for M in GO.bn_rows(C) + ([GO.BIG[0]] if C == GO.BIG[1] else []):
            x, a, b = GO.bn_inputs(M, C, M % 1013 + C)
            for relu in (0, 1):
                _say(f"host bn_apply M={M} C={C} relu={relu}", GO.cmp_bn(x, a, b, relu, GO.emu_bn(x, a, b, relu)))


def test_emulated_ingest_passes():
    for H, W in GO.INGEST_HW:
        for C in (1, 3):
            fl, sh = GO.ingest_shifts(H, W)
            img = GO.ingest_images(len(fl), H, W, C, H * 10 + W + C)
            pix = GO.ingest_pixels(img, fl, sh)
            for mean, std in GO.INGEST_STATS:
                o16, o32 = GO.emu_ingest(img, fl, sh, mean, std)
                _say(f"host ingest {H}x{W} C={C} mean={mean}", GO.cmp_ingest(pix, mean, std, o16, o32))


def test_emulated_scalars_and_mixing_pass():
    rs = np.random.RandomState(0)
    for n in (8, 2048, 70000):
        x = GO.sumsq_inputs(n, n)
        _say(f"host sumsq n={n}", GO.cmp_sumsq(x, 3.25, np.array([F32(3.25) + GO.emu_sum32((x * x).reshape(-1, 1), 256)[0]], F32)))
        xr = (rs.randn(n) * 3).astype(F32)
        ss, cnt, fin, scale = float(np.sum(f64(xr) ** 2)), 7.0, 0.37, 0.25
        f = F32(1) / max(F32(np.sqrt(ss / cnt)), F32(1e-20))
        _say(f"host renorm n={n}", GO.cmp_renorm(xr, scale, ss, cnt, fin, (xr * (f * F32(scale))).astype(F16), F32(fin) * f))
        xh, yh = rs.randn(n).astype(F16), rs.randn(n).astype(F16)
        a, pa, b = F32(0.75), F32(GO.THIRD), F32(-1.3)
        aa = a * pa
        _say(f"host axpby n={n}", GO.cmp_axpby(xh, yh, a, pa, b, (aa * xh.astype(F32) + b * yh.astype(F32)).astype(F16)))
        _say(f"host axpby y=None n={n}", GO.cmp_axpby(xh, None, a, pa, 0.0, (aa * xh.astype(F32)).astype(F16)))
    # the 1e-20 floor
    z = np.zeros(16, F32)
    f = F32(1) / F32(1e-20)
    _say("host renorm all-zero", GO.cmp_renorm(z, 0.25, 0.0, 16.0, 0.5, (z * (f * F32(0.25))).astype(F16), F32(0.5) * f))
    assert GO.absmax_ref(np.array([1.0, np.nan, -3.0, -0.0], F32), 2.0)[0] == 3.0
    assert GO.absmax_ref(np.array([np.nan], F32), 2.0)[0] == 2.0 and np.isinf(GO.absmax_ref(np.array([-np.inf, 1], F32), 0.0)[0])


# ---------------------------------------------------------------------------------------------------------------------
# the checks reject wrong kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_planted_conversion_faults_fail():
    """1. one element one fp16 ulp off;  2. one padded lane non-zero."""
    M, C, Cp = 257, 12, 16
    x = GO.conv_values(M * C, 7, as16=False).reshape(M, C)
    ref = GO.rows_f32_to_f16_ref(x, Cp, GO.THIRD)
    good = _emu_conv("rows_f32_to_f16", x, C, Cp, GO.THIRD)
    _say("host fault none", GO.cmp_conv(good, ref, C))
    bad = good.copy()
    bad.view(np.uint16)[100, 5] += 1                                      # the neighbouring fp16 value
    assert np.isfinite(good[100, 5])
    _say("host fault 1: one fp16 ulp", GO.cmp_conv(bad, ref, C), expect=False)
    bad = good.copy()
    bad.view(np.uint16)[256, 13] = 1                                      # the smallest subnormal in a padded lane
    _say("host fault 2: padded lane", GO.cmp_conv(bad, ref, C), expect=False)
    x = GO.conv_values(3 * 9 * 7, 8, as16=False).reshape(3, 9, 7)
    bad = _emu_conv("nchw_to_nhwc", x, 9, 16, 1.0)
    bad[2, 6, 15] = -0.0                                                  # even a negative zero
    _say("host fault 2: padded channel -0", GO.cmp_conv(bad, GO.nchw_to_nhwc_ref(x, 16), 9), expect=False)


def test_planted_sum_faults_fail():
    """3. one row of 2^20 dropped from a column sum;  4. one row counted twice (exact-grid inputs, C = 8)."""
    M, C = 2 ** 20, 8
    x = GO.colsum_src(M, C, "grid", True, 11)
    x32 = x.astype(F32)
    row = int(np.argmax(np.all(x32 != 0, axis=1)))                       # a row without a zero: every column notices
    prior = GO.colsum_prior(C, "grid", 1)
    for name, delta in (("3: a row dropped", -1), ("4: a row doubled", +1)):
        t = x32.copy() if delta < 0 else np.concatenate([x32, x32[row:row + 1]])
        if delta < 0:
            t[row] = 0
        s = np.stack([GO.emu_sum32(t, 65536), GO.emu_sum32(t * t, 65536)])
        db = prior.copy()
        db[:3] = db[:3] + F32(0.5) * s[0][:3]
        res = _say(f"host fault {name} (colsum_rows)", GO.cmp_colsum_rows(x, "grid", s, db, prior, 3, 0.5), expect=False)
        assert all(v == (C if w != "dbias" else 3) for w, _, v, _ in res), res           # every column, both halves
    # the same two faults in fmri_act_bwd's column sums
    y, dy = GO.act_inputs(M, C, GO.ACT_TANH, "grid", 12)
    d16, s, _ = GO.emu_act(y, dy, GO.ACT_TANH, 65536)
    g = GO.act_bwd64(y, dy, GO.ACT_TANH)
    row = int(np.argmax(np.all(g != 0, axis=1)))
    for name, sgn in (("3: a row dropped", -1.0), ("4: a row doubled", 1.0)):
        _say(f"host fault {name} (act_bwd tanh)", GO.cmp_act(y, dy, GO.ACT_TANH, "grid", d16, (f64(s) + sgn * g[row]).astype(F32)), expect=False)


def test_planted_act_faults_fail():
    """5. ReLU mask on >=;  6. tanh' as 1 - y;  7. dbias folded without gscale."""
    M, C = 129, 64
    for fam in ("grid", "real"):
        y, dy = GO.act_inputs(M, C, GO.ACT_RELU, fam, 21)
        d16, s, _ = GO.emu_act(y, dy, GO.ACT_RELU, 32, relu_ge=True)
        res = _say(f"host fault 5: relu >= ({fam})", GO.cmp_act(y, dy, GO.ACT_RELU, fam, d16, s), expect=False)
        assert res[0][2] > 0                                              # dpre itself, not only the sums
        y, dy = GO.act_inputs(M, C, GO.ACT_TANH, fam, 22)
        d16, s, _ = GO.emu_act(y, dy, GO.ACT_TANH, 32, tanh_1my=True)
        _say(f"host fault 6: tanh' = 1 - y ({fam})", GO.cmp_act(y, dy, GO.ACT_TANH, fam, d16, s), expect=False)
        gs = 0.5 if fam == "grid" else GO.THIRD
        prior = GO.colsum_prior(C, fam, 3)
        d16, s, db = GO.emu_act(y, dy, GO.ACT_TANH, 32, prior, 3, gs, no_gscale=True)
        res = _say(f"host fault 7: dbias without gscale ({fam})", GO.cmp_act(y, dy, GO.ACT_TANH, fam, d16, s, (db, 3), prior, gs), expect=False)
        assert GO.passed(res[:2]) and not GO.passed(res[2:])              # only the dbias check objects
        # and a dbias folded past dbias_n
        d16, s, db = GO.emu_act(y, dy, GO.ACT_TANH, 32, prior, 4, gs)
        _say(f"host fault 7b: dbias written behind dbias_n ({fam})", GO.cmp_act(y, dy, GO.ACT_TANH, fam, d16, s, (db, 3), prior, gs), expect=False)


def test_planted_ingest_faults_fail():
    """8. shift before flip;  9. shift sign reversed;  10. edge clamp off by one;  11. the last sweep left unwritten."""
    H, W, C = 5, 7, 3
    fl, sh = GO.ingest_shifts(H, W)
    img = GO.ingest_images(len(fl), H, W, C, 31)
    pix = GO.ingest_pixels(img, fl, sh)
    mean, std = GO.INGEST_STATS[1]
    _say("host fault none (ingest)", GO.cmp_ingest(pix, mean, std, *GO.emu_ingest(img, fl, sh, mean, std)))
    for name, kw in (("8: shift before flip", dict(shift_first=True)), ("9: shift sign reversed", dict(sign=-1)),
                     ("10: clamp off by one", dict(clamp_off=1)), ("11: last sweep unwritten", dict(sweep_items=len(fl) * H * W - 3))):
        res = _say(f"host fault {name}", GO.cmp_ingest(pix, mean, std, *GO.emu_ingest(img, fl, sh, mean, std, **kw)), expect=False)
        assert res[0][2] > 1 and res[1][2] > 1                             # the fp32 and the fp16 output both
    # fault 8 shows on the flipped images with a column shift only -- and is told from the right order on every one of them
    o16, o32 = GO.emu_ingest(img, fl, sh, mean, std, shift_first=True)
    p, b = GO.ingest64(pix, mean, std)
    wrong = (np.abs(f64(o32) - p) > b).reshape(len(fl), -1).any(1)
    assert np.array_equal(wrong, (fl == 1) & (sh[:, 1] != 0))
    # fault 11 at the batch past the block cap: one pixel of the second sweep
    N, H, W = GO.INGEST_CAP
    img = GO.ingest_images(N, H, W, 1, 32)
    fl = (np.arange(N) % 2).astype(np.int32)
    sh = np.stack([np.arange(N) % 9 - 4, np.arange(N) % 7 - 3], 1).astype(np.int32)
    pix = GO.ingest_pixels(img, fl, sh)
    _say("host fault 11: second sweep (65 x 128 x 128)",
         GO.cmp_ingest(pix, mean, std, *GO.emu_ingest(img, fl, sh, mean, std, sweep_items=N * H * W - 1)), expect=False)
