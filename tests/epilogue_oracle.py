"""TEST INFRASTRUCTURE ONLY -- what tests/test_epilogue_oracle_host.py and tests/test_conv_epilogues_gpu.py share: the
cases, the route table, the seeded inputs, the float64 restatements and the bounds of the checks on

  * the BatchNorm-statistics epilogue of the contraction kernels (fmri_igemm_ep with fmri_epilogue.stat_part: StatEpi),
  * the folds of its rows (fmri_bn_fold, fmri_bn_fold_finalize, fmri_bn_bwd_fold; csrc/norm.hip fold_columns),
  * BatchNorm.forward from those rows, and
  * the eval-mode affine epilogue (fmri_epilogue.aff_*).

Nothing here imports the library under test; functions that need it take the module as an argument.  Everything is torch
float64 on whatever device the operands live on (tests/conv_oracle.py is the convolution).

The epilogue sums the STORED, fp16-rounded outputs, so the reference of its sums is the float64 column sum of the tensor
the kernel itself wrote: no float64 convolution is needed and the step's sizes cost milliseconds.

Two input families (the convention of tests/glue_oracle.py):
  * grid: x in {-1, 0, 1} with P(x != 0) = 1/4, w in {-1, 0, 1} with density 8 / (25 cin) and at least one non-zero tap
    per output channel.  Outputs are small integers; ``assert_grid_valid`` checks from float64 sums of the stored output
    that max |y| <= 2048 and that sum |y| and sum y^2 are below 2^24 per channel and group.  Every partial sum of the
    epilogue and of the folds, in any order, is then an integer below 2^24, exact in fp32, and the comparison is bitwise
    (kind "bits": the number of differing elements, which must be 0).  The plain output is exact too (integer products,
    fp32 accumulation below 2^24, an exact fp16 conversion) and so is a map y * (+-2^k) + j / 16 below 128.
  * real: fp16-rounded normals, checked against bounds from the number formats (u = 2^-24), derived below where used.

One printed line per check: ``[epilogue] <case> | <quantity> | err/bound = r`` (r > 1 fails) or
``[epilogue] <case> | <quantity> | bitwise: k of n differ`` (k > 0 fails).
"""
import math

import torch

U = 2.0 ** -24
H16 = 2.0 ** -11
SUB16 = 2.0 ** -25
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))          # the eps every caller passes, as the C ABI receives it
MOM32 = float(torch.tensor(0.9, dtype=torch.float32))
K5, PAD = 5, 2
LIMIT = 2.0 ** 24


def pad8(c):
    return (c + 7) // 8 * 8


def out_hw(kind, H, stride, op):
    return (H + 2 * PAD - K5) // stride + 1 if kind == "conv" else (H - 1) * 2 - 2 * PAD + K5 + op


# =====================================================================================================================
# cases
# =====================================================================================================================
# name -> ((kind, cin, cout, stride, H, out_pad, N), BatchNorm groups).  The FULL_SIZE rows of tests/test_kernels_gpu.py
# whose layer feeds a train-mode BatchNorm, with the group count the step uses (fmri_hip/nets.py: ConvStack and the
# discriminator ask for 1 group, the decoder for its call groups -- 2 in the Stage-I and WAE steps, 1 and 3 in Stages
# II / III; no step stacks 4 decoder calls, so there is no 4-group row).
STAT_FULL = {
    "discriminator.conv.1": (("conv", 32, 128, 2, 64, 0, 768), 1),
    "discriminator.conv.2": (("conv", 128, 256, 2, 32, 0, 768), 1),
    "discriminator.conv.3": (("conv", 256, 256, 2, 16, 0, 768), 1),
    "encoder.conv.0": (("conv", 3, 64, 2, 64, 0, 256), 1),
    "encoder.conv.1": (("conv", 64, 128, 2, 32, 0, 256), 1),
    "encoder.conv.2": (("conv", 128, 256, 2, 16, 0, 256), 1),
    "decoder.conv.0": (("deconv", 256, 256, 2, 8, 1, 512), 2),
    "decoder.conv.1": (("deconv", 256, 128, 2, 16, 1, 512), 2),
    "decoder.conv.2": (("deconv", 128, 32, 2, 32, 1, 512), 2),
    "encoder.conv.0 @128": (("conv", 3, 64, 2, 128, 0, 128), 1),
    "encoder.conv.1 @128": (("conv", 64, 128, 2, 64, 0, 128), 1),
    "encoder.conv.2 @128": (("conv", 128, 256, 2, 32, 0, 128), 1),
    "decoder.conv.0 @128": (("deconv", 256, 256, 2, 16, 1, 128), 2),
    "decoder.conv.1 @128": (("deconv", 256, 128, 2, 32, 1, 128), 2),
    "decoder.conv.2 @128": (("deconv", 128, 32, 2, 64, 1, 128), 2),
    "decoder.conv.1 groups=1": (("deconv", 256, 128, 2, 16, 1, 512), 1),      # Stage II / III: one decoder call
    "decoder.conv.1 groups=3": (("deconv", 256, 128, 2, 16, 1, 384), 3),      # Stage II with three call groups of 128
}
# the cheap geometries of EPI_STAT_CASES (tests/test_kernels_gpu.py) restated, plus N = 1
STAT_EDGE = {
    "px100 3->64 100px N=3": (("conv", 3, 64, 2, 100, 0, 3), 1),              # generic kernel, 100 -> 50, odd N
    "px100 64->128 50px N=2 g=2": (("conv", 64, 128, 2, 50, 0, 2), 2),       # 50 -> 25, two groups of one image
    "px100 128->256 25px N=3": (("conv", 128, 256, 2, 25, 0, 3), 1),         # 25 -> 13, partial tiles, odd N
    "px100 256->256 13px N=3 deconv": (("deconv", 256, 256, 2, 13, 0, 3), 1),    # 13 -> 25, output_padding 0
    "px100 128->64 25px N=2 g=2 deconv": (("deconv", 128, 64, 2, 25, 1, 2), 2),  # 25 -> 50, 64-channel tile
    "one tile per group conv": (("conv", 256, 256, 2, 16, 0, 6), 3),          # three groups of two images = one tile each
    "one tile per group deconv": (("deconv", 256, 256, 2, 8, 1, 8), 2),       # four images per tile = one tile per group
    "straddle conv": (("conv", 256, 256, 2, 16, 0, 3), 3),                    # a two-image tile would hold two groups
    "straddle deconv": (("deconv", 256, 256, 2, 8, 1, 6), 2),                 # a tile would hold images of two groups
    "N=1 conv": (("conv", 128, 256, 2, 32, 0, 1), 1),
    "N=1 deconv": (("deconv", 256, 128, 2, 16, 1, 1), 1),
    "solo classes deconv N=12 g=3": (("deconv", 128, 128, 2, 32, 1, 12), 3),  # one parity class per block, four rows a tile
}
STAT_CASES = {**STAT_FULL, **STAT_EDGE}

# name -> (kernel instantiation fmri_igemm_route names for the statistics request, epilogue expected, rows per group).
# A declined request (decoder.conv.2: igemm_tc32 has no statistics epilogue; the straddle cases) names the plain
# instantiation, writes no row and leaves BatchNorm to its own pass.  The generic kernel (igemm_kernel) keeps one
# name with and without the epilogue: there the rows tell.
STAT_ROUTES = {
    "discriminator.conv.1": ("fmri::igemm_c5w_kernel<16,1>", True, 256),
    "discriminator.conv.2": ("fmri::igemm_c5w_kernel<16,1>", True, 128),
    "discriminator.conv.3": ("fmri::igemm_c5w_kernel<8,1>", True, 192),
    "encoder.conv.0": ("fmri::igemm_kernel<128,64,2,2,false,false>", True, 2048),
    "encoder.conv.1": ("fmri::igemm_c5w_kernel<16,1>", True, 256),
    "encoder.conv.2": ("fmri::igemm_c5w_kernel<8,1>", True, 64),
    "decoder.conv.0": ("fmri::igemm_tc5w_kernel<8,1,false>", True, 64),
    "decoder.conv.1": ("fmri::igemm_tc5w_kernel<16,1,false>", True, 256),
    "decoder.conv.2": ("fmri::igemm_tc32_kernel<false>", False, 0),
    "encoder.conv.0 @128": ("fmri::igemm_kernel<128,64,2,2,false,false>", True, 4096),
    "encoder.conv.1 @128": ("fmri::igemm_c5w_kernel<16,1>", True, 256),
    "encoder.conv.2 @128": ("fmri::igemm_c5w_kernel<16,1>", True, 128),
    "decoder.conv.0 @128": ("fmri::igemm_tc5w_kernel<16,1,false>", True, 64),
    "decoder.conv.1 @128": ("fmri::igemm_tc5w_kernel<16,1,false>", True, 256),
    "decoder.conv.2 @128": ("fmri::igemm_tc32_kernel<false>", False, 0),
    "decoder.conv.1 groups=1": ("fmri::igemm_tc5w_kernel<16,1,false>", True, 512),
    "decoder.conv.1 groups=3": ("fmri::igemm_tc5w_kernel<16,1,false>", True, 128),
    "px100 3->64 100px N=3": ("fmri::igemm_kernel<128,64,2,2,false,false>", True, 59),
    "px100 64->128 50px N=2 g=2": ("fmri::igemm_c5w_kernel<16,1>", True, 4),
    "px100 128->256 25px N=3": ("fmri::igemm_c5w_kernel<16,1>", True, 3),
    "px100 256->256 13px N=3 deconv": ("fmri::igemm_tc5w_kernel<16,1,true>", True, 12),
    "px100 128->64 25px N=2 g=2 deconv": ("fmri::igemm_tc5_kernel<64,6,1>", True, 8),
    "one tile per group conv": ("fmri::igemm_c5_kernel<8,1>", True, 1),
    "one tile per group deconv": ("fmri::igemm_tc5w_kernel<8,1,true>", True, 4),
    "straddle conv": ("fmri::igemm_c5_kernel<8,0>", False, 0),
    "straddle deconv": ("fmri::igemm_tc5_kernel<128,4,0>", False, 0),
    "N=1 conv": ("fmri::igemm_c5w_kernel<16,1>", True, 1),
    "N=1 deconv": ("fmri::igemm_tc5w_kernel<16,1,true>", True, 4),
    "solo classes deconv N=12 g=3": ("fmri::igemm_tc5w_kernel<16,1,true>", True, 64),
}

# rows_cap exactly the rows a group needs, and one fewer: name of a STAT_CASES row -> (kernel at cap = rows, kernel at
# cap = rows - 1, rows written at cap = rows - 1).  The first three must come back with *ep_done = 0, every row
# untouched and the plain output (the generic kernel's name does not show its epilogue); the wide transposed form
# hands the call to the narrow one, whose 8 x 16 tiles need 6 rows.
CAP_CASES = {
    "px100 128->256 25px N=3": ("fmri::igemm_c5w_kernel<16,1>", "fmri::igemm_c5_kernel<16,0>", 0),
    "px100 128->64 25px N=2 g=2 deconv": ("fmri::igemm_tc5_kernel<64,6,1>", "fmri::igemm_tc5_kernel<64,6,0>", 0),
    "px100 3->64 100px N=3": ("fmri::igemm_kernel<128,64,2,2,false,false>", "fmri::igemm_kernel<128,64,2,2,false,false>", 0),
    "px100 256->256 13px N=3 deconv": ("fmri::igemm_tc5w_kernel<16,1,true>", "fmri::igemm_tc5_kernel<128,6,1>", 6),
}

# BatchNorm from the rows, end to end: one c5w case, one tc5w case with two groups, the generic kernel
BN_CASES = ("discriminator.conv.2", "decoder.conv.1", "encoder.conv.0")

# eval-mode affine epilogue, grid family at the step's sizes: name -> (case, kernel with the affine request, applied)
AFFINE_FULL = {
    "discriminator.conv.1": (("conv", 32, 128, 2, 64, 0, 768), "fmri::igemm_c5w_kernel<16,0>", True),
    "discriminator.conv.2": (("conv", 128, 256, 2, 32, 0, 768), "fmri::igemm_c5w_kernel<16,0>", True),
    "discriminator.conv.3": (("conv", 256, 256, 2, 16, 0, 768), "fmri::igemm_c5w_kernel<8,0>", True),
    "encoder.conv.0": (("conv", 3, 64, 2, 64, 0, 256), "fmri::igemm_kernel<128,64,2,2,false,false>", False),
    "encoder.conv.1": (("conv", 64, 128, 2, 32, 0, 256), "fmri::igemm_c5w_kernel<16,0>", True),
    "encoder.conv.2": (("conv", 128, 256, 2, 16, 0, 256), "fmri::igemm_c5w_kernel<8,0>", True),
    "decoder.conv.0": (("deconv", 256, 256, 2, 8, 1, 512), "fmri::igemm_tc5w_kernel<8,0,false>", True),
    "decoder.conv.1": (("deconv", 256, 128, 2, 16, 1, 512), "fmri::igemm_tc5w_kernel<16,0,false>", True),
    "decoder.conv.2": (("deconv", 128, 32, 2, 32, 1, 512), "fmri::igemm_tc32_kernel<false>", False),
    "encoder.conv.1 @128": (("conv", 64, 128, 2, 64, 0, 128), "fmri::igemm_c5w_kernel<16,0>", True),
    "decoder.conv.0 @128": (("deconv", 256, 256, 2, 16, 1, 128), "fmri::igemm_tc5w_kernel<16,0,false>", True),
    "decoder.conv.1 @128": (("deconv", 256, 128, 2, 32, 1, 128), "fmri::igemm_tc5w_kernel<16,0,false>", True),
}
# real family: AFFINE_CASES of tests/test_kernels_gpu.py (kind, cin, cout, H, out_pad, N, expect) as full case tuples,
# plus partial-tile and odd-N edges
AFFINE_SMALL = {
    "128->256 32px N=3": (("conv", 128, 256, 2, 32, 0, 3), True),
    "256->256 16px N=5": (("conv", 256, 256, 2, 16, 0, 5), True),
    "32->128 20px N=2": (("conv", 32, 128, 2, 20, 0, 2), True),
    "256->128 16px N=2 deconv": (("deconv", 256, 128, 2, 16, 1, 2), True),
    "256->256 8px N=6 deconv": (("deconv", 256, 256, 2, 8, 1, 6), True),
    "128->32 16px N=2 deconv": (("deconv", 128, 32, 2, 16, 1, 2), False),
    "128->256 25px N=3": (("conv", 128, 256, 2, 25, 0, 3), True),             # 13 x 13 outputs: partial 16 x 16 tile
    "256->256 13px N=1": (("conv", 256, 256, 2, 13, 0, 1), True),             # 7 x 7 outputs, three empty tile slots
    "256->256 13px N=3 deconv": (("deconv", 256, 256, 2, 13, 0, 3), True),    # 25 x 25 outputs, output_padding 0
    "256->256 7px N=7 deconv": (("deconv", 256, 256, 2, 7, 0, 7), True),      # 13 x 13 outputs, 7 images in 4-image tiles
}

# rows of the direct fold tests: the row-lane count (32), the four-deep unroll (128), the switch to two stages (512),
# fewer than 32 stage-1 blocks (513: 17 rows per block -> 31 blocks), the largest capacity a step allocates
# (768 * 32 * 32 / 128 + 8)
FOLD_ROWS = (1, 2, 31, 32, 33, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 6152)
FOLD_C = (8, 24, 32, 40, 256, 1024)
FOLD_STAGE_ROWS = 32
FOLD_SWITCH = 512


class Group:
    """Minimal FlatGroup stand-in for single-layer tests (as ``_G`` of tests/test_kernels_gpu.py), on any device."""

    def __init__(self, tensors, device, bufs=None):
        self.views = {k: v.to(device).contiguous() for k, v in tensors.items()}
        self.grads = {k: torch.zeros_like(v) for k, v in self.views.items()}
        self.bufs = {k: v.to(device) for k, v in (bufs or {}).items()}
        self.version = 0
        self.device = torch.device(device)


def bn_group(weights, C, device, seed):
    """``weights`` plus BatchNorm parameters and NON-trivial running statistics for C channels."""
    g = torch.Generator().manual_seed(seed)
    t = dict(weights)
    t["bn.weight"] = torch.rand(C, generator=g) + 0.5
    t["bn.bias"] = torch.randn(C, generator=g) * 0.2
    bufs = {"bn.running_mean": torch.randn(C, generator=g) * 0.3, "bn.running_var": torch.rand(C, generator=g) + 0.5,
            "bn.num_batches_tracked": torch.full((), 3, dtype=torch.int64)}
    return Group(t, device, bufs)


def make_layer(ops, group, case):
    kind, cin, cout, stride, H, op, N = case
    return ops.ConvLayer(group, "w", None, kind, cin, cout, K5, stride, PAD, op)


def route_of(ops, layer, case, rows_cap=0, group_n=0, affine=False):
    """The kernel instantiation behind ``layer.forward`` for this case, asked of the library (fmri_igemm_route: host code)."""
    kind, cin, cout, stride, H, op, N = case
    Ho = out_hw(kind, H, stride, op)
    return ops.igemm_route(N, H, H, layer.cinp, Ho, Ho, layer.coutp, layer.cout, K5, stride, PAD,
                           ops.MODE_CONV if kind == "conv" else ops.MODE_TCONV2, ops.ACT_NONE, False, 1, layer.t_out,
                           layer.pw_f.buf.numel(), stat_rows_cap=rows_cap, stat_group_n=group_n, want_affine=affine)


def usual_cap(case, groups):
    """Row capacity per group ConvLayer.forward allocates (N Ho Wo / 128 + 8 rows per group always suffice)."""
    kind, cin, cout, stride, H, op, N = case
    Ho = out_hw(kind, H, stride, op)
    return (N // groups) * Ho * Ho // 128 + 8


# =====================================================================================================================
# inputs
# =====================================================================================================================
def case_seed(case, groups=1):
    kind, cin, cout, stride, H, op, N = case
    return cin * 7 + cout * 3 + H * 5 + N + 1000 * groups + (0 if kind == "conv" else 500000)


def weight_shape(case):
    kind, cin, cout = case[:3]
    return (cout, cin, K5, K5) if kind == "conv" else (cin, cout, K5, K5)


def grid_weight(case, seed):
    """fp32 weight in {-1, 0, 1}, density 8 / (25 cin), at least one non-zero tap per output channel (CPU tensor)."""
    kind, cin, cout = case[:3]
    g = torch.Generator().manual_seed(seed)
    shape = weight_shape(case)
    nz = torch.rand(shape, generator=g) < 8.0 / (25.0 * cin)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    w = (nz * sign).float()
    co_axis = 0 if kind == "conv" else 1
    per = w.abs().sum([a for a in range(4) if a != co_axis])
    for co in torch.nonzero(per == 0).flatten().tolist():
        idx = [co % cin, co % cin, 2, 2]          # the centre tap of input channel co mod cin
        idx[co_axis] = co
        w[tuple(idx)] = 1.0
    return w


def real_weight(case, seed):
    cin = case[1]
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(weight_shape(case), generator=g) * (1.0 / (5.0 * cin ** 0.5))).half().float()


def make_input(case, family, seed, device, groups=1, zero_group=None):
    """x16 [N][H][H][cinp] fp16, pad channels zero.  With more than one group the groups get visibly different inputs:
    group 1 is scaled by 2 (exact in fp16), and ``zero_group`` is all zero."""
    kind, cin, cout, stride, H, op, N = case
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.zeros(N, H, H, pad8(cin), dtype=torch.float16, device=device)
    if family == "grid":
        r = torch.randint(0, 8, (N, H, H, cin), generator=g, device=device)
        x[..., :cin] = ((r == 0).to(torch.float16) - (r == 1).to(torch.float16))
    else:
        x[..., :cin] = torch.randn(N, H, H, cin, generator=g, device=device).half()
    B = N // groups
    if groups > 1:
        x[B:2 * B] *= 2
    if zero_group is not None:
        x[zero_group * B:(zero_group + 1) * B] = 0
    return x


def conv64(x16, w, case, images=None):
    """float64 convolution of (some images of) x16 with the fp32 weight w: tests/conv_oracle.py."""
    import conv_oracle as CO
    kind, cin, cout, stride, H, op, N = case
    x = x16[..., :cin] if images is None else x16[images][..., :cin]
    w64 = w.to(x16.device).double()
    if kind == "conv":
        return CO.conv_fwd(x, w64, stride, PAD, 16)
    return CO.deconv_fwd(x, w64, 2, PAD, op, 16)


def sample_images(N):
    return sorted({0, N // 2, N - 1})


# =====================================================================================================================
# checks
# =====================================================================================================================
def bits(what, got, ref):
    """Number of elements whose bits differ (NaN equals NaN; +0 and -0 differ)."""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    it = {2: torch.int16, 4: torch.int32}[got.element_size()]
    gn, rn = torch.isnan(got), torch.isnan(ref)
    bad = (gn != rn) | (~gn & ~rn & (got.contiguous().view(it) != ref.contiguous().view(it)))
    n = int(bad.sum())
    if n:
        idx = torch.nonzero(bad)[:4]
        first = [(tuple(int(v) for v in i), float(got[tuple(i)]), float(ref[tuple(i)])) for i in idx]
        print(f"[epilogue]   {what}: first differences (index, got, reference): {first}", flush=True)
    return (what, "bits", n, int(ref.numel()))


def rat(what, got, ref, bound):
    """max err / bound over every element (an error with a zero bound is an infinite ratio)."""
    got = got.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not bool(torch.isfinite(got).all()):
        return (what, "ratio", float("inf"), int(ref.numel()))
    err = (got - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64, device=err.device).expand_as(err)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return (what, "ratio", float(r.max()) if r.numel() else 0.0, int(ref.numel()))


def passed(results):
    return all((v == 0) if kind == "bits" else (v <= 1.0) for _, kind, v, _ in results)


def lines(case, results):
    out = []
    for what, kind, v, n in results:
        if kind == "bits":
            out.append(f"[epilogue] {case} | {what} | bitwise: {v} of {n} differ")
        else:
            out.append(f"[epilogue] {case} | {what} | err/bound = {v:.4f}")
    return out


def report(case, results):
    """Print every line, then assert: the figures of a failing check are on the output before the assertion fires."""
    for ln in lines(case, results):
        print(ln, flush=True)
    bad = [(w, k, v) for w, k, v, _ in results if (v != 0 if k == "bits" else not v <= 1.0)]
    assert not bad, f"{case}: {bad}"


# =====================================================================================================================
# statistics of the stored output
# =====================================================================================================================
def group_sums64(y16, groups, chunk=1 << 20):
    """float64 [groups][3][C]: sum y, sum y^2, sum |y| over the images of each group of the STORED output y16 [N]...[C]."""
    C = y16.shape[-1]
    rows = y16.reshape(groups, -1, C)
    out = torch.zeros(groups, 3, C, dtype=torch.float64, device=y16.device)
    for g in range(groups):
        for a in range(0, rows.shape[1], chunk):
            v = rows[g, a:a + chunk].double()
            out[g, 0] += v.sum(0)
            out[g, 1] += (v * v).sum(0)
            out[g, 2] += v.abs().sum(0)
    return out


def assert_grid_valid(y16, sums):
    """Validity of a grid input (a check on the INPUT, not on the kernel): every partial sum the epilogue and the folds can
    form is an integer below 2^24."""
    assert bool((y16 == y16.round()).all()), "grid output off the integers"
    assert float(y16.abs().max()) <= 2048.0, "grid output beyond fp16's exact integers"
    assert float(sums[:, 2].max()) < LIMIT, "sum |y| of a channel could leave fp32's exact range"
    assert float(sums[:, 1].max()) < LIMIT, "sum y^2 of a channel could leave fp32's exact range"


def fold_chain(rows, depth):
    """Longest addition chain of one pass of fold_columns<DEPTH> over ``rows`` rows (csrc/norm.hip): row lane 0 takes
    ceil(rows / 32) rows, DEPTH accumulators by turns with the remainder on accumulator 0, then the pairwise sum of the
    accumulators, then the 32 lane sums added in turn."""
    mine = (rows + 31) // 32
    return mine // depth + mine % depth + int(math.log2(depth)) + 32


def fold_chains(rows, depth):
    """Chain of the whole fold: more than 512 rows go through stage 1 (blocks of ceil(rows / 32) rows, DEPTH 4) and the
    final pass (``depth``: 4 for fmri_bn_fold / fmri_bn_bwd_fold, 2 for fmri_bn_fold_finalize) folds the block rows."""
    if rows <= FOLD_SWITCH:
        return fold_chain(rows, depth)
    per = (rows + FOLD_STAGE_ROWS - 1) // FOLD_STAGE_ROWS
    ny = (rows + per - 1) // per
    return fold_chain(per, 4) + fold_chain(ny, depth)


def stat_chain(pixels, rows, depth):
    """D of the statistics epilogue: a loader lane adds at most ceil(pixels per group / (rows 16)) stored values (a block
    owns pixels / rows of them, 16 lanes share a channel), 16 lane sums meet in the block's row, then the fold."""
    return (pixels + rows * 16 - 1) // (rows * 16) + 16 + fold_chains(rows, depth)


def cmp_stat_sums(family, sums, got, pixels, rows, depth, what):
    """``got`` [2][C] fp32 (the library's fold of the kernel's rows of ONE group) against ``sums`` [3][C] float64 of the
    stored output.  grid: bit-equal.  real: the project bounds (2e-5 sqrt(M) ||y|| on sum y, 2e-5 sum y^2 + 1e-6 on
    sum y^2: tests/test_kernels_gpu.py) and the sharp ones, 4 u sqrt(D) sum |y| and 4 u sqrt(D) sum y^2: every addend is
    an fp16 value or its exact fp32 square, only the additions round, each by at most u times a partial sum <= sum |t|;
    D roundings of random sign add up like sqrt(D), and 4 is the slack on the random walk.  At the largest case
    (discriminator.conv.1: M = 786 432, D = 244) the bound on sum y^2 is 2.9 RMS^2: a dropped image row (32 pixels) is 11
    bounds, the project bound lets 15 pixels through, and the single pixel is what the grid family is for."""
    s1, s2, sa = sums[0], sums[1], sums[2]
    if family == "grid":
        return [bits(f"{what} sum y", got[0], s1.float()), bits(f"{what} sum y^2", got[1], s2.float())]
    D = stat_chain(pixels, rows, depth)
    return [rat(f"{what} sum y | project", got[0], s1, 2e-5 * math.sqrt(pixels) * s2.sqrt().clamp_min(1e-6)),
            rat(f"{what} sum y^2 | project", got[1], s2, 2e-5 * s2 + 1e-6),
            rat(f"{what} sum y | sharp", got[0], s1, 4 * U * math.sqrt(D) * sa),
            rat(f"{what} sum y^2 | sharp", got[1], s2, 4 * U * math.sqrt(D) * s2)]


def stat_sum_bounds(sums, pixels, rows, depth):
    """The sharp bounds of cmp_stat_sums as tensors (B sum y, B sum y^2), for propagation into BatchNorm."""
    D = stat_chain(pixels, rows, depth)
    return 4 * U * math.sqrt(D) * sums[2], 4 * U * math.sqrt(D) * sums[1]


# =====================================================================================================================
# folds of synthetic rows
# =====================================================================================================================
def fold_rows_input(rows, n, family, seed, device, groups=1, cap=None):
    """[groups][cap][n] fp32, rows beyond ``rows`` NaN (they must not be read).  grid: integers in [-1000, 1000] (6152 rows
    of them stay below 2^24); real: normals with a per-column offset."""
    cap = rows if cap is None else cap
    g = torch.Generator(device=device).manual_seed(seed)
    if family == "grid":
        p = torch.randint(-1000, 1001, (groups, rows, n), generator=g, device=device).float()
    else:
        p = torch.randn(groups, rows, n, generator=g, device=device) * 3.0 + torch.randn(1, 1, n, generator=g, device=device)
    out = torch.full((groups, cap, n), float("nan"), device=device)
    out[:, :rows] = p
    return out


def cmp_fold(family, part, rows, got, depth, what):
    """``got`` [groups][n] against the float64 column sums of part[:, :rows].  real: u D sum |p|, D the fold's longest
    chain (every addition rounds by at most u times a partial sum <= sum |p|; first order in u)."""
    p = part[:, :rows].double()
    ref = p.sum(1)
    if family == "grid":
        assert float(p.abs().sum(1).max()) < LIMIT
        return [bits(what, got, ref.float())]
    return [rat(what, got, ref, U * fold_chains(rows, depth) * p.abs().sum(1))]


def cmp_param_grad(family, sums32, prior, gscale, got, what):
    """dbeta / dgamma = prior + gscale * (the kernel's own fp32 sum): one rounding of the product, one of the addition."""
    want = prior.double() + gscale * sums32.double()
    if family == "grid":
        return [bits(what, got, want.float())]
    return [rat(what, got, want, U * (abs(gscale) * sums32.double().abs() + want.abs()) + 1e-300)]


# =====================================================================================================================
# finalize
# =====================================================================================================================
def finalize64(sx, sxx, count, gamma, beta, updates=0, rm=None, rv=None, Bsx=0.0, Bsxx=0.0, Brm=0.0, Brv=0.0):
    """bn_finalize_channel (csrc/norm.hip) in float64 from the sums sx, sxx (float64 tensors), eps = 1e-5f and momentum
    0.9f as the C ABI receives them, with the bound of every output for inputs that are off by at most Bsx / Bsxx
    (0: the kernel's own fp32 sums, which isolates finalize from the fold) and running statistics that are off by at most
    Brm / Brv (a second call of a chain).  Returns name -> (reference, bound).

    Derivation (fp32 roundings of relative size u; covers the contracted and the uncontracted forms):
      mean = sx / count                        B_mean = Bsx / count + u |mean|
      var  = max(sxx / count - mean^2, 0)      q = sxx / count rounds by u q; mean carries u |mean|, so mean^2 is off by
                                               2 u mean^2 and rounds by u mean^2; the difference rounds by u |var| <= u q:
                                               B_var = 3 u (q + mean^2) + Bsxx / count + 2 |mean| Bsx / count (+ 2nd order)
      rstd = rsqrt(var + eps)                  an interval, not a derivative -- in a channel with |mean| >> std B_var
                                               exceeds var: v32 lies in [(max(var - B_var, 0) + eps)(1 - u),
                                               (var + B_var + eps)(1 + u)] (the kernel clamps var at 0) and rsqrtf is
                                               taken as 2 ulp = 4 u relative: B_rstd = the farther end's distance
      scale = gamma rstd                       B_scale = |gamma| B_rstd + u |scale|
      shift = beta - mean scale                B_shift = |mean| B_scale + |scale| B_mean + B_mean B_scale
                                                         + u |mean scale| + u |shift|
      unbiased = var count / (count - 1)       (count = 1: var) B_unb = B_var count / (count - 1) + 2 u unbiased
      running  = (1 - m) running + m new       per update: B' = (1 - m) B + m B_new + u ((1 - m) |r| + m |new|) + u |r'|
                                               ((1 - m) is exact in fp32: Sterbenz)."""
    f = lambda t: torch.as_tensor(t, dtype=torch.float64, device=sx.device)
    gamma, beta, Bsx, Bsxx = f(gamma), f(beta), f(Bsx), f(Bsxx)
    mean = sx / count
    Bmean = Bsx / count + U * mean.abs()
    q = sxx / count
    var = (q - mean * mean).clamp_min(0.0)
    Bin = Bsx / count
    Bvar = 3 * U * (q.abs() + mean * mean) + Bsxx / count + 2 * mean.abs() * Bin + Bin * Bin
    v = var + EPS32
    vlo = ((var - Bvar).clamp_min(0.0) + EPS32) * (1 - U)
    vhi = (var + Bvar + EPS32) * (1 + U)
    rstd = v.rsqrt()
    Brstd = torch.maximum(vlo.rsqrt() * (1 + 4 * U) - rstd, rstd - vhi.rsqrt() * (1 - 4 * U))
    scale = gamma * rstd
    Bscale = gamma.abs() * Brstd + U * scale.abs()
    shift = beta - mean * scale
    Bshift = mean.abs() * Bscale + scale.abs() * Bmean + Bmean * Bscale + U * (mean * scale).abs() + U * shift.abs()
    out = {"mean": (mean, Bmean), "var": (var, Bvar), "rstd": (rstd, Brstd), "scale": (scale, Bscale),
           "shift": (shift, Bshift)}
    if rm is not None:
        unb = var * count / (count - 1.0) if count > 1 else var
        Bunb = (Bvar * count / (count - 1.0) if count > 1 else Bvar) + 2 * U * unb
        r, Br, s, Bs = f(rm).clone(), f(Brm) + torch.zeros_like(mean), f(rv).clone(), f(Brv) + torch.zeros_like(mean)
        m, om = MOM32, 1.0 - MOM32
        for _ in range(int(updates)):
            r2 = om * r + m * mean
            Br = om * Br + m * Bmean + U * (om * r.abs() + m * mean.abs()) + U * r2.abs()
            r = r2
            s2 = om * s + m * unb
            Bs = om * Bs + m * Bunb + U * (om * s.abs() + m * unb.abs()) + U * s2.abs()
            s = s2
        out["running_mean"], out["running_var"] = (r, Br), (s, Bs)
    return out


def hard_sums(C, count, seed, device):
    """fp32 (sx, sxx) [C] of ``count`` samples per channel with mean / std cycling through 0, 2, 8, 64, 1000 and an
    all-zero channel: channel c % 8 == 5 is constant zero, c % 8 == 6 a constant 3 (var exactly 0 in float64)."""
    g = torch.Generator().manual_seed(seed)
    ratio = torch.tensor([0.0, 2.0, 8.0, 64.0, 1000.0])[torch.arange(C) % 5]
    std = torch.rand(C, generator=g) + 0.5
    mean = ratio * std * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
    sx = (mean * count).double()
    sxx = ((std.double() ** 2 + mean.double() ** 2) * count)
    c = torch.arange(C)
    sx[c % 8 == 5], sxx[c % 8 == 5] = 0.0, 0.0
    sx[c % 8 == 6], sxx[c % 8 == 6] = 3.0 * count, 9.0 * count
    return sx.float().to(device), sxx.float().to(device)


# =====================================================================================================================
# BatchNorm (+ ReLU) of the stored output, per element; the eval-mode affine map
# =====================================================================================================================
def cmp_bn_apply(what, x16, got16, fin, relu=True, chunk=1 << 22):
    """got16 = relu?(x scale + shift) stored in fp16 against float64 with ``fin`` = finalize64(...) of the TRUE float64 sums
    and the bounds of the kernel's sums: fp32 error A = |x| B_scale + B_shift + u (|x scale| + |p|) (the product and the
    sum, or one FMA), then ONE fp16 rounding: A + 2^-11 (|p| + A) + 2^-25.  ReLU is 1-Lipschitz."""
    C = x16.shape[-1]
    (sc, Bsc), (sh, Bsh) = fin["scale"], fin["shift"]
    xs, gs = x16.reshape(-1, C), got16.reshape(-1, C)
    worst, finite = 0.0, True
    for a in range(0, xs.shape[0], chunk):
        x = xs[a:a + chunk].double()
        p = x * sc + sh
        A = x.abs() * Bsc + Bsh + U * ((x * sc).abs() + p.abs())
        if relu:
            p = p.clamp_min(0.0)
        g = gs[a:a + chunk].double()
        finite = finite and bool(torch.isfinite(g).all())
        err = (g - p).abs()
        r = torch.where(err == 0, torch.zeros_like(err), err / (A + H16 * (p.abs() + A) + SUB16))
        worst = max(worst, float(r.max()))
    return [(what, "ratio", worst if finite else float("inf"), int(xs.numel()))]


def affine_params(C, seed, device):
    """scale in {+-2^k, k = -2 .. 1}, shift a multiple of 2^-4 in [-4, 4] (fp32 [C]): on integer outputs with
    2 max |y| + 4 < 128 the map y scale + shift is a multiple of 2^-4 below 2^7 -- exact in fp32 and in fp16."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-2, 2, (C,), generator=g)
    sign = torch.randint(0, 2, (C,), generator=g) * 2 - 1
    scale = (sign * torch.pow(2.0, k.double())).float()
    shift = (torch.randint(-64, 65, (C,), generator=g).double() / 16.0).float()
    return scale.to(device), shift.to(device)


def affine64(y64, scale, shift, relu):
    p = y64 * scale.double() + shift.double()
    return p.clamp_min(0.0) if relu else p


def cmp_affine_real(what, got16, conv_ref, scale, shift, relu, K):
    """Fused output against float64 convolution + affine map: |scale| e + 2^-11 (|ref| + |scale| e) + 2^-25 with
    e = 4 u sqrt(K) RMS(conv) of tests/test_fullbatch_conv_gpu.py -- ONE fp16 rounding (the unfused chain rounds twice)."""
    rms = float(conv_ref.pow(2).mean().sqrt()) + 1e-300
    e = 4 * U * math.sqrt(K) * rms * scale.double().abs()
    ref = affine64(conv_ref, scale, shift, relu)
    return [rat(what, got16, ref, e + H16 * (ref.abs() + e) + SUB16)]
