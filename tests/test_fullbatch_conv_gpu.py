"""The convolution kernels at the sizes of the B = 256 step: every image of the forward and of the data gradient, every
element of the weight gradient, against the float64 slicing-and-matmul reference of tests/conv_oracle.py on the device.

tests/test_kernels_gpu.py compares these kernels element by element at 2 - 9 images; at the real sizes it looks at three
images and ties the weight gradient down with one scalar.  What the weight-gradient code does depends on the size
(fmri_wgrad_route in csrc/api.hip, asked through ops.wgrad_plan): ROUTES below states, for each case and each of the
three launch settings (side stream on / off, deterministic mode), the kernel, the ``atomic`` mode, the ``splits`` argument
and the K pieces per parity plane, as literal values; tests/test_conv_oracle_host.py holds that table against the
library's plan and asserts what the table as a whole has to cover, and every case here holds its own fmri_wgrad_if
launch and buffer request against both the table and the plan.

Cases: the 19 FULL_SIZE layers of tests/test_kernels_gpu.py plus EDGE_CASES, cheap shapes that meet the piece-edge
conditions (unequal plane pieces, planes clamped to the tile count, a last piece of one tile, fewer stored slabs than
allocated), plus PX100_CASES: the eleven layers of the as-shipped 100-px configuration (100 -> 50 -> 25 -> 13 -> 7) at
the reference's batch of 64 and at a remainder batch of 5.  Their planes are no multiple of any tile, so every window
kernel runs with masked tiles and odd last rows and columns, and decoder.conv.3 (64 -> 3 channels) runs forward, tanh
epilogue, data gradient and role-exchanged weight gradient on the generic kernels; KERNELS states the forward and
data-gradient kernel of each of them, and the host module holds that table against ops.igemm_route.  Nothing is sampled.

Unwritten memory: every fp16 output buffer is handed to the layer filled with NaN, and for the duration of each
weight-gradient check ops._grad_buffer returns NaN-filled buffers wherever the kernel is to store (not add): an element
that is never written fails the finiteness assertion instead of passing on stale bytes.

Conventions (as tests/test_fullbatch_ops_gpu.py): inputs pre-rounded to fp16, one line
``[fullbatch-conv] <case> | <quantity> | err/bound = r`` per check, r > 1 fails; wall time and peak device memory are
printed without assertion.  profiles/fullbatch_conv_parity.md records the lines of one run.

Bounds -- two per quantity, both asserted.  ``project``: tol RMS(ref) + tol |ref| of test_kernels_gpu._close (2e-3 for
fp16-stored results, 3e-3 for weight gradients).  ``sharp``, with u = 2^-24, derived, not measured:

  * fp32 weight / bias gradient over M = N Yc Xc pixels: 4 u sqrt(M) RMS(ref) + 4 u |ref|.  Products of two fp16 values
    are exact in fp32, only the accumulation rounds; a strictly sequential fp32 sum -- the worst order a kernel here
    could use -- has a random-walk error of about u sqrt(M) RMS / sqrt(2).  A lost or doubled 8 x 8 tile moves an
    element by about 8 RMS / sqrt(M): 10.7 x the bound at the largest M here, more at the others.  The ``scale``
    argument is a power of two, so emit_grad adds no rounding.
  * fp16-stored forward / data gradient with reduction length K = 25 Cin (25 Cout for the data gradient):
    e + 2^-11 (|ref| + e) + 2^-25, e = 4 u sqrt(K) RMS(ref): the fp32 accumulation, then one round-to-nearest fp16
    conversion (the kernels convert with a plain ``(half_t)`` cast, which rounds to nearest even; 2^-25 is half the
    smallest fp16 subnormal).  ReLU and tanh are 1-Lipschitz, so the same e holds behind them, with the activation
    applied to the float64 reference.  tanh adds the error of the device's tanh: csrc/igemm_narrow.hip computes
    copysign((1 - E) / (1 + E), v) with E = __expf(-2 |v|).  E carries a relative error of (1 + 2 |v|) 2^-23 at most (the
    rounding of its argument and two units of the exponential), so 1 - E is off by E (1 + 2 |v|) 2^-23 <= 2^-23
    absolute (E (1 + 2 |v|) <= 1 for every v), and the quotient adds two roundings of a value below 1: T_TANH = 2^-22
    absolute.  test_device_tanh_of_the_narrow_kernel measures it over every fp16 pre-activation in [-16, 16] (the
    pre-activations of decoder.conv.3 have an RMS of about 1): see its docstring for the figure.
    The generic kernel (csrc/igemm.hip, act_apply of csrc/common.h) calls the device library's ``tanhf`` instead; it is
    what decoder.conv.3 runs on at 64 input channels (100 px).  The documentation installed with ROCm's device
    libraries (rocm-device-libs) states no ULP figure for tanhf, so T_TANHF is measured, not derived:
    test_device_tanh_of_the_generic_kernel stores half(tanhf(v)) for every fp16 v in [-16, 16], TANHF_EXCESS is the largest |stored - tanh(v)| beyond the fp16 rounding allowance
    2^-11 |tanh(v)| + 2^-25 on the MI355X run recorded in profiles/fullbatch_conv_parity.md, and T_TANHF is twice that
    excess (the factor covers the pre-activations between fp16 values, which the sweep cannot reach), zero if there
    is none.  Measured: -2.980e-08 -- no stored value left the rounding allowance of the exact tanh, i.e. tanhf's error is
    below what an fp16 store resolves -- so T_TANHF = 0 and the tanh epilogue of decoder.conv.3 @100 is held to the bound
    of a plain fp16-stored result.
"""
import math
import time

import pytest
import torch

import conv_oracle as CO
from test_kernels_gpu import FULL_SIZE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
T_TANH = 2.0 ** -22
# the generic kernel's tanhf (module docstring): the measured excess and the allowance made of it
TANHF_EXCESS = -2.980e-08
T_TANHF = 2.0 * max(TANHF_EXCESS, 0.0)
K5, PAD = 5, 2
RELU, TANH = 1, 2

# names of the FULL_SIZE rows, in its order
FULL_NAMES = ["discriminator.conv.0", "discriminator.conv.1", "discriminator.conv.2", "discriminator.conv.3",
              "encoder.conv.0", "encoder.conv.1", "encoder.conv.2", "decoder.conv.0", "decoder.conv.1", "decoder.conv.2",
              "decoder.conv.3", "encoder.conv.0 @128", "encoder.conv.1 @128", "encoder.conv.2 @128", "decoder.conv.0 @128",
              "decoder.conv.1 @128", "decoder.conv.2 @128", "decoder.conv.3 @128", "discriminator.conv.0 @128"]
assert len(FULL_NAMES) == len(FULL_SIZE) == 19

# cheap shapes for the piece edges of the window kernel (one 8 x 8 tile per image) and of the generic kernel's slabs
EDGE_CASES = [
    # name, (kind, cin, cout, stride, H, out_pad, N)
    ("edge 128->256 16px N=7", ("conv", 128, 256, 2, 16, 0, 7)),      # budget 256: pieces 7/7/7/4, planes 0-2 clamped
    ("edge 128->256 16px N=41", ("conv", 128, 256, 2, 16, 0, 41)),    # budget 256: 9/7/7/6, plane 0 ends in one tile
    ("edge 3->64 100px N=4", ("conv", 3, 64, 2, 100, 0, 4)),          # generic, 19 slabs allocated, 18 stored
]
# the 100-px geometry (ArchConfig.px100: 100 -> 50 -> 25 -> 13 -> 7, the as-shipped configuration) at the reference's
# shipped batch of 64 (N = 64 / 128 / 192 for encoder / decoder / discriminator) and at a remainder batch of 5 (the
# reference's DataLoader keeps the partial last batch): planes of 50, 25, 13 and 7 pixels are no multiple of any tile
PX100_LAYERS = [
    # name, kind, cin, cout, stride, H, out_pad, images per sample of the batch
    ("encoder.conv.0", "conv", 3, 64, 2, 100, 0, 1),
    ("encoder.conv.1", "conv", 64, 128, 2, 50, 0, 1),
    ("encoder.conv.2", "conv", 128, 256, 2, 25, 0, 1),
    ("decoder.conv.0", "deconv", 256, 256, 2, 13, 0, 2),
    ("decoder.conv.1", "deconv", 256, 128, 2, 25, 1, 2),
    ("decoder.conv.2", "deconv", 128, 64, 2, 50, 1, 2),
    ("decoder.conv.3", "conv", 64, 3, 1, 100, 0, 2),
    ("discriminator.conv.0", "conv", 3, 32, 2, 100, 0, 3),
    ("discriminator.conv.1", "conv", 32, 128, 2, 50, 0, 3),
    ("discriminator.conv.2", "conv", 128, 256, 2, 25, 0, 3),
    ("discriminator.conv.3", "conv", 256, 256, 2, 13, 0, 3),
]
PX100_BATCH, PX100_REMAINDER = 64, 5
PX100_CASES = [(f"{r[0]} @100", r[1:7] + (PX100_BATCH * r[7],)) for r in PX100_LAYERS] + \
              [(f"{r[0]} @100 N={PX100_REMAINDER * r[7]}", r[1:7] + (PX100_REMAINDER * r[7],)) for r in PX100_LAYERS]
CASES = list(zip(FULL_NAMES, FULL_SIZE)) + EDGE_CASES + PX100_CASES

# the epilogue the step uses on a layer (nets.py): bias + ReLU on discriminator.conv.0, bias + tanh on decoder.conv.3
EPILOGUE = {"discriminator.conv.0": RELU, "discriminator.conv.0 @128": RELU, "decoder.conv.3": TANH,
            "decoder.conv.3 @128": TANH, "discriminator.conv.0 @100": RELU, "decoder.conv.3 @100": TANH}
# cases that also run the ReLU-mask data gradient (relu_y) the step uses behind discriminator.conv.0
RELU_MASK = ("discriminator.conv.1", "discriminator.conv.1 @100")
# absolute error allowed to the device tanh of a TANH case that does not run on igemm_narrow (T_TANH otherwise)
TANH_ALLOWANCE = {"decoder.conv.3 @100": T_TANHF}
SETTINGS = ("side stream on", "side stream off", "deterministic")

# Weight-gradient route per case and setting: (kernel, ``atomic`` argument, ``splits`` argument, detail).  detail: the K
# pieces of the four parity planes (window kernel; more than 24 at the plane with the most -> atomics, else that many
# slabs), the slabs allocated (narrow kernel), the slabs the library stores (generic kernel in mode 4; 0 otherwise).
# atomic: 1 = atomics into one zeroed matrix, 2 = plane-piece slabs, 3 = the narrow kernel's slabs, 4 = K-split slabs.
ROUTES = {
    "discriminator.conv.0": (("narrow", 3, 4, 4), ("narrow", 3, 4, 4), ("narrow", 3, 768, 768)),
    "discriminator.conv.1": (("win", 1, 160, (50, 39, 39, 31)), ("win", 1, 256, (81, 62, 62, 50)),
                             ("win", 2, 256, (81, 62, 62, 50))),
    "discriminator.conv.2": (("win", 2, 20, (6, 5, 5, 4)), ("win", 2, 32, (10, 8, 8, 6)),
                             ("win", 2, 32, (10, 8, 8, 6))),
    "discriminator.conv.3": (("win", 2, 10, (3, 2, 2, 2)), ("win", 2, 16, (5, 4, 4, 3)), ("win", 2, 16, (5, 4, 4, 3))),
    "encoder.conv.0": (("generic", 1, 512, 0), ("generic", 1, 512, 0), ("generic", 4, 512, 512)),
    "encoder.conv.1": (("win", 1, 80, (25, 20, 20, 16)), ("win", 1, 128, (40, 31, 31, 25)),
                       ("win", 2, 128, (40, 31, 31, 25))),
    "encoder.conv.2": (("win", 2, 20, (6, 5, 5, 4)), ("win", 2, 32, (10, 8, 8, 6)), ("win", 2, 32, (10, 8, 8, 6))),
    "decoder.conv.0": (("win", 2, 10, (3, 2, 2, 2)), ("win", 2, 16, (5, 4, 4, 3)), ("win", 2, 16, (5, 4, 4, 3))),
    "decoder.conv.1": (("win", 2, 20, (6, 5, 5, 4)), ("win", 2, 32, (10, 8, 8, 6)), ("win", 2, 32, (10, 8, 8, 6))),
    "decoder.conv.2": (("win", 1, 160, (50, 39, 39, 31)), ("win", 1, 256, (81, 62, 62, 50)),
                       ("win", 2, 256, (81, 62, 62, 50))),
    "decoder.conv.3": (("narrow", 3, 4, 4), ("narrow", 3, 4, 4), ("narrow", 3, 768, 768)),
    "encoder.conv.0 @128": (("generic", 1, 512, 0), ("generic", 1, 512, 0), ("generic", 4, 512, 512)),
    "encoder.conv.1 @128": (("win", 1, 80, (25, 20, 20, 16)), ("win", 1, 128, (40, 31, 31, 25)),
                            ("win", 2, 128, (40, 31, 31, 25))),
    "encoder.conv.2 @128": (("win", 2, 20, (6, 5, 5, 4)), ("win", 2, 32, (10, 8, 8, 6)), ("win", 2, 32, (10, 8, 8, 6))),
    "decoder.conv.0 @128": (("win", 2, 10, (3, 2, 2, 2)), ("win", 2, 16, (5, 4, 4, 3)), ("win", 2, 16, (5, 4, 4, 3))),
    "decoder.conv.1 @128": (("win", 2, 20, (6, 5, 5, 4)), ("win", 2, 32, (10, 8, 8, 6)), ("win", 2, 32, (10, 8, 8, 6))),
    "decoder.conv.2 @128": (("win", 1, 160, (50, 39, 39, 31)), ("win", 1, 256, (81, 62, 62, 50)),
                            ("win", 2, 256, (81, 62, 62, 50))),
    "decoder.conv.3 @128": (("narrow", 3, 4, 4), ("narrow", 3, 4, 4), ("narrow", 3, 768, 768)),
    "discriminator.conv.0 @128": (("generic", 1, 512, 0), ("generic", 1, 512, 0), ("generic", 4, 512, 512)),
    "edge 128->256 16px N=7": (("win", 2, 20, (4, 4, 4, 4)), ("win", 2, 32, (7, 7, 7, 4)),
                               ("win", 2, 32, (7, 7, 7, 4))),
    "edge 128->256 16px N=41": (("win", 2, 20, (6, 5, 5, 4)), ("win", 2, 32, (9, 7, 7, 6)),
                                ("win", 2, 32, (9, 7, 7, 6))),
    "edge 3->64 100px N=4": (("generic", 1, 19, 0), ("generic", 1, 19, 0), ("generic", 4, 19, 18)),
    "encoder.conv.0 @100": (("generic", 1, 312, 0), ("generic", 1, 312, 0), ("generic", 4, 312, 278)),
    "encoder.conv.1 @100": (("win", 1, 80, (25, 20, 20, 16)), ("win", 1, 128, (40, 31, 31, 25)),
                            ("win", 2, 128, (40, 31, 31, 25))),
    "encoder.conv.2 @100": (("win", 2, 20, (6, 5, 5, 4)), ("win", 2, 32, (10, 8, 8, 6)), ("win", 2, 32, (10, 8, 8, 6))),
    "decoder.conv.0 @100": (("win", 2, 10, (3, 2, 2, 2)), ("win", 2, 16, (5, 4, 4, 3)), ("win", 2, 16, (5, 4, 4, 3))),
    "decoder.conv.1 @100": (("win", 2, 20, (6, 5, 5, 4)), ("win", 2, 32, (10, 8, 8, 6)), ("win", 2, 32, (10, 8, 8, 6))),
    "decoder.conv.2 @100": (("win", 1, 80, (25, 20, 20, 16)), ("win", 1, 128, (40, 31, 31, 25)),
                            ("win", 2, 128, (40, 31, 31, 25))),
    "decoder.conv.3 @100": (("generic", 1, 512, 0), ("generic", 1, 512, 0), ("generic", 4, 512, 500)),
    "discriminator.conv.0 @100": (("generic", 1, 512, 0), ("generic", 1, 512, 0), ("generic", 4, 512, 500)),
    "discriminator.conv.1 @100": (("win", 1, 160, (50, 39, 39, 31)), ("win", 1, 256, (81, 62, 62, 50)),
                                  ("win", 2, 256, (81, 62, 62, 50))),
    "discriminator.conv.2 @100": (("win", 2, 20, (6, 5, 5, 4)), ("win", 2, 32, (10, 8, 8, 6)),
                                  ("win", 2, 32, (10, 8, 8, 6))),
    "discriminator.conv.3 @100": (("win", 2, 10, (3, 2, 2, 2)), ("win", 2, 16, (5, 4, 4, 3)),
                                  ("win", 2, 16, (5, 4, 4, 3))),
    "encoder.conv.0 @100 N=5": (("generic", 1, 24, 0), ("generic", 1, 24, 0), ("generic", 4, 24, 22)),
    "encoder.conv.1 @100 N=5": (("win", 2, 80, (20, 20, 20, 16)), ("win", 1, 128, (40, 27, 27, 20)),
                                ("win", 2, 128, (40, 27, 27, 20))),
    "encoder.conv.2 @100 N=5": (("win", 2, 20, (5, 5, 5, 4)), ("win", 2, 32, (10, 7, 7, 5)),
                                ("win", 2, 32, (10, 7, 7, 5))),
    "decoder.conv.0 @100 N=10": (("win", 2, 10, (3, 2, 2, 2)), ("win", 2, 16, (5, 4, 4, 3)),
                                 ("win", 2, 16, (5, 4, 4, 3))),
    "decoder.conv.1 @100 N=10": (("win", 2, 20, (6, 5, 5, 4)), ("win", 2, 32, (10, 8, 8, 6)),
                                 ("win", 2, 32, (10, 8, 8, 6))),
    "decoder.conv.2 @100 N=10": (("win", 1, 80, (25, 20, 20, 16)), ("win", 1, 128, (38, 31, 31, 25)),
                                 ("win", 2, 128, (38, 31, 31, 25))),
    "decoder.conv.3 @100 N=10": (("generic", 1, 195, 0), ("generic", 1, 195, 0), ("generic", 4, 195, 174)),
    "discriminator.conv.0 @100 N=15": (("generic", 1, 73, 0), ("generic", 1, 73, 0), ("generic", 4, 73, 66)),
    "discriminator.conv.1 @100 N=15": (("win", 1, 160, (48, 35, 35, 30)), ("win", 1, 256, (80, 60, 60, 48)),
                                       ("win", 2, 256, (80, 60, 60, 48))),
    "discriminator.conv.2 @100 N=15": (("win", 2, 20, (6, 5, 5, 4)), ("win", 2, 32, (10, 8, 8, 6)),
                                       ("win", 2, 32, (10, 8, 8, 6))),
    "discriminator.conv.3 @100 N=15": (("win", 2, 10, (3, 2, 2, 2)), ("win", 2, 16, (5, 4, 4, 3)),
                                       ("win", 2, 16, (5, 4, 4, 3))),
}

# Forward and data-gradient kernel per 100-px case, instantiation included, as fmri_igemm_route names it: (forward,
# forward + the EPILOGUE of the case, data gradient, data gradient + ReLU mask of the RELU_MASK cases); None where the case
# does not make that launch.  tests/test_conv_oracle_host.py holds the table against ops.igemm_route and asserts what the
# family has to cover; every case asserts the names its own launches route to.
_GEN = "fmri::igemm_kernel<128,%s>"
_G64, _G32, _G32U = _GEN % "64,2,2,false,false", _GEN % "32,4,1,false,false", _GEN % "32,4,1,false,true"
_C5W16, _C5W8, _TC5, _TC32 = ("fmri::igemm_c5w_kernel<16,0>", "fmri::igemm_c5w_kernel<8,0>",
                              "fmri::igemm_tc5_kernel<64,6,0>", "fmri::igemm_tc32_kernel<%s>")
_TC5W = "fmri::igemm_tc5w_kernel<%s>"
KERNELS = {
    "encoder.conv.0 @100": (_G64, None, _G32U, None),
    "encoder.conv.1 @100": (_C5W16, None, _TC5, None),
    "encoder.conv.2 @100": (_C5W16, None, _TC5W % "16,0,true", None),
    "decoder.conv.0 @100": (_TC5W % "16,0,false", None, _C5W16, None),
    "decoder.conv.1 @100": (_TC5W % "16,0,false", None, _C5W16, None),
    "decoder.conv.2 @100": (_TC5, None, _C5W16, None),
    "decoder.conv.3 @100": (_G32U, _G32U, _G64, None),
    "discriminator.conv.0 @100": (_G32, _G32, _G32, None),
    "discriminator.conv.1 @100": (_C5W16, None, _TC32 % "false", _TC32 % "true"),
    "discriminator.conv.2 @100": (_C5W16, None, _TC5W % "16,0,false", None),
    "discriminator.conv.3 @100": (_C5W8, None, _TC5W % "8,0,true", None),
    "encoder.conv.0 @100 N=5": (_G64, None, _G32U, None),
    "encoder.conv.1 @100 N=5": (_C5W16, None, _TC5, None),
    "encoder.conv.2 @100 N=5": (_C5W16, None, _TC5W % "16,0,true", None),
    "decoder.conv.0 @100 N=10": (_TC5W % "16,0,true", None, _C5W16, None),
    "decoder.conv.1 @100 N=10": (_TC5W % "16,0,true", None, _C5W16, None),
    "decoder.conv.2 @100 N=10": (_TC5, None, _C5W16, None),
    "decoder.conv.3 @100 N=10": (_G32U, None, _G64, None),
    "discriminator.conv.0 @100 N=15": (_G32, None, _G32, None),
    "discriminator.conv.1 @100 N=15": (_C5W16, None, _TC32 % "false", None),
    "discriminator.conv.2 @100 N=15": (_C5W16, None, _TC5W % "16,0,true", None),
    "discriminator.conv.3 @100 N=15": (_C5W8, None, _TC5W % "8,0,true", None),
}


def _h(t):
    return t.half().float()


def geometry(kind, cin, cout, stride, H, op, N):
    """The arguments ConvLayer._wgrad hands to ops.run_wgrad for this layer (restated from fmri_hip/ops.py): rows A of
    the packed gradient, gathered columns Bc, the sampled plane Yc x Yc, the gathered plane Hq x Hq, stride, flip; and
    the layer's output size."""
    pad8 = lambda c: (c + 7) // 8 * 8
    cinp, coutp = pad8(cin), pad8(cout)
    if kind == "conv":
        Ho = CO.out_size(H, K5, stride, PAD)
        if stride == 1 and cinp > coutp:
            return dict(A=cinp, Bc=coutp, Yc=H, Hq=Ho, stride=1, flip=1, Ho=Ho, M=N * Ho * Ho)
        return dict(A=coutp, Bc=cinp, Yc=Ho, Hq=H, stride=stride, flip=0, Ho=Ho, M=N * Ho * Ho)
    Ho = CO.deconv_out_size(H, K5, 2, PAD, op)
    return dict(A=cinp, Bc=coutp, Yc=H, Hq=Ho, stride=2, flip=0, Ho=Ho, M=N * H * H)


def plane_pieces(ntiles, splits, k=K5, pad=PAD):
    """wgrad_plane_pieces of csrc/api.hip restated: (tiles per piece, pieces) of the four parity planes for a budget of
    ``splits`` blocks per tile group.  The host module holds max(pieces) against the library's fmri_wgrad_slabs over a
    sweep of tile counts and budgets."""
    nsh = [0, 0]
    for t in range(k):
        nsh[(t - pad) & 1] += 1
    total = max(splits, 4)
    total -= total & 3
    cost = [128.0 * nsh[pl >> 1] * nsh[pl & 1] + 550.0 for pl in range(4)]
    csum = sum(cost)
    tps, pieces = [], []
    for pl in range(4):
        sp = int(total * cost[pl] / csum + 0.5)
        sp = max(sp, 1)
        if sp > ntiles:
            sp = max(ntiles, 1)
        t = max((ntiles + sp - 1) // sp, 1)
        tps.append(t)
        pieces.append((ntiles + t - 1) // t if ntiles > 0 else 1)
    return tuple(tps), tuple(pieces)


def planned_pieces(ntiles, splits, k=K5, pad=PAD):
    """The block counts the planner AIMS at per plane, before they are cut to the tile count (a plane is 'clamped' when
    its aim exceeds the tile count)."""
    total = max(splits, 4)
    total -= total & 3
    nsh = [0, 0]
    for t in range(k):
        nsh[(t - pad) & 1] += 1
    cost = [128.0 * nsh[pl >> 1] * nsh[pl & 1] + 550.0 for pl in range(4)]
    return tuple(max(int(total * c / sum(cost) + 0.5), 1) for c in cost)


FAMILY = {"fmri::wgrad_win_kernel": "win", "fmri::wgrad_narrow_kernel": "narrow", "fmri::wgrad_kernel": "generic"}


def plan_route(plan):
    """(kernel, atomic, splits, detail) of ROUTES out of an ops.WgradPlan (fmri_wgrad_route: the library's own statement
    of the routing, host code only)."""
    kern = FAMILY[plan.kernel.split("<")[0]]
    detail = {"win": plan.pieces, "narrow": plan.slabs, "generic": plan.stored}[kern]
    return (kern, plan.atomic, plan.splits, detail)


def case_plan(case, setting):
    """ops.wgrad_plan for the arguments ConvLayer._wgrad hands to run_wgrad for this case, under a launch setting."""
    from fmri_hip.ops import wgrad_plan
    g = geometry(*case)
    return wgrad_plan(case[6], g["Yc"], g["Yc"], g["A"], g["Hq"], g["Hq"], g["Bc"], K5, g["stride"], PAD, g["flip"],
                      side=setting != "side stream off", det=setting == "deterministic")


def routes_of(name, case):
    return ROUTES[name]


def igemm_kernels(name, case):
    """The four entries of KERNELS for a case, asked of the library (ops.igemm_route: host code only, no GPU) with the
    arguments ConvLayer.forward / ConvLayer.dgrad hand to run_igemm, restated from fmri_hip/ops.py; tile sizes and the
    packed-weight element counts come from a ConvLayer built on the CPU.  Every GPU case also asserts the names of its
    own launches, so a change of those arguments fails there even if this copy were left behind."""
    from fmri_hip.ops import ConvLayer, igemm_route, MODE_CONV, MODE_CONV_FLIP, MODE_TCONV2
    kind, cin, cout, stride, H, op, N = case
    shape = (cout, cin, 5, 5) if kind == "conv" else (cin, cout, 5, 5)
    tensors = {"w": torch.zeros(shape)}
    if name in EPILOGUE:
        tensors["b"] = torch.zeros(cout)
    layer = ConvLayer(_G(tensors, "cpu"), "w", "b" if "b" in tensors else None, kind, cin, cout, 5, stride, 2, op)
    Ho = geometry(*case)["Ho"]
    cip, cop, wf, wd = layer.cinp, layer.coutp, layer.pw_f.buf.numel(), layer.pw_d.buf.numel()
    fmode = MODE_CONV if kind == "conv" else MODE_TCONV2
    fwd = lambda act: igemm_route(N, H, H, cip, Ho, Ho, cop, cout, 5, stride, 2, fmode, act, False, 1, layer.t_out, wf,
                                  has_bias=name in EPILOGUE)
    if kind == "conv":
        dmode, dstride = (MODE_TCONV2 if stride == 2 else MODE_CONV_FLIP), stride
    else:
        dmode, dstride = MODE_CONV, 2
    dgr = lambda act_y: igemm_route(N, Ho, Ho, cop, H, H, cip, cin, 5, dstride, 2, dmode, 0, False, 1, layer.t_in, wd,
                                    want_act_y=act_y)
    return (fwd(0), fwd(EPILOGUE[name]) if name in EPILOGUE else None, dgr(False),
            dgr(True) if name in RELU_MASK else None)


# =====================================================================================================================
# helpers of the GPU checks
# =====================================================================================================================
class _G:
    """Minimal FlatGroup stand-in for single-layer tests (as in tests/test_kernels_gpu.py)."""

    def __init__(self, tensors, device=DEV):
        self.views = {k: v.to(device).contiguous() for k, v in tensors.items()}
        self.grads = {k: torch.zeros_like(v) for k, v in self.views.items()}
        self.version = 0
        self.device = torch.device(device)


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

    def args_of(self, name):
        return [a for n, a in self.calls if n == name]


class _NanBuffers:
    """For the duration of the block a weight-gradient buffer requested with ``zeroed=False`` (ops._grad_buffer) comes
    back filled with NaN: an element the kernel is supposed to write and does not then fails the finiteness assertion
    instead of adding whatever the allocator handed back.  Buffers requested zeroed are left as they are."""

    def __enter__(self):
        from fmri_hip import ops
        self.ops, self.orig, self.requests = ops, ops._grad_buffer, []

        def grad_buffer(hold, shape, zeroed, device):
            out = self.orig(hold, shape, zeroed, device)
            self.requests.append((tuple(shape), bool(zeroed)))
            if not zeroed:
                out.fill_(float("nan"))
            return out
        ops._grad_buffer = grad_buffer
        return self

    def __exit__(self, *exc):
        self.ops._grad_buffer = self.orig


def _say(case, what, r):
    print(f"[fullbatch-conv] {case} | {what} | err/bound = {r:.4f}", flush=True)
    assert r <= 1.0, f"{case}: {what}: err / bound = {r:.4f}"
    return r


def _rms(ref):
    return ref.pow(2).mean().sqrt().item() + 1e-300


def _max_ratio(err, bound):
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


def _check_f16(case, what, got, ref, K, extra=0.0):
    """Both bounds of an fp16-stored result (module docstring); ``extra``: absolute error of the device activation."""
    got = got.double()
    assert got.shape == ref.shape, (case, what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{case}: {what}: non-finite"
    err = (got - ref).abs_()
    rms = _rms(ref)
    mag = ref.abs()
    _say(case, f"{what} | project", _max_ratio(err, 2e-3 * rms + 2e-3 * mag))
    e = 4 * U * math.sqrt(K) * rms + extra
    _say(case, f"{what} | sharp", _max_ratio(err, e + 2.0 ** -11 * (mag + e) + 2.0 ** -25))


def _check_grad(case, what, got, ref, M):
    """Both bounds of an fp32 weight / bias gradient summed over M pixels (module docstring)."""
    got = got.double()
    assert got.shape == ref.shape, (case, what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{case}: {what}: non-finite (an element of a buffer was never written)"
    err = (got - ref).abs_()
    rms = _rms(ref)
    mag = ref.abs()
    _say(case, f"{what} | project", _max_ratio(err, 3e-3 * rms + 3e-3 * mag))
    _say(case, f"{what} | sharp", _max_ratio(err, 4 * U * math.sqrt(M) * rms + 4 * U * mag))


def _igemm_name(a, act_y=False):
    """Kernel instantiation behind a recorded fmri_igemm_ep call (asked of the library: fmri_igemm_route)."""
    from fmri_hip.ops import igemm_route
    return igemm_route(*a[5:18], bool(a[18]), a[19], a[21], a[22], has_bias=bool(a[3]), want_act_y=act_y)


def _nan16(*shape):
    """An fp16 output buffer filled with NaN: a pixel the kernel does not store fails the finiteness assertion (a fresh
    torch.empty may hold the right values of an earlier launch of the same shape)."""
    return torch.full(shape, float("nan"), dtype=torch.float16, device=DEV)


def _layer_and_data(name, case):
    """Layer, fp16 device operands and the float64 views of the same values."""
    from fmri_hip.ops import ConvLayer
    kind, cin, cout, stride, H, op, N = case
    torch.manual_seed(cin * 7 + cout + H + N)
    shape = (cout, cin, 5, 5) if kind == "conv" else (cin, cout, 5, 5)
    w = _h(torch.randn(shape) * (1.0 / (5.0 * cin ** 0.5)))
    tensors = {"w": w}
    if name in EPILOGUE:
        tensors["b"] = _h(torch.randn(cout) * 0.1)
    g = _G(tensors)
    layer = ConvLayer(g, "w", "b" if "b" in tensors else None, kind, cin, cout, 5, stride, 2, op)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(cin + 3 * cout + 5 * H + N)
    geo = geometry(*case)
    Ho = geo["Ho"]
    x16 = torch.zeros(N, H, H, layer.cinp, dtype=torch.float16, device=DEV)
    x16[..., :cin] = torch.randn(N, H, H, cin, device=DEV, generator=gen).half()
    dy16 = torch.zeros(N, Ho, Ho, layer.coutp, dtype=torch.float16, device=DEV)
    dy16[..., :cout] = torch.randn(N, Ho, Ho, cout, device=DEV, generator=gen).half()
    return g, layer, x16, dy16, geo


def _chunk(case, Ho):
    kind, cin, cout, stride, H, op, N = case
    if kind == "conv":
        return CO.images_per_chunk(N, H, H, cin, Ho, Ho, cout)
    return CO.images_per_chunk(N, Ho, Ho, cout, H, H, cin)


# =====================================================================================================================
# the checks
# =====================================================================================================================
def test_device_tanh_of_the_narrow_kernel():
    """The tanh of csrc/igemm_narrow.hip against float64 tanh at EVERY fp16 pre-activation in [-16, 16], through the
    launch decoder.conv.3 makes in the step (32 -> 3 channels, 512 images of 64 x 64): the weight is the identity on the
    centre tap, so the accumulator is the fp16 input exactly and the stored value is half(tanh_device(v)).  Asserted:
    |stored - tanh(v)| <= T + 2^-11 (|tanh(v)| + T) + 2^-25 with the derived T = T_TANH = 2^-22 of the module docstring.
    Printed: the largest |stored - tanh(v)| minus the fp16 rounding allowance 2^-11 |tanh(v)| + 2^-25, an upper estimate
    of the device error itself.  On the MI355X run recorded in profiles/fullbatch_conv_parity.md it is -3.0e-08: no
    stored value left the rounding allowance of the exact tanh, i.e. the device error is below what an fp16 store
    resolves, and T_TANH stays the derived figure."""
    from fmri_hip.ops import ConvLayer, igemm_route, MODE_CONV
    N, H = 512, 64
    bits = torch.arange(0, 0x7C00, dtype=torch.int16)
    pos = bits.view(torch.float16)
    pos = pos[pos <= 16.0]
    vals = torch.cat([pos, -pos]).to(DEV)
    w = torch.zeros(3, 32, 5, 5)
    for c in range(3):
        w[c, c, 2, 2] = 1.0
    g = _G({"w": w, "b": torch.zeros(3)})
    layer = ConvLayer(g, "w", "b", "conv", 32, 3, 5, 1, 2)
    name = igemm_route(N, H, H, 32, H, H, 8, 3, 5, 1, 2, MODE_CONV, TANH, False, 1, layer.t_out, layer.pw_f.buf.numel(),
                       has_bias=True)
    assert name.startswith("fmri::igemm_narrow_kernel<32"), name
    x16 = torch.zeros(N, H, H, 32, dtype=torch.float16, device=DEV)
    flat = x16.view(-1, 32)
    reps = (flat.shape[0] * 3 + vals.numel() - 1) // vals.numel()
    flat[:, :3] = vals.repeat(reps)[:flat.shape[0] * 3].view(-1, 3)
    y16 = layer.forward(x16, TANH, out=_nan16(N, H, H, 8))
    torch.cuda.synchronize()
    ref = torch.tanh(flat[:, :3].double())
    got = y16.view(-1, 8)[:, :3].double()
    assert bool(torch.isfinite(got).all()) and bool((y16[..., 3:] == 0).all())
    err = (got - ref).abs()
    over = float((err - (2.0 ** -11 * ref.abs() + 2.0 ** -25)).max())
    print(f"[fullbatch-conv] tanh of igemm_narrow, {vals.numel()} fp16 values in [-16, 16] | largest error beyond the fp16 "
          f"rounding allowance = {over:.3e} = {over / T_TANH:.3f} of T_TANH", flush=True)
    _say("tanh of igemm_narrow", "stored vs float64 tanh | sharp",
         _max_ratio(err, T_TANH + 2.0 ** -11 * (ref.abs() + T_TANH) + 2.0 ** -25))


def test_device_tanh_of_the_generic_kernel():
    """The tanh of the generic tap-list kernel (``tanhf`` in act_apply, csrc/common.h) against float64 tanh at EVERY fp16
    pre-activation in [-16, 16], through the launch decoder.conv.3 makes at 100 px (64 -> 3 channels; igemm_narrow takes
    8 or 32 input channels only): 4 images of 100 x 100 give 120 000 slots for the 38 914 values; identity centre tap and
    zero bias, so the accumulator is the fp16 input exactly and the stored value is half(tanhf(v)).  Asserted: the route is
    the generic kernel, and |stored - tanh(v)| <= T + 2^-11 (|tanh(v)| + T) + 2^-25 with T = T_TANHF of the module
    docstring.  Printed: the largest |stored - tanh(v)| minus the fp16 rounding allowance 2^-11 |tanh(v)| + 2^-25, the
    figure T_TANHF is twice of (TANHF_EXCESS; profiles/fullbatch_conv_parity.md records the run it was read from)."""
    from fmri_hip.ops import ConvLayer, igemm_route, MODE_CONV
    N, H = 4, 100
    bits = torch.arange(0, 0x7C00, dtype=torch.int16)
    pos = bits.view(torch.float16)
    pos = pos[pos <= 16.0]
    vals = torch.cat([pos, -pos]).to(DEV)
    assert vals.numel() == 38914 and N * H * H * 3 >= vals.numel()
    w = torch.zeros(3, 64, 5, 5)
    for c in range(3):
        w[c, c, 2, 2] = 1.0
    g = _G({"w": w, "b": torch.zeros(3)})
    layer = ConvLayer(g, "w", "b", "conv", 64, 3, 5, 1, 2)
    name = igemm_route(N, H, H, 64, H, H, 8, 3, 5, 1, 2, MODE_CONV, TANH, False, 1, layer.t_out, layer.pw_f.buf.numel(),
                       has_bias=True)
    assert name == KERNELS["decoder.conv.3 @100"][1] and name.startswith("fmri::igemm_kernel<"), name
    x16 = torch.zeros(N, H, H, 64, dtype=torch.float16, device=DEV)
    flat = x16.view(-1, 64)
    reps = (flat.shape[0] * 3 + vals.numel() - 1) // vals.numel()
    flat[:, :3] = vals.repeat(reps)[:flat.shape[0] * 3].view(-1, 3)
    with _Spy() as spy:
        y16 = layer.forward(x16, TANH, out=_nan16(N, H, H, 8))
    torch.cuda.synchronize()
    assert _igemm_name(spy.args_of("fmri_igemm_ep")[0]) == name
    ref = torch.tanh(flat[:, :3].double())
    got = y16.view(-1, 8)[:, :3].double()
    assert bool(torch.isfinite(got).all()) and bool((y16[..., 3:] == 0).all())
    err = (got - ref).abs()
    over = float((err - (2.0 ** -11 * ref.abs() + 2.0 ** -25)).max())
    print(f"[fullbatch-conv] tanhf of igemm_kernel, {vals.numel()} fp16 values in [-16, 16] | largest error beyond the fp16 "
          f"rounding allowance = {over:.3e}; T_TANHF = {T_TANHF:.3e}", flush=True)
    _say("tanhf of igemm_kernel", "stored vs float64 tanh | sharp",
         _max_ratio(err, T_TANHF + 2.0 ** -11 * (ref.abs() + T_TANHF) + 2.0 ** -25))


@pytest.mark.parametrize("name,case", CASES, ids=[c[0].replace(" ", "_").replace("->", "to") for c in CASES])
def test_conv_layer_every_element(name, case):
    """Forward and data gradient of every image, weight (and bias) gradient of every element in the three launch
    settings, against float64; routes observed at the launches against ROUTES."""
    from fmri_hip import ops
    from fmri_hip.ops import ACT_NONE, act_backward
    kind, cin, cout, stride, H, op, N = case
    label = f"{name} {kind} {cin}->{cout} s{stride} {H}px N={N}"
    torch.cuda.reset_peak_memory_stats()
    torch.cuda.synchronize()
    t_start = time.time()
    g, layer, x16, dy16, geo = _layer_and_data(name, case)
    Ho, M = geo["Ho"], geo["M"]
    chunk = _chunk(case, Ho)
    w64 = g.views["w"].double()
    x64v, dy64v = x16[..., :cin], dy16[..., :cout]

    # ---- forward, every image
    with _Spy() as spy:
        if layer.b is None:
            y16 = layer.forward(x16, ACT_NONE, out=_nan16(N, Ho, Ho, layer.coutp))
        else:
            # the plain contraction of a layer that has a bias: the same launch with a zero bias
            keep = layer.b.clone()
            layer.b.zero_()
            y16 = layer.forward(x16, ACT_NONE, out=_nan16(N, Ho, Ho, layer.coutp))
            torch.cuda.synchronize()
            layer.b.copy_(keep)
    kernels = KERNELS.get(name)

    def seen_kernel(what, which, act_y=False):
        kname = _igemm_name(spy.args_of("fmri_igemm_ep")[0], act_y=act_y)
        print(f"[fullbatch-conv] {label} | {what} kernel {kname}", flush=True)
        assert kernels is None or kname == kernels[which], (label, what, kname, kernels[which])

    seen_kernel("forward", 0)
    if kind == "conv":
        ref = CO.conv_fwd(x64v, w64, stride, PAD, chunk)
    else:
        ref = CO.deconv_fwd(x64v, w64, 2, PAD, op, chunk)
    assert y16.shape == (N, Ho, Ho, layer.coutp)
    _check_f16(label, "forward, every image", y16[..., :cout], ref, 25 * cin)
    assert bool((y16[..., cout:] == 0).all()), "padded output channels"
    if name in EPILOGUE:
        act = EPILOGUE[name]
        with _Spy() as spy:
            ya = layer.forward(x16, act, out=_nan16(N, Ho, Ho, layer.coutp))
        seen_kernel("forward + epilogue", 1)
        ref += layer.b.double()
        ref = torch.relu_(ref) if act == RELU else torch.tanh_(ref)
        _check_f16(label, f"forward, bias + {'ReLU' if act == RELU else 'tanh'}, every image", ya[..., :cout], ref,
                   25 * cin, extra=TANH_ALLOWANCE.get(name, T_TANH) if act == TANH else 0.0)
        assert bool((ya[..., cout:] == 0).all()), "padded output channels (epilogue)"
        del ya
    del ref, y16

    # ---- data gradient, every image
    with _Spy() as spy:
        dx16 = layer.dgrad(dy16, H, H, out=_nan16(N, H, H, layer.cinp))
    seen_kernel("data-gradient", 2)
    if kind == "conv":
        ref = CO.conv_dgrad(dy64v, w64, stride, PAD, H, H, chunk)
    else:
        ref = CO.deconv_dgrad(dy64v, w64, 2, PAD, chunk)
    assert dx16.shape == (N, H, H, layer.cinp)
    _check_f16(label, "data gradient, every image", dx16[..., :cin], ref, 25 * cout)
    assert bool((dx16[..., cin:] == 0).all()), "padded channels of the data gradient"
    del ref
    if name in RELU_MASK:
        gen = torch.Generator(device=DEV)
        gen.manual_seed(11)
        y0 = torch.relu(torch.randn(N, H, H, cin, device=DEV, generator=gen)).half()
        with _Spy() as spy:
            masked = layer.dgrad(dy16, H, H, out=_nan16(N, H, H, layer.cinp), relu_y=y0)
        seen_kernel("data-gradient + ReLU mask", 3, act_y=True)
        assert layer.act_applied, "the ReLU-backward epilogue was declined at the size the step uses it"
        assert torch.equal(masked, act_backward(y0, dx16, ops.ACT_RELU)), "relu_y epilogue != dgrad + act_backward"
        print(f"[fullbatch-conv] {label} | data gradient with relu_y == plain + act_backward | err/bound = 0.0000")
        del masked, y0
    del dx16

    # ---- weight gradient, every element, three settings
    if kind == "conv":
        wref = CO.conv_wgrad(x64v, dy64v, 5, stride, PAD, chunk)
    else:
        wref = CO.deconv_wgrad(x64v, dy64v, 5, 2, PAD, chunk)
    bias_too = layer.b is not None and kind == "conv" and cin < cout
    bref = CO.bias_grad(dy64v) if bias_too else None
    expected = routes_of(name, case)
    SCALE = 4.0
    side_was, det_was = ops._SIDE["on"], ops.deterministic()
    try:
        for si, setting in enumerate(SETTINGS):
            ops._SIDE["on"] = setting != "side stream off"
            ops.set_deterministic(setting == "deterministic")
            runs = []
            for rep in range(2 if setting == "deterministic" else 1):
                for v in g.grads.values():
                    v.zero_()
                with _Spy() as spy, _NanBuffers() as nb:
                    layer.wgrad(x16, dy16, SCALE, bias_too=bias_too)
                    ops.join_side()
                torch.cuda.synchronize()
                a = spy.args_of("fmri_wgrad_if")
                assert len(a) == 1, len(a)
                kern, mode, splits, detail = expected[si]
                # the library's plan for the geometry of this very launch: it is the table's row, and what was launched
                plan = ops.wgrad_plan(*a[0][5:16], side=ops._SIDE["on"], det=ops.deterministic())
                assert plan_route(plan) == expected[si] == plan_route(case_plan(case, setting)), (label, setting, plan)
                seen = (FAMILY[plan.kernel.split("<")[0]], a[0][20], a[0][19])
                assert seen == (kern, mode, splits) == (kern, plan.atomic, plan.splits), (label, setting, seen, expected[si])
                # the buffer the launch was given: slabs as the route says, NaN-filled unless the kernel adds into it
                shape, zeroed = nb.requests[0]
                slabs_alloc = shape[0] if len(shape) == 3 else 0
                assert (slabs_alloc, zeroed) == (plan.slabs, plan.zeroed), (shape, zeroed, plan)
                if kern == "win":
                    assert (slabs_alloc, zeroed) == ((max(detail), False) if mode == 2 else (0, True)), (shape, zeroed)
                elif kern == "narrow":
                    assert (slabs_alloc, zeroed) == (detail, True), (shape, zeroed)
                else:
                    assert (slabs_alloc, zeroed) == ((splits, True) if mode == 4 else (0, splits > 1)), (shape, zeroed)
                runs.append({k: v.clone() for k, v in g.grads.items()})
            print(f"[fullbatch-conv] {label} | route, {setting}: {kern} atomic={mode} splits={splits} detail={detail} "
                  f"buffer={shape}", flush=True)
            _check_grad(label, f"weight gradient, {setting}", runs[0]["w"] * SCALE, wref, M)
            if bias_too:
                _check_grad(label, f"bias gradient, {setting}", runs[0]["b"] * SCALE, bref, M)
            if setting == "deterministic":
                assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0]), "deterministic mode: two runs differ"
    finally:
        ops._SIDE["on"] = side_was
        ops.set_deterministic(det_was)
    torch.cuda.synchronize()
    print(f"[fullbatch-conv] {label} | wall {time.time() - t_start:.1f} s, peak device memory "
          f"{torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB", flush=True)
