"""fmri_image_metrics (csrc/evalmetrics.hip) -- PCC, mean SSIM and MSE of a batch in the engine's image layout in two
launches -- against the float64 restatement tests/eval_oracle.py on ident_oracle.edge_batch images rounded to fp16.

Bars: PCC and SSIM 2e-6 absolute against float64, the bar of every metric kernel of the project (tests/test_metrics.py:81,
tests/test_ident_edges_gpu.py:21); MSE 2^-22 relative (inputs exact in fp64, fp64 sums: one fp32 rounding remains).
Every check prints one ``err/bound`` line before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import eval_oracle as EO
import ident_oracle as IO

pytestmark = pytest.mark.gpu

BAR_ABS = 2e-6
BAR_MSE_REL = 2.0 ** -22
SHAPES = [(1, 11, 11), (2, 11, 40), (2, 17, 16), (3, 33, 31), (5, 64, 64), (3, 100, 100), (2, 128, 128), (300, 11, 11)]


def _call(pred16, truth16, N, H, W, C=3, affine=None, out=None, acc=None, acc_mode=0, Cp=8, ws_short=0):
    """One fmri_image_metrics call on torch's current stream; returns (code, out7 device tensor)."""
    from fmri_hip import lib
    L = lib.load()
    nbytes = L.fmri_image_metrics_ws_bytes(N, H, W)
    assert nbytes == 56 * N * ((H + 15) // 16) * ((W + 15) // 16)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device="cuda")
    if out is None:
        out = torch.full((7,), -7.0, dtype=torch.float32, device="cuda")
    sc = sf = None
    if affine is not None:
        sc, sf = (ctypes.c_float * C)(*affine[0][:C]), (ctypes.c_float * C)(*affine[1][:C])
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    code = L.fmri_image_metrics(ptr(pred16), ptr(truth16), N, H, W, C, Cp,
                                None if sc is None else ctypes.cast(sc, ctypes.c_void_p),
                                None if sf is None else ctypes.cast(sf, ctypes.c_void_p),
                                ws.data_ptr(), nbytes - ws_short, out.data_ptr(), ptr(acc), acc_mode, lib.stream())
    torch.cuda.synchronize()          # (ws stays alive until the launches are done)
    return code, out


def _pair(N, H, W, C=3, seed=None, pad=0.0):
    k = max(N, 2)                 # (edge_batch mixes every image with another one)
    p, t = IO.edge_batch(k, k, C, H, W, 31 + N + H + W if seed is None else seed)
    return EO.to_layout(p[:N], pad), EO.to_layout(t[:N], pad)


def _check(tag, got, want):
    """got: out7[0..2] (numpy fp32); want: float64 (pcc, ssim, mse).  Prints, then asserts the three bars."""
    errs = [abs(float(got[0]) - want[0]), abs(float(got[1]) - want[1]), abs(float(got[2]) - want[2]) / want[2]]
    bounds = [BAR_ABS, BAR_ABS, BAR_MSE_REL]
    for name, e, b in zip(("pcc", "ssim", "mse(rel)"), errs, bounds):
        print(f"image_metrics {tag} {name}: err/bound {e:.3g}/{b:.3g} = {e / b:.3f}")
    for e, b in zip(errs, bounds):
        assert e <= b, (tag, errs, bounds)


@pytest.mark.parametrize("affine", [None, EO.DENORM], ids=["raw", "denorm"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_image_metrics_against_fp64(shape, affine):
    """Smallest SSIM geometry (every halo pixel outside), H < W with a partial last tile, one row past a tile, odd sizes,
    the paper geometry 100 = 6 * 16 + 4, 128 x 128, and more partials than the fold has threads -- raw and with the
    ImageNet denormalisation."""
    N, H, W = shape
    p16, t16 = _pair(N, H, W)
    code, out = _call(p16.cuda(), t16.cuda(), N, H, W, 3, affine)
    assert code == 0
    got = out.cpu().numpy()
    assert (got[3:] == -7.0).all()                      # no accumulator: out7[3..6] are left alone
    sc, sf = affine if affine is not None else (None, None)
    _check(f"{shape} {'denorm' if affine else 'raw'}", got, EO.image_metrics64(p16, t16, 3, sc, sf))
    if affine is None:
        # agreement with the single-pair kernels on fp32 NCHW copies: logged, each side is within 2e-6 of float64
        from train.train_utils import PearsonCorrelation, StructuralSimilarity
        a = EO.from_layout(p16, 3).float().cuda()
        b = EO.from_layout(t16, 3).float().cuda()
        ds = abs(StructuralSimilarity()(a, b).item() - float(got[1]))
        dp = abs(PearsonCorrelation()(a, b).item() - float(got[0]))
        print(f"image_metrics {shape} vs fmri_ssim {ds:.3g}, vs fmri_pcc {dp:.3g} (bound {2 * BAR_ABS:.3g})")
        assert ds <= 2 * BAR_ABS and dp <= 2 * BAR_ABS


@pytest.mark.parametrize("affine", [None, EO.DENORM], ids=["raw", "denorm"])
def test_image_metrics_one_channel(affine):
    """C = 1 at one row past a tile: lanes 1..7 are pad."""
    N, H, W = 2, 17, 16
    p16, t16 = _pair(N, H, W, C=1, pad=3.0)
    code, out = _call(p16.cuda(), t16.cuda(), N, H, W, 1, affine)
    assert code == 0
    sc, sf = affine if affine is not None else (None, None)
    _check(f"(2, 17, 16) C=1 {'denorm' if affine else 'raw'}", out.cpu().numpy(), EO.image_metrics64(p16, t16, 1, sc, sf))


def _bits(out):
    return out[:3].cpu().numpy().view(np.int32).tolist()


def test_pad_lanes_reach_no_sum():
    """Lanes 3..7 filled with NaN give the bits of zeros, raw and denormalised."""
    N, H, W = 3, 33, 31
    for affine in (None, EO.DENORM):
        outs = []
        for pad in (0.0, float("nan")):
            p16, t16 = _pair(N, H, W, pad=pad)
            code, out = _call(p16.cuda(), t16.cuda(), N, H, W, 3, affine)
            assert code == 0
            outs.append(_bits(out))
        assert outs[0] == outs[1], outs
        assert np.isfinite(np.array(outs[1], dtype=np.int32).view(np.float32)).all()


def test_position_independent_and_repeatable():
    """Images [2:5] of a batch through a pointer offset give the bits of their copy; two calls are bit-identical with the
    deterministic mode on and off."""
    from fmri_hip import ops
    H, W = 33, 31
    p16, t16 = [t.cuda() for t in _pair(6, H, W)]
    code, whole = _call(p16[2:5], t16[2:5], 3, H, W, 3, EO.DENORM)
    assert code == 0 and p16[2:5].data_ptr() != p16.data_ptr()
    pc, tc = p16[2:5].clone(), t16[2:5].clone()
    ref = _bits(_call(pc, tc, 3, H, W, 3, EO.DENORM)[1])
    assert _bits(whole) == ref
    was = ops.set_deterministic(True)
    try:
        on = [_bits(_call(pc, tc, 3, H, W, 3, EO.DENORM)[1]) for _ in range(2)]
        ops.set_deterministic(False)
        off = [_bits(_call(pc, tc, 3, H, W, 3, EO.DENORM)[1]) for _ in range(2)]
    finally:
        ops.set_deterministic(was)
    assert on[0] == on[1] == off[0] == off[1] == ref


def test_accumulator_reset_add_add():
    """reset / add / add over three batches: the running means are within one fp32 ulp of the float64 mean of the three
    out[0..2], the count is 3, and 'reset' does not read what the accumulator held."""
    H, W = 17, 16
    acc = torch.full((4,), 1e9, dtype=torch.float64, device="cuda")
    rows = []
    for k, mode in enumerate((0, 1, 1)):
        p16, t16 = _pair(2, H, W, seed=100 + k)
        code, out = _call(p16.cuda(), t16.cuda(), 2, H, W, 3, None, acc=acc, acc_mode=mode)
        assert code == 0
        rows.append(out.cpu().numpy())
        assert rows[-1][6] == k + 1
    mean64 = np.stack([r[:3] for r in rows]).astype(np.float64).mean(0)
    for j, name in enumerate(("pcc", "ssim", "mse")):
        err, ulp = abs(float(rows[2][3 + j]) - mean64[j]), float(np.spacing(np.float32(abs(mean64[j]))))
        print(f"image_metrics accumulator mean {name}: err/bound {err:.3g}/{ulp:.3g} = {err / ulp:.3f}")
        assert err <= ulp
    assert acc.cpu().tolist()[3] == 3.0
    # after the first call the means are that batch's own values
    assert rows[0][3:6].tolist() == rows[0][:3].tolist()


def test_error_returns_launch_nothing():
    """H = 10 and Cp = 4: FMRI_E_UNSUPPORTED; a workspace one byte short: FMRI_E_WORKSPACE; a bad accumulator mode and a
    misaligned image pointer: FMRI_E_BADARG -- and the output is untouched."""
    p16, t16 = [t.cuda() for t in _pair(2, 17, 16)]
    out = torch.full((7,), -7.0, dtype=torch.float32, device="cuda")
    assert _call(p16, t16, 2, 10, 16, out=out)[0] == -2
    assert _call(p16, t16, 2, 17, 10, out=out)[0] == -2
    assert _call(p16, t16, 2, 17, 16, out=out, Cp=4)[0] == -2
    assert _call(p16, t16, 2, 17, 16, out=out, ws_short=1)[0] == -4
    acc = torch.zeros(4, dtype=torch.float64, device="cuda")
    assert _call(p16, t16, 2, 17, 16, out=out, acc=acc, acc_mode=2)[0] == -1
    assert _call(p16.data_ptr() + 8, t16, 2, 17, 16, out=out)[0] == -1
    assert (out.cpu() == -7.0).all() and (acc.cpu() == 0).all()
