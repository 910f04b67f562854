"""Host side of tests/test_layout_update_gpu.py, no GPU needed.

1. tests/layout_oracle.py against torch permute / reshape / tap-slicing restatements of the same weights, for the layout
   maps that ops.ConvLayer (conv and deconv), the four ops._tconv parity classes and ops.DenseLayer (plain, in_perm,
   out_perm) actually build, in both orientations -- so that the oracle is not the kernels' index formula again -- and
   unpack_ref as the inverse of pack_ref.
2. The GPU module's table against the library's host functions: fmri_pack_entry_fill / fmri_apply_entry_fill return the
   block counts include/fmri_hip.h documents, and 0 for exactly the maps it calls ineligible.
"""
import ctypes

import numpy as np
import pytest
import torch

import layout_oracle as LO
import test_layout_update_gpu as T


class _G:
    """Minimal FlatGroup stand-in on the CPU: the layer constructors only size and zero their fp16 copies."""

    def __init__(self, tensors):
        self.views = {k: v.contiguous() for k, v in tensors.items()}
        self.grads = {k: torch.zeros_like(v) for k, v in self.views.items()}
        self.version = 0
        self.device = torch.device("cpu")


@pytest.fixture(scope="module")
def lib():
    from fmri_hip import build, lib as L
    build.build(verbose=False)
    return L.load()


def _padded(x3, rows_pad, kpad):
    """[rows][taps][B] -> the packed matrix [rows_pad][kpad]: channels padded to 8 per tap, zero fill."""
    rows, nt, b = x3.shape
    bp = LO.pad8(b)
    out = torch.zeros(rows_pad, kpad, dtype=torch.float64)
    out[:rows, :nt * bp].view(rows, nt, bp)[:, :, :b] = x3
    return out.numpy()


def _blocks(pw):
    return list(zip(pw.specs, pw.kpads, pw.offsets))


def _check_pack(w, pw, restate):
    """Every block of PackedWeight ``pw``: pack_ref of the flat weight == ``restate(spec)`` ([rows][taps][B], torch)."""
    for sp, kpad, _ in _blocks(pw):
        got = LO.pack_ref(w.numpy().ravel(), sp, pw.rows_pad, kpad)
        x3 = restate(sp)
        assert x3.shape == (sp.TA * sp.A, sp.TH * sp.TW, sp.B), (x3.shape, sp)
        assert np.array_equal(got, _padded(x3, pw.rows_pad, kpad)), sp


def _check_inverse(w, pw):
    """unpack_ref(pack_ref(w)) == w: each full-tap block alone, the four parity classes together (``into``)."""
    flat = w.numpy().ravel()
    back = np.zeros(flat.size)
    for sp, kpad, _ in _blocks(pw):
        packed = LO.pack_ref(flat, sp, pw.rows_pad, kpad)
        back = LO.unpack_ref(packed[None], sp, kpad, 1.0, into=back)
        if len(pw.specs) == 1:
            assert np.array_equal(LO.unpack_ref(packed, sp, kpad, 1.0), flat)
            two = LO.unpack_ref(np.stack([packed, 3.0 * packed]), sp, kpad, 0.5)        # slab sum and scale
            assert np.array_equal(two, 2.0 * flat)
    assert np.array_equal(back, flat), "the blocks together do not cover the weight exactly once"


def _taps(x4, sp):
    """[rows][k][k][B] -> the taps of one class ([rows][TH * TW][B]) by slicing: rows py, py + step, ..."""
    sl = x4[:, sp.py::sp.step, sp.px::sp.step, :] if sp.step > 1 else x4
    assert sl.shape[1:3] == (sp.TH, sp.TW), (sl.shape, sp)
    return sl.reshape(x4.shape[0], sp.TH * sp.TW, x4.shape[3])


@pytest.mark.parametrize("k,stride", [(5, 1), (5, 2), (3, 1)])
@pytest.mark.parametrize("cin,cout", [(3, 5), (12, 7)])
def test_conv_layer_maps(lib, cin, cout, k, stride):
    from fmri_hip import ops
    torch.manual_seed(cin * 100 + cout + k)
    w = torch.randn(cout, cin, k, k, dtype=torch.float64).float()
    layer = ops.ConvLayer(_G({"w": w}), "w", None, "conv", cin, cout, k, stride, k // 2)
    wd = w.double()
    # forward: rows co, columns (ky, kx, ci)
    _check_pack(w, layer.pw_f, lambda sp: wd.permute(0, 2, 3, 1).reshape(cout, k * k, cin))
    # data gradient: rows ci, columns (ky, kx, co) -- all taps (stride 1) or the taps of one parity class (stride 2)
    assert len(layer.pw_d.specs) == (4 if stride == 2 else 1)
    _check_pack(w, layer.pw_d, lambda sp: _taps(wd.permute(1, 2, 3, 0), sp))
    assert layer.gspec == layer.pw_f.specs[0]
    for pw in (layer.pw_f, layer.pw_d):
        _check_inverse(w, pw)


@pytest.mark.parametrize("cin,cout", [(6, 4), (9, 16)])
def test_deconv_layer_maps(lib, cin, cout):
    from fmri_hip import ops
    torch.manual_seed(cin * 10 + cout)
    k = 5
    w = torch.randn(cin, cout, k, k, dtype=torch.float64).float()
    layer = ops.ConvLayer(_G({"w": w}), "w", None, "deconv", cin, cout, k, 2, 2, 1)
    wd = w.double()
    assert len(layer.pw_f.specs) == 4
    # forward: rows co, columns (class taps, ci); data gradient and weight gradient: rows ci, columns (ky, kx, co)
    _check_pack(w, layer.pw_f, lambda sp: _taps(wd.permute(1, 2, 3, 0), sp))
    _check_pack(w, layer.pw_d, lambda sp: wd.permute(0, 2, 3, 1).reshape(cin, k * k, cout))
    assert layer.gspec == layer.pw_d.specs[0]
    for pw in (layer.pw_f, layer.pw_d):
        _check_inverse(w, pw)


def test_tconv_classes_of_the_table_are_the_library_s(lib):
    """The class geometry written into the GPU module's table is what fmri_tconv_class answers for k = 5, pad = 2, and
    what ops._tconv builds from it."""
    from fmri_hip import lib as L, ops
    for (cy, cx), (py, px, th, tw) in T.CLASSES_K5P2.items():
        g = L.tconv_class(5, 2, cy, cx, 40, 32)
        assert (g["py"], g["px"], g["th"], g["tw"]) == (py, px, th, tw)
    w = torch.zeros(40, 6, 5, 5)
    layer = ops.ConvLayer(_G({"w": w}), "w", None, "conv", 6, 40, 5, 2, 2)
    mine = [c.spec for c in T.CASES if c.spec.step == 2]
    assert [tuple(T.spec_args(sp)) for sp in layer.pw_d.specs] == [tuple(T.spec_args(sp)) for sp in mine]


@pytest.mark.parametrize("perm", ["plain", "in_perm", "out_perm"])
@pytest.mark.parametrize("C,HW,other", [(8, 16, 5), (16, 9, 12), (8, 100, 3)])
def test_dense_layer_maps(lib, perm, C, HW, other):
    from fmri_hip import ops
    torch.manual_seed(C + HW + other)
    if perm == "in_perm":
        N, K = other, C * HW
        kw = dict(in_perm=(C, HW))
    elif perm == "out_perm":
        N, K = C * HW, other
        kw = dict(out_perm=(C, HW))
    else:
        N, K = other, C * HW
        kw = {}
    w = torch.randn(N, K, dtype=torch.float64).float()
    layer = ops.DenseLayer(_G({"w": w}), "w", None, K, N, **kw)
    wd = w.double()
    if perm == "in_perm":
        # the engine's input features are (hw, c), the reference's (c, hw)
        eng = wd.reshape(N, C, HW).permute(0, 2, 1).reshape(N, K)
        fwd = lambda sp: eng.reshape(N, HW, C)                           # rows n, 'taps' hw, channels c
        dgr = lambda sp: eng.t().reshape(K, 1, N)                        # rows (hw, c), one tap, channels n
    elif perm == "out_perm":
        # the engine's output features are (hw, c), the reference's (c, hw)
        eng = wd.reshape(C, HW, K).permute(1, 0, 2).reshape(N, K)
        fwd = lambda sp: eng.reshape(N, 1, K)                            # rows (hw, c)
        dgr = lambda sp: eng.reshape(HW, C, K).permute(2, 0, 1)          # rows k, 'taps' hw, channels c
    else:
        fwd = lambda sp: wd.reshape(N, 1, K)
        dgr = lambda sp: wd.t().reshape(K, 1, N)
    _check_pack(w, layer.pw_f, fwd)
    _check_pack(w, layer.pw_d, dgr)
    assert layer.gspec == layer.pw_f.specs[0]
    for pw in (layer.pw_f, layer.pw_d):
        _check_inverse(w, pw)
    # the GPU module's constructors restate the same maps
    f, d, n = T._dense(N, K, **kw)
    assert tuple(T.spec_args(f)) == tuple(T.spec_args(layer.pw_f.specs[0]))
    assert tuple(T.spec_args(d)) == tuple(T.spec_args(layer.pw_d.specs[0])) and n == w.numel()


def test_conv_maps_of_the_table_are_the_layers(lib):
    from fmri_hip import ops
    for cout, cin, k in ((5, 3, 5), (2, 130, 5), (7, 3, 3)):
        layer = ops.ConvLayer(_G({"w": torch.zeros(cout, cin, k, k)}), "w", None, "conv", cin, cout, k, 1, k // 2)
        assert tuple(T.spec_args(T._conv_f(cout, cin, k)[0])) == tuple(T.spec_args(layer.pw_f.specs[0]))
        assert tuple(T.spec_args(T._conv_d(cout, cin, k)[0])) == tuple(T.spec_args(layer.pw_d.specs[0]))


def test_rmsprop_ref_is_torch_rmsprop_in_float64():
    torch.manual_seed(5)
    n = 501
    p = torch.randn(n, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.RMSprop([p], lr=1e-4, alpha=float(np.float32(0.9)), eps=1e-8)
    w, sq = p.detach().numpy().copy(), np.zeros(n)
    for lr in (1e-4, 5e-5, 2e-4):
        g = torch.randn(n, dtype=torch.float64) * 3.0
        opt.param_groups[0]["lr"] = float(np.float32(lr))
        p.grad = (g / 4.0).clamp(-0.5, 0.5)
        opt.step()
        w, sq = LO.rmsprop_ref(w, sq, g.numpy(), lr, 0.9, 1e-8, 1.0, 4.0, 0.5)
    assert np.abs(w - p.detach().numpy()).max() <= 1e-15
    assert np.abs(sq - opt.state[p]["square_avg"].numpy()).max() <= 1e-15


def test_table_routes_and_block_counts_without_gpu(lib):
    """The statements of the GPU module's table against the library's host code, with fake non-null pointers: blocks
    rows * ceil(B / 32) from fmri_pack_entry_fill for the maps the batched pack kernel takes, 0 for the others;
    rows * ceil(B / bt) (bt = 64 iff B >= 64) for apply kind 0, ceil(rows * B / 1024) for kind 1, ceil(n / 1024) for a flat
    segment, and 0 for exactly the ineligible maps: the three the header names -- a tap run above 64, a tap subset (the
    step-2 classes), a single tap whose b stride is not 1 -- and the one apply_entry_tiles adds, several taps that are not
    contiguous in the reference layout (stb != 1: the tapped out_perm data-gradient maps)."""
    pe = ctypes.create_string_buffer(lib.fmri_pack_entry_bytes())
    ae = ctypes.create_string_buffer(lib.fmri_apply_entry_bytes())
    P = ctypes.c_void_p
    w, sq, g, src, pk = P(0x10000), P(0x20000), P(0x30000), P(0x40000), P(0x50000)
    zero_apply = []
    for c in T.CASES:
        sp = c.spec
        rows, rows_pad, kpad = T.geometry(sp)
        nt, run = sp.TH * sp.TW, T.run_of(sp)
        assert T.routes(sp) == (c.pack, c.unpack, c.apply), c.name
        n = lib.fmri_pack_entry_fill(pe, src, pk, *T.spec_args(sp), rows_pad, kpad, 0)
        if nt > 1 and sp.stb == 1 and run <= 64:
            assert n == rows * ((sp.B + 31) // 32) > 0 and c.pack == "tile", (c.name, n)
        else:
            assert n == 0 and c.pack != "tile", (c.name, n)
        n = lib.fmri_apply_entry_fill(ae, src, w, sq, g, pk, *T.spec_args(sp), kpad, kpad, 2, rows * kpad, 1, 0.5, 0, 7)
        ineligible = run > 64 or sp.step == 2 or (nt == 1 and sp.sb != 1) or (nt > 1 and sp.stb != 1)
        if ineligible:
            assert n == 0 and c.apply is None, (c.name, n)
            zero_apply.append(c.name)
        elif nt > 1:
            bt = 64 if sp.B >= 64 else 32
            assert n == rows * ((sp.B + bt - 1) // bt) and c.apply == 0, (c.name, n)
        else:
            assert n == (rows * sp.B + 1023) // 1024 and c.apply == 1, (c.name, n)
    assert len(zero_apply) == sum(c.apply is None for c in T.CASES) >= 8
    for flat in T.FLAT_LENGTHS + (1024, 1 << 20):
        n = lib.fmri_apply_entry_fill(ae, None, w, sq, g, None, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 1, 0, 0, 1.0, flat, 0)
        assert n == (flat + 1023) // 1024, (flat, n)
    # every reason of ineligibility is in the table
    reasons = {"run": any(T.run_of(c.spec) > 64 for c in T.CASES), "class": any(c.spec.step == 2 for c in T.CASES),
               "single tap, sb != 1": any(c.spec.TH * c.spec.TW == 1 and c.spec.sb != 1 for c in T.CASES),
               "taps not contiguous": any(c.spec.TH * c.spec.TW > 1 and c.spec.stb != 1 for c in T.CASES)}
    assert all(reasons.values()), reasons


def test_apply_rows_of_the_gpu_module_mix_what_they_claim():
    rows = T._apply_rows()
    assert len(rows) + len(T.FLAT_LENGTHS) > 64
    for kind in (0, 1):
        mine = [r for r in rows if r.case.apply == kind]
        assert {r.nslabs for r in mine} == set(T.NSLABS)
        assert {(r.clear, r.has_pk) for r in mine} == {(a, b) for a in (True, False) for b in (True, False)}
    k0 = [r for r in rows if r.case.apply == 0]
    assert {r.ld - r.case.spec.TH * r.case.spec.TW * LO.pad8(r.case.spec.B) for r in k0 if r.clear} == {0, 8, 24}
    assert all(np.log2(r.scale) == int(np.log2(r.scale)) for r in rows)
