"""Host side of tests/test_fullbatch_conv_gpu.py, no GPU needed: the float64 slicing-and-matmul reference
(tests/conv_oracle.py) against torch's float64 convolutions and autograd on the CPU, and the weight-gradient route table
of the GPU module against the library's own host functions, with the conditions the table as a whole has to cover."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import conv_oracle as CO
import test_fullbatch_conv_gpu as T

RTOL = 1e-12


def _rel(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / ref.abs().max())


SIZES = [(9, 11), (13, 7), (16, 16), (25, 25), (50, 50)]


@pytest.mark.parametrize("chunk", [None, 1, 2])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("H,W", SIZES)
def test_conv_oracle_matches_float64_torch(H, W, stride, chunk):
    torch.manual_seed(H * 31 + W + stride)
    N, cin, cout = 3, 5, 7
    x = torch.randn(N, cin, H, W, dtype=torch.float64, requires_grad=True)
    w = torch.randn(cout, cin, 5, 5, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, stride, 2)
    dy = torch.randn_like(y)
    y.backward(dy)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    assert _rel(CO.conv_fwd(nhwc(x), w.detach(), stride, 2, chunk), nhwc(y)) <= RTOL
    assert _rel(CO.conv_dgrad(nhwc(dy), w.detach(), stride, 2, H, W, chunk), nhwc(x.grad)) <= RTOL
    assert _rel(CO.conv_wgrad(nhwc(x), nhwc(dy), 5, stride, 2, chunk), w.grad) <= RTOL
    assert _rel(CO.bias_grad(nhwc(dy)), dy.sum((0, 2, 3))) <= RTOL


@pytest.mark.parametrize("chunk", [None, 1, 2])
@pytest.mark.parametrize("out_pad", [0, 1])
@pytest.mark.parametrize("H,W", SIZES)
def test_deconv_oracle_matches_float64_torch(H, W, out_pad, chunk):
    torch.manual_seed(H * 17 + W + out_pad)
    N, cin, cout = 3, 6, 4
    x = torch.randn(N, cin, H, W, dtype=torch.float64, requires_grad=True)
    w = torch.randn(cin, cout, 5, 5, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(x, w, None, 2, 2, output_padding=out_pad)
    dy = torch.randn_like(y)
    y.backward(dy)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    assert y.shape[2] == CO.deconv_out_size(H, 5, 2, 2, out_pad) and y.shape[3] == CO.deconv_out_size(W, 5, 2, 2, out_pad)
    assert _rel(CO.deconv_fwd(nhwc(x), w.detach(), 2, 2, out_pad, chunk), nhwc(y)) <= RTOL
    assert _rel(CO.deconv_dgrad(nhwc(dy), w.detach(), 2, 2, chunk), nhwc(x.grad)) <= RTOL
    assert _rel(CO.deconv_wgrad(nhwc(x), nhwc(dy), 5, 2, 2, chunk), w.grad) <= RTOL


def test_chunks_keep_the_temporaries_of_the_largest_layers_near_one_gib():
    for name, (kind, cin, cout, stride, H, op, N) in T.CASES:
        Ho = T.geometry(kind, cin, cout, stride, H, op, N)["Ho"]
        n = T._chunk((kind, cin, cout, stride, H, op, N), Ho)
        big_hw, big_c, small_hw, small_c = ((H, cin, Ho, cout) if kind == "conv" else (Ho, cout, H, cin))
        worst = 8 * n * max((big_hw + 4) ** 2 * big_c, small_hw ** 2 * max(big_c, small_c))
        assert 1 <= n <= N and (worst <= 2 ** 30 or n == 1), (name, n, worst)


# ---------------------------------------------------------------------------------------------------------------------
# the route table
# ---------------------------------------------------------------------------------------------------------------------
def test_plane_pieces_restatement_agrees_with_the_library():
    """max over the planes of T.plane_pieces == fmri_wgrad_slabs, over a sweep of tile counts and budgets."""
    from fmri_hip import lib
    L = lib.load()
    for N in list(range(1, 70)) + [96, 128, 256, 512, 768, 1000]:
        for Yc in (2, 8, 13, 16, 32):
            ntiles = N * ((Yc + 7) // 8) ** 2
            for splits in (1, 4, 5, 8, 10, 16, 20, 32, 40, 64, 80, 128, 160, 256):
                assert max(T.plane_pieces(ntiles, splits)[1]) == L.fmri_wgrad_slabs(N, Yc, Yc, 5, 2, splits), \
                    (N, Yc, splits)


def test_route_table_is_what_the_library_and_run_wgrad_give():
    """ROUTES, written out in the GPU module, is what the code that runs decides: ops.wgrad_plan (fmri_wgrad_route, the
    plan run_wgrad launches) per case and setting; the slab counts behind it are the library's (fmri_wgrad_slabs,
    fmri_wgrad_narrow_blocks); the policy constants are ops' defaults.  (With a kernel family switched off its rows fail.)"""
    from fmri_hip import lib, ops
    L = lib.load()
    assert (ops._WW_SLABS, ops._WW_SIDE_BLOCKS, ops._WW_BLOCKS) == (24, 160, 0)
    assert set(T.ROUTES) == {name for name, _ in T.CASES} and len(T.CASES) == 44
    for name, case in T.CASES:
        kind, cin, cout, stride, H, op, N = case
        g = T.geometry(*case)
        for si, setting in enumerate(T.SETTINGS):
            plan = T.case_plan(case, setting)
            route = T.plan_route(plan)
            assert T.ROUTES[name][si] == route, (name, setting, T.ROUTES[name][si], route)
            assert 0 <= plan.stored <= plan.slabs and plan.colsum == (route[0] == "narrow"), (name, setting, plan)
            kern, mode, splits, detail = route
            print(f"[fullbatch-conv] route {name:28s} {setting:16s} {kern:8s} atomic={mode} splits={splits:3d} {detail}")
            if kern == "win":
                assert max(detail) == L.fmri_wgrad_slabs(N, g["Yc"], g["Yc"], 5, 2, splits), (name, setting)
                assert (mode == 2) == (max(detail) <= 24 or setting == "deterministic")
            elif kern == "narrow":
                assert detail == (L.fmri_wgrad_narrow_blocks(N, g["Yc"], g["Yc"]) if setting == "deterministic" else 4)
            else:
                assert mode in (0, 1, 4) and (mode == 4) == (setting == "deterministic" and splits > 1)


def _win(setting_filter=None):
    """(name, setting, mode, splits, ntiles, tiles per piece, pieces) of every window-kernel route of the table."""
    out = []
    for name, case in T.CASES:
        g = T.geometry(*case)
        ntiles = case[6] * ((g["Yc"] + 7) // 8) ** 2
        for si, setting in enumerate(T.SETTINGS):
            kern, mode, splits, detail = T.ROUTES[name][si]
            if kern == "win":
                tps, pieces = T.plane_pieces(ntiles, splits)
                assert pieces == detail
                out.append((name, setting, mode, splits, ntiles, tps, pieces))
    return out


def test_route_table_covers_the_piece_edges():
    """What the table as a whole has to hold; a routing change that loses one of these fails here, not silently."""
    win = _win()
    slab = [r for r in win if r[2] == 2]
    unequal = [r for r in slab if len(set(r[6])) > 1]
    assert unequal, "window kernel, slab mode, unequal plane pieces"
    # at scale: pieces of 150 - 770 tiles with a shorter last piece, 6 - 10 slabs, under both budgets
    at_scale = [r for r in unequal if min(r[5]) >= 150 and max(r[5]) <= 770 and 6 <= max(r[6]) <= 10
                and any(r[4] % t for t in r[5])]
    assert {r[1] for r in at_scale} == set(T.SETTINGS), at_scale
    assert any(r[4] == 3072 and r[5][0] == 308 and r[4] - 9 * 308 == 300 for r in at_scale), "300 of 308"
    # a last piece of exactly one tile, on a plane with more than one piece
    assert any(p > 1 and r[4] - (p - 1) * t == 1 for r in slab for t, p in zip(r[5], r[6])), "one-tile last piece"
    # some planes clamped to the tile count and others not
    clamped = [[aim > r[4] for aim in T.planned_pieces(r[4], r[3])] for r in slab]
    assert any(any(c) and not all(c) for c in clamped), "planes clamped to ntiles beside planes that are not"
    # atomic mode of the window kernel, on the 32- and on the 64-channel layers
    atomic = {T.geometry(*dict(T.CASES)[r[0]])["Bc"] for r in win if r[2] == 1}
    assert atomic == {32, 64}, atomic
    # deterministic mode turns those into more than 24 slabs
    assert any(r[2] == 2 and max(r[6]) > 24 and r[1] == "deterministic" for r in win)
    routes = [(name, T.geometry(*case), T.ROUTES[name]) for name, case in T.CASES]
    narrow = [(n, g, r) for n, g, r in routes if r[0][0] == "narrow"]
    assert any(not g["flip"] for _, g, _ in narrow), "narrow kernel, direct"
    assert any(g["flip"] for _, g, _ in narrow), "narrow kernel, role-exchanged"
    assert any(g["flip"] and dict(T.CASES)[n][6] * (g["Yc"] // 8) ** 2 == 32768 for n, g, _ in narrow), "exactly 32 768 tiles"
    assert all(r[2] == ("narrow", 3, 768, 768) for _, _, r in narrow), "one slab per block in deterministic mode"
    generic = [r for _, _, r in routes if r[0][0] == "generic"]
    assert any(r[0][1] == 1 and r[0][2] > 1 for r in generic), "generic kernel, K splits in atomic mode"
    assert any(r[2][1] == 4 and r[2][3] == r[2][2] for r in generic), "generic kernel, slab mode 4, every slab stored"
    assert any(r[2][1] == 4 and 0 < r[2][3] < r[2][2] for r in generic), "slab mode 4, fewer slabs stored than allocated"
    # ... at two different ratios at least (the K steps of the 100-px planes do not divide by the split count)
    short = {(r[2][3], r[2][2]) for r in generic if r[2][1] == 4 and 0 < r[2][3] < r[2][2]}
    assert len({stored / alloc for stored, alloc in short}) >= 2 and {(278, 312), (500, 512), (22, 24)} <= short, short
    # the role-exchanged generic route with 64-row tiles (decoder.conv.3 at 64 input channels)
    assert any(g["flip"] and g["A"] == 64 and r[0][0] == "generic" and r[0][2] > 1 and r[2][1] == 4
               for _, g, r in routes), "generic kernel, role-exchanged, 64-row tiles"
    # window-kernel pieces of fewer than 8 tiles on planes of partial tiles (a plane side that is no multiple of 8)
    partial = [r for r in slab if T.geometry(*dict(T.CASES)[r[0]])["Yc"] % 8 and min(r[5]) < 8]
    assert {r[1] for r in partial} == set(T.SETTINGS), "pieces of fewer than 8 tiles, partial tiles, every setting"
    assert any(min(r[5]) == 2 for r in partial) and any(max(r[5]) == 5 for r in partial), "2 - 5 tiles per piece"


# ---------------------------------------------------------------------------------------------------------------------
# the recorded sweep: what run_wgrad decided, per geometry and setting, at the commit before it asked the library's plan
# ---------------------------------------------------------------------------------------------------------------------
ROUTES_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_routes.json")
SWEEP_BATCHES = (1, 2, 3, 4, 5, 8, 16, 32, 64, 100, 128, 255, 256, 257, 512)
SETTING_FLAGS = ((True, False), (False, False), (True, True))       # (side stream, deterministic) of T.SETTINGS
ROUTE_KERNELS = ["fmri::wgrad_win_kernel", "fmri::wgrad_narrow_kernel", "fmri::wgrad_kernel"]


def sweep_geometries():
    """(N, Yc, Xc, A, Hq, Wq, Bc, k, stride, pad, flip) as ConvLayer._wgrad / DenseLayer._wgrad hand them to run_wgrad:
    the FULL_SIZE, PX100_LAYERS and DENSE_TABLE layers at SWEEP_BATCHES samples times the layer's images per sample (255,
    256 and 257 straddle the narrow kernel's 32 768 tiles, the dense rows the generic kernel's 512 output tiles)."""
    import test_fullbatch_ops_gpu as D
    from fmri_hip.ops import pad8
    layers = [(case[:6], case[6] // (256 if i < 11 else 128)) for i, (_, case) in enumerate(T.CASES[:19])]
    layers += [(row[1:7], row[7]) for row in T.PX100_LAYERS]
    per_sample = lambda name: 3 if name.startswith("discriminator") else 2 if name.startswith(("decoder", "latent")) else 1
    dense = [(c[1], c[2], per_sample(c[0])) for c in D.DENSE_TABLE]
    out = []
    for B in SWEEP_BATCHES:
        for shape, per in layers:
            g = T.geometry(*shape, B * per)
            out.append((B * per, g["Yc"], g["Yc"], g["A"], g["Hq"], g["Hq"], g["Bc"], T.K5, g["stride"], T.PAD, g["flip"]))
        out += [(B * per, 1, 1, pad8(N), 1, 1, pad8(K), 1, 1, 0, 0) for K, N, per in dense]
    return list(dict.fromkeys(out))


def route_by_run_wgrad(geo, side, det):
    """[kernel-name prefix, atomic, splits, buffer shape, zeroed] of one ops.run_wgrad call on the CPU: lib.call,
    lib.note and ops._grad_buffer are recorders for its duration, the operands one-element tensors."""
    from fmri_hip import lib, ops
    seen, one = {}, torch.zeros(1, dtype=torch.float16)
    saved = (lib.call, lib.note, lib.PROFILE, ops._grad_buffer, ops._SIDE["on"], ops._DET["on"])

    def buffer(hold, shape, zeroed, device):
        seen["buffer"] = [list(shape), bool(zeroed)]
        return one

    lib.call = lambda name, *a: seen.update(call=(name, a))
    lib.note = lambda **kw: seen.update(kernel=kw["kernel"])
    lib.PROFILE, ops._grad_buffer, ops._SIDE["on"], ops._DET["on"] = [], buffer, side, det
    try:
        ops.run_wgrad(one, one, *geo)
    finally:
        lib.call, lib.note, lib.PROFILE, ops._grad_buffer, ops._SIDE["on"], ops._DET["on"] = saved
    name, a = seen["call"]
    assert name == "fmri_wgrad_if" and tuple(a[5:16]) == tuple(geo), (name, a)
    return [seen["kernel"].split("<")[0], a[20], a[19]] + seen["buffer"]


def route_by_plan(geo, side, det):
    """The same five values from ops.wgrad_plan."""
    from fmri_hip import ops
    p = ops.wgrad_plan(*geo, side=side, det=det)
    apad, ldo = ops.ceil_to(geo[3], ops.tile_for(geo[3])), ops.ceil_to(geo[7] * geo[7] * geo[6], 128)
    return [p.kernel.split("<")[0], p.atomic, p.splits, ([p.slabs] if p.slabs else []) + [apad, ldo], p.zeroed]


def write_routes_json(route=route_by_run_wgrad):
    """tests/golden/make_golden.py: one compact row per geometry -- the eleven run_wgrad arguments, then per setting
    [index into ``kernels``, atomic, splits, buffer shape, zeroed (0 / 1)]."""
    rows = []
    for geo in sweep_geometries():
        per = [route(geo, side, det) for side, det in SETTING_FLAGS]
        rows.append(list(geo) + [[ROUTE_KERNELS.index(r[0]), r[1], r[2], r[3], int(r[4])] for r in per])
    head = json.dumps({"settings": list(T.SETTINGS), "kernels": ROUTE_KERNELS}, separators=(",", ":"))
    with open(ROUTES_JSON, "w") as f:
        f.write(head[:-1] + ',"rows":[\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]}\n")
    return len(rows)


def test_recorded_routes_replay_through_the_plan_and_through_run_wgrad():
    """Every row of tests/golden/wgrad_routes.json -- kernel, ``atomic``, ``splits``, buffer shape, zeroed, recorded off
    run_wgrad before the routing moved into fmri_wgrad_route -- is what ops.wgrad_plan states and what run_wgrad hands
    to its launch today, for the whole sweep and the three settings."""
    assert os.path.getsize(ROUTES_JSON) < 100 * 1024
    with open(ROUTES_JSON) as f:
        doc = json.load(f)
    assert doc["settings"] == list(T.SETTINGS) and doc["kernels"] == ROUTE_KERNELS
    assert [tuple(r[:11]) for r in doc["rows"]] == sweep_geometries()
    families = set()
    for row in doc["rows"]:
        geo = tuple(row[:11])
        for (side, det), (kern, atomic, splits, shape, zeroed) in zip(SETTING_FLAGS, row[11:]):
            recorded = [ROUTE_KERNELS[kern], atomic, splits, shape, bool(zeroed)]
            assert route_by_plan(geo, side, det) == recorded, (geo, side, det)
            assert route_by_run_wgrad(geo, side, det) == recorded, (geo, side, det)
            families.add((kern, atomic))
    assert families == {(0, 1), (0, 2), (1, 3), (2, 0), (2, 1), (2, 4)}, families


def test_cases_are_the_full_size_list_plus_the_edges():
    from test_kernels_gpu import FULL_SIZE
    assert [c for _, c in T.CASES[:19]] == list(FULL_SIZE)
    assert len({n for n, _ in T.CASES}) == len(T.CASES)
    # the epilogue layers are the stride-1 / stride_gan first discriminator layer and the decoder's last layer
    for name, act in T.EPILOGUE.items():
        kind, cin, cout = dict(T.CASES)[name][:3]
        assert (kind, cin, cout) in ([("conv", 3, 32)] if act == T.RELU else [("conv", 32, 3), ("conv", 64, 3)])
    tanh_layers = {n for n, act in T.EPILOGUE.items() if act == T.TANH}
    assert tanh_layers == {"decoder.conv.3", "decoder.conv.3 @128", "decoder.conv.3 @100"}
    assert {dict(T.CASES)[n][:3] for n in tanh_layers} == {("conv", 32, 3), ("conv", 64, 3)}
    # the 100-px family: the eleven layers at the shipped batch and at the remainder batch, in that order
    assert [n for n, _ in T.CASES[22:]] == [n for n, _ in T.PX100_CASES] and len(T.PX100_CASES) == 22
    assert [c[6] for _, c in T.PX100_CASES] == [64] * 3 + [128] * 4 + [192] * 4 + [5] * 3 + [10] * 4 + [15] * 4


# ---------------------------------------------------------------------------------------------------------------------
# forward / data-gradient kernels of the 100-px family
# ---------------------------------------------------------------------------------------------------------------------
def _launches():
    """(case name, kernel family, instantiation, epilogue or None, side of the plane the kernel tiles) of every launch
    KERNELS states.  The window kernels of the stride-2 convolution (c5 / c5w) tile the output plane, those of the
    transposed convolution (tc5 / tc5w / tc32) the parity-class grid, ceil(output side / 2); the generic kernel tiles
    the flattened pixels of all images in 128."""
    out = []
    for name, case in T.PX100_CASES:
        kind, cin, cout, stride, H, op, N = case
        Ho = T.geometry(*case)["Ho"]
        fwd_out, dgr_out = Ho, H                                       # output plane of the forward / the data gradient
        for which, kname in enumerate(T.KERNELS[name]):
            if kname is None:
                continue
            side = fwd_out if which < 2 else dgr_out
            family = kname.split("::")[1].split("<")[0]
            ep = T.EPILOGUE.get(name) if which == 1 else None
            if family == "igemm_kernel":
                out.append((name, family, kname, ep, N * side * side, 128))
            elif family in ("igemm_c5_kernel", "igemm_c5w_kernel"):
                out.append((name, family, kname, ep, side, 8))
            else:
                assert family in ("igemm_tc5_kernel", "igemm_tc5w_kernel", "igemm_tc32_kernel"), kname
                out.append((name, family, kname, ep, (side + 1) // 2, 8))
    return out


def test_kernel_table_is_what_the_library_routes_to_and_covers_the_families():
    """KERNELS, written out in the GPU module, equals what ops.igemm_route gives for the arguments ConvLayer hands over
    (no GPU: the library's routing is host code); and the family as a whole meets every window kernel and the generic
    kernel on a plane that is no multiple of its tile, the generic kernel also with the tanh epilogue."""
    assert set(T.KERNELS) == {n for n, _ in T.PX100_CASES}
    for name, case in T.PX100_CASES:
        got = T.igemm_kernels(name, case)
        assert got == T.KERNELS[name], (name, got, T.KERNELS[name])
        print(f"[fullbatch-conv] kernels {name:32s} {got}")
    launches = _launches()
    # every tile edge of the window kernels is 8 or 16 (8 x 8, 8 x 16, 16 x 16): a side that is no multiple of 8 is a
    # multiple of none of them; the generic kernel's last 128-pixel tile is partial when the pixel count is no multiple
    ragged = {family for _, family, _, _, extent, tile in launches if extent % tile}
    assert {"igemm_tc5_kernel", "igemm_tc5w_kernel", "igemm_tc32_kernel", "igemm_kernel"} <= ragged, ragged
    assert ragged & {"igemm_c5_kernel", "igemm_c5w_kernel"}, ragged
    assert any(family == "igemm_kernel" and ep == T.TANH for _, family, _, ep, _, _ in launches), \
        "generic kernel with the tanh epilogue"
    assert any(family == "igemm_kernel" and ep == T.RELU for _, family, _, ep, _, _ in launches)
    # both tile widths of the wide window kernels, and the ReLU-mask form of igemm_tc32, on such planes
    names = {kname for _, _, kname, _, extent, tile in launches if extent % tile}
    assert {"fmri::igemm_c5w_kernel<16,0>", "fmri::igemm_c5w_kernel<8,0>", "fmri::igemm_tc32_kernel<true>"} <= names
    assert any(k.startswith("fmri::igemm_tc5w_kernel<16,") for k in names)
    assert any(k.startswith("fmri::igemm_tc5w_kernel<8,") for k in names)
