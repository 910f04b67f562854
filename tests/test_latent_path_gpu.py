"""The kernels between encoder and decoder (csrc/loss.hip fmri_latent_fwd / fmri_latent_bwd) and the fused WAE latent
discriminator (csrc/mlp.hip fmri_mlp_fwd / fmri_mlp_bwd), every element of every output against the float64 references of
tests/latent_oracle.py:

  A. the latent kernels through lib.call: padding columns (zp > Z), widths that are no multiple of the 64 lanes, one row,
     partial last blocks, the one-block deterministic launch, sample = 0, every NULL-able argument, the += into *kl_total,
     and one backward case large enough for a second pass of the grid-stride loop;
  B. the fused MLP through lib.call, one layer at a time and teacher-forced on the kernel's own previous layer, under
     bounds derived from the number formats (see the oracle's docstring): row counts around the 32-row block, the four
     widths of the backward and the two only the forward takes, Z < Zp, every NULL-able argument, nonzero bias-gradient
     priors, sentinel rows behind M and the one-allocation layout of the network;
  C. WaeDiscriminatorNet.forward / .backward at M = 512: weight and bias gradients from the kernel's own cotangents.

tests/test_latent_oracle_host.py shows on the CPU that these comparisons accept float32 arithmetic and reject five subtly
wrong kernels.  Every check prints ``[latent] <case> | <quantity> | err/bound = r``; profiles/latent_path_parity.md
records those of one GPU run.
"""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import latent_oracle as LO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E_BADARG, E_UNSUPPORTED = -1, -2
S16, S32 = 0x5A5A, 0x5A5A5A5A            # sentinel bit patterns (fp16 207.25, fp32 1.5e16)


def _say(case, what, r, asserted=True):
    print(f"[latent] {case} | {what} | err/bound = {r:.4f}" + ("" if asserted else " (report only)"), flush=True)
    if asserted:
        assert r <= 1.0, f"{case}: {what}: err / bound = {r:.4f}"
    return r


@pytest.fixture(params=[False, True], ids=["default", "deterministic"])
def reduction_mode(request):
    from fmri_hip import ops
    was = ops.set_deterministic(request.param)
    try:
        yield request.param
    finally:
        ops.set_deterministic(was)


def _sent16(*shape):
    return torch.full(shape, S16, dtype=torch.int16, device=DEV).view(torch.float16)


def _sent32(*shape):
    return torch.full(shape, S32, dtype=torch.int32, device=DEV).view(torch.float32)


def _is_sent(t):
    if t.dtype == torch.float16:
        return bool((t.view(torch.int16) == S16).all())
    return bool((t.view(torch.int32) == S32).all())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _ptrs(tensors):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


# =====================================================================================================================
# A. fmri_latent_fwd / fmri_latent_bwd
# =====================================================================================================================
@pytest.mark.parametrize("Z,zp", LO.LATENT_ZS, ids=[f"Z{z}-zp{p}" for z, p in LO.LATENT_ZS])
@pytest.mark.parametrize("B", LO.LATENT_B)
def test_latent_fwd(B, Z, zp, reduction_mode):
    """z16 (all of it, padding columns exactly zero), kl_rows and prior + sum in *kl_total against latent_fwd64 under the
    tolerances of test_loss_kernels (2e-3 fp16, 1e-4 rows, 1e-3 total), for sample = 1 and 0 (eps = NULL), plain inputs
    and inputs with the edge entries; z16 bit-identical whichever of kl_rows / kl_total is NULL; the total bit-identical
    over two launches in deterministic mode; a sentinel row behind row B of z16 and kl_rows untouched."""
    from fmri_hip import lib
    P = lib.ptr
    prior = 12.5
    for edges in (False, True):
        head, eps, _ = LO.latent_inputs(B, Z, seed=1000 * B + Z + zp, edges=edges)
        hd, ed = _dev(head), _dev(eps)
        for sample in (1, 0):
            case = (f"A latent_fwd B={B} Z={Z} zp={zp} sample={sample} {'edges' if edges else 'plain'} "
                    f"{'det' if reduction_mode else 'default'}")
            z_ref, klr_ref, klt_ref = LO.latent_fwd64(head, eps, Z, zp, sample)
            e = P(ed) if sample else None
            z16, klr = _sent16(B + 1, zp), _sent32(B + 1)
            klt = torch.full((1,), prior, device=DEV)
            lib.call("fmri_latent_fwd", P(hd), e, B, Z, zp, P(z16), P(klr), P(klt), sample)
            torch.cuda.synchronize()
            assert _is_sent(z16[B:]) and _is_sent(klr[B:]), "written behind row B"
            assert bool((z16[:B, Z:] == 0).all()), "padding columns of z16"
            _say(case, "z16", LO.close_ratio(_np(z16[:B]), z_ref, 2e-3))
            _say(case, "kl_rows", LO.close_ratio(_np(klr[:B]), klr_ref, 1e-4))
            _say(case, "kl_total (prior + sum)", abs(klt.item() - (prior + klt_ref)) / (1e-3 * abs(prior + klt_ref)))
            for rows_null, tot_null in ((True, False), (False, True), (True, True)):
                zb, kb = _sent16(B + 1, zp), _sent32(B + 1)
                kt = torch.full((1,), prior, device=DEV)
                lib.call("fmri_latent_fwd", P(hd), e, B, Z, zp, P(zb), None if rows_null else P(kb),
                         None if tot_null else P(kt), sample)
                torch.cuda.synchronize()
                assert torch.equal(zb.view(torch.int16), z16.view(torch.int16)), ("z16 depends on a NULL", rows_null, tot_null)
                if not rows_null:
                    assert torch.equal(kb.view(torch.int32), klr.view(torch.int32))
                if reduction_mode and not tot_null:
                    assert torch.equal(kt, klt), "deterministic mode: two launches differ in kl_total"


LATENT_BWD = [(B, Z, zp) for B in LO.LATENT_B for Z, zp in LO.LATENT_ZS] + [(2049, 512, 512)]


@pytest.mark.parametrize("B,Z,zp", LATENT_BWD, ids=[f"B{b}-Z{z}-zp{p}" for b, z, p in LATENT_BWD])
def test_latent_bwd(B, Z, zp):
    """dhead32 (1e-4) and dhead16 (2e-3, times out_scale) against latent_bwd64 with dz rows of stride Z, zp and zp + 24
    (NaN between the rows: only columns [0, Z) may be read), dz = NULL, kl_dev NULL / given, out_scale 1 / 16, either
    output NULL, and sample = 0 with an eps buffer of NaN; sentinel rows behind B untouched.  With the edge entries
    (sigma = e^10, exp(logvar) = e^20) the KL weight and dz_unscale are small enough for the fp16 output to stay finite.
    B = 2049, Z = 512 has B * Z > 4096 * 256 elements: the grid-stride loop makes a second pass.  No step of the engine
    reaches that size; it is here because nothing else runs the loop's second pass."""
    from fmri_hip import lib
    P = lib.ptr
    nan_eps = torch.full((B, Z), float("nan"), device=DEV)
    #          ldz       dz     kl_dev sample dhead16 out_scale dhead32
    variants = [(Z,       True,  False, 1,     True,   16.0,     True),
                (zp,      True,  True,  1,     True,   1.0,      False),
                (zp + 24, True,  True,  1,     False,  1.0,      True),
                (Z,       False, False, 1,     True,   16.0,     True),
                (zp + 24, True,  True,  0,     True,   16.0,     True)]
    for edges in (False, True):
        head, eps, dz = LO.latent_inputs(B, Z, seed=7000 + 10 * B + Z + zp, edges=edges)
        kl_w, unscale, kdev = (2e-6, 1.0 / 64, 1.5) if edges else (0.7, 0.5, 3.0)
        hd, ed = _dev(head), _dev(eps)
        kd = torch.tensor([kdev], device=DEV)
        for ldz, has_dz, has_kd, sample, has16, out_scale, has32 in variants:
            case = (f"A latent_bwd B={B} Z={Z} ldz={ldz if has_dz else 'NULL'} kl_dev={'yes' if has_kd else 'NULL'} "
                    f"sample={sample} out_scale={out_scale:g} {'edges' if edges else 'plain'}")
            dzl = np.full((B, ldz), np.nan, np.float32)
            dzl[:, :Z] = dz
            ref, ref_s = LO.latent_bwd64(head, eps, dzl if has_dz else None, ldz, unscale, kl_w, kdev if has_kd else None,
                                         out_scale, sample)
            dzd = _dev(dzl) if has_dz else None
            d16 = _sent16(B + 1, 2 * Z) if has16 else None
            d32 = _sent32(B + 1, 2 * Z) if has32 else None
            lib.call("fmri_latent_bwd", P(hd), P(ed if sample else nan_eps), P(dzd), ldz, unscale, kl_w,
                     P(kd) if has_kd else None, B, Z, out_scale, P(d16), P(d32), sample)
            torch.cuda.synchronize()
            if has32:
                assert _is_sent(d32[B:]), "dhead32 written behind row B"
                _say(case, "dhead32", LO.close_ratio(_np(d32[:B]), ref, 1e-4))
            if has16:
                assert _is_sent(d16[B:]), "dhead16 written behind row B"
                _say(case, "dhead16", LO.close_ratio(_np(d16[:B]), ref_s, 2e-3))


# =====================================================================================================================
# B. fmri_mlp_fwd / fmri_mlp_bwd
# =====================================================================================================================
_NETS = {}


def _weights(Z):
    """The latent discriminator at latent_dim = Z with the oracle's parameters, packed by the project's own DenseLayer /
    fmri_pack_weight as WaeDiscriminatorNet does, and host copies of the fp16 matrices the kernels read."""
    if Z in _NETS:
        return _NETS[Z]
    from fmri_hip import nets
    from fmri_hip.params import ArchConfig
    net = nets.WaeDiscriminatorNet(dataclasses.replace(ArchConfig.px64(), latent_dim=Z), DEV)
    sd = LO.mlp_params(Z)
    net.group.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    L = net.layers
    W = dict(net=net, wf=[l.pw_f.get() for l in L], kp=[l.pw_f.kpads[0] for l in L], b=[l.b for l in L],
             wd=[L[i].pw_d.get() for i in range(4)], kpd=[L[i].pw_d.kpads[0] for i in range(4)])
    torch.cuda.synchronize()
    W["Wf"] = [_np(W["wf"][i].view(L[i].pw_f.rows_pad, W["kp"][i])[:L[i].n_out, :L[i].k_in]) for i in range(5)]
    W["Wd"] = [_np(W["wd"][i].view(L[i].pw_d.rows_pad, W["kpd"][i])[:L[i].k_in, :L[i].n_out]) for i in range(4)]
    W["bs"] = [_np(b) for b in W["b"]]
    for i, idx in enumerate((0, 2, 4, 6, 8)):            # the packed copies are the fp16-rounded masters, both ways
        assert np.array_equal(W["Wf"][i], sd[f"main.{idx}.weight"].astype(np.float16)), f"forward pack of layer {i}"
        if i < 4:
            assert np.array_equal(W["Wd"][i], W["Wf"][i].T), f"data-gradient pack of layer {i}"
    _NETS[Z] = W
    return W


def _run_mlp(W, z16, dl16, M, Zp, Z, priors, *, ldl=8, inv=0.25, bias=True, dbias="all", need_dz=True, production=False,
             backward=True):
    """One forward (+ backward) launch.  Every output buffer has 32 sentinel rows behind row M (``production``: the
    network's layout instead, one [4][M][512] allocation per pass and no slack); they must come back untouched.
    dlogit16 is [M][ldl] with NaN in columns 1...  dbias: "all", None (dbias5 = NULL) or the index of one NULL entry."""
    from fmri_hip import lib
    P = lib.ptr
    slack = 0 if production else 32
    zd = _dev(z16)
    if production:
        hbuf, dbuf = _sent16(4, M, 512), _sent16(4, M, 512)
        hs, delta = [hbuf[i] for i in range(4)], [dbuf[i] for i in range(4)]
    else:
        hs, delta = [_sent16(M + 32, 512) for _ in range(4)], [_sent16(M + 32, 512) for _ in range(4)]
    logit = _sent32(M + slack)
    kps = (ctypes.c_int * 5)(*W["kp"])
    lib.call("fmri_mlp_fwd", P(zd), M, Zp, 512, _ptrs(W["wf"]), kps, _ptrs(W["b"] if bias else [None] * 5), _ptrs(hs),
             P(logit))
    torch.cuda.synchronize()
    out = dict(hs=[_np(h[:M]) for h in hs], logit=_np(logit[:M]), delta=None, dz=None, dbias=None)
    assert all(_is_sent(h[M:]) for h in hs) and _is_sent(logit[M:]), "forward wrote behind row M"
    if not backward:
        return out
    dl = torch.full((M, ldl), float("nan"), dtype=torch.float16, device=DEV)
    dl[:, 0] = _dev(dl16)
    dz = _sent32(M + slack, Z) if need_dz else None
    db = None
    if dbias is not None:
        db = [_dev(p.copy()) for p in priors]
        if dbias != "all":
            db[dbias] = None
    wds = list(W["wd"])
    if not need_dz:
        wds[0] = None
    kpd = (ctypes.c_int * 4)(*W["kpd"])
    lib.call("fmri_mlp_bwd", P(dl), ldl, M, Zp, Z, 512, _ptrs(hs), P(W["wf"][4]), _ptrs(wds), kpd, _ptrs(delta),
             None if db is None else _ptrs(db), P(dz), inv)
    torch.cuda.synchronize()
    assert all(_is_sent(d[M:]) for d in delta), "backward wrote behind row M of delta"
    assert all(np.array_equal(_np(h[:M]), o) for h, o in zip(hs, out["hs"])), "backward changed hs"
    out["delta"] = [_np(d[:M]) for d in delta]
    if need_dz:
        assert _is_sent(dz[M:]), "dz written behind its last row"
        out["dz"] = _np(dz[:M])
    if db is not None:
        out["dbias"] = [None if t is None else _np(t) for t in db]
    return out


def _same(a, b, keys):
    for k in keys:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for x, y in zip(xs, ys):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{k} differs"


def _report(case, out, W, z16, dl16, inv, Z, priors, bias=True):
    rs = LO.mlp_ratios(out, z16, W["Wf"], W["bs"] if bias else [None] * 5, W["Wd"], dl16, inv, Z, priors)
    for what, r in rs.items():
        _say(case, what, r)
    return rs


@pytest.mark.parametrize("M,Z", LO.MLP_SHAPES, ids=[f"M{m}-Z{z}" for m, z in LO.MLP_SHAPES])
def test_mlp_fused_per_element(M, Z):
    """hs[0..3], logit, delta[3..0], dz and the five bias gradients (onto nonzero priors) per element, teacher-forced.
    Launches: (1) biases, ldl = 8, inv_scale = 1/4, all bias gradients, dz; (2) the same again: hs, logit, delta and dz
    bit-identical; (3) the same in the network's [4][M][512] layout without slack: bit-identical again, so no layer's
    store reached row 0 of the next layer's buffer; (4) dbias5 = NULL: delta and dz bit-identical; (5) bias5 all NULL,
    ldl = 1, inv_scale = 1, one NULL entry in dbias5, dz32 = NULL and wd4[0] = NULL."""
    W = _weights(Z)
    z16, dl16, priors = LO.mlp_inputs(M, Z, Z, seed=1000 * Z + M)
    case = f"B mlp M={M} Zp={Z}"
    a = _run_mlp(W, z16, dl16, M, Z, Z, priors)
    assert all(bool((h == 0).any()) for h in a["hs"]), "exact zeros behind the ReLU"
    _report(case, a, W, z16, dl16, 0.25, Z, priors)
    b = _run_mlp(W, z16, dl16, M, Z, Z, priors)
    _same(a, b, ("hs", "logit", "delta", "dz"))
    c = _run_mlp(W, z16, dl16, M, Z, Z, priors, production=True)
    _same(a, c, ("hs", "logit", "delta", "dz"))
    _report(case + " one allocation", c, W, z16, dl16, 0.25, Z, priors)
    d = _run_mlp(W, z16, dl16, M, Z, Z, priors, dbias=None)
    _same(a, d, ("delta", "dz"))
    skip = M % 5
    e = _run_mlp(W, z16, dl16, M, Z, Z, priors, ldl=1, inv=1.0, bias=False, dbias=skip, need_dz=False)
    assert e["dz"] is None and e["dbias"][skip] is None
    rs = _report(case + f" no biases, ldl=1, inv_scale=1, dbias[{skip}]=NULL, dz=NULL", e, W, z16, dl16, 1.0, Z, priors,
                 bias=False)
    assert f"dbias[{skip}]" not in rs and len(rs) == 5 + 4 + 4


def test_mlp_z_narrower_than_zp():
    """Z = 100, Zp = 128 with buffers built here: columns [100, 128) of z16 zero, wd4[0] with 128 rows of which
    [100, 128) are zero, dz [M][100] per element and the float behind its last row's last column untouched."""
    M, Z, Zp = 77, 100, 128
    sd = LO.mlp_params(Z)
    Wf = [sd[f"main.{i}.weight"].astype(np.float16) for i in (0, 2, 4, 6, 8)]
    Wf[0] = np.concatenate([Wf[0], np.zeros((512, Zp - Z), np.float16)], axis=1)
    Wd = [np.ascontiguousarray(w.T) for w in Wf[:4]]
    bs = [sd[f"main.{i}.bias"] for i in (0, 2, 4, 6, 8)]
    W = dict(wf=[_dev(w) for w in Wf], kp=[Zp, 512, 512, 512, 512], b=[_dev(b) for b in bs], wd=[_dev(w) for w in Wd],
             kpd=[512] * 4, Wf=Wf, Wd=Wd, bs=bs)
    assert W["wd"][0].shape == (Zp, 512) and not Wd[0][Z:].any()
    z16, dl16, priors = LO.mlp_inputs(M, Z, Zp, seed=1000 * Zp + M)
    assert not z16[:, Z:].any()
    out = _run_mlp(W, z16, dl16, M, Zp, Z, priors)
    assert out["dz"].shape == (M, Z)
    _report(f"B mlp M={M} Z={Z} Zp={Zp}", out, W, z16, dl16, 0.25, Z, priors)
    _same(out, _run_mlp(W, z16, dl16, M, Zp, Z, priors, production=True), ("hs", "logit", "delta", "dz"))


@pytest.mark.parametrize("M,Zp", LO.MLP_FWD_ONLY, ids=[f"M{m}-Zp{z}" for m, z in LO.MLP_FWD_ONLY])
def test_mlp_forward_takes_wider_latents(M, Zp):
    """fmri_mlp_fwd accepts Zp up to 512 (include/fmri_hip.h): per element at 320 and 512."""
    W = _weights(Zp)
    z16, dl16, priors = LO.mlp_inputs(M, Zp, Zp, seed=1000 * Zp + M)
    a = _run_mlp(W, z16, dl16, M, Zp, Zp, priors, backward=False)
    _report(f"B mlp forward only M={M} Zp={Zp}", a, W, z16, dl16, 1.0, Zp, priors)
    _same(a, _run_mlp(W, z16, dl16, M, Zp, Zp, priors, backward=False, production=True), ("hs", "logit"))


def test_mlp_width_contract():
    """What the launches refuse (FMRI_E_UNSUPPORTED, nothing launched, outputs untouched): the backward at Zp = 320, and
    on either entry point a Zp that is no multiple of 64 or H != 512."""
    from fmri_hip import lib
    P, L = lib.ptr, lib.load()
    M = 33
    W320, W = _weights(320), _weights(128)
    hs, delta = [_sent16(M, 512) for _ in range(4)], [_sent16(M, 512) for _ in range(4)]
    logit, dz = _sent32(M), _sent32(M, 320)
    z = torch.zeros(M, 320, dtype=torch.float16, device=DEV)
    dl = torch.zeros(M, 8, dtype=torch.float16, device=DEV)

    def fwd(w, Zp, H):
        return L.fmri_mlp_fwd(P(z), M, Zp, H, _ptrs(w["wf"]), (ctypes.c_int * 5)(*w["kp"]), _ptrs(w["b"]), _ptrs(hs),
                              P(logit), lib.stream())

    def bwd(w, Zp, Z, H):
        return L.fmri_mlp_bwd(P(dl), 8, M, Zp, Z, H, _ptrs(hs), P(w["wf"][4]), _ptrs(w["wd"]), (ctypes.c_int * 4)(*w["kpd"]),
                              _ptrs(delta), None, P(dz), 1.0, lib.stream())
    assert bwd(W320, 320, 320, 512) == E_UNSUPPORTED
    assert fwd(W, 100, 512) == E_UNSUPPORTED and bwd(W, 100, 100, 512) == E_UNSUPPORTED
    assert fwd(W, 96, 512) == E_UNSUPPORTED and bwd(W, 32, 32, 512) == E_UNSUPPORTED
    assert fwd(W, 128, 256) == E_UNSUPPORTED and bwd(W, 128, 128, 256) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(_is_sent(t) for t in hs + delta + [logit, dz]), "a refused call wrote something"


# =====================================================================================================================
# C. the network path
# =====================================================================================================================
def test_latent_discriminator_net_gradients(reduction_mode):
    """WaeDiscriminatorNet.forward / .backward at M = 512, train, need_dz: every weight gradient per element against the
    float64 product of the kernel's own delta and hs (the dense weight-gradient bound of tests/test_fullbatch_ops_gpu.py:
    3e-3 of RMS + 3e-3 of the value; same kernel, same row count), the bias gradients under the bound of section B --
    from the fused kernel's atomics in default mode, from bias_grad's fixed-order column sums in deterministic mode,
    where two runs must be bit-identical.  delta is a plain store the network does not return: it is read from a direct
    fmri_mlp_bwd launch on the network's own hs (bit-reproducible, section B)."""
    from fmri_hip import lib
    P = lib.ptr
    M, Z, scale = 512, 128, 4.0
    W = _weights(Z)
    net = W["net"]
    z16, dl16, priors = LO.mlp_inputs(M, Z, Z, seed=99)
    case = f"C net M={M} {'det' if reduction_mode else 'default'}"
    zd = _dev(z16)
    dlog = torch.zeros(M, 8, dtype=torch.float16, device=DEV)
    dlog[:, 0] = _dev(dl16)
    runs = []
    for rep in range(2):
        net.group.zero_grad()
        logit, ctx = net.forward(zd)
        assert ctx.get("fused")
        dz = net.backward(ctx, dlog, scale, True, True)
        torch.cuda.synchronize()
        runs.append(({k: v.clone() for k, v in net.group.grads.items()}, dz.clone(), logit.clone()))
    grads, dz, logit = runs[0]
    hs = ctx["hs"]
    delta = [torch.empty(M, 512, dtype=torch.float16, device=DEV) for _ in range(4)]
    dz2 = torch.empty(M, Z, device=DEV)
    lib.call("fmri_mlp_bwd", P(dlog), 8, M, Z, Z, 512, _ptrs(hs[1:5]), P(W["wf"][4]), _ptrs(W["wd"]),
             (ctypes.c_int * 4)(*W["kpd"]), _ptrs(delta), None, P(dz2), 1.0 / scale)
    torch.cuda.synchronize()
    assert torch.equal(dz, dz2), "dz of the network differs from a direct launch"
    out = dict(hs=[_np(h) for h in hs[1:5]], logit=_np(logit).reshape(-1), delta=[_np(d) for d in delta], dz=_np(dz),
               dbias=[_np(grads[f"main.{i}.bias"]) for i in (0, 2, 4, 6, 8)])
    zero = [np.zeros_like(p) for p in priors]
    _report(case, out, W, z16, dl16, 1.0 / scale, Z, zero)
    xs = [z16] + out["hs"]
    ds = out["delta"] + [dl16.reshape(M, 1)]
    for j, idx in enumerate((0, 2, 4, 6, 8)):
        ref = LO.f64(ds[j]).T @ LO.f64(xs[j])
        _say(case, f"main.{idx}.weight grad", LO.close_ratio(_np(grads[f"main.{idx}.weight"]) * scale, ref, 3e-3))
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2]), "dz / logit differ between runs"
    if reduction_mode:
        for k in runs[0][0]:
            assert torch.equal(runs[0][0][k], runs[1][0][k]), f"deterministic mode: {k} differs between two runs"
