"""Numerics monitor on the device: fmri_tensor_stats against float64 torch, the counting BatchNorm-backward variants
against the uncounted ones and an fp32 reference, the step statistics against ``named_grads()`` / ``state_dict()`` /
``outputs()``, and the monitor-off path unchanged bit for bit."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _stats(segs):
    from fmri_hip import lib, monitor
    ws = torch.empty(lib.load().fmri_tensor_stats_ws_bytes(8), dtype=torch.uint8, device=DEV)
    out = torch.zeros(len(segs) * 32, dtype=torch.uint8, device=DEV)
    monitor.tensor_stats([dict(s, out=out.data_ptr() + 32 * i) for i, s in enumerate(segs)], ws)
    torch.cuda.synchronize()
    return np.frombuffer(out.cpu().numpy().tobytes(), dtype=monitor.STAT_DTYPE)


def test_tensor_stats_against_float64():
    torch.manual_seed(1)
    sizes = [1, 7, 1023, 1025, 4 * 1024 * 1024 + 3]
    xs = [torch.randn(n, device=DEV) * 3 for n in sizes]
    xs[1][2] = float("inf")
    xs[2][5], xs[2][900] = float("nan"), -float("inf")
    xs[3][1024] = 1e30
    xs[4][123456], xs[4][4000000] = float("nan"), -1e30
    strided = torch.randn(33, 40, device=DEV)
    strided[4, 3] = float("nan")                     # inside the segment (cols [0, 17))
    strided[5, 30] = 1e30                            # outside it
    segs = [dict(x=x.data_ptr(), rows=1, cols=x.numel()) for x in xs]
    segs.append(dict(x=strided.data_ptr(), rows=33, cols=17, ld=40))
    divt = torch.tensor([4.0], device=DEV)
    segs.append(dict(x=xs[3].data_ptr(), rows=1, cols=xs[3].numel(), div=divt.data_ptr(), scale=2.0, clamp=0.5))
    got = _stats(segs)
    again = _stats(segs)
    assert got.tobytes() == again.tobytes(), "two runs differ"
    refs = [x for x in xs] + [strided[:, :17]] + [xs[3] * np.float32(2.0 / 4.0)]
    for i, r in enumerate(refs):
        r = r.float().cpu().reshape(-1)
        fin = torch.isfinite(r)
        rf = r[fin].double()
        g = got[i]
        assert g["written"] == 1
        assert int(g["nonfinite"]) == int((~fin).sum()), i
        assert float(g["max"]) == float(r[fin].max()), i
        assert float(g["min"]) == float(r[fin].min()), i
        assert float(g["max_abs"]) == float(r[fin].abs().max()), i
        ss = float((rf * rf).sum())
        assert abs(float(g["sumsq"]) - ss) <= 1e-12 * ss, (i, float(g["sumsq"]), ss)
    clamped = int(((refs[-1].abs() > 0.5) | torch.isnan(refs[-1])).sum())
    assert int(got[-1]["clamped"]) == clamped and clamped > 0
    # a gated-off segment leaves its record alone
    gate = torch.zeros(1, dtype=torch.int32, device=DEV)
    off = _stats([dict(x=xs[0].data_ptr(), rows=1, cols=1, gate=gate.data_ptr())])
    assert off[0]["written"] == 0 and off[0]["sumsq"] == 0.0


def _bn_case():
    """test_latent_range_gpu's saturation construction: a nearly constant feature with a large gamma, plus a NaN."""
    M, C = 64, 64
    torch.manual_seed(9)
    x = torch.randn(M, C)
    x[:, 5] = 1.0 + 1e-4 * torch.randn(M)
    gam = torch.ones(C)
    gam[5] = 50.0
    mean = x.mean(0)
    rstd = 1.0 / torch.sqrt(x.var(0, unbiased=False) + 1e-5)
    dy = (torch.randn(2 * M, C) * 100.0).half()
    dy[3, 9] = float("nan")
    return M, C, x.half(), gam, mean, rstd, dy


def _ref_dx(x16, dy16, mean, rstd, gam, sums, M):
    xh = (x16.float() - mean) * rstd
    g = dy16.float()
    return gam * rstd * (g - sums[0] / M - xh * sums[1] / M)


def test_counted_batchnorm_backward_matches_and_counts():
    from fmri_hip import lib
    L = lib.load()
    M, C, x16, gam, mean, rstd, dy = _bn_case()
    d = lambda t: t.to(DEV).contiguous()
    X, DY, G, MU, RS, BE = d(x16), d(dy), d(gam), d(mean), d(rstd), d(torch.zeros(C))
    P = lib.ptr

    def run(name, args, cnt=None, nout=M):
        out = torch.empty(nout, C, dtype=torch.float16, device=DEV)
        extra = () if cnt is None else (P(cnt),)
        lib.check(getattr(L, name)(*args(out), *extra, lib.stream()), name)
        return out

    results = {}
    for ns in (1, 2):
        sums_a = torch.zeros(2 * ns, C, device=DEV)
        sums_b = torch.zeros(2 * ns, C, device=DEV)
        cnt = torch.zeros(2, dtype=torch.int32, device=DEV)
        a = run("fmri_bn_cols_bwd", lambda o: (P(X), P(DY), P(o), M, C, ns, float(M), P(MU), P(RS), P(G), P(BE), 0,
                                               P(sums_a), None, None, 0.0, 0), nout=ns * M)
        b = run("fmri_bn_cols_bwd_cnt", lambda o: (P(X), P(DY), P(o), M, C, ns, float(M), P(MU), P(RS), P(G), P(BE), 0,
                                                   P(sums_b), None, None, 0.0, 0), cnt=cnt, nout=ns * M)
        results[f"cols{ns}"] = (a, b, cnt, sums_a)
    sums2, sums4 = results["cols1"][3], results["cols2"][3]
    cnt1 = torch.zeros(2, dtype=torch.int32, device=DEV)
    a = run("fmri_bn_bwd_apply", lambda o: (P(X), P(DY), P(o), M, C, float(M), P(MU), P(RS), P(G), P(BE), 0, P(sums2)))
    b = run("fmri_bn_bwd_apply_cnt", lambda o: (P(X), P(DY), P(o), M, C, float(M), P(MU), P(RS), P(G), P(BE), 0,
                                                P(sums2)), cnt=cnt1)
    results["apply"] = (a, b, cnt1, sums2)
    cnt2 = torch.zeros(2, dtype=torch.int32, device=DEV)
    a = run("fmri_bn_bwd_apply2", lambda o: (P(X), P(DY), P(o), M, C, float(M), P(MU), P(RS), P(G), P(BE), 0, P(sums4)),
            nout=2 * M)
    b = run("fmri_bn_bwd_apply2_cnt", lambda o: (P(X), P(DY), P(o), M, C, float(M), P(MU), P(RS), P(G), P(BE), 0,
                                                 P(sums4)), cnt=cnt2, nout=2 * M)
    results["apply2"] = (a, b, cnt2, sums4)
    torch.cuda.synchronize()
    for key, (a, b, cnt, sums) in results.items():
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), key + ": dx differs"
        ns = 2 if key in ("cols2", "apply2") else 1
        s = sums.cpu()
        ref = torch.cat([_ref_dx(x16, dy[st * M:(st + 1) * M], mean, rstd, gam, s[2 * st:2 * st + 2], M)
                         for st in range(ns)])
        fin = ~torch.isnan(ref)
        lo = int((ref[fin].abs() > 65504 * 1.01).sum())
        hi = int((ref[fin].abs() > 65504 * 0.99).sum())
        sat, nan = cnt.cpu().tolist()
        assert lo > 0, key
        assert lo <= sat <= hi, (key, lo, sat, hi)
        assert nan == int(torch.isnan(b.float()).sum().item()) == int((~fin).sum()), (key, nan)


def _stage1(monitor, seed=0, mode="vae-gan", state=None):
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import Stage1Step
    st = Stage1Step(ArchConfig.px64(), DEV, monitor=monitor, mode=mode)
    if state is None:
        st.load_recipe(seed, True)
    else:
        st.load_state_dict({k: (v.reshape(()) if k.endswith("num_batches_tracked") else v.clone())
                            for k, v in state.items()})
    return st


def _data(B=4, seed=1234, steps=3, V=0):
    from oracle import vaegan_oracle as O
    return O.synth_batch(B, O.ArchCfg.px64(), n_voxels=V, seed=seed, steps=steps)


_NETS = {"encoder": "enc", "decoder": "dec", "discriminator": "dis"}


def test_stage1_statistics_against_named_grads():
    from oracle import vaegan_oracle as O
    B = 4
    P = O.fill_state(O.vaegan_spec(O.ArchCfg.px64()), 0, True)
    st = _stage1(True, state=P)
    data = _data(B, steps=1)
    st.forward(data["x"].to(DEV), data["noise"][0, 0].to(DEV), data["noise"][0, 1].to(DEV))
    st.gate(B)
    st.backward()
    ng = st.named_grads()
    st.apply()
    num = st.numerics()
    logs = st.logs()
    flags = dict(encoder=True, decoder=logs["train_dec"], discriminator=logs["train_dis"])
    for net, attr in _NETS.items():
        gr = num["grad"][net]
        assert gr["updated"] == flags[net], net
        if not gr["updated"]:
            assert gr["norm"] is None and num["param"][net]["max_abs"] is None
            continue
        gs = [v.double().reshape(-1) for k, v in ng.items() if k.startswith(net + ".")]
        norm = math.sqrt(sum(float((g * g).sum()) for g in gs))
        mx = max(float(g.abs().max()) for g in gs)
        assert abs(gr["norm"] - norm) <= 1e-6 * norm, (net, gr["norm"], norm)
        assert abs(gr["max_abs"] - mx) <= 1e-6 * mx, (net, gr["max_abs"], mx)
        assert gr["nonfinite"] == 0 and gr["clamped"] == 0
        views = getattr(st, attr).group.views
        pmax = max(float(v.abs().max()) for v in views.values())
        assert num["param"][net]["max_abs"] == pmax, net
        assert num["param"][net]["nonfinite"] == 0
    assert num["losses_finite"] is True
    assert num["latent"]["range_exp"] == [0.0, 0.0, 0.0, 0.0]
    assert set(num["bn_backward"]) >= {"decoder.fc.1"}
    assert all(v == dict(saturated=0, nonfinite=0) for v in num["bn_backward"].values())


def test_stage1_norms_against_the_reference_goldens(golden_dir):
    """tests/golden/stage1_b4.npz, step 0: the reference's per-key gradient norms (step0/grad_sum[:, 0]; NaN = not
    computed) against the monitor's per-network norm."""
    import os
    from oracle import vaegan_oracle as O
    g = np.load(os.path.join(golden_dir, "stage1_b4.npz"))
    B, seed, perturb, steps = int(g["meta/B"]), int(g["meta/seed"]), bool(g["meta/perturb"]), int(g["meta/steps"])
    keys = [str(k) for k in g["step0/grad_keys"]]
    gsum = np.asarray(g["step0/grad_sum"], dtype=np.float64)
    P = O.fill_state(O.vaegan_spec(O.ArchCfg.px64()), seed, perturb)
    st = _stage1(True, state=P)
    data = O.synth_batch(B, O.ArchCfg.px64(), seed=1234, steps=steps)
    st.step(data["x"].to(DEV), data["noise"][0, 0].to(DEV), data["noise"][0, 1].to(DEV))
    num = st.numerics()
    checked = 0
    for net in _NETS:
        col = np.array([gsum[i, 0] for i, k in enumerate(keys) if k.startswith(net + ".")])
        if not num["grad"][net]["updated"] or col.size == 0 or np.isnan(col).any():
            continue
        ref = math.sqrt(float((col ** 2).sum()))
        assert abs(num["grad"][net]["norm"] - ref) <= 2e-2 * ref, (net, num["grad"][net]["norm"], ref)
        checked += 1
    assert checked >= 1


def _run_steps(st, kind, data, mode, steps=3):
    x = data["x"].to(DEV)
    nz = [data["noise"][s] for s in range(steps)]
    if kind == "stage1":
        args = (x, nz[0][0].to(DEV), nz[0][1].to(DEV))
    elif kind == "dual":
        args = (x, nz[0][0].to(DEV), nz[0][1].to(DEV), nz[0][2].to(DEV))
    elif kind == "cog":
        args = (data["fmri"].to(DEV), x, nz[0][0].to(DEV), nz[0][1].to(DEV), nz[0][2].to(DEV))
    else:
        args = (x, nz[0][2].to(DEV))
    if mode == "eager":
        for _ in range(steps):
            st.step(*args)
    elif mode == "capture":
        run = st.capture(*args, warmup=steps - 1)
        run()
    else:
        run = st.capture_forward(*args, warmup=steps - 1)
        run()
    torch.cuda.synchronize()


def _make(kind, monitor, V=16):
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import CognitiveStep
    from fmri_hip.wae_steps import DualStage1Step, WaeStep
    cfg = ArchConfig.px64()
    if kind == "stage1":
        st = _stage1(monitor)
    elif kind == "dual":
        st = DualStage1Step(cfg, DEV, monitor=monitor)
        st.load_recipe(0, True)
    elif kind == "cog":
        st = CognitiveStep(cfg, V, DEV, 2, monitor=monitor)
        st.load_recipe(0, True)
    else:
        st = WaeStep(cfg, DEV, 1, monitor=monitor)
        st.load_recipe(0, False)
    return st


CASES = [("stage1", "eager"), ("stage1", "capture"), ("stage1", "capture_forward"), ("cog", "eager"),
         ("cog", "capture"), ("wae", "eager"), ("dual", "eager")]


@pytest.mark.parametrize("kind,mode", CASES)
def test_monitor_off_is_unchanged(kind, mode, deterministic):
    data = _data(4, steps=3, V=16)
    out = []
    for on in (False, True):
        st = _make(kind, on)
        _run_steps(st, kind, data, mode)
        out.append((st.state_dict(), st.logs()))
        if on:
            num = st.numerics()
            assert num["losses_finite"] is True
            assert any(v["updated"] for v in num["grad"].values())
    (sd0, lg0), (sd1, lg1) = out
    assert lg0 == lg1
    assert sd0.keys() == sd1.keys()
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k


def test_same_numbers_on_every_launch_mode(deterministic, monkeypatch):
    from fmri_hip import ops
    data = _data(4, steps=3)
    nums = {}
    for mode in ("eager", "capture", "capture_forward"):
        st = _make("stage1", True)
        _run_steps(st, "stage1", data, mode)
        nums[mode] = st.numerics()
    assert nums["eager"] == nums["capture"] == nums["capture_forward"]
    monkeypatch.setattr(ops, "_FUSED_APPLY", False)
    st = _make("stage1", True)
    _run_steps(st, "stage1", data, "eager")
    nf, ref = st.numerics(), nums["eager"]
    for net in _NETS:
        a, b = nf["grad"][net], ref["grad"][net]
        assert a["updated"] == b["updated"], net
        if not a["updated"]:
            continue
        for f in ("max_abs", "nonfinite", "clamped"):
            assert a[f] == b[f], (net, f, a[f], b[f])
        assert abs(a["norm"] - b["norm"]) <= 1e-9 * b["norm"], (net, a["norm"], b["norm"])
        assert nf["param"][net] == ref["param"][net], net
    assert nf["latent"] == ref["latent"] and nf["bn_backward"] == ref["bn_backward"]


def test_latent_excursion_is_reported():
    from oracle import vaegan_oracle as O
    B = 8
    data = O.synth_batch(B, O.ArchCfg.px64(), seed=77, steps=1)
    P = O.fill_state(O.vaegan_spec(O.ArchCfg.px64()), 5, True)
    healthy = _stage1(True, state=P)
    P["encoder.l_var.bias"] = P["encoder.l_var.bias"] + 24.0
    st = _stage1(True, state=P)
    args = (data["x"].to(DEV), data["noise"][0, 0].to(DEV), data["noise"][0, 1].to(DEV))
    st.step(*args)
    num = st.numerics()
    lv = st.outputs()["log_variances"]
    assert num["latent"]["logvar_max"] > 23
    assert num["latent"]["logvar_max"] == float(lv.max())
    assert num["latent"]["logvar_min"] == float(lv.min())
    z0 = float(st.zs[0])
    assert num["latent"]["range_exp"][0] == -math.log2(z0) > 0
    healthy.step(*args)
    hn = healthy.numerics()
    assert hn["latent"]["range_exp"] == [0.0, 0.0, 0.0, 0.0]
    assert all(v == dict(saturated=0, nonfinite=0) for v in hn["bn_backward"].values())


def test_clamp_count_of_stage2():
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import CognitiveStep
    B, V = 4, 16
    data = _data(B, steps=1, V=V)
    st = CognitiveStep(ArchConfig.px64(), V, DEV, 2, monitor=True)
    st.load_recipe(0, True)
    nz = data["noise"][0]
    st.forward(data["fmri"].to(DEV), data["x"].to(DEV), nz[0].to(DEV), nz[1].to(DEV), nz[2].to(DEV))
    st.gate(B)
    st.backward()
    ng = st.named_grads()
    st.apply()
    num = st.numerics()
    assert num["grad"]["decoder"]["updated"] is False              # Stage II: the decoder is frozen
    for net in ("encoder", "discriminator"):
        if not num["grad"][net]["updated"]:
            continue
        g = torch.cat([v.double().reshape(-1) for k, v in ng.items() if k.startswith(net + ".")]).abs()
        lo, hi = int((g > 1 + 1e-6).sum()), int((g > 1 - 1e-6).sum())
        assert lo <= num["grad"][net]["clamped"] <= hi, (net, lo, num["grad"][net]["clamped"], hi)
