"""GPU checks of the MMD latent penalty: csrc/mmd.hip (fmri_mmd_imq) against the fp64 statistic and gradient, its
determinism and HIP-graph capture, fmri_hip.mmd.imq_mmd as an autograd function, and WaeStep(penalty="mmd") for Stages
I / II / III against the composed oracle step of tests/mmd_oracle.py (the reference has no MMD, SURVEY 0.4: the parity
here is with the formula and with the reference-pinned oracle pieces).  Step tolerances are those tests/test_wae_gpu.py
applies to the GAN step."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import gradcheck
import mmd_oracle as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WAE_KEYS = ("loss_reconstruction", "loss_penalty", "loss_discriminator_fake", "loss_discriminator_real")


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-12)


def _terr(got, ref):
    got, ref = got.detach().float().cpu().reshape(-1), ref.detach().float().cpu().reshape(-1)
    return ((got - ref).norm() / (ref.norm() + 1e-20)).item()


def _mmd64(q, p, sigma2=0.25, scales=M.SCALES):
    """fp64 MMD_u and dMMD_u/dq through exact pairwise distances (Gram form in fp64: r = |a|^2 + |b|^2 - 2 a.b has an
    error ~1e-16 |a|^2 there, far below the fp32 kernel's); the diagonal is excluded by index."""
    q = q.detach().double().requires_grad_(True)
    p = p.detach().double()
    n, d = q.shape
    cs = [2.0 * d * sigma2 * s for s in scales]
    off = ~torch.eye(n, dtype=torch.bool, device=q.device)

    def r2(a, b):
        return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.t()).clamp_min(0.0)

    def k(r):
        return sum(c / (c + r) for c in cs)
    v = (k(r2(p, p))[off].sum() + k(r2(q, q))[off].sum()) / (n * (n - 1)) - 2.0 / (n * n) * k(r2(q, p)).sum()
    (g,) = torch.autograd.grad(v, q)
    return v.item(), g


def _data(n, d, seed, pad):
    g = torch.Generator().manual_seed(seed)
    qw = torch.randn(n, d + pad, generator=g) * 0.6 + 0.1       # encoder-like means, off-centre
    pw = torch.randn(n, d + pad, generator=g) * 0.5             # 0.5 * N(0, I): the Stage-I prior
    return qw.to(DEV)[:, :d], pw.to(DEV)[:, :d]                 # leading dimension d + pad


def _kernel(q, p, dq_pad=0):
    from fmri_hip.mmd import mmd_imq
    n, d = q.shape
    total = torch.zeros(1, dtype=torch.float32, device=DEV)
    dqw = torch.full((n, d + dq_pad), float("nan"), dtype=torch.float32, device=DEV)
    dq = dqw[:, :d]
    mmd_imq(q, p, 0.25, total=total, dq=dq)
    return total, dq, dqw


def test_fp64_reference_matches_the_oracle_definition():
    q, p = _data(9, 128, 0, 0)
    v, g = _mmd64(q, p)
    v0, g0 = M.mmd_u_grad(q.cpu(), p.cpu())
    assert abs(v - v0.item()) < 1e-12 and (g.cpu() - g0).abs().max().item() < 1e-12


@pytest.mark.parametrize("d", [128, 512, 1024])
@pytest.mark.parametrize("n", [2, 3, 17, 64, 256, 1000])
def test_kernel_matches_fp64(n, d):
    q, p = _data(n, d, n * 7 + d, 4 if n % 2 else 12)
    total, dq, dqw = _kernel(q, p, dq_pad=8)
    torch.cuda.synchronize()
    v, g = _mmd64(q, p)
    got = total.item()
    rms = ((dq.double() - g).norm() / g.norm()).item()
    print(f"n {n} d {d}: MMD {got:.8e} ref {v:.8e} |err| {abs(got - v):.2e}  dq rel RMS {rms:.2e}")
    assert abs(got - v) < 1e-5, (got, v)
    assert rms < 1e-4, rms
    assert torch.isnan(dqw[:, d:]).all()                     # nothing written past d in a padded output row


def test_kernel_two_calls_bit_identical_and_graph_replay_equals_eager():
    n, d = 256, 128
    q, p = _data(n, d, 5, 4)
    t1, dq1, _ = _kernel(q, p)
    t2, dq2, _ = _kernel(q, p)
    torch.cuda.synchronize()
    assert torch.equal(t1, t2) and torch.equal(dq1, dq2)
    from fmri_hip.mmd import mmd_imq
    total = torch.zeros(1, dtype=torch.float32, device=DEV)
    dq = torch.empty(n, d, dtype=torch.float32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mmd_imq(q, p, 0.25, total=total, dq=dq)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        total.zero_()
        mmd_imq(q, p, 0.25, total=total, dq=dq)
    dq.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(total, t1) and torch.equal(dq, dq1)


def test_kernel_weight_gscale_value_only_and_accumulation():
    from fmri_hip.mmd import mmd_imq
    n, d = 40, 512
    q, p = _data(n, d, 9, 0)
    t1, dq1, _ = _kernel(q, p)
    total = torch.full((1,), 2.0, dtype=torch.float32, device=DEV)
    dq = torch.empty(n, d, dtype=torch.float32, device=DEV)
    mmd_imq(q, p, 0.25, w=3.0, total=total, dq=dq, gscale=0.5)
    t0 = torch.full((1,), 2.0, dtype=torch.float32, device=DEV)
    mmd_imq(q, p, 0.25, w=3.0, total=t0)                       # value only
    torch.cuda.synchronize()
    assert abs(total.item() - (2.0 + 3.0 * t1.item())) < 1e-6 and torch.equal(total, t0)
    assert ((dq - 1.5 * dq1).norm() / dq1.norm()).item() < 1e-6


def test_imq_mmd_autograd_function():
    from fmri_hip.mmd import imq_mmd
    n, d = 33, 128
    q, p = _data(n, d, 3, 0)
    qq = q.clone().requires_grad_(True)
    pp = p.clone().requires_grad_(True)
    v = imq_mmd(qq, pp)
    (3.0 * v).backward()
    ref_v, ref_g = _mmd64(q, p)
    assert v.dim() == 0 and abs(v.item() - ref_v) < 1e-5
    assert ((qq.grad.double() - 3.0 * ref_g).norm() / (3.0 * ref_g).norm()).item() < 1e-4
    assert pp.grad is None
    with pytest.raises(ValueError):
        imq_mmd(q[:1], p[:1])


# ---- WaeStep(penalty="mmd") against the composed oracle step ---------------------------------------------------------
def _wae_state(O, cfg, stage, V, seed):
    if stage == 1:
        return O.fill_state(O.encoder_spec(cfg) + O.decoder_spec(cfg) + O.wae_discriminator_spec(cfg), seed, False)
    teacher = O.fill_state(O.encoder_spec(cfg) + O.decoder_spec(cfg) + O.wae_discriminator_spec(cfg), seed, True)
    P = dict(O.fill_state(O.cognitive_encoder_spec(cfg, V), seed + 100, True))
    P.update({k: v for k, v in teacher.items() if k.startswith("decoder.")})
    P.update(O.fill_state(O.wae_discriminator_spec(cfg), seed + 200, True))
    P.update({"teacher_net." + k: v for k, v in teacher.items() if k.startswith("encoder.")})
    return P


def _opts(O, stage):
    lr = 1e-4 if stage == 1 else 1e-3
    return {"encoder": O.OptState(kind="adam", lr=lr), "decoder": O.OptState(kind="adam", lr=lr)}


@pytest.mark.parametrize("B", [4, 32])
@pytest.mark.parametrize("stage", [1, 2, 3])
def test_mmd_wae_step_matches_composed_oracle(stage, B):
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    from fmri_hip.wae_steps import WaeStep
    seed, steps, V = 5, 3, (512 if stage > 1 else 0)
    cfg_o = O.ArchCfg.px64()
    data = O.synth_batch(B, cfg_o, n_voxels=V, seed=1234, steps=steps)
    st = WaeStep(ArchConfig.px64(), DEV, stage, V, penalty="mmd")
    st.load_recipe(seed, False)
    rec = gradcheck.Recorder(st)
    wd0 = {k: v.clone() for k, v in st.state_dict().items() if k.startswith("discriminator.")}
    assert wd0
    P = _wae_state(O, cfg_o, stage, V, seed)
    opts = _opts(O, stage)
    x = data["x"].to(DEV)
    for s in range(steps):
        zf = data["noise"][s, 2]
        fm = data["fmri"] if stage > 1 else None
        rec.clear()
        if stage == 1:
            st.step(x, zf.to(DEV))
        else:
            st.step(x, fmri=fm.to(DEV))
        ref = M.wae_mmd_step(P, opts, stage, cfg_o, data["x"], zf, fm, V, keep_grads=True)
        logs = st.logs()
        for k in WAE_KEYS:
            print(stage, B, s, k, logs[k], ref["logs"][k], _rel(logs[k], ref["logs"][k]))
            if k.startswith("loss_discriminator"):
                assert logs[k] == 0.0, k
            elif s == 0:
                assert _rel(logs[k], ref["logs"][k]) < (1e-3 if k != "loss_penalty" else 5e-3), k
            elif k == "loss_penalty" and stage == 1:
                # Stage I after the first (sign-like) Adam update: the engine's latents sit 5-15 % (relative L2) from the
                # oracle's (fp16 rounding decides the sign of the near-zero gradients of the 16M-weight fc.0), and at
                # B = 4 the unbiased statistic is a near-cancelling difference (24.7 at step 0, -3.4 at step 1) that
                # amplifies this to 7 %.  The penalty is held instead to the fp64 statistic of the engine's OWN latents
                # and prior sample (1e-3); the trajectory is held by the reconstruction loss (5e-2).
                z_eng = st.outputs()["z_real"].cpu()
                own = 10.0 * B * M.mmd_u(z_eng, 0.5 * zf).item()
                print(stage, B, s, "penalty of the engine's own latents", own, "z_real err",
                      _terr(z_eng, ref["fw"]["z_real"]))
                assert _rel(logs[k], own) < 1e-3, (s, k, logs[k], own)
            else:
                assert _rel(logs[k], ref["logs"][k]) < 5e-2, (s, k)
        if s == 0:
            outs = st.outputs()
            for k in ("x_recon", "z_real"):
                e = _terr(outs[k], ref["fw"][k])
                print(stage, B, "fw", k, e)
                assert e < 1e-2, (k, e)
            grads = st.named_grads()
            assert not any(k.startswith("discriminator.") for k in grads)
            P16 = _wae_state(O, cfg_o, stage, V, seed)
            with gradcheck.pinned(O, gradcheck.wae_masks(rec, B, stage, penalty="mmd")):
                ref16 = M.wae_mmd_step(P16, _opts(O, stage), stage, cfg_o, data["x"], zf, fm, V, keep_grads=True)
            # l_mu.bias: the batch sum of d/dmu, where the reconstruction part cancels through the decoder's first BN
            # (see tests/test_wae_gpu.py) -- reported, not bounded, as for the GAN step
            special = [k for k in ref["grads"] if k.endswith("l_mu.bias")]
            for k in special:
                print(stage, B, "grad", k, _terr(grads[k], ref["grads"][k]))
            gradcheck.check(grads, ref["grads"], ref16["grads"], f"wae{stage}-mmd-b{B}", skip=special)
        # the latent discriminator is neither run nor updated
        sd = st.state_dict()
        for k, v in wd0.items():
            assert torch.equal(sd[k], v), k


def test_mmd_stage1_150_steps_stay_finite():
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    from fmri_hip.wae_steps import WaeStep
    B = 64
    cfg_o = O.ArchCfg.px64()
    data = O.synth_batch(B, cfg_o, seed=77, steps=150)
    st = WaeStep(ArchConfig.px64(), DEV, 1, penalty="mmd")
    st.load_recipe(2, True)
    x, noise = data["x"].to(DEV), data["noise"][:, 2].to(DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    for s in range(150):
        scal = st.step(x, noise[s])
        bad += (~torch.isfinite(scal[:4])).any().int()
    torch.cuda.synchronize()
    logs = st.logs()
    print("after 150 steps", logs)
    assert bad.item() == 0
    assert all(np.isfinite(v) for v in logs.values())
    assert all(bool(torch.isfinite(v).all()) for v in st.state_dict().values() if v.is_floating_point())


# ---- self-checks ------------------------------------------------------------------------------------------------------
@pytest.mark.selfcheck
@pytest.mark.parametrize("stage", [1, 2])
def test_mmd_wae_step_recorded_into_a_hip_graph_equals_eager_steps(deterministic, stage):
    from fmri_hip.params import ArchConfig
    from fmri_hip.wae_steps import WaeStep
    cfg, V, B = ArchConfig.px64(), 512, 8
    rs = np.random.RandomState(11)
    x = torch.tanh(torch.from_numpy(rs.standard_normal((B, 3, 64, 64)).astype(np.float32))).to(DEV)
    zf = torch.from_numpy(rs.standard_normal((B, cfg.latent_dim)).astype(np.float32)).to(DEV)
    fm = torch.from_numpy(rs.standard_normal((B, V)).astype(np.float32)).to(DEV)
    args = (x, zf) if stage == 1 else (x, None, fm)

    def make():
        st = WaeStep(cfg, DEV, stage, V if stage > 1 else 0, penalty="mmd")
        st.load_recipe(5, False if stage == 1 else None)
        return st
    a, b = make(), make()
    s0 = {k: v.clone() for k, v in a.state_dict().items()}
    for _ in range(5):
        a.step(*args)
    run = b.capture(*args)            # two eager warm-up steps inside; records a one-stream step
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    assert a.logs() == b.logs()
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    moved = [k for k in sa if sa[k].dtype.is_floating_point and sa[k].numel() >= 1024 and "running" not in k
             and not torch.equal(sa[k], s0[k])]
    assert moved and not any(k.startswith("discriminator.") for k in moved)


def _worker_mmd(rank, world, port, stage, q):
    import traceback
    try:
        import test_distributed as TD
        TD._init(rank, world, port)
        import torch.distributed as dist
        from oracle import vaegan_oracle as O
        torch.cuda.set_device(0)
        B = 4
        data = O.synth_batch(2 * B, O.ArchCfg.px64(), n_voxels=512, seed=1234, steps=1)
        st = _mmd_step(stage, True)
        logs, sdn = _run_mmd(stage, st, data, slice(rank * B, (rank + 1) * B))
        q.put((rank, logs, sdn))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:
        q.put(("error", traceback.format_exc()))
        raise


def _mmd_step(stage, dist_on):
    from fmri_hip.params import ArchConfig
    from fmri_hip.wae_steps import WaeStep
    st = WaeStep(ArchConfig.px64(), "cuda:0", stage, 512 if stage > 1 else 0, distributed=dist_on, sync_bn=True,
                 penalty="mmd")
    st.load_recipe(5, False)
    return st


def _run_mmd(stage, st, data, sl):
    x, nz = data["x"][sl].cuda(), data["noise"][0][:, sl].cuda()
    if stage == 1:
        st.step(x, nz[2])
    else:
        st.step(x, fmri=data["fmri"][sl].cuda())
    torch.cuda.synchronize()
    return st.logs(), {k: float(v.float().norm()) for k, v in st.state_dict().items()}


@pytest.mark.selfcheck
@pytest.mark.parametrize("stage", [1, 2, 3])
def test_mmd_two_rank_equals_single_process_global_batch(stage):
    """distributed=True on two half batches (q and p gathered by one SUM all-reduce, the global statistic on both ranks,
    each rank's own gradient rows) against one process on the full batch, in the pattern of
    tests/test_distributed.py::test_two_rank_other_steps_equal_single_process_global_batch."""
    import test_distributed as TD
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = TD._free_port()
    procs = [ctx.Process(target=_worker_mmd, args=(r, 2, port, stage, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(TD._collect(procs, q, 2), key=lambda t: t[0])
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    from oracle import vaegan_oracle as O
    data = O.synth_batch(8, O.ArchCfg.px64(), n_voxels=512, seed=1234, steps=1)
    logs1, sd1 = _run_mmd(stage, _mmd_step(stage, False), data, slice(0, 8))
    assert logs1["loss_penalty"] != 0.0
    for rank, logs, sdn in res:
        for k, v in logs1.items():
            assert abs(logs[k] - v) < 5e-4 * abs(v) + 1e-6, (stage, rank, k, logs[k], v)
        for k, v in sd1.items():
            slack = 1e-3 if v < 1.0 else 0.0
            assert abs(sdn[k] - v) < 3e-3 * v + slack + 1e-6, (stage, rank, k, sdn[k], v)
    for k in res[0][2]:
        assert abs(res[0][2][k] - res[1][2][k]) <= 1e-6 * abs(res[0][2][k]) + 1e-9, (stage, k)
