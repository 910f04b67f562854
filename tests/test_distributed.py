"""Data-parallel path (one process per GPU, SUM all-reduce + SyncBN), world size 2.

CPU / gloo:
  * the engine's distributed glue (`fmri_hip.steps._Dist`) reduces with SUM and reports the world size;
  * the SyncBN scheme the HIP BatchNorm uses (all-reduce [sum x | sum x^2] forward and
    [sum g | sum g*xhat] backward, parameter gradients from LOCAL sums, then one SUM all-reduce of the
    flat gradient buffer) is numerically identical to a single process on the global batch, for losses
    that are batch SUMS (train_vgan_stage1.py:369-372).
GPU (2 ranks sharing the one GPU of the test box, gloo backend on device tensors):
  * the real fused Stage-I step with distributed=True on two half batches reproduces the single-process
    step on the full batch.
"""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _collect(procs, q, n, timeout=240.0):
    """n results from the worker queue; fails (instead of blocking forever) when a worker died or nothing arrives."""
    import time
    out, t0 = [], time.time()
    while len(out) < n:
        if not q.empty():
            item = q.get()
            if isinstance(item, tuple) and len(item) == 2 and item[0] == "error":
                for p in procs:
                    p.kill()
                raise AssertionError("worker failed:\n" + item[1])
            out.append(item)
            continue
        if time.time() - t0 > timeout or all(not p.is_alive() for p in procs):
            if not q.empty():
                continue
            for p in procs:
                p.kill()
            raise AssertionError(f"workers delivered {len(out)}/{n} results (exit codes {[p.exitcode for p in procs]})")
        time.sleep(0.05)
    return out


def _guarded(fn):
    """Worker wrapper: an exception is reported through the queue (the peer would otherwise wait in a collective)."""
    import functools
    import traceback

    @functools.wraps(fn)
    def wrapper(*args):
        try:
            fn(*args)
        except BaseException:
            args[-1].put(("error", traceback.format_exc()))
            raise
    return wrapper


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    for p in (ROOT, os.path.join(ROOT, "thesis-fmri-reconstruction_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)


class _SyncBNRelu(torch.autograd.Function):
    """Python restatement of the engine's SyncBN (fmri_hip.ops.BatchNorm with a reducer + csrc/norm.hip)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, reducer):
        M, C = x.shape
        sums = torch.stack([x.sum(0), (x * x).sum(0)])
        count = float(M) * reducer(sums)
        mean = sums[0] / count
        var = (sums[1] / count - mean * mean).clamp_min(0)
        rstd = torch.rsqrt(var + 1e-5)
        xh = (x - mean) * rstd
        pre = xh * gamma + beta
        ctx.save_for_backward(xh, pre, gamma, rstd)
        ctx.count, ctx.reducer = count, reducer
        return pre.clamp_min(0)

    @staticmethod
    def backward(ctx, dy):
        xh, pre, gamma, rstd = ctx.saved_tensors
        g = dy * (pre > 0)
        sums = torch.stack([g.sum(0), (g * xh).sum(0)])
        dgamma, dbeta = sums[1].clone(), sums[0].clone()       # LOCAL sums -> param grads
        ctx.reducer(sums)                                      # global sums -> dx
        dx = gamma * rstd * (g - sums[0] / ctx.count - xh * sums[1] / ctx.count)
        return dx, dgamma, dbeta, None


def _toy_loss(x, w1, gamma, beta, w2, reducer):
    h = _SyncBNRelu.apply(F.linear(x, w1), gamma, beta, reducer)
    return (F.linear(h, w2) ** 2).sum()            # a batch SUM, like every reference loss


@_guarded
def _worker_cpu(rank, world, port, q):
    _init(rank, world, port)
    from fmri_hip.steps import _Dist
    d = _Dist(True, True)
    assert d.on and d.world == world
    t = torch.full((3,), float(rank + 1))
    d.all_reduce(t)
    assert torch.equal(t, torch.full((3,), 3.0))
    red = d.bn_reducer()
    s = torch.tensor([[1.0, 2.0], [3.0, 4.0]]) * (rank + 1)
    assert red(s) == world and torch.equal(s, torch.tensor([[3.0, 6.0], [9.0, 12.0]]))
    # SyncBN + SUM-of-gradients == single process on the global batch
    g = torch.Generator().manual_seed(0)
    X = torch.randn(8, 6, generator=g, dtype=torch.float64)
    W1 = torch.randn(5, 6, generator=g, dtype=torch.float64)
    GA, BE = torch.rand(5, generator=g, dtype=torch.float64) + 0.5, torch.randn(5, generator=g, dtype=torch.float64)
    W2 = torch.randn(3, 5, generator=g, dtype=torch.float64)
    ps = [p.clone().requires_grad_(True) for p in (W1, GA, BE, W2)]
    loss = _toy_loss(X[rank * 4:(rank + 1) * 4], ps[0], ps[1], ps[2], ps[3], red)
    loss.backward()
    flat = torch.cat([p.grad.reshape(-1) for p in ps])
    lsum = loss.detach().clone().reshape(1)
    d.all_reduce(flat)
    d.all_reduce(lsum)
    pr = [p.clone().requires_grad_(True) for p in (W1, GA, BE, W2)]
    ref = _toy_loss(X, pr[0], pr[1], pr[2], pr[3], lambda s_: 1)
    ref.backward()
    flat_ref = torch.cat([p.grad.reshape(-1) for p in pr])
    ok = torch.allclose(flat, flat_ref, rtol=1e-10, atol=1e-12) and torch.allclose(lsum, ref.detach().reshape(1))
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_syncbn_sum_allreduce_equals_global_batch_cpu_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_cpu, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    res = sorted(_collect(procs, q, 2))
    assert res == [(0, True), (1, True)]


@_guarded
def _worker_gpu(rank, world, port, q):
    _init(rank, world, port)
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import Stage1Step
    torch.cuda.set_device(0)
    B = 4
    cfg = O.ArchCfg.px64()
    data = O.synth_batch(2 * B, cfg, seed=1234, steps=1)
    sl = slice(rank * B, (rank + 1) * B)
    st = Stage1Step(ArchConfig.px64(), "cuda:0", distributed=True, sync_bn=True)
    st.load_recipe(0, True)
    st.forward(data["x"][sl].cuda(), data["noise"][0, 0][sl].cuda(), data["noise"][0, 1][sl].cuda())
    st.gate(2 * B)
    st.backward()
    grads = {k: v.cpu() for k, v in st.named_grads().items()}
    st.apply()
    torch.cuda.synchronize()
    q.put((rank, st.logs(), {k: float(v.norm()) for k, v in grads.items()},
           {k: float(v.float().norm()) for k, v in st.state_dict().items()}))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.selfcheck
def test_two_rank_stage1_step_equals_single_process_global_batch():
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_gpu, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(_collect(procs, q, 2), key=lambda t: t[0])
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    # single process, global batch 8
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import Stage1Step
    B = 8
    cfg = O.ArchCfg.px64()
    data = O.synth_batch(B, cfg, seed=1234, steps=1)
    st = Stage1Step(ArchConfig.px64(), "cuda:0")
    st.load_recipe(0, True)
    st.forward(data["x"].cuda(), data["noise"][0, 0].cuda(), data["noise"][0, 1].cuda())
    st.gate(B)
    st.backward()
    g1 = {k: float(v.norm()) for k, v in st.named_grads().items()}
    st.apply()
    logs1 = st.logs()
    sd1 = {k: float(v.float().norm()) for k, v in st.state_dict().items()}
    for rank, logs, gn, sdn in res:
        for k in ("loss_encoder", "loss_decoder", "loss_discriminator", "kl", "mse", "nle"):
            assert abs(logs[k] - logs1[k]) < 2e-4 * abs(logs1[k]), (rank, k, logs[k], logs1[k])
        assert logs["train_dis"] == logs1["train_dis"] and logs["train_dec"] == logs1["train_dec"]
        for k, v in g1.items():
            # the 3-element bias gradient of the decoder's last conv is a heavily cancelling sum over 2B*64*64 fp16
            # cotangents: its norm moves by several % with the summation split (per-rank batch) alone
            tol = 0.15 if k == "decoder.conv.3.0.bias" else 0.05
            assert abs(gn[k] - v) < tol * v + 1e-6, (rank, k, gn[k], v)
        for k, v in sd1.items():
            # same 3-element bias: RMSprop's first update is +-3.16e-4 per element whatever the gradient's size, so
            # one sign flip of a near-zero gradient element moves the norm by that much
            slack = 7e-4 if k == "decoder.conv.3.0.bias" else 1e-6
            assert abs(sdn[k] - v) < 2e-3 * v + slack, (rank, k, sdn[k], v)
    # both ranks hold identical parameters after the step
    for k in res[0][3]:
        assert abs(res[0][3][k] - res[1][3][k]) <= 1e-6 * abs(res[0][3][k]) + 1e-9, k


@_guarded
def _worker_hybrid(rank, world, port, q):
    """Per-rank BN statistics (bench.py's default): the recorded-forward hybrid step against the eager step, both
    data parallel over 2 ranks (gloo over device tensors)."""
    _init(rank, world, port)
    from oracle import vaegan_oracle as O
    from fmri_hip import ops
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import Stage1Step
    torch.cuda.set_device(0)
    B = 4
    data = O.synth_batch(2 * B, O.ArchCfg.px64(), seed=1234, steps=1)
    sl = slice(rank * B, (rank + 1) * B)
    x, e, zp = data["x"][sl].cuda(), data["noise"][0, 0][sl].cuda(), data["noise"][0, 1][sl].cuda()
    a = Stage1Step(ArchConfig.px64(), "cuda:0", distributed=True, sync_bn=False)
    a.load_recipe(0, True)
    run = a.capture_forward(x, e, zp, warmup=1)
    b = Stage1Step(ArchConfig.px64(), "cuda:0", distributed=True, sync_bn=False)
    b.load_state_dict(a.state_dict())
    for oa, ob in ((a.opt_enc, b.opt_enc), (a.opt_dec, b.opt_dec), (a.opt_dis, b.opt_dis)):
        ob.s1.copy_(oa.s1)
    run()
    ops.join_side()
    fused, real = [0], ops.apply_group

    def counting(*aa, **kw):
        r = real(*aa, **kw)
        fused[0] += 1 if r else 0
        return r
    ops.apply_group = counting
    b.step(x, e, zp)
    ops.apply_group = real
    ops.join_side()
    torch.cuda.synchronize()
    # the data-parallel step takes the one-launch update for all three sub-networks (mode 0 in front of each all-reduce,
    # mode 3 behind it -- the encoder's gradients are materialised in two parts)
    assert fused[0] == 3, f"fmri_apply_batch updated {fused[0]} of 3 sub-networks in the data-parallel step"
    la, lb = a.logs(), b.logs()
    sa, sb = a.state_dict(), b.state_dict()
    # per tensor: number of elements that differ by more than a quarter RMSprop step (8e-5), over the allowance
    # max(4, 1 %) (see tests/test_stage1_gpu.py::_same_update for why single elements may flip)
    worst = 0.0
    for k in sa:
        ta, tb = sa[k].float().reshape(-1), sb[k].float().reshape(-1)
        lim = max(2e-5 * float(tb.abs().max()), 8e-5)
        bad = int(((ta - tb).abs() > lim).sum())
        worst = max(worst, bad / max(4, ta.numel() // 100))
    q.put((rank, {k: (la[k], lb[k]) for k in ("loss_encoder", "loss_decoder", "loss_discriminator", "kl")}, worst,
           {k: float(v.float().norm()) for k, v in sa.items()}))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.selfcheck
def test_two_rank_hybrid_step_equals_eager_step_local_bn():
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_hybrid, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(_collect(procs, q, 2), key=lambda t: t[0])
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    for rank, logs, worst, _ in res:
        for k, (va, vb) in logs.items():
            assert abs(va - vb) < 1e-5 * abs(vb), (rank, k, va, vb)
        assert worst <= 1.0, (rank, worst)
    # gradients were summed over the ranks: both hold identical parameters after the step (the running statistics are
    # per rank in this mode)
    for k in res[0][3]:
        if "running_" in k:
            continue
        assert abs(res[0][3][k] - res[1][3][k]) <= 1e-6 * abs(res[0][3][k]) + 1e-9, k


@_guarded
def _worker_segments(port, q):
    """1-rank RCCL group on the GPU (FMRI_FORCE_DIST): a step replayed as graph segments + eager collectives must
    leave the same state as eagerly issued steps."""
    os.environ["FMRI_FORCE_DIST"] = "1"
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import Stage1Step
    B = 8
    data = O.synth_batch(B, O.ArchCfg.px64(), seed=77, steps=1)
    x, e, z = data["x"].cuda(), data["noise"][0, 0].cuda(), data["noise"][0, 1].cuda()
    out = []
    for mode in ("eager", "segments"):
        st = Stage1Step(ArchConfig.px64(), "cuda:0", distributed=True, sync_bn=True)
        assert st.dd.on
        st.load_recipe(3, True)
        st.step(x, e, z)                               # lazy initialisation outside any capture
        if mode == "eager":
            st.step(x, e, z)
        else:
            run = st.capture(x, e, z, warmup=0)
            n_graphs = sum(isinstance(it, torch.cuda.CUDAGraph) for it in st._graph.items)
            n_coll = len(st._graph.items) - n_graphs
            assert n_coll >= 30 and n_graphs == n_coll + 1, (n_graphs, n_coll)
            run()
        torch.cuda.synchronize()
        out.append((st.logs(), {k: v.float().cpu() for k, v in st.state_dict().items()}))
    (la, sa), (lb, sb) = out
    # same inputs, (almost) same state -- the first step already differs by the accumulation order of float atomics in
    # the weight gradients: the losses of the second step agree to 1e-3, the updated state agrees globally (a sign-like RMSprop step can flip on individual ~0 gradients)
    num = sum(((sa[k] - sb[k]) ** 2).sum().item() for k in sa)
    den = sum((sa[k] ** 2).sum().item() for k in sa)
    worst = (num / den) ** 0.5
    ok = worst < 2e-3 and all(abs(la[k] - lb[k]) <= 1e-3 * abs(la[k]) + 1e-6
                              for k in ("loss_encoder", "loss_decoder", "loss_discriminator", "kl", "mse", "nle"))
    q.put((bool(ok), worst, la["loss_encoder"], lb["loss_encoder"]))
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.selfcheck
def test_graph_segments_with_eager_collectives_equal_eager_steps():
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    p = ctx.Process(target=_worker_segments, args=(_free_port(), q))
    p.start()
    p.join(300)
    assert p.exitcode == 0
    ok, worst, la, lb = _collect([p], q, 1)[0]
    assert ok, (worst, la, lb)


# ---- the other fused steps, two ranks (global-batch BatchNorm statistics) vs one process on the global batch ----------
def _build_step(kind, dist_on):
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import CognitiveStep
    from fmri_hip.wae_steps import DualStage1Step, WaeStep
    cfg = ArchConfig.px64()
    if kind in ("stage2", "stage3"):
        st = CognitiveStep(cfg, 512, "cuda:0", int(kind[-1]), distributed=dist_on, sync_bn=True)
        st.load_recipe(1, True)
    elif kind in ("wae1", "wae2", "wae3"):
        st = WaeStep(cfg, "cuda:0", int(kind[-1]), 512 if kind != "wae1" else 0, distributed=dist_on, sync_bn=True)
        st.load_recipe(5, False)
    else:
        st = DualStage1Step(cfg, "cuda:0", distributed=dist_on, sync_bn=True)
        st.load_recipe(8, True)
    return st


def _run_step(kind, st, data, sl):
    x, nz = data["x"][sl].cuda(), data["noise"][0][:, sl].cuda()
    if kind in ("stage2", "stage3"):
        st.step(data["fmri"][sl].cuda(), x, nz[0], nz[1], nz[2])
    elif kind == "wae1":
        st.step(x, nz[2])
    elif kind in ("wae2", "wae3"):
        st.step(x, fmri=data["fmri"][sl].cuda())
    else:
        st.step(x, nz[0], nz[1], nz[2])
    torch.cuda.synchronize()
    return st.logs(), {k: float(v.float().norm()) for k, v in st.state_dict().items()}


@_guarded
def _worker_other(rank, world, port, kind, q):
    _init(rank, world, port)
    from oracle import vaegan_oracle as O
    torch.cuda.set_device(0)
    B = 4
    data = O.synth_batch(2 * B, O.ArchCfg.px64(), n_voxels=512, seed=1234, steps=1)
    st = _build_step(kind, True)
    logs, sdn = _run_step(kind, st, data, slice(rank * B, (rank + 1) * B))
    q.put((rank, logs, sdn))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.selfcheck
@pytest.mark.parametrize("kind", ["stage2", "stage3", "wae1", "wae2", "wae3", "dual1"])
def test_two_rank_other_steps_equal_single_process_global_batch(kind):
    """CognitiveStep (Stage II / III), WaeStep and DualStage1Step with distributed=True on two half batches (asynchronous
    per-sub-network gradient reductions, global-batch BatchNorm statistics, summed loss scalars) against the same step in
    one process on the full batch: same logged losses, same parameters after the step, identical on both ranks."""
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_other, args=(r, 2, port, kind, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(_collect(procs, q, 2), key=lambda t: t[0])
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    from oracle import vaegan_oracle as O
    data = O.synth_batch(8, O.ArchCfg.px64(), n_voxels=512, seed=1234, steps=1)
    logs1, sd1 = _run_step(kind, _build_step(kind, False), data, slice(0, 8))
    for rank, logs, sdn in res:
        for k, v in logs1.items():
            if isinstance(v, float):
                assert abs(logs[k] - v) < 5e-4 * abs(v) + 1e-6, (kind, rank, k, logs[k], v)
            else:
                assert logs[k] == v, (kind, rank, k)
        for k, v in sd1.items():
            slack = 1e-3 if v < 1.0 else 0.0       # tiny tensors (biases): one sign-like update flips the norm
            assert abs(sdn[k] - v) < 3e-3 * v + slack + 1e-6, (kind, rank, k, sdn[k], v)
    for k in res[0][2]:
        assert abs(res[0][2][k] - res[1][2][k]) <= 1e-6 * abs(res[0][2][k]) + 1e-9, (kind, k)


@pytest.mark.gpu
@pytest.mark.selfcheck
@pytest.mark.parametrize("extra", [[], ["--sync-bn"], ["--full"]])
def test_bench_two_rank_control_flow_rehearsal(extra, tmp_path):
    """bench.py's multi-process control flow (what the driver launches for N > 1) with two ranks sharing this one GPU,
    gloo as the collective backend: launch-mode probe decided collectively, barrier + max-over-ranks timing, one JSON
    line from rank 0 with the whole-job aggregate, finite losses, exit code 0; with --full also the collective gate-skip
    pass and the one-stream profiling pass.  (Two GPUs over RCCL are not available to the tests; the data path of the
    ranks is covered by the 2-rank step tests above.)"""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, FMRI_REHEARSE_ON_ONE_GPU="1", FMRI_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "8",
           "--warmup", "3", "--batch", "64", "--no-cpu-baseline", "--no-hbm-rows", "--no-pmc"] + extra
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 8 and out["warmup"] == 3 and out["scaling"] == "weak"
    assert out["config"]["global_batch"] == 128 and out["config"]["batch_per_gpu"] == 64
    assert out["config"]["parallelism"] == ("dp2-syncbn" if "--sync-bn" in extra else "dp2-localbn")
    assert ("gate_skip" in out and "roofline" in out) == ("--full" in extra)
    assert out["losses_finite"] is True and out["value"] > 0
    assert abs(out["value"] - 128 * 8 / (out["ms_per_step"] * 8e-3)) < 0.01 * out["value"]      # whole-job aggregate


@_guarded
def _worker_gpu_range(rank, world, port, q):
    """SyncBN step whose latent batch leaves fp16's range on ONE rank only (that rank's eps is scaled by 3e5)."""
    _init(rank, world, port)
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import Stage1Step
    torch.cuda.set_device(0)
    B = 4
    data = O.synth_batch(2 * B, O.ArchCfg.px64(), seed=1234, steps=1)
    eps = data["noise"][0, 0].clone()
    eps[B:] *= 3.0e5
    sl = slice(rank * B, (rank + 1) * B)
    st = Stage1Step(ArchConfig.px64(), "cuda:0", distributed=True, sync_bn=True)
    st.load_recipe(0, True)
    st.step(data["x"][sl].cuda(), eps[sl].cuda(), data["noise"][0, 1][sl].cuda())
    torch.cuda.synchronize()
    sd = st.state_dict()
    q.put((rank, st.logs(), float(st.zs[0]), all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point()),
           {k: float(v.float().norm()) for k, v in sd.items() if k.startswith("decoder.fc")}))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.selfcheck
def test_two_rank_syncbn_latent_range_is_the_global_maximum():
    """Range-scaled latent rows under SyncBN: the decoder's BatchNorm batch is the GLOBAL one, so the power-of-two
    scale must come from the global max |z| (MAX all-reduce) -- here only rank 1's rows leave fp16's range.  Both ranks use
    the scale of the single-process global batch, stay finite and reproduce its losses and its decoder.fc update."""
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_gpu_range, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(_collect(procs, q, 2), key=lambda t: t[0])
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import Stage1Step
    B = 8
    data = O.synth_batch(B, O.ArchCfg.px64(), seed=1234, steps=1)
    eps = data["noise"][0, 0].clone()
    eps[B // 2:] *= 3.0e5
    st = Stage1Step(ArchConfig.px64(), "cuda:0")
    st.load_recipe(0, True)
    st.step(data["x"].cuda(), eps.cuda(), data["noise"][0, 1].cuda())
    torch.cuda.synchronize()
    logs1, s1 = st.logs(), float(st.zs[0])
    sd1 = {k: float(v.float().norm()) for k, v in st.state_dict().items() if k.startswith("decoder.fc")}
    assert s1 < 1.0 / 512, s1                     # |z| ~ 3e5 * sigma: far outside fp16 at scale 1
    for rank, logs, s, finite, sdn in res:
        assert s == s1, (rank, s, s1)
        assert finite, rank
        for k in ("loss_encoder", "loss_decoder", "loss_discriminator", "kl", "mse", "nle"):
            assert abs(logs[k] - logs1[k]) < 2e-3 * abs(logs1[k]), (rank, k, logs[k], logs1[k])
        for k, v in sd1.items():
            assert abs(sdn[k] - v) < 2e-3 * v + 1e-6, (rank, k, sdn[k], v)
