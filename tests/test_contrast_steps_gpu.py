"""GPU checks of WaeStep(contrast=LatentContrast(...)) for Stages II / III under either latent penalty: against the composed
oracle step of tests/contrast_oracle.py (tolerances: those tests/test_mmd_gpu.py applies to the MMD step), the frozen
Stage-III encoder, weight = 0 against the plain step, the untouched step without the keyword, HIP-graph capture, two
ranks against one process on the global batch, and a 150-step run."""
import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import contrast_oracle as CO
import gradcheck

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WAE_KEYS = ("loss_reconstruction", "loss_penalty", "loss_discriminator_fake", "loss_discriminator_real")
CON_KEYS = ("loss_contrast", "latent_top1")
V, TAU = 512, 0.07


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-12)


def _terr(got, ref):
    got, ref = got.detach().float().cpu().reshape(-1), ref.detach().float().cpu().reshape(-1)
    return ((got - ref).norm() / (ref.norm() + 1e-20)).item()


def _state(O, cfg, seed):
    teacher = O.fill_state(O.encoder_spec(cfg) + O.decoder_spec(cfg) + O.wae_discriminator_spec(cfg), seed, True)
    P = dict(O.fill_state(O.cognitive_encoder_spec(cfg, V), seed + 100, True))
    P.update({k: v for k, v in teacher.items() if k.startswith("decoder.")})
    P.update(O.fill_state(O.wae_discriminator_spec(cfg), seed + 200, True))
    P.update({"teacher_net." + k: v for k, v in teacher.items() if k.startswith("encoder.")})
    return P


def _opts(O):
    return {"encoder": O.OptState(kind="adam", lr=1e-3), "decoder": O.OptState(kind="adam", lr=1e-3),
            "discriminator": O.OptState(kind="adam", lr=5e-4)}


def _step(stage, penalty, contrast, **kw):
    from fmri_hip.params import ArchConfig
    from fmri_hip.wae_steps import WaeStep
    st = WaeStep(ArchConfig.px64(), DEV, stage, V, penalty=penalty, contrast=contrast, **kw)
    st.load_recipe(5, False)
    return st


def _con(weight=1.0):
    from fmri_hip.contrast import LatentContrast
    return LatentContrast(weight, TAU)


@pytest.mark.parametrize("B", [4, 32])
@pytest.mark.parametrize("penalty", ["gan", "mmd"])
@pytest.mark.parametrize("stage", [2, 3])
def test_contrast_wae_step_matches_composed_oracle(stage, penalty, B):
    """Tolerances: 1e-3 first-step losses, 5e-3 penalty and contrast term, 5e-2 later steps, 1e-2 outputs.  Measured on an
    MI355X: loss_contrast 4.5e-4 (B = 4) / 4.6e-7 (B = 32) at the first step; later Stage-II steps 1.1e-4 ... 1.2e-2 except
    B = 4 under the GAN penalty at the third step, 4.7e-2 -- the four pairs are memorised by then and the loss is 2.0e-4, a
    relative error of a near-zero value (the same figure in four repeated runs; profiles/contrast.md).  That case sits at
    94 % of the bound the step tests prescribe and rests on the step being bit-reproducible; should it ever fail, read it
    with the check below it: loss_contrast against the float64 loss of the engine's OWN latents (1e-3) is what pins the
    term itself there, the 5e-2 only how far the trajectory has drifted from the oracle's."""
    from oracle import vaegan_oracle as O
    seed, steps = 5, 3
    cfg_o = O.ArchCfg.px64()
    data = O.synth_batch(B, cfg_o, n_voxels=V, seed=1234, steps=steps)
    st = _step(stage, penalty, _con())
    rec = gradcheck.Recorder(st)
    enc0 = {k: v.clone() for k, v in st.state_dict().items() if k.startswith("encoder.")}
    P, opts = _state(O, cfg_o, seed), _opts(O)
    x, fm = data["x"].to(DEV), data["fmri"].to(DEV)
    for s in range(steps):
        rec.clear()
        st.step(x, fmri=fm)
        ref = CO.wae_nce_step(P, opts, stage, cfg_o, data["x"], data["fmri"], V, penalty, 1.0, TAU, keep_grads=True)
        logs = st.logs()
        assert tuple(logs) == WAE_KEYS + CON_KEYS
        for k in WAE_KEYS + CON_KEYS[:1]:
            print(stage, penalty, B, s, k, logs[k], ref["logs"][k], _rel(logs[k], ref["logs"][k]))
            if k.startswith("loss_discriminator") and penalty == "mmd":
                assert logs[k] == 0.0, k
            elif s == 0:
                assert _rel(logs[k], ref["logs"][k]) < (5e-3 if k in ("loss_penalty", "loss_contrast") else 1e-3), k
            else:
                assert _rel(logs[k], ref["logs"][k]) < 5e-2, (s, k)
        # the top-1 rate: the float64 count on the engine's own latents, rows within 2 eps_s of a tie left out
        outs = st.outputs()
        own = CO.nce64(outs["z_real"].cpu(), outs["z_teacher"].cpu(), TAU)
        hits, near = CO.top1_count(own, CO.eps_s(outs["z_real"].shape[1], TAU))
        got = logs["latent_top1"] * B
        print(stage, penalty, B, s, "latent_top1", logs["latent_top1"], "own hits", hits, "near", int(near.sum()),
              "own loss", float(own["loss"]))
        assert abs(got - round(got)) < 1e-3 and hits <= round(got) <= hits + int(near.sum()), (got, hits)
        assert _rel(logs["loss_contrast"], float(own["loss"])) < 1e-3
        assert logs["loss_contrast"] != 0.0
        if s == 0:
            for k in ("x_recon", "z_real"):
                e = _terr(outs[k], ref["fw"][k])
                print(stage, penalty, B, "fw", k, e)
                assert e < 1e-2, (k, e)
            grads = st.named_grads()
            P16 = _state(O, cfg_o, seed)
            with gradcheck.pinned(O, gradcheck.wae_masks(rec, B, stage, penalty=penalty)):
                ref16 = CO.wae_nce_step(P16, _opts(O), stage, cfg_o, data["x"], data["fmri"], V, penalty, 1.0, TAU,
                                        keep_grads=True)
            # the discriminator's gradients cancel 20-50 x between the two passes and l_mu.bias through the decoder's
            # first BatchNorm (tests/test_wae_gpu.py): reported there, not bounded here
            special = [k for k in ref["grads"] if k.startswith("discriminator.") or k.endswith("l_mu.bias")]
            for k in special:
                if k.endswith("l_mu.bias"):
                    print(stage, penalty, B, "grad", k, _terr(grads[k], ref["grads"][k]))
            gradcheck.check(grads, ref["grads"], ref16["grads"], f"wae{stage}-{penalty}-nce-b{B}", skip=special)
    if stage == 3:
        sd = st.state_dict()
        for k, v in enc0.items():
            if "running" not in k and "num_batches" not in k:
                assert torch.equal(sd[k], v), k


@pytest.mark.parametrize("penalty", ["gan", "mmd"])
def test_weight_zero_equals_the_plain_step_bit_for_bit(deterministic, penalty):
    from oracle import vaegan_oracle as O
    data = O.synth_batch(4, O.ArchCfg.px64(), n_voxels=V, seed=1234, steps=1)
    x, fm = data["x"].to(DEV), data["fmri"].to(DEV)
    a, b = _step(2, penalty, None), _step(2, penalty, _con(0.0))
    for _ in range(3):
        a.step(x, fmri=fm)
        b.step(x, fmri=fm)
    torch.cuda.synchronize()
    la, lb = a.logs(), b.logs()
    assert tuple(la) == WAE_KEYS                       # without the keyword: the four keys it always had
    assert tuple(lb) == WAE_KEYS + CON_KEYS and lb["loss_contrast"] == 0.0
    for k in WAE_KEYS:
        assert la[k] == lb[k], k
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_step_without_the_keyword_is_untouched_and_stage1_is_rejected():
    from fmri_hip.params import ArchConfig
    from fmri_hip.schedule import TrainLog
    from fmri_hip.wae_steps import WaeStep
    st = _step(2, "gan", None, log=TrainLog(8))
    cols, losses = st._log_columns()
    assert tuple(c[0] for c in cols) == WAE_KEYS and tuple(losses) == WAE_KEYS
    sc = _step(3, "mmd", _con(), log=TrainLog(8))
    cols, losses = sc._log_columns()
    assert tuple(c[0] for c in cols) == WAE_KEYS + CON_KEYS and "latent_top1" not in losses
    rs = np.random.RandomState(3)
    x = torch.tanh(torch.from_numpy(rs.standard_normal((4, 3, 64, 64)).astype(np.float32))).to(DEV)
    fm = torch.from_numpy(rs.standard_normal((4, V)).astype(np.float32)).to(DEV)
    for _ in range(2):
        st.step(x, fmri=fm)
        sc.step(x, fmri=fm)
    h, hc = st.history(), sc.history()
    assert set(st.outputs()) == {"x_recon", "z_real"} and "z_teacher" in sc.outputs()
    assert "loss_contrast" not in h and "latent_top1" not in h
    assert len(hc["loss_contrast"]) == 2 and hc["loss_contrast"][-1] == np.float32(sc.logs()["loss_contrast"])
    assert 0.0 <= hc["latent_top1"][-1] <= 1.0
    with pytest.raises(ValueError):
        WaeStep(ArchConfig.px64(), DEV, 1, contrast=_con())
    # a global batch without in-batch negatives is refused before anything of the step is launched
    before = sc.logs()
    with pytest.raises(ValueError, match="global batch"):
        sc.step(x[:1], fmri=fm[:1])
    assert sc.logs() == before


def test_stage2_150_steps_stay_finite():
    from oracle import vaegan_oracle as O
    B = 64
    data = O.synth_batch(B, O.ArchCfg.px64(), n_voxels=V, seed=77, steps=1)
    st = _step(2, "gan", _con())
    x, fm = data["x"].to(DEV), data["fmri"].to(DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    for s in range(150):
        scal = st.step(x, fmri=fm)
        bad += (~torch.isfinite(scal[:28])).any().int()
    torch.cuda.synchronize()
    logs = st.logs()
    print("after 150 steps", logs)
    assert bad.item() == 0
    assert all(np.isfinite(v) for v in logs.values())
    assert all(bool(torch.isfinite(v).all()) for v in st.state_dict().values() if v.is_floating_point())


# ---- self-checks ------------------------------------------------------------------------------------------------------
@pytest.mark.selfcheck
@pytest.mark.parametrize("penalty", ["gan", "mmd"])
def test_contrast_step_recorded_into_a_hip_graph_equals_eager_steps(deterministic, penalty):
    B = 8
    rs = np.random.RandomState(11)
    x = torch.tanh(torch.from_numpy(rs.standard_normal((B, 3, 64, 64)).astype(np.float32))).to(DEV)
    fm = torch.from_numpy(rs.standard_normal((B, V)).astype(np.float32)).to(DEV)
    args = (x, None, fm)
    a, b = _step(2, penalty, _con()), _step(2, penalty, _con())
    s0 = {k: v.clone() for k, v in a.state_dict().items()}
    for _ in range(5):
        a.step(*args)
    run = b.capture(*args)            # two eager warm-up steps inside; records a one-stream step
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    la = a.logs()
    assert la == b.logs() and la["loss_contrast"] != 0.0
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert any(k.startswith("encoder.") and not torch.equal(sa[k], s0[k]) for k in sa)


def _worker(rank, world, port, stage, q):
    import traceback
    try:
        import test_distributed as TD
        TD._init(rank, world, port)
        import torch.distributed as dist
        from oracle import vaegan_oracle as O
        torch.cuda.set_device(0)
        B = 4
        data = O.synth_batch(2 * B, O.ArchCfg.px64(), n_voxels=V, seed=1234, steps=1)
        st = _step(stage, "gan", _con(), distributed=True, sync_bn=True)
        logs, sdn = _run(st, data, slice(rank * B, (rank + 1) * B))
        q.put((rank, logs, sdn))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:
        q.put(("error", traceback.format_exc()))
        raise


def _run(st, data, sl):
    st.step(data["x"][sl].cuda(), fmri=data["fmri"][sl].cuda())
    torch.cuda.synchronize()
    return st.logs(), {k: float(v.float().norm()) for k, v in st.state_dict().items()}


@pytest.mark.selfcheck
@pytest.mark.parametrize("stage", [2, 3])
def test_contrast_two_rank_equals_single_process_global_batch(stage):
    """distributed=True on two half batches (q and t gathered by one SUM all-reduce, the global statistic on both ranks,
    each rank's own gradient rows) against one process on the full batch, in the pattern and with the tolerances of
    tests/test_mmd_gpu.py::test_mmd_two_rank_equals_single_process_global_batch."""
    import test_distributed as TD
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = TD._free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, stage, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(TD._collect(procs, q, 2), key=lambda t: t[0])
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    from oracle import vaegan_oracle as O
    data = O.synth_batch(8, O.ArchCfg.px64(), n_voxels=V, seed=1234, steps=1)
    logs1, sd1 = _run(_step(stage, "gan", _con()), data, slice(0, 8))
    assert logs1["loss_contrast"] != 0.0
    for rank, logs, sdn in res:
        for k, v in logs1.items():
            assert abs(logs[k] - v) < 5e-4 * abs(v) + 1e-6, (stage, rank, k, logs[k], v)
        for k, v in sd1.items():
            slack = 1e-3 if v < 1.0 else 0.0
            assert abs(sdn[k] - v) < 3e-3 * v + slack + 1e-6, (stage, rank, k, sdn[k], v)
    assert res[0][1]["latent_top1"] == res[1][1]["latent_top1"]
    for k in res[0][2]:
        assert abs(res[0][2][k] - res[1][2][k]) <= 1e-6 * abs(res[0][2][k]) + 1e-9, (stage, k)
