"""Numerics monitor in a data-parallel step (2 ranks sharing the one GPU of the test box, gloo on device tensors, the
pattern of tests/test_distributed.py): the gradient statistics are taken after the SUM all-reduce, so both ranks report
the same values; the BatchNorm counts and the latent statistics are each rank's own."""
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_distributed import _collect, _free_port, _guarded, _init

pytestmark = pytest.mark.gpu


@_guarded
def _worker(rank, world, port, q):
    _init(rank, world, port)
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import Stage1Step
    torch.cuda.set_device(0)
    B = 4
    data = O.synth_batch(2 * B, O.ArchCfg.px64(), seed=1234, steps=1)
    sl = slice(rank * B, (rank + 1) * B)
    st = Stage1Step(ArchConfig.px64(), "cuda:0", distributed=True, sync_bn=True, monitor=True)
    st.load_recipe(0, True)
    st.step(data["x"][sl].cuda(), data["noise"][0, 0][sl].cuda(), data["noise"][0, 1][sl].cuda())
    num = st.numerics()
    mu = st.outputs()["mus"]
    q.put((rank, num["grad"], num["latent"]["mu_max_abs"], float(mu.abs().max())))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_report_the_same_gradient_statistics():
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(_collect(procs, q, 2), key=lambda t: t[0])
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    (_, g0, m0, r0), (_, g1, m1, r1) = res
    assert g0 == g1, (g0, g1)
    assert any(v["updated"] for v in g0.values())
    assert g0["encoder"]["updated"] and g0["encoder"]["norm"] > 0
    # latent statistics are the rank's own rows
    assert m0 == r0 and m1 == r1
