"""The deferred weight-gradient queue (ops.GradQueue) on the device, at the B = 4, 64-px configuration of the ``*_b4``
goldens: what a fused step leaves in the declared state, and a layer that issues two weight gradients in one pass."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 4


def _step_and_batch():
    from oracle import vaegan_oracle as O
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import Stage1Step
    data = O.synth_batch(B, O.ArchCfg.px64(), seed=1234, steps=1)
    st = Stage1Step(ArchConfig.px64(), DEV)
    st.load_recipe(0, True)
    return st, (data["x"].to(DEV), data["noise"][0, 0].to(DEV), data["noise"][0, 1].to(DEV))


def _layers(net):
    """Every object of a sub-network that issues weight gradients (the layers, also inside lists and the fused heads)."""
    from fmri_hip import ops
    found = []
    for v in vars(net).values():
        for lay in (v if isinstance(v, (list, tuple)) else [v]):
            for obj in [lay] + (list(vars(lay).values()) if hasattr(lay, "__dict__") else []):
                if isinstance(getattr(obj, "ghold", None), ops.GradHold) and not any(obj is f for f in found):
                    found.append(obj)
    return found


def _finish():
    from fmri_hip import ops
    ops.join_side()
    torch.cuda.synchronize()


def test_a_fused_step_leaves_the_queues_empty_and_the_holds_free():
    st, args = _step_and_batch()
    nets = (st.enc, st.dec, st.dis)
    st.step(*args)
    _finish()
    layers = [lay for n in nets for lay in _layers(n)]
    assert len(layers) >= 15, f"only {len(layers)} layers found: the walk over the sub-networks missed them"
    assert sum(len(lay.ghold.bufs) for lay in layers) >= len(layers), "the step did not go through the layers' holds"
    for lay in layers:
        assert lay.ghold.busy is False, f"{type(lay).__name__}: hold still busy after the step"
    for n in nets:
        q = n.group.gq
        assert q.pending == [] and q.materialized == [] and q.defer is False
        assert q.consumed is True, "the sub-network did not take the one-launch update"
        with pytest.raises(RuntimeError, match="consumed by its fused update"):
            n.group.check_grads_readable()
    st.forward(*args)
    st.gate(B)
    st.backward()
    _finish()
    for n in nets:
        n.group.check_grads_readable()
        assert n.group.gq.consumed is False and n.group.gq.pending == []
    assert all(lay.ghold.busy is False for lay in layers)


def test_two_gradients_of_one_layer_in_one_pass(deterministic):
    """Both cotangent streams train the discriminator: every conv layer issues two weight gradients into the same tensor.
    Deferred, the second launch finds the layer's hold busy and gets a fresh, untracked buffer; the table of the
    one-launch update cannot describe two gradients of one tensor, so the queue falls back to the separate launches --
    which must leave the bits the non-deferred pass leaves."""
    from fmri_hip import ops
    a, args = _step_and_batch()
    b, _ = _step_and_batch()

    def backward(st, defer):
        st.forward(*args)
        st.gate(B)
        group = st.dis.group
        ops.begin_grads(group, defer)
        dlogit16, dfeat16, _ = st._start_cotangents(B)
        st.dis.backward(st.fw["sctx"], dlogit16, st.sc.a, dfeat16, st.sc.b, True, None, train_b=True)
        return group

    ga = backward(a, True)
    q = ga.gq
    assert q.defer and len(q.pending) > 0
    by_tensor = {}
    for e in q.pending:
        by_tensor.setdefault(e.grad_view.data_ptr(), []).append(e)
    twice = [es for es in by_tensor.values() if len(es) == 2]
    assert len(twice) >= 4, f"only {len(twice)} tensors with two queued gradients"
    for first, second in twice:
        assert first.out.hold is not None and first.out.hold.busy and first.out.hold.bufs[
            (tuple(first.out.buf.shape), first.out.clear)] is first.out.buf
        assert second.out.hold is None and second.out.clear is False
        assert second.out.buf.data_ptr() != first.out.buf.data_ptr() and second.out.buf.shape == first.out.buf.shape
    assert q.plan(a.opt_dis.s1) is None, "a table was built for two gradients of one tensor"
    assert ops.apply_group(ga, a.opt_dis.s1, a.opt_dis.lr_dev, a.opt_dis.alpha, a.opt_dis.eps, None, None) is False
    assert q.pending == [] and q.defer is False and q.consumed is False
    assert all(lay.ghold.busy is False for lay in _layers(a.dis))
    gb = backward(b, False)
    assert gb.gq.pending == []
    _finish()
    assert float(ga.grad.abs().max()) > 0
    bad = int((ga.grad != gb.grad).sum())
    assert bad == 0, f"{bad} of {ga.grad.numel()} gradient elements differ between the deferred and the direct pass"
