"""The declared state of the deferred weight-gradient path (ops.GradQueue, ops.GradHold, ops.WgradOut) on the host: what
FlatGroup and the layers declare at construction, the one accessor for stand-in groups, and the hand-out rules of a
layer's hold.  No launch is made: the layer constructors only size and zero their fp16 copies."""
import pytest
import torch

import epilogue_oracle as EO
from fmri_hip import ops
from fmri_hip.nets import _Versioned
from fmri_hip.params import ArchConfig, FlatGroup, encoder_spec

CPU = torch.device("cpu")


class _VersionedViews(_Versioned):
    """``_Versioned`` exposes only ``.version`` (FusedHeads hands its dense layer explicit tensor pairs); a ConvLayer looks
    its tensors up by key, so for that layer the adapter also passes the owner's ``views`` / ``grads`` through."""

    def __init__(self, group):
        super().__init__(group)
        self.views, self.grads = group.views, group.grads


def _tensors():
    g = torch.Generator().manual_seed(5)
    return {"c.weight": torch.randn(16, 8, 5, 5, generator=g), "c.bias": torch.randn(16, generator=g),
            "d.weight": torch.randn(24, 40, generator=g), "d.bias": torch.randn(24, generator=g)}


def _stand_in(kind):
    owner = EO.Group(_tensors(), CPU)
    return owner if kind == "Group" else _VersionedViews(owner)


@pytest.mark.parametrize("kind", ["Group", "_Versioned"])
def test_layers_on_a_stand_in_group_register_their_weights_and_never_defer(kind):
    group = _stand_in(kind)
    assert "gq" not in vars(group) and "packed" not in vars(group)
    conv = ops.ConvLayer(group, "c.weight", "c.bias", "conv", 8, 16, 5, 2, 2)
    if kind == "Group":
        dense = ops.DenseLayer(group, "d.weight", "d.bias", 40, 24)
    else:                   # as FusedHeads builds its fallback layer: explicit (weight, grad) / (bias, grad) pairs
        dense = ops.DenseLayer(group, (group.views["d.weight"], group.grads["d.weight"]), (group.views["d.bias"], None),
                               40, 24)
    assert group.packed == [conv.pw_f, conv.pw_d, dense.pw_f, dense.pw_d]
    assert all(isinstance(pw, ops.PackedWeight) and pw.version == -1 for pw in group.packed)
    assert conv.pw_d.taps_of is conv.pw_f and dense.pw_d.transpose_of is dense.pw_f
    q = ops.grad_queue(group)
    assert isinstance(q, ops.GradQueue) and q is group.gq and q is ops.grad_queue(group) and q.group is group
    assert q.defer is False and q.gate is None and q.pending == [] and q.materialized == []
    for layer in (conv, dense):
        assert isinstance(layer.ghold, ops.GradHold) and layer.ghold.busy is False and layer.ghold.bufs == {}
        assert ops._hold_of(layer) is None and ops._gate_of(layer) is None
    assert (conv._stat_part, conv._bwd_part, conv._stat_rows, conv._bwd_rows) == (None, None, 0, 0)
    assert conv.aff_applied is False and conv.act_applied is False
    assert conv.take_stats() is None and conv.take_bwd_stats() is None


def test_flat_group_declares_its_queue_at_construction():
    group = FlatGroup(encoder_spec(ArchConfig.px64()), CPU)
    q = group.gq
    assert isinstance(q, ops.GradQueue) and ops.grad_queue(group) is q and q.group is group
    assert group.packed == []
    assert vars(q) == dict(group=group, defer=False, gate=None, pending=[], materialized=[], consumed=False, cleared="all",
                           flat_clear=None, plans={}, no_state=None, pack_tables={})
    group.check_grads_readable()                       # nothing consumed, nothing deferred
    layer = ops.DenseLayer(group, "l_mu.weight", "l_mu.bias", 1024, 128)
    assert group.packed == [layer.pw_f, layer.pw_d] and group.gq is q
    # what the queue's owner may do without a device: forget an empty queue, clear the whole buffer
    group.grad.fill_(1.0)
    q.consumed = True
    group.zero_grad()
    assert float(group.grad.abs().max()) == 0.0 and q.consumed is False and q.cleared == "all"
    q.defer = True
    with pytest.raises(RuntimeError, match="consumed by its fused update"):
        group.check_grads_readable()
    group.drop_pending()
    assert q.defer is False
    group.check_grads_readable()


def test_batchnorm_declares_its_lazy_running_state():
    C = 16
    group = EO.bn_group({}, C, CPU, seed=1)
    group.flush_hooks, group.buf_version = [], 0
    bn = ops.BatchNorm(group, "bn.", C, perm=(4, 4))
    assert (bn._lazy, bn._run_v, bn._run_dirty) == (False, -1, False)
    bn.enable_lazy_running()
    bn.enable_lazy_running()                           # (idempotent: one flush hook)
    assert (bn._lazy, bn._run_v, bn._run_dirty) == (True, -1, False) and group.flush_hooks == [bn.flush_running]
    plain = ops.BatchNorm(group, "bn.", C)
    plain.enable_lazy_running()                        # only the (C,H,W)-permuted form has engine-order copies
    assert plain._lazy is False


def test_a_hold_hands_out_its_buffer_once_per_pass_and_fresh_tensors_while_busy():
    hold = ops.GradHold()
    a = ops._wgrad_out(hold, (2, 32, 128), True, CPU, 128)
    assert a.hold is hold and a.clear is True and a.colsum is False and a.ld == 128 and hold.busy is True
    assert hold.bufs == {((2, 32, 128), True): a.buf} and float(a.buf.abs().max()) == 0.0
    # a second gradient of the layer in the same pass: a fresh, untracked tensor whose release is a no-op
    b = ops._wgrad_out(hold, (2, 32, 128), True, CPU, 128, colsum=True)
    assert b.hold is None and b.clear is False and b.colsum is True and b.buf.data_ptr() != a.buf.data_ptr()
    assert tuple(b.buf.shape) == (2, 32, 128) and float(b.buf.abs().max()) == 0.0 and len(hold.bufs) == 1
    q = ops.GradQueue(None)
    gv, sp = torch.zeros(4), ops.PackSpec(sa=1, sta=0, A=1, TA=1, sb=1, stb=0, B=1)
    b.buf.fill_(3.0)
    q._retire([ops.GradEntry(b, gv, sp, 1.0)], zero=True)
    assert hold.busy is True and float(b.buf.min()) == 3.0
    a.buf.fill_(3.0)
    q._retire([ops.GradEntry(a, gv, sp, 1.0)], zero=True)
    assert hold.busy is False and float(a.buf.abs().max()) == 0.0
    # the next pass gets the same storage back; a buffer the kernel stores into is another one and is never cleared
    a2 = ops._wgrad_out(hold, (2, 32, 128), True, CPU, 128)
    assert a2.buf is a.buf and a2.hold is hold
    hold.busy = False
    c = ops._wgrad_out(hold, (32, 128), False, CPU, 128)
    assert c.hold is hold and c.clear is False and len(hold.bufs) == 2
    # without a hold (gradients not deferred): fresh, nothing to release
    d = ops._wgrad_out(None, (32, 128), True, CPU, 128)
    assert d.hold is None and d.clear is False and float(d.buf.abs().max()) == 0.0


def test_a_hold_does_not_collect_a_buffer_per_batch_size():
    hold = ops.GradHold()
    for n in range(1, 7):
        ops._grad_buffer(hold, (n, 8), True, CPU)
        hold.busy = False
    assert len(hold.bufs) == 6
    kept = ops._grad_buffer(hold, (3, 8), True, CPU)       # a shape it has: nothing is dropped
    hold.busy = False
    assert len(hold.bufs) == 6 and kept is hold.bufs[((3, 8), True)]
    ops._grad_buffer(hold, (7, 8), True, CPU)              # a seventh shape: the six go, the new one stays
    assert list(hold.bufs) == [((7, 8), True)]


def test_weight_gradient_buffers_are_taken_through_the_module_global(monkeypatch):
    """tests/test_fullbatch_conv_gpu.py replaces ``ops._grad_buffer`` and expects every weight-gradient launch to go
    through the replacement."""
    seen = []
    real = ops._grad_buffer

    def spy(hold, shape, zeroed, device):
        seen.append((tuple(shape), bool(zeroed)))
        return real(hold, shape, zeroed, device)
    monkeypatch.setattr(ops, "_grad_buffer", spy)
    out = ops._wgrad_out(None, (32, 128), False, CPU, 128)
    assert seen == [((32, 128), False)] and tuple(out.buf.shape) == (32, 128)
