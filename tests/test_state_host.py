"""Host side of the training-state ring (fmri_hip/state.py; include/fmri_hip.h fmri_state_layout / fmri_state_copy): the
slot layout, the layout fingerprint, the firing predicate's slot arithmetic and the ``TrainState`` file.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from fmri_hip import build, lib as L
    build.build(verbose=False)
    return L.load()


def _layout(lib, nbytes):
    n = len(nbytes)
    arr = (ctypes.c_int64 * max(n, 1))(*nbytes)
    offs = (ctypes.c_int64 * max(n, 1))()
    size = lib.fmri_state_layout(arr, n, offs)
    return size, list(offs)[:n]


def test_layout_is_a_header_and_16_byte_aligned_segments(lib):
    from fmri_hip import state
    nbytes = [0, 4, 12, 16, 20, 4096 + 4]
    size, offs = _layout(lib, nbytes)
    # 64-byte header, every segment rounded up to 16 bytes: 0, 16, 16, 16, 32, 4112
    assert offs == [64, 64, 80, 96, 112, 144]
    assert size == 64 + 0 + 16 + 16 + 16 + 32 + 4112
    assert all(o % 16 == 0 and o >= 64 for o in offs)
    for (o, b), nxt in zip(zip(offs, nbytes), offs[1:] + [size]):
        assert o + b <= nxt < o + b + 16                         # apart, and no more than the padding between them
    assert _layout(lib, []) == (64, [])
    assert lib.fmri_state_layout(None, 0, None) == 64
    assert lib.fmri_state_layout((ctypes.c_int64 * 2)(8, 24), 2, None) == 64 + 16 + 32      # offsets_out may be NULL
    assert state.layout(nbytes) == (size, offs)


def test_layout_rejects_bad_arguments(lib):
    from fmri_hip import state
    assert _layout(lib, [16, -4])[0] < 0
    for bad in (1, 2, 3, 6, 4097):
        assert _layout(lib, [16, bad, 16])[0] < 0, bad
    assert lib.fmri_state_layout((ctypes.c_int64 * 1)(16), -1, None) == -1
    assert lib.fmri_state_layout(None, 2, None) == -1
    with pytest.raises(ValueError):
        state.layout([16, 6])


def test_copy_rejects_bad_arguments_without_a_gpu(lib):
    """fmri_state_copy checks the host copy of its table before anything is enqueued."""
    from fmri_hip import lib as L
    z = ctypes.c_void_p(0x1000)

    def copy(rows, slot=4096, ring=3 * 4096, direction=0, feed=None, every=0, capacity=2, segs_dev=z, base=z):
        tab = (L.StateSeg * max(len(rows), 1))()
        for t, (live, off, nb, c0) in zip(tab, rows):
            t.live, t.offset, t.bytes, t.chunk0 = live, off, nb, c0
        return lib.fmri_state_copy(tab, segs_dev, len(rows), base, ring, slot, direction, feed, every, capacity, 7, None,
                                   None)
    ok = [(0x2000, 64, 16, 0)]
    assert copy([(0x2002, 64, 16, 0)]) == -1                         # live address not a multiple of 4
    assert copy([(0x2000, 64, 18, 0)]) == -1                         # byte count not a multiple of 4
    assert copy([(0x2000, 72, 16, 0)]) == -1                         # slot offset not a multiple of 16
    assert copy([(0x2000, 48, 16, 0)]) == -1                         # inside the header
    assert copy([(0x2000, 64, 32, 0), (0x3000, 80, 16, 1)]) == -1    # overlapping its predecessor
    assert copy([(0x2000, 64, 16, 0), (0x3000, 80, 16, 0)]) == -1    # chunk0 is not the running chunk count
    assert copy([(0x2000, 4080, 32, 0)]) == -1                       # behind the end of the slot
    assert copy(ok, ring=2 * 4096) == -1                             # ring smaller than capacity + 1 slots
    assert copy(ok, slot=4100) == -1 and copy(ok, base=ctypes.c_void_p(0x1008)) == -1
    assert copy(ok, every=2) == -1                                   # a period needs the feed's state
    assert copy(ok, every=2, feed=z, capacity=0) == -1
    assert copy(ok, direction=1, feed=z) == -1 and copy(ok, direction=2) == -1
    assert copy(ok, segs_dev=None) == -1


def test_fingerprint_follows_name_dtype_and_size():
    from fmri_hip.state import fingerprint, segment_lines
    head = ["class=Stage1Step", "mode=vae-gan"]
    segs = [("group:encoder.data", "float32", 4096), ("opt:encoder.t", "int32", 4), ("feed", "int64", 24)]
    fp = fingerprint(head + segment_lines(segs))
    assert 0 <= fp < 2 ** 64 and fp == fingerprint(head + segment_lines(list(segs)))
    seen = {fp}
    for i, change in ((0, ("group:decoder.data", "float32", 4096)), (1, ("opt:encoder.t", "int64", 4)),
                      (2, ("feed", "int64", 32))):
        other = list(segs)
        other[i] = change
        seen.add(fingerprint(head + segment_lines(other)))
    seen.add(fingerprint(["class=Stage1Step", "mode=vae"] + segment_lines(segs)))
    seen.add(fingerprint(head + segment_lines(segs[:2])))
    seen.add(fingerprint(head + segment_lines([segs[1], segs[0], segs[2]])))
    assert len(seen) == 7


@pytest.mark.parametrize("every", [1, 2, 5])
@pytest.mark.parametrize("capacity", [1, 2, 3])
def test_slot_arithmetic_equals_the_epoch_loop(every, capacity):
    """``for idx_epoch in range(E): ...train...; if not idx_epoch % every: save`` keeps its k-th save in slot k % capacity;
    the step that sees it is the first of epoch idx_epoch + 1."""
    from fmri_hip.state import slot_of
    saves, want = 0, {}
    for idx_epoch in range(23):
        if not idx_epoch % every:
            want[idx_epoch + 1] = saves % capacity
            saves += 1
    for epoch in range(0, 24):
        assert slot_of(epoch, 0, every, capacity) == want.get(epoch), epoch
        assert slot_of(epoch, 4, every, capacity) is None
    assert slot_of(0, 0, every, capacity) is None and slot_of(1, 0, every, capacity) == 0


def _synthetic():
    from fmri_hip.state import TrainState, fingerprint
    g = torch.Generator().manual_seed(5)
    model = {"encoder.conv.weight": torch.randn(3, 5, generator=g),
             "encoder.bn.num_batches_tracked": torch.tensor(7, dtype=torch.int64)}
    model["encoder.conv.weight"][0, 0] = float("nan")                # bit for bit: a NaN payload survives too
    engine = {"opt:encoder.s1": torch.rand(17, generator=g), "opt:encoder.t": torch.tensor([3], dtype=torch.int32),
              "feed": torch.tensor([-(2 ** 63), 4, 8], dtype=torch.int64)}
    sig = ["class=Synthetic", "seg feed int64 24"]
    meta = dict(epoch=4, cursor=8, step=13, fingerprint=fingerprint(sig), signature=sig, host={"it": 2})
    return TrainState(model, engine, meta)


def _bits(t):
    return t.contiguous().view(torch.uint8).flatten() if t.dim() else t.reshape(1).view(torch.uint8)


def test_train_state_round_trips_bit_for_bit(tmp_path):
    from fmri_hip.state import FORMAT, TrainState
    st = _synthetic()
    path = tmp_path / "state.pt"
    st.save(path)
    raw = torch.load(path, weights_only=True)
    assert sorted(raw) == ["engine", "format", "meta", "model"] and raw["format"] == FORMAT == "fmri_hip.train_state/1"
    back = TrainState.load(path)
    assert (back.epoch, back.cursor, back.step, back.fingerprint) == (4, 8, 13, st.fingerprint)
    assert back.meta == st.meta
    for a, b in ((st.model, back.model), (st.engine, back.engine)):
        assert list(a) == list(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(_bits(a[k]), _bits(b[k])), k


def test_train_state_load_rejects_other_files(tmp_path):
    from fmri_hip.state import FORMAT, TrainState
    st = _synthetic()
    good = {"format": FORMAT, "model": st.model, "engine": st.engine, "meta": st.meta}
    cases = {"other format": dict(good, format="fmri_hip.train_state/0"), "no format": {k: v for k, v in good.items()
                                                                                        if k != "format"},
             "not a dict": [1, 2, 3]}
    for k in ("model", "engine", "meta"):
        cases["no " + k] = {n: v for n, v in good.items() if n != k}
    cases["meta without fingerprint"] = dict(good, meta={k: v for k, v in st.meta.items() if k != "fingerprint"})
    for what, blob in cases.items():
        path = tmp_path / "bad.pt"
        torch.save(blob, path)
        with pytest.raises(ValueError):
            TrainState.load(path)
            pytest.fail(what)
    path = tmp_path / "good.pt"
    torch.save(good, path)
    assert TrainState.load(path).step == 13
