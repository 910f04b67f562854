"""The many-segment copy of the training-state ring alone (csrc/state.hip, fmri_state_copy) on seeded random bytes, against
numpy: every payload byte, and every byte that must NOT change -- the padding between segments, a canary slot in front of
and behind the ring, 64 canary bytes behind every live tensor.

Segment sizes cover an empty segment, sizes below one 16-byte access, dword tails, one chunk (16 KiB) minus / plus one
dword and a segment of 65 chunks; every size is tried at a live address that is 16-byte aligned and at +4 and +8 from it
(the dword path).  Several small segments share the chunk numbering with the large ones, so the block -> segment search
is exercised in front of, between and behind multi-chunk segments."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KIB = 1024
SIZES = [0, 4, 12, 16, 20, 60, 64, 16 * KIB - 4, 16 * KIB, 16 * KIB + 4, 1024 * KIB + 12]
CANARY = 64
MAGIC = 0x31544154534d4621
FP = 0xF1E2D3C4B5A69788                                       # a fingerprint with the top bit set


class Rig:
    """Live tensors carved out of one arena (segment i at a 256-byte boundary + 4 * ((i + rot) % 3), 64 canary bytes behind
    it), the table on both sides, and a ring of capacity + 1 slots with one more slot of canary bytes on either side."""

    def __init__(self, sizes, rot, capacity=2, seed=0):
        from fmri_hip import lib, state
        self.L, self.lib = lib, lib.load()
        self.sizes, self.capacity = list(sizes), capacity
        self.rs = np.random.RandomState(seed)
        self.slot_bytes, self.offs = state.layout(self.sizes)
        self.at, end = [], 0
        for i, n in enumerate(self.sizes):
            self.at.append(end + 4 * ((i + rot) % 3))
            end = -(-(self.at[-1] + n + CANARY) // 256) * 256
        self.arena = torch.zeros(max(end, 256), dtype=torch.uint8, device=DEV)
        assert self.arena.data_ptr() % 256 == 0
        self.table = (lib.StateSeg * max(len(self.sizes), 1))()
        chunks = 0
        for row, a, o, n in zip(self.table, self.at, self.offs, self.sizes):
            row.live, row.offset, row.bytes, row.chunk0 = self.arena.data_ptr() + a, o, n, chunks
            chunks += -(-n // lib.STATE_CHUNK)
        self.chunks = chunks
        self.table_dev = torch.frombuffer(bytearray(bytes(self.table)), dtype=torch.uint8).to(DEV)
        self.ring_all = torch.zeros((capacity + 3) * self.slot_bytes, dtype=torch.uint8, device=DEV)
        self.ring = self.ring_all[self.slot_bytes:(capacity + 2) * self.slot_bytes]
        assert self.ring.data_ptr() % 16 == 0
        self.feed = torch.zeros(3, dtype=torch.int64, device=DEV)
        self.counter = torch.full((1,), 41, dtype=torch.int64, device=DEV)

    def randomize(self, t):
        t.copy_(torch.from_numpy(self.rs.randint(0, 256, t.numel(), dtype=np.uint8)))

    def copy(self, direction=0, feed=None, every=0, counter=True, table=None, nseg=None):
        """Returns the entry point's code; ``feed``: (epoch, cursor) or None for feed_state = NULL."""
        if feed is not None:
            self.feed.copy_(torch.tensor([1234, feed[0], feed[1]], dtype=torch.int64))
        code = self.lib.fmri_state_copy(
            self.table if table is None else table, self.table_dev.data_ptr(), len(self.sizes) if nseg is None else nseg,
            self.ring.data_ptr(), self.ring.numel(), self.slot_bytes, direction,
            self.feed.data_ptr() if feed is not None else None, every, self.capacity, FP,
            self.counter.data_ptr() if counter else None, self.L.stream())
        torch.cuda.synchronize()
        return code

    def host(self):
        return self.arena.cpu().numpy(), self.ring_all.cpu().numpy()

    def expect_gather(self, arena, ring_all, slot, epoch, cursor, step):
        """numpy: ``ring_all`` after a firing gather of ``arena`` into ``slot``."""
        want = ring_all.copy()
        base = (slot + 1) * self.slot_bytes
        want[base:base + 64].view(np.int64)[:] = [MAGIC, np.uint64(FP).astype(np.int64), epoch, cursor, step,
                                                  self.slot_bytes - 64, 0, 0]
        for a, o, n in zip(self.at, self.offs, self.sizes):
            want[base + o:base + o + n] = arena[a:a + n]
        return want


@pytest.fixture(scope="module", params=[0, 1, 2])
def rig(request):
    r = Rig(SIZES, request.param, seed=request.param)
    aligned = [a % 16 == 0 for a in r.at]
    assert any(aligned) and not all(aligned) and r.chunks == 6 + 1 + 1 + 2 + 65      # six small non-empty segments
    return r


def test_gather_moves_every_payload_byte_and_nothing_else(rig):
    rig.randomize(rig.arena)
    rig.randomize(rig.ring_all)
    arena, ring = rig.host()
    assert rig.copy(0, feed=None) == 0                          # feed_state = NULL: the manual slot, position -1
    arena2, ring2 = rig.host()
    assert np.array_equal(arena2, arena)
    want = rig.expect_gather(arena, ring, rig.capacity, -1, -1, 41)
    assert np.array_equal(ring2, want), np.flatnonzero(ring2 != want)[:8]
    # the manual slot only: the ring's own slots, the padding and both canary slots are the random bytes they were
    lo, hi = (rig.capacity + 1) * rig.slot_bytes, (rig.capacity + 2) * rig.slot_bytes
    assert np.array_equal(ring2[:lo], ring[:lo]) and np.array_equal(ring2[hi:], ring[hi:])
    assert not np.array_equal(ring2[lo:hi], ring[lo:hi])


def test_scatter_reproduces_the_live_tensors(rig):
    rig.randomize(rig.arena)
    rig.randomize(rig.ring_all)
    live = torch.zeros_like(rig.arena, dtype=torch.bool)
    for a, n in zip(rig.at, rig.sizes):
        live[a:a + n] = True
    rig.arena[live] = 0                                         # zeroed live tensors, random canaries around them
    arena, ring = rig.host()
    assert rig.copy(1, feed=None, counter=False) == 0
    arena2, ring2 = rig.host()
    assert np.array_equal(ring2, ring)
    want = arena.copy()
    base = (rig.capacity + 1) * rig.slot_bytes                  # dir = 1 reads slot `capacity`
    for a, o, n in zip(rig.at, rig.offs, rig.sizes):
        want[a:a + n] = ring[base + o:base + o + n]
    assert np.array_equal(arena2, want), np.flatnonzero(arena2 != want)[:8]
    keep = ~live.cpu().numpy()
    assert np.array_equal(arena2[keep], arena[keep])            # the bytes behind (and between) the live tensors


def test_gather_then_scatter_is_the_identity(rig):
    rig.randomize(rig.arena)
    arena, _ = rig.host()
    assert rig.copy(0, feed=None) == 0
    for a, n in zip(rig.at, rig.sizes):
        rig.arena[a:a + n] = 0
    assert rig.copy(1, feed=None, counter=False) == 0
    assert np.array_equal(rig.host()[0], arena)


def test_predicate_and_slots(rig):
    """every = 2, capacity = 2: the launch copies at the first step of epochs 1, 3, 5 -- the ends of epochs 0, 2, 4 -- into
    slots 0, 1, 0, and changes no byte of the ring at any other position."""
    rig.randomize(rig.ring_all)
    for epoch, cursor in ((0, 0), (1, 4), (2, 0), (4, 0)):
        rig.randomize(rig.arena)
        _, ring = rig.host()
        assert rig.copy(0, feed=(epoch, cursor), every=2) == 0
        assert np.array_equal(rig.host()[1], ring), (epoch, cursor)
    for (epoch, cursor), slot in (((1, 0), 0), ((3, 0), 1), ((5, 0), 0)):
        rig.randomize(rig.arena)
        arena, ring = rig.host()
        assert rig.copy(0, feed=(epoch, cursor), every=2) == 0
        want = rig.expect_gather(arena, ring, slot, epoch, cursor, 41)
        got = rig.host()[1]
        assert np.array_equal(got, want), (epoch, slot, np.flatnonzero(got != want)[:8])
        head = got[(slot + 1) * rig.slot_bytes:][:64].view(np.int64)
        assert (head[2], head[3]) == (epoch, cursor)
    # every = 0 with a feed state: unconditional, the manual slot, the header carries the feed's position; no log: -1
    arena, ring = rig.host()
    assert rig.copy(0, feed=(2, 8), every=0, counter=False) == 0
    assert np.array_equal(rig.host()[1], rig.expect_gather(arena, ring, rig.capacity, 2, 8, -1))


def test_an_empty_table_writes_the_header_only():
    r = Rig([], 0, capacity=1)
    assert r.slot_bytes == 64 and r.chunks == 0
    r.randomize(r.ring_all)
    _, ring = r.host()
    assert r.copy(0, feed=None) == 0
    want = r.expect_gather(None, ring, 1, -1, -1, 41)
    assert np.array_equal(r.host()[1], want)
    assert r.copy(0, feed=(1, 0), every=1) == 0
    assert np.array_equal(r.host()[1], r.expect_gather(None, want, 0, 1, 0, 41))


def test_misaligned_tables_are_refused_without_a_launch(rig):
    from fmri_hip import lib
    rig.randomize(rig.arena)
    rig.randomize(rig.ring_all)
    arena, ring = rig.host()
    n = len(SIZES)

    def broken(i, **change):
        tab = (lib.StateSeg * n)()
        ctypes.memmove(tab, rig.table, ctypes.sizeof(tab))
        for k, v in change.items():
            setattr(tab[i], k, v)
        return tab
    big = n - 1
    cases = [broken(big, live=rig.table[big].live + 2),          # live address not a multiple of 4
             broken(big, live=rig.table[big].live + 1),
             broken(big, bytes=rig.table[big].bytes - 2),        # byte count not a multiple of 4
             broken(3, bytes=18),
             broken(big, offset=rig.table[big].offset + 8),      # slot offset not a multiple of 16
             broken(big, offset=rig.table[big].offset + 16),     # behind the end of the slot
             broken(big, chunk0=rig.table[big].chunk0 + 1)]
    for direction in (0, 1):
        for tab in cases:
            assert rig.copy(direction, feed=None, counter=False, table=tab) == -1
    a2, r2 = rig.host()
    assert np.array_equal(a2, arena) and np.array_equal(r2, ring)
