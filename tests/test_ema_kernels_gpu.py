"""The two kernels of the weight average alone (csrc/ema.hip: fmri_ema_update, fmri_ema_swap) on seeded values.

One table covers, in ONE launch: segments of 0, 1, 3, 4, 5, 1023, 4096, 4097 and 3 * 4096 + 2 floats with both bases 16-byte
aligned (a chunk is 4096 floats: below, at and above one chunk, dword tails of 1, 2 and 3), one segment whose live base is
offset by one float and one whose shadow base is (the dword path), all carved from two arenas -- one for the live side, one
for the shadows -- with 64 guard words between segments that must keep their fill pattern."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import ema_oracle as EO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
GUARD_BITS = 0x7FC0BEEF                                       # a NaN with a payload: an update that touched it would show
CH = 4096
# (floats, live base offset in floats, shadow base offset in floats)
SEGS = [(0, 0, 0), (1, 0, 0), (3, 0, 0), (4, 0, 0), (5, 0, 0), (1023, 0, 0), (CH, 0, 0), (CH + 1, 0, 0), (3 * CH + 2, 0, 0),
        (2 * CH + 7, 1, 0), (CH + 5, 0, 1), (0, 0, 0), (9, 1, 1)]
CONFIGS = [(0.999, True, 0), (0.999, True, 3), (0.5, False, 0), (0.0, False, 0)]
STEPS = 13                                                    # t = 0..12


class Rig:
    def __init__(self):
        from fmri_hip import lib
        self.L, self.lib = lib, lib.load()
        self.at_live, self.at_shadow, end_l, end_s = [], [], GUARD, GUARD
        for n, ol, os_ in SEGS:
            self.at_live.append(end_l + ol)
            self.at_shadow.append(end_s + os_)
            end_l = -(-(self.at_live[-1] + n + GUARD) // 4) * 4      # the next base: 16-byte aligned, >= 64 words on
            end_s = -(-(self.at_shadow[-1] + n + GUARD) // 4) * 4
        self.live = torch.zeros(end_l, dtype=torch.int32, device=DEV)
        self.shadow = torch.zeros(end_s, dtype=torch.int32, device=DEV)
        assert self.live.data_ptr() % 16 == 0 and self.shadow.data_ptr() % 16 == 0
        self.table = (lib.EmaSeg * len(SEGS))()
        chunks = 0
        for row, (n, _, _), a, b in zip(self.table, SEGS, self.at_live, self.at_shadow):
            row.live, row.shadow = self.live.data_ptr() + 4 * a, self.shadow.data_ptr() + 4 * b
            row.n, row.chunk0 = n, chunks
            chunks += -(-n // lib.EMA_CHUNK)
        assert chunks == 5 + 1 + 2 + 4 + 3 + 2 + 1
        self.table_dev = torch.frombuffer(bytearray(bytes(self.table)), dtype=torch.uint8).to(DEV)
        self.state = torch.zeros(4, dtype=torch.int32, device=DEV)
        self.mask_live = self._mask(self.live.numel(), self.at_live)
        self.mask_shadow = self._mask(self.shadow.numel(), self.at_shadow)

    @staticmethod
    def _mask(total, at):
        m = np.zeros(total, dtype=bool)
        for (n, _, _), a in zip(SEGS, at):
            m[a:a + n] = True
        return m

    def fill(self, arena, mask, bits):
        """``bits``: int32 payload for the segments' words, in arena order; everything else is the guard pattern."""
        host = np.full(mask.size, GUARD_BITS, dtype=np.int64).astype(np.uint32).view(np.int32)
        host[mask] = bits
        arena.copy_(torch.from_numpy(host))
        return host

    def set_state(self, t, start, decay, warmup):
        bits = struct.unpack("<i", struct.pack("<f", decay))[0]
        self.state.copy_(torch.tensor([t, start, bits, 1 if warmup else 0], dtype=torch.int32))

    def update(self):
        code = self.lib.fmri_ema_update(C.cast(self.table, C.c_void_p), self.table_dev.data_ptr(), len(SEGS),
                                        self.state.data_ptr(), self.L.stream())
        assert code == 0
        code = self.lib.fmri_counter_inc(self.state.data_ptr(), self.L.stream())
        assert code == 0

    def swap(self):
        assert self.lib.fmri_ema_swap(C.cast(self.table, C.c_void_p), self.table_dev.data_ptr(), len(SEGS),
                                      self.L.stream()) == 0


@pytest.fixture(scope="module")
def rig():
    return Rig()


def _normal_bits(rs, n, scale=1.0):
    return (rs.standard_normal(n) * scale).astype(np.float32).view(np.int32)


@pytest.mark.parametrize("decay,warmup,start", CONFIGS)
def test_update_is_the_fp32_oracle_bit_for_bit_and_within_the_f64_bound(rig, decay, warmup, start):
    """t = 0..12 successive launches with the counter increment between them; fresh live values in front of every launch.
    After every launch every word of both arenas is compared: the shadows' words with the numpy fp32 oracle as int32, the
    live words and all guard words with what they were.  At the end the shadows against the exact float64 recurrence:
    |e_gpu - e_f64| <= 4 k 2^-24 M after k launches, M the largest |w| or |e| fed in -- two fp32 roundings in w - e and
    the sum, one in the product, each at most 2^-24 M because the result is a convex combination of values below M (the
    difference is at most 2 M, times omd <= 1: counted twice), earlier error contracted by d <= 1."""
    rs = np.random.RandomState(int(decay * 1e4) + 7 * start + warmup)
    n_live, n_sh = int(rig.mask_live.sum()), int(rig.mask_shadow.sum())
    assert n_live == n_sh == sum(n for n, _, _ in SEGS)
    sh_host = rig.fill(rig.shadow, rig.mask_shadow, _normal_bits(rs, n_sh))
    e32 = sh_host[rig.mask_shadow].view(np.float32).copy()
    e64 = e32.astype(np.float64)
    M = float(np.abs(e32).max())
    rig.set_state(0, start, decay, warmup)
    # the shadows' payload in LIVE arena order and back: segment i of either arena holds the same elements
    for t in range(STEPS):
        live_host = rig.fill(rig.live, rig.mask_live, _normal_bits(rs, n_live))
        w32 = live_host[rig.mask_live].view(np.float32)
        M = max(M, float(np.abs(w32).max()))
        rig.update()
        d = EO.decay_at(t, start, decay, warmup)
        e32 = EO.update(e32, w32, d)
        e64 = EO.update_f64(e64, w32, d)
        want = sh_host.copy()
        want[rig.mask_shadow] = e32.view(np.int32)
        got_sh, got_live = rig.shadow.cpu().numpy(), rig.live.cpu().numpy()
        assert np.array_equal(got_live, live_host), (t, np.flatnonzero(got_live != live_host)[:8])
        assert torch.equal(torch.from_numpy(got_sh), torch.from_numpy(want)), (t, np.flatnonzero(got_sh != want)[:8])
        sh_host = want
    assert rig.state.tolist()[0] == STEPS
    got = rig.shadow.cpu().numpy()[rig.mask_shadow].view(np.float32).astype(np.float64)
    err, bound = float(np.abs(got - e64).max()), 4 * STEPS * 2.0 ** -24 * M
    print(f"ema update decay={decay} warmup={warmup} start={start}: err/bound {err:.3g}/{bound:.3g} = {err / bound:.3f}")
    assert err <= bound


def _special_bits(rs, n):
    """Random 32-bit words with NaNs of many payloads, both infinities, zeros of both signs and denormals among them."""
    bits = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    k = n // 8
    bits[0 * k:1 * k] |= 0x7FC00000                           # quiet NaNs, random payloads and signs
    bits[1 * k:2 * k] = (bits[1 * k:2 * k] & 0x803FFFFF) | 0x7F800001      # signalling NaNs
    bits[2 * k:2 * k + 4] = [0x7F800000, 0xFF800000, 0x00000000, 0x80000000]
    bits[3 * k:4 * k] &= 0x807FFFFF                           # denormals
    rs.shuffle(bits)
    return bits.view(np.int32)


def test_swap_exchanges_every_word_and_two_swaps_are_the_identity(rig):
    rs = np.random.RandomState(99)
    n = int(rig.mask_live.sum())
    live0 = rig.fill(rig.live, rig.mask_live, _special_bits(rs, n))
    sh0 = rig.fill(rig.shadow, rig.mask_shadow, _special_bits(rs, n))
    assert not np.array_equal(live0[rig.mask_live], sh0[rig.mask_shadow])
    rig.swap()
    live1, sh1 = rig.live.cpu().numpy(), rig.shadow.cpu().numpy()
    want_l, want_s = live0.copy(), sh0.copy()
    want_l[rig.mask_live] = sh0[rig.mask_shadow]
    want_s[rig.mask_shadow] = live0[rig.mask_live]
    assert np.array_equal(live1, want_l), np.flatnonzero(live1 != want_l)[:8]      # payload exchanged, guards intact
    assert np.array_equal(sh1, want_s), np.flatnonzero(sh1 != want_s)[:8]
    rig.swap()
    assert np.array_equal(rig.live.cpu().numpy(), live0) and np.array_equal(rig.shadow.cpu().numpy(), sh0)
