"""numpy restatement of the epoch sampler (csrc/rng.hip; include/fmri_hip.h fmri_sampler_indices), written from the header:
the keyed bijection pi(seed, epoch) of [0, N) -- a six-round balanced Feistel network over 2k bits whose round function is
one Philox4x32-10 block, cycle-walked into [0, N) -- and the [seed, epoch, cursor] state machine with drop-last batches.
Not a test: tests/test_sampler_host.py pins it, tests/test_feed_gpu.py the kernels against it."""
import numpy as np

from rng_oracle import philox4x32_10

SID_PERM = 16
ROUNDS = 6
M64 = (1 << 64) - 1


def _network(x, k, seed, epoch):
    """One pass of the Feistel network over the uint64 array ``x`` (values below 2^(2k))."""
    mask = np.uint64((1 << k) - 1)
    kk = np.uint64(k)
    seed, epoch = int(seed) & M64, int(epoch) & M64
    L, R = x >> kk, x & mask
    c1 = np.full(x.shape, epoch & 0xFFFFFFFF, np.uint64)
    c2 = np.full(x.shape, SID_PERM, np.uint64)
    c3 = np.full(x.shape, 0x80000000 | (epoch >> 32), np.uint64)
    for r in range(ROUNDS):
        f = philox4x32_10((np.uint64(r << 16) | R, c1, c2, c3), (seed & 0xFFFFFFFF, seed >> 32))[0]
        L, R = R, L ^ (f & mask)
    return (L << kk) | R


def pi(seed, epoch, i, N):
    """pi(seed, epoch)(i) for an int or an array of positions ``i`` in [0, N) -> int64 array."""
    i = np.atleast_1d(np.asarray(i, dtype=np.int64))
    assert N >= 1 and i.min() >= 0 and i.max() < N
    if N == 1:
        return np.zeros(i.shape, np.int64)
    k = ((N - 1).bit_length() + 1) // 2
    x = i.astype(np.uint64)
    todo = np.ones(x.shape, bool)
    while todo.any():                      # cycle walking: only the values still outside [0, N) take another pass
        x[todo] = _network(x[todo], k, seed, epoch)
        todo = x >= np.uint64(N)
    return x.astype(np.int64)


class Sampler:
    """The state machine of fmri_sampler_indices / fmri_sampler_advance."""

    def __init__(self, seed, N, epoch=0, cursor=0):
        self.seed, self.N, self.epoch, self.cursor = seed, N, epoch, cursor

    def indices(self, B, row0=0):
        pos = (self.cursor + row0 + np.arange(B, dtype=np.int64)) % self.N
        return pi(self.seed, self.epoch, pos, self.N)

    def advance(self, B_global):
        assert B_global <= self.N
        self.cursor += B_global
        if self.N - self.cursor < B_global:
            self.epoch += 1
            self.cursor = 0

    def next(self, B_global):
        """The global batch and the advance behind it."""
        idx = self.indices(B_global)
        self.advance(B_global)
        return idx
