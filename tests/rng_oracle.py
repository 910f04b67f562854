"""numpy restatement of the device generator (csrc/rng.hip; include/fmri_hip.h fmri_rng_normal): Philox4x32-10 on uint64
arrays, the uniform map and Box-Muller in float64, and the (seed, offset, global row, column, stream id) -> number layout.
Not a test: tests/test_rng_host.py pins it against the Random123 known answers, tests/test_rng_gpu.py the kernels against it."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: 4 arrays (or ints) of 32-bit words, key: 2 -> 4 uint64 arrays holding the 32-bit output words."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in ctr]
    k = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in key]
    m32, s32 = np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]          # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & m32, (p0 >> s32) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(W0)) & m32, (k[1] + np.uint64(W1)) & m32]
    return c


def words(seed, offset, first, n, sid):
    """Output words of elements first .. first + n of stream ``sid``: element e is word e % 4 of block offset + e // 4."""
    e = np.arange(n, dtype=np.uint64) + np.uint64(first)
    blk0 = int(first) // 4
    nblk = (int(first) + n - 1) // 4 - blk0 + 1
    # 64-bit counter with wrap-around, built from Python ints (numpy would warn on the overflow)
    ctr = np.array([(int(offset) + blk0 + i) & 0xFFFFFFFFFFFFFFFF for i in range(nblk)], dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    out = philox4x32_10((ctr & np.uint64(MASK), ctr >> np.uint64(32), np.full(nblk, sid, np.uint64),
                         np.zeros(nblk, np.uint64)), (seed & MASK, seed >> 32))
    w = np.stack(out, axis=1)              # [nblk, 4]
    bi = (e // np.uint64(4) - np.uint64(blk0)).astype(np.int64)
    return w, bi, (e % np.uint64(4)).astype(np.int64)


def uniform(w):
    return ((w >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def normal(seed, offset, rows, cols, row0=0, sid=0, scale=1.0):
    """float64 [rows, cols]: what fmri_rng_normal computes in fp32."""
    w, bi, wi = words(seed, offset, int(row0) * cols, rows * cols, sid)
    u = uniform(w)
    ra = np.sqrt(-2.0 * np.log(u[:, [0, 2]]))
    ang = 2.0 * np.pi * u[:, [1, 3]]
    z = np.empty(w.shape, np.float64)
    z[:, 0::2] = ra * np.cos(ang)
    z[:, 1::2] = ra * np.sin(ang)
    return (scale * z[bi, wi]).reshape(rows, cols)


def raw_words(seed, offset, n, sid):
    w, bi, wi = words(seed, offset, 0, n, sid)
    return w[bi, wi]


def integers(seed, offset, n, lo, hi, sid):
    """int64 [n] in [lo, hi]: lo + ((w * (hi - lo + 1)) >> 32)."""
    w = raw_words(seed, offset, n, sid)
    return (w * np.uint64(hi - lo + 1) >> np.uint64(32)).astype(np.int64) + lo
