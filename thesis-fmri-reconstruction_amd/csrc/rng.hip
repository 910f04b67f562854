// Counter-based random numbers for the fused steps: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as
// 1, 2, 3", SC 2011; the Random123 constants), the latent noise (eps, z_p, z_fake) and the augmentation draws of
// fmri_ingest_u8 made on the device (include/fmri_hip.h fmri_rng_normal for the counter layout).
//
//   rng_normal_kernel   thread t owns Philox block b0 + t of the draw: one Philox call, two Box-Muller pairs, and the up
//                       to four elements of the block that fall inside the caller's rows -- one 16-byte store when all
//                       four lie in one row at an aligned address, single stores otherwise (first / last block of a draw
//                       whose row0 * cols is no multiple of 4, rows with cols % 4 != 0, ld % 4 != 0).
//   rng_u32_kernel      thread t owns block start / 4 + t: four words mapped to [lo, hi] by multiply-high; the elements
//                       start .. start + n - 1 of the stream (a rank's slice of the flip / shift draws) land at out[0 ..].
//   rng_advance_kernel  offset += nblocks, one thread, a plain store.
//   sampler_*_kernel    the epoch sampler of the device-resident dataset (fmri_hip/feed.py): a keyed bijection of [0, N)
//                       evaluated per index, and its [seed, epoch, cursor] state machine (below).
//
// The state [seed, offset] is read from device memory by every thread (two scalar loads): the host never knows the
// offset, so a step recorded into a HIP graph draws fresh numbers at every replay.  A number depends on (seed, offset,
// global row, column, stream id) only -- not on the launch shape, the rank or the vector / scalar store path.
#include "kernels.h"
#include "philox.h"

namespace fmri {

namespace {

// e0 = row0 * cols: first global element of the caller's rows; n = rows * cols (< 2^31); b0 = e0 / 4
__global__ __launch_bounds__(256) void rng_normal_kernel(const int64_t* __restrict__ state, float* __restrict__ out,
                                                         uint64_t e0, uint32_t n, uint64_t b0, uint32_t nblk,
                                                         uint32_t cols, uint32_t ld, uint32_t sid, float scale,
                                                         int vec_ok) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nblk) return;
    const uint64_t blk = b0 + t;
    const u32x4 x = rng_block(state, blk, sid);
    float z[4];
    box_muller(x.w[0], x.w[1], scale, z[0], z[1]);
    box_muller(x.w[2], x.w[3], scale, z[2], z[3]);
    // local index of the block's first element; "negative" (wraps) only for the first block when e0 % 4 != 0
    const int64_t l0 = (int64_t)(4 * blk - e0);
    if (l0 >= 0 && l0 + 3 < (int64_t)n) {
        const uint32_t l = (uint32_t)l0, r = l / cols, c = l - r * cols;
        const uint64_t at = (uint64_t)r * ld + c;
        if (vec_ok && c + 3 < cols && (at & 3) == 0) {
            *(float4*)(out + at) = make_float4(z[0], z[1], z[2], z[3]);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t lk = l0 + k;
        if (lk < 0 || lk >= (int64_t)n) continue;
        const uint32_t l = (uint32_t)lk, r = l / cols, c = l - r * cols;
        out[(uint64_t)r * ld + c] = z[k];
    }
}

// element e = start + i of the stream goes to out[i]; b0 = start / 4.  Thread t owns block b0 + t, as in rng_normal_kernel
__global__ __launch_bounds__(256) void rng_u32_kernel(const int64_t* __restrict__ state, int32_t* __restrict__ out,
                                                      uint64_t n, uint64_t start, uint64_t b0, uint64_t nblk,
                                                      uint32_t sid, int64_t lo, uint64_t span) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= nblk) return;
    const u32x4 x = rng_block(state, b0 + t, sid);
    int32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (int32_t)(lo + (int64_t)(((uint64_t)x.w[k] * span) >> 32));
    // local index of the block's first element; negative only for the first block when start % 4 != 0
    const int64_t l0 = (int64_t)(4 * (b0 + t) - start);
    if (l0 >= 0 && l0 + 3 < (int64_t)n && ((uintptr_t)(out + l0) & 15) == 0) {
        *(int4*)(out + l0) = make_int4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (l0 + k >= 0 && l0 + k < (int64_t)n) out[l0 + k] = v[k];
}

__global__ void rng_advance_kernel(int64_t* state, int64_t nblocks) {
    if (threadIdx.x == 0 && blockIdx.x == 0) state[1] = (int64_t)((uint64_t)state[1] + (uint64_t)nblocks);
}

// ---- epoch sampler (include/fmri_hip.h fmri_sampler_indices for the construction) --------------------------------------
// pi(seed, epoch) on [0, N): a balanced Feistel network over 2k bits, cycle-walked into [0, N).  The domain 2^(2k) is
// below 4 N, so a walk takes fewer than 4 network passes on average; one thread per index, SAMPLER_ROUNDS Philox blocks
// per pass -- a few hundred blocks for a batch of 256, against ~8 k for one [256, 128] noise draw.
constexpr uint32_t SID_PERM = 16;
constexpr int SAMPLER_ROUNDS = 6;

__device__ __forceinline__ uint32_t sampler_pi(uint64_t seed, uint64_t epoch, uint32_t i, uint32_t N) {
    if (N <= 1) return 0;
    const int bits = 32 - __clz((int)(N - 1));          // N - 1 >= 1
    const int k = (bits + 1) / 2;                       // 1 .. 16
    const uint32_t mask = (1u << k) - 1u;
    const uint32_t c1 = (uint32_t)epoch, c3 = 0x80000000u | (uint32_t)(epoch >> 32);
    uint32_t x = i;
    do {
        uint32_t L = x >> k, R = x & mask;
        for (int r = 0; r < SAMPLER_ROUNDS; ++r) {
            const u32x4 f = philox4x32_10(((uint32_t)r << 16) | R, c1, SID_PERM, c3, (uint32_t)seed,
                                          (uint32_t)(seed >> 32));
            const uint32_t t = L ^ (f.w[0] & mask);
            L = R;
            R = t;
        }
        x = (L << k) | R;
    } while (x >= N);
    return x;
}

__global__ __launch_bounds__(256) void sampler_indices_kernel(const int64_t* __restrict__ state, uint32_t N, uint32_t B,
                                                              uint64_t row0, int32_t* __restrict__ idx) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= B) return;
    const uint64_t seed = (uint64_t)state[0], epoch = (uint64_t)state[1];
    const uint64_t pos = ((uint64_t)state[2] + row0 + t) % N;       // (a position past the epoch's end wraps: in bounds)
    idx[t] = (int32_t)sampler_pi(seed, epoch, (uint32_t)pos, N);
}

__global__ void sampler_advance_kernel(int64_t* state, int64_t N, int64_t Bg) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t cur = state[2] + Bg;
    if (N - cur < Bg) {                                  // fewer than a global batch left: the tail is dropped
        state[1] = state[1] + 1;
        state[2] = 0;
    } else {
        state[2] = cur;
    }
}

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? OK : E_LAUNCH)

}  // namespace

int rng_normal_launch(const int64_t* state, float* out, int rows, int cols, int ld, int64_t row0, int sid, float scale,
                      hipStream_t st) {
    const int64_t n = (int64_t)rows * cols;
    // one thread per Philox block with 32-bit local indices; global rows up to 2^40 keep (row0 + rows) * cols in 64 bits
    if (n > INT32_MAX || row0 > (1ll << 40)) return E_UNSUPPORTED;
    const uint64_t e0 = (uint64_t)row0 * (uint64_t)cols, e1 = e0 + (uint64_t)n;
    const uint64_t b0 = e0 / 4, b1 = (e1 - 1) / 4;
    const uint32_t nblk = (uint32_t)(b1 - b0 + 1);
    hipLaunchKernelGGL(rng_normal_kernel, dim3((nblk + 255) / 256), dim3(256), 0, st, state, out, e0, (uint32_t)n, b0,
                       nblk, (uint32_t)cols, (uint32_t)ld, (uint32_t)sid, scale, ((uintptr_t)out & 15) == 0 ? 1 : 0);
    return LAUNCH_OK();
}

int rng_u32_launch(const int64_t* state, int32_t* out, int64_t n, int64_t start, int sid, int lo, int hi,
                   hipStream_t st) {
    // 2^31 - 1 thread blocks of 1024 numbers at most; start + n stays far inside 64 bits
    if (n > (1ll << 40) || start > (1ll << 40)) return E_UNSUPPORTED;
    const uint64_t b0 = (uint64_t)start / 4, b1 = ((uint64_t)start + (uint64_t)n - 1) / 4;
    const uint64_t nblk = b1 - b0 + 1;
    hipLaunchKernelGGL(rng_u32_kernel, dim3((uint32_t)((nblk + 255) / 256)), dim3(256), 0, st, state, out, (uint64_t)n,
                       (uint64_t)start, b0, nblk, (uint32_t)sid, (int64_t)lo, (uint64_t)((int64_t)hi - (int64_t)lo + 1));
    return LAUNCH_OK();
}

int rng_advance_launch(int64_t* state, int64_t nblocks, hipStream_t st) {
    hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(64), 0, st, state, nblocks);
    return LAUNCH_OK();
}

int sampler_indices_launch(const int64_t* state, int N, int B, int64_t row0, int32_t* idx, hipStream_t st) {
    hipLaunchKernelGGL(sampler_indices_kernel, dim3(((uint32_t)B + 255) / 256), dim3(256), 0, st, state, (uint32_t)N,
                       (uint32_t)B, (uint64_t)row0, idx);
    return LAUNCH_OK();
}

int sampler_advance_launch(int64_t* state, int64_t N, int64_t B_global, hipStream_t st) {
    hipLaunchKernelGGL(sampler_advance_kernel, dim3(1), dim3(64), 0, st, state, N, B_global);
    return LAUNCH_OK();
}

}  // namespace fmri
