// Augmentation of the fMRI rows of the Stage-II / Stage-III steps (include/fmri_hip.h fmri_voxaug_apply for the formula
// and the counter layout; fmri_hip/voxaug.py): trial noise, voxel dropout, a masked span of voxels, gain jitter.
//
//   voxaug_params_kernel  thread b owns table row b = global row row0 + b: ONE Philox block (block row0 + b of the row
//                         stream) -> gain, span start, the apply decision; k = 1 / (1 - p) is computed here, once.
//   voxaug_apply_kernel   gather_rows_kernel's shape (csrc/ingest.hip): one thread per 8 columns of a row, two 16-byte
//                         loads (V % 4 == 0 and aligned rows; single loads otherwise), one 16-byte fp16 store, optionally
//                         the fp32 result, a grid-stride loop.  The thread's elements e0 .. e0 + 7 (e0 = (row0 + b) V + c0)
//                         of the noise and of the dropout stream lie in Philox blocks e0 / 4 .. : two per stream, three
//                         when e0 % 4 != 0, fewer at the end of a row -- exactly those are evaluated, and none of a
//                         stream whose parameter is zero in the row (sigma == 0: no noise block, p == 0: no dropout block).
//
// State and table are read from device memory: the launches sit in a recorded step and draw fresh numbers at every replay.
// A value depends on (seed, offset, global row, column, stream id) only -- not on the launch shape, the vector / scalar
// path or the rank.  The normal is box_muller of csrc/philox.h, the definition rng_normal_kernel uses: element for
// element the number fmri_rng_normal gives for (rows, cols = V, row0) at the same offset.
#include "kernels.h"
#include "philox.h"

namespace fmri {

namespace {

// (uint32)((double)q * 2^32) for 0 <= q < 1: the threshold a raw word is compared with -- an integer comparison
__device__ __forceinline__ uint32_t prob_threshold(float q) { return (uint32_t)((double)q * 4294967296.0); }

__global__ __launch_bounds__(256) void voxaug_params_kernel(const int64_t* __restrict__ state, float* __restrict__ table,
                                                            int rows, uint64_t row0, uint32_t sid, uint32_t V, float gain,
                                                            float sigma, float p, int rescale, uint32_t L, float prob) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= rows) return;
    const u32x4 w = rng_block(state, row0 + (uint64_t)b, sid);
    float4 t0 = make_float4(1.f, 0.f, 0.f, 1.f), t1 = make_float4(0.f, 0.f, 0.f, 0.f);       // the neutral row
    if (prob >= 1.f || w.w[3] < prob_threshold(prob)) {
        float z0, z1;
        box_muller(w.w[0], w.w[1], 1.f, z0, z1);
        t0.x = fmaf(gain, z0, 1.f);
        t0.y = sigma;
        t0.z = p;
        t0.w = rescale ? 1.f / (1.f - p) : 1.f;
        t1.x = (float)__umulhi(w.w[2], V - L + 1u);
        t1.y = (float)L;
    }
    *(float4*)(table + 8 * (int64_t)b) = t0;
    *(float4*)(table + 8 * (int64_t)b + 4) = t1;
}

// word / normal j (0 <= j < 8) of a thread's elements out of the up to 12 of its blocks, which start `sh` words earlier:
// selects over compile-time indices (a run-time index would put the array into scratch memory)
template <typename T>
__device__ __forceinline__ T pick(const T (&a)[12], int j, uint32_t sh) {
    return sh == 0 ? a[j] : (sh == 1 ? a[j + 1] : (sh == 2 ? a[j + 2] : a[j + 3]));
}

template <bool VEC>
__global__ __launch_bounds__(256) void voxaug_apply_kernel(const float* __restrict__ src, int V, int Vp, int B,
                                                           const float* __restrict__ table,
                                                           const int64_t* __restrict__ state, uint64_t row0,
                                                           uint32_t sid_noise, uint32_t sid_drop,
                                                           half_t* __restrict__ dst16, float* __restrict__ dst32) {
    const int chunks = Vp / 8;
    const int64_t total = (int64_t)B * chunks;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ch = (int)(i % chunks);
        const int b = (int)(i / chunks);
        const int c0 = ch * 8;
        const float* s = src + (int64_t)b * V + c0;
        float v[8];
        if (VEC) {                                               // V % 4 == 0: each group of four lies inside or outside
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 a = c0 < V ? *(const float4*)s : z;
            const float4 c = c0 + 4 < V ? *(const float4*)(s + 4) : z;
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = c.x; v[5] = c.y; v[6] = c.z; v[7] = c.w;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = c0 + k < V ? s[k] : 0.f;
        }
        const float4 t0 = *(const float4*)(table + 8 * (int64_t)b);
        const float4 t1 = *(const float4*)(table + 8 * (int64_t)b + 4);
        const float g = t0.x, sigma = t0.y, p = t0.z, kf = t0.w;
        const int s0 = (int)t1.x, s1 = s0 + (int)t1.y;           // the masked span [s0, s1)
        const int nv = V - c0 < 8 ? V - c0 : 8;                  // real columns of the chunk (>= 1)
        const uint64_t e0 = (row0 + (uint64_t)b) * (uint64_t)V + (uint64_t)c0;
        const uint64_t blk = e0 >> 2;
        const uint32_t sh = VEC ? 0u : (uint32_t)(e0 & 3);
        const int nblk = (int)((sh + (uint32_t)nv - 1u) >> 2) + 1;                  // 1 .. 3
        float n[12];
        uint32_t d[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            n[k] = 0.f;
            d[k] = 0xFFFFFFFFu;
        }
        if (sigma != 0.f) {
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (q < nblk && (!VEC || q < 2)) {
                    const u32x4 x = rng_block(state, blk + q, sid_noise);
                    box_muller(x.w[0], x.w[1], 1.f, n[4 * q], n[4 * q + 1]);
                    box_muller(x.w[2], x.w[3], 1.f, n[4 * q + 2], n[4 * q + 3]);
                }
        }
        const uint32_t thr = prob_threshold(p);
        if (thr != 0u) {
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (q < nblk && (!VEC || q < 2)) {
                    const u32x4 x = rng_block(state, blk + q, sid_drop);
#pragma unroll
                    for (int k = 0; k < 4; ++k) d[4 * q + k] = x.w[k];
                }
        }
        float y[8];
        h8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = c0 + k;
            float t = g * v[k];
            if (sigma != 0.f) t = fmaf(sigma, pick(n, k, sh), t);          // (skipped, not fma(0, n, t): -0 stays -0)
            const bool zero = c >= V || (c >= s0 && c < s1) || pick(d, k, sh) < thr;
            const half_t h = mul_then_f16(t, kf);
            y[k] = zero ? 0.f : t * kf;
            o[k] = zero ? (half_t)0.f : h;
        }
        *(h8*)(dst16 + (int64_t)b * Vp + c0) = o;
        if (dst32) {
            float* dd = dst32 + (int64_t)b * V + c0;
            if (VEC) {
                if (c0 < V) *(float4*)dd = make_float4(y[0], y[1], y[2], y[3]);
                if (c0 + 4 < V) *(float4*)(dd + 4) = make_float4(y[4], y[5], y[6], y[7]);
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (c0 + k < V) dd[k] = y[k];
            }
        }
    }
}

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? OK : E_LAUNCH)

}  // namespace

int voxaug_params_launch(const int64_t* state, float* table, int rows, int64_t row0, int sid, int V, float gain, float sigma,
                         float p, int rescale, int span_len, float prob, hipStream_t st) {
    hipLaunchKernelGGL(voxaug_params_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, state, table, rows, (uint64_t)row0,
                       (uint32_t)sid, (uint32_t)V, gain, sigma, p, rescale, (uint32_t)span_len, prob);
    return LAUNCH_OK();
}

int voxaug_apply_launch(const float* src, int V, int B, const float* table, const int64_t* state, int64_t row0,
                        int sid_noise, int sid_drop, half_t* dst16, float* dst32, hipStream_t st) {
    const int Vp = (V + 7) / 8 * 8;
    const int64_t total = (int64_t)B * (Vp / 8);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    const bool vec = V % 4 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst32 & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(voxaug_apply_kernel<true>, dim3(blocks), dim3(256), 0, st, src, V, Vp, B, table, state,
                           (uint64_t)row0, (uint32_t)sid_noise, (uint32_t)sid_drop, dst16, dst32);
    else
        hipLaunchKernelGGL(voxaug_apply_kernel<false>, dim3(blocks), dim3(256), 0, st, src, V, Vp, B, table, state,
                           (uint64_t)row0, (uint32_t)sid_noise, (uint32_t)sid_drop, dst16, dst32);
    return LAUNCH_OK();
}

}  // namespace fmri
