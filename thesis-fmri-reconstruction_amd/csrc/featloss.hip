// Feature-matching loss head for WIDE rows (recon_level 1 / 2: F = 131 072 / 65 536 halves per sample at 64 px).
//
// loss.hip's feat_mse_kernel / feat_mse_bwd_kernel give one 256-thread block to a sample: sized for recon_level 3
// (F = 16 384, 32 KB per row).  At the lower levels a row is up to 256 KB, B blocks of four waves leave most of the
// device idle, and the deterministic forward (one block) walks the whole tensor alone.  Here the unit of work is a
// (row, column chunk) task of FEAT_CHUNK halves; the grid is sized from the CU count, not from B, and walks the tasks
// with a grid stride.  Streaming kernels: 16-byte loads and stores, one h8 per lane and operand, fully coalesced.
//
//   forward : task t = (b, c) -> part[t] = sum over the chunk of 0.5 (f_o - f_p)^2 (fp32, fixed order inside the block);
//             a second one-block launch folds part[] in index order: row sums -> mse_rows, their sum is added onto
//             *mse_total.  No atomics anywhere, so the bits do not depend on fmri_set_deterministic, the grid or the CU
//             count.
//   backward: the arithmetic of feat_mse_bwd_kernel per element (same bits), tasks as above; the zero rows of the sampled
//             images are written only on request.
// Offsets are formed in 64 bits BEFORE the multiply: 3 B F passes 2^31 bytes at B = 256, level 1, 128 px.
#include "kernels.h"

namespace fmri {

namespace {

constexpr int FEAT_CHUNK = 4096;         // halves per task: two h8 per lane and operand
constexpr int FEAT_BLOCKS_PER_CU = 8;    // 8 x 4 waves: full occupancy of a CU's four SIMDs for a kernel with few VGPRs

__device__ __forceinline__ float wide_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float wide_block_sum(float v, float* sh /* >= 4 floats */) {
    v = wide_wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void feat_mse_wide_kernel(const half_t* __restrict__ feat, int B, int F, int nch,
                                                            float* __restrict__ part) {
    __shared__ float sh[4];
    const int64_t tasks = (int64_t)B * nch;
    for (int64_t t = blockIdx.x; t < tasks; t += gridDim.x) {
        const int b = (int)(t / nch);
        const int c = (int)(t - (int64_t)b * nch);
        const int c0 = c * FEAT_CHUNK;
        const int c1 = min(F, c0 + FEAT_CHUNK);
        const half_t* fo = feat + (int64_t)b * F;
        const half_t* fp = feat + ((int64_t)B + b) * F;
        float s = 0.f;
        for (int i = c0 + (int)threadIdx.x * 8; i < c1; i += 256 * 8) {
            const h8 o = *(const h8*)(fo + i);
            const h8 p = *(const h8*)(fp + i);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float df = (float)o[j] - (float)p[j];
                s += 0.5f * df * df;
            }
        }
        s = wide_block_sum(s, sh);
        if (threadIdx.x == 0) part[t] = s;
    }
}

// one block: thread b adds the nch partials of row b in chunk order; the rows are summed in a fixed tree
__global__ __launch_bounds__(256) void feat_mse_wide_fold_kernel(const float* __restrict__ part, int B, int nch,
                                                                 float* __restrict__ mse_rows,
                                                                 float* __restrict__ mse_total) {
    __shared__ float sh[4];
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float* p = part + (int64_t)b * nch;
        float s = 0.f;
        for (int c = 0; c < nch; ++c) s += p[c];
        if (mse_rows) mse_rows[b] = s;
        acc += s;
    }
    acc = wide_block_sum(acc, sh);
    if (threadIdx.x == 0 && mse_total) *mse_total += acc;
}

__global__ __launch_bounds__(256) void feat_mse_bwd_wide_kernel(const half_t* __restrict__ feat, int B, int F, int nch,
                                                                half_t* __restrict__ dfeat, float gscale,
                                                                const float* __restrict__ norm, int zero_rows) {
    const float sc = gscale * (norm ? *norm : 1.f);
    const int64_t tasks = (int64_t)B * nch;
    for (int64_t t = blockIdx.x; t < tasks; t += gridDim.x) {
        const int b = (int)(t / nch);
        const int c = (int)(t - (int64_t)b * nch);
        const int c0 = c * FEAT_CHUNK;
        const int c1 = min(F, c0 + FEAT_CHUNK);
        const int64_t ro = (int64_t)b * F, rp = ((int64_t)B + b) * F, rs = (2 * (int64_t)B + b) * F;
        for (int i = c0 + (int)threadIdx.x * 8; i < c1; i += 256 * 8) {
            const h8 o = *(const h8*)(feat + ro + i);
            const h8 p = *(const h8*)(feat + rp + i);
            h8 d, nd, z;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float df = ((float)o[j] - (float)p[j]) * sc;
                d[j] = (half_t)df;
                nd[j] = (half_t)(-df);
                z[j] = (half_t)0.f;
            }
            *(h8*)(dfeat + ro + i) = d;
            *(h8*)(dfeat + rp + i) = nd;
            if (zero_rows) *(h8*)(dfeat + rs + i) = z;
        }
    }
}

int cu_count() {
    static int cus = 0;
    if (cus <= 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1)
            v = 256;
        cus = v;
    }
    return cus;
}

inline int chunks(int F) { return (F + FEAT_CHUNK - 1) / FEAT_CHUNK; }

inline int wide_grid(int B, int F) {
    const int64_t tasks = (int64_t)B * chunks(F);
    const int64_t cap = (int64_t)cu_count() * FEAT_BLOCKS_PER_CU;
    return (int)(tasks < cap ? tasks : cap);
}

}  // namespace

int feat_mse_wide_chunk() { return FEAT_CHUNK; }
int64_t feat_mse_wide_ws_floats(int B, int F) { return (int64_t)B * chunks(F); }

int feat_mse_wide_launch(const half_t* feat, int B, int F, float* mse_rows, float* mse_total, float* ws,
                         hipStream_t st) {
    const int nch = chunks(F);
    hipLaunchKernelGGL(feat_mse_wide_kernel, dim3(wide_grid(B, F)), dim3(256), 0, st, feat, B, F, nch, ws);
    hipLaunchKernelGGL(feat_mse_wide_fold_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, B, nch, mse_rows,
                       mse_total);
    return hipGetLastError() == hipSuccess ? OK : E_LAUNCH;
}

int feat_mse_bwd_wide_launch(const half_t* feat, int B, int F, half_t* dfeat, float gscale, const float* norm,
                             int zero_rows, hipStream_t st) {
    hipLaunchKernelGGL(feat_mse_bwd_wide_kernel, dim3(wide_grid(B, F)), dim3(256), 0, st, feat, B, F, chunks(F), dfeat,
                       gscale, norm, zero_rows);
    return hipGetLastError() == hipSuccess ? OK : E_LAUNCH;
}

}  // namespace fmri
