// Probe behind DESIGN 5 ("the ReLU mask is spelled per stream count"): bn_bwd_reduce_kernel<NS> of csrc/norm.hip with ONE
// spelling of the ReLU mask for both stream counts, in the three ways that were tried before the kernel got one per count.
// Register counts and occupancy per spelling (no GPU needed):
//   for m in 0 1 2; do hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -DMASK=$m --cuda-device-only -c \
//       tools/probes/bn_reduce_merged.hip -o /dev/null -Rpass-analysis=kernel-resource-usage; done
//   MASK 0, `on ? g : 0` (the two-stream one):           NS = 1: 134 VGPRs, 3 waves/SIMD (parent 122, 4)   NS = 2: 142, 3 (= parent)
//   MASK 1, `if (relu && !(..)) g = 0` (the one-stream one): NS = 1: 120, 4                                NS = 2: 200, 2 (parent 142, 3)
//   MASK 2, row loops compiled once per value of relu:     NS = 1: 128, 4   NS = 2: 154, 3 -- and NS = 1 ran 31.3 us against 24.4
#include <type_traits>

#include "../../thesis-fmri-reconstruction_amd/csrc/kernels.h"

#ifndef MASK
#define MASK 0
#endif
#if MASK == 0
#define MASK_ONCE const bool on = !relu || (xh * ga[j] + be[j] > 0.f);
#define MASKED_G const float g = on ? (float)gv[s][j] : 0.f;
#elif MASK == 1
#define MASK_ONCE
#define MASKED_G float g = (float)gv[s][j]; if (relu && !(xh * ga[j] + be[j] > 0.f)) g = 0.f;
#else
#define MASK_ONCE
#define MASKED_G const float g = (masked() && !(xh * ga[j] + be[j] > 0.f)) ? 0.f : (float)gv[s][j];
#endif

namespace fmri {

template <int NS>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const half_t* __restrict__ x, const half_t* __restrict__ dy,
                                                            int M, int C, int cx_log2, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int relu,
                                                            float* __restrict__ part /* [gridDim.y][2 NS][C] */) {
    __shared__ float red[256 * 17];
    const int CX = 1 << cx_log2;
    const int RY = 256 >> cx_log2;
    const int cx = threadIdx.x & (CX - 1);
    const int ry = threadIdx.x >> cx_log2;
    const int chunk = blockIdx.x * CX + cx;
    const int nch = C >> 3;
    float s0[NS][8], s1[NS][8];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) { s0[s][j] = 0.f; s1[s][j] = 0.f; }
    if (chunk < nch) {
        float mu[8], rs[8], ga[8], be[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            mu[j] = mean[chunk * 8 + j]; rs[j] = rstd[chunk * 8 + j];
            ga[j] = gamma[chunk * 8 + j]; be[j] = beta[chunk * 8 + j];
        }
        const int stride = gridDim.y * RY;
        const int64_t coff = (int64_t)chunk * 8;
        const int64_t sstride = (int64_t)M * C;
        auto rows = [&](auto masked) {
            auto body = [&](const h8& xv, const h8 (&gv)[NS]) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xh = ((float)xv[j] - mu[j]) * rs[j];
                    MASK_ONCE
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        MASKED_G
                        s0[s][j] += g; s1[s][j] += g * xh;
                    }
                }
            };
            int m = blockIdx.y * RY + ry;
            for (; m + 3 * stride < M; m += 4 * stride) {
                h8 xv[4], gv[4][NS];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t o = (int64_t)(m + u * stride) * C + coff;
                    xv[u] = *(const h8*)(x + o);
#pragma unroll
                    for (int s = 0; s < NS; ++s) gv[u][s] = *(const h8*)(dy + s * sstride + o);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) body(xv[u], gv[u]);
            }
            for (; m < M; m += stride) {
                const int64_t o = (int64_t)m * C + coff;
                h8 gv[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) gv[s] = *(const h8*)(dy + s * sstride + o);
                body(*(const h8*)(x + o), gv);
            }
        };
#if MASK == 2
        if (relu) rows(std::true_type{});
        else rows(std::false_type{});
#else
        rows(0);
#endif
    }
    // block reduction of the 16 per-thread values of a stream over the RY row lanes, stream by stream
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s) __syncthreads();              // (the previous stream's fold is done with `red`)
#pragma unroll
        for (int j = 0; j < 8; ++j) { red[threadIdx.x * 17 + j] = s0[s][j]; red[threadIdx.x * 17 + 8 + j] = s1[s][j]; }
        __syncthreads();
        for (int t = threadIdx.x; t < CX * 16; t += 256) {
            const int c = t >> 4, j = t & 15;
            const int ch = blockIdx.x * CX + c;
            if (ch >= nch) continue;
            float v = 0.f;
            for (int r = 0; r < RY; ++r) v += red[((r << cx_log2) + c) * 17 + j];
            part[((int64_t)blockIdx.y * 2 * NS + 2 * s + (j >> 3)) * C + ch * 8 + (j & 7)] = v;
        }
    }
}

template __global__ void bn_bwd_reduce_kernel<1>(const half_t*, const half_t*, int, int, int, const float*, const float*,
                                                 const float*, const float*, int, float*);
template __global__ void bn_bwd_reduce_kernel<2>(const half_t*, const half_t*, int, int, int, const float*, const float*,
                                                 const float*, const float*, int, float*);

}  // namespace fmri
