// What the fp64 SSIM kernels share (ident.hip, evalmetrics.hip): the tile geometry of the 11 x 11 window, the window
// itself and the fixed-order block sum.
#pragma once
#include "kernels.h"

namespace fmri {

constexpr int SS_TS = 16, SS_WIN = 11, SS_PAD = 5, SS_R = SS_TS + SS_WIN - 1;   // 26

// fixed-order sum over a 256-thread block (wave tree, then the four waves in order); every thread gets the total
__device__ inline double block_sum_fixed(double v, double* sh) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) sh[w] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// gaussian(11, 1.5) normalised to sum 1, in fp64 (the reference's window is the fp32 rounding of the same numbers)
__device__ inline void gauss11(double* g) {
    if (threadIdx.x < SS_WIN) {
        double s = 0.0;
        for (int i = 0; i < SS_WIN; ++i) s += exp(-(double)((i - 5) * (i - 5)) / 4.5);
        const int i = threadIdx.x;
        g[i] = exp(-(double)((i - 5) * (i - 5)) / 4.5) / s;
    }
}

}  // namespace fmri
