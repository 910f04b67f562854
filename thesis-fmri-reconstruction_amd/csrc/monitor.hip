// Numerics monitor kernels (opt-in, fmri_hip/monitor.py): statistics of tensor segments -- true-scale gradients,
// weights, the encoder head, the loss slots -- into fmri_stat records.
//
// Bit-reproducible by construction: every thread walks a fixed set of elements in a fixed order, every block folds its
// threads with an xor-shuffle tree and its waves in index order (stat_block), and the fold kernels read the per-block
// records in index order.  No float atomics (sumsq64_kernel / rows_absmax_kernel of loss.hip add their blocks with
// atomics, whose order varies between runs: they serve the step itself, where that order does not matter).
#include "kernels.h"

namespace fmri {

// blockIdx.y = segment, blockIdx.x = one of the segment's nblk partial records
__global__ __launch_bounds__(256) void tensor_stats_kernel(const StatSegs segs, StatRec* __restrict__ ws) {
    __shared__ StatAcc red[4];
    const int s = blockIdx.y;
    const StatSeg& g = segs.s[s];
    const int nb = segs.nblk[s];
    if ((int)blockIdx.x >= nb) return;
    if (g.gate && *g.gate == 0) return;
    const float gs = g.scale / (g.div ? *g.div : 1.f);         // (fmri_rmsprop_dev / fmri_adam_dev: g_true = g * gs)
    const int64_t total = g.rows * g.cols;
    const int64_t step = (int64_t)nb * 256;
    StatAcc a;
    stat_init(a);
    if (g.ld == g.cols) {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += step)
            stat_add_clamped(a, g.x[i] * gs, g.clamp);
    } else {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
            const int64_t r = i / g.cols, c = i - r * g.cols;
            stat_add_clamped(a, g.x[r * g.ld + c] * gs, g.clamp);
        }
    }
    const StatAcc b = stat_block(a, red);
    if (threadIdx.x == 0) ws[(int64_t)s * STAT_BLOCKS + blockIdx.x] = stat_rec(b, 0);
}

// records p[k * step] (k < n) folded in index order: each thread takes a fixed strided subset, then stat_block
__device__ __forceinline__ StatAcc fold_records(const StatRec* __restrict__ p, int n, int step, StatAcc* red) {
    StatAcc a;
    stat_init(a);
    for (int k = threadIdx.x; k < n; k += 256) stat_merge_rec(a, p[(int64_t)k * step]);
    return stat_block(a, red);
}

// one block per segment
__global__ __launch_bounds__(256) void tensor_stats_fold_kernel(const StatSegs segs, const StatRec* __restrict__ ws) {
    __shared__ StatAcc red[4];
    const int s = blockIdx.x;
    const StatSeg& g = segs.s[s];
    if (g.gate && *g.gate == 0) return;
    const StatAcc a = fold_records(ws + (int64_t)s * STAT_BLOCKS, segs.nblk[s], 1, red);
    if (threadIdx.x == 0) *g.out = stat_rec(a, 1);
}

// apply_batch_stats_kernel's interleaved records: block k (0 = gradient, 1 = weights) folds part[2 b + k] into out[k]
__global__ __launch_bounds__(256) void stat_fold_kernel(const StatRec* __restrict__ part, int nrec,
                                                        const int* __restrict__ flag, StatRec* __restrict__ out) {
    __shared__ StatAcc red[4];
    if (flag && *flag == 0) return;
    const StatAcc a = fold_records(part + blockIdx.x, nrec, 2, red);
    if (threadIdx.x == 0) out[blockIdx.x] = stat_rec(a, 1);
}

int tensor_stats_launch(const StatSegs& segs, int nseg, StatRec* ws, hipStream_t st) {
    if (nseg < 1) return OK;
    int mx = 1;
    for (int s = 0; s < nseg; ++s) mx = segs.nblk[s] > mx ? segs.nblk[s] : mx;
    hipLaunchKernelGGL(tensor_stats_kernel, dim3((unsigned)mx, (unsigned)nseg), dim3(256), 0, st, segs, ws);
    hipLaunchKernelGGL(tensor_stats_fold_kernel, dim3((unsigned)nseg), dim3(256), 0, st, segs, (const StatRec*)ws);
    return hipGetLastError() == hipSuccess ? OK : E_LAUNCH;
}

int stat_fold_launch(const StatRec* part, int nrec, const int* flag, StatRec* out, hipStream_t st) {
    hipLaunchKernelGGL(stat_fold_kernel, dim3(2), dim3(256), 0, st, part, nrec, flag, out);
    return hipGetLastError() == hipSuccess ? OK : E_LAUNCH;
}

}  // namespace fmri
