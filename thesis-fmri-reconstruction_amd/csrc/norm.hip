// Batch-norm (train mode) kernels over NHWC fp16 rows [M][C]  (BatchNorm2d and BatchNorm1d alike).
//
// Replaces nn.BatchNorm2d / nn.BatchNorm1d(momentum=0.9) + ReLU of the reference blocks
// (models/vae_gan.py:21,28-29,54,58-59,81,108,158) and their autograd backward:
//   stats    : per-channel sum / sum-of-squares                                      -- HBM bound
//   finalize : mean, rstd, scale/shift, running-stat update (momentum 0.9, unbiased running var,
//              `updates` consecutive updates for the discriminator's REC+GAN double pass)
//   apply    : y = relu(x*scale + shift)                                               -- HBM bound
//   bwd_reduce / bwd_apply : dgamma, dbeta and dx through ReLU + BN (batch statistics)
// The sums are kept outside the kernels so that a data-parallel run can all-reduce them (SyncBN).
//
// All streaming kernels use one thread mapping: a 256-thread block is CX chunk-columns (8 channels =
// 16 bytes each) x RY row lanes; a thread keeps its channel chunk for the whole kernel, so the
// per-channel parameters live in registers and a wave always touches whole contiguous rows.  Row loops
// are unrolled x4 to keep 4 independent 16-byte loads in flight per lane.  Reductions write per-block
// partials to a workspace and a second tiny kernel folds them (no float atomics: 2048 blocks adding
// into the same 2*C words serialise at the memory side).
//
// The backward exists once per direction, templated on the number NS of cotangent streams that share one saved forward
// (bn_bwd_reduce_kernel<NS>, bn_bwd_apply_kernel<NS, COUNT>, bn_cols_bwd_kernel<NS, COUNT>; COUNT: the numerics
// monitor), and every fold of partial rows runs through fold_columns.
#include <type_traits>

#include "kernels.h"

namespace fmri {

struct RowGeom {
    int cx_log2;
    int gx, gy;
};

static RowGeom row_geometry(int M, int C, int max_gy) {
    RowGeom g;
    const int nch = C / 8;
    g.cx_log2 = 0;
    while ((1 << g.cx_log2) < nch && g.cx_log2 < 8) ++g.cx_log2;
    const int CX = 1 << g.cx_log2, RY = 256 >> g.cx_log2;
    g.gx = (nch + CX - 1) / CX;
    int gy = (M + RY * 16 - 1) / (RY * 16);          // >= 16 rows per thread
    int cap = 768 / g.gx;                             // ~3 blocks per CU
    if (cap < 1) cap = 1;
    if (gy > cap) gy = cap;
    if (gy > max_gy) gy = max_gy;
    if (gy < 1) gy = 1;
    g.gy = gy;
    return g;
}

// fp16 store of a BatchNorm-backward result that SATURATES at +-65504 instead of overflowing to inf.  dx = gamma * rstd *
// (...) is the one place of the backward pass where a healthy cotangent is multiplied by an unbounded factor: a feature
// whose batch variance is tiny has rstd up to 1 / sqrt(eps) = 316 -- and 1 / (s sqrt(eps)) behind a range-scaled latent
// batch (bn_finalize_channel) -- so a few of the 8 M results of a step that follows a latent excursion cross fp16's
// range (measured: 1-6 values per such step).  An inf there turns the whole step into NaN (inf - inf in the
// GEMMs that consume it); the saturated value is a clipped gradient for the handful of weights it touches.
// A NaN stays a NaN (v_med3_f32 would return one of the bounds for it): only finite overflow is clipped.
__device__ __forceinline__ half_t sat16(float v) {
    return (half_t)(v == v ? __builtin_amdgcn_fmed3f(v, -65504.f, 65504.f) : v);
}

// Counting variants of the three backward apply kernels (the numerics monitor, fmri_bn_*_cnt; COUNT = true): per lane,
// the results sat16 clips (|v| > 65504, inf included) and the NaNs it stores; at the end of the kernel one ballot +
// popcount per bit of the lane counts sums them over the wave and the wave's first lane adds them to cnt[0] / cnt[1]
// (integer adds: the totals do not depend on the order).  With COUNT = false nothing is counted and `cnt` is not read.
struct SatCount {
    int sat = 0, nan = 0;
};
template <bool COUNT>
__device__ __forceinline__ half_t sat16c(float v, SatCount& n) {
    if (COUNT) {
        const bool fin = v == v;
        n.nan += fin ? 0 : 1;
        n.sat += (fin && fabsf(v) > 65504.f) ? 1 : 0;
    }
    return sat16(v);
}
__device__ __forceinline__ void sat_count_flush(const SatCount& n, int* cnt) {
    if (!__ballot((n.sat | n.nan) != 0)) return;            // (the healthy case: no atomic at all)
    int s = 0, q = 0;
    for (int b = 0; b < 24; ++b) {
        s += __popcll(__ballot((n.sat >> b) & 1)) << b;
        q += __popcll(__ballot((n.nan >> b) & 1)) << b;
    }
    if ((int)__lane_id() == __ffsll((unsigned long long)__ballot(1)) - 1) {
        if (s) atomicAdd(cnt, s);
        if (q) atomicAdd(cnt + 1, q);
    }
}

// MODE 0: sum x, sum x^2.
// MODE 2: activation backward: dpre = dy*act'(y) (y passed as `x`) written to `dout`, column sums of dpre.
// (mean, rstd, gamma and beta are not read: the BatchNorm backward reduction is bn_bwd_reduce_kernel; the argument list
// keeps the code objects of the two modes unchanged.)
template <int MODE>
__global__ __launch_bounds__(256) void bn_reduce_kernel(const half_t* __restrict__ x, const half_t* __restrict__ dy,
                                                        half_t* __restrict__ dout, int M, int C, int cx_log2,
                                                        const float* __restrict__ mean,
                                                        const float* __restrict__ rstd,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, int relu_or_act,
                                                        float* __restrict__ part /* [gridDim.y][2][C] */) {
    __shared__ float red[256 * 17];
    const int CX = 1 << cx_log2;
    const int RY = 256 >> cx_log2;
    const int cx = threadIdx.x & (CX - 1);
    const int ry = threadIdx.x >> cx_log2;
    const int chunk = blockIdx.x * CX + cx;
    const int nch = C >> 3;
    float s0[8], s1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s0[j] = 0.f; s1[j] = 0.f; }
    if (chunk < nch) {
        const int stride = gridDim.y * RY;
        const int64_t coff = (int64_t)chunk * 8;
        auto body = [&](const h8& xv, const h8& gv, int m) {
            if (MODE == 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { const float f = (float)xv[j]; s0[j] += f; s1[j] += f * f; }
            } else {
                h8 ov;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float yy = (float)xv[j];
                    float g = (float)gv[j];
                    if (relu_or_act == ACT_RELU) g = yy > 0.f ? g : 0.f;
                    else if (relu_or_act == ACT_TANH) g = g * (1.f - yy * yy);
                    ov[j] = (half_t)g;
                    s0[j] += g;
                }
                *(h8*)(dout + (int64_t)m * C + coff) = ov;
            }
        };
        int m = blockIdx.y * RY + ry;
        for (; m + 3 * stride < M; m += 4 * stride) {
            h8 xv[4], gv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                xv[u] = *(const h8*)(x + (int64_t)(m + u * stride) * C + coff);
                if (MODE != 0) gv[u] = *(const h8*)(dy + (int64_t)(m + u * stride) * C + coff);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) body(xv[u], gv[u], m + u * stride);
        }
        for (; m < M; m += stride) {
            h8 xv = *(const h8*)(x + (int64_t)m * C + coff), gv;
            if (MODE != 0) gv = *(const h8*)(dy + (int64_t)m * C + coff);
            body(xv, gv, m);
        }
    }
    if (part == nullptr) return;
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[threadIdx.x * 17 + j] = s0[j]; red[threadIdx.x * 17 + 8 + j] = s1[j]; }
    __syncthreads();
    // 16 values per chunk column, summed over the RY row lanes; spread over the block's threads
    for (int t = threadIdx.x; t < CX * 16; t += 256) {
        const int c = t >> 4, j = t & 15;
        const int ch = blockIdx.x * CX + c;
        if (ch >= nch) continue;
        float s = 0.f;
        for (int r = 0; r < RY; ++r) s += red[((r << cx_log2) + c) * 17 + j];
        part[((int64_t)blockIdx.y * 2 + (j >> 3)) * C + ch * 8 + (j & 7)] = s;
    }
}

// ---- folds of partial rows.  The partial matrices are small, but a single serial chain per column is latency bound
// (few blocks, tiny data), so a 1024-thread block takes 32 columns x 32 row lanes and every lane keeps DEPTH loads per
// column in flight.
//
// The one fold loop: rows [lo, hi) of the NC columns i, i + cstride, .. of a partial matrix with n columns.  Row lane r
// (threadIdx.x >> 5) sums rows lo + r, lo + r + 32, .. into DEPTH accumulators by turns, adds them pairwise
// ((s0 + s1) + (s2 + s3)), and row lane 0 adds the 32 lane sums in lane order: out[] is the block's result THERE and
// meaningless in the other row lanes.  `live` = this lane's columns exist.  Contains a __syncthreads.
template <int DEPTH, int NC>
__device__ __forceinline__ void fold_columns(const float* __restrict__ part, int lo, int hi, int n, int i, int cstride,
                                             bool live, float (&out)[NC]) {
    static_assert(DEPTH == 2 || DEPTH == 4, "pairwise sum of the accumulators");
    __shared__ float red[NC][32][33];
    const int cx = threadIdx.x & 31, gy = threadIdx.x >> 5;
    float s[NC][DEPTH];
#pragma unroll
    for (int k = 0; k < NC; ++k)
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) s[k][u] = 0.f;
    if (live) {
        int p = lo + gy;
        for (; p + 32 * (DEPTH - 1) < hi; p += 32 * DEPTH)
#pragma unroll
            for (int u = 0; u < DEPTH; ++u)
#pragma unroll
                for (int k = 0; k < NC; ++k) s[k][u] += part[(int64_t)(p + 32 * u) * n + i + k * cstride];
        for (; p < hi; p += 32)
#pragma unroll
            for (int k = 0; k < NC; ++k) s[k][0] += part[(int64_t)p * n + i + k * cstride];
    }
#pragma unroll
    for (int k = 0; k < NC; ++k)
        red[k][gy][cx] = DEPTH == 4 ? (s[k][0] + s[k][1]) + (s[k][2] + s[k][3]) : s[k][0] + s[k][1];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NC; ++k) out[k] = 0.f;
    if (gy == 0)
#pragma unroll
        for (int r = 0; r < 32; ++r)
#pragma unroll
            for (int k = 0; k < NC; ++k) out[k] += red[k][r][cx];
}

// sums[g][i] = sum_p part[g][p][i], i < n, for the groups g = blockIdx.y (group stride part_gstride floats; the partials
// of one reduction are one group, BnBwdEpi's statistics rows are up to four cotangent groups).  Group `pgroup` also
// accumulates its folded sums into parameter gradients -- one writer per element, no atomics: columns [gOff, gOff + gC)
// -> g0 += gscale * sum (d beta, or a bias gradient), [gOff + gC, gOff + 2 gC) -> g1 (d gamma); either may be null.
__global__ __launch_bounds__(1024) void fold_sums_kernel(const float* __restrict__ part, int nparts, int n,
                                                         int64_t part_gstride, float* __restrict__ sums,
                                                         float* __restrict__ g0, float* __restrict__ g1, float gscale,
                                                         int pgroup, int gOff, int gC) {
    const int i = blockIdx.x * 32 + (threadIdx.x & 31);
    float s[1];
    fold_columns<4, 1>(part + blockIdx.y * part_gstride, 0, nparts, n, i, 0, i < n, s);
    if (threadIdx.x < 32 && i < n) {
        sums[(int64_t)blockIdx.y * n + i] = s[0];
        if ((int)blockIdx.y == pgroup) {
            if (g0 && i >= gOff && i < gOff + gC) g0[i - gOff] += gscale * s[0];
            if (g1 && i >= gOff + gC && i < gOff + 2 * gC) g1[i - gOff - gC] += gscale * s[0];
        }
    }
}

// stage 1 of a long fold (statistics rows written by a contraction's epilogue, StatEpi): block (x, y, g) sums rows
// [y*per, (y+1)*per) of columns 32x .. 32x+31 of group g into out[g][y][n].
__global__ __launch_bounds__(1024) void fold_rows_kernel(const float* __restrict__ part, int nparts, int n, int per,
                                                         float* __restrict__ out, int64_t part_gstride,
                                                         int64_t out_gstride) {
    const int i = blockIdx.x * 32 + (threadIdx.x & 31);
    const int lo = blockIdx.y * per;
    const int hi = lo + per < nparts ? lo + per : nparts;
    float s[1];
    fold_columns<4, 1>(part + blockIdx.z * part_gstride, lo, hi, n, i, 0, i < n, s);
    if (threadIdx.x < 32 && i < n) out[blockIdx.z * out_gstride + (int64_t)blockIdx.y * n + i] = s[0];
}

// channel c from its batch sums (every finalizing kernel); returns (scale, shift).
// ``in_scale``: the rows are s * x for a power of two s (a latent batch stored range-scaled, fmri_latent_fwd_ranged):
// BN_eps(x) == BN_{eps s^2}(s x), so the normalisation runs on the stored values with eps * s^2 -- mean / rstd / scale /
// shift are those of the STORED rows (what the apply and backward kernels read) -- and the running statistics receive
// the true-scale mean / s and var / s^2.
__device__ __forceinline__ float2 bn_finalize_channel(int c, float sx, float sxx, float count, const BnFinalize& f) {
    const float in_s = f.in_scale ? *f.in_scale : 1.f;
    const float gamma = f.gamma[c], beta = f.beta[c];     // (read before the stores: the struct's pointers may alias)
    const float mean = sx / count;
    float var = sxx / count - mean * mean;
    var = var > 0.f ? var : 0.f;
    const float rstd = rsqrtf(var + f.eps * in_s * in_s);
    f.mean[c] = mean;
    f.rstd[c] = rstd;
    const float sc = gamma * rstd, sh = beta - mean * sc;
    f.scale[c] = sc;
    f.shift[c] = sh;
    if (f.running_mean && f.updates > 0) {
        const float inv_s = 1.f / in_s;
        const float unb = (count > 1.f ? var * count / (count - 1.f) : var) * inv_s * inv_s;
        const float mean_t = mean * inv_s;
        float rm = f.running_mean[c], rv = f.running_var[c];
        for (int u = 0; u < f.updates; ++u) {
            rm = (1.f - f.momentum) * rm + f.momentum * mean_t;
            rv = (1.f - f.momentum) * rv + f.momentum * unb;
        }
        f.running_mean[c] = rm;
        f.running_var[c] = rv;
    }
    return make_float2(sc, sh);
}
// num_batches_tracked: one thread of a finalizing launch
__device__ __forceinline__ void bn_count_batches(const BnFinalize& f) {
    if (f.nbt && f.updates > 0) *f.nbt += f.updates;
}

// fold of the statistics partials [nparts][2][C] + finalize in one launch (forward BatchNorm without a statistics
// exchange between ranks): block = 32 channels x 32 row lanes, both sums of a channel are folded by the same lanes.
__global__ __launch_bounds__(1024) void fold_finalize_kernel(const float* __restrict__ part, int nparts, int C,
                                                             float* __restrict__ sums, float count, BnFinalize f) {
    const int c = blockIdx.x * 32 + (threadIdx.x & 31);
    float s[2];
    fold_columns<2, 2>(part, 0, nparts, 2 * C, c, C, c < C, s);
    if (blockIdx.x == 0 && threadIdx.x == 0) bn_count_batches(f);
    if (threadIdx.x < 32 && c < C) {
        sums[c] = s[0];
        sums[C + c] = s[1];
        bn_finalize_channel(c, s[0], s[1], count, f);
    }
}

// one thread per channel
__global__ void bn_finalize_kernel(const float* __restrict__ sums, int C, float count, BnFinalize f) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0) bn_count_batches(f);
    if (c >= C) return;
    bn_finalize_channel(c, sums[c], sums[C + c], count, f);
}

// y = act(x*scale + shift): the forward apply.  Template argument and argument list are those of the one forward /
// backward streaming kernel this was mode 0 of (dy, gamma, beta, inv_count and sums are not read), which keeps its code
// object unchanged; the backward modes are bn_bwd_apply_kernel.
template <int MODE>
__global__ __launch_bounds__(256) void bn_stream_kernel(const half_t* __restrict__ x, const half_t* __restrict__ dy,
                                                        half_t* __restrict__ out, int M, int C, int cx_log2,
                                                        const float* __restrict__ p0, const float* __restrict__ p1,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, int relu, float inv_count,
                                                        const float* __restrict__ sums) {
    static_assert(MODE == 0, "forward apply only");
    const int CX = 1 << cx_log2;
    const int RY = 256 >> cx_log2;
    const int cx = threadIdx.x & (CX - 1);
    const int ry = threadIdx.x >> cx_log2;
    const int chunk = blockIdx.x * CX + cx;
    if (chunk >= (C >> 3)) return;
    float a[8], b[8];       // scale, shift
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = chunk * 8 + j;
        a[j] = p0[c]; b[j] = p1[c];
    }
    const int stride = gridDim.y * RY;
    const int64_t coff = (int64_t)chunk * 8;
    auto body = [&](const h8& xv, int m) {
        h8 ov;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float f = (float)xv[j] * a[j] + b[j];
            if (relu) f = f > 0.f ? f : 0.f;
            ov[j] = (half_t)f;
        }
        *(h8*)(out + (int64_t)m * C + coff) = ov;
    };
    int m = blockIdx.y * RY + ry;
    for (; m + 3 * stride < M; m += 4 * stride) {
        h8 xv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) xv[u] = *(const h8*)(x + (int64_t)(m + u * stride) * C + coff);
#pragma unroll
        for (int u = 0; u < 4; ++u) body(xv[u], m + u * stride);
    }
    for (; m < M; m += stride) {
        h8 xv = *(const h8*)(x + (int64_t)m * C + coff);
        body(xv, m);
    }
}

// ---- BatchNorm backward of NS cotangent streams through one saved forward, stacked along the rows: dy = [stream 0 rows |
// stream 1 rows], M rows each (NS = 2: the discriminator's logit stream A and feature stream B).  The forward tensor x
// and everything derived from it (xhat, the ReLU mask) are read and computed once for all streams: 3 + 5 tensor passes
// instead of 2 x (2 + 3) at NS = 2.  g_s = dy_s masked by the ReLU of the forward;
// partials / sums layout [NS][2][C]: (sum g_s | sum g_s*xhat) per stream, stream A first.
// The ReLU mask is spelled per stream count, `if (relu && !(..)) g = 0` for one stream and `on ? g : 0` for two, in the
// reduction and in the apply kernel alike: the compiler hoists the test on `relu` out of the row loop for the first
// spelling only, and each count is fastest with the code it always had.  One spelling for both costs one of them an
// occupancy step or 5-8 % of the two-stream apply (tools/probes/bn_reduce_merged.hip,
// profiles/bn_refactor_ab.txt).  The values are the same either way.
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
        auto body = [&](const h8& xv, const h8 (&gv)[NS]) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float xh = ((float)xv[j] - mu[j]) * rs[j];
                const bool on = !relu || (xh * ga[j] + be[j] > 0.f);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    float g = (float)gv[s][j];
                    if (NS == 1) { if (relu && !(xh * ga[j] + be[j] > 0.f)) g = 0.f; }
                    else g = on ? g : 0.f;
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

// dx_s = gamma*rstd*(g_s - sum_g_s/M - xhat*sum_gx_s/M) for every stream, x read once.  A lane keeps 4 / NS rows (3, or 2 x
// 3, 16-byte loads) in flight.
template <int NS, bool COUNT>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const half_t* __restrict__ x, const half_t* __restrict__ dy,
                                                           half_t* __restrict__ dx, int M, int C, int cx_log2,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, int relu, float inv_count,
                                                           const float* __restrict__ sums /* [NS][2][C] */,
                                                           int* __restrict__ cnt) {
    constexpr int U = 4 / NS;
    SatCount nc;
    const int CX = 1 << cx_log2;
    const int RY = 256 >> cx_log2;
    const int cx = threadIdx.x & (CX - 1);
    const int ry = threadIdx.x >> cx_log2;
    const int chunk = blockIdx.x * CX + cx;
    if (chunk < (C >> 3)) {
        // xhat = (x - mu)*rs;  dx_s = k*(g_s - c0_s - xhat*c1_s), k = gamma*rstd, c0_s = sum_g_s/M, c1_s = sum_gx_s/M
        float mu[8], rs[8], ga[8], be[8], k[8], c0[NS][8], c1[NS][8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = chunk * 8 + j;
            mu[j] = mean[c]; rs[j] = rstd[c]; ga[j] = gamma[c]; be[j] = beta[c];
            k[j] = ga[j] * rs[j];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                c0[s][j] = sums[(2 * s) * C + c] * inv_count;
                c1[s][j] = sums[(2 * s + 1) * C + c] * inv_count;
            }
        }
        const int stride = gridDim.y * RY;
        const int64_t coff = (int64_t)chunk * 8;
        const int64_t sstride = (int64_t)M * C;
        auto body = [&](const h8& xv, const h8 (&gv)[NS], int m) {
            h8 ov[NS];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float xh = ((float)xv[j] - mu[j]) * rs[j];
                const bool on = !relu || (xh * ga[j] + be[j] > 0.f);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    float g = (float)gv[s][j];
                    if (NS == 1) { if (relu && !(xh * ga[j] + be[j] > 0.f)) g = 0.f; }      // (the note above)
                    else g = on ? g : 0.f;
                    ov[s][j] = sat16c<COUNT>(k[j] * (g - c0[s][j] - xh * c1[s][j]), nc);
                }
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) *(h8*)(dx + s * sstride + (int64_t)m * C + coff) = ov[s];
        };
        int m = blockIdx.y * RY + ry;
        for (; m + (U - 1) * stride < M; m += U * stride) {
            h8 xv[U], gv[U][NS];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t o = (int64_t)(m + u * stride) * C + coff;
                xv[u] = *(const h8*)(x + o);
#pragma unroll
                for (int s = 0; s < NS; ++s) gv[u][s] = *(const h8*)(dy + s * sstride + o);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) body(xv[u], gv[u], m + u * stride);
        }
        for (; m < M; m += stride) {
            const int64_t o = (int64_t)m * C + coff;
            h8 gv[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) gv[s] = *(const h8*)(dy + s * sstride + o);
            body(*(const h8*)(x + o), gv, m);
        }
    }
    if (COUNT) sat_count_flush(nc, cnt);
}

// ---- BatchNorm over FEW rows (the dense layers: BatchNorm1d behind fc.0 / fc1.0, M = batch rows) in ONE launch per
// direction.  The streaming kernels above pay three launches per call (partial sums, fold, apply) -- 15-20 us for half a
// megabyte of data, six times per step and direction.  Here a block owns 32 channels (4 chunk columns x 64 row lanes) for
// all rows: pass 1 sums its columns, the block folds them in LDS and finalizes (mean, rstd, scale, shift, running
// statistics / the backward constants and the parameter gradients), pass 2 re-reads the rows (L2) and writes the result.
// Fixed summation order: bit-reproducible.
constexpr int COLS_CX = 4, COLS_RY = 64;

// dst[16] <- sums of the 16 per-thread values of chunk column cx over the row lanes (called by threads < COLS_CX * 16)
__device__ __forceinline__ float cols_fold(const float* red, int cx, int j) {
    float s = 0.f;
    for (int r = 0; r < COLS_RY; ++r) s += red[((r * COLS_CX) + cx) * 17 + j];
    return s;
}

__global__ __launch_bounds__(256) void bn_cols_fwd_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, int M,
                                                          int C, float count, BnFinalize fin, float* __restrict__ sums,
                                                          int relu) {
    __shared__ float red[256 * 17];
    __shared__ float par[COLS_CX * 8][2];
    const int cx = threadIdx.x & (COLS_CX - 1), ry = threadIdx.x >> 2;
    const int chunk = blockIdx.x * COLS_CX + cx;
    const int nch = C >> 3;
    const int64_t coff = (int64_t)chunk * 8;
    float s0[8], s1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s0[j] = 0.f; s1[j] = 0.f; }
    if (chunk < nch)
        for (int m = ry; m < M; m += COLS_RY) {
            const h8 v = *(const h8*)(x + (int64_t)m * C + coff);
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float f = (float)v[j]; s0[j] += f; s1[j] += f * f; }
        }
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[threadIdx.x * 17 + j] = s0[j]; red[threadIdx.x * 17 + 8 + j] = s1[j]; }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) bn_count_batches(fin);
    if (threadIdx.x < COLS_CX * 8) {
        const int c_ = threadIdx.x >> 3, j = threadIdx.x & 7;
        const int c = (blockIdx.x * COLS_CX + c_) * 8 + j;
        if (c < C) {
            const float sx = cols_fold(red, c_, j), sxx = cols_fold(red, c_, 8 + j);
            sums[c] = sx;
            sums[C + c] = sxx;
            const float2 ss = bn_finalize_channel(c, sx, sxx, count, fin);
            par[threadIdx.x][0] = ss.x;
            par[threadIdx.x][1] = ss.y;
        }
    }
    __syncthreads();
    if (chunk >= nch) return;
    float a[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { a[j] = par[cx * 8 + j][0]; b[j] = par[cx * 8 + j][1]; }
    for (int m = ry; m < M; m += COLS_RY) {
        const h8 v = *(const h8*)(x + (int64_t)m * C + coff);
        h8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float f = (float)v[j] * a[j] + b[j];
            if (relu) f = f > 0.f ? f : 0.f;
            o[j] = (half_t)f;
        }
        *(h8*)(y + (int64_t)m * C + coff) = o;
    }
}

// backward through (ReLU o BN) of NS cotangent streams stacked along the rows (dy = [stream 0 rows | stream 1 rows]);
// sums [NS][2][C] = (sum g | sum g*xhat) per stream; dbeta / dgamma (may be null) += gscale * sums of stream `pstream`
template <int NS, bool COUNT>
__global__ __launch_bounds__(256) void bn_cols_bwd_kernel(const half_t* __restrict__ x, const half_t* __restrict__ dy,
                                                          half_t* __restrict__ dx, int M, int C, float inv_count,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, int relu,
                                                          float* __restrict__ sums, float* __restrict__ dbeta,
                                                          float* __restrict__ dgamma, float gscale, int pstream,
                                                          int* __restrict__ cnt) {
    __shared__ float red[256 * 17];
    __shared__ float par[NS][COLS_CX * 8][2];
    SatCount nc;
    const int cx = threadIdx.x & (COLS_CX - 1), ry = threadIdx.x >> 2;
    const int chunk = blockIdx.x * COLS_CX + cx;
    const int nch = C >> 3;
    const int64_t coff = (int64_t)chunk * 8;
    const int64_t sstride = (int64_t)M * C;
    float mu[8], rs[8], ga[8], be[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = chunk < nch ? chunk * 8 + j : 0;
        mu[j] = mean[c]; rs[j] = rstd[c]; ga[j] = gamma[c]; be[j] = beta[c];
    }
    for (int st = 0; st < NS; ++st) {
        float s0[8], s1[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { s0[j] = 0.f; s1[j] = 0.f; }
        if (chunk < nch)
            for (int m = ry; m < M; m += COLS_RY) {
                const int64_t o = (int64_t)m * C + coff;
                const h8 xv = *(const h8*)(x + o);
                const h8 gv = *(const h8*)(dy + st * sstride + o);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xh = ((float)xv[j] - mu[j]) * rs[j];
                    float g = (float)gv[j];
                    if (relu && !(xh * ga[j] + be[j] > 0.f)) g = 0.f;
                    s0[j] += g; s1[j] += g * xh;
                }
            }
        __syncthreads();                     // (the previous stream's fold is done with `red`)
#pragma unroll
        for (int j = 0; j < 8; ++j) { red[threadIdx.x * 17 + j] = s0[j]; red[threadIdx.x * 17 + 8 + j] = s1[j]; }
        __syncthreads();
        if (threadIdx.x < COLS_CX * 8) {
            const int c_ = threadIdx.x >> 3, j = threadIdx.x & 7;
            const int c = (blockIdx.x * COLS_CX + c_) * 8 + j;
            if (c < C) {
                const float sg = cols_fold(red, c_, j), sgx = cols_fold(red, c_, 8 + j);
                sums[(st * 2) * C + c] = sg;
                sums[(st * 2 + 1) * C + c] = sgx;
                par[st][threadIdx.x][0] = sg * inv_count;
                par[st][threadIdx.x][1] = sgx * inv_count;
                if (st == pstream) {
                    if (dbeta) dbeta[c] += gscale * sg;
                    if (dgamma) dgamma[c] += gscale * sgx;
                }
            }
        }
    }
    __syncthreads();
    if (chunk < nch)
        for (int st = 0; st < NS; ++st) {
            float c0[8], c1[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { c0[j] = par[st][cx * 8 + j][0]; c1[j] = par[st][cx * 8 + j][1]; }
            for (int m = ry; m < M; m += COLS_RY) {
                const int64_t o = (int64_t)m * C + coff;
                const h8 xv = *(const h8*)(x + o);
                const h8 gv = *(const h8*)(dy + st * sstride + o);
                h8 ov;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xh = ((float)xv[j] - mu[j]) * rs[j];
                    float g = (float)gv[j];
                    if (relu && !(xh * ga[j] + be[j] > 0.f)) g = 0.f;
                    ov[j] = sat16c<COUNT>(ga[j] * rs[j] * (g - c0[j] - xh * c1[j]), nc);
                }
                *(h8*)(dx + st * sstride + o) = ov;
            }
        }
    if (COUNT) sat_count_flush(nc, cnt);
}

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? OK : E_LAUNCH)

// launch(NS, COUNT) with the run-time stream count and counter switch as compile-time constants
template <class F>
static int bwd_dispatch(int nstreams, bool count, F launch) {
    using std::integral_constant;
    if (nstreams == 1)
        return count ? launch(integral_constant<int, 1>{}, std::true_type{})
                     : launch(integral_constant<int, 1>{}, std::false_type{});
    if (nstreams == 2)
        return count ? launch(integral_constant<int, 2>{}, std::true_type{})
                     : launch(integral_constant<int, 2>{}, std::false_type{});
    return E_UNSUPPORTED;
}

int64_t bn_ws_floats(int M, int C) {
    const RowGeom g = row_geometry(M, C, 1 << 30);
    return (int64_t)g.gy * 2 * C;
}

// part [G][..][n] (group stride gstride floats, `rows` rows each) -> sums [G][n] (+ parameter gradients, fold_sums_kernel)
static void fold_sums(const float* part, int rows, int n, int G, int64_t gstride, float* sums, float* g0, float* g1,
                      float gscale, int pgroup, int gOff, int gC, hipStream_t st) {
    hipLaunchKernelGGL(fold_sums_kernel, dim3((n + 31) / 32, G), dim3(1024), 0, st, part, rows, n, gstride, sums, g0, g1,
                       gscale, pgroup, gOff, gC);
}

// bn_reduce_kernel<MODE> over the rows + the fold of its partials; sums (may be null: then nothing is reduced) gets [2][C];
// g0 / g1 (may be null): g0[c] += gscale * sums[0][c], g1[c] += gscale * sums[1][c], c < g_count
template <int MODE>
static int reduce_launch(const half_t* x, const half_t* dy, half_t* dout, int M, int C, const float* mean,
                         const float* rstd, const float* gamma, const float* beta, int flag, float* sums, float* ws,
                         int64_t ws_floats, hipStream_t st, float* g0, float* g1, float gscale, int g_count) {
    int max_gy = 1 << 30;
    if (sums) {
        if (!ws || ws_floats < 2 * (int64_t)C) return E_WORKSPACE;
        max_gy = (int)(ws_floats / (2 * (int64_t)C));
    }
    const RowGeom g = row_geometry(M, C, max_gy);
    hipLaunchKernelGGL((bn_reduce_kernel<MODE>), dim3(g.gx, g.gy), dim3(256), 0, st, x, dy, dout, M, C, g.cx_log2,
                       mean, rstd, gamma, beta, flag, sums ? ws : (float*)nullptr);
    if (sums) fold_sums(ws, g.gy, 2 * C, 1, 0, sums, g0, g1, gscale, 0, 0, g_count, st);
    return LAUNCH_OK();
}

int bn_stats_finalize_launch(const half_t* x, int M, int C, float* sums, float* ws, int64_t ws_floats, float count,
                             const BnFinalize& f, hipStream_t st) {
    if (!ws || ws_floats < 2 * (int64_t)C) return E_WORKSPACE;
    const RowGeom g = row_geometry(M, C, (int)(ws_floats / (2 * (int64_t)C)));
    hipLaunchKernelGGL((bn_reduce_kernel<0>), dim3(g.gx, g.gy), dim3(256), 0, st, x, (const half_t*)nullptr,
                       (half_t*)nullptr, M, C, g.cx_log2, (const float*)nullptr, (const float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, 0, ws);
    hipLaunchKernelGGL(fold_finalize_kernel, dim3((C + 31) / 32), dim3(1024), 0, st, ws, g.gy, C, sums, count, f);
    return LAUNCH_OK();
}
// Statistics rows of a contraction's epilogue (StatEpi), G groups of them: part [G][..][n], group stride `gstride`.  More
// than 512 rows are folded in two stages through `scratch` ([G][FOLD_STAGE_ROWS][n] floats): returns the rows to fold
// next and updates their count and group stride.
static const float* fold_stage1(const float* part, int& rows, int n, int G, int64_t& gstride, float* scratch,
                                hipStream_t st) {
    if (rows <= 512) return part;        // one 1024-thread block per 32 channels folds 512 rows in 8 four-deep iterations
    const int per = (rows + FOLD_STAGE_ROWS - 1) / FOLD_STAGE_ROWS;
    const int ny = (rows + per - 1) / per;
    const int64_t out_gstride = (int64_t)FOLD_STAGE_ROWS * n;
    hipLaunchKernelGGL(fold_rows_kernel, dim3((n + 31) / 32, ny, G), dim3(1024), 0, st, part, rows, n, per, scratch,
                       gstride, out_gstride);
    rows = ny;
    gstride = out_gstride;
    return scratch;
}
int bn_fold_finalize_launch(const float* part, int rows, int C, float* scratch, float* sums, float count,
                            const BnFinalize& f, hipStream_t st) {
    int64_t gstride = 0;
    const float* src = fold_stage1(part, rows, 2 * C, 1, gstride, scratch, st);
    hipLaunchKernelGGL(fold_finalize_kernel, dim3((C + 31) / 32), dim3(1024), 0, st, src, rows, C, sums, count, f);
    return LAUNCH_OK();
}
int bn_fold_launch(const float* part, int rows, int n, float* scratch, float* sums, hipStream_t st) {
    int64_t gstride = 0;
    const float* src = fold_stage1(part, rows, n, 1, gstride, scratch, st);
    fold_sums(src, rows, n, 1, 0, sums, nullptr, nullptr, 0.f, 0, 0, 0, st);
    return LAUNCH_OK();
}
// part [G][rows_cap][2][C] (the first `rows` rows of each group are valid) -> sums [G][2][C]; group `pgroup` also gives
// the parameter gradients d beta += gscale * sum g, d gamma += gscale * sum g*xhat
int bn_bwd_fold_launch(const float* part, int rows, int rows_cap, int C, int G, float* scratch, float* sums,
                       float* dbeta, float* dgamma, float gscale, int pgroup, hipStream_t st) {
    const int n = 2 * C;
    int64_t gstride = (int64_t)rows_cap * n;
    const float* src = fold_stage1(part, rows, n, G, gstride, scratch, st);
    fold_sums(src, rows, n, G, gstride, sums, dbeta, dgamma, gscale, pgroup, 0, C, st);
    return LAUNCH_OK();
}
int bn_cols_fwd_launch(const half_t* x, half_t* y, int M, int C, float count, const BnFinalize& f, float* sums2C,
                       int relu, hipStream_t st) {
    const int nch = C / 8;
    hipLaunchKernelGGL(bn_cols_fwd_kernel, dim3((nch + COLS_CX - 1) / COLS_CX), dim3(256), 0, st, x, y, M, C, count, f,
                       sums2C, relu);
    return LAUNCH_OK();
}
int bn_cols_bwd_launch(const half_t* x, const half_t* dy, half_t* dx, int M, int C, int nstreams, float count,
                       const float* mean, const float* rstd, const float* gamma, const float* beta, int relu, float* sums,
                       float* dbeta, float* dgamma, float gscale, int pstream, int* cnt, hipStream_t st) {
    const int nch = C / 8;
    return bwd_dispatch(nstreams, cnt != nullptr, [&](auto ns, auto count_on) {
        hipLaunchKernelGGL((bn_cols_bwd_kernel<ns(), count_on()>), dim3((nch + COLS_CX - 1) / COLS_CX), dim3(256), 0, st,
                           x, dy, dx, M, C, 1.f / count, mean, rstd, gamma, beta, relu, sums, dbeta, dgamma, gscale,
                           pstream, cnt);
        return LAUNCH_OK();
    });
}
int bn_stats_launch(const half_t* x, int M, int C, float* sums, float* ws, int64_t ws_floats, hipStream_t st) {
    return reduce_launch<0>(x, nullptr, nullptr, M, C, nullptr, nullptr, nullptr, nullptr, 0, sums, ws, ws_floats, st,
                            nullptr, nullptr, 0.f, 0);
}
// column sums of fp16 rows [M][C] (C % 8 == 0) through the statistics reduction: sums2C = [sum x | sum x^2]; dbias (may be
// null): dbias[c] += gscale * sum x[c], c < dbias_n.  The many-row form of colsum_acc_launch (layout.hip).
int colsum_rows_launch(const half_t* x, int M, int C, float* sums2C, float* ws, int64_t ws_floats, float* dbias,
                       int dbias_n, float gscale, hipStream_t st) {
    return reduce_launch<0>(x, nullptr, nullptr, M, C, nullptr, nullptr, nullptr, nullptr, 0, sums2C, ws, ws_floats, st, dbias,
                            nullptr, gscale, dbias_n);
}
// colsum may be null (then no reduction is performed); colsum gets [2][C] (second half unused).  dbias (may be null):
// dbias[c] += gscale * colsum[c], c < dbias_n <= C, in the fold of the partial sums (one writer per element).
int act_bwd_launch(const half_t* y, const half_t* dy, half_t* dpre, int M, int C, int act, float* colsum, float* ws,
                   int64_t ws_floats, float* dbias, int dbias_n, float gscale, hipStream_t st) {
    return reduce_launch<2>(y, dy, dpre, M, C, nullptr, nullptr, nullptr, nullptr, act, colsum, ws, ws_floats, st, dbias,
                            nullptr, gscale, dbias_n);
}
// sums [nstreams][2][C]; dbeta / dgamma (may be null) += gscale * the sums of stream `param_stream`
int bn_bwd_reduce_launch(const half_t* x, const half_t* dy, int M, int C, int nstreams, const float* mean,
                         const float* rstd, const float* gamma, const float* beta, int relu, float* sums, float* ws,
                         int64_t ws_floats, float* dbeta, float* dgamma, float gscale, int param_stream,
                         hipStream_t st) {
    const int64_t n = 2 * (int64_t)nstreams * C;
    if (!ws || ws_floats < n) return E_WORKSPACE;
    const RowGeom g = row_geometry(M, C, (int)(ws_floats / n));
    return bwd_dispatch(nstreams, false, [&](auto ns, auto) {
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<ns()>), dim3(g.gx, g.gy), dim3(256), 0, st, x, dy, M, C, g.cx_log2, mean,
                           rstd, gamma, beta, relu, ws);
        fold_sums(ws, g.gy, (int)n, 1, 0, sums, dbeta, dgamma, gscale, 0, param_stream * 2 * C, C, st);
        return LAUNCH_OK();
    });
}
int bn_finalize_launch(const float* sums, int C, float count, const BnFinalize& f, hipStream_t st) {
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, st, sums, C, count, f);
    return LAUNCH_OK();
}
static RowGeom stream_geometry(int M, int C) {
    RowGeom g = row_geometry(M, C, 1 << 30);
    // streaming kernels have no per-block epilogue: allow more blocks for short row loops
    const int RY = 256 >> g.cx_log2;
    int gy = (M + RY * 8 - 1) / (RY * 8);
    int cap = 2048 / g.gx;
    if (cap < 1) cap = 1;
    g.gy = gy > cap ? cap : (gy < 1 ? 1 : gy);
    return g;
}
int bn_apply_launch(const half_t* x, half_t* y, int M, int C, const float* scale, const float* shift, int relu,
                    hipStream_t st) {
    const RowGeom g = stream_geometry(M, C);
    hipLaunchKernelGGL((bn_stream_kernel<0>), dim3(g.gx, g.gy), dim3(256), 0, st, x, (const half_t*)nullptr, y, M, C,
                       g.cx_log2, scale, shift, (const float*)nullptr, (const float*)nullptr, relu, 0.f,
                       (const float*)nullptr);
    return LAUNCH_OK();
}
int bn_bwd_apply_launch(const half_t* x, const half_t* dy, half_t* dx, int M, int C, int nstreams, float count,
                        const float* mean, const float* rstd, const float* gamma, const float* beta, int relu,
                        const float* sums, int* cnt, hipStream_t st) {
    const RowGeom g = stream_geometry(M, C);
    return bwd_dispatch(nstreams, cnt != nullptr, [&](auto ns, auto count_on) {
        hipLaunchKernelGGL((bn_bwd_apply_kernel<ns(), count_on()>), dim3(g.gx, g.gy), dim3(256), 0, st, x, dy, dx, M, C,
                           g.cx_log2, mean, rstd, gamma, beta, relu, 1.f / count, sums, cnt);
        return LAUNCH_OK();
    });
}

}  // namespace fmri
