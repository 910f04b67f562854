// IMQ-kernel MMD latent penalty of the Wasserstein auto-encoder (Tolstikhin et al., ICLR 2018), value and gradient
// w.r.t. the encoder side in one pass over the pairs (include/fmri_hip.h fmri_mmd_imq for the formula).
//
//   mmd_norms_kernel   |q_i|^2, |p_i|^2 (one wave per row, fixed-order sum)
//   mmd_tile_kernel    block (row tile, column split): 16 rows of q (or of p, for the p-p term) against the 16-column
//                      tiles of its split.  Per tile: Gram 16 x 16 with v_mfma_f32_16x16x4_f32 (each wave one quarter
//                      of d, the four partials summed through LDS in wave order), r = |a|^2 + |b|^2 - 2 a.b clamped at
//                      0, k(r) and kappa'(r) in registers, then the weighted rows W.X with a second MFMA into a 16 x d
//                      accumulator (each wave a quarter of d).  Writes its split's slab of sum_j W_ij X_j, the row sums
//                      of W and an fp64 partial of the statistic -- plain stores, every slot written by one block.
//   mmd_finalize_kernel  dq_i = gscale * w * sum_s (slab_s,i - rowsum_s,i * q_i), statistic = fixed-order fp64 sum of
//                      the partials; no atomics anywhere, so two calls are bit-identical.
#include "kernels.h"

namespace fmri {

namespace {

constexpr int MMD_MAX_SCALES = 8;
constexpr int64_t MMD_SLAB_CAP = 8ll << 20;    // floats: the per-split dq slabs stay under 32 MB
constexpr int MMD_TARGET_BLOCKS = 1024;         // enough blocks for every CU even at n = 64

struct MmdArgs {
    const float* q;
    const float* p;
    int ldq, ldp, n, d;
    int tc;             // 16-row / 16-column tiles per operand: ceil(n / 16)
    int splits;
    int ns;
    float c[MMD_MAX_SCALES];
    float aw, bw;       // 4 / (n (n - 1)), 4 / n^2
    double vs, vx;      // 1 / (n (n - 1)), -2 / n^2
    const float* nrm;   // [2n]: q rows, then p rows
    float* slab;        // [splits][n][d]
    float* rs;          // [splits][n]
    double* vals;       // [splits][2 tc]
    int want_dq;
};

__device__ inline float wave_sum_fixed(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline double wave_sum_fixed(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void mmd_norms_kernel(const float* __restrict__ q, int ldq,
                                                        const float* __restrict__ p, int ldp, int n, int d,
                                                        float* __restrict__ nrm) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= 2 * n) return;
    const float* x = row < n ? q + (int64_t)row * ldq : p + (int64_t)(row - n) * ldp;
    float s = 0.f;
    for (int k = lane; k < d; k += 64) s = fmaf(x[k], x[k], s);
    s = wave_sum_fixed(s);
    if (lane == 0) nrm[row] = s;
}

template <int NT>   // NT = d / 64: 16-column dq tiles per wave
__global__ __launch_bounds__(256) void mmd_tile_kernel(MmdArgs a) {
    __shared__ float part[4][16][17];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lr = lane & 15, lg = lane >> 4;
    const int n = a.n, d = a.d, tc = a.tc;
    const bool is_q = (int)blockIdx.x < tc;
    const int row0 = (is_q ? blockIdx.x : blockIdx.x - tc) * 16;
    const float* R = is_q ? a.q : a.p;
    const int ldr = is_q ? a.ldq : a.ldp;
    const float* nrm_r = is_q ? a.nrm : a.nrm + n;
    const int ct = is_q ? 2 * tc : tc;
    const int t0 = (int)((int64_t)blockIdx.y * ct / a.splits), t1 = (int)((int64_t)(blockIdx.y + 1) * ct / a.splits);
    const int kq = d / 4, kb = wave * kq;
    const bool dq_on = is_q && a.want_dq;

    const int ra = row0 + lr;
    const float* rrow = R + (int64_t)(ra < n ? ra : 0) * ldr;
    f4 acc2[NT];
#pragma unroll
    for (int s = 0; s < NT; ++s) acc2[s] = f4{0.f, 0.f, 0.f, 0.f};
    float rsum = 0.f;
    double vacc = 0.0;

    for (int t = t0; t < t1; ++t) {
        const bool x_is_q = is_q && t < tc;        // q-q tile (else q-p, or p-p for a p-row block)
        const int col0 = (x_is_q || !is_q ? t : t - tc) * 16;
        const float* X = x_is_q ? a.q : a.p;
        const int ldx = x_is_q ? a.ldq : a.ldp;
        const float* nrm_x = x_is_q ? a.nrm : a.nrm + n;
        const bool same = x_is_q || !is_q;          // the diagonal pairs i == j are excluded
        const double vc = is_q && !x_is_q ? a.vx : a.vs;

        // Gram tile G[i][j] = R_{row0+i} . X_{col0+j} over this wave's quarter of d.  Lane (lr, lg) feeds row / column
        // lr with k = k0 + 4 lg + e of a float4; the four e-MFMAs cover the 16 k of one step (both operands use the
        // same k order, so the sum is the dot product in a fixed order).
        const int cb = col0 + lr;
        const float* xrow = X + (int64_t)(cb < n ? cb : 0) * ldx;
        f4 g = f4{0.f, 0.f, 0.f, 0.f};
        for (int k = kb + 4 * lg; k < kb + kq; k += 16) {
            float4 av = ra < n ? *(const float4*)(rrow + k) : make_float4(0.f, 0.f, 0.f, 0.f);
            float4 bv = cb < n ? *(const float4*)(xrow + k) : make_float4(0.f, 0.f, 0.f, 0.f);
            g = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, g, 0, 0, 0);
            g = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, g, 0, 0, 0);
            g = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, g, 0, 0, 0);
            g = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, g, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) part[wave][lg * 4 + r][lr] = g[r];
        __syncthreads();

        // weights in the A-operand layout of the W.X product: lane (lr, lg), k-step tt holds W[lr][4 tt + lg]
        float wa[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const int jj = 4 * tt + lg;
            const float gs = ((part[0][lr][jj] + part[1][lr][jj]) + part[2][lr][jj]) + part[3][lr][jj];
            const int gi = row0 + lr, gj = col0 + jj;
            const bool valid = gi < n && gj < n && !(same && gi == gj);
            float kv = 0.f, kd = 0.f;
            if (valid) {
                const float r = fmaxf(nrm_r[gi] + nrm_x[gj] - 2.f * gs, 0.f);
                for (int s = 0; s < a.ns; ++s) {
                    const float u = 1.f / (a.c[s] + r);
                    kv = fmaf(a.c[s], u, kv);
                    kd = fmaf(-a.c[s] * u, u, kd);
                }
            }
            if (wave == 0) vacc += vc * (double)kv;
            const float wt = !is_q ? 0.f : (x_is_q ? -a.aw * kd : a.bw * kd);
            rsum += wt;
            wa[tt] = wt;
        }
        __syncthreads();            // `part` is rewritten by the next tile

        if (dq_on) {
            // acc2 += W (16 x 16) . X[col0 .. col0 + 16][this wave's quarter of d]
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const int j = col0 + 4 * tt + lg;
                const float* xr = X + (int64_t)(j < n ? j : 0) * ldx + kb + lr;
#pragma unroll
                for (int s = 0; s < NT; ++s) {
                    const float b = j < n ? xr[s * 16] : 0.f;
                    acc2[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[tt], b, acc2[s], 0, 0, 0);
                }
            }
        }
    }

    if (dq_on) {
        float* slab = a.slab + (int64_t)blockIdx.y * n * d;
#pragma unroll
        for (int s = 0; s < NT; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = row0 + lg * 4 + r;
                if (gi < n) slab[(int64_t)gi * d + kb + s * 16 + lr] = acc2[s][r];
            }
        if (wave == 0) {
            // row sum of W: lanes lr, lr + 16, lr + 32, lr + 48 hold the four column residues, added in that order
            const float r0 = __shfl(rsum, lr), r1 = __shfl(rsum, lr + 16), r2 = __shfl(rsum, lr + 32),
                        r3 = __shfl(rsum, lr + 48);
            if (lane < 16 && row0 + lane < n) a.rs[(int64_t)blockIdx.y * n + row0 + lane] = ((r0 + r1) + r2) + r3;
        }
    }
    if (wave == 0) {
        vacc = wave_sum_fixed(vacc);
        if (lane == 0) a.vals[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = vacc;
    }
}

__global__ __launch_bounds__(256) void mmd_finalize_kernel(const float* __restrict__ q, int ldq, int n, int d,
                                                           int splits, const float* __restrict__ slab,
                                                           const float* __restrict__ rs, const double* __restrict__ vals,
                                                           int nvals, float w, float gscale, float* __restrict__ total,
                                                           float* __restrict__ dq, int ldd) {
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        double v = 0.0;
        for (int i = threadIdx.x; i < nvals; i += 64) v += vals[i];
        v = wave_sum_fixed(v);
        if (threadIdx.x == 0 && total) *total += (float)((double)w * v);
    }
    if (!dq) return;
    const int64_t nd = (int64_t)n * d;
    const float f = w * gscale;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nd; e += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(e / d), c = (int)(e - (int64_t)i * d);
        float acc = 0.f, rsum = 0.f;
        for (int s = 0; s < splits; ++s) {
            acc += slab[(int64_t)s * nd + e];
            rsum += rs[(int64_t)s * n + i];
        }
        dq[(int64_t)i * ldd + c] = f * (acc - rsum * q[(int64_t)i * ldq + c]);
    }
}

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? OK : E_LAUNCH)

inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

struct MmdPlan {
    int tc, splits;
    int64_t off_slab, off_rs, off_vals, bytes;
};

MmdPlan mmd_plan(int n, int d) {
    MmdPlan pl;
    pl.tc = (n + 15) / 16;
    int s = (MMD_TARGET_BLOCKS + 2 * pl.tc - 1) / (2 * pl.tc);
    const int64_t cap = MMD_SLAB_CAP / ((int64_t)n * d);
    if (s > cap) s = (int)cap;
    if (s > pl.tc) s = pl.tc;
    if (s < 1) s = 1;
    pl.splits = s;
    pl.off_slab = align256((int64_t)2 * n * 4);
    pl.off_rs = pl.off_slab + align256((int64_t)s * n * d * 4);
    pl.off_vals = pl.off_rs + align256((int64_t)s * n * 4);
    pl.bytes = pl.off_vals + align256((int64_t)s * 2 * pl.tc * 8);
    return pl;
}

}  // namespace

int64_t mmd_imq_ws_bytes(int n, int d) {
    if (n < 2 || d < 64 || d > 1024 || d % 64) return -1;
    return mmd_plan(n, d).bytes;
}

int mmd_imq_launch(const float* q, int ldq, const float* p, int ldp, int n, int d, float sigma2, const float* scales,
                   int nscales, float w, float* total, float* dq, int ldd, float gscale, void* ws, int64_t ws_bytes,
                   hipStream_t st) {
    const MmdPlan pl = mmd_plan(n, d);
    if (ws_bytes < pl.bytes) return E_WORKSPACE;
    char* base = (char*)ws;
    MmdArgs a;
    a.q = q; a.p = p; a.ldq = ldq; a.ldp = ldp; a.n = n; a.d = d; a.tc = pl.tc; a.splits = pl.splits;
    a.ns = nscales;
    for (int s = 0; s < MMD_MAX_SCALES; ++s)
        a.c[s] = s < nscales ? (float)(2.0 * d * (double)sigma2 * (double)scales[s]) : 1.f;
    const double nn1 = (double)n * (n - 1), n2 = (double)n * n;
    a.aw = (float)(4.0 / nn1); a.bw = (float)(4.0 / n2);
    a.vs = 1.0 / nn1; a.vx = -2.0 / n2;
    a.nrm = (const float*)base;
    a.slab = (float*)(base + pl.off_slab);
    a.rs = (float*)(base + pl.off_rs);
    a.vals = (double*)(base + pl.off_vals);
    a.want_dq = dq != nullptr;

    hipLaunchKernelGGL(mmd_norms_kernel, dim3((2 * n + 3) / 4), dim3(256), 0, st, q, ldq, p, ldp, n, d, (float*)a.nrm);
    const dim3 grid(2 * pl.tc, pl.splits);
    switch (d / 64) {
#define MMD_CASE(NT) case NT: hipLaunchKernelGGL(mmd_tile_kernel<NT>, grid, dim3(256), 0, st, a); break;
        MMD_CASE(1) MMD_CASE(2) MMD_CASE(3) MMD_CASE(4) MMD_CASE(5) MMD_CASE(6) MMD_CASE(7) MMD_CASE(8)
        MMD_CASE(9) MMD_CASE(10) MMD_CASE(11) MMD_CASE(12) MMD_CASE(13) MMD_CASE(14) MMD_CASE(15) MMD_CASE(16)
#undef MMD_CASE
        default: return E_UNSUPPORTED;
    }
    const int64_t nd = dq ? (int64_t)n * d : 0;
    int fg = (int)((nd + 255) / 256);
    if (fg < 1) fg = 1;
    if (fg > 4096) fg = 4096;
    hipLaunchKernelGGL(mmd_finalize_kernel, dim3(fg), dim3(256), 0, st, q, ldq, n, d, pl.splits, a.slab, a.rs, a.vals,
                       (int)(pl.splits * 2 * pl.tc), w, gscale, total, dq, ldd);
    return LAUNCH_OK();
}

}  // namespace fmri
