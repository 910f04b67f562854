// Contrastive latent alignment (symmetric InfoNCE, the "CLIP" loss) between the cognitive encoder's means q and the
// teacher's means t: value, in-batch top-1 retrieval rate and gradient w.r.t. q (include/fmri_hip_contrast.h fmri_latent_nce for
// the formula).  Close kin of mmd.hip: an fp32-MFMA Gram of two [n, d] batches, then a weighted second product.
//
//   nce_norms_kernel     1/|q_i|, 1/|t_j| (one wave per row, squared norm in fp64, fixed order; 0 for a zero row)
//   nce_logits_kernel    block (16-row tile, column split): per 16-column tile of its split the Gram 16 x 16 with
//                        v_mfma_f32_16x16x4_f32 (each wave one quarter of d, the four partials summed through LDS in wave
//                        order), s = clamp(g / (|q_i||t_j|), -1, 1) / tau.  Every lane carries an online (max, sum) pair
//                        of its row over the columns it sees; wave w reduces the (max, sum) of columns 4w .. 4w + 3 of the
//                        tile over the 16 rows.  Writes the tile of logits (in the A-operand order of the second product),
//                        the diagonal, one row pair per (split, row) and one column pair per (row tile, column).
//   nce_fold_kernel      thread i: folds row i's pairs over the splits and column i's pairs over the row tiles in index
//                        order -> (max, log sum) of row i and column i, the fp64 loss term and the hit flag of row i; one
//                        fp64 partial of each per block.
//   nce_weight_kernel    block (16-row tile, column split): G = ((P + Q) / 2 - I) / n from the stored logits, then
//                        acc (16 x d) += (G_ij / |t_j|) . t with a second MFMA (each wave a quarter of d); writes its
//                        split's slab.
//   nce_finalize_kernel  loss and hit count = fixed-order fp64 sums of the block partials; one wave per row:
//                        da = sum of the slabs in split order, dq = gscale * w * (da - (a . da) a) / (tau |q_i|).
// No atomics, every slot written by exactly one block, every fold in a fixed order: two calls are bit-identical.
#include "kernels.h"

#include <cmath>

namespace fmri {

namespace {

constexpr int64_t NCE_SLAB_CAP = 8ll << 20;    // floats: the per-split dq slabs stay under 32 MB
constexpr int NCE_TARGET_BLOCKS = 1024;
constexpr int NCE_MAX_N = 4096;                 // the n x n logits stay under 64 MB

struct NceArgs {
    const float* q;
    const float* t;
    int ldq, ldt, n, d;
    int tc;             // 16-row / 16-column tiles: ceil(n / 16)
    int splits;
    float tau, ninv;    // 1 / n
    int sym, want_dq;
    float* inv;         // [2n]: 1 / |q_i|, then 1 / |t_j|
    float* diag;        // [n]: s_ii
    float2* rowp;       // [splits][n]: (max, sum exp(s - max)) of row i over the split's columns
    float2* colp;       // [tc][n]: the same of column j over the row tile's rows
    float2* lse;        // [2][n]: (max, log sum) of row i, then of column j
    float4* S;          // [tc][tc][64]: lane (lr, lg) of a tile holds s[lr][4 tt + lg], tt = 0 .. 3
    float* slab;        // [splits][n][d]
    double* vals;       // [2][ceil(n / 256)]: loss terms, hits
};

__device__ inline float wave_sum_fixed(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline double wave_sum_fixed(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// (m, l) <- (m, l) (+) (m2, l2) for l = sum exp(. - m); an empty pair is (-inf, 0)
__device__ inline void lse_merge(float& m, float& l, float m2, float l2) {
    const float mn = fmaxf(m, m2);
    const float f1 = m == mn ? 1.f : expf(m - mn), f2 = m2 == mn ? 1.f : expf(m2 - mn);
    l = l * f1 + l2 * f2;
    m = mn;
}

__global__ __launch_bounds__(256) void nce_norms_kernel(const float* __restrict__ q, int ldq,
                                                        const float* __restrict__ t, int ldt, int n, int d,
                                                        float* __restrict__ inv) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= 2 * n) return;
    const float* x = row < n ? q + (int64_t)row * ldq : t + (int64_t)(row - n) * ldt;
    double s = 0.0;
    for (int k = lane; k < d; k += 64) s += (double)x[k] * (double)x[k];
    s = wave_sum_fixed(s);
    if (lane == 0) inv[row] = s > 0.0 ? (float)(1.0 / sqrt(s)) : 0.f;
}

template <int NT>   // NT = d / 64: float4 k-steps per wave in the Gram
__global__ __launch_bounds__(256) void nce_logits_kernel(NceArgs a) {
    __shared__ float part[4][16][17];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lr = lane & 15, lg = lane >> 4;
    const int n = a.n, tc = a.tc;
    const int rt = blockIdx.x, row0 = rt * 16;
    const int t0 = (int)((int64_t)blockIdx.y * tc / a.splits), t1 = (int)((int64_t)(blockIdx.y + 1) * tc / a.splits);
    const int kb = wave * (a.d / 4) + 4 * lg;
    const float* inv_t = a.inv + n;

    // this lane's A fragments of the Gram: row lr of the tile, k = kb + 16 s + e of a float4
    const int gi = row0 + lr;
    const float* qrow = a.q + (int64_t)(gi < n ? gi : 0) * a.ldq + kb;
    float4 qa[NT];
#pragma unroll
    for (int s = 0; s < NT; ++s)
        qa[s] = gi < n ? *(const float4*)(qrow + 16 * s) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float iq = gi < n ? a.inv[gi] : 0.f;
    float rm = -INFINITY, rl = 0.f;         // online (max, sum) of row lr over the columns == lg (mod 4) of every tile

    for (int t = t0; t < t1; ++t) {
        const int col0 = t * 16;
        const int cb = col0 + lr;
        const float* trow = a.t + (int64_t)(cb < n ? cb : 0) * a.ldt + kb;
        f4 g = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            const float4 bv = cb < n ? *(const float4*)(trow + 16 * s) : make_float4(0.f, 0.f, 0.f, 0.f);
            g = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[s].x, bv.x, g, 0, 0, 0);
            g = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[s].y, bv.y, g, 0, 0, 0);
            g = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[s].z, bv.z, g, 0, 0, 0);
            g = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[s].w, bv.w, g, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) part[wave][lg * 4 + r][lr] = g[r];
        __syncthreads();

        // logits in the A-operand layout of the second product: lane (lr, lg), k-step tt holds s[lr][4 tt + lg]
        float sv[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const int jj = 4 * tt + lg, gj = col0 + jj;
            const float gs = ((part[0][lr][jj] + part[1][lr][jj]) + part[2][lr][jj]) + part[3][lr][jj];
            const float it = gj < n ? inv_t[gj] : 0.f;
            const float c = fminf(fmaxf((gs * iq) * it, -1.f), 1.f);      // (a NaN from an overflowed dot product: -1)
            sv[tt] = gi < n && gj < n ? c / a.tau : -INFINITY;
        }
        __syncthreads();            // `part` is rewritten by the next tile

        const float tm = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
        if (tm > -INFINITY) {
            const float mn = fmaxf(rm, tm);
            float acc = rl * (rm == mn ? 1.f : expf(rm - mn));
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) acc += sv[tt] > -INFINITY ? expf(sv[tt] - mn) : 0.f;
            rl = acc;
            rm = mn;
        }
        if (a.sym) {
            // wave w: columns 4 w + lg of the tile over the 16 rows (lanes of equal lg)
            float v = sv[0];
            if (wave == 1) v = sv[1];
            if (wave == 2) v = sv[2];
            if (wave == 3) v = sv[3];
            float cm = v;
            for (int o = 1; o < 16; o <<= 1) cm = fmaxf(cm, __shfl_xor(cm, o));
            float e = v > -INFINITY ? expf(v - cm) : 0.f;
            for (int o = 1; o < 16; o <<= 1) e += __shfl_xor(e, o);
            const int gj = col0 + 4 * wave + lg;
            if (lr == 0 && gj < n) a.colp[(int64_t)rt * n + gj] = make_float2(cm, e);
        }
        if (wave == 0) {
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                if (gi < n && gi == col0 + 4 * tt + lg) a.diag[gi] = sv[tt];
                if (!(sv[tt] > -INFINITY)) sv[tt] = 0.f;
            }
            if (a.want_dq) a.S[((int64_t)rt * tc + t) * 64 + lane] = make_float4(sv[0], sv[1], sv[2], sv[3]);
        }
    }

    if (wave == 0) {
        // row pair: lanes lr, lr + 16, lr + 32, lr + 48 hold the four column residues, merged in that order
        float m = __shfl(rm, lr), l = __shfl(rl, lr);
        for (int k = 1; k < 4; ++k) {
            const float m2 = __shfl(rm, lr + 16 * k), l2 = __shfl(rl, lr + 16 * k);
            lse_merge(m, l, m2, l2);
        }
        if (lane < 16 && row0 + lane < n) a.rowp[(int64_t)blockIdx.y * n + row0 + lane] = make_float2(m, l);
    }
}

__global__ __launch_bounds__(256) void nce_fold_kernel(NceArgs a) {
    __shared__ double sh[2][4];
    const int n = a.n, i = blockIdx.x * 256 + threadIdx.x;
    double v = 0.0, h = 0.0;
    if (i < n) {
        float m = -INFINITY, l = 0.f;
        for (int s = 0; s < a.splits; ++s) {
            const float2 p = a.rowp[(int64_t)s * n + i];
            lse_merge(m, l, p.x, p.y);
        }
        const float ll = logf(l), dg = a.diag[i];
        a.lse[i] = make_float2(m, ll);
        v = ((double)m - (double)dg) + (double)ll;
        h = dg >= m ? 1.0 : 0.0;
        if (a.sym) {
            float m2 = -INFINITY, l2 = 0.f;
            for (int r = 0; r < a.tc; ++r) {
                const float2 p = a.colp[(int64_t)r * n + i];
                lse_merge(m2, l2, p.x, p.y);
            }
            const float lc = logf(l2);
            a.lse[n + i] = make_float2(m2, lc);
            v = 0.5 * (v + (((double)m2 - (double)dg) + (double)lc));
        }
    }
    v = wave_sum_fixed(v);
    h = wave_sum_fixed(h);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[0][wave] = v; sh[1][wave] = h; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.vals[blockIdx.x] = ((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3];
        a.vals[gridDim.x + blockIdx.x] = ((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3];
    }
}

template <int NT>   // NT = d / 64: 16-column dq tiles per wave
__global__ __launch_bounds__(256) void nce_weight_kernel(NceArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lr = lane & 15, lg = lane >> 4;
    const int n = a.n, d = a.d, tc = a.tc;
    const int rt = blockIdx.x, row0 = rt * 16;
    const int t0 = (int)((int64_t)blockIdx.y * tc / a.splits), t1 = (int)((int64_t)(blockIdx.y + 1) * tc / a.splits);
    const int kb = wave * (d / 4);
    const float* inv_t = a.inv + n;
    const int gi = row0 + lr;
    const float2 lrow = gi < n ? a.lse[gi] : make_float2(0.f, 0.f);
    f4 acc2[NT];
#pragma unroll
    for (int s = 0; s < NT; ++s) acc2[s] = f4{0.f, 0.f, 0.f, 0.f};

    for (int t = t0; t < t1; ++t) {
        const int col0 = t * 16;
        const float4 s4 = a.S[((int64_t)rt * tc + t) * 64 + lane];
        const float sv[4] = {s4.x, s4.y, s4.z, s4.w};
        // weights in the A-operand layout: lane (lr, lg), k-step tt holds G[lr][4 tt + lg] / |t_j|
        float wa[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const int gj = col0 + 4 * tt + lg;
            float wt = 0.f;
            if (gi < n && gj < n) {
                float p = expf((sv[tt] - lrow.x) - lrow.y);
                if (a.sym) {
                    const float2 lc = a.lse[n + gj];
                    p = 0.5f * (p + expf((sv[tt] - lc.x) - lc.y));
                }
                if (gi == gj) p -= 1.f;
                wt = (p * a.ninv) * inv_t[gj];
            }
            wa[tt] = wt;
        }
        // acc2 += W (16 x 16) . t[col0 .. col0 + 16][this wave's quarter of d]
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const int j = col0 + 4 * tt + lg;
            const float* xr = a.t + (int64_t)(j < n ? j : 0) * a.ldt + kb + lr;
#pragma unroll
            for (int s = 0; s < NT; ++s) {
                const float b = j < n ? xr[s * 16] : 0.f;
                acc2[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[tt], b, acc2[s], 0, 0, 0);
            }
        }
    }

    float* slab = a.slab + (int64_t)blockIdx.y * n * d;
#pragma unroll
    for (int s = 0; s < NT; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int go = row0 + lg * 4 + r;
            if (go < n) slab[(int64_t)go * d + kb + s * 16 + lr] = acc2[s][r];
        }
}

__global__ __launch_bounds__(256) void nce_finalize_kernel(NceArgs a, int nvals, float w, float gscale,
                                                           float* __restrict__ total, float* __restrict__ top1,
                                                           float* __restrict__ dq, int ldd) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = a.n, d = a.d;
    if (blockIdx.x == 0 && wave == 0) {
        double v = 0.0, h = 0.0;
        for (int i = lane; i < nvals; i += 64) { v += a.vals[i]; h += a.vals[nvals + i]; }
        v = wave_sum_fixed(v);
        h = wave_sum_fixed(h);
        if (lane == 0) {
            if (total) *total += (float)((double)w * v / (double)n);
            if (top1) *top1 += (float)(h / (double)n);
        }
    }
    if (!dq) return;
    const int row = blockIdx.x * 4 + wave;
    if (row >= n) return;
    const float iq = a.inv[row];
    const int64_t nd = (int64_t)n * d;
    const float* qrow = a.q + (int64_t)row * a.ldq;
    float da[16], av[16];
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        da[c] = av[c] = 0.f;
        if (c * 64 < d) {
            const int k = c * 64 + lane;
            float acc = 0.f;
            for (int s = 0; s < a.splits; ++s) acc += a.slab[(int64_t)s * nd + (int64_t)row * d + k];
            da[c] = acc;
            av[c] = qrow[k] * iq;
            dot += av[c] * acc;
        }
    }
    dot = wave_sum_fixed(dot);
    const float coef = (w * gscale) * (iq / a.tau);
#pragma unroll
    for (int c = 0; c < 16; ++c)
        if (c * 64 < d) {
            const float g = coef * (da[c] - dot * av[c]);
            dq[(int64_t)row * ldd + c * 64 + lane] = iq > 0.f ? g : 0.f;
        }
}

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? OK : E_LAUNCH)

inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

struct NcePlan {
    int tc, splits, nb;
    int64_t off_diag, off_rowp, off_colp, off_lse, off_vals, off_S, off_slab, bytes;
};

NcePlan nce_plan(int n, int d) {
    NcePlan pl;
    pl.tc = (n + 15) / 16;
    pl.nb = (n + 255) / 256;
    int s = (NCE_TARGET_BLOCKS + pl.tc - 1) / pl.tc;
    const int64_t cap = NCE_SLAB_CAP / ((int64_t)n * d);
    if (s > cap) s = (int)cap;
    if (s > pl.tc) s = pl.tc;
    if (s < 1) s = 1;
    pl.splits = s;
    pl.off_diag = align256((int64_t)2 * n * 4);
    pl.off_rowp = pl.off_diag + align256((int64_t)n * 4);
    pl.off_colp = pl.off_rowp + align256((int64_t)s * n * 8);
    pl.off_lse = pl.off_colp + align256((int64_t)pl.tc * n * 8);
    pl.off_vals = pl.off_lse + align256((int64_t)2 * n * 8);
    pl.off_S = pl.off_vals + align256((int64_t)2 * pl.nb * 8);
    pl.off_slab = pl.off_S + align256((int64_t)pl.tc * pl.tc * 1024);
    pl.bytes = pl.off_slab + align256((int64_t)s * n * d * 4);
    return pl;
}

}  // namespace

int64_t latent_nce_ws_bytes(int n, int d) {
    if (n < 2 || n > NCE_MAX_N || d < 64 || d > 1024 || d % 64) return -1;
    return nce_plan(n, d).bytes;
}

int latent_nce_launch(const float* q, int ldq, const float* t, int ldt, int n, int d, float tau, int symmetric, float w,
                      float* total, float* top1, float* dq, int ldd, float gscale, void* ws, int64_t ws_bytes,
                      hipStream_t st) {
    if (latent_nce_ws_bytes(n, d) < 0) return E_UNSUPPORTED;
    const NcePlan pl = nce_plan(n, d);
    if (ws_bytes < pl.bytes) return E_WORKSPACE;
    char* base = (char*)ws;
    NceArgs a;
    a.q = q; a.t = t; a.ldq = ldq; a.ldt = ldt; a.n = n; a.d = d; a.tc = pl.tc; a.splits = pl.splits;
    a.tau = tau; a.ninv = (float)(1.0 / n);
    a.sym = symmetric != 0; a.want_dq = dq != nullptr;
    a.inv = (float*)base;
    a.diag = (float*)(base + pl.off_diag);
    a.rowp = (float2*)(base + pl.off_rowp);
    a.colp = (float2*)(base + pl.off_colp);
    a.lse = (float2*)(base + pl.off_lse);
    a.vals = (double*)(base + pl.off_vals);
    a.S = (float4*)(base + pl.off_S);
    a.slab = (float*)(base + pl.off_slab);

    hipLaunchKernelGGL(nce_norms_kernel, dim3((2 * n + 3) / 4), dim3(256), 0, st, q, ldq, t, ldt, n, d, a.inv);
    const dim3 grid(pl.tc, pl.splits);
    switch (d / 64) {
#define NCE_CASE(NT) case NT: hipLaunchKernelGGL(nce_logits_kernel<NT>, grid, dim3(256), 0, st, a); break;
        NCE_CASE(1) NCE_CASE(2) NCE_CASE(3) NCE_CASE(4) NCE_CASE(5) NCE_CASE(6) NCE_CASE(7) NCE_CASE(8)
        NCE_CASE(9) NCE_CASE(10) NCE_CASE(11) NCE_CASE(12) NCE_CASE(13) NCE_CASE(14) NCE_CASE(15) NCE_CASE(16)
#undef NCE_CASE
        default: return E_UNSUPPORTED;
    }
    hipLaunchKernelGGL(nce_fold_kernel, dim3(pl.nb), dim3(256), 0, st, a);
    if (dq) {
        switch (d / 64) {
#define NCE_CASE(NT) case NT: hipLaunchKernelGGL(nce_weight_kernel<NT>, grid, dim3(256), 0, st, a); break;
            NCE_CASE(1) NCE_CASE(2) NCE_CASE(3) NCE_CASE(4) NCE_CASE(5) NCE_CASE(6) NCE_CASE(7) NCE_CASE(8)
            NCE_CASE(9) NCE_CASE(10) NCE_CASE(11) NCE_CASE(12) NCE_CASE(13) NCE_CASE(14) NCE_CASE(15) NCE_CASE(16)
#undef NCE_CASE
            default: return E_UNSUPPORTED;
        }
    }
    hipLaunchKernelGGL(nce_finalize_kernel, dim3(dq ? (n + 3) / 4 : 1), dim3(256), 0, st, a, pl.nb, w, gscale, total,
                       top1, dq, ldd);
    return LAUNCH_OK();
}

}  // namespace fmri
