// Pairwise similarity of n-way identification (the reference's objective_assessment, train/train_utils.py:752-816):
// every reconstruction against every ground-truth image (or a list of such pairs), PCC (PearsonCorrelation.forward,
// :276-292, over one image) and mean SSIM (StructuralSimilarity.forward, :343-420), fp32 in.
//
//   PCC [N x M]
//     ident_rowstats_kernel  one block per row of pred / truth: fp64 mean, then the fp64 sum of (x - mean)^2 of the
//                            fp32-centred row; fixed-order block sums
//     ident_gram_kernel      one wave per (16 x 16 tile, K chunk of PCC_KC): centred Gram tile with
//                            v_mfma_f32_16x16x4_f32, each operand centred as it is loaded, fp32 over 16 k, then fp64
//     ident_pcc_final_kernel S_ij = sum over the chunks in chunk order (fp64) / (|vx_i| |vy_j|)
//   SSIM of a pair list (fp32 images in, every filtered statistic and the SSIM map in fp64, window built in fp64)
//     ident_ssim_stats_kernel   Gaussian-filtered x and x^2 of every image plane, once per image, into the workspace
//     ident_ssim_pair_kernel    one block per pair: the filtered cross term G * (x_i y_j) in separable form in LDS,
//                               tile by tile in a fixed order, fp64 per-thread sums, fixed-order block sum
//   The variances E[x^2] - mu^2 cancel: in fp32, windows where |x| = 1 almost everywhere (a saturated output against a
//   flat background) lose ~1e-7 against C2 = 9e-4, and a pair's mean SSIM was 2e-5 from the exact value.  In fp64 they
//   are exact to ~1e-12.
//
// A pair's value is a bitwise function of the two images alone: the chunking depends on D only, the tile order on
// (C, H, W) only, and there are no atomics.  Two calls are bit-identical, a pair's value does not depend on its
// position in the list, on N, M or P, and truth_j == truth_i bitwise gives S_ij == S_ii bitwise.
#include "kernels.h"
#include "ssim_window.h"

namespace fmri {

namespace {

constexpr int PCC_KC = 1024;      // K chunk of the Gram: fixed, so a pair's partial sums depend on D only

__global__ __launch_bounds__(256) void ident_rowstats_kernel(const float* __restrict__ pred, int N,
                                                             const float* __restrict__ truth, int M, int64_t D,
                                                             float* __restrict__ mean, double* __restrict__ norm) {
    __shared__ double sh[4];
    const int row = blockIdx.x;
    const float* x = row < N ? pred + (int64_t)row * D : truth + (int64_t)(row - N) * D;
    double s = 0.0;
    for (int64_t k = threadIdx.x; k < D; k += 256) s += (double)x[k];
    s = block_sum_fixed(s, sh);
    const float m = (float)(s / (double)D);
    double q = 0.0;
    for (int64_t k = threadIdx.x; k < D; k += 256) {
        const double c = (double)(x[k] - m);
        q += c * c;
    }
    q = block_sum_fixed(q, sh);
    if (threadIdx.x == 0) {
        mean[row] = m;
        norm[row] = sqrt(q);
    }
}

// grid (ceil(N/16), ceil(M/16), chunks), one wave.  Lane (lr, lg) feeds row lr of A (pred) and column lr of B (truth)
// with k = kb + 4 lg + e in the e-th MFMA of a 16-step: both operands use the same k order, so every element of the
// tile is the same k-ordered chain whatever its position.  Out-of-range k and rows enter as exact zeros.  Each 16-step
// starts a fresh fp32 chain and is added to an fp64 sum: one fp32 chain over the whole chunk grows with the partial
// sum of a correlated pair and was 5e-6 from fp64 at D = 30000.
__global__ __launch_bounds__(64) void ident_gram_kernel(const float* __restrict__ pred, int N,
                                                        const float* __restrict__ truth, int M, int64_t D,
                                                        const float* __restrict__ mean, float* __restrict__ part) {
    const int lane = threadIdx.x, lr = lane & 15, lg = lane >> 4;
    const int ra = blockIdx.x * 16 + lr, cb = blockIdx.y * 16 + lr;
    const int64_t k0 = (int64_t)blockIdx.z * PCC_KC;
    const int64_t k1 = k0 + PCC_KC < D ? k0 + PCC_KC : D;
    const bool va = ra < N, vb = cb < M;
    const float* xa = pred + (int64_t)(va ? ra : 0) * D;
    const float* xb = truth + (int64_t)(vb ? cb : 0) * D;
    const float ma = va ? mean[ra] : 0.f, mb = vb ? mean[N + cb] : 0.f;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t kb = k0; kb < k1; kb += 16) {     // wave-uniform trip count: every lane issues every MFMA
        f4 g = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t kk = kb + 4 * lg + e;
            const float a = va && kk < k1 ? xa[kk] - ma : 0.f;
            const float b = vb && kk < k1 ? xb[kk] - mb : 0.f;
            g = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, g, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += (double)g[r];
    }
    // C/D layout: column lane & 15, row 4 (lane >> 4) + r
    const int gj = blockIdx.y * 16 + lr;
    float* out = part + (int64_t)blockIdx.z * N * M;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int gi = blockIdx.x * 16 + lg * 4 + r;
        if (gi < N && gj < M) out[(int64_t)gi * M + gj] = (float)acc[r];
    }
}

__global__ __launch_bounds__(256) void ident_pcc_final_kernel(const float* __restrict__ part, int chunks, int N, int M,
                                                              const double* __restrict__ norm, float* __restrict__ S,
                                                              int ldS) {
    const int64_t nm = (int64_t)N * M;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < nm; e += (int64_t)gridDim.x * 256) {
        const int i = (int)(e / M), j = (int)(e - (int64_t)i * M);
        double g = 0.0;
        for (int c = 0; c < chunks; ++c) g += (double)part[(int64_t)c * nm + e];
        S[(int64_t)i * ldS + j] = (float)(g / (norm[i] * norm[N + j]));
    }
}

// grid (images * C, ceil(H/16), ceil(W/16)): filtered x (mu) and x^2 (e) of one 16 x 16 tile of one plane, zero padding
__global__ __launch_bounds__(256) void ident_ssim_stats_kernel(const float* __restrict__ pred, int N,
                                                               const float* __restrict__ truth, int C, int H, int W,
                                                               double* __restrict__ mu, double* __restrict__ ex) {
    __shared__ float t[SS_R][SS_R + 1];
    __shared__ double hx[2][SS_R][SS_TS + 1];
    __shared__ double g[SS_WIN];
    const int tx0 = blockIdx.z * SS_TS, ty0 = blockIdx.y * SS_TS;
    const int plane = blockIdx.x;
    const int64_t hw = (int64_t)H * W;
    const float* src = plane < N * C ? pred + (int64_t)plane * hw : truth + (int64_t)(plane - N * C) * hw;
    gauss11(g);
    for (int e = threadIdx.x; e < SS_R * SS_R; e += 256) {
        const int j = e / SS_R, i = e - j * SS_R;
        const int y = ty0 - SS_PAD + j, x = tx0 - SS_PAD + i;
        t[j][i] = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W ? src[(int64_t)y * W + x] : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < SS_R * SS_TS; e += 256) {
        const int j = e / SS_TS, i = e - j * SS_TS;
        double s0 = 0.0, s1 = 0.0;
        for (int k = 0; k < SS_WIN; ++k) {
            const double w = g[k], u = t[j][i + k];
            s0 += w * u;
            s1 += w * (u * u);
        }
        hx[0][j][i] = s0;
        hx[1][j][i] = s1;
    }
    __syncthreads();
    const int oy = threadIdx.x >> 4, ox = threadIdx.x & 15;
    const int y = ty0 + oy, x = tx0 + ox;
    if (y < H && x < W) {
        double m = 0.0, q = 0.0;
        for (int k = 0; k < SS_WIN; ++k) {
            m += g[k] * hx[0][oy + k][ox];
            q += g[k] * hx[1][oy + k][ox];
        }
        mu[(int64_t)plane * hw + (int64_t)y * W + x] = m;
        ex[(int64_t)plane * hw + (int64_t)y * W + x] = q;
    }
}

// one block per pair; mu / ex hold the N pred planes, then the M truth planes
__global__ __launch_bounds__(256) void ident_ssim_pair_kernel(const float* __restrict__ pred, int N,
                                                              const float* __restrict__ truth, int M, int C, int H,
                                                              int W, const int* __restrict__ pairs,
                                                              const double* __restrict__ mu,
                                                              const double* __restrict__ ex, float* __restrict__ out) {
    __shared__ double t[SS_R][SS_R + 1];
    __shared__ double hx[SS_R][SS_TS + 1];
    __shared__ double g[SS_WIN];
    __shared__ double sh[4];
    const int p = blockIdx.x;
    const int pi = pairs[2 * p], pj = pairs[2 * p + 1];
    if (pi < 0 || pi >= N || pj < 0 || pj >= M) {    // checked by the caller; never read outside the images
        if (threadIdx.x == 0) out[p] = __builtin_nanf("");
        return;
    }
    gauss11(g);
    const int64_t hw = (int64_t)H * W;
    const int tw = (W + SS_TS - 1) / SS_TS, th = (H + SS_TS - 1) / SS_TS;
    const int oy = threadIdx.x >> 4, ox = threadIdx.x & 15;
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    double acc = 0.0;
    for (int c = 0; c < C; ++c) {
        const int64_t pa = ((int64_t)pi * C + c) * hw, pb = ((int64_t)pj * C + c) * hw;
        const int64_t sa = pa, sb = ((int64_t)(N + pj) * C + c) * hw;
        for (int ty = 0; ty < th; ++ty)
            for (int tx = 0; tx < tw; ++tx) {
                const int tx0 = tx * SS_TS, ty0 = ty * SS_TS;
                __syncthreads();        // t / hx of the previous tile are consumed
                for (int e = threadIdx.x; e < SS_R * SS_R; e += 256) {
                    const int j = e / SS_R, i = e - j * SS_R;
                    const int y = ty0 - SS_PAD + j, x = tx0 - SS_PAD + i;
                    const int64_t o = (int64_t)y * W + x;
                    t[j][i] = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W   // exact product in fp64
                                  ? (double)pred[pa + o] * (double)truth[pb + o] : 0.0;
                }
                __syncthreads();
                for (int e = threadIdx.x; e < SS_R * SS_TS; e += 256) {
                    const int j = e / SS_TS, i = e - j * SS_TS;
                    double s = 0.0;
                    for (int k = 0; k < SS_WIN; ++k) s += g[k] * t[j][i + k];
                    hx[j][i] = s;
                }
                __syncthreads();
                const int y = ty0 + oy, x = tx0 + ox;
                if (y < H && x < W) {
                    double e12 = 0.0;
                    for (int k = 0; k < SS_WIN; ++k) e12 += g[k] * hx[oy + k][ox];
                    const int64_t o = (int64_t)y * W + x;
                    const double m1 = mu[sa + o], m2 = mu[sb + o], e11 = ex[sa + o], e22 = ex[sb + o];
                    const double m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
                    const double s1 = e11 - m11, s2 = e22 - m22, s12 = e12 - m12;
                    acc += ((2.0 * m12 + C1) * (2.0 * s12 + C2)) / ((m11 + m22 + C1) * (s1 + s2 + C2));
                }
            }
    }
    acc = block_sum_fixed(acc, sh);
    if (threadIdx.x == 0) out[p] = (float)(acc / (double)((int64_t)C * hw));
}

inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

}  // namespace

int64_t pcc_matrix_ws_bytes(int N, int M, int64_t D) {
    if (N < 1 || M < 1 || D < 1) return -1;
    const int64_t chunks = (D + PCC_KC - 1) / PCC_KC;
    return align256((int64_t)(N + M) * 4) + align256((int64_t)(N + M) * 8) + align256(chunks * N * M * 4);
}

int pcc_matrix_launch(const float* pred, const float* truth, int N, int M, int64_t D, float* S, int ldS, void* ws,
                      int64_t ws_bytes, hipStream_t st) {
    if (ws_bytes < pcc_matrix_ws_bytes(N, M, D)) return E_WORKSPACE;
    const int chunks = (int)((D + PCC_KC - 1) / PCC_KC);
    char* base = (char*)ws;
    float* mean = (float*)base;
    double* norm = (double*)(base + align256((int64_t)(N + M) * 4));
    float* part = (float*)(base + align256((int64_t)(N + M) * 4) + align256((int64_t)(N + M) * 8));
    hipLaunchKernelGGL(ident_rowstats_kernel, dim3(N + M), dim3(256), 0, st, pred, N, truth, M, D, mean, norm);
    hipLaunchKernelGGL(ident_gram_kernel, dim3((N + 15) / 16, (M + 15) / 16, chunks), dim3(64), 0, st, pred, N, truth,
                       M, D, (const float*)mean, part);
    int64_t fg = ((int64_t)N * M + 255) / 256;
    if (fg > 4096) fg = 4096;
    hipLaunchKernelGGL(ident_pcc_final_kernel, dim3((int)fg), dim3(256), 0, st, (const float*)part, chunks, N, M,
                       (const double*)norm, S, ldS);
    return hipGetLastError() == hipSuccess ? OK : E_LAUNCH;
}

int64_t ssim_pairs_ws_bytes(int N, int M, int C, int H, int W) {
    if (N < 1 || M < 1 || C < 1 || H < 1 || W < 1) return -1;
    return 2 * align256((int64_t)(N + M) * C * H * W * 8);
}

int ssim_pairs_launch(const float* pred, const float* truth, int N, int M, int C, int H, int W, const int* pairs, int P,
                      float* out, void* ws, int64_t ws_bytes, hipStream_t st) {
    if (ws_bytes < ssim_pairs_ws_bytes(N, M, C, H, W)) return E_WORKSPACE;
    if (P == 0) return OK;
    const int64_t one = align256((int64_t)(N + M) * C * H * W * 8);
    double* mu = (double*)ws;
    double* ex = (double*)((char*)ws + one);
    hipLaunchKernelGGL(ident_ssim_stats_kernel, dim3((N + M) * C, (H + SS_TS - 1) / SS_TS, (W + SS_TS - 1) / SS_TS),
                       dim3(256), 0, st, pred, N, truth, C, H, W, mu, ex);
    hipLaunchKernelGGL(ident_ssim_pair_kernel, dim3(P), dim3(256), 0, st, pred, N, truth, M, C, H, W, pairs,
                       (const double*)mu, (const double*)ex, out);
    return hipGetLastError() == hipSuccess ? OK : E_LAUNCH;
}

}  // namespace fmri
