// n-way identification of one batch in the engine's own image layout (fp16 [n][H][W][8], channels 0..C-1 real), for the
// validation pass of the fused steps (fmri_hip/evaluate.py; include/fmri_hip.h fmri_nway_scores): the reference's
// objective_assessment (train/train_utils.py:752-816) with the similarity matrices, the distractor draws, the counting
// and the running score all on the device.  The definitions are those of ident.hip, applied to the fp32 values of the
// fp16 elements; five launches per call, whatever n is:
//
//   nway_stats_kernel   one block per image (n pred, then n truth): one 16-byte load per pixel of a 26 x 26 halo tile;
//                       per channel the Gaussian-filtered x (mu) and x^2 (ex) in fp64, and a planar fp32 copy
//                       [image][c][y][x] that the next two launches read without the five dead lanes; then the image's
//                       fp64 mean and the fp64 norm of its fp32-centred elements.
//   nway_gram_kernel    grid (n/16, n/16, K chunks of 1024): both operands of a 16 x 16 tile go through LDS, 256 k at a
//                       time, centred as they are stored.  Wave w takes k = 64 w .. 64 w + 63 of every 256: fresh fp32
//                       chains of 16 k from v_mfma_f32_16x16x4_f32, summed in fp64; the four waves in wave order.
//   nway_ssim_kernel    blocked like a GEMM: a block owns one 16 x 16 tile of one channel for 16 pred x 8 truth images.
//                       The truth halo tiles and their mu / ex tiles are loaded into LDS once per block, a wave keeps its
//                       pred image's halo row and statistics in registers over the 8 truths.  Per pair the wave forms
//                       the cross term x_i y_j (exact), filters it separably in fp64 through a wave-private LDS tile
//                       and sums the SSIM map of the tile: one fp64 partial per (tile, channel, pair).
//   nway_rows_kernel    one block per pred image i: S_pcc[i][:] and S_ssim[i][:] from the partials in a fixed order,
//                       the counts #{j != i : S_ij < S_ii}, the distractors d[i][k] (Philox, the mapping of
//                       fmri_rng_u32) and whether S_ii beats all of them, the term (count / (n - 1))^(top - 1).
//   nway_fold_kernel    the rows in index order, the accumulator and out8.
//
// No atomics, no allocation, no memset, no host sync.  A pair's value is a bitwise function of its two images and
// (C, H, W) only: the statistics of an image depend on that image alone, the K chunking on D, the tile and channel order
// on (C, H, W), and the arithmetic of a pair on nothing that depends on its place in a group.  Wherever S_ii or S_id is
// needed again (the count, the hits) it is re-formed by the same function of the same partials, so it has the same bits.
#include "kernels.h"
#include "philox.h"
#include "ssim_window.h"

namespace fmri {

namespace {

constexpr int NW_CMAX = 4;          // real channels the workspace is sized for (fmri_nway_ws_bytes has no C)
constexpr int NW_KC = 1024;         // K chunk of the Gram: fixed, so a pair's partial sums depend on D only
constexpr int NW_KS = 256;          // k staged in LDS at a time
constexpr int NW_LD = NW_KS + 4;    // LDS row stride of a staged operand (floats; rows stay 16-byte aligned)
constexpr int NW_GP = 16;           // pred images per SSIM block (4 per wave)
constexpr int NW_GT = 8;            // truth images per SSIM block
constexpr int NW_HL = 52;           // lanes of the horizontal pass: 26 halo rows x 2 halves of 8 columns

inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }
inline int tiles_of(int H, int W) { return ((H + SS_TS - 1) / SS_TS) * ((W + SS_TS - 1) / SS_TS); }

struct NwayWs {
    float* x;           // [2n][C][H][W]
    double *mu, *ex;    // [2n][C][H][W]
    float* mean;        // [2n]
    double* norm;       // [2n]
    double* gpart;      // [chunks][n][n]
    double* spart;      // [C tiles][n][n]
    double* rows;       // [n][4]: hit_pcc, hit_ssim, term_pcc, term_ssim
    int64_t bytes;
};

// the layout for C real channels; sized with C = NW_CMAX it is the workspace requirement
NwayWs nway_ws(void* ws, int n, int H, int W, int C) {
    const int64_t el = (int64_t)2 * n * C * H * W, D = (int64_t)C * H * W, nn = (int64_t)n * n;
    const uintptr_t p = (uintptr_t)ws;      // (ws = NULL: only the size is wanted)
    int64_t o = 0;
    NwayWs w;
    w.mu = (double*)(p + o);    o += align256(el * 8);
    w.ex = (double*)(p + o);    o += align256(el * 8);
    w.x = (float*)(p + o);      o += align256(el * 4);
    w.norm = (double*)(p + o);  o += align256((int64_t)2 * n * 8);
    w.mean = (float*)(p + o);   o += align256((int64_t)2 * n * 4);
    w.gpart = (double*)(p + o); o += align256((D + NW_KC - 1) / NW_KC * nn * 8);
    w.spart = (double*)(p + o); o += align256((int64_t)C * tiles_of(H, W) * nn * 8);
    w.rows = (double*)(p + o);  o += align256((int64_t)n * 4 * 8);
    w.bytes = o;
    return w;
}

// ---- statistics ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nway_stats_kernel(const uint4* __restrict__ pred, const uint4* __restrict__ truth,
                                                         int n, int H, int W, int C, float* __restrict__ xp,
                                                         double* __restrict__ mu, double* __restrict__ ex,
                                                         float* __restrict__ mean, double* __restrict__ norm) {
    __shared__ __attribute__((aligned(16))) half_t raw[SS_R * SS_R][8];
    __shared__ float t[SS_R][SS_R + 1];
    __shared__ double hx[2][SS_R][SS_TS + 1];
    __shared__ double g[SS_WIN];
    __shared__ double sh[4];
    const int img = blockIdx.x;
    const int64_t hw = (int64_t)H * W;
    const uint4* src = img < n ? pred + (int64_t)img * hw : truth + (int64_t)(img - n) * hw;
    gauss11(g);
    const int tw = (W + SS_TS - 1) / SS_TS, th = (H + SS_TS - 1) / SS_TS;
    const int oy = threadIdx.x >> 4, ox = threadIdx.x & 15;
    double s = 0.0;
    for (int ty = 0; ty < th; ++ty)
        for (int tx = 0; tx < tw; ++tx) {
            const int tx0 = tx * SS_TS, ty0 = ty * SS_TS;
            // (raw of the previous tile was last read two barriers ago)
            for (int e = threadIdx.x; e < SS_R * SS_R; e += 256) {
                const int j = e / SS_R, i = e - j * SS_R;
                const int y = ty0 - SS_PAD + j, x = tx0 - SS_PAD + i;
                if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W)     // pixels outside are never read back
                    *(uint4*)raw[e] = src[(int64_t)y * W + x];
            }
            for (int c = 0; c < C; ++c) {
                __syncthreads();        // raw is written / t and hx of the previous channel are consumed
                for (int e = threadIdx.x; e < SS_R * SS_R; e += 256) {
                    const int j = e / SS_R, i = e - j * SS_R;
                    const int y = ty0 - SS_PAD + j, x = tx0 - SS_PAD + i;
                    t[j][i] = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W ? (float)raw[e][c] : 0.f;
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
                const int y = ty0 + oy, x = tx0 + ox;
                if (y < H && x < W) {
                    double m = 0.0, q = 0.0;
                    for (int k = 0; k < SS_WIN; ++k) {
                        m += g[k] * hx[0][oy + k][ox];
                        q += g[k] * hx[1][oy + k][ox];
                    }
                    const int64_t o = ((int64_t)img * C + c) * hw + (int64_t)y * W + x;
                    const float v = t[oy + SS_PAD][ox + SS_PAD];
                    mu[o] = m;
                    ex[o] = q;
                    xp[o] = v;
                    s += (double)v;
                }
            }
        }
    s = block_sum_fixed(s, sh);
    const float m = (float)(s / (double)((int64_t)C * hw));
    double q = 0.0;
    for (int64_t p = threadIdx.x; p < hw; p += 256) {
        union {
            uint4 u;
            half_t h[8];
        } v;
        v.u = src[p];
#pragma unroll
        for (int c = 0; c < NW_CMAX; ++c) {
            const double d = (double)((float)v.h[c] - m);      // the fp32 centring the Gram applies
            q += c < C ? d * d : 0.0;
        }
    }
    q = block_sum_fixed(q, sh);
    if (threadIdx.x == 0) {
        mean[img] = m;
        norm[img] = sqrt(q);
    }
}

// ---- PCC: the centred Gram ----------------------------------------------------------------------------------------------
// Lane (lr, lg) of a wave feeds row lr of A (pred) and column lr of B (truth) with k = kb + 4 lg + e in the e-th MFMA
// of a 16-step, one 16-byte LDS read per operand and step.  Rows past n and k past D enter as exact zeros.  Every 16-step
// starts a fresh fp32 chain (ident.hip: one chain over a chunk was 5e-6 from fp64 at D = 30000).
__global__ __launch_bounds__(256) void nway_gram_kernel(const float* __restrict__ xp, int n, int64_t D,
                                                        const float* __restrict__ mean, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sa[16][NW_LD];
    __shared__ __attribute__((aligned(16))) float sb[16][NW_LD];
    __shared__ float sm[2][16];
    __shared__ double red[4][4][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lg = lane >> 4;
    const int i0 = blockIdx.x * 16, j0 = blockIdx.y * 16;
    const int64_t k0 = (int64_t)blockIdx.z * NW_KC;
    const int64_t k1 = k0 + NW_KC < D ? k0 + NW_KC : D;
    if (tid < 32) {
        const int r = tid & 15, row = tid < 16 ? i0 + r : j0 + r;
        sm[tid >> 4][r] = row < n ? mean[tid < 16 ? row : n + row] : 0.f;
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t ks = k0; ks < k1; ks += NW_KS) {          // block-uniform trip count
        __syncthreads();        // sm is written / sa and sb of the previous step are consumed
        const int64_t k = ks + tid;
#pragma unroll 4
        for (int r = 0; r < 16; ++r) {
            const bool va = i0 + r < n && k < k1, vb = j0 + r < n && k < k1;
            sa[r][tid] = va ? xp[(int64_t)(i0 + r) * D + k] - sm[0][r] : 0.f;
            sb[r][tid] = vb ? xp[(int64_t)(n + j0 + r) * D + k] - sm[1][r] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int kb = wave * 64 + s * 16 + 4 * lg;
            const f4 a = *(const f4*)&sa[lr][kb], b = *(const f4*)&sb[lr][kb];
            f4 gq = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) gq = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], gq, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] += (double)gq[r];
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][r][lane] = acc[r];
    __syncthreads();
    if (wave == 0) {
        // C/D layout: column lane & 15, row 4 (lane >> 4) + r
        const int gj = j0 + lr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gi = i0 + lg * 4 + r;
            if (gi < n && gj < n)
                part[((int64_t)blockIdx.z * n + gi) * n + gj] =
                    ((red[0][r][lane] + red[1][r][lane]) + red[2][r][lane]) + red[3][r][lane];
        }
    }
}

// ---- SSIM of every pair -------------------------------------------------------------------------------------------------
// grid (C tiles, ceil(n / NW_GT), ceil(n / NW_GP)).  Horizontal pass: lane l < 52 owns halo row l % 26 and the 8 output
// columns of half l / 26: 18 products, 8 x 11 fma, into the wave's own hx tile.  Vertical pass: lane l owns column l & 15
// and the 4 rows 4 (l >> 4) ..: 14 reads of hx, 4 x 11 fma, 4 pixels of the SSIM map.  All four waves run the same trip
// counts; a wave whose pred image is past n only skips the arithmetic.  hx[wave] is written and read by its own wave
// only, so between the two passes of a pair no block barrier is needed (wave_sync_lds): the four waves drift apart and
// one wave's horizontal pass overlaps another's vertical pass and divisions.
// Orders the LDS traffic of ONE wave: the hardware executes a wave's LDS instructions in order, so data one lane stored
// is there for another lane's later load; this only keeps the compiler from moving either across the point.
__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(256) void nway_ssim_kernel(const float* __restrict__ xp, const double* __restrict__ mu,
                                                        const double* __restrict__ ex, int n, int C, int H, int W,
                                                        double* __restrict__ part) {
    __shared__ float tt[NW_GT][SS_R][SS_R + 1];
    __shared__ double ts[NW_GT][2][SS_TS * SS_TS];
    __shared__ double hx[4][SS_R][SS_TS + 1];
    __shared__ double g[SS_WIN];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tw = (W + SS_TS - 1) / SS_TS, tiles = tw * ((H + SS_TS - 1) / SS_TS);
    const int tc = blockIdx.x, c = tc / tiles, tile = tc - c * tiles;
    const int ty0 = (tile / tw) * SS_TS, tx0 = (tile % tw) * SS_TS;
    const int j0 = blockIdx.y * NW_GT, i0 = blockIdx.z * NW_GP;
    const int nt = n - j0 < NW_GT ? n - j0 : NW_GT;
    const int64_t hw = (int64_t)H * W;
    gauss11(g);
    for (int e = tid; e < nt * SS_R * SS_R; e += 256) {
        const int tj = e / (SS_R * SS_R), r = e - tj * (SS_R * SS_R), j = r / SS_R, i = r - j * SS_R;
        const int y = ty0 - SS_PAD + j, x = tx0 - SS_PAD + i;
        tt[tj][j][i] = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W
                           ? xp[((int64_t)(n + j0 + tj) * C + c) * hw + (int64_t)y * W + x] : 0.f;
    }
    for (int e = tid; e < nt * SS_TS * SS_TS; e += 256) {
        const int tj = e >> 8, p = e & 255, y = ty0 + (p >> 4), x = tx0 + (p & 15);
        const bool in = y < H && x < W;
        const int64_t o = ((int64_t)(n + j0 + tj) * C + c) * hw + (int64_t)y * W + x;
        ts[tj][0][p] = in ? mu[o] : 0.0;
        ts[tj][1][p] = in ? ex[o] : 0.0;
    }
    __syncthreads();
    double gr[SS_WIN];
#pragma unroll
    for (int k = 0; k < SS_WIN; ++k) gr[k] = g[k];
    const int hh = lane / SS_R, hj = lane - hh * SS_R;       // horizontal pass (lane < NW_HL)
    const int ox = lane & 15, oy0 = (lane >> 4) * 4;         // vertical pass
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    for (int pi = 0; pi < NW_GP / 4; ++pi) {
        const int i = i0 + wave + 4 * pi;
        const bool vi = i < n;                               // wave-uniform
        float pa[18];
        double pm[4], pe[4];
        if (vi) {
            const int64_t base = ((int64_t)i * C + c) * hw;
            if (lane < NW_HL) {
                const int y = ty0 - SS_PAD + hj;
#pragma unroll
                for (int k = 0; k < 18; ++k) {
                    const int x = tx0 - SS_PAD + hh * 8 + k;
                    pa[k] = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W ? xp[base + (int64_t)y * W + x] : 0.f;
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int y = ty0 + oy0 + r, x = tx0 + ox;
                const bool in = y < H && x < W;
                pm[r] = in ? mu[base + (int64_t)y * W + x] : 0.0;
                pe[r] = in ? ex[base + (int64_t)y * W + x] : 0.0;
            }
        }
        for (int tj = 0; tj < nt; ++tj) {
            wave_sync_lds();        // hx of the previous pair is consumed
            if (vi && lane < NW_HL) {
                double p[18];
#pragma unroll
                for (int k = 0; k < 18; ++k)      // fp16 x fp16: 22 significant bits, exact in fp32
                    p[k] = (double)(pa[k] * tt[tj][hj][hh * 8 + k]);
#pragma unroll
                for (int o = 0; o < 8; ++o) {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < SS_WIN; ++k) s = fma(gr[k], p[o + k], s);
                    hx[wave][hj][hh * 8 + o] = s;
                }
            }
            wave_sync_lds();
            if (vi) {
                double col[SS_WIN + 3];
#pragma unroll
                for (int k = 0; k < SS_WIN + 3; ++k) col[k] = hx[wave][oy0 + k][ox];
                double acc = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double e12 = 0.0;
#pragma unroll
                    for (int k = 0; k < SS_WIN; ++k) e12 = fma(gr[k], col[r + k], e12);
                    const int p = (oy0 + r) * SS_TS + ox;
                    const double m1 = pm[r], e11 = pe[r], m2 = ts[tj][0][p], e22 = ts[tj][1][p];
                    const double m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
                    const double s1 = e11 - m11, s2 = e22 - m22, s12 = e12 - m12;
                    const double v = ((2.0 * m12 + C1) * (2.0 * s12 + C2)) / ((m11 + m22 + C1) * (s1 + s2 + C2));
                    acc += ty0 + oy0 + r < H && tx0 + ox < W ? v : 0.0;
                }
                for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
                if (lane == 0) part[((int64_t)tc * n + i) * n + (j0 + tj)] = acc;
            }
        }
    }
}

// ---- rows: matrices, counts, draws, hits --------------------------------------------------------------------------------
struct NwayPartials {
    const double *gpart, *spart, *norm;
    int chunks, tcs, n;
    double count;       // C H W
};

// S_pcc[i][j], S_ssim[i][j]: the partials in chunk / (channel, tile) order -- the same bits wherever it is called
__device__ __forceinline__ void nway_pair(const NwayPartials& q, int i, int j, float& pcc, float& ssim) {
    const int64_t nn = (int64_t)q.n * q.n, e = (int64_t)i * q.n + j;
    double gs = 0.0, ss = 0.0;
    for (int k = 0; k < q.chunks; ++k) gs += q.gpart[k * nn + e];
    for (int k = 0; k < q.tcs; ++k) ss += q.spart[k * nn + e];
    pcc = (float)(gs / (q.norm[i] * q.norm[q.n + j]));
    ssim = (float)(ss / q.count);
}

__global__ __launch_bounds__(256) void nway_rows_kernel(NwayPartials q, int top, const int64_t* __restrict__ state,
                                                        uint32_t sid, float* __restrict__ s_pcc,
                                                        float* __restrict__ s_ssim, int32_t* __restrict__ distractors,
                                                        double* __restrict__ rows) {
    __shared__ double sh[4];
    const int i = blockIdx.x, n = q.n;
    float dp, ds;
    nway_pair(q, i, i, dp, ds);
    double cp = 0.0, cs = 0.0;      // #{j != i: S_ij < S_ii}: NaN compares false
    for (int j = threadIdx.x; j < n; j += 256) {
        float p, s;
        nway_pair(q, i, j, p, s);
        s_pcc[(int64_t)i * n + j] = p;
        s_ssim[(int64_t)i * n + j] = s;
        if (j != i) {
            cp += p < dp ? 1.0 : 0.0;
            cs += s < ds ? 1.0 : 0.0;
        }
    }
    cp = block_sum_fixed(cp, sh);
    cs = block_sum_fixed(cs, sh);
    double lp = 0.0, ls = 0.0;      // draws the ground truth does not strictly beat
    if (state) {
        for (int k = threadIdx.x; k < top - 1; k += 256) {
            const uint64_t e = (uint64_t)i * (uint64_t)(top - 1) + (uint64_t)k;
            const u32x4 b = rng_block(state, e >> 2, sid);
            const uint32_t w = (e & 2) ? ((e & 1) ? b.w[3] : b.w[2]) : ((e & 1) ? b.w[1] : b.w[0]);
            const uint32_t u = (uint32_t)(((uint64_t)w * (uint64_t)(n - 1)) >> 32);
            const int d = (int)u + (u >= (uint32_t)i ? 1 : 0);
            if (distractors) distractors[e] = d;
            float p, s;
            nway_pair(q, i, d, p, s);
            lp += dp > p ? 0.0 : 1.0;
            ls += ds > s ? 0.0 : 1.0;
        }
        lp = block_sum_fixed(lp, sh);
        ls = block_sum_fixed(ls, sh);
    }
    if (threadIdx.x == 0) {
        const double qp = cp / (double)(n - 1), qs = cs / (double)(n - 1);
        double tp = 1.0, tsv = 1.0;
        for (int k = 0; k < top - 1; ++k) {
            tp *= qp;
            tsv *= qs;
        }
        const double nan = __builtin_nan("");
        rows[4 * (int64_t)i + 0] = state ? (lp == 0.0 ? 1.0 : 0.0) : nan;
        rows[4 * (int64_t)i + 1] = state ? (ls == 0.0 ? 1.0 : 0.0) : nan;
        rows[4 * (int64_t)i + 2] = tp;
        rows[4 * (int64_t)i + 3] = tsv;
    }
}

// threads 0..3 each sum one column of rows in index order; thread 0 then updates the accumulator and writes out8
__global__ __launch_bounds__(64) void nway_fold_kernel(const double* __restrict__ rows, int n, float* __restrict__ out8,
                                                       double* __restrict__ acc, int acc_mode) {
    __shared__ double stage[64][4], tot[4];
    double s = 0.0;
    for (int i0 = 0; i0 < n; i0 += 64) {            // 64 rows per step into LDS, then summed in index order
        __syncthreads();
        if (i0 + (int)threadIdx.x < n)
            for (int k = 0; k < 4; ++k) stage[threadIdx.x][k] = rows[4 * (int64_t)(i0 + threadIdx.x) + k];
        __syncthreads();
        if (threadIdx.x < 4)
            for (int i = 0; i < 64 && i0 + i < n; ++i) s += stage[i][threadIdx.x];
    }
    if (threadIdx.x < 4) tot[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x) return;
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (acc_mode)
        for (int k = 0; k < 6; ++k) a[k] = acc[k];
    for (int k = 0; k < 4; ++k) {
        a[k] += tot[k];
        out8[k] = (float)(tot[k] / (double)n);
    }
    a[4] += (double)n;
    a[5] += 1.0;
    for (int k = 0; k < 6; ++k) acc[k] = a[k];
    for (int k = 0; k < 4; ++k) out8[4 + k] = (float)(a[k] / a[4]);
}

}  // namespace

int nway_cmax() { return NW_CMAX; }

int64_t nway_ws_bytes(int n, int H, int W) {
    if (n < 1 || H < 1 || W < 1) return -1;
    return nway_ws(nullptr, n, H, W, NW_CMAX).bytes;
}

int nway_scores_launch(const half_t* pred, const half_t* truth, int n, int H, int W, int C, int top,
                       const int64_t* rng_state, int sid, void* ws, int64_t ws_bytes, float* s_pcc, float* s_ssim,
                       int32_t* distractors, float* out8, double* acc6, int acc_mode, hipStream_t st) {
    if (C > NW_CMAX) return E_UNSUPPORTED;
    if (ws_bytes < nway_ws_bytes(n, H, W)) return E_WORKSPACE;
    const NwayWs w = nway_ws(ws, n, H, W, C);
    const int64_t D = (int64_t)C * H * W;
    const int chunks = (int)((D + NW_KC - 1) / NW_KC), tcs = C * tiles_of(H, W);
    hipLaunchKernelGGL(nway_stats_kernel, dim3(2 * n), dim3(256), 0, st, (const uint4*)pred, (const uint4*)truth, n, H, W,
                       C, w.x, w.mu, w.ex, w.mean, w.norm);
    hipLaunchKernelGGL(nway_gram_kernel, dim3((n + 15) / 16, (n + 15) / 16, chunks), dim3(256), 0, st,
                       (const float*)w.x, n, D, (const float*)w.mean, w.gpart);
    hipLaunchKernelGGL(nway_ssim_kernel, dim3(tcs, (n + NW_GT - 1) / NW_GT, (n + NW_GP - 1) / NW_GP), dim3(256), 0, st,
                       (const float*)w.x, (const double*)w.mu, (const double*)w.ex, n, C, H, W, w.spart);
    const NwayPartials q = {w.gpart, w.spart, w.norm, chunks, tcs, n, (double)D};
    hipLaunchKernelGGL(nway_rows_kernel, dim3(n), dim3(256), 0, st, q, top, rng_state, (uint32_t)sid, s_pcc, s_ssim,
                       distractors, w.rows);
    hipLaunchKernelGGL(nway_fold_kernel, dim3(1), dim3(64), 0, st, (const double*)w.rows, n, out8, acc6, acc_mode);
    return hipGetLastError() == hipSuccess ? OK : E_LAUNCH;
}

}  // namespace fmri
