// The validation metrics of a batch of image pairs in one pass over the engine's own image layout (fp16 [N][H][W][8],
// channels 0..C-1 real: what the decoder writes and ingest / images_to_nhwc produce), for the evaluation pass of the fused
// steps (fmri_hip/evaluate.py).  The formulas are those of metrics.hip:
//
//   PCC  = PearsonCorrelation.forward over the whole batch (train/train_utils.py:276-292)
//   SSIM = StructuralSimilarity.forward, size_average (:343-420): 11x11 Gaussian sigma 1.5, zero padding 5, C1 = 1e-4,
//          C2 = 9e-4, mean over (n, c, y, x)
//   MSE  = nn.MSELoss over the N*C*H*W real elements
//
// optionally of v * scale[c] + shift[c] (denormalize_image, :234-240) instead of the stored v: the affine is applied in
// fp32 to in-image pixels only, the padding stays 0 (the reference pads the denormalised tensor).
//
//   image_metrics_tile_kernel   grid (ceil(W/16), ceil(H/16), N); one block = one 16 x 16 output tile of one image pair,
//                               all channels.  The 26 x 26 halo tile of both tensors is loaded with one 16-byte load per
//                               pixel; lanes C..7 of a pixel never leave LDS.  Window, the five filtered statistics and
//                               the SSIM map are fp64, as fmri_ssim_pairs: with the denormalising affine the variances
//                               E[x^2] - mu^2 of an fp32 filter are 4e-6 from the exact mean SSIM.  The same
//                               block sums x, y, x^2, y^2, xy and (x - y)^2 of its tile in fp64 -- (x - y)^2 as a sum of
//                               its own: derived from the other five it would cancel.  7 doubles to ws[block].
//   image_metrics_fold_kernel   one block: the partials in a fixed order (thread t takes t, t + 256, ...; then the block
//                               sum), out[0..2] = pcc, ssim, mse (fp32).  With an accumulator (device double[4]: sum of
//                               pcc, ssim, mse, batches) it also adds the batch -- the fp32 values it just wrote -- after
//                               clearing it (acc_mode 0) or not (1), and writes the running means and the batch count
//                               to out[3..6]: the mean over a pass needs no launch of its own and no memset.
//
// No atomics, no allocation, no host sync; two launches per call.  out[0..2] is a bitwise function of the two tensors and
// (N, H, W, C, affine) only: two calls are bit-identical, with fmri_set_deterministic on or off, and a batch addressed
// through a pointer offset gives the bits of its copy.
#include "kernels.h"
#include "ssim_window.h"

namespace fmri {

namespace {

struct ImgAffine {
    float scale[8], shift[8];
    int on;
};

constexpr int EM_SUMS = 7;      // sum x, y, x^2, y^2, xy, (x - y)^2, ssim

__global__ __launch_bounds__(256) void image_metrics_tile_kernel(const uint4* __restrict__ pred,
                                                                 const uint4* __restrict__ truth, int H, int W, int C,
                                                                 ImgAffine aff, double* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) half_t raw[2][SS_R * SS_R][8];
    __shared__ float t[2][SS_R][SS_R + 1];
    __shared__ double hx[5][SS_R][SS_TS + 1];
    __shared__ double g[SS_WIN];
    __shared__ double sh[4];
    const int tx0 = blockIdx.x * SS_TS, ty0 = blockIdx.y * SS_TS;
    const int64_t img = (int64_t)blockIdx.z * H * W;
    gauss11(g);
    for (int e = threadIdx.x; e < SS_R * SS_R; e += 256) {
        const int j = e / SS_R, i = e - j * SS_R;
        const int y = ty0 - SS_PAD + j, x = tx0 - SS_PAD + i;
        if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {      // pixels outside are never read back
            const int64_t o = img + (int64_t)y * W + x;
            *(uint4*)raw[0][e] = pred[o];
            *(uint4*)raw[1][e] = truth[o];
        }
    }
    const int oy = threadIdx.x >> 4, ox = threadIdx.x & 15;
    const bool inside = ty0 + oy < H && tx0 + ox < W;
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    double acc[EM_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < C; ++c) {
        __syncthreads();            // raw is written / t and hx of the previous channel are consumed
        const float sc = aff.scale[c], sf = aff.shift[c];
        for (int e = threadIdx.x; e < SS_R * SS_R; e += 256) {
            const int j = e / SS_R, i = e - j * SS_R;
            const int y = ty0 - SS_PAD + j, x = tx0 - SS_PAD + i;
            float u = 0.f, v = 0.f;
            if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
                u = (float)raw[0][e][c];
                v = (float)raw[1][e][c];
                if (aff.on) {
                    u = u * sc + sf;
                    v = v * sc + sf;
                }
            }
            t[0][j][i] = u;
            t[1][j][i] = v;
        }
        __syncthreads();
        // horizontal pass: the five filtered quantities of 26 rows x 16 columns (products of fp32 values: exact in fp64)
        for (int e = threadIdx.x; e < SS_R * SS_TS; e += 256) {
            const int j = e / SS_TS, i = e - j * SS_TS;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
            for (int k = 0; k < SS_WIN; ++k) {
                const double w = g[k], u = t[0][j][i + k], v = t[1][j][i + k];
                s0 += w * u;
                s1 += w * v;
                s2 += w * (u * u);
                s3 += w * (v * v);
                s4 += w * (u * v);
            }
            hx[0][j][i] = s0; hx[1][j][i] = s1; hx[2][j][i] = s2; hx[3][j][i] = s3; hx[4][j][i] = s4;
        }
        __syncthreads();
        if (inside) {
            double m1 = 0.0, m2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
            for (int k = 0; k < SS_WIN; ++k) {
                const double w = g[k];
                m1 += w * hx[0][oy + k][ox];
                m2 += w * hx[1][oy + k][ox];
                e11 += w * hx[2][oy + k][ox];
                e22 += w * hx[3][oy + k][ox];
                e12 += w * hx[4][oy + k][ox];
            }
            const double m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
            const double s1 = e11 - m11, s2 = e22 - m22, s12 = e12 - m12;
            const double u = t[0][oy + SS_PAD][ox + SS_PAD], v = t[1][oy + SS_PAD][ox + SS_PAD], d = u - v;
            acc[0] += u;
            acc[1] += v;
            acc[2] += u * u;
            acc[3] += v * v;
            acc[4] += u * v;
            acc[5] += d * d;
            acc[6] += ((2.0 * m12 + C1) * (2.0 * s12 + C2)) / ((m11 + m22 + C1) * (s1 + s2 + C2));
        }
    }
    const int64_t block = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
#pragma unroll
    for (int k = 0; k < EM_SUMS; ++k) {
        const double s = block_sum_fixed(acc[k], sh);
        if (threadIdx.x == 0) ws[block * EM_SUMS + k] = s;
    }
}

__global__ __launch_bounds__(256) void image_metrics_fold_kernel(const double* __restrict__ ws, int64_t blocks, double n,
                                                                 float* __restrict__ out, double* __restrict__ acc,
                                                                 int acc_mode) {
    __shared__ double sh[4];
    double s[EM_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t b = threadIdx.x; b < blocks; b += 256)
#pragma unroll
        for (int k = 0; k < EM_SUMS; ++k) s[k] += ws[b * EM_SUMS + k];
#pragma unroll
    for (int k = 0; k < EM_SUMS; ++k) s[k] = block_sum_fixed(s[k], sh);
    if (threadIdx.x) return;
    const double mx = s[0] / n, my = s[1] / n;
    const double sxx = s[2] - n * mx * mx, syy = s[3] - n * my * my, sxy = s[4] - n * mx * my;
    const float pcc = (float)(sxy / (sqrt(sxx) * sqrt(syy))), ssim = (float)(s[6] / n), mse = (float)(s[5] / n);
    out[0] = pcc;
    out[1] = ssim;
    out[2] = mse;
    if (acc) {
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        if (acc_mode)
            for (int k = 0; k < 4; ++k) a[k] = acc[k];
        a[0] += (double)pcc;
        a[1] += (double)ssim;
        a[2] += (double)mse;
        a[3] += 1.0;
        for (int k = 0; k < 4; ++k) acc[k] = a[k];
        out[3] = (float)(a[0] / a[3]);
        out[4] = (float)(a[1] / a[3]);
        out[5] = (float)(a[2] / a[3]);
        out[6] = (float)a[3];
    }
}

inline int64_t tiles_of(int N, int H, int W) {
    return (int64_t)N * ((H + SS_TS - 1) / SS_TS) * ((W + SS_TS - 1) / SS_TS);
}

}  // namespace

int64_t image_metrics_ws_bytes(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1) return -1;
    return tiles_of(N, H, W) * EM_SUMS * (int64_t)sizeof(double);
}

int image_metrics_launch(const half_t* pred, const half_t* truth, int N, int H, int W, int C, const float* scale,
                         const float* shift, void* ws, int64_t ws_bytes, float* out7, double* acc4, int acc_mode,
                         hipStream_t st) {
    if (ws_bytes < image_metrics_ws_bytes(N, H, W)) return E_WORKSPACE;
    ImgAffine aff = {};
    aff.on = scale != nullptr;
    for (int c = 0; c < C && aff.on; ++c) {
        aff.scale[c] = scale[c];
        aff.shift[c] = shift[c];
    }
    const dim3 grid((W + SS_TS - 1) / SS_TS, (H + SS_TS - 1) / SS_TS, N);
    hipLaunchKernelGGL(image_metrics_tile_kernel, grid, dim3(256), 0, st, (const uint4*)pred, (const uint4*)truth, H, W, C,
                       aff, (double*)ws);
    hipLaunchKernelGGL(image_metrics_fold_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, tiles_of(N, H, W),
                       (double)N * C * H * W, out7, acc4, acc_mode);
    return hipGetLastError() == hipSuccess ? OK : E_LAUNCH;
}

}  // namespace fmri
