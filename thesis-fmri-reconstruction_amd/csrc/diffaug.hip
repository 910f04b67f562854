// Differentiable augmentation of the discriminator's inputs (Zhao et al., "Differentiable Augmentation for Data-Efficient
// GAN Training", NeurIPS 2020; policy colour + translation + cutout) on NHWC8 fp16 images: the transform, its adjoint and
// the draw of the per-image parameter rows (include/fmri_hip.h fmri_diffaug_fwd for the contract).
//
//   diffaug_params_kernel  thread r owns row row0 + r of the draw: Philox blocks 2 (row0 + r) and 2 (row0 + r) + 1 of the
//                          stream at the state's offset (the element layout of fmri_rng_u32), decoded to the 8 fp32 values
//                          [b, s, c, ty, tx, cy, cx, cut] -- exact in fp32 but c from 1 on, the fp32 sum rounded to nearest
//                          even -- and stored as two 16-byte items.
//   diffaug_fwd_kernel     one workgroup (16 waves) per image.  A wave owns rows y = wave, wave + 16, ..., a lane the pixels
//                          x = lane, lane + 64, ... of a row: one 16-byte load and one 16-byte store per pixel, rows whole
//                          and in order, and the row tests (inside the image after the shift, inside the cutout window) are
//                          compares on wave-uniform integers.  Contrast needs the image's mean before anything can be
//                          written: a first pass over the image sums it, the second pass re-reads the 64 / 156 / 256 KiB
//                          the workgroup has just pulled through its XCD's L2 (HBM is read once).  An image whose contrast
//                          factor is 1 skips the first pass.
//   diffaug_bwd_kernel     the adjoint of the linear part, same shape: the mean of the shifted, masked cotangent in the
//                          first pass (skipped for c = 1), the two mean terms and the saturating store in the second.
//                          blockIdx.y picks one of up to two cotangent streams, so both go in one launch.
//
// Arithmetic.  The colour stages are affine maps with cancelling terms ((v - M) c + M is near zero for v near M (1 - 1/c)):
// evaluated in fp32 the result misses the fp16 rounding of the exact value by many fp16 ulps there.  The per-element
// arithmetic and the sums are therefore fp64 -- ~25 operations per 32 bytes moved, far under the memory time -- and the
// result is rounded once to fp32 and once to fp16.  Sums run in a fixed order (per thread in pixel order, 64 lanes by a
// shuffle tree, the 16 waves in wave order): a launch is deterministic with or without fmri_set_deterministic.  A stage
// whose parameter is neutral (b = 0, s = 1, c = 1) is skipped, not evaluated: the neutral row copies the three real
// channels bit for bit.  No atomics, no LDS beyond the 16 partial sums, no per-element divide.
#include "kernels.h"
#include "philox.h"

namespace fmri {

namespace {

// 16 waves per image: at B = 256 the grid is only 3 images per CU, and a wave has one 1-KiB row in flight -- 4 waves per
// image streamed at 0.65 / 0.71 of axpby's rate, 8 at 0.73 / 0.75, 16 at 0.78 / 0.82 (profiles/diffaug.md)
constexpr int AUG_THREADS = 1024;
constexpr int AUG_WAVES = AUG_THREADS / 64;
constexpr double THIRD = 1.0 / 3.0;

struct AugRow {
    double b, s, c;
    int ty, tx;
    int y0, y1, x0, x1;      // cutout window, both ends inclusive; empty: y0 > y1
    bool colour;
};

// image `img` of the steps' [orig | pred | sampled] layout (B images each) -> its row of the [2B][8] table: orig and pred
// share rows 0 .. B-1, sampled has rows B .. 2B-1
__device__ __forceinline__ AugRow aug_row(const float* __restrict__ table, int img, int B, int H) {
    const int row = img < B ? img : img - B;
    const float4 p0 = *(const float4*)(table + 8 * (int64_t)row);
    const float4 p1 = *(const float4*)(table + 8 * (int64_t)row + 4);
    AugRow a;
    a.b = (double)p0.x;
    a.s = (double)p0.y;
    a.c = (double)p0.z;
    a.ty = (int)p0.w;
    a.tx = (int)p1.x;
    const int cy = (int)p1.y, cx = (int)p1.z, cut = (int)p1.w;
    if (cut > 0) {
        // { clamp(cy - cut / 2 + i, 0, H - 1) : 0 <= i < cut } is the interval between its clamped ends
        a.y0 = min(max(cy - cut / 2, 0), H - 1);
        a.y1 = min(max(cy - cut / 2 + cut - 1, 0), H - 1);
        a.x0 = min(max(cx - cut / 2, 0), H - 1);
        a.x1 = min(max(cx - cut / 2 + cut - 1, 0), H - 1);
    } else {
        a.y0 = a.x0 = 1;
        a.y1 = a.x1 = 0;
    }
    a.colour = p0.x != 0.f || p0.y != 1.f || p0.z != 1.f;
    return a;
}

// sum over the workgroup in a fixed order; every thread gets it
__device__ __forceinline__ double aug_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = red[0];
#pragma unroll
    for (int w = 1; w < AUG_WAVES; ++w) t += red[w];
    return t;
}

// brightness and saturation of one pixel (stages 1 and 2 of the transform)
__device__ __forceinline__ void aug_bs(const AugRow& a, const h8& v, double (&o)[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = (double)(float)v[j];
    if (a.b != 0.0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) o[j] += a.b;
    }
    if (a.s != 1.0) {
        const double m = ((o[0] + o[1]) + o[2]) * THIRD;
#pragma unroll
        for (int j = 0; j < 3; ++j) o[j] = (o[j] - m) * a.s + m;
    }
}

__device__ __forceinline__ half_t aug_sat16(double v) {
    const double c = v == v ? fmin(fmax(v, -65504.0), 65504.0) : v;
    return (half_t)(float)c;
}

__global__ __launch_bounds__(AUG_THREADS) void diffaug_fwd_kernel(const half_t* __restrict__ src,
                                                                  half_t* __restrict__ dst, int H,
                                                                  const float* __restrict__ table, int B, int img0,
                                                                  double inv_n) {
    __shared__ double red[AUG_WAVES];
    const int img = blockIdx.x;
    const AugRow a = aug_row(table, img0 + img, B, H);
    const h8* __restrict__ s = (const h8*)src + (int64_t)img * H * H;
    h8* __restrict__ d = (h8*)dst + (int64_t)img * H * H;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    double M = 0.0;
    if (a.c != 1.0) {
        double acc = 0.0;
        for (int y = wid; y < H; y += AUG_WAVES)
            for (int x = lane; x < H; x += 64) {
                double u[3];
                aug_bs(a, s[y * H + x], u);
                acc += (u[0] + u[1]) + u[2];
            }
        M = aug_block_sum(acc, red) * inv_n;
    }
    for (int y = wid; y < H; y += AUG_WAVES) {
        const int sy = y + a.ty;
        const bool row_in = sy >= 0 && sy < H;
        const bool row_cut = y >= a.y0 && y <= a.y1;
        for (int x = lane; x < H; x += 64) {
            const int sx = x + a.tx;
            h8 o = {0, 0, 0, 0, 0, 0, 0, 0};
            if (row_in && sx >= 0 && sx < H && !(row_cut && x >= a.x0 && x <= a.x1)) {
                const h8 v = s[sy * H + sx];
                if (a.colour) {
                    double u[3];
                    aug_bs(a, v, u);
                    if (a.c != 1.0) {
#pragma unroll
                        for (int j = 0; j < 3; ++j) u[j] = (u[j] - M) * a.c + M;
                    }
#pragma unroll
                    for (int j = 0; j < 3; ++j) o[j] = (half_t)(float)u[j];
                } else {
#pragma unroll
                    for (int j = 0; j < 3; ++j) o[j] = v[j];
                }
            }
            d[y * H + x] = o;
        }
    }
}

// the masked, shifted cotangent g1[y][x] of one pixel: g[y - ty][x - tx] where that lies inside the image and outside the
// cutout window, else 0
__device__ __forceinline__ bool aug_src_ok(const AugRow& a, int qy, int qx, int H) {
    return qy >= 0 && qy < H && qx >= 0 && qx < H && !(qy >= a.y0 && qy <= a.y1 && qx >= a.x0 && qx <= a.x1);
}

__global__ __launch_bounds__(AUG_THREADS) void diffaug_bwd_kernel(const half_t* __restrict__ ga, half_t* __restrict__ da,
                                                                  const half_t* __restrict__ gb, half_t* __restrict__ db,
                                                                  int H, const float* __restrict__ table, int B, int img0,
                                                                  double inv_n) {
    __shared__ double red[AUG_WAVES];
    const int img = blockIdx.x;
    const AugRow a = aug_row(table, img0 + img, B, H);
    const h8* __restrict__ g = (const h8*)(blockIdx.y ? gb : ga) + (int64_t)img * H * H;
    h8* __restrict__ d = (h8*)(blockIdx.y ? db : da) + (int64_t)img * H * H;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    double mean = 0.0;
    if (a.c != 1.0) {
        double acc = 0.0;
        for (int y = wid; y < H; y += AUG_WAVES) {
            const int qy = y - a.ty;
            for (int x = lane; x < H; x += 64) {
                const int qx = x - a.tx;
                if (aug_src_ok(a, qy, qx, H)) {
                    const h8 v = g[qy * H + qx];
                    acc += ((double)(float)v[0] + (double)(float)v[1]) + (double)(float)v[2];
                }
            }
        }
        mean = aug_block_sum(acc, red) * inv_n;
    }
    const double cm = (1.0 - a.c) * mean;
    for (int y = wid; y < H; y += AUG_WAVES) {
        const int qy = y - a.ty;
        for (int x = lane; x < H; x += 64) {
            const int qx = x - a.tx;
            h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (aug_src_ok(a, qy, qx, H)) v = g[qy * H + qx];
            double t[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) t[j] = (double)(float)v[j];
            if (a.c != 1.0) {
#pragma unroll
                for (int j = 0; j < 3; ++j) t[j] = a.c * t[j] + cm;
            }
            if (a.s != 1.0) {
                const double m = (1.0 - a.s) * (((t[0] + t[1]) + t[2]) * THIRD);
#pragma unroll
                for (int j = 0; j < 3; ++j) t[j] = a.s * t[j] + m;
            }
            h8 o = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 3; ++j) o[j] = aug_sat16(t[j]);
            d[y * H + x] = o;
        }
    }
}

// row r of the draw: elements 8 R .. 8 R + 7 (R = row0 + r) of stream sid = the words of blocks 2 R and 2 R + 1
__global__ __launch_bounds__(256) void diffaug_params_kernel(const int64_t* __restrict__ state, float* __restrict__ table,
                                                             int rows, uint64_t row0, uint32_t sid, int H, int sh, int cut,
                                                             int policy) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const uint64_t R = row0 + (uint64_t)r;
    const u32x4 w0 = rng_block(state, 2 * R, sid), w1 = rng_block(state, 2 * R + 1, sid);
    float4 p0 = make_float4(0.f, 1.f, 1.f, 0.f), p1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (policy & 1) {
        p0.x = (float)(w0.w[0] >> 8) * 0x1p-24f - 0.5f;
        p0.y = (float)(w0.w[1] >> 8) * 0x1p-23f;
        p0.z = (float)(w0.w[2] >> 8) * 0x1p-24f + 0.5f;
    }
    if (policy & 2) {
        const uint32_t span = 2u * (uint32_t)sh + 1u;
        p0.w = (float)((int)__umulhi(w0.w[3], span) - sh);
        p1.x = (float)((int)__umulhi(w1.w[0], span) - sh);
    }
    if (policy & 4) {
        const uint32_t span = (uint32_t)(H - (cut & 1) + 1);
        p1.y = (float)__umulhi(w1.w[1], span);
        p1.z = (float)__umulhi(w1.w[2], span);
        p1.w = (float)cut;
    }
    *(float4*)(table + 8 * (int64_t)r) = p0;
    *(float4*)(table + 8 * (int64_t)r + 4) = p1;
}

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? OK : E_LAUNCH)

}  // namespace

int diffaug_params_launch(const int64_t* state, float* table, int rows, int64_t row0, int sid, int H, int sh, int cut,
                          int policy, hipStream_t st) {
    hipLaunchKernelGGL(diffaug_params_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, state, table, rows,
                       (uint64_t)row0, (uint32_t)sid, H, sh, cut, policy);
    return LAUNCH_OK();
}

int diffaug_fwd_launch(const half_t* src, half_t* dst, int N, int H, const float* table, int B, int img0,
                       hipStream_t st) {
    hipLaunchKernelGGL(diffaug_fwd_kernel, dim3(N), dim3(AUG_THREADS), 0, st, src, dst, H, table, B, img0,
                       1.0 / (3.0 * H * H));
    return LAUNCH_OK();
}

int diffaug_bwd_launch(const half_t* ga, half_t* da, const half_t* gb, half_t* db, int N, int H, const float* table, int B,
                       int img0, hipStream_t st) {
    hipLaunchKernelGGL(diffaug_bwd_kernel, dim3(N, gb ? 2 : 1), dim3(AUG_THREADS), 0, st, ga, da, gb, db, H, table, B,
                       img0, 1.0 / (3.0 * H * H));
    return LAUNCH_OK();
}

}  // namespace fmri
