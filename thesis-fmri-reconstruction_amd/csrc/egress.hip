// Image egress: the engine's image layout (fp16 [n][H][W][8], channels 0..2 real: what the decoder writes and ingest
// produces) -> the uint8 pixels the scripts write to disk, on the device (fmri_hip/egress.py; include/fmri_hip.h
// fmri_images_u8).  Two shapes of output:
//
//   mode 0   save_image(F.interpolate(im, size=R), normalize=True) of every image by itself (evaluate(save=True),
//            train/train_utils.py:728-735): out [n][R][R][3], nearest-neighbour source index
//            min((int)floorf(dst * ((float)H / R)), H - 1), one range per image.
//   mode 1   make_grid(x, nrow, padding, normalize=True) (train/train_vgan_stage1.py:465-485): one range over all n
//            images, out the grid as HWC bytes, padding and empty cells 0, n == 1 the bare image.
//
// The arithmetic restates torchvision 0.5.0's norm_ip and save_image as torch runs them on the CPU, every operation a
// separately rounded fp32 operation: d = (float)((double)hi - (double)lo + 1e-5), y = (x + (-lo)) / d with a correctly
// rounded division, b = (uint8)clamp(y * 255 + 0.5, 0, 255).
//
//   egress_range_kernel    grid n; one block = one image, one 16-byte load per pixel, lanes 3..7 dropped in registers;
//                          min / max of the block in LDS, [lo, hi] to ws[image].
//   egress_pixels_kernel   output-stationary over the output as a flat array of dwords: every lane decodes its first byte
//                          index to (image, row, column, channel) and steps through the other three, reads a source
//                          pixel (8 bytes) per output pixel it touches and issues one dword store (bytes behind the end
//                          of the output are 0).  Mode 1: every block folds the n ranges itself.
//                          With slot_dev the output base is moved by (slot_dev[0] mod slot_mod) * slot_stride bytes --
//                          read on the device, so the launch can sit in front of or behind the launch that increments
//                          the counter in any replay -- and present[slot] = 1.
//   egress_open_kernel     one thread: the first call for a pass clears the slot's present flags (fmri_images_u8_open).
//
// No atomics, no memset, no allocation, no host sync.  min / max are exact and the rest is element-wise: the bytes are a
// function of the input and the geometry only, whatever fmri_set_deterministic says.  A non-finite pixel gives
// unspecified bytes; no address depends on a pixel value.
#include "kernels.h"

namespace fmri {

namespace {

struct EgressGeom {
    int32_t n, H, W, mode;
    int32_t Ho, Wo;                 // mode 0: side(s) of an output image; mode 1: the grid
    int32_t resize;                 // mode 0: 1 = nearest-neighbour H x W -> Ho x Wo
    int32_t xmaps, padding, bare;   // mode 1; bare: n == 1, the image alone
    float sy, sx;                   // (float)H / Ho, (float)W / Wo
    uint32_t total;                 // bytes of the output (< 2^31)
    FastDiv fdRow, fdImg;           // / (Wo * 3), / (Ho * Wo * 3)
    FastDiv fdCellH, fdCellW;       // / (H + padding), / (W + padding)
};

__device__ __forceinline__ void block_minmax(float& lo, float& hi, float* s_lo, float* s_hi) {
    s_lo[threadIdx.x] = lo;
    s_hi[threadIdx.x] = hi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_lo[threadIdx.x] = fminf(s_lo[threadIdx.x], s_lo[threadIdx.x + s]);
            s_hi[threadIdx.x] = fmaxf(s_hi[threadIdx.x], s_hi[threadIdx.x + s]);
        }
        __syncthreads();
    }
    lo = s_lo[0];
    hi = s_hi[0];
}

__global__ __launch_bounds__(256) void egress_range_kernel(const uint4* __restrict__ src, int HW, float* __restrict__ ws) {
    __shared__ float s_lo[256], s_hi[256];
    const uint4* p = src + (int64_t)blockIdx.x * HW;
    float lo = INFINITY, hi = -INFINITY;
    for (int e = threadIdx.x; e < HW; e += 256) {
        const uint4 v = p[e];
        const h8 h = __builtin_bit_cast(h8, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float f = (float)h[c];
            lo = fminf(lo, f);
            hi = fmaxf(hi, f);
        }
    }
    block_minmax(lo, hi, s_lo, s_hi);
    if (threadIdx.x == 0) {
        ws[2 * blockIdx.x] = lo;
        ws[2 * blockIdx.x + 1] = hi;
    }
}

__device__ __forceinline__ float range_div(float lo, float hi) { return (float)((double)hi - (double)lo + 1e-5); }

__device__ __forceinline__ uint32_t quantise(float x, float lo, float d) {
    const float y = __fdiv_rn(__fadd_rn(x, -lo), d);
    const float v = fminf(fmaxf(__fadd_rn(__fmul_rn(y, 255.f), 0.5f), 0.f), 255.f);
    return (uint32_t)(int)v;
}

// source pixel (k, y, x) of output pixel (row, col) -- of image k in mode 0; false: padding or an empty cell
__device__ __forceinline__ bool egress_source(const EgressGeom& g, int row, int col, int& k, int& y, int& x) {
    if (g.mode == 0) {
        y = g.resize ? min((int)floorf((float)row * g.sy), g.H - 1) : row;
        x = g.resize ? min((int)floorf((float)col * g.sx), g.W - 1) : col;
        return true;
    }
    if (g.bare) {
        k = 0; y = row; x = col;
        return true;
    }
    const int ry = row - g.padding, rx = col - g.padding;
    if (ry < 0 || rx < 0) return false;
    const int cy = (int)fd_div((uint32_t)ry, g.fdCellH), cx = (int)fd_div((uint32_t)rx, g.fdCellW);
    y = ry - cy * (g.H + g.padding);
    x = rx - cx * (g.W + g.padding);
    k = cy * g.xmaps + cx;
    return y < g.H && x < g.W && cx < g.xmaps && k < g.n;
}

__global__ __launch_bounds__(256) void egress_pixels_kernel(const half_t* __restrict__ src, EgressGeom g,
                                                            const float* __restrict__ ws, uint8_t* __restrict__ out,
                                                            const int64_t* __restrict__ slot_dev, int64_t slot_stride,
                                                            int slot_mod, uint8_t* __restrict__ present) {
    __shared__ float s_lo[256], s_hi[256];
    float glo = INFINITY, ghi = -INFINITY;
    if (g.mode == 1) {
        for (int i = threadIdx.x; i < g.n; i += 256) {
            glo = fminf(glo, ws[2 * i]);
            ghi = fmaxf(ghi, ws[2 * i + 1]);
        }
        block_minmax(glo, ghi, s_lo, s_hi);
    }
    int64_t slot = 0;
    if (slot_dev) {
        slot = slot_dev[0] % slot_mod;
        if (slot < 0) slot += slot_mod;
    }
    if (present && blockIdx.x == 0 && threadIdx.x == 0) present[slot] = 1;
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= (g.total + 3u) / 4u) return;
    // (image, row, column, channel) of the lane's first byte by division, of the other three by stepping; a source
    // pixel is loaded (8 bytes: lanes 0..3) when the output pixel changes, a range when the image does
    const uint32_t idx0 = q * 4u;
    int k = 0;
    uint32_t r = idx0;
    if (g.mode == 0) {
        k = (int)fd_div(idx0, g.fdImg);
        r = idx0 - (uint32_t)k * (uint32_t)(g.Ho * g.Wo * 3);
    }
    int row = (int)fd_div(r, g.fdRow);
    const uint32_t r2 = r - (uint32_t)row * (uint32_t)(g.Wo * 3);
    int col = (int)(r2 / 3u), ch = (int)(r2 - (uint32_t)(r2 / 3u) * 3u);
    float lo = glo, d = g.mode == 1 ? range_div(glo, ghi) : 1.f;
    bool new_px = true, new_img = true, valid = false;
    h4 p = {};
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (idx0 + j < g.total) {               // bytes behind the end of the output are 0
            if (new_px) {
                int sk = k, y, x;
                valid = egress_source(g, row, col, sk, y, x);
                if (valid) p = *(const h4*)(src + (((int64_t)sk * g.H + y) * g.W + x) * 8);
                if (g.mode == 0 && new_img) {
                    lo = ws[2 * k];
                    d = range_div(lo, ws[2 * k + 1]);
                    new_img = false;
                }
                new_px = false;
            }
            if (valid) {
                const float v = (float)(ch == 0 ? p[0] : ch == 1 ? p[1] : p[2]);
                word |= quantise(v, lo, d) << (8 * j);
            }
        }
        if (++ch == 3) {
            ch = 0;
            new_px = true;
            if (++col == g.Wo) {
                col = 0;
                if (++row == g.Ho && g.mode == 0) {
                    row = 0;
                    ++k;
                    new_img = true;
                }
            }
        }
    }
    ((uint32_t*)(out + slot * slot_stride))[q] = word;
}

__global__ void egress_open_kernel(const int64_t* __restrict__ slot_dev, int slot_mod, int64_t* __restrict__ opened,
                                   uint8_t* __restrict__ present, int64_t present_stride, int kinds) {
    const int64_t c = slot_dev[0];
    if (opened[0] == c + 1) return;             // this pass has opened its slot already
    int64_t slot = c % slot_mod;
    if (slot < 0) slot += slot_mod;
    for (int k = 0; k < kinds; ++k) present[k * present_stride + slot] = 0;
    opened[0] = c + 1;
}

}  // namespace

int64_t images_u8_ws_bytes(int n) {
    if (n < 1) return -1;
    return (int64_t)n * 2 * (int64_t)sizeof(float);
}

int64_t images_u8_out_bytes(int n, int H, int W, int mode, int R, int nrow, int padding) {
    if (mode == 0) return (int64_t)n * (R ? R : H) * (R ? R : W) * 3;
    if (n == 1) return (int64_t)H * W * 3;
    const int64_t xmaps = nrow < n ? nrow : n, ymaps = (n + xmaps - 1) / xmaps;
    return (ymaps * (H + padding) + padding) * (xmaps * ((int64_t)W + padding) + padding) * 3;
}

int images_u8_launch(const half_t* src, int n, int H, int W, int mode, int R, int nrow, int padding, void* ws,
                     int64_t ws_bytes, uint8_t* out, const int64_t* slot_dev, int64_t slot_stride, int slot_mod,
                     uint8_t* present_dev, hipStream_t st) {
    if (ws_bytes < images_u8_ws_bytes(n)) return E_WORKSPACE;
    const int64_t total = images_u8_out_bytes(n, H, W, mode, R, nrow, padding);
    if (total >= (int64_t)1 << 31) return E_UNSUPPORTED;
    EgressGeom g = {};
    g.n = n; g.H = H; g.W = W; g.mode = mode;
    g.total = (uint32_t)total;
    if (mode == 0) {
        g.Ho = R ? R : H;
        g.Wo = R ? R : W;
        g.resize = R != 0;
        g.sy = (float)H / (float)g.Ho;
        g.sx = (float)W / (float)g.Wo;
        g.xmaps = 1;
    } else {
        g.bare = n == 1;
        g.padding = g.bare ? 0 : padding;
        g.xmaps = nrow < n ? nrow : n;
        const int ymaps = (n + g.xmaps - 1) / g.xmaps;
        g.Ho = g.bare ? H : ymaps * (H + padding) + padding;
        g.Wo = g.bare ? W : g.xmaps * (W + padding) + padding;
    }
    g.fdRow = make_fastdiv((uint32_t)g.Wo * 3u);
    g.fdImg = make_fastdiv((uint32_t)g.Ho * (uint32_t)g.Wo * 3u);
    g.fdCellH = make_fastdiv((uint32_t)(H + g.padding));
    g.fdCellW = make_fastdiv((uint32_t)(W + g.padding));
    hipLaunchKernelGGL(egress_range_kernel, dim3(n), dim3(256), 0, st, (const uint4*)src, H * W, (float*)ws);
    const uint32_t dwords = (g.total + 3u) / 4u;
    hipLaunchKernelGGL(egress_pixels_kernel, dim3((dwords + 255u) / 256u), dim3(256), 0, st, src, g, (const float*)ws, out,
                       slot_dev, slot_stride, slot_mod, present_dev);
    return hipGetLastError() == hipSuccess ? OK : E_LAUNCH;
}

int images_u8_open_launch(const int64_t* slot_dev, int slot_mod, int64_t* opened_dev, uint8_t* present_dev,
                          int64_t present_stride, int kinds, hipStream_t st) {
    hipLaunchKernelGGL(egress_open_kernel, dim3(1), dim3(1), 0, st, slot_dev, slot_mod, opened_dev, present_dev,
                       present_stride, kinds);
    return hipGetLastError() == hipSuccess ? OK : E_LAUNCH;
}

}  // namespace fmri
