// extern "C" surface of libfmri_hip.so (declared in include/fmri_hip.h).
// Host-side geometry derivation + argument validation; all device work is enqueued on the caller's stream.
#include "../../include/fmri_hip.h"
#include "kernels.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <cstdlib>

using namespace fmri;

static_assert(sizeof(fmri_stat) == sizeof(StatRec) && sizeof(fmri_stat) == 32, "fmri_stat layout");
static_assert(sizeof(fmri_stat_seg) == sizeof(StatSeg) && sizeof(fmri_stat_seg) == 64, "fmri_stat_seg layout");
static_assert(FMRI_STAT_MAX_SEGS == STAT_MAX_SEGS && FMRI_STAT_BLOCKS == STAT_BLOCKS, "monitor limits");

namespace {
inline hipStream_t S(void* s) { return (hipStream_t)s; }
inline int pad_to(int v, int m) { return (v + m - 1) / m * m; }

struct TClass { int py, px, th, tw, dy0, dx0, kpad; int64_t w_off; };

// parity classes of a k x k stride-2 pad-p transposed convolution (see csrc/igemm.hip header)
void tconv_classes(int k, int pad, int ci, int rows_pad, TClass out[4]) {
    int64_t off = 0;
    for (int cy = 0; cy < 2; ++cy)
        for (int cx = 0; cx < 2; ++cx) {
            TClass& c = out[cy * 2 + cx];
            c.py = (cy + pad) & 1;
            c.px = (cx + pad) & 1;
            c.th = (k - c.py + 1) / 2;
            c.tw = (k - c.px + 1) / 2;
            c.dy0 = (cy + pad - c.py) / 2;
            c.dx0 = (cx + pad - c.px) / 2;
            c.kpad = pad_to(c.th * c.tw * ci, 64);
            c.w_off = off;
            off += (int64_t)rows_pad * c.kpad;
        }
}
}  // namespace

// ---- routing probe (kernels.h): thread-local, so that fmri_igemm_route is re-entrant like every other entry point
namespace {
thread_local bool t_probe_on = false;
thread_local char t_probe_name[128];
}  // namespace
namespace fmri {
bool route_probe(const char* fmt, ...) {
    if (!t_probe_on) return false;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t_probe_name, sizeof(t_probe_name), fmt, ap);
    va_end(ap);
    return true;
}
}  // namespace fmri

extern "C" {

/* ---- batch ingest (tail of the image transforms of train_vgan_stage1.py:162-170, data_loader.py:186-217,374-401) ---- */
int fmri_ingest_u8(const uint8_t* src, int N, int H, int W, int C, const int* flip_dev, const int* shift_dev,
                   float mean0, float mean1, float mean2, float std0, float std1, float std2, void* dst16,
                   float* dst32, void* stream) {
    if (!src || N < 1 || H < 1 || W < 1 || (C != 1 && C != 3) || (!dst16 && !dst32) || std0 == 0.f || std1 == 0.f ||
        std2 == 0.f)
        return FMRI_E_BADARG;
    const float m[3] = {mean0, mean1, mean2}, sd[3] = {std0, std1, std2};
    return ingest_u8_launch(src, N, H, W, C, flip_dev, shift_dev, m, sd, (half_t*)dst16, dst32, S(stream));
}

/* ---- the same out of a device-resident pool, by index (fmri_hip/feed.py) ---- */
int fmri_ingest_u8_gather(const uint8_t* src, const int32_t* idx_dev, int N_pool, int N, int H, int W, int C,
                          const int* flip_dev, const int* shift_dev, float mean0, float mean1, float mean2, float std0,
                          float std1, float std2, void* dst16, float* dst32, int* err_dev, void* stream) {
    if (!src || !idx_dev || N_pool < 1 || N < 1 || H < 1 || W < 1 || (C != 1 && C != 3) || (!dst16 && !dst32) ||
        std0 == 0.f || std1 == 0.f || std2 == 0.f || ((uintptr_t)dst16 & 15) || ((uintptr_t)dst32 & 3) ||
        ((uintptr_t)idx_dev & 3) || ((uintptr_t)err_dev & 3))
        return FMRI_E_BADARG;
    const float m[3] = {mean0, mean1, mean2}, sd[3] = {std0, std1, std2};
    return ingest_u8_gather_launch(src, idx_dev, N_pool, N, H, W, C, flip_dev, shift_dev, m, sd, (half_t*)dst16, dst32,
                                   err_dev, S(stream));
}
int fmri_gather_rows_f32(const float* src, int N_pool, int V, const int32_t* idx_dev, int B, float* dst32, void* dst16,
                         int* err_dev, void* stream) {
    if (!src || !idx_dev || N_pool < 1 || V < 1 || B < 1 || (!dst16 && !dst32) || ((uintptr_t)src & 3) ||
        ((uintptr_t)dst32 & 3) || ((uintptr_t)dst16 & 15) || ((uintptr_t)idx_dev & 3) || ((uintptr_t)err_dev & 3))
        return FMRI_E_BADARG;
    return gather_rows_launch(src, N_pool, V, idx_dev, B, dst32, (half_t*)dst16, err_dev, S(stream));
}

/* ---- head of the image transforms: CenterCrop + Resize (train_vgan_stage1.py:162-165) --------------------------- */
int fmri_resize_coeffs(int in_size, int out_size, int32_t* bounds, int32_t* coef, int ksize_cap) {
    if (in_size < 1 || out_size < 1 || !bounds || !coef || ksize_cap < 1) return FMRI_E_BADARG;
    if ((double)in_size / out_size > 30.0) return FMRI_E_UNSUPPORTED;       /* 64 taps per output pixel at most */
    const int r = resize_coeffs(in_size, out_size, bounds, coef, ksize_cap);
    return r < 0 ? FMRI_E_WORKSPACE : r;
}
int fmri_crop_resize_u8(const uint8_t* pool, const int64_t* offsets_dev, const int32_t* dims_dev, int N, int crop, int size,
                        const int32_t* hb_dev, const int32_t* hk_dev, int hks, const int32_t* vb_dev, const int32_t* vk_dev,
                        int vks, int vcount_max, uint8_t* out, void* stream) {
    if (!pool || !offsets_dev || !dims_dev || N < 1 || crop < 1 || size < 1 || !out || hks < 0 || vks < 0) return FMRI_E_BADARG;
    if ((hks > 0 && (!hb_dev || !hk_dev)) || (vks > 0 && (!vb_dev || !vk_dev)) || vcount_max < 1 || vcount_max > vks + (vks == 0))
        return FMRI_E_BADARG;
    if ((hks == 0 || vks == 0) && crop != size) return FMRI_E_BADARG;
    return crop_resize_u8_launch(pool, offsets_dev, dims_dev, N, crop, size, hb_dev, hk_dev, hks, vb_dev, vk_dev, vks, vcount_max,
                                 out, S(stream));
}

/* ---- evaluation metrics (train/train_utils.py:267-292, :295-420) ---- */
int fmri_pcc(const float* pred, const float* truth, int64_t n, double* ws5, float* out, void* stream) {
    if (!pred || !truth || !ws5 || !out || n < 2) return FMRI_E_BADARG;
    return pcc_launch(pred, truth, n, ws5, out, S(stream));
}
int fmri_ssim(const float* img1, const float* img2, int planes, int H, int W, double* ws2, float* ssim,
              float* contrast, void* stream) {
    if (!img1 || !img2 || !ws2 || planes < 1 || H < 1 || W < 1 || (!ssim && !contrast)) return FMRI_E_BADARG;
    return ssim_launch(img1, img2, planes, H, W, ws2, ssim, contrast, S(stream));
}
/* ---- pairwise PCC / SSIM of n-way identification (train/train_utils.py:752-816) ---- */
int64_t fmri_pcc_matrix_ws_bytes(int N, int M, int64_t D) { return pcc_matrix_ws_bytes(N, M, D); }
int fmri_pcc_matrix(const float* pred, const float* truth, int N, int M, int64_t D, float* sim, int ldS, void* ws,
                    int64_t ws_bytes, void* stream) {
    if (!pred || !truth || !sim || !ws || N < 1 || M < 1 || D < 1 || ldS < M) return FMRI_E_BADARG;
    // grid limits: N + M row blocks, ceil(M / 16) and ceil(D / 1024) in the y / z grid dimensions
    if ((int64_t)N + M > INT32_MAX || M > 65535 * 16 || (D + 1023) / 1024 > 65535) return FMRI_E_UNSUPPORTED;
    return pcc_matrix_launch(pred, truth, N, M, D, sim, ldS, ws, ws_bytes, S(stream));
}
int64_t fmri_ssim_pairs_ws_bytes(int N, int M, int C, int H, int W) { return ssim_pairs_ws_bytes(N, M, C, H, W); }
int fmri_ssim_pairs(const float* pred, const float* truth, int N, int M, int C, int H, int W, const int* pairs, int P,
                    float* out, void* ws, int64_t ws_bytes, void* stream) {
    if (!pred || !truth || !ws || N < 1 || M < 1 || C < 1 || H < 1 || W < 1 || P < 0 || (P && (!pairs || !out)))
        return FMRI_E_BADARG;
    if (H < 11 || W < 11) return FMRI_E_UNSUPPORTED;   // as fmri_ssim: the reference's window shrinks, its padding not
    if (((int64_t)N + M) * C > INT32_MAX || H > 65535 * 16 || W > 65535 * 16) return FMRI_E_UNSUPPORTED;
    return ssim_pairs_launch(pred, truth, N, M, C, H, W, pairs, P, out, ws, ws_bytes, S(stream));
}
/* ---- PCC / SSIM / MSE of a batch in the engine's image layout (the evaluation pass, fmri_hip/evaluate.py) ---- */
int64_t fmri_image_metrics_ws_bytes(int N, int H, int W) { return image_metrics_ws_bytes(N, H, W); }
int fmri_image_metrics(const void* pred16, const void* truth16, int N, int H, int W, int C, int Cp, const float* scale,
                       const float* shift, void* ws, int64_t ws_bytes, float* out7, double* acc4, int acc_mode,
                       void* stream) {
    if (!pred16 || !truth16 || !ws || !out7 || N < 1 || H < 1 || W < 1 || C < 1 || C > 8 || (!scale) != (!shift) ||
        ((uintptr_t)pred16 & 15) || ((uintptr_t)truth16 & 15) || ((uintptr_t)ws & 7) || ((uintptr_t)out7 & 3) ||
        ((uintptr_t)acc4 & 7) || (acc4 && acc_mode != 0 && acc_mode != 1))
        return FMRI_E_BADARG;
    if (Cp != 8) return FMRI_E_UNSUPPORTED;            // one 16-byte load per pixel
    if (H < 11 || W < 11) return FMRI_E_UNSUPPORTED;   // as fmri_ssim: the reference's window shrinks, its padding not
    if (N > 65535 || H > 65535 * 16) return FMRI_E_UNSUPPORTED;     // y / z grid dimensions
    return image_metrics_launch((const half_t*)pred16, (const half_t*)truth16, N, H, W, C, scale, shift, ws, ws_bytes,
                                out7, acc4, acc_mode, S(stream));
}
/* ---- n-way identification of a batch in the engine's image layout (the evaluation pass, fmri_hip/evaluate.py) ---- */
int64_t fmri_nway_ws_bytes(int n, int H, int W) { return nway_ws_bytes(n, H, W); }
int fmri_nway_scores(const void* pred16, const void* truth16, int n, int H, int W, int C, int Cp, int top,
                     const int64_t* rng_state, int sid, void* ws, int64_t ws_bytes, float* s_pcc, float* s_ssim,
                     int32_t* distractors, float* out8, double* acc6, int acc_mode, void* stream) {
    if (!pred16 || !truth16 || !ws || !s_pcc || !s_ssim || !out8 || !acc6 || n < 2 || top < 1 || H < 1 || W < 1 ||
        C < 1 || C > 8 || sid < 0 || (acc_mode != 0 && acc_mode != 1) || ((uintptr_t)pred16 & 15) ||
        ((uintptr_t)truth16 & 15) || ((uintptr_t)ws & 15) || ((uintptr_t)rng_state & 7) || ((uintptr_t)s_pcc & 3) ||
        ((uintptr_t)s_ssim & 3) || ((uintptr_t)distractors & 3) || ((uintptr_t)out8 & 3) || ((uintptr_t)acc6 & 7))
        return FMRI_E_BADARG;
    if (Cp != 8) return FMRI_E_UNSUPPORTED;            // one 16-byte load per pixel
    if (H < 11 || W < 11) return FMRI_E_UNSUPPORTED;   // as fmri_ssim: the reference's window shrinks, its padding not
    if (C > nway_cmax()) return FMRI_E_UNSUPPORTED;    // the workspace is sized without knowing C
    if (n > 65535 * 8) return FMRI_E_UNSUPPORTED;      // y / z grid dimensions of the pair launches
    return nway_scores_launch((const half_t*)pred16, (const half_t*)truth16, n, H, W, C, top, rng_state, sid, ws, ws_bytes,
                              s_pcc, s_ssim, distractors, out8, acc6, acc_mode, S(stream));
}
/* ---- uint8 image egress of a batch in the engine's image layout (fmri_hip/egress.py) ---- */
int64_t fmri_images_u8_ws_bytes(int n) { return images_u8_ws_bytes(n); }
int64_t fmri_images_u8_out_bytes(int n, int H, int W, int mode, int R, int nrow, int padding) {
    if (n < 1 || H < 1 || W < 1 || H > 32768 || W > 32768 || (mode != 0 && mode != 1) || R > 32768 ||
        (mode == 0 && R < 0) || (mode == 1 && (nrow < 1 || padding < 0 || padding > 32768)))
        return -1;
    return images_u8_out_bytes(n, H, W, mode, R, nrow, padding);
}
int fmri_images_u8(const void* src16, int n, int H, int W, int C, int Cp, int mode, int R, int nrow, int padding,
                   void* ws, int64_t ws_bytes, uint8_t* out, const int64_t* slot_dev, int64_t slot_stride, int slot_mod,
                   uint8_t* present_dev, void* stream) {
    if (Cp != 8 || C != 3) return FMRI_E_UNSUPPORTED;  // one 16-byte load per pixel, three bytes per output pixel
    if (!src16 || !ws || !out || fmri_images_u8_out_bytes(n, H, W, mode, R, nrow, padding) < 0 ||
        ((uintptr_t)src16 & 15) || ((uintptr_t)ws & 3) || ((uintptr_t)out & 3) || ((uintptr_t)slot_dev & 7) ||
        (slot_dev && (slot_mod < 1 || slot_stride < 0 || (slot_stride & 3))))
        return FMRI_E_BADARG;
    // a smaller output would drop source pixels from the image, the scripts' range is that of the RESIZED image
    if (mode == 0 && R != 0 && (R < H || R < W)) return FMRI_E_UNSUPPORTED;
    return images_u8_launch((const half_t*)src16, n, H, W, mode, R, nrow, padding, ws, ws_bytes, out, slot_dev, slot_stride,
                            slot_mod, present_dev, S(stream));
}
int fmri_images_u8_open(const int64_t* slot_dev, int slot_mod, int64_t* opened_dev, uint8_t* present_dev,
                        int64_t present_stride, int kinds, void* stream) {
    if (!slot_dev || !opened_dev || !present_dev || slot_mod < 1 || present_stride < slot_mod || kinds < 1 ||
        ((uintptr_t)slot_dev & 7) || ((uintptr_t)opened_dev & 7))
        return FMRI_E_BADARG;
    return images_u8_open_launch(slot_dev, slot_mod, opened_dev, present_dev, present_stride, kinds, S(stream));
}

int fmri_version(void) { return 100; }

const char* fmri_last_error_string(int code) {
    switch (code) {
        case FMRI_OK: return "ok";
        case FMRI_E_BADARG: return "bad argument (shape/alignment constraint violated)";
        case FMRI_E_UNSUPPORTED: return "unsupported configuration";
        case FMRI_E_LAUNCH: return "HIP kernel launch failed";
        case FMRI_E_WORKSPACE: return "workspace too small";
        default: return "unknown error";
    }
}

uint32_t fmri_test_fastdiv(uint32_t n, uint32_t d) { return fd_div(n, make_fastdiv(d)); }

int fmri_kpad(int taps, int ci) { return pad_to(taps * ci, 64); }

int fmri_tconv_class(int k, int pad, int cy, int cx, int ci, int rows_pad, int* py, int* px, int* th, int* tw,
                     int* kpad, int64_t* w_off) {
    if (cy < 0 || cy > 1 || cx < 0 || cx > 1 || k < 1 || ci < 1) return FMRI_E_BADARG;
    TClass c[4];
    tconv_classes(k, pad, ci, rows_pad, c);
    const TClass& t = c[cy * 2 + cx];
    *py = t.py; *px = t.px; *th = t.th; *tw = t.tw; *kpad = t.kpad; *w_off = t.w_off;
    return FMRI_OK;
}

int fmri_pack_weight(const float* src, void* dst, int64_t sa, int64_t sta, int64_t sb, int64_t stb, int A, int TA,
                     int B, int KW, int py, int px, int step, int TH, int TW, int rows_pad, int kpad, void* stream) {
    if (!src || !dst || A < 1 || TA < 1 || B < 1 || TH < 1 || TW < 1) return FMRI_E_BADARG;
    PackArgs p;
    p.src = src; p.dst = (half_t*)dst; p.sa = sa; p.sta = sta; p.sb = sb; p.stb = stb;
    p.A = A; p.TA = TA; p.B = B; p.Bp = pad_to(B, 8);
    p.KW = KW; p.py = py; p.px = px; p.step = step; p.TH = TH; p.TW = TW;
    p.rows_pad = rows_pad; p.kpad = kpad;
    if (rows_pad < TA * A || kpad < TH * TW * p.Bp) return FMRI_E_BADARG;
    return pack_weight_launch(p, S(stream));
}

int fmri_pack_entry_bytes(void) { return (int)sizeof(PackEntry); }

// Fills one host-side table row; returns the number of blocks the row occupies (tile_begin of the next row =
// tile_begin + that), 0 if this weight/orientation is not eligible for the batched kernel, < 0 on bad arguments.
int fmri_pack_entry_fill(void* host_entry, const float* src, void* dst, int64_t sa, int64_t sta, int64_t sb,
                         int64_t stb, int A, int TA, int B, int KW, int py, int px, int step, int TH, int TW,
                         int rows_pad, int kpad, int tile_begin) {
    if (!host_entry || !src || !dst || A < 1 || TA < 1 || B < 1 || TH < 1 || TW < 1) return FMRI_E_BADARG;
    PackEntry e;
    memset(&e, 0, sizeof(e));
    PackArgs& p = e.p;
    p.src = src; p.dst = (half_t*)dst; p.sa = sa; p.sta = sta; p.sb = sb; p.stb = stb;
    p.A = A; p.TA = TA; p.B = B; p.Bp = pad_to(B, 8);
    p.KW = KW; p.py = py; p.px = px; p.step = step; p.TH = TH; p.TW = TW;
    p.rows_pad = rows_pad; p.kpad = kpad;
    if (rows_pad < TA * A || kpad < TH * TW * p.Bp) return FMRI_E_BADARG;
    const int tiles = pack_tile_count(p, &e.run);
    e.tile_begin = tile_begin;
    memcpy(host_entry, &e, sizeof(e));
    return tiles;
}

int fmri_pack_weight_batch(const void* table_dev, int n, int total_tiles, void* stream) {
    if (!table_dev || n < 0 || total_tiles < 0) return FMRI_E_BADARG;
    return pack_batch_launch((const PackEntry*)table_dev, n, total_tiles, S(stream));
}

int fmri_transpose_f16(const void* src, void* dst, int R, int C, int src_rows, int ld_src, int ld_dst, void* stream) {
    if (!src || !dst || R < 1 || C < 1 || src_rows < R || ld_src < C || ld_dst < R || (ld_src & 7) || (ld_dst & 7) ||
        ld_dst < ((R + 7) & ~7))
        return FMRI_E_BADARG;
    return transpose_f16_launch((const half_t*)src, (half_t*)dst, R, C, src_rows, ld_src, ld_dst, S(stream));
}

int fmri_transpose_entry_bytes(void) { return (int)sizeof(TransposeEntry); }

int fmri_transpose_entry_fill(void* host_entry, const void* src, void* dst, int R, int C, int src_rows, int width,
                              int ld_src, int ld_dst, int tile_begin) {
    if (!host_entry || !src || !dst || R < 1 || C < 1 || src_rows < R || width < C || ld_src < width || (ld_src & 7) ||
        (ld_dst & 7) || ld_dst < ((R + 7) & ~7) || tile_begin < 0 || (((uintptr_t)src | (uintptr_t)dst) & 15))
        return FMRI_E_BADARG;
    TransposeEntry e;
    memset(&e, 0, sizeof(e));
    e.src = (const half_t*)src; e.dst = (half_t*)dst; e.R = R; e.C = C; e.Rbuf = src_rows; e.width = width;
    e.lds = ld_src; e.ldd = ld_dst; e.tile_begin = tile_begin;
    memcpy(host_entry, &e, sizeof(e));
    return ((R + 63) / 64) * ((C + 63) / 64);
}

int fmri_transpose_f16_batch(const void* table_dev, int n, int total_tiles, void* stream) {
    if (!table_dev || n < 0 || total_tiles < 0) return FMRI_E_BADARG;
    return transpose_batch_launch((const TransposeEntry*)table_dev, n, total_tiles, S(stream));
}

int fmri_apply_entry_bytes(void) { return (int)sizeof(ApplyEntry); }

int fmri_apply_entry_fill(void* host_entry, const float* gsrc, float* w, float* sq, float* grad, void* pk, int64_t sa,
                          int64_t sta, int64_t sb, int64_t stb, int A, int TA, int B, int KW, int py, int px, int step,
                          int TH, int TW, int ld, int kpad, int nslabs, int64_t slab_stride, int clear, float scale,
                          int64_t flat_n, int tile_begin) {
    if (!host_entry || !w || !sq || tile_begin < 0) return FMRI_E_BADARG;
    ApplyEntry e;
    memset(&e, 0, sizeof(e));
    e.w = w; e.sq = sq; e.grad = grad; e.tile_begin = tile_begin;
    if (flat_n > 0) {
        if (!grad) return FMRI_E_BADARG;
        e.kind = 2; e.n = flat_n;
    } else {
        if (!gsrc || A < 1 || TA < 1 || B < 1 || TH < 1 || TW < 1 || nslabs < 1) return FMRI_E_BADARG;
        e.gsrc = gsrc; e.pk = (half_t*)pk; e.sa = sa; e.sta = sta; e.sb = sb; e.slab_stride = slab_stride;
        e.A = A; e.TA = TA; e.B = B; e.Bp = pad_to(B, 8); e.ld = ld; e.kpad = kpad; e.nslabs = nslabs;
        e.clear = clear ? 1 : 0; e.scale = scale;
        if (ld < TH * TW * e.Bp || (pk && kpad < TH * TW * e.Bp)) return FMRI_E_BADARG;
    }
    const int tiles = apply_entry_tiles(e, TH, TW, KW, py, px, step, stb);
    memcpy(host_entry, &e, sizeof(e));
    return tiles;
}

int fmri_apply_batch(const void* table_dev, int n, int total_tiles, int mode, const float* lr_dev, float alpha, float eps,
                     float gscale, const float* gdev, float clamp, const int* flag, int gated, void* stream) {
    if (!table_dev || n < 0 || total_tiles < 0 || mode < 0 || mode > 3 || ((mode == 1 || mode == 3) && !lr_dev)) return FMRI_E_BADARG;
    ApplyOpt o;
    o.lr_dev = lr_dev; o.gdev = gdev; o.flag = flag; o.alpha = alpha; o.eps = eps; o.gscale = gscale; o.clamp = clamp;
    o.mode = mode; o.gated = gated ? 1 : 0;
    return apply_batch_launch((const ApplyEntry*)table_dev, n, total_tiles, o, S(stream));
}

int fmri_apply_batch_stats(const void* table_dev, int n, int total_tiles, int mode, const float* lr_dev, float alpha,
                           float eps, float gscale, const float* gdev, float clamp, const int* flag, int gated,
                           fmri_stat* part, void* stream) {
    if (!table_dev || !part || ((uintptr_t)part & 7) || n < 0 || total_tiles < 0 || (mode != 1 && mode != 3) || !lr_dev)
        return FMRI_E_BADARG;
    ApplyOpt o;
    o.lr_dev = lr_dev; o.gdev = gdev; o.flag = flag; o.alpha = alpha; o.eps = eps; o.gscale = gscale; o.clamp = clamp;
    o.mode = mode; o.gated = gated ? 1 : 0;
    return apply_batch_stats_launch((const ApplyEntry*)table_dev, n, total_tiles, o, (StatRec*)part, S(stream));
}
int fmri_stat_fold(const fmri_stat* part, int nrec, const int* flag, fmri_stat* out, void* stream) {
    if (!part || !out || nrec < 0 || ((uintptr_t)part & 7) || ((uintptr_t)out & 7)) return FMRI_E_BADARG;
    return stat_fold_launch((const StatRec*)part, nrec, flag, (StatRec*)out, S(stream));
}
int fmri_tensor_stats_ws_bytes(int nseg) {
    return nseg < 1 || nseg > FMRI_STAT_MAX_SEGS ? 0 : nseg * STAT_BLOCKS * (int)sizeof(StatRec);
}
int fmri_tensor_stats(const fmri_stat_seg* segs, int nseg, void* ws, void* stream) {
    if (!segs || nseg < 1 || nseg > FMRI_STAT_MAX_SEGS || !ws || ((uintptr_t)ws & 7)) return FMRI_E_BADARG;
    StatSegs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < nseg; ++i) {
        const fmri_stat_seg& g = segs[i];
        if (!g.x || !g.out || ((uintptr_t)g.out & 7) || g.rows < 0 || g.cols < 1 || g.ld < g.cols) return FMRI_E_BADARG;
        StatSeg& d = a.s[i];
        d.x = g.x; d.rows = g.rows; d.cols = g.cols; d.ld = g.ld; d.div = g.div; d.gate = g.gate;
        d.out = (StatRec*)g.out; d.scale = g.scale; d.clamp = g.clamp;
        const int64_t n = g.rows * g.cols, want = (n + 2047) / 2048;
        a.nblk[i] = (int)(want < 1 ? 1 : (want > STAT_BLOCKS ? STAT_BLOCKS : want));
    }
    return tensor_stats_launch(a, nseg, (StatRec*)ws, S(stream));
}

int fmri_unpack_grad(const float* src, float* dst, int64_t sa, int64_t sta, int64_t sb, int64_t stb, int A, int TA,
                     int B, int KW, int py, int px, int step, int TH, int TW, int ld, float scale, int accumulate,
                     int nslabs, int64_t slab_stride, void* stream) {
    if (!src || !dst || A < 1 || TA < 1 || B < 1 || nslabs < 1) return FMRI_E_BADARG;
    UnpackArgs p;
    p.src = src; p.dst = dst; p.sa = sa; p.sta = sta; p.sb = sb; p.stb = stb;
    p.A = A; p.TA = TA; p.B = B; p.Bp = pad_to(B, 8);
    p.KW = KW; p.py = py; p.px = px; p.step = step; p.TH = TH; p.TW = TW;
    p.ld = ld; p.scale = scale; p.accumulate = accumulate; p.nslabs = nslabs; p.slab_stride = slab_stride;
    if (ld < TH * TW * p.Bp) return FMRI_E_BADARG;
    return unpack_grad_launch(p, S(stream));
}

int fmri_igemm(const void* in, const void* w, void* out, const float* bias, const void* zero16, int N, int Hi, int Wi,
               int Ci, int Ho, int Wo, int CoStore, int Co, int k, int stride, int pad, int mode, int act,
               int out_f32, int splits, int64_t slab_stride, int bn_tile, void* stream) {
    return fmri_igemm_ep(in, w, out, bias, zero16, N, Hi, Wi, Ci, Ho, Wo, CoStore, Co, k, stride, pad, mode, act, out_f32,
                         splits, slab_stride, bn_tile, 0, nullptr, nullptr, stream);
}

int fmri_igemm_route(int N, int Hi, int Wi, int Ci, int Ho, int Wo, int CoStore, int Co, int k, int stride, int pad,
                     int mode, int act, int out_f32, int splits, int bn_tile, int64_t w_elems, int has_bias,
                     int stat_rows_cap, int stat_group_n, int want_bn_bwd, int want_act_y, int want_affine, char* name_out,
                     int cap) {
    if (!name_out || cap < 2) return FMRI_E_BADARG;
    name_out[0] = 0;
    // the routing decisions read sizes, flags and NULL-ness only: every pointer is a non-NULL dummy that is never
    // dereferenced, every launcher stops at route_probe()
    void* const dummy = (void*)(uintptr_t)64;
    fmri_epilogue e;
    memset(&e, 0, sizeof(e));
    if (stat_rows_cap > 0) { e.stat_part = (float*)dummy; e.stat_rows_cap = stat_rows_cap; e.stat_group_n = stat_group_n; }
    if (want_bn_bwd) {
        e.bn_x = dummy; e.bn_gamma = (const float*)dummy; e.bn_beta = (const float*)dummy; e.bn_relu = 1;
        for (int i = 0; i < 4; ++i) { e.bn_mean[i] = (const float*)dummy; e.bn_rstd[i] = (const float*)dummy; }
    }
    if (want_act_y) e.act_y = dummy;
    if (want_affine) { e.aff_scale = (const float*)dummy; e.aff_shift = (const float*)dummy; }
    const bool any_ep = stat_rows_cap > 0 || want_bn_bwd || want_act_y || want_affine;
    int done = 0;
    t_probe_name[0] = 0;
    t_probe_on = true;
    const int r = fmri_igemm_ep(dummy, dummy, dummy, has_bias ? (const float*)dummy : nullptr, dummy, N, Hi, Wi, Ci, Ho, Wo,
                                CoStore, Co, k, stride, pad, mode, act, out_f32, splits, 0, bn_tile, w_elems,
                                any_ep ? &e : nullptr, &done, nullptr);
    t_probe_on = false;
    if (r != FMRI_OK) return r;
    snprintf(name_out, (size_t)cap, "%s", t_probe_name[0] ? t_probe_name : "none");
    return FMRI_OK;
}

// kill switch of a kernel family: FMRI_<family>=off (only "off") disables it; call sites keep the answer in a static
static bool family_off(const char* var) { const char* v = getenv(var); return v && !strcmp(v, "off"); }
// What the family selectors route a validated fmri_igemm_ep call on besides the tap-list kernel's arguments a (a.st,
// a.bb: the statistics and BatchNorm-backward epilogues as the caller requested them).
struct IgemmReq {
    AffEpi aff;
    const half_t* act_y;
    int mode, k, stride, pad, bn_tile, copad, maxM;
    bool out_f32;
    int64_t w_elems;
    int* ep_done;
    hipStream_t st;
};
// Statistics-row planner (StatEpi): a block writes one row per statistics group it covers, so the group_n images of a
// group (0: one group of all ntiles tiles) must fill whole tiles of ipt images (tpi tiles per ipt images) and whole
// blocks of tpb tiles (the caller picks tpb), and a group's rows (mult per block) must fit rows_cap.  Sets st.tpg[cls]
// to the rows per group; false: statistics were requested and do not fit.  The caller's decline policy is
// plain_output(), or E_UNSUPPORTED to leave the call to the narrower family.
static bool plan_stat_rows(StatEpi& st, int cls, int64_t group_n, int64_t ipt, int64_t tpi, int64_t ntiles, int tpb, int mult) {
    if (!st.part) return true;
    const int64_t tiles = group_n > 0 ? (group_n + ipt - 1) / ipt * tpi : ntiles;
    st.tpg[cls] = (int)((tiles + tpb - 1) / tpb) * mult;
    return group_n % ipt == 0 && st.tpg[cls] <= st.rows_cap;
}
// decline policy of the narrow forms: no statistics rows, no BatchNorm-backward masking (*ep_done = 0 tells the caller)
static void plain_output(StatEpi& st, BnBwdEpi& bb) { st.part = nullptr; bb.x = nullptr; }
// *ep_done after a launch: statistics rows per group (summed over the classes; 0: none) | flags of the epilogues applied
static int ep_report(int r, int* ep_done, const StatEpi* st, const float* aff_scale, const half_t* relu_y) {
    if (r == OK && ep_done)
        *ep_done = (st && st->part ? st->tpg[0] + st->tpg[1] + st->tpg[2] + st->tpg[3] : 0) |
                   (aff_scale ? FMRI_EP_AFFINE_APPLIED : 0) | (relu_y ? FMRI_EP_ACT_APPLIED : 0);
    return r;
}
// The class geometry of a k5 p2 stride-2 transposed convolution that igemm_tc5 and igemm_tc32 hard-wire: class i writes
// output parity (i >> 1, i & 1); parity-0 classes have 3 taps from input offset +1 downwards, parity-1 classes 2 taps.
static bool k5p2_classes(const IgemmArgs& a) {
    for (int i = 0; i < 4; ++i) {
        const IgemmClass& s = a.cls[i];
        if (s.T / s.TW != ((i >> 1) ? 2 : 3) || s.TW != ((i & 1) ? 2 : 3) || s.dy0 != 1 || s.dx0 != 1 || s.dstep != -1 ||
            s.oy0 != (i >> 1) || s.ox0 != (i & 1) || s.Kpad < s.T * a.Ci)
            return false;
    }
    return true;
}

// Every family selector below returns its launcher's code, or E_UNSUPPORTED to pass the call on to the next family.
// 5x5 stride-1 convolutions between 3(8)- and 32-channel maps -> register-resident-weight kernel
// (csrc/igemm_narrow.hip); FMRI_NARROW=off disables
static int select_narrow(const IgemmArgs& a, const IgemmReq& r) {
    static const bool off = family_off("FMRI_NARROW");
    const int co_tiles = a.Co <= 16 ? 1 : 2;
    if (off || (r.mode != FMRI_CONV && r.mode != FMRI_CONV_FLIP) || r.stride != 1 || r.k != 5 || r.pad != 2 ||
        !(a.Ci == 8 || (a.Ci == 32 && co_tiles == 1)) || a.Co > 32 || r.out_f32 || a.splits != 1 || a.Hi != a.Ho ||
        a.Wi != a.Wo || (int64_t)a.N * a.Hi * a.Wi * 32 >= 0x7fffffffLL || r.copad < co_tiles * 16 ||
        a.cls[0].Kpad < (a.Ci == 32 ? 800 : 224))
        return E_UNSUPPORTED;
    NarrowArgs q;
    q.in = a.in; q.w = a.w + a.cls[0].w_off; q.out = (half_t*)a.out; q.bias = a.bias;
    q.N = a.N; q.H = a.Hi; q.W = a.Wi; q.CoStore = a.CoStore; q.Co = a.Co; q.Kpad = a.cls[0].Kpad; q.act = a.act;
    q.tiles_y = (a.Hi + 15) / 16; q.tiles_x = (a.Wi + 15) / 16; q.ntiles = a.N * q.tiles_y * q.tiles_x;
    return igemm_narrow_launch(q, a.Ci, co_tiles, r.mode == FMRI_CONV_FLIP, r.st);
}
// wide form of the c5 family (csrc/igemm_c5w.hip): 16 x 16-pixel tiles of one image or 8 x 8-pixel tiles of four, one
// 8-wave block per CU, loader / compute waves; FMRI_C5W=off disables.  n: the narrow form's arguments
static int select_c5w(const IgemmArgs& a, const IgemmReq& r, const C5Args& n) {
    static const bool off = family_off("FMRI_C5W");
    // (gated on the caller's REQUEST for the BatchNorm-backward epilogue, bb.x: the wide kernel has none, and the narrow
    // form clears its bb.x when its rows do not fit -- the wide form, needing fewer rows, would then emit FORWARD
    // statistics rows that the caller reads as (sum g, sum g*xhat))
    if (off || a.bb.x || (n.pw16 && a.Ho <= 8)) return E_UNSUPPORTED;
    C5Args w = n;
    const int ipb = n.pw16 ? 1 : 4, ph = n.pw16 ? 16 : 8, ncol = r.copad / 128, group_n = n.st.group_n;
    w.tiles_y = (a.Ho + ph - 1) / ph;
    w.ntiles = ((a.N + ipb - 1) / ipb) * w.tiles_y * w.tiles_x;
    w.fdTPI = make_fastdiv((uint32_t)(w.tiles_y * w.tiles_x));
    const int tpg = group_n > 0 ? (group_n / ipb) * w.tiles_y * w.tiles_x : w.ntiles;
    // whole rounds of one block per CU, statistics groups not sharing a block
    w.tpb = 1;
    for (int t = (w.ntiles * ncol) / 256; t > 1; --t)
        if (tpg % t == 0 && w.ntiles % t == 0 && ((w.ntiles / t) * ncol) % 256 == 0) { w.tpb = t; break; }
    if (!plan_stat_rows(w.st, 0, group_n, ipb, w.tiles_y * w.tiles_x, w.ntiles, w.tpb, 1)) return E_UNSUPPORTED;
    w.aff = r.aff;
    return ep_report(igemm_c5w_launch(w, r.copad, r.st), r.ep_done, &w.st, w.aff.scale, nullptr);
}
// stride-2 convolution k5 p2, Ci % 32 == 0, 128-channel tiles, no bias / activation -> window-resident kernels: the wide
// form, then csrc/igemm_c5.hip; FMRI_C5=off disables both
static int select_c5(const IgemmArgs& a, const IgemmReq& r) {
    static const bool off = family_off("FMRI_C5");
    const IgemmClass& c = a.cls[0];
    if (off || r.mode != FMRI_CONV || r.stride != 2 || r.k != 5 || r.pad != 2 || (a.Ci & 31) || r.bn_tile != 128 ||
        r.out_f32 || a.splits != 1 || a.bias || a.act != FMRI_ACT_NONE ||
        a.Ho != (a.Hi - 1) / 2 + 1 || a.Wo != (a.Wi - 1) / 2 + 1 || c.Kpad < 25 * a.Ci ||
        (int64_t)a.N * a.Hi * a.Wi * a.Ci * 2 >= 0x7fffffffLL || (int64_t)r.copad * c.Kpad * 2 >= 0xffffffffLL ||
        (r.w_elems != 0 && r.w_elems < (int64_t)r.copad * c.Kpad))
        return E_UNSUPPORTED;
    C5Args q;
    memset(&q, 0, sizeof(q));      // no affine epilogue
    q.in = a.in; q.w = a.w + c.w_off; q.out = (half_t*)a.out;
    q.N = a.N; q.Hi = a.Hi; q.Wi = a.Wi; q.Ci = a.Ci; q.Ho = a.Ho; q.Wo = a.Wo; q.CoStore = a.CoStore; q.Co = a.Co;
    q.Kpad = c.Kpad; q.nsub = a.Ci / 32;
    q.pw16 = a.Wo > 8 ? 1 : 0;
    const int ipb = q.pw16 ? 1 : 2;
    q.tiles_x = q.pw16 ? (a.Wo + 15) / 16 : 1;
    q.tiles_y = (a.Ho + 7) / 8;
    q.ntiles = ((a.N + ipb - 1) / ipb) * q.tiles_y * q.tiles_x;
    q.in_bytes = (uint32_t)((int64_t)a.N * a.Hi * a.Wi * a.Ci * 2);
    q.w_bytes = (uint32_t)((int64_t)r.copad * q.Kpad * 2);
    q.fdTPI = make_fastdiv((uint32_t)(q.tiles_y * q.tiles_x));
    q.fdTX = make_fastdiv((uint32_t)q.tiles_x);
    q.st = a.st; q.bb = a.bb;
    // persistent blocks: tpb consecutive tiles each when that makes whole rounds of 2 blocks per CU
    q.tpb = (q.ntiles * (r.copad / 128)) / 512;      // whole rounds only: fewer, longer blocks leave CUs idle
    if (q.tpb < 1) q.tpb = 1;
    const int rw = select_c5w(a, r, q);
    if (rw != E_UNSUPPORTED) return rw;
    // statistics: one row per block; the blocks of a group's tiles must not reach into the next group
    const int group_n = q.st.group_n, tpi = q.tiles_y * q.tiles_x;
    if (q.st.part && group_n > 0 && group_n % ipb == 0)
        while (((group_n / ipb) * tpi) % q.tpb) --q.tpb;
    if (!plan_stat_rows(q.st, 0, group_n, ipb, tpi, q.ntiles, q.tpb, 1)) plain_output(q.st, q.bb);
    return ep_report(igemm_c5_launch(q, r.copad, r.st), r.ep_done, &q.st, nullptr, nullptr);
}
// wide form of the tc5 family (csrc/igemm_tc5w.hip): 16 x 16-position tiles, one 8-wave block per CU, loader / compute
// waves; FMRI_TC5W=off disables.  n: the narrow form's arguments
static int select_tc5w(const IgemmArgs& a, const IgemmReq& r, const Tc5Args& n) {
    static const bool off = family_off("FMRI_TC5W");
    const int Yc0 = a.cls[0].Yc, Xc0 = a.cls[0].Xc;
    const bool wide16 = Xc0 > 8 && Yc0 > 8;
    const bool wide8 = Xc0 <= 8 && Yc0 <= 8 && a.Hi <= 8 && a.Wi <= 8;
    if (off || r.bn_tile != 128 || !(wide16 || wide8) || a.bb.x || (n.nchunks & 1)) return E_UNSUPPORTED;  // bb.x: as c5w
    Tc5Args w = n;
    if (wide16) {
        w.pw_log2 = 4; w.ph_log2 = 4; w.PH = 16; w.IPB = 1; w.IH = 18; w.IW = 18; w.nslice = 11;
        w.tiles_x = (Xc0 + 15) / 16;
        w.tiles_y = (Yc0 + 15) / 16;
        w.ntiles = a.N * w.tiles_y * w.tiles_x;
    } else {
        w.pw_log2 = 3; w.ph_log2 = 3; w.PH = 8; w.IPB = 4; w.IH = 10; w.IW = 10; w.nslice = 13;
        w.tiles_x = w.tiles_y = 1;
        w.ntiles = (a.N + 3) / 4;
    }
    w.fdTPI = make_fastdiv((uint32_t)(w.tiles_y * w.tiles_x));
    w.fdTX = make_fastdiv((uint32_t)w.tiles_x);
    // few tiles (at most 128 tile x column-block pairs): one parity class per block, grid.z = 4, one row per class block
    w.solo = w.ntiles * (r.copad / 128) <= 128 ? 1 : 0;
    if (!plan_stat_rows(w.st, 0, w.st.group_n, w.IPB, w.tiles_y * w.tiles_x, w.ntiles, 1, w.solo ? 4 : 1))
        return E_UNSUPPORTED;
    w.aff = r.aff;
    return ep_report(igemm_tc5w_launch(w, r.copad, r.st), r.ep_done, &w.st, w.aff.scale, nullptr);
}
// stride-2 transposed convolution k5 p2, Ci % 128 == 0, >= 64 output channels, no bias / activation: all four parity
// classes per block -- the wide form, then csrc/igemm_tc5.hip; FMRI_TC5=off disables both
static int select_tc5(const IgemmArgs& a, const IgemmReq& r) {
    static const bool off = family_off("FMRI_TC5");
    if (off || r.mode != FMRI_TCONV2 || r.k != 5 || r.pad != 2 || (a.Ci & 127) || r.bn_tile < 64 || r.out_f32 ||
        a.splits != 1 || a.bias || a.act != FMRI_ACT_NONE || r.w_elems <= 0 || r.w_elems * 2 >= 0xffffffffLL ||
        (int64_t)a.N * a.Hi * a.Wi * a.Ci * 2 >= 0x7fffffffLL || !k5p2_classes(a))
        return E_UNSUPPORTED;
    Tc5Args q;
    memset(&q, 0, sizeof(q));      // no bias, affine epilogue or one-class-per-block form
    q.in = a.in; q.w = a.w; q.out = (half_t*)a.out;
    q.N = a.N; q.Hi = a.Hi; q.Wi = a.Wi; q.Ci = a.Ci; q.Ho = a.Ho; q.Wo = a.Wo; q.CoStore = a.CoStore; q.Co = a.Co;
    q.act = a.act; q.nchunks = a.Ci / 64;
    for (int i = 0; i < 4; ++i) {
        if (a.cls[i].w_off + (int64_t)r.copad * a.cls[i].Kpad > r.w_elems) return E_UNSUPPORTED;
        q.cls[i] = {a.cls[i].Yc, a.cls[i].Xc, a.cls[i].Kpad, 0, a.cls[i].w_off};
    }
    const int Yc0 = a.cls[0].Yc, Xc0 = a.cls[0].Xc;          // class (0, 0) has the largest grid
    q.pw_log2 = Xc0 > 8 ? 4 : 3;
    q.ph_log2 = (q.pw_log2 == 3 && Yc0 > 8) ? 4 : 3;
    q.PH = 1 << q.ph_log2;
    q.IPB = 128 >> (q.pw_log2 + q.ph_log2);
    q.IH = q.PH + 2;
    q.IW = (1 << q.pw_log2) + 2;
    q.tiles_x = (Xc0 + (1 << q.pw_log2) - 1) >> q.pw_log2;
    q.tiles_y = (Yc0 + q.PH - 1) >> q.ph_log2;
    q.ntiles = Yc0 > 0 && Xc0 > 0 ? ((a.N + q.IPB - 1) / q.IPB) * q.tiles_y * q.tiles_x : 0;
    q.nslice = (q.IPB * q.IH * q.IW * 8 + 255) / 256;
    // whole class grid (and input) inside one 8 x 8 tile per image: the window's halo is all padding -> dense form
    if (q.IPB == 2 && q.tiles_x == 1 && q.tiles_y == 1 && a.Hi <= 8 && a.Wi <= 8) q.nslice = 4;
    q.in_bytes = (uint32_t)((int64_t)a.N * a.Hi * a.Wi * a.Ci * 2);
    q.w_bytes = (uint32_t)(r.w_elems * 2);
    q.fdTPI = make_fastdiv((uint32_t)(q.tiles_y * q.tiles_x));
    q.fdTX = make_fastdiv((uint32_t)q.tiles_x);
    q.fdIHW = make_fastdiv((uint32_t)(q.IH * q.IW));
    q.fdIW = make_fastdiv((uint32_t)q.IW);
    q.st = a.st; q.bb = a.bb;
    const int rw = select_tc5w(a, r, q);
    if (rw != E_UNSUPPORTED || q.ntiles < 1) return rw;
    // statistics: one row per tile
    if (!plan_stat_rows(q.st, 0, q.st.group_n, q.IPB, q.tiles_y * q.tiles_x, q.ntiles, 1, 1)) plain_output(q.st, q.bb);
    return ep_report(igemm_tc5_launch(q, r.bn_tile, r.copad, r.st), r.ep_done, &q.st, nullptr, nullptr);
}
// stride-2 transposed convolution 128 -> <= 32 channels -> persistent register-resident-weight kernel
// (csrc/igemm_tc32.hip); FMRI_TC32=off disables
static int select_tc32(const IgemmArgs& a, const IgemmReq& r) {
    static const bool off = family_off("FMRI_TC32");
    const int tiles_y = (a.cls[0].Yc + 7) / 8, tiles_x = (a.cls[0].Xc + 15) / 16;     // class (0,0) has the largest grid
    if (off || r.mode != FMRI_TCONV2 || a.Ci != 128 || a.CoStore > 32 || r.out_f32 || a.splits != 1 ||
        (int64_t)a.N * a.Hi * a.Wi * 128 >= 0x7fffffffLL || r.copad < 32 || r.k != 5 || r.pad != 2 || !k5p2_classes(a) ||
        a.N * tiles_y * tiles_x < 1)
        return E_UNSUPPORTED;
    Tc32Args q;
    q.in = a.in; q.w = a.w; q.out = (half_t*)a.out; q.bias = a.bias;
    q.N = a.N; q.Hi = a.Hi; q.Wi = a.Wi; q.Ho = a.Ho; q.Wo = a.Wo; q.CoStore = a.CoStore; q.Co = a.Co; q.act = a.act;
    for (int i = 0; i < 4; ++i) q.cls[i] = {a.cls[i].Yc, a.cls[i].Xc, a.cls[i].Kpad, 0, a.cls[i].w_off};
    q.tiles_y = tiles_y; q.tiles_x = tiles_x; q.ntiles = a.N * tiles_y * tiles_x;
    q.relu_y = r.act_y;
    const int begin = q.ntiles < 256 ? q.ntiles : 256;                          // one persistent block per CU
    // E_UNSUPPORTED: bias / activation epilogue
    return ep_report(igemm_tc32_launch(q, begin, r.st), r.ep_done, nullptr, nullptr, q.relu_y);
}
// generic tap-list kernel (csrc/igemm.hip): one statistics row per row tile of bm output positions, so the planner's
// images are a class's output positions here -- a tile must not straddle two statistics groups
static int select_generic(IgemmArgs& a, const IgemmReq& r) {
    if (a.st.part) {
        const int bm = igemm_bm(a, r.maxM, r.bn_tile, r.copad, false);
        bool fits = true;
        int rows = 0;
        for (int i = 0; i < a.ncls; ++i) {
            const IgemmClass& c = a.cls[i];
            fits &= plan_stat_rows(a.st, i, (int64_t)a.st.group_n * c.Yc * c.Xc, bm, 1, ((int64_t)c.M + bm - 1) / bm, 1, 1);
            rows += a.st.tpg[i];
        }
        if (!fits || rows > a.st.rows_cap) plain_output(a.st, a.bb);
    }
    return ep_report(igemm_launch(a, r.maxM, r.bn_tile, r.copad, r.out_f32, r.st), r.ep_done, &a.st, nullptr, nullptr);
}

// the output-pixel classes of the contraction: one for a convolution, the four parity classes of a stride-2 transposed
// convolution; *maxM = the rows of the largest
static int igemm_classes(IgemmArgs& a, int mode, int k, int stride, int pad, int copad, int* maxM) {
    *maxM = 0;
    auto set_class = [&](IgemmClass& c, int Yc, int Xc, int oy0, int ox0, int TH, int TW, int dy0, int dx0, int dstep,
                         int kpad, int64_t w_off) -> bool {
        c.Yc = Yc; c.Xc = Xc; c.oy0 = oy0; c.ox0 = ox0; c.T = TH * TW; c.TW = TW;
        c.dy0 = dy0; c.dx0 = dx0; c.dstep = dstep;
        const int64_t M = (int64_t)a.N * Yc * Xc;
        if (M > 0x7fffff00LL) return false;
        c.M = (int)(M > 0 ? M : 0);
        c.Kpad = kpad; c.ksteps = kpad / 64; c.w_off = w_off;
        c.fdX = make_fastdiv((uint32_t)(Xc > 0 ? Xc : 1));
        c.fdYX = make_fastdiv((uint32_t)(Yc * Xc > 0 ? Yc * Xc : 1));
        c.fdTW = make_fastdiv((uint32_t)TW);
        if (c.M > *maxM) *maxM = c.M;
        return true;
    };
    if (mode == FMRI_CONV || mode == FMRI_CONV_FLIP) {
        if (mode == FMRI_CONV_FLIP && stride != 1) return FMRI_E_UNSUPPORTED;
        a.s = stride; a.os = 1; a.ncls = 1;
        const int d0 = mode == FMRI_CONV ? -pad : pad, ds = mode == FMRI_CONV ? 1 : -1;
        if (!set_class(a.cls[0], a.Ho, a.Wo, 0, 0, k, k, d0, d0, ds, pad_to(k * k * a.Ci, 64), 0)) return FMRI_E_BADARG;
        for (int i = 1; i < 4; ++i) a.cls[i] = a.cls[0];
    } else if (mode == FMRI_TCONV2) {
        if (stride != 2) return FMRI_E_UNSUPPORTED;
        a.s = 1; a.os = 2; a.ncls = 4;
        TClass tc[4];
        tconv_classes(k, pad, a.Ci, copad, tc);
        for (int cy = 0; cy < 2; ++cy)
            for (int cx = 0; cx < 2; ++cx) {
                const TClass& t = tc[cy * 2 + cx];
                const int Yc = (a.Ho - cy + 1) / 2, Xc = (a.Wo - cx + 1) / 2;
                if (!set_class(a.cls[cy * 2 + cx], Yc, Xc, cy, cx, t.th, t.tw, t.dy0, t.dx0, -1, t.kpad, t.w_off))
                    return FMRI_E_BADARG;
            }
    } else {
        return FMRI_E_UNSUPPORTED;
    }
    // no empty split: every split must own >= 1 K-step in every class
    for (int i = 0; i < a.ncls; ++i) {
        const int per = (a.cls[i].ksteps + a.splits - 1) / a.splits;
        if (per * (a.splits - 1) >= a.cls[i].ksteps && a.splits > 1) return FMRI_E_BADARG;
    }
    return FMRI_OK;
}

int fmri_igemm_ep(const void* in, const void* w, void* out, const float* bias, const void* zero16, int N, int Hi,
                  int Wi, int Ci, int Ho, int Wo, int CoStore, int Co, int k, int stride, int pad, int mode, int act,
                  int out_f32, int splits, int64_t slab_stride, int bn_tile, int64_t w_elems, const fmri_epilogue* ep,
                  int* ep_done, void* stream) {
    if (ep_done) *ep_done = 0;
    if (!in || !w || !out || !zero16) return FMRI_E_BADARG;
    IgemmArgs a;
    AffEpi aff;
    memset(&a, 0, sizeof(a));      // no statistics, BatchNorm backward or affine epilogue unless ep asks
    memset(&aff, 0, sizeof(aff));
    a.st.C = CoStore;
    if (ep && ep->bn_x && !ep->stat_part) return FMRI_E_BADARG;
    if (ep && ep->aff_scale) {
        if (!ep->aff_shift || ep->stat_part || bias || act != FMRI_ACT_NONE || out_f32) return FMRI_E_BADARG;
        aff.scale = ep->aff_scale; aff.shift = ep->aff_shift; aff.relu = ep->aff_relu ? 1 : 0;
    }
    if (ep && ep->stat_part) {
        if (ep->stat_rows_cap < 1 || ep->stat_group_n < 0 || out_f32 || (ep->stat_group_n > 0 && N % ep->stat_group_n))
            return FMRI_E_BADARG;
        a.st.part = ep->stat_part; a.st.rows_cap = ep->stat_rows_cap; a.st.group_n = ep->stat_group_n;
        if (ep->bn_x) {
            // BatchNorm backward: <= 4 groups, every used group fully described; no bias / activation
            const int groups = a.st.group_n > 0 ? N / a.st.group_n : 1;
            if (groups > 4 || !ep->bn_gamma || !ep->bn_beta || bias || act != FMRI_ACT_NONE || Co != CoStore)
                return FMRI_E_BADARG;
            a.bb.x = (const half_t*)ep->bn_x; a.bb.gamma = ep->bn_gamma; a.bb.beta = ep->bn_beta; a.bb.relu = ep->bn_relu;
            for (int i = 0; i < groups; ++i) {
                if (!ep->bn_mean[i] || !ep->bn_rstd[i] || ep->bn_x_img0[i] < 0) return FMRI_E_BADARG;
                a.bb.mean[i] = ep->bn_mean[i]; a.bb.rstd[i] = ep->bn_rstd[i]; a.bb.x_img0[i] = ep->bn_x_img0[i];
            }
        }
    }
    if (N < 1 || Ci < 8 || (Ci & 7) || CoStore < 4 || (CoStore & 3) || Co < 1 || Co > CoStore) return FMRI_E_BADARG;
    if (bn_tile != 32 && bn_tile != 64 && bn_tile != 128) return FMRI_E_UNSUPPORTED;
    if (splits < 1 || (splits > 1 && !out_f32)) return FMRI_E_BADARG;
    const int copad = pad_to(Co, bn_tile);
    if (copad < CoStore) return FMRI_E_BADARG;   // every stored channel must be covered by a tile
    a.in = (const half_t*)in; a.w = (const half_t*)w; a.out = out; a.bias = bias; a.zero = (const half_t*)zero16;
    a.N = N; a.Hi = Hi; a.Wi = Wi; a.Ci = Ci; a.Ho = Ho; a.Wo = Wo; a.CoStore = CoStore; a.Co = Co;
    a.act = act; a.splits = splits; a.slab_stride = slab_stride;
    a.fdCi = make_fastdiv((uint32_t)Ci);
    a.fdCpt = make_fastdiv((uint32_t)(Ci >= 64 ? Ci / 64 : 1));
    int maxM;
    const int e = igemm_classes(a, mode, k, stride, pad, copad, &maxM);
    if (e != FMRI_OK || maxM == 0) return e;
    const IgemmReq r = {aff, ep ? (const half_t*)ep->act_y : nullptr, mode, k, stride, pad, bn_tile, copad, maxM,
                        out_f32 != 0, w_elems, ep_done, S(stream)};
    // the specialised families in order of preference, then the generic tap-list kernel
    for (auto select : {select_narrow, select_c5, select_tc5, select_tc32}) {
        const int ret = select(a, r);
        if (ret != E_UNSUPPORTED) return ret;
    }
    return select_generic(a, r);
}

// K pieces (8 x 8 pixel tiles per block) of the four parity planes of fmri_wgrad's window kernel for a budget of `splits`
// blocks per (row block, column block) over the planes.  A K-step costs ~128 cycles per shift of the plane (8 MFMAs of one
// wave) + ~550 of barrier, fragment reads and waits (csrc/wgrad_win.hip, measured 1 825 / 1 430 / 1 033 cycles at 9 / 6 / 4
// shifts), so the planes get pieces in inverse proportion: all blocks of a launch finish together.  Returns the number of pieces of the plane with the most (= slabs written).
static int wgrad_plane_pieces(int N, int Yc, int Xc, int k, int pad, int splits, int tps_out[4]) {
    const int ntiles = N * ((Yc + 7) / 8) * ((Xc + 7) / 8);
    int nsh[2] = {0, 0};
    for (int t = 0; t < k; ++t) ++nsh[(t - pad) & 1];
    int total = splits < 4 ? 4 : splits;
    total -= total & 3;
    double cost[4], csum = 0;
    for (int pl = 0; pl < 4; ++pl) { cost[pl] = 128.0 * nsh[pl >> 1] * nsh[pl & 1] + 550.0; csum += cost[pl]; }
    int smax = 1;
    for (int pl = 0; pl < 4; ++pl) {
        int sp = (int)(total * cost[pl] / csum + 0.5);
        if (sp < 1) sp = 1;
        if (sp > ntiles) sp = ntiles > 0 ? ntiles : 1;
        const int tps = (ntiles + sp - 1) / sp;
        tps_out[pl] = tps < 1 ? 1 : tps;
        const int pieces = ntiles > 0 ? (ntiles + tps_out[pl] - 1) / tps_out[pl] : 1;
        if (pieces > smax) smax = pieces;
    }
    return smax;
}

// number of per-split slabs fmri_wgrad(..., atomic = 2) writes for a budget of `splits` blocks per tile group
int fmri_wgrad_slabs(int N, int Yc, int Xc, int k, int pad, int splits) {
    int tps[4];
    return wgrad_plane_pieces(N, Yc, Xc, k, pad, splits, tps);
}

static int wgrad_narrow_blocks(int N, int Yc, int Xc) {
    const int64_t ntiles = (int64_t)N * ((Yc + 7) / 8) * ((Xc + 7) / 8);
    int64_t nb = (ntiles + 31) / 32;                // >= 16 tiles per wave PAIR, at most three 4-wave blocks per CU
    if (nb > 768) nb = 768;
    if (nb < 1) nb = 1;
    return (int)nb;
}
int fmri_wgrad_narrow_blocks(int N, int Yc, int Xc) {
    return (N < 1 || Yc < 1 || Xc < 1) ? 0 : wgrad_narrow_blocks(N, Yc, Xc);
}

int fmri_set_deterministic(int on) {
    const int was = g_deterministic;
    g_deterministic = on ? 1 : 0;
    return was;
}
int fmri_get_deterministic(void) { return g_deterministic; }

int fmri_wgrad(const void* P, const void* Q, float* out, const void* zero16, int N, int Yc, int Xc, int A, int Hq,
               int Wq, int Bc, int k, int stride, int pad, int flip, int apad, int ba_tile, int ldo, int splits,
               int atomic, void* stream) {
    return fmri_wgrad_if(nullptr, P, Q, out, zero16, N, Yc, Xc, A, Hq, Wq, Bc, k, stride, pad, flip, apad, ba_tile, ldo,
                         splits, atomic, stream);
}

// One fmri_wgrad_if call.  A kernel family's geometry test (wgrad_win_fits, wgrad_narrow_fits) reads the sizes only: the
// dispatch of fmri_wgrad_if and the plan of fmri_wgrad_route ask the same one, so the plan cannot choose a kernel the
// dispatch would not run.
struct WgradReq {
    const int* gate; const half_t *P, *Q, *zero; float* out;
    int N, Yc, Xc, A, Hq, Wq, Bc, k, stride, pad, flip, apad, ba_tile, ldo, splits, atomic;
    hipStream_t st;
};
static int wgrad_check(const WgradReq& q) {
    if (!q.P || !q.Q || !q.out || !q.zero) return FMRI_E_BADARG;
    if (q.flip && q.stride != 1) return FMRI_E_UNSUPPORTED;
    if (q.N < 1 || q.A < 8 || (q.A & 7) || q.Bc < 8 || (q.Bc & 7) || q.k < 1 || q.splits < 1) return FMRI_E_BADARG;
    if (q.ba_tile != 32 && q.ba_tile != 64 && q.ba_tile != 128) return FMRI_E_UNSUPPORTED;
    if (q.apad % q.ba_tile || q.apad < q.A) return FMRI_E_BADARG;
    if (q.ldo % 128 || q.ldo < q.k * q.k * q.Bc) return FMRI_E_BADARG;
    if (q.splits > 1 && q.atomic == FMRI_WGRAD_STORE) return FMRI_E_BADARG;
    if (q.atomic < FMRI_WGRAD_STORE || q.atomic > FMRI_WGRAD_KSPLIT_SLABS) return FMRI_E_BADARG;
    const int64_t M = (int64_t)q.N * q.Yc * q.Xc;
    if (M < 1 || M > 0x7fffff00LL) return FMRI_E_BADARG;
    return FMRI_OK;
}
static int wgrad_tiles8(const WgradReq& q) { return q.N * ((q.Yc + 7) / 8) * ((q.Xc + 7) / 8); }
// taps of parity `par` of a k-tap window with padding `pad` under stride 2: their number, *tmin = the first one's source
// offset in the parity plane
static int wgrad_parity_taps(int k, int pad, int par, int* tmin) {
    int cnt = 0, emin = 0;
    for (int t = 0; t < k; ++t)
        if (((t - pad) & 1) == par) { if (!cnt) emin = t - pad; ++cnt; }
    *tmin = (emin - par) / 2;      // exact: emin and par have the same parity
    return cnt;
}
// 5x5 pad-2 stride-2 sampling (2 or 3 taps per parity), 128-row tiles, 32-channel column blocks, 32-bit buffer offsets:
// window-resident kernel (csrc/wgrad_win.hip).  FMRI_WGRAD_WIN=off disables.
static bool wgrad_win_fits(const WgradReq& q) {
    static const bool off = family_off("FMRI_WGRAD_WIN");
    if (off || q.stride != 2 || q.flip || q.k != 5 || q.pad != 2 || q.ba_tile != 128 || (q.Bc & 31) || q.Yc * q.Xc <= 1 ||
        (int64_t)q.N * q.Hq * q.Wq * q.Bc * 2 >= 0x80000000LL || (int64_t)q.N * q.Yc * q.Xc * q.A * 2 >= 0x80000000LL)
        return false;
    for (int par = 0; par < 2; ++par) {
        int tmin;
        const int cnt = wgrad_parity_taps(q.k, q.pad, par, &tmin);
        if (cnt < 2 || cnt > 3) return false;
    }
    return true;
}
// 5x5 stride-1 layers between 32 and 3(8) channels, P within 2^31 elements: wave-private window kernel
// (csrc/wgrad_narrow.hip).  FMRI_WGRAD_NARROW=off disables.
static bool wgrad_narrow_fits(const WgradReq& q) {
    static const bool off = family_off("FMRI_WGRAD_NARROW");
    return !off && q.stride == 1 && q.k == 5 && q.pad == 2 && q.A == 32 && q.Bc == 8 && q.apad == 32 && q.Yc == q.Hq &&
           q.Xc == q.Wq && (int64_t)q.N * q.Yc * q.Xc * 32 < 0x7fffffffLL;
}
// K steps of 64 rows per split of the generic kernel; *used = the splits that get any (<= splits)
static int wgrad_ksplit_steps(const WgradReq& q, int splits, int* used) {
    const int steps = (int)(((int64_t)q.N * q.Yc * q.Xc + 63) / 64);
    if (splits > steps) splits = steps;
    const int per = (steps + splits - 1) / splits;
    *used = (steps + per - 1) / per;
    return per;
}

// window-resident kernel, pre-zeroed fp32 output (FMRI_WGRAD_ATOMIC) or plane-piece slabs (FMRI_WGRAD_PLANE_SLABS)
static int wgrad_win(const WgradReq& q) {
    WgradWinArgs w;
    for (int par = 0; par < 2; ++par) w.nsy[par] = w.nsx[par] = wgrad_parity_taps(q.k, q.pad, par, &w.tmin[par]);
    w.gate = q.gate; w.P = q.P; w.Q = q.Q; w.out = q.out; w.zero = q.zero;
    w.N = q.N; w.Yc = q.Yc; w.Xc = q.Xc; w.A = q.A; w.Hq = q.Hq; w.Wq = q.Wq; w.Bc = q.Bc; w.pad = q.pad; w.TW = q.k;
    w.ldo = q.ldo; w.a_tiles = q.apad / 128;
    w.slab_stride = q.atomic == FMRI_WGRAD_PLANE_SLABS ? (int64_t)q.apad * q.ldo : 0;
    w.tiles_y = (q.Yc + 7) / 8; w.tiles_x = (q.Xc + 7) / 8; w.ntiles = wgrad_tiles8(q);
    // `splits` = blocks per (row block, column block) over the 4 planes; K pieces per plane: wgrad_plane_pieces()
    int tps4[4];
    const int smax = wgrad_plane_pieces(q.N, q.Yc, q.Xc, q.k, q.pad, q.splits, tps4);  // = fmri_wgrad_slabs(): in slab mode
    for (int pl = 0; pl < 4; ++pl) {                                                   // the caller sized the output with
        w.plane_tps[pl] = tps4[pl];                                                    // it, and every allocated slab is
        w.plane_pieces[pl] = (w.ntiles + tps4[pl] - 1) / tps4[pl];                     // written
    }
    w.splits = smax;
    w.fdTPI = make_fastdiv((uint32_t)(w.tiles_y * w.tiles_x));
    w.fdTX = make_fastdiv((uint32_t)w.tiles_x);
    return wgrad_win_launch(w, q.apad, q.st);
}
// generic weight-gradient kernel (csrc/wgrad.hip)
static int wgrad_generic(const WgradReq& q) {
    WgradArgs a;
    a.gate = q.gate; a.P = q.P; a.Q = q.Q; a.out = q.out; a.zero = q.zero;
    a.N = q.N; a.Yc = q.Yc; a.Xc = q.Xc; a.A = q.A; a.Hq = q.Hq; a.Wq = q.Wq; a.Bc = q.Bc;
    a.s = q.stride; a.T = q.k * q.k; a.TW = q.k;
    a.dy0 = q.flip ? q.pad : -q.pad; a.dx0 = a.dy0; a.dstep = q.flip ? -1 : 1;
    a.M = (int)((int64_t)q.N * q.Yc * q.Xc); a.ldo = q.ldo;
    // FMRI_WGRAD_KSPLIT_SLABS: the caller allocated `splits` (as passed in) slabs of apad x ldo; the kernel writes every
    // element of the first a.splits (<= splits) of them with plain stores, the rest stay as the caller left them
    // (zero-filled)
    a.steps_per_split = wgrad_ksplit_steps(q, q.splits, &a.splits);
    a.atomic = q.atomic == FMRI_WGRAD_KSPLIT_SLABS ? 2 : q.atomic;
    a.slab_stride = (int64_t)q.apad * q.ldo;
    a.ncol_chunks = a.T * q.Bc / 8;
    a.fdX = make_fastdiv((uint32_t)q.Xc);
    a.fdYX = make_fastdiv((uint32_t)(q.Yc * q.Xc));
    a.fdTW = make_fastdiv((uint32_t)q.k);
    a.fdBc8 = make_fastdiv((uint32_t)(q.Bc / 8));
    return wgrad_launch(a, q.apad, q.ba_tile, q.st);
}
// wave-private window kernel, `splits` pre-zeroed slabs (FMRI_WGRAD_NARROW_SLABS)
static int wgrad_narrow(const WgradReq& q) {
    WgradNarrowArgs w;
    w.gate = q.gate; w.P = q.P; w.Q = q.Q; w.out = q.out; w.zero = q.zero;
    w.N = q.N; w.H = q.Yc; w.W = q.Xc; w.ldo = q.ldo; w.flip = q.flip;
    w.tiles_y = (q.Yc + 7) / 8; w.tiles_x = (q.Xc + 7) / 8; w.ntiles = wgrad_tiles8(q);
    w.nslabs = q.splits; w.pad0 = 0;                       // the caller allocated `splits` zeroed slabs of apad x ldo
    w.slab_stride = (int64_t)q.apad * q.ldo;
    return wgrad_narrow_launch(w, wgrad_narrow_blocks(q.N, q.Yc, q.Xc), q.st);
}

int fmri_wgrad_if(const int* gate, const void* P, const void* Q, float* out, const void* zero16, int N, int Yc, int Xc,
                  int A, int Hq, int Wq, int Bc, int k, int stride, int pad, int flip, int apad, int ba_tile, int ldo,
                  int splits, int atomic, void* stream) {
    const WgradReq q = {gate, (const half_t*)P, (const half_t*)Q, (const half_t*)zero16, out, N, Yc, Xc, A, Hq, Wq, Bc, k,
                        stride, pad, flip, apad, ba_tile, ldo, splits, atomic, S(stream)};
    const int e = wgrad_check(q);
    if (e != FMRI_OK) return e;
    // the slab modes belong to one kernel each: a geometry that kernel does not fit is refused, not sent to another one
    if ((atomic == FMRI_WGRAD_ATOMIC || atomic == FMRI_WGRAD_PLANE_SLABS) && wgrad_win_fits(q)) return wgrad_win(q);
    if (atomic == FMRI_WGRAD_NARROW_SLABS) return wgrad_narrow_fits(q) ? wgrad_narrow(q) : FMRI_E_UNSUPPORTED;
    if (atomic == FMRI_WGRAD_PLANE_SLABS) return FMRI_E_UNSUPPORTED;
    return wgrad_generic(q);
}

int fmri_wgrad_route(int N, int Yc, int Xc, int A, int Hq, int Wq, int Bc, int k, int stride, int pad, int flip, int apad,
                     int ba_tile, int ldo, int win_blocks, int slab_limit, int deterministic, fmri_wgrad_plan* plan) {
    if (!plan) return FMRI_E_BADARG;
    memset(plan, 0, sizeof(*plan));
    // as in fmri_igemm_route: the pointers are non-NULL dummies that are never dereferenced, the launcher stops at
    // route_probe()
    const half_t* const dummy = (const half_t*)(uintptr_t)64;
    WgradReq q = {nullptr, dummy, dummy, dummy, (float*)(uintptr_t)64, N, Yc, Xc, A, Hq, Wq, Bc, k, stride, pad, flip, apad,
                  ba_tile, ldo, 1, FMRI_WGRAD_STORE, nullptr};
    const int e = wgrad_check(q);
    if (e != FMRI_OK) return e;
    fmri_wgrad_plan& p = *plan;
    if (wgrad_win_fits(q)) {
        // blocks = 32-channel column blocks x 128-row blocks x 4 parity planes x K pieces over the 8 x 8 pixel tiles:
        // the budget per (row block, column block) group over the 4 planes; few pieces: one slab each, else atomics
        const int groups = (Bc / 32) * (apad / 128), ntiles = wgrad_tiles8(q);
        q.splits = win_blocks / groups < 4 ? 4 : win_blocks / groups;
        int tps[4];
        const int smax = wgrad_plane_pieces(N, Yc, Xc, k, pad, q.splits, tps);
        for (int pl = 0; pl < 4; ++pl) p.pieces[pl] = (ntiles + tps[pl] - 1) / tps[pl];
        const bool slabs = smax <= slab_limit || deterministic;
        q.atomic = slabs ? FMRI_WGRAD_PLANE_SLABS : FMRI_WGRAD_ATOMIC;
        p.slabs = p.stored = slabs ? smax : 0;
        p.zeroed = !slabs;
    } else if (wgrad_narrow_fits(q) && wgrad_tiles8(q) >= 32768) {
        // the kernel needs >= ~16 tiles per wave to amortise its block reduction: measured 1.9x on the 3B-image
        // discriminator layer, a loss on the B-image decoder layer.  Blocks add into slab (block index % 4), a quarter
        // of the same-address atomics; deterministic: one slab per block, every element added once, onto zero
        q.atomic = FMRI_WGRAD_NARROW_SLABS;
        q.splits = deterministic ? wgrad_narrow_blocks(N, Yc, Xc) : 4;
        p.slabs = p.stored = q.splits;
        p.zeroed = p.colsum = 1;
    } else {
        // generic kernel: K splits while the output tiles alone do not fill the GPU; atomics, or one slab per split
        const int tiles = (ldo / 128) * (apad / ba_tile), steps = (int)(((int64_t)N * Yc * Xc + 63) / 64);
        if (tiles < 512 && steps >= 16) {
            const int by_steps = steps / 8, by_tiles = (1024 + tiles - 1) / tiles;
            q.splits = by_steps < by_tiles ? by_steps : by_tiles;      // (steps >= 16: at least 2)
        }
        if (q.splits > 1) {
            q.atomic = deterministic ? FMRI_WGRAD_KSPLIT_SLABS : FMRI_WGRAD_ATOMIC;
            p.zeroed = 1;
            if (deterministic) { p.slabs = q.splits; wgrad_ksplit_steps(q, q.splits, &p.stored); }
        }
    }
    p.atomic = q.atomic;
    p.splits = q.splits;
    t_probe_name[0] = 0;
    t_probe_on = true;
    const int r = fmri_wgrad_if(q.gate, q.P, q.Q, q.out, q.zero, N, Yc, Xc, A, Hq, Wq, Bc, k, stride, pad, flip, apad,
                                ba_tile, ldo, q.splits, q.atomic, nullptr);
    t_probe_on = false;
    if (r != FMRI_OK) return r;
    snprintf(p.kernel, sizeof(p.kernel), "%s", t_probe_name);
    return FMRI_OK;
}

int fmri_nchw_to_nhwc(const float* src, void* dst, int N, int C, int HW, int Cp, void* stream) {
    if (!src || !dst || (Cp & 7) || C > Cp) return FMRI_E_BADARG;
    return nchw_to_nhwc_launch(src, (half_t*)dst, N, C, HW, Cp, S(stream));
}
int fmri_nhwc_to_nchw(const void* src, float* dst, int N, int C, int HW, int Cp, float scale, void* stream) {
    if (!src || !dst || C > Cp) return FMRI_E_BADARG;
    return nhwc_to_nchw_launch((const half_t*)src, dst, N, C, HW, Cp, scale, S(stream));
}
int fmri_rows_f32_to_f16(const float* src, void* dst, int M, int C, int Cp, float scale, void* stream) {
    if (!src || !dst || C > Cp) return FMRI_E_BADARG;
    return rows_f32_to_f16_launch(src, (half_t*)dst, M, C, Cp, scale, S(stream));
}
int fmri_rows_f16_to_f32(const void* src, float* dst, int M, int C, int Cp, float scale, void* stream) {
    if (!src || !dst || C > Cp) return FMRI_E_BADARG;
    return rows_f16_to_f32_launch((const half_t*)src, dst, M, C, Cp, scale, S(stream));
}
int fmri_reduce_slabs(const float* slabs, int nslabs, int64_t slab_stride, int M, int C, int ld, const float* bias,
                      int act, float* out32, int ld32, void* out16, int ld16, void* stream) {
    if (!slabs || nslabs < 1 || C > ld) return FMRI_E_BADARG;
    return reduce_slabs_launch(slabs, nslabs, slab_stride, M, C, ld, bias, act, out32, ld32, (half_t*)out16, ld16,
                               S(stream));
}
int fmri_permute_chw(const float* src, float* dst, int C, int HW, int to_engine, float scale, int accumulate,
                     void* stream) {
    if (!src || !dst) return FMRI_E_BADARG;
    return permute_chw_launch(src, dst, C, HW, to_engine, scale, accumulate, S(stream));
}

int64_t fmri_bn_ws_floats(int M, int C) { return (M < 1 || C < 8) ? 0 : bn_ws_floats(M, C); }

int fmri_bn_stats(const void* x, int M, int C, float* sums2C, float* ws, int64_t ws_floats, void* stream) {
    if (!x || !sums2C || (C & 7) || M < 1) return FMRI_E_BADARG;
    return bn_stats_launch((const half_t*)x, M, C, sums2C, ws, ws_floats, S(stream));
}
// the finalize arguments of an entry point (in_scale: null = rows stored at true scale)
static BnFinalize bn_fin(const float* gamma, const float* beta, float eps, float momentum, int updates,
                         float* running_mean, float* running_var, float* mean, float* rstd, float* scale, float* shift,
                         int64_t* num_batches_tracked, const float* in_scale = nullptr) {
    return {gamma, beta, eps, momentum, updates, running_mean, running_var, mean, rstd, scale, shift,
            (long long*)num_batches_tracked, in_scale};
}
static bool bn_fin_ok(const BnFinalize& f) { return f.gamma && f.beta && f.mean && f.rstd && f.scale && f.shift; }

int fmri_bn_finalize(const float* sums2C, int C, float count, const float* gamma, const float* beta, float eps,
                     float momentum, int updates, float* running_mean, float* running_var, float* mean, float* rstd,
                     float* scale, float* shift, int64_t* num_batches_tracked, void* stream) {
    return fmri_bn_finalize_s(sums2C, C, count, gamma, beta, eps, momentum, updates, running_mean, running_var, mean,
                              rstd, scale, shift, num_batches_tracked, nullptr, stream);
}
int fmri_bn_finalize_s(const float* sums2C, int C, float count, const float* gamma, const float* beta, float eps,
                       float momentum, int updates, float* running_mean, float* running_var, float* mean, float* rstd,
                       float* scale, float* shift, int64_t* num_batches_tracked, const float* in_scale, void* stream) {
    const BnFinalize f = bn_fin(gamma, beta, eps, momentum, updates, running_mean, running_var, mean, rstd, scale,
                                shift, num_batches_tracked, in_scale);
    if (!sums2C || !bn_fin_ok(f)) return FMRI_E_BADARG;
    return bn_finalize_launch(sums2C, C, count, f, S(stream));
}
int fmri_bn_stats_finalize(const void* x, int M, int C, float* sums2C, float* ws, int64_t ws_floats, float count,
                           const float* gamma, const float* beta, float eps, float momentum, int updates,
                           float* running_mean, float* running_var, float* mean, float* rstd, float* scale,
                           float* shift, int64_t* num_batches_tracked, void* stream) {
    const BnFinalize f = bn_fin(gamma, beta, eps, momentum, updates, running_mean, running_var, mean, rstd, scale,
                                shift, num_batches_tracked);
    if (!x || !sums2C || (C & 7) || M < 1 || !bn_fin_ok(f)) return FMRI_E_BADARG;
    return bn_stats_finalize_launch((const half_t*)x, M, C, sums2C, ws, ws_floats, count, f, S(stream));
}
int fmri_bn_cols_fwd(const void* x, void* y, int M, int C, float count, const float* gamma, const float* beta, float eps,
                     float momentum, int updates, float* running_mean, float* running_var, float* mean, float* rstd,
                     float* scale, float* shift, float* sums2C, int64_t* num_batches_tracked, int relu, void* stream) {
    return fmri_bn_cols_fwd_s(x, y, M, C, count, gamma, beta, eps, momentum, updates, running_mean, running_var, mean,
                              rstd, scale, shift, sums2C, num_batches_tracked, relu, nullptr, stream);
}
int fmri_bn_cols_fwd_s(const void* x, void* y, int M, int C, float count, const float* gamma, const float* beta, float eps,
                       float momentum, int updates, float* running_mean, float* running_var, float* mean, float* rstd,
                       float* scale, float* shift, float* sums2C, int64_t* num_batches_tracked, int relu,
                       const float* in_scale, void* stream) {
    const BnFinalize f = bn_fin(gamma, beta, eps, momentum, updates, running_mean, running_var, mean, rstd, scale,
                                shift, num_batches_tracked, in_scale);
    if (!x || !y || !sums2C || (C & 7) || C < 8 || M < 1 || !bn_fin_ok(f)) return FMRI_E_BADARG;
    return bn_cols_fwd_launch((const half_t*)x, (half_t*)y, M, C, count, f, sums2C, relu, S(stream));
}
int fmri_bn_cols_bwd(const void* x, const void* dy, void* dx, int M, int C, int nstreams, float count, const float* mean,
                     const float* rstd, const float* gamma, const float* beta, int relu, float* sums, float* dbeta,
                     float* dgamma, float gscale, int param_stream, void* stream) {
    if (!x || !dy || !dx || !sums || (C & 7) || C < 8 || M < 1 || !mean || !rstd || !gamma || !beta || count <= 0.f ||
        param_stream < 0 || param_stream >= nstreams)
        return FMRI_E_BADARG;
    return bn_cols_bwd_launch((const half_t*)x, (const half_t*)dy, (half_t*)dx, M, C, nstreams, count, mean, rstd, gamma,
                              beta, relu, sums, dbeta, dgamma, gscale, param_stream, nullptr, S(stream));
}
int fmri_bn_cols_bwd_cnt(const void* x, const void* dy, void* dx, int M, int C, int nstreams, float count,
                         const float* mean, const float* rstd, const float* gamma, const float* beta, int relu,
                         float* sums, float* dbeta, float* dgamma, float gscale, int param_stream, int* cnt,
                         void* stream) {
    if (!cnt || !x || !dy || !dx || !sums || (C & 7) || C < 8 || M < 1 || !mean || !rstd || !gamma || !beta ||
        count <= 0.f || param_stream < 0 || param_stream >= nstreams)
        return FMRI_E_BADARG;
    return bn_cols_bwd_launch((const half_t*)x, (const half_t*)dy, (half_t*)dx, M, C, nstreams, count, mean, rstd, gamma,
                              beta, relu, sums, dbeta, dgamma, gscale, param_stream, cnt, S(stream));
}
int fmri_bn_fold_finalize(const float* stat_part, int rows, int C, float* scratch, float* sums2C, float count,
                          const float* gamma, const float* beta, float eps, float momentum, int updates,
                          float* running_mean, float* running_var, float* mean, float* rstd, float* scale, float* shift,
                          int64_t* num_batches_tracked, void* stream) {
    const BnFinalize f = bn_fin(gamma, beta, eps, momentum, updates, running_mean, running_var, mean, rstd, scale,
                                shift, num_batches_tracked);
    if (!stat_part || rows < 1 || C < 1 || !scratch || !sums2C || !bn_fin_ok(f)) return FMRI_E_BADARG;
    return bn_fold_finalize_launch(stat_part, rows, C, scratch, sums2C, count, f, S(stream));
}
int fmri_bn_fold(const float* stat_part, int rows, int C, float* scratch, float* sums2C, void* stream) {
    if (!stat_part || rows < 1 || C < 1 || !scratch || !sums2C) return FMRI_E_BADARG;
    return bn_fold_launch(stat_part, rows, 2 * C, scratch, sums2C, S(stream));
}
int fmri_bn_fold_scratch_floats(int C) { return C < 1 ? 0 : FOLD_STAGE_ROWS * 2 * C; }
int fmri_bn_bwd_fold(const float* stat_part, int rows, int rows_cap, int C, int groups, float* scratch, float* sums,
                     float* dbeta, float* dgamma, float gscale, int param_group, void* stream) {
    if (!stat_part || rows < 1 || rows > rows_cap || C < 1 || groups < 1 || groups > 4 || !scratch || !sums)
        return FMRI_E_BADARG;
    return bn_bwd_fold_launch(stat_part, rows, rows_cap, C, groups, scratch, sums, dbeta, dgamma, gscale, param_group,
                              S(stream));
}
int fmri_bn_apply(const void* x, void* y, int M, int C, const float* scale, const float* shift, int relu,
                  void* stream) {
    if (!x || !y || (C & 7)) return FMRI_E_BADARG;
    return bn_apply_launch((const half_t*)x, (half_t*)y, M, C, scale, shift, relu, S(stream));
}
int fmri_bn_bwd_reduce(const void* x, const void* dy, int M, int C, const float* mean, const float* rstd,
                       const float* gamma, const float* beta, int relu, float* sums2C, float* ws,
                       int64_t ws_floats, float* dbeta, float* dgamma, float gscale, void* stream) {
    if (!x || !dy || !sums2C || (C & 7)) return FMRI_E_BADARG;
    return bn_bwd_reduce_launch((const half_t*)x, (const half_t*)dy, M, C, 1, mean, rstd, gamma, beta, relu, sums2C, ws,
                                ws_floats, dbeta, dgamma, gscale, 0, S(stream));
}
int fmri_bn_bwd_reduce2(const void* x, const void* dy2, int M, int C, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, int relu, float* sums4C, float* ws, int64_t ws_floats,
                        float* dbeta, float* dgamma, float gscale, int param_stream, void* stream) {
    if (!x || !dy2 || !sums4C || (C & 7) || M < 1 || (param_stream & ~1)) return FMRI_E_BADARG;
    return bn_bwd_reduce_launch((const half_t*)x, (const half_t*)dy2, M, C, 2, mean, rstd, gamma, beta, relu, sums4C, ws,
                                ws_floats, dbeta, dgamma, gscale, param_stream, S(stream));
}
int fmri_bn_bwd_apply2(const void* x, const void* dy2, void* dx2, int M, int C, float count, const float* mean,
                       const float* rstd, const float* gamma, const float* beta, int relu, const float* sums4C,
                       void* stream) {
    if (!x || !dy2 || !dx2 || !sums4C || (C & 7) || M < 1) return FMRI_E_BADARG;
    return bn_bwd_apply_launch((const half_t*)x, (const half_t*)dy2, (half_t*)dx2, M, C, 2, count, mean, rstd, gamma, beta,
                               relu, sums4C, nullptr, S(stream));
}
int fmri_bn_bwd_apply(const void* x, const void* dy, void* dx, int M, int C, float count, const float* mean,
                      const float* rstd, const float* gamma, const float* beta, int relu, const float* sums2C,
                      void* stream) {
    if (!x || !dy || !dx || (C & 7)) return FMRI_E_BADARG;
    return bn_bwd_apply_launch((const half_t*)x, (const half_t*)dy, (half_t*)dx, M, C, 1, count, mean, rstd, gamma, beta,
                               relu, sums2C, nullptr, S(stream));
}
int fmri_bn_bwd_apply2_cnt(const void* x, const void* dy2, void* dx2, int M, int C, float count, const float* mean,
                           const float* rstd, const float* gamma, const float* beta, int relu, const float* sums4C,
                           int* cnt, void* stream) {
    if (!cnt || !x || !dy2 || !dx2 || !sums4C || (C & 7) || M < 1) return FMRI_E_BADARG;
    return bn_bwd_apply_launch((const half_t*)x, (const half_t*)dy2, (half_t*)dx2, M, C, 2, count, mean, rstd, gamma, beta,
                               relu, sums4C, cnt, S(stream));
}
int fmri_bn_bwd_apply_cnt(const void* x, const void* dy, void* dx, int M, int C, float count, const float* mean,
                          const float* rstd, const float* gamma, const float* beta, int relu, const float* sums2C,
                          int* cnt, void* stream) {
    if (!cnt || !x || !dy || !dx || (C & 7)) return FMRI_E_BADARG;
    return bn_bwd_apply_launch((const half_t*)x, (const half_t*)dy, (half_t*)dx, M, C, 1, count, mean, rstd, gamma, beta,
                               relu, sums2C, cnt, S(stream));
}
int fmri_act_bwd(const void* y, const void* dy, void* dpre, int M, int C, int act, float* colsum2C, float* ws,
                 int64_t ws_floats, float* dbias, int dbias_n, float gscale, void* stream) {
    if (!y || !dy || !dpre || (C & 7) || (dbias && (!colsum2C || dbias_n < 1 || dbias_n > C))) return FMRI_E_BADARG;
    return act_bwd_launch((const half_t*)y, (const half_t*)dy, (half_t*)dpre, M, C, act, colsum2C, ws, ws_floats, dbias,
                          dbias_n, gscale, S(stream));
}
int fmri_colsum_rows(const void* x16, int M, int C, float* sums2C, float* ws, int64_t ws_floats, float* dbias,
                     int dbias_n, float gscale, void* stream) {
    if (!x16 || !sums2C || !ws || M < 1 || C < 8 || (C & 7) || (dbias && (dbias_n < 1 || dbias_n > C))) return FMRI_E_BADARG;
    return colsum_rows_launch((const half_t*)x16, M, C, sums2C, ws, ws_floats, dbias, dbias_n, gscale, S(stream));
}
int fmri_colsum_acc(const void* src, int is_f16, int M, int C, int64_t ld_row, int64_t ld_col, float scale, float* dst,
                    void* stream) {
    if (!src || !dst || M < 1 || C < 1) return FMRI_E_BADARG;
    return colsum_acc_launch(src, is_f16, M, C, ld_row, ld_col, scale, dst, S(stream));
}

int fmri_latent_fwd(const float* head, const float* eps, int B, int Z, int zp, void* z16, float* kl_rows,
                    float* kl_total, int sample, void* stream) {
    if (!head || !z16 || (sample && !eps) || zp < Z) return FMRI_E_BADARG;
    return latent_fwd_launch(head, eps, B, Z, zp, (half_t*)z16, kl_rows, kl_total, sample, S(stream));
}
int fmri_latent_fwd_ranged(const float* head, const float* eps, int B, int Z, int zp, void* z16, float* kl_rows,
                           float* kl_total, int sample, float* z32, float* zmax, float* zscale, float cap, int phase,
                           void* stream) {
    if (!z32 || !zmax || phase < 1 || phase > 3 || zp < Z || B < 1 || Z < 1) return FMRI_E_BADARG;
    if ((phase & 1) && (!head || (sample && !eps))) return FMRI_E_BADARG;
    if ((phase & 2) && (!z16 || !zscale || !(cap > 0.f))) return FMRI_E_BADARG;
    return latent_ranged_launch(head, eps, B, Z, zp, (half_t*)z16, kl_rows, kl_total, sample, z32, zmax, zscale, cap, phase,
                                S(stream));
}
float fmri_latent_range_scale(float zmax, float cap) { return latent_range_scale_host(zmax, cap); }
int fmri_rows_absmax(const float* x, int64_t n, float* zmax, void* stream) {
    if (!x || !zmax || n < 1) return FMRI_E_BADARG;
    return rows_absmax_launch(x, n, zmax, S(stream));
}
int fmri_latent_bwd(const float* head, const float* eps, const float* dz, int ldz, float dz_unscale, float kl_w,
                    const float* kl_dev, int B, int Z, float out_scale, void* dhead16, float* dhead32, int sample,
                    void* stream) {
    if (!head || (sample && !eps)) return FMRI_E_BADARG;
    return latent_bwd_launch(head, eps, dz, ldz, dz_unscale, kl_w, kl_dev, B, Z, out_scale, (half_t*)dhead16, dhead32,
                             sample, S(stream));
}
int fmri_feat_mse(const void* feat, int B, int F, float* mse_rows, float* mse_total, void* stream) {
    if (!feat || (F & 7)) return FMRI_E_BADARG;
    return feat_mse_launch((const half_t*)feat, B, F, mse_rows, mse_total, S(stream));
}
int fmri_feat_mse_bwd(const void* feat, int B, int F, void* dfeat, float gscale, const float* norm, void* stream) {
    if (!feat || !dfeat || (F & 7)) return FMRI_E_BADARG;
    return feat_mse_bwd_launch((const half_t*)feat, B, F, (half_t*)dfeat, gscale, norm, S(stream));
}
int fmri_feat_mse_wide_chunk(void) { return feat_mse_wide_chunk(); }
int64_t fmri_feat_mse_wide_ws_floats(int B, int F) { return (B < 1 || F < 8) ? 0 : feat_mse_wide_ws_floats(B, F); }
int fmri_feat_mse_wide(const void* feat, int B, int F, float* mse_rows, float* mse_total, float* ws, int64_t ws_floats,
                       void* stream) {
    if (!feat || !ws || B < 1 || F < 8 || (F & 7)) return FMRI_E_BADARG;
    if (ws_floats < feat_mse_wide_ws_floats(B, F)) return FMRI_E_WORKSPACE;
    return feat_mse_wide_launch((const half_t*)feat, B, F, mse_rows, mse_total, ws, S(stream));
}
int fmri_feat_mse_bwd_wide(const void* feat, int B, int F, void* dfeat, float gscale, const float* norm,
                           int write_zero_rows, void* stream) {
    if (!feat || !dfeat || B < 1 || F < 8 || (F & 7)) return FMRI_E_BADARG;
    return feat_mse_bwd_wide_launch((const half_t*)feat, B, F, (half_t*)dfeat, gscale, norm, write_zero_rows ? 1 : 0,
                                    S(stream));
}
int fmri_pixel_sq(const void* x, const void* xt, int64_t npix, int C, int Cp, float* total, void* dxt, float gscale,
                  void* stream) {
    if (!x || !xt) return FMRI_E_BADARG;
    return pixel_sq_launch((const half_t*)x, (const half_t*)xt, npix, C, Cp, total, (half_t*)dxt, gscale, S(stream));
}
int fmri_gan_head(const float* logit, int ldl, int B, float* prob, float* scal, void* stream) {
    if (!logit || !scal) return FMRI_E_BADARG;
    return gan_head_launch(logit, ldl, B, prob, scal, 7, S(stream));
}
int fmri_gan_head_bwd(const float* logit, int ldl, int B, void* dlogit, int ldg, float gscale, const float* norm,
                      void* stream) {
    if (!logit || !dlogit) return FMRI_E_BADARG;
    return gan_head_bwd_launch(logit, ldl, B, (half_t*)dlogit, ldg, gscale, norm, 7, S(stream));
}
int fmri_gan_head_parts(const float* logit, int ldl, int B, float* prob, float* scal, int parts, void* stream) {
    if (!logit || !scal || parts < 0 || parts > 7) return FMRI_E_BADARG;
    return gan_head_launch(logit, ldl, B, prob, scal, parts, S(stream));
}
int fmri_gan_head_bwd_parts(const float* logit, int ldl, int B, void* dlogit, int ldg, float gscale, const float* norm,
                            int parts, void* stream) {
    if (!logit || !dlogit || parts < 0 || parts > 7) return FMRI_E_BADARG;
    return gan_head_bwd_launch(logit, ldl, B, (half_t*)dlogit, ldg, gscale, norm, parts, S(stream));
}
int fmri_wae_logloss(const float* logit, int ldl, int n, int one_minus, float w, float* total, float* prob,
                     void* dlogit, int ldg, float gscale, void* stream) {
    if (!logit) return FMRI_E_BADARG;
    return wae_logloss_launch(logit, ldl, n, one_minus, w, total, prob, (half_t*)dlogit, ldg, gscale, S(stream));
}
int64_t fmri_mmd_imq_ws_bytes(int n, int d) { return mmd_imq_ws_bytes(n, d); }
int fmri_mmd_imq(const float* q, int ldq, const float* p, int ldp, int n, int d, float sigma2, const float* scales,
                 int nscales, float w, float* total, float* dq, int ldd, float gscale, void* ws, int64_t ws_bytes,
                 void* stream) {
    static const float kScales[7] = {0.1f, 0.2f, 0.5f, 1.f, 2.f, 5.f, 10.f};
    if (!scales) { scales = kScales; nscales = 7; }
    if (!q || !p || !ws || n < 2 || d < 1 || ldq < d || ldp < d || !(sigma2 > 0.f) || nscales < 1 || nscales > 8)
        return FMRI_E_BADARG;
    for (int s = 0; s < nscales; ++s)
        if (!(scales[s] > 0.f)) return FMRI_E_BADARG;
    if (dq && ldd < d) return FMRI_E_BADARG;
    if (d % 64 || d > 1024) return FMRI_E_UNSUPPORTED;
    // float4 loads of the q / p rows
    if (((uintptr_t)q | (uintptr_t)p) % 16 || ldq % 4 || ldp % 4) return FMRI_E_BADARG;
    return mmd_imq_launch(q, ldq, p, ldp, n, d, sigma2, scales, nscales, w, total, dq, ldd, gscale, ws, ws_bytes,
                          S(stream));
}
int64_t fmri_latent_nce_ws_bytes(int n, int d) { return latent_nce_ws_bytes(n, d); }
int fmri_latent_nce(const float* q, int ldq, const float* t, int ldt, int n, int d, float tau, int symmetric, float w,
                    float* total, float* top1, float* dq, int ldd, float gscale, void* ws, int64_t ws_bytes,
                    void* stream) {
    if (!q || !t || !ws || n < 2 || d < 1 || ldq < d || ldt < d || !(tau >= 0.01f && tau <= 1.f))
        return FMRI_E_BADARG;
    if (dq && ldd < d) return FMRI_E_BADARG;
    if (latent_nce_ws_bytes(n, d) < 0) return FMRI_E_UNSUPPORTED;
    // float4 loads of the q / t rows
    if (((uintptr_t)q | (uintptr_t)t) % 16 || ldq % 4 || ldt % 4) return FMRI_E_BADARG;
    return latent_nce_launch(q, ldq, t, ldt, n, d, tau, symmetric, w, total, top1, dq, ldd, gscale, ws, ws_bytes,
                             S(stream));
}
int fmri_mlp_fwd(const void* z16, int M, int Zp, int H, const void* const* w5, const int* kp5, const float* const* bias5,
                 void* const* hs4, float* logit, void* stream) {
    if (!z16 || !w5 || !kp5 || !bias5 || !hs4 || !logit || M < 1) return FMRI_E_BADARG;
    MlpFwdArgs a;
    memset(&a, 0, sizeof(a));
    a.z = (const half_t*)z16; a.M = M; a.Zp = Zp; a.H = H; a.logit = logit;
    for (int i = 0; i < 5; ++i) {
        if (!w5[i] || kp5[i] < (i == 0 ? Zp : H)) return FMRI_E_BADARG;
        a.w[i] = (const half_t*)w5[i]; a.kp[i] = kp5[i]; a.bias[i] = bias5[i];
    }
    for (int i = 0; i < 4; ++i) {
        if (!hs4[i]) return FMRI_E_BADARG;
        a.hs[i] = (half_t*)hs4[i];
    }
    return mlp_fwd_launch(a, S(stream));
}
int fmri_mlp_bwd(const void* dlogit16, int ldl, int M, int Zp, int Z, int H, const void* const* hs4, const void* w4row,
                 const void* const* wd4, const int* kpd4, void* const* delta4, float* const* dbias5, float* dz32,
                 float inv_scale, void* stream) {
    if (!dlogit16 || !hs4 || !w4row || !wd4 || !kpd4 || !delta4 || M < 1 || ldl < 1 || Z > Zp) return FMRI_E_BADARG;
    MlpBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.dlogit = (const half_t*)dlogit16; a.ldl = ldl; a.M = M; a.Zp = Zp; a.H = H; a.Z = Z;
    a.w4 = (const half_t*)w4row; a.dz = dz32; a.inv_scale = inv_scale;
    for (int i = 0; i < 4; ++i) {
        if (!hs4[i] || !delta4[i]) return FMRI_E_BADARG;
        if ((i > 0 || dz32) && (!wd4[i] || kpd4[i] < H)) return FMRI_E_BADARG;
        a.hs[i] = (const half_t*)hs4[i]; a.delta[i] = (half_t*)delta4[i];
        a.wd[i] = (const half_t*)wd4[i]; a.kpd[i] = kpd4[i];
    }
    for (int i = 0; i < 5; ++i) a.dbias[i] = dbias5 ? dbias5[i] : nullptr;
    return mlp_bwd_launch(a, S(stream));
}
int fmri_compose_gate(float* scal, int* flags, float batch, float nfeat, float lambda_mse, float equilibrium,
                      float margin, int gate_on, int force_dis, int force_dec, void* stream) {
    if (!scal || !flags) return FMRI_E_BADARG;
    return compose_gate_launch(scal, flags, batch, nfeat, 0.f, lambda_mse, equilibrium, margin, 1.f, nullptr, 0, gate_on,
                               force_dis, force_dec, S(stream));
}
int fmri_compose_gate_dev(float* scal, int* flags, float batch, float nfeat, float npix, const float* hp4_dev, int mode,
                          int gate_on, int force_dis, int force_dec, void* stream) {
    if (!scal || !flags || !hp4_dev || mode < 0 || mode > 3) return FMRI_E_BADARG;
    return compose_gate_launch(scal, flags, batch, nfeat, npix, 0.f, 0.f, 0.f, 0.f, hp4_dev, mode, gate_on, force_dis,
                               force_dec, S(stream));
}
int fmri_counter_inc(int* counter_dev, void* stream) {
    if (!counter_dev) return FMRI_E_BADARG;
    return counter_inc_launch(counter_dev, S(stream));
}
int fmri_rng_normal(const int64_t* state, float* out, int rows, int cols, int ld, int64_t row0, int sid, float scale,
                    void* stream) {
    if (!state || ((uintptr_t)state & 7) || !out || ((uintptr_t)out & 3) || rows < 1 || cols < 1 || ld < cols ||
        row0 < 0 || sid < 0)
        return FMRI_E_BADARG;
    return rng_normal_launch(state, out, rows, cols, ld, row0, sid, scale, S(stream));
}
int fmri_rng_u32(const int64_t* state, int32_t* out, int64_t n, int sid, int lo, int hi, void* stream) {
    if (!state || ((uintptr_t)state & 7) || !out || ((uintptr_t)out & 3) || n < 1 || sid < 0 || hi < lo)
        return FMRI_E_BADARG;
    return rng_u32_launch(state, out, n, 0, sid, lo, hi, S(stream));
}
int fmri_rng_u32_at(const int64_t* state, int32_t* out, int64_t n, int64_t start, int sid, int lo, int hi,
                    void* stream) {
    if (!state || ((uintptr_t)state & 7) || !out || ((uintptr_t)out & 3) || n < 1 || start < 0 || sid < 0 || hi < lo)
        return FMRI_E_BADARG;
    return rng_u32_launch(state, out, n, start, sid, lo, hi, S(stream));
}
int fmri_rng_advance(int64_t* state, int64_t nblocks, void* stream) {
    if (!state || ((uintptr_t)state & 7) || nblocks < 0) return FMRI_E_BADARG;
    return rng_advance_launch(state, nblocks, S(stream));
}
int fmri_sampler_indices(const int64_t* state, int N, int B, int64_t row0, int32_t* idx_out, void* stream) {
    if (!state || ((uintptr_t)state & 7) || !idx_out || ((uintptr_t)idx_out & 3) || N < 1 || B < 1 || row0 < 0)
        return FMRI_E_BADARG;
    if (row0 + B > N) return FMRI_E_UNSUPPORTED;
    return sampler_indices_launch(state, N, B, row0, idx_out, S(stream));
}
int fmri_sampler_advance(int64_t* state, int N, int B_global, void* stream) {
    if (!state || ((uintptr_t)state & 7) || N < 1 || B_global < 1) return FMRI_E_BADARG;
    if (N < B_global) return FMRI_E_UNSUPPORTED;
    return sampler_advance_launch(state, N, B_global, S(stream));
}
int fmri_diffaug_params(const int64_t* state, float* table, int rows, int64_t row0, int sid, int H, int sh, int cut,
                        int policy_mask, void* stream) {
    if (!state || ((uintptr_t)state & 7) || !table || ((uintptr_t)table & 15) || rows < 1 || row0 < 0 ||
        row0 > (1ll << 40) || sid < 0 || H < 1 || sh < 0 || sh > H || cut < 0 || cut > H || (policy_mask & ~7))
        return FMRI_E_BADARG;
    if (H > 128) return FMRI_E_UNSUPPORTED;
    return diffaug_params_launch(state, table, rows, row0, sid, H, sh, cut, policy_mask, S(stream));
}
// the checks fmri_diffaug_fwd / fmri_diffaug_bwd share, for one (input, output) pair of [N][H][W][8] fp16 tensors
static int diffaug_check(const void* src, const void* dst, int N, int H, int W, const float* table, int B, int img0) {
    if (!src || ((uintptr_t)src & 15) || !dst || ((uintptr_t)dst & 15) || !table || ((uintptr_t)table & 15) || N < 1 ||
        H < 1 || W < 1 || B < 1 || img0 < 0 || (int64_t)img0 + N > 3ll * B)
        return FMRI_E_BADARG;
    if (H != W || H > 128) return FMRI_E_UNSUPPORTED;
    const uintptr_t bytes = (uintptr_t)N * H * W * 16, s = (uintptr_t)src, d = (uintptr_t)dst;
    if (s < d + bytes && d < s + bytes) return FMRI_E_BADARG;
    return FMRI_OK;
}
int fmri_diffaug_fwd(const void* src16, void* dst16, int N, int H, int W, const float* table, int B, int img0,
                     void* stream) {
    const int rc = diffaug_check(src16, dst16, N, H, W, table, B, img0);
    if (rc != FMRI_OK) return rc;
    return diffaug_fwd_launch((const half_t*)src16, (half_t*)dst16, N, H, table, B, img0, S(stream));
}
int fmri_diffaug_bwd(const void* g_a, void* dst_a, const void* g_b, void* dst_b, int N, int H, int W, const float* table,
                     int B, int img0, void* stream) {
    int rc = diffaug_check(g_a, dst_a, N, H, W, table, B, img0);
    if (rc != FMRI_OK) return rc;
    if ((g_b == nullptr) != (dst_b == nullptr)) return FMRI_E_BADARG;
    if (g_b) {
        rc = diffaug_check(g_b, dst_b, N, H, W, table, B, img0);
        if (rc == FMRI_OK) rc = diffaug_check(g_a, dst_b, N, H, W, table, B, img0);      // no output over an input
        if (rc == FMRI_OK) rc = diffaug_check(g_b, dst_a, N, H, W, table, B, img0);
        if (rc == FMRI_OK) rc = diffaug_check(dst_a, dst_b, N, H, W, table, B, img0);
        if (rc != FMRI_OK) return rc;
    }
    return diffaug_bwd_launch((const half_t*)g_a, (half_t*)dst_a, (const half_t*)g_b, (half_t*)dst_b, N, H, table, B,
                              img0, S(stream));
}
int fmri_voxaug_params(const int64_t* state, float* table, int rows, int64_t row0, int sid_row, int V, float gain,
                       float sigma, float p, int rescale, int span_len, float prob, void* stream) {
    if (!state || ((uintptr_t)state & 7) || !table || ((uintptr_t)table & 15) || rows < 1 || row0 < 0 ||
        row0 > (1ll << 40) || sid_row < 0 || V < 1 || V >= (1 << 24) || span_len < 0 || span_len > V || !(gain >= 0.f) ||
        !(sigma >= 0.f) || !(p >= 0.f && p < 1.f) || !(prob >= 0.f && prob <= 1.f))
        return FMRI_E_BADARG;
    return voxaug_params_launch(state, table, rows, row0, sid_row, V, gain, sigma, p, rescale ? 1 : 0, span_len, prob,
                                S(stream));
}
int fmri_voxaug_apply(const float* src32, int V, int B, const float* table, const int64_t* state, int64_t row0,
                      int sid_noise, int sid_drop, void* dst16, float* dst32, void* stream) {
    if (!src32 || ((uintptr_t)src32 & 3) || !table || ((uintptr_t)table & 15) || !state || ((uintptr_t)state & 7) ||
        !dst16 || ((uintptr_t)dst16 & 15) || ((uintptr_t)dst32 & 3) || V < 1 || V >= (1 << 24) || B < 1 || row0 < 0 ||
        row0 > (1ll << 40) || sid_noise < 0 || sid_drop < 0 || sid_noise == sid_drop)
        return FMRI_E_BADARG;
    if ((int64_t)B * V > INT32_MAX) return FMRI_E_UNSUPPORTED;
    const uintptr_t bytes = (uintptr_t)B * V * 4, s = (uintptr_t)src32, d = (uintptr_t)dst32;
    if (dst32 && s < d + bytes && d < s + bytes) return FMRI_E_BADARG;               // no fp32 result over its input
    return voxaug_apply_launch(src32, V, B, table, state, row0, sid_noise, sid_drop, (half_t*)dst16, dst32, S(stream));
}
int fmri_schedule_seek_host(fmri_schedule* s, int64_t epoch, float* out7) {
    if (!s || s->lr_step < 1 || epoch < 0) return FMRI_E_BADARG;
    return schedule_seek_host(s, epoch, out7);
}
int fmri_epoch_begin(const int64_t* feed_state, fmri_schedule* sched, float* lr_out0, float* lr_out1, float* lr_out2,
                     float* lr_out3, float* hp3_out, int64_t* epoch_out, void* stream) {
    if (!feed_state || ((uintptr_t)feed_state & 7) || ((uintptr_t)sched & 7) || ((uintptr_t)epoch_out & 7) ||
        (!sched && !epoch_out))
        return FMRI_E_BADARG;
    if ((((uintptr_t)lr_out0 | (uintptr_t)lr_out1 | (uintptr_t)lr_out2 | (uintptr_t)lr_out3 | (uintptr_t)hp3_out) & 3))
        return FMRI_E_BADARG;
    return epoch_begin_launch(feed_state, sched, lr_out0, lr_out1, lr_out2, lr_out3, hp3_out, epoch_out, S(stream));
}
int fmri_trainlog_append(const void* const* src_dev, const int32_t* kind_dev, int K, float* ring, int64_t capacity,
                         int64_t* counter, void* stream) {
    if (!src_dev || ((uintptr_t)src_dev & 7) || !kind_dev || ((uintptr_t)kind_dev & 3) || K < 1 || K > 64 || !ring ||
        ((uintptr_t)ring & 3) || capacity < 1 || !counter || ((uintptr_t)counter & 7))
        return FMRI_E_BADARG;
    return trainlog_append_launch(src_dev, kind_dev, K, ring, capacity, counter, S(stream));
}
int64_t fmri_state_layout(const int64_t* bytes, int nseg, int64_t* offsets_out) {
    if (nseg < 0 || (nseg > 0 && !bytes)) return FMRI_E_BADARG;
    return state_layout(bytes, nseg, offsets_out);
}
int fmri_state_nontemporal(int on) { return state_nontemporal(on); }
int fmri_state_copy(const fmri_state_seg* segs_host, const fmri_state_seg* segs_dev, int nseg, void* ring,
                    int64_t ring_bytes, int64_t slot_bytes, int dir, const int64_t* feed_state, int every, int capacity,
                    uint64_t fingerprint, const int64_t* log_counter, void* stream) {
    if (nseg < 0 || (nseg > 0 && (!segs_host || !segs_dev || ((uintptr_t)segs_dev & 7))) || !ring ||
        ((uintptr_t)ring & 15) || slot_bytes < FMRI_STATE_HEADER || (slot_bytes & 15) || capacity < 0 || every < 0 ||
        (dir != 0 && dir != 1) || ((uintptr_t)feed_state & 7) || ((uintptr_t)log_counter & 7))
        return FMRI_E_BADARG;
    if (every > 0 && (!feed_state || capacity < 1)) return FMRI_E_BADARG;
    if (dir == 1 && (feed_state || every)) return FMRI_E_BADARG;
    if (slot_bytes > ring_bytes / ((int64_t)capacity + 1)) return FMRI_E_BADARG;
    const int64_t chunks = state_table_chunks(segs_host, nseg, slot_bytes);
    if (chunks < 0) return FMRI_E_BADARG;
    return state_copy_launch(segs_dev, nseg, chunks, ring, slot_bytes, dir, feed_state, every, capacity, fingerprint,
                             log_counter, S(stream));
}
float fmri_ema_decay_at(int32_t t, int32_t start, float decay, int32_t warmup) {
    return ema_decay_at(t, start, decay, warmup);
}
static int ema_call(const fmri_ema_seg* segs_host, const fmri_ema_seg* segs_dev, int nseg, const void* state_dev, int op,
                    void* stream) {
    if (nseg < 0 || (nseg > 0 && (!segs_host || !segs_dev || ((uintptr_t)segs_dev & 7)))) return FMRI_E_BADARG;
    if (op == 0 && (!state_dev || ((uintptr_t)state_dev & 3))) return FMRI_E_BADARG;
    const int64_t chunks = ema_table_chunks(segs_host, nseg);
    if (chunks < 0) return FMRI_E_BADARG;
    return ema_launch(segs_dev, nseg, chunks, state_dev, op, S(stream));
}
int fmri_ema_update(const fmri_ema_seg* segs_host, const fmri_ema_seg* segs_dev, int nseg,
                    const fmri_ema_state* state_dev, void* stream) {
    return ema_call(segs_host, segs_dev, nseg, state_dev, 0, stream);
}
int fmri_ema_swap(const fmri_ema_seg* segs_host, const fmri_ema_seg* segs_dev, int nseg, void* stream) {
    return ema_call(segs_host, segs_dev, nseg, nullptr, 1, stream);
}
int fmri_axpby_f16(const void* x, const void* y, void* out, int64_t n, float a, float b, const float* a_dev,
                   void* stream) {
    if (!x || !out || (n & 7)) return FMRI_E_BADARG;
    return axpby_f16_launch((const half_t*)x, (const half_t*)y, (half_t*)out, n, a, b, a_dev, nullptr, S(stream));
}
int fmri_axpby2_f16(const void* x, const void* y, void* out, int64_t n, float a, float b, const float* a_dev,
                    const float* b_dev, void* stream) {
    if (!x || !out || (n & 7)) return FMRI_E_BADARG;
    return axpby_f16_launch((const half_t*)x, (const half_t*)y, (half_t*)out, n, a, b, a_dev, b_dev, S(stream));
}
int fmri_sumsq(const float* x, int64_t n, float* acc, void* stream) {
    if (!x || !acc) return FMRI_E_BADARG;
    return sumsq_launch(x, n, acc, S(stream));
}
int fmri_renorm(const float* x, void* out16, int64_t n, float scale, const float* sumsq, float count,
                const float* factor_in, float* factor_out, void* stream) {
    if (!x || !out16 || !sumsq || count <= 0.f) return FMRI_E_BADARG;
    return renorm_launch(x, (half_t*)out16, n, scale, sumsq, count, factor_in, factor_out, S(stream));
}
int fmri_sumsq_f64(const float* x, int64_t n, double* acc, int zero_first, void* stream) {
    if (!x || !acc || ((uintptr_t)acc & 7)) return FMRI_E_BADARG;
    return sumsq64_launch(x, n, acc, zero_first, S(stream));
}
int fmri_renorm_f64(const float* x, void* out16, int64_t n, float scale, const double* sumsq, float count,
                    const float* factor_in, float* factor_out, void* stream) {
    if (!x || !out16 || !sumsq || ((uintptr_t)sumsq & 7) || count <= 0.f) return FMRI_E_BADARG;
    return renorm64_launch(x, (half_t*)out16, n, scale, sumsq, count, factor_in, factor_out, S(stream));
}
int fmri_rmsprop(float* p, const float* g, float* sq, int64_t n, float lr, float alpha, float eps, float gscale,
                 const float* gdev, float clamp, const int* flag, void* stream) {
    if (!p || !g || !sq) return FMRI_E_BADARG;
    return rmsprop_launch(p, g, sq, n, lr, alpha, eps, gscale, gdev, clamp, flag, nullptr, S(stream));
}
int fmri_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps,
              float bc1, float bc2_sqrt, float gscale, const float* gdev, float clamp, const int* flag,
              void* stream) {
    if (!p || !g || !m || !v) return FMRI_E_BADARG;
    return adam_launch(p, g, m, v, n, lr, b1, b2, eps, bc1, bc2_sqrt, gscale, gdev, clamp, flag, nullptr, nullptr,
                       S(stream));
}
int fmri_rmsprop_dev(float* p, const float* g, float* sq, int64_t n, const float* lr_dev, float alpha, float eps,
                     float gscale, const float* gdev, float clamp, const int* flag, void* stream) {
    if (!p || !g || !sq || !lr_dev) return FMRI_E_BADARG;
    return rmsprop_launch(p, g, sq, n, 0.f, alpha, eps, gscale, gdev, clamp, flag, lr_dev, S(stream));
}
int fmri_adam_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev, float b1, float b2,
                  float eps, const int* t_dev, float gscale, const float* gdev, float clamp, const int* flag,
                  void* stream) {
    if (!p || !g || !m || !v || !lr_dev || !t_dev) return FMRI_E_BADARG;
    return adam_launch(p, g, m, v, n, 0.f, b1, b2, eps, 1.f, 1.f, gscale, gdev, clamp, flag, lr_dev, t_dev, S(stream));
}

}  // extern "C"
