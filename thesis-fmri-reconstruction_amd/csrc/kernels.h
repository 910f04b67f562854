// Internal launcher declarations shared between the kernel translation units and api.hip.
#pragma once
#include "common.h"

namespace fmri {

struct PackArgs {
    const float* src;
    half_t* dst;
    int64_t sa, sta, sb, stb;
    int32_t A, TA, B, Bp;          // Bp = B padded to a multiple of 8
    int32_t KW, py, px, step, TH, TW;
    int32_t rows_pad, kpad;        // destination matrix [rows_pad][kpad]
};

struct PackEntry {      // one row of the device-resident table of fmri_pack_weight_batch
    PackArgs p;
    int32_t run;
    int32_t tile_begin;
};

struct UnpackArgs {
    const float* src;      // packed [rows][ld]
    float* dst;            // reference layout
    int64_t sa, sta, sb, stb;
    int32_t A, TA, B, Bp;
    int32_t KW, py, px, step, TH, TW;
    int32_t ld;
    float scale;
    int32_t accumulate;
    int32_t nslabs;        // src holds nslabs partial matrices, slab_stride elements apart; they are summed
    int64_t slab_stride;
};

// One row of the device-resident table of fmri_apply_batch (round 4): everything that happens to ONE parameter tensor
// between its weight-gradient GEMM and the next forward pass -- slab sum, scaling, the map from the GEMM layout to the
// reference layout, the optimizer update, the fp16 GEMM copy in the gradient's own orientation -- in one pass.
struct ApplyEntry {
    const float* gsrc;     // kinds 0 / 1: packed fp32 gradient [nslabs][rows][ld] (a weight-gradient GEMM's output)
    float* w;              // master parameters, reference layout: tensor base (kinds 0 / 1) or segment base (kind 2)
    float* sq;             // RMSprop state at the same offsets
    float* grad;           // reference-layout gradient: kind 2 reads it (mode 1) / clears it (mode 2); kinds 0 / 1 write it in mode 0
    half_t* pk;            // fp16 GEMM copy [rows_pad][kpad] in the orientation of gsrc, or null
    int64_t sa, sta, sb;   // reference-layout strides of a, ta, b (taps are contiguous)
    int64_t slab_stride;
    int64_t n;             // kind 2: elements of the segment
    int32_t A, TA, B, Bp;
    int32_t run;           // taps (kind 0)
    int32_t ld, kpad, nslabs;
    int32_t clear;         // write zeros back over gsrc (buffers a weight-gradient kernel ADDS into)
    int32_t kind;          // 0 tap-transposing tile, 1 row-contiguous, 2 flat segment of the parameter buffer
    int32_t bt;            // kind 0: b per tile (32 or 64)
    int32_t tile_begin;
    float scale;
    int32_t pad_;
};
struct ApplyOpt {
    const float* lr_dev; const float* gdev; const int* flag;
    float alpha, eps, gscale, clamp;
    int32_t gated;         // the weight gradients were launched under the same flag (fmri_wgrad_if): when it is 0 they
                           // added nothing, so there is nothing to clear either
    int32_t mode;          // 0: gradients only (reference layout, first-writer stores), 1: RMSprop update + fp16 copy,
                           // 2: clear the flat segments' gradients, 3: as 1 with the gradient read from the reference
                           //    layout (`grad`, e.g. after an all-reduce) instead of gsrc
};
constexpr int APPLY_CHUNK = 1024;       // elements per block of kinds 1 / 2
int apply_entry_tiles(ApplyEntry& e, int TH, int TW, int KW, int py, int px, int step, int64_t stb);
int apply_batch_launch(const ApplyEntry* tab, int n, int total_tiles, const ApplyOpt& o, hipStream_t st);

// Numerics monitor (fmri_stat / fmri_stat_seg of include/fmri_hip.h, same layout)
struct StatRec {
    double sumsq;
    float max, min, max_abs;
    int32_t nonfinite, clamped, written;
};
struct StatSeg {
    const float* x;
    int64_t rows, cols, ld;
    const float* div;
    const int* gate;
    StatRec* out;
    float scale, clamp;
};
constexpr int STAT_MAX_SEGS = 8, STAT_BLOCKS = 256;
struct StatSegs {
    StatSeg s[STAT_MAX_SEGS];
    int32_t nblk[STAT_MAX_SEGS];   // partial records (blocks) of each segment
};
// `part` gets 2 * total_tiles records (gradient, weights) per block
int apply_batch_stats_launch(const ApplyEntry* tab, int n, int total_tiles, const ApplyOpt& o, StatRec* part,
                             hipStream_t st);
int stat_fold_launch(const StatRec* part, int nrec, const int* flag, StatRec* out, hipStream_t st);
int tensor_stats_launch(const StatSegs& segs, int nseg, StatRec* ws, hipStream_t st);

// per-thread accumulator of a StatRec (finite elements: double sum of squares, max, min, max |v|; the rest counted)
struct StatAcc {
    double ss;
    float mx, mn, amax;
    int nf, cl;
};
__device__ __forceinline__ void stat_init(StatAcc& a) {
    a.ss = 0.0; a.mx = -__builtin_inff(); a.mn = __builtin_inff(); a.amax = 0.f; a.nf = 0; a.cl = 0;
}
__device__ __forceinline__ void stat_add(StatAcc& a, float v) {
    if (__builtin_isfinite(v)) {
        a.ss += (double)v * (double)v;
        a.mx = fmaxf(a.mx, v); a.mn = fminf(a.mn, v); a.amax = fmaxf(a.amax, fabsf(v));
    } else {
        a.nf += 1;
    }
}
// (what the optimizers' clamp does to v: fminf(fmaxf(v, -c), c) -- a NaN becomes -c and is counted as changed)
__device__ __forceinline__ void stat_add_clamped(StatAcc& a, float v, float clamp) {
    stat_add(a, v);
    if (clamp > 0.f) a.cl += fminf(fmaxf(v, -clamp), clamp) != v ? 1 : 0;
}
__device__ __forceinline__ void stat_merge(StatAcc& a, const StatAcc& b) {
    a.ss += b.ss; a.mx = fmaxf(a.mx, b.mx); a.mn = fminf(a.mn, b.mn); a.amax = fmaxf(a.amax, b.amax);
    a.nf += b.nf; a.cl += b.cl;
}
__device__ __forceinline__ void stat_merge_rec(StatAcc& a, const StatRec& r) {
    a.ss += r.sumsq; a.mx = fmaxf(a.mx, r.max); a.mn = fminf(a.mn, r.min); a.amax = fmaxf(a.amax, r.max_abs);
    a.nf += r.nonfinite; a.cl += r.clamped;
}
__device__ __forceinline__ StatRec stat_rec(const StatAcc& a, int written) {
    StatRec r;
    r.sumsq = a.ss; r.max = a.mx; r.min = a.mn; r.max_abs = a.amax; r.nonfinite = a.nf; r.clamped = a.cl;
    r.written = written;
    return r;
}
// the block's total (fixed order: an xor-shuffle tree per wave, then the waves in index order); valid in thread 0.
// `red` = __shared__ StatAcc[blockDim.x / 64]; starts and ends with a barrier (callable twice in a row)
__device__ __forceinline__ StatAcc stat_block(StatAcc a, StatAcc* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a.ss += __shfl_xor(a.ss, o, 64);
        a.mx = fmaxf(a.mx, __shfl_xor(a.mx, o, 64));
        a.mn = fminf(a.mn, __shfl_xor(a.mn, o, 64));
        a.amax = fmaxf(a.amax, __shfl_xor(a.amax, o, 64));
        a.nf += __shfl_xor(a.nf, o, 64);
        a.cl += __shfl_xor(a.cl, o, 64);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    StatAcc r = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) stat_merge(r, red[w]);
    return r;
}

int igemm_launch(const IgemmArgs& a, int maxM, int bn_tile, int copad, bool out_f32, hipStream_t st);
int igemm_bm(const IgemmArgs& a, int maxM, int bn_tile, int copad, bool out_f32);   // row tile igemm_launch will use
int igemm_tc32_launch(const Tc32Args& a, int nblocks, hipStream_t st);
int igemm_tc5_launch(const Tc5Args& a, int bn_tile, int copad, hipStream_t st);
int igemm_c5_launch(const C5Args& a, int copad, hipStream_t st);
int igemm_c5w_launch(const C5Args& a, int copad, hipStream_t st);
int igemm_tc5w_launch(const Tc5Args& a, int copad, hipStream_t st);
int mlp_fwd_launch(const MlpFwdArgs& a, hipStream_t st);
int mlp_bwd_launch(const MlpBwdArgs& a, hipStream_t st);
int igemm_narrow_launch(const NarrowArgs& a, int ci, int co_tiles, bool flip, hipStream_t st);
int wgrad_launch(const WgradArgs& a, int apad, int ba_tile, hipStream_t st);
int wgrad_win_launch(const WgradWinArgs& a, int apad, hipStream_t st);
int wgrad_narrow_launch(const WgradNarrowArgs& a, int nblocks, hipStream_t st);

int pack_weight_launch(const PackArgs& p, hipStream_t st);
int unpack_grad_launch(const UnpackArgs& p, hipStream_t st);
int pack_tile_count(const PackArgs& p, int* run_out);
int pack_batch_launch(const PackEntry* tab, int n, int total_tiles, hipStream_t st);
struct TransposeEntry {    // one row of the device-resident table of fmri_transpose_f16_batch
    const half_t* src;     // first element of the [R][C] source slice (row stride lds)
    half_t* dst;           // first element of the [C][R] destination slice (row stride ldd)
    int32_t R, C, Rbuf;    // Rbuf >= R rows exist behind src (the rows from R on are zero)
    int32_t width;         // source columns readable from src on (>= C; whole 16-byte items are read)
    int32_t lds, ldd;
    int32_t tile_begin, pad_;
};
int transpose_batch_launch(const TransposeEntry* tab, int n, int total_tiles, hipStream_t st);
int transpose_f16_launch(const half_t* src, half_t* dst, int R, int C, int Rbuf, int lds_, int ldd, hipStream_t st);
int nchw_to_nhwc_launch(const float* s, half_t* d, int N, int C, int HW, int Cp, hipStream_t st);
int nhwc_to_nchw_launch(const half_t* s, float* d, int N, int C, int HW, int Cp, float scale, hipStream_t st);
int rows_f32_to_f16_launch(const float* s, half_t* d, int M, int C, int Cp, float scale, hipStream_t st);
int rows_f16_to_f32_launch(const half_t* s, float* d, int M, int C, int Cp, float scale, hipStream_t st);
int reduce_slabs_launch(const float* slabs, int nslabs, int64_t slab_stride, int M, int C, int ld, const float* bias,
                        int act, float* out32, int ld32, half_t* out16, int ld16, hipStream_t st);
int permute_chw_launch(const float* s, float* d, int C, int HW, int to_engine, float scale, int accumulate,
                       hipStream_t st);

// What a BatchNorm finalize reads and writes besides the batch sums and their count (bn_finalize_channel, norm.hip).
// api.hip fills one per entry point; it travels by value down to the kernels.
struct BnFinalize {
    const float *gamma, *beta;
    float eps, momentum;
    int updates;                            // consecutive running-statistics updates of this call (0: none)
    float *running_mean, *running_var;      // may be null
    float *mean, *rstd, *scale, *shift;     // outputs, C floats each
    long long* nbt;                         // num_batches_tracked, += updates (may be null)
    const float* in_scale;                  // device scalar s of range-scaled rows s * x (null: s = 1)
};
int64_t bn_ws_floats(int M, int C);
int bn_stats_launch(const half_t* x, int M, int C, float* sums, float* ws, int64_t ws_floats, hipStream_t st);
int bn_stats_finalize_launch(const half_t* x, int M, int C, float* sums, float* ws, int64_t ws_floats, float count,
                             const BnFinalize& f, hipStream_t st);
constexpr int FOLD_STAGE_ROWS = 32;     // rows of the intermediate buffer of a two-stage statistics fold
int bn_fold_finalize_launch(const float* part, int rows, int C, float* scratch, float* sums, float count,
                            const BnFinalize& f, hipStream_t st);
int bn_fold_launch(const float* part, int rows, int n, float* scratch, float* sums, hipStream_t st);
int bn_bwd_fold_launch(const float* part, int rows, int rows_cap, int C, int G, float* scratch, float* sums,
                       float* dbeta, float* dgamma, float gscale, int pgroup, hipStream_t st);
int bn_finalize_launch(const float* sums, int C, float count, const BnFinalize& f, hipStream_t st);
int bn_cols_fwd_launch(const half_t* x, half_t* y, int M, int C, float count, const BnFinalize& f, float* sums2C,
                       int relu, hipStream_t st);
int bn_cols_bwd_launch(const half_t* x, const half_t* dy, half_t* dx, int M, int C, int nstreams, float count,
                       const float* mean, const float* rstd, const float* gamma, const float* beta, int relu, float* sums,
                       float* dbeta, float* dgamma, float gscale, int pstream, int* cnt, hipStream_t st);
int bn_apply_launch(const half_t* x, half_t* y, int M, int C, const float* scale, const float* shift, int relu,
                    hipStream_t st);
// backward of nstreams (1 or 2) cotangent streams stacked along the rows of dy / dx; sums [nstreams][2][C]
int bn_bwd_reduce_launch(const half_t* x, const half_t* dy, int M, int C, int nstreams, const float* mean,
                         const float* rstd, const float* gamma, const float* beta, int relu, float* sums, float* ws,
                         int64_t ws_floats, float* dbeta, float* dgamma, float gscale, int param_stream, hipStream_t st);
int bn_bwd_apply_launch(const half_t* x, const half_t* dy, half_t* dx, int M, int C, int nstreams, float count,
                        const float* mean, const float* rstd, const float* gamma, const float* beta, int relu,
                        const float* sums, int* cnt, hipStream_t st);
int act_bwd_launch(const half_t* y, const half_t* dy, half_t* dpre, int M, int C, int act, float* colsum, float* ws,
                   int64_t ws_floats, float* dbias, int dbias_n, float gscale, hipStream_t st);
int colsum_rows_launch(const half_t* x, int M, int C, float* sums2C, float* ws, int64_t ws_floats, float* dbias,
                       int dbias_n, float gscale, hipStream_t st);
int colsum_acc_launch(const void* src, int is_f16, int M, int C, int64_t ld_row, int64_t ld_col, float scale, float* dst,
                      hipStream_t st);

// api.hip: routing probe (fmri_igemm_route, fmri_wgrad_route).  Every igemm and wgrad launch function calls route_probe()
// with the name of the kernel instantiation it is about to launch, after its own support checks and before any HIP call;
// while a probe is active on the calling thread the name is recorded and `true` returned: the launcher then returns OK
// without touching the GPU.
bool route_probe(const char* fmt, ...);

// loss.hip: process-wide deterministic-reduction switch (fmri_set_deterministic)
extern int g_deterministic;

int latent_fwd_launch(const float* head, const float* eps, int B, int Z, int zp, half_t* z16, float* kl_rows,
                      float* kl_total, int sample, hipStream_t st);
int latent_ranged_launch(const float* head, const float* eps, int B, int Z, int zp, half_t* z16, float* kl_rows,
                         float* kl_total, int sample, float* z32, float* zmax, float* zscale, float cap, int phase,
                         hipStream_t st);
int rows_absmax_launch(const float* x, int64_t n, float* zmax, hipStream_t st);
float latent_range_scale_host(float zmax, float cap);
int latent_bwd_launch(const float* head, const float* eps, const float* dz, int ldz, float dz_unscale, float kl_w,
                      const float* kl_dev, int B, int Z, float out_scale, half_t* dhead16, float* dhead32, int sample,
                      hipStream_t st);
int feat_mse_launch(const half_t* feat, int B, int F, float* mse_rows, float* mse_total, hipStream_t st);
int feat_mse_bwd_launch(const half_t* feat, int B, int F, half_t* dfeat, float gscale, const float* norm,
                        hipStream_t st);
// featloss.hip: the feature-matching term for wide rows (recon_level 1 / 2), (row, column chunk) tasks on a CU-sized grid
int feat_mse_wide_chunk();
int64_t feat_mse_wide_ws_floats(int B, int F);
int feat_mse_wide_launch(const half_t* feat, int B, int F, float* mse_rows, float* mse_total, float* ws,
                         hipStream_t st);
int feat_mse_bwd_wide_launch(const half_t* feat, int B, int F, half_t* dfeat, float gscale, const float* norm,
                             int zero_rows, hipStream_t st);
int pixel_sq_launch(const half_t* x, const half_t* xt, int64_t npix, int C, int Cp, float* total, half_t* dxt,
                    float gscale, hipStream_t st);
int gan_head_launch(const float* logit, int ldl, int B, float* prob, float* scal, int parts, hipStream_t st);
int gan_head_bwd_launch(const float* logit, int ldl, int B, half_t* dlogit, int ldg, float gscale, const float* norm,
                        int parts, hipStream_t st);
int wae_logloss_launch(const float* logit, int ldl, int n, int one_minus, float w, float* total, float* prob,
                       half_t* dlogit, int ldg, float gscale, hipStream_t st);
int64_t mmd_imq_ws_bytes(int n, int d);
int mmd_imq_launch(const float* q, int ldq, const float* p, int ldp, int n, int d, float sigma2, const float* scales,
                   int nscales, float w, float* total, float* dq, int ldd, float gscale, void* ws, int64_t ws_bytes,
                   hipStream_t st);
int64_t latent_nce_ws_bytes(int n, int d);
int latent_nce_launch(const float* q, int ldq, const float* t, int ldt, int n, int d, float tau, int symmetric, float w,
                      float* total, float* top1, float* dq, int ldd, float gscale, void* ws, int64_t ws_bytes,
                      hipStream_t st);
int compose_gate_launch(float* scal, int* flags, float batch, float nfeat, float npix, float lambda_mse,
                        float equilibrium, float margin, float beta, const float* hp_dev, int mode, int gate_on,
                        int force_dis, int force_dec, hipStream_t st);
int counter_inc_launch(int* t, hipStream_t st);
int rng_normal_launch(const int64_t* state, float* out, int rows, int cols, int ld, int64_t row0, int sid, float scale,
                      hipStream_t st);
int rng_u32_launch(const int64_t* state, int32_t* out, int64_t n, int64_t start, int sid, int lo, int hi,
                   hipStream_t st);
int rng_advance_launch(int64_t* state, int64_t nblocks, hipStream_t st);
int sampler_indices_launch(const int64_t* state, int N, int B, int64_t row0, int32_t* idx, hipStream_t st);
int sampler_advance_launch(int64_t* state, int64_t N, int64_t B_global, hipStream_t st);
// csrc/diffaug.hip (square images of H x H pixels; `img0`: the first image's index in the [orig | pred | sampled] layout)
int diffaug_params_launch(const int64_t* state, float* table, int rows, int64_t row0, int sid, int H, int sh, int cut,
                          int policy, hipStream_t st);
int diffaug_fwd_launch(const half_t* src, half_t* dst, int N, int H, const float* table, int B, int img0, hipStream_t st);
int diffaug_bwd_launch(const half_t* ga, half_t* da, const half_t* gb, half_t* db, int N, int H, const float* table, int B,
                       int img0, hipStream_t st);
// csrc/voxaug.hip (fMRI rows fp32 [B][V] -> fp16 [B][pad8(V)]; `table`: fp32 [B][8], include/fmri_hip.h fmri_voxaug_apply)
int voxaug_params_launch(const int64_t* state, float* table, int rows, int64_t row0, int sid, int V, float gain, float sigma,
                         float p, int rescale, int span_len, float prob, hipStream_t st);
int voxaug_apply_launch(const float* src, int V, int B, const float* table, const int64_t* state, int64_t row0,
                        int sid_noise, int sid_drop, half_t* dst16, float* dst32, hipStream_t st);
// csrc/schedule.hip (`sched`: an fmri_schedule of include/fmri_hip.h)
int epoch_begin_launch(const int64_t* feed_state, void* sched, float* lr0, float* lr1, float* lr2, float* lr3, float* hp3,
                       int64_t* epoch_out, hipStream_t st);
int schedule_seek_host(void* sched, int64_t epoch, float* out7);
int trainlog_append_launch(const void* const* src, const int32_t* kind, int K, float* ring, int64_t capacity,
                           int64_t* counter, hipStream_t st);
// csrc/state.hip (`segs`: fmri_state_seg tables of include/fmri_hip.h; state_table_chunks: the host check of a table,
// its chunk count or E_BADARG)
int64_t state_layout(const int64_t* bytes, int nseg, int64_t* offsets_out);
int state_nontemporal(int on);
int64_t state_table_chunks(const void* segs_host, int nseg, int64_t slot_bytes);
int state_copy_launch(const void* segs_dev, int nseg, int64_t chunks, void* ring, int64_t slot_bytes, int dir,
                      const int64_t* feed_state, int every, int capacity, uint64_t fingerprint,
                      const int64_t* log_counter, hipStream_t st);
// csrc/ema.hip (`segs`: fmri_ema_seg tables, `state`: an fmri_ema_state of include/fmri_hip.h; ema_table_chunks: the host
// check of a table, its chunk count or E_BADARG; op 0 updates the shadows, 1 exchanges live and shadow)
float ema_decay_at(int32_t t, int32_t start, float decay, int32_t warmup);
int64_t ema_table_chunks(const void* segs_host, int nseg);
int ema_launch(const void* segs_dev, int nseg, int64_t chunks, const void* state_dev, int op, hipStream_t st);
int axpby_f16_launch(const half_t* x, const half_t* y, half_t* out, int64_t n, float a, float b, const float* pa,
                     const float* pb, hipStream_t st);
int sumsq_launch(const float* x, int64_t n, float* acc, hipStream_t st);
int renorm_launch(const float* x, half_t* out, int64_t n, float scale, const float* sumsq, float count,
                  const float* factor_in, float* factor_out, hipStream_t st);
int sumsq64_launch(const float* x, int64_t n, double* acc, int zero_first, hipStream_t st);
int renorm64_launch(const float* x, half_t* out, int64_t n, float scale, const double* sumsq, float count,
                    const float* factor_in, float* factor_out, hipStream_t st);
int rmsprop_launch(float* p, const float* g, float* sq, int64_t n, float lr, float alpha, float eps, float gscale,
                   const float* gdev, float clamp, const int* flag, const float* lr_dev, hipStream_t st);
int adam_launch(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps,
                float bc1, float bc2_sqrt, float gscale, const float* gdev, float clamp, const int* flag,
                const float* lr_dev, const int* t_dev, hipStream_t st);

int ingest_u8_launch(const uint8_t* src, int N, int H, int W, int C, const int* flip, const int* shift,
                     const float* mean3, const float* std3, half_t* dst16, float* dst32, hipStream_t st);
int ingest_u8_gather_launch(const uint8_t* src, const int32_t* idx, int N_pool, int N, int H, int W, int C,
                            const int* flip, const int* shift, const float* mean3, const float* std3, half_t* dst16,
                            float* dst32, int* err, hipStream_t st);
int gather_rows_launch(const float* src, int N_pool, int V, const int32_t* idx, int B, float* dst32, half_t* dst16,
                       int* err, hipStream_t st);
int resize_coeffs(int in_size, int out_size, int32_t* bounds, int32_t* coef, int ksize_cap);
int crop_resize_u8_launch(const uint8_t* pool, const int64_t* offsets, const int32_t* dims, int N, int crop, int S,
                          const int32_t* hb, const int32_t* hk, int hks, const int32_t* vb, const int32_t* vk, int vks,
                          int vcount_max, uint8_t* out, hipStream_t st);
int pcc_launch(const float* x, const float* y, int64_t n, double* sums5, float* out, hipStream_t st);
int ssim_launch(const float* a, const float* b, int planes, int H, int W, double* acc2, float* ssim, float* contrast,
                hipStream_t st);
int64_t pcc_matrix_ws_bytes(int N, int M, int64_t D);
int pcc_matrix_launch(const float* pred, const float* truth, int N, int M, int64_t D, float* S, int ldS, void* ws,
                      int64_t ws_bytes, hipStream_t st);
int64_t ssim_pairs_ws_bytes(int N, int M, int C, int H, int W);
int ssim_pairs_launch(const float* pred, const float* truth, int N, int M, int C, int H, int W, const int* pairs, int P,
                      float* out, void* ws, int64_t ws_bytes, hipStream_t st);
int64_t image_metrics_ws_bytes(int N, int H, int W);
int image_metrics_launch(const half_t* pred, const half_t* truth, int N, int H, int W, int C, const float* scale,
                         const float* shift, void* ws, int64_t ws_bytes, float* out7, double* acc4, int acc_mode,
                         hipStream_t st);
// csrc/nway.hip
int nway_cmax();
int64_t nway_ws_bytes(int n, int H, int W);
int nway_scores_launch(const half_t* pred, const half_t* truth, int n, int H, int W, int C, int top,
                       const int64_t* rng_state, int sid, void* ws, int64_t ws_bytes, float* s_pcc, float* s_ssim,
                       int32_t* distractors, float* out8, double* acc6, int acc_mode, hipStream_t st);
// csrc/egress.hip
int64_t images_u8_ws_bytes(int n);
int64_t images_u8_out_bytes(int n, int H, int W, int mode, int R, int nrow, int padding);
int images_u8_launch(const half_t* src, int n, int H, int W, int mode, int R, int nrow, int padding, void* ws,
                     int64_t ws_bytes, uint8_t* out, const int64_t* slot_dev, int64_t slot_stride, int slot_mod,
                     uint8_t* present_dev, hipStream_t st);
int images_u8_open_launch(const int64_t* slot_dev, int slot_mod, int64_t* opened_dev, uint8_t* present_dev,
                          int64_t present_stride, int kinds, hipStream_t st);

}  // namespace fmri
