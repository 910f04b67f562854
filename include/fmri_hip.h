/*
 * fmri_hip.h -- C ABI of libfmri_hip.so, the MI355X (gfx950) kernel library behind the drop-in
 * `models.vae_gan` engine.
 *
 * The reference (MariaPdg/thesis-fmri-reconstruction) is pure Python on PyTorch: it has no FFI of its
 * own.  The boundary this library sits behind is the ATen operator set that `models/vae_gan.py` calls
 * (SURVEY.md 8a row a15); each entry point below names the reference call site(s) it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; every buffer (incl. workspaces) is owned by the caller
 *     (the PyTorch caching allocator in our host code); the library allocates nothing and keeps no
 *     mutable global state => re-entrant, callable from autograd worker threads.
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*); no host sync.
 *   - return 0 on success, a negative fmri_err otherwise; never throws, never exits.
 *   - activations: fp16 NHWC rows [N][H][W][C] with C a multiple of 8 (images are channel-padded 3->8);
 *     weights: fp16 "packed" matrices [rows_pad][kpad] produced by fmri_pack_weight;
 *     reductions / statistics / losses / master weights: fp32.
 */
#ifndef FMRI_HIP_H
#define FMRI_HIP_H
#include <stdint.h>
#include "fmri_hip_contrast.h"   /* contrastive latent alignment: its two entry points are declared there */
#ifdef __cplusplus
extern "C" {
#endif

enum fmri_err { FMRI_OK = 0, FMRI_E_BADARG = -1, FMRI_E_UNSUPPORTED = -2, FMRI_E_LAUNCH = -3, FMRI_E_WORKSPACE = -4 };
enum fmri_act { FMRI_ACT_NONE = 0, FMRI_ACT_RELU = 1, FMRI_ACT_TANH = 2, FMRI_ACT_SIGMOID = 3 };
/* contraction modes of fmri_igemm */
enum fmri_mode {
    FMRI_CONV = 0,        /* correlation: in pixel = out*stride + k - pad          (nn.Conv2d fwd, deconv dgrad) */
    FMRI_TCONV2 = 1,      /* stride-2 transposed conv as 4 parity classes          (nn.ConvTranspose2d fwd, conv-s2 dgrad) */
    FMRI_CONV_FLIP = 2    /* stride-1 correlation with flipped taps: in = out + pad - k   (conv-s1 dgrad) */
};

int fmri_version(void);
const char* fmri_last_error_string(int code);

/* exact division helper exported for the host-side tests of the kernels' index arithmetic */
uint32_t fmri_test_fastdiv(uint32_t n, uint32_t d);

/* Geometry of parity class (cy,cx) of a k x k, stride-2, pad-p transposed convolution: first tap
 * (py,px), tap grid TH x TW, padded K and element offset of the class's packed weight block. */
int fmri_tconv_class(int k, int pad, int cy, int cx, int ci, int rows_pad, int* py, int* px, int* th, int* tw,
                     int* kpad, int64_t* w_off);
/* padded K (multiple of 64) of a T-tap, ci-channel reduction */
int fmri_kpad(int taps, int ci);

/* ---- weights ------------------------------------------------------------------------------------
 * dst[(ta*A + a)][(tb*Bp + b)] = (fp16) src[a*sa + ta*sta + b*sb + t(tb)*stb],  t(tb) = (py+step*ty)*KW + (px+step*tx),
 * zero padded to [rows_pad][kpad].  Replaces the implicit weight layout handling of ATen conv/linear
 * (models/vae_gan.py:18,46,79,107,119,146,156) incl. the (C,H,W) flatten order at :89,:127,:181. */
int fmri_pack_weight(const float* src, void* dst, int64_t sa, int64_t sta, int64_t sb, int64_t stb, int A, int TA,
                     int B, int KW, int py, int px, int step, int TH, int TW, int rows_pad, int kpad, void* stream);
/* Batched fmri_pack_weight: a device-resident table of rows (filled on the host with fmri_pack_entry_fill, which
 * returns the number of blocks of the row, 0 = not eligible, use fmri_pack_weight) repacked by ONE launch --
 * what a sub-network needs after its optimizer step. */
int fmri_pack_entry_bytes(void);
int fmri_pack_entry_fill(void* host_entry, const float* src, void* dst, int64_t sa, int64_t sta, int64_t sb,
                         int64_t stb, int A, int TA, int B, int KW, int py, int px, int step, int TH, int TW,
                         int rows_pad, int kpad, int tile_begin);
int fmri_pack_weight_batch(const void* table_dev, int n, int total_tiles, void* stream);
/* inverse map for fp32 weight gradients: dst[...] (+)= scale * sum_z src[z*slab_stride + (ta*A+a)*ld + tb*Bp + b],
 * z < nslabs (the per-split partial results of fmri_wgrad, mode 2) */
int fmri_unpack_grad(const float* src, float* dst, int64_t sa, int64_t sta, int64_t sb, int64_t stb, int A, int TA,
                     int B, int KW, int py, int px, int step, int TH, int TW, int ld, float scale, int accumulate,
                     int nslabs, int64_t slab_stride, void* stream);

/* ---- contractions (MFMA) ------------------------------------------------------------------------
 * out = act(bias + contraction(in, w)); see csrc/igemm.hip.  Replaces F.conv2d / F.conv_transpose2d /
 * F.linear forward and data-gradient (models/vae_gan.py:26,32,57,90-92,126,128,175,182).
 * out_f32 != 0: raw fp32 result written to `splits` slabs (slab_stride elements apart), no bias/act. */
int fmri_igemm(const void* in, const void* w, void* out, const float* bias, const void* zero16, int N, int Hi, int Wi,
               int Ci, int Ho, int Wo, int CoStore, int Co, int k, int stride, int pad, int mode, int act,
               int out_f32, int splits, int64_t slab_stride, int bn_tile, void* stream);
/* The same contraction with an epilogue that a following BatchNorm needs (models/vae_gan.py:26-34,57-59: conv -> bn):
 * every block writes, per output channel, sum x and sum x^2 of the values it STORED (valid output pixels only) to its
 * own row of stat_part[group][stat_rows_cap][2][CoStore] (plain stores, deterministic), group = image / stat_group_n
 * (stat_group_n = 0: one group; a row tile never mixes groups).  *ep_done = rows written per group (they are the
 * first rows of each group; fold them with fmri_bn_fold_finalize), or 0 when the kernel behind this geometry has no
 * such epilogue, a tile would straddle two groups or stat_rows_cap is too small -- then use fmri_bn_stats on the
 * output.  N*Ho*Wo/128 + 8 rows per group always suffice.  w_elems: elements of the packed weight buffer `w` (the
 * descriptor-addressed kernels bound their weight DMA with it; 0 = unknown, those kernels are skipped). */
typedef struct fmri_epilogue {
    float* stat_part;        /* NULL: no statistics */
    int32_t stat_rows_cap;   /* rows allocated per group */
    int32_t stat_group_n;    /* images per statistics group, 0 = all images */
    /* BatchNorm (+ReLU) BACKWARD statistics, for the data gradient that produces the cotangent dy of a BatchNorm output
     * (autograd of models/vae_gan.py:28-29,58-59): with the saved forward input bn_x of that BatchNorm (geometry of
     * `out`), xhat = (x - mean)*rstd and on = !relu || xhat*gamma + beta > 0, `out` receives g = on ? dy : 0 and the rows
     * hold (sum g, sum g*xhat).  Group i (<= 4: cotangent streams / decoder calls stacked along the batch) reads x from
     * image bn_x_img0[i] on, with the batch statistics of its forward call.  NULL bn_x: forward statistics.  Requires
     * stat_part, no bias / activation; if *ep_done comes back 0 `out` holds the plain dy (use fmri_bn_bwd_reduce). */
    const void* bn_x;
    const float* bn_gamma;
    const float* bn_beta;
    const float* bn_mean[4];
    const float* bn_rstd[4];
    int32_t bn_x_img0[4];
    int32_t bn_relu;
    int32_t reserved;
    /* ReLU backward of the layer BELOW, for a data gradient whose output is the cotangent of that layer's ReLU output
     * (autograd of nn.ReLU after discriminator.conv.0, models/vae_gan.py:145-147): act_y = the saved ReLU output
     * (geometry of `out`), `out` receives (act_y > 0) ? dy : 0.  Independent of the statistics fields.  Kernels that
     * apply it set FMRI_EP_ACT_APPLIED in *ep_done; if the bit comes back clear `out` holds the plain dy (use
     * fmri_act_bwd). */
    const void* act_y;
    /* Per-channel affine map (+ ReLU) on the fp32 accumulators in front of the fp16 store: out = relu?(acc * aff_scale[co] +
     * aff_shift[co]) -- an eval-mode BatchNorm (running statistics, models/vae_gan.py:288-297 under model.eval()) folded
     * into the convolution that feeds it: no pass over the raw output, one rounding less.  Vectors of CoStore floats.  Only
     * without statistics, bias and activation.  Kernels that apply it set FMRI_EP_AFFINE_APPLIED in *ep_done; if the bit
     * comes back clear `out` holds the plain contraction (use fmri_bn_apply). */
    const float* aff_scale;
    const float* aff_shift;
    int32_t aff_relu;
    int32_t reserved2;
} fmri_epilogue;
#define FMRI_EP_ACT_APPLIED 0x40000000
#define FMRI_EP_AFFINE_APPLIED 0x20000000
int fmri_igemm_ep(const void* in, const void* w, void* out, const float* bias, const void* zero16, int N, int Hi,
                  int Wi, int Ci, int Ho, int Wo, int CoStore, int Co, int k, int stride, int pad, int mode, int act,
                  int out_f32, int splits, int64_t slab_stride, int bn_tile, int64_t w_elems, const fmri_epilogue* ep,
                  int* ep_done, void* stream);
/* Name of the kernel instantiation fmri_igemm_ep routes a call with these arguments to, e.g.
 * "fmri::igemm_c5w_kernel<16,1>" ("none": nothing to launch).  The device pointers of fmri_igemm_ep are replaced by
 * flags (has_bias; stat_rows_cap > 0: statistics epilogue asked with that row capacity / stat_group_n; want_bn_bwd,
 * want_act_y, want_affine: the other fmri_epilogue fields set).  Pure host code -- no GPU is touched, it runs on a machine
 * without one -- and the ONLY statement of the routing: profilers, benches and tests ask it instead of mirroring the
 * rules.  name_out receives at most cap - 1 characters. */
int fmri_igemm_route(int N, int Hi, int Wi, int Ci, int Ho, int Wo, int CoStore, int Co, int k, int stride, int pad,
                     int mode, int act, int out_f32, int splits, int bn_tile, int64_t w_elems, int has_bias,
                     int stat_rows_cap, int stat_group_n, int want_bn_bwd, int want_act_y, int want_affine, char* name_out,
                     int cap);
/* dW[a][tap*Bc+b] (+)= sum_m P[m][a] * Q[gather(m,tap)][b]; see csrc/wgrad.hip.  Replaces the weight
 * gradients autograd computes for the same modules (train/train_vgan_stage1.py:412,422,430). */
int fmri_wgrad(const void* P, const void* Q, float* out, const void* zero16, int N, int Yc, int Xc, int A, int Hq,
               int Wq, int Bc, int k, int stride, int pad, int flip, int apad, int ba_tile, int ldo, int splits,
               int atomic, void* stream);
/* The same launch under a device-side condition: with gate != NULL and *gate == 0 when the kernel starts, it does
 * nothing (`out` is left as it is).  The reference runs `loss_decoder.backward()` / `loss_discriminator.backward()` only
 * `if train_dec:` / `if train_dis:` (train_vgan_stage1.py:420-431: the equilibrium gate of :395-403); the engine's
 * gate is evaluated on the device (fmri_compose_gate_dev), so the host always issues the launches and the kernels of a
 * sub-network that is not trained in this step retire at once. */
int fmri_wgrad_if(const int* gate, const void* P, const void* Q, float* out, const void* zero16, int N, int Yc, int Xc,
                  int A, int Hq, int Wq, int Bc, int k, int stride, int pad, int flip, int apad, int ba_tile, int ldo,
                  int splits, int atomic, void* stream);
/* flip = 0: Q pixel = m*stride + tap - pad.  flip = 1 (stride 1 only): Q pixel = m + pad - tap, i.e. the roles of
 * the two activations are exchanged so that the GATHERED operand is the one with fewer channels.
 *
 * `atomic` is one of the five modes below; it fixes what `out` is and what `splits` counts.  A caller does not work the
 * pair out itself: fmri_wgrad_route plans it for a geometry, and the dispatch of fmri_wgrad_if runs exactly what the plan
 * names.  Three kernels stand behind the modes: the window-resident kernel (csrc/wgrad_win.hip: 5x5, pad 2, stride 2,
 * 128-row tiles, Bc a multiple of 32, operands within 2^30 elements), the narrow kernel (csrc/wgrad_narrow.hip: 5x5,
 * pad 2, stride 1, A = apad = 32, Bc = 8, equal planes, P within 2^31 elements) and the generic kernel (csrc/wgrad.hip). */
#define FMRI_WGRAD_STORE 0         /* out [apad][ldo], plain stores; splits = 1.  Generic kernel. */
#define FMRI_WGRAD_ATOMIC 1        /* out [apad][ldo], PRE-ZEROED, atomic adds.  Window kernel where the geometry fits it:
                                    * splits = block budget per (128-row, 32-channel) group over the 4 parity planes.
                                    * Else the generic kernel: splits = K splits. */
#define FMRI_WGRAD_PLANE_SLABS 2   /* window kernel only (else FMRI_E_UNSUPPORTED): splits = the same block budget; K piece
                                    * z of a parity plane stores to out + z*apad*ldo.  fmri_wgrad_slabs() slabs, every one
                                    * written in full. */
#define FMRI_WGRAD_NARROW_SLABS 3  /* narrow kernel only (else FMRI_E_UNSUPPORTED): out holds `splits` PRE-ZEROED slabs that
                                    * the blocks add into round-robin; column k*k*Bc of row a holds sum_m P[m][a].  With
                                    * splits = fmri_wgrad_narrow_blocks(), the blocks launched, every element is added
                                    * once, onto zero: bit-reproducible. */
#define FMRI_WGRAD_KSPLIT_SLABS 4  /* generic kernel: out holds `splits` ZERO-FILLED slabs, K split z stores slab z with
                                    * plain stores.  The kernel may use fewer splits than asked for (the plan's `stored`);
                                    * the other slabs stay zero.  Summed in slab order: bit-reproducible. */
/* fmri_unpack_grad / fmri_apply_batch sum the slabs of modes 2 - 4. */
int fmri_wgrad_slabs(int N, int Yc, int Xc, int k, int pad, int splits);
/* number of blocks fmri_wgrad(..., FMRI_WGRAD_NARROW_SLABS) launches for this geometry */
int fmri_wgrad_narrow_blocks(int N, int Yc, int Xc);
/* What to launch for a geometry, and into what: the counterpart of fmri_igemm_route and the ONLY statement of the
 * weight-gradient routing.  Pure host code -- no GPU is touched, it runs on a machine without one.  The geometry
 * arguments are those of fmri_wgrad_if up to ldo.  The caller's policy: win_blocks, the window kernel's block budget for
 * the whole launch (per group it is win_blocks / groups, at least 4); slab_limit, the most K pieces the window kernel
 * still writes as slabs before it turns to atomics; deterministic != 0 asks for a slab mode wherever partial sums meet.
 * Returns what fmri_wgrad_if returns for the planned call (the geometry is validated the same way). */
typedef struct {
    int32_t atomic;      /* the FMRI_WGRAD_* mode to pass to fmri_wgrad_if */
    int32_t splits;      /* the `splits` argument to pass */
    int32_t slabs;       /* 0: out is one [apad][ldo] matrix; n: out is [n][apad][ldo] */
    int32_t zeroed;      /* out must hold zeros at the launch */
    int32_t stored;      /* slabs the launch writes (< slabs possible in FMRI_WGRAD_KSPLIT_SLABS); 0 when slabs is 0 */
    int32_t colsum;      /* narrow kernel: the spare column holds the bias gradient's sums */
    int32_t pieces[4];   /* window kernel: K pieces of parity plane py*2 + px; else 0 */
    char kernel[64];     /* the instantiation the dispatch reached under the probe, e.g. "fmri::wgrad_kernel<64,1,4>" */
} fmri_wgrad_plan;
int fmri_wgrad_route(int N, int Yc, int Xc, int A, int Hq, int Wq, int Bc, int k, int stride, int pad, int flip, int apad,
                     int ba_tile, int ldo, int win_blocks, int slab_limit, int deterministic, fmri_wgrad_plan* plan);

/* ---- deterministic-reduction mode (process-wide; initial value: environment FMRI_DETERMINISTIC=1).  When on, the
 * loss / norm kernels that end in an atomic add onto a device scalar (fmri_latent_fwd, fmri_feat_mse, fmri_pixel_sq,
 * fmri_gan_head*, fmri_wae_logloss, fmri_sumsq, fmri_pcc) are launched as ONE block each, i.e. every total is a
 * fixed-order sum.  Together with the slab forms of fmri_wgrad (atomic = 2, 3 with one slab per block, 4) and
 * dbias5 = NULL in fmri_mlp_bwd -- which the caller selects -- two runs of the same training step on the same inputs
 * then produce bit-identical parameters.  A verification mode (the one-block sums cost a few hundred microseconds at
 * batch 256); the default trades the fixed order for atomics.  Returns the previous value. */
int fmri_set_deterministic(int on);
int fmri_get_deterministic(void);

/* ---- batch ingest: uint8 [N][H][W][C = 1|3] (already cropped / resized) -> normalised fp16 NHWC8 (engine input)
 * and / or fp32 NCHW (module API input).  Per image: optional horizontal flip (flip_dev[n] != 0, may be NULL), then an
 * integer shift (shift_dev[2n] rows, [2n+1] columns, edge-replicated like scipy.ndimage.shift(order=0, 'nearest'),
 * may be NULL), u8/255, grey -> 3 channels, (v - mean) / std.  Replaces RandomHorizontalFlip / RandomShift / ToTensor
 * / GreyToColor / Normalize of train_vgan_stage1.py:162-170 and data_preprocessing/data_loader.py:186-217,374-401. */
int fmri_ingest_u8(const uint8_t* src, int N, int H, int W, int C, const int* flip_dev, const int* shift_dev,
                   float mean0, float mean1, float mean2, float std0, float std1, float std2, void* dst16,
                   float* dst32, void* stream);
/* The same for a batch read out of a device-resident pool by index (fmri_hip/feed.py): image n of the output is
 * src[idx_dev[n]] of the pool src [N_pool][H][W][C] (idx_dev: int32 [N], e.g. from fmri_sampler_indices) passed through
 * the same flip (flip_dev[n]) / shift (shift_dev[2n], [2n+1]) / /255 / grey -> RGB / normalise; dst16 (fp16 NHWC8, 16-byte
 * aligned) and dst32 (fp32 NCHW) are bit-identical to fmri_ingest_u8 on the gathered images.  One pass: the pool is read
 * in place, no gathered uint8 batch is written.  An index outside [0, N_pool) is never dereferenced: it is clamped into
 * the range, and err_dev (device int, may be NULL, caller-zeroed, added to) counts the images it happened to. */
int fmri_ingest_u8_gather(const uint8_t* src, const int32_t* idx_dev, int N_pool, int N, int H, int W, int C,
                          const int* flip_dev, const int* shift_dev, float mean0, float mean1, float mean2, float std0,
                          float std1, float std2, void* dst16, float* dst32, int* err_dev, void* stream);
/* Row gather of the same feed: src [N_pool][V] fp32 (the fMRI of the dataset) -> dst32 [B][V] = src[idx_dev[b]] and / or
 * dst16 [B][pad8(V)] (16-byte aligned) = fp16 of it, round to nearest even as fmri_rows_f32_to_f16 at scale 1, the columns
 * from V on zero.  Either may be NULL.  Indices are clamped and counted as above (once per row). */
int fmri_gather_rows_f32(const float* src, int N_pool, int V, const int32_t* idx_dev, int B, float* dst32, void* dst16,
                         int* err_dev, void* stream);

/* ---- CenterCrop((crop, crop)) + Resize((S, S)) of a ragged batch of decoded uint8 images, the head of the COCO
 * pipeline (train/train_vgan_stage1.py:162-165: torchvision 0.5.0 transforms on PIL images).  Bit-exact with
 * torchvision.transforms.functional.center_crop / .resize over Pillow's 8-bit ImagingResample (BILINEAR: antialiased
 * triangle filter, 22-bit fixed-point coefficients, horizontal pass rounded to uint8, then vertical pass).
 * fmri_resize_coeffs (HOST function, no stream): coefficient tables of one pass in_size -> out_size: bounds[out][2] =
 *   (first input index, count), coef[out][ksize]; returns ksize > 0, 0 when in_size == out_size (identity pass: no tables
 *   needed), FMRI_E_WORKSPACE when ksize > ksize_cap (ksize = 2 * ceil(max(in / out, 1)) + 1).
 * fmri_crop_resize_u8: pool = the images back to back (HWC, C = 1 or 3 per image), offsets_dev[n] = byte offset of image
 *   n, dims_dev[n] = (H, W, C); both passes resample crop -> S with the tables of fmri_resize_coeffs(crop, S) uploaded by
 *   the caller (hks / vks = their ksize, 0 = identity), vcount_max = the largest count of the vertical table (LDS rows
 *   per block; 1 for the identity).  out [N][S][S][3] uint8, grey images replicated to three channels (GreyToColor,
 *   data_preprocessing/data_loader.py:374-401).  Pixels of the crop box outside the image are zeros (PIL crop). */
int fmri_resize_coeffs(int in_size, int out_size, int32_t* bounds, int32_t* coef, int ksize_cap);
int fmri_crop_resize_u8(const uint8_t* pool, const int64_t* offsets_dev, const int32_t* dims_dev, int N, int crop, int S,
                        const int32_t* hb_dev, const int32_t* hk_dev, int hks, const int32_t* vb_dev, const int32_t* vk_dev,
                        int vks, int vcount_max, uint8_t* out, void* stream);

/* ---- evaluation metrics of the validation loop (train/train_utils.py) ------------------------------
 * fmri_pcc : PearsonCorrelation.forward (:276-292) over n fp32 elements (whole batch), *out = coefficient.
 * fmri_ssim: StructuralSimilarity.forward (:343-420, size_average=True): mean SSIM (and the mean contrast term of
 *            full=True) over planes = N*C images of H x W (>= 11), 11x11 Gaussian sigma 1.5, zero padding.
 * ws5 / ws2: 5 / 2 doubles of device scratch (zeroed by the call). */
int fmri_pcc(const float* pred, const float* truth, int64_t n, double* ws5, float* out, void* stream);
int fmri_ssim(const float* img1, const float* img2, int planes, int H, int W, double* ws2, float* ssim,
              float* contrast, void* stream);

/* ---- pairwise similarity of n-way identification (objective_assessment, train/train_utils.py:752-816) ----------
 * fmri_pcc_matrix: S[i * ldS + j] = PearsonCorrelation.forward(pred_i, truth_j) (:276-292 over ONE image) for
 *   pred [N][D], truth [M][D] fp32 contiguous rows, D = C*H*W.  First pass: per-row mean and centred norm in fp64;
 *   second pass: the centred Gram from v_mfma_f32_16x16x4_f32, each operand centred as it is loaded, K split into
 *   fixed 1024-element chunks summed in chunk order (fp64).  ws: fmri_pcc_matrix_ws_bytes(N, M, D) bytes (< 0: bad
 *   geometry); FMRI_E_WORKSPACE if smaller.
 * fmri_ssim_pairs: out[p] = StructuralSimilarity.forward(pred[pairs[2p]], truth[pairs[2p+1]]) (:343-420, size_average,
 *   mean over C, H, W) for pred [N][C][H][W], truth [M][C][H][W] fp32 and pairs int32 [P][2] in device memory
 *   (0 <= i < N, 0 <= j < M; a pair outside writes NaN).  11x11 Gaussian sigma 1.5, padding 5, C1 = 1e-4,
 *   C2 = 9e-4; H or W < 11: FMRI_E_UNSUPPORTED, as fmri_ssim.  The filtered x and x^2 of every image are computed
 *   once per call into ws (fmri_ssim_pairs_ws_bytes(N, M, C, H, W) bytes: 16 (N + M) C H W), then one block per pair
 *   filters the cross term x_i y_j and sums its SSIM map in a fixed order.  Window, filtered statistics and SSIM map
 *   are fp64 (the variances cancel in fp32).  P = 0 launches nothing.
 * Both: no atomics, no allocation, no host sync.  A pair's value is a bitwise function of the two images only (not of
 *   its position, N, M or P), so two calls are bit-identical and truth_j == truth_i bitwise gives S_ij == S_ii. */
int64_t fmri_pcc_matrix_ws_bytes(int N, int M, int64_t D);
int fmri_pcc_matrix(const float* pred, const float* truth, int N, int M, int64_t D, float* sim, int ldS, void* ws,
                    int64_t ws_bytes, void* stream);
int64_t fmri_ssim_pairs_ws_bytes(int N, int M, int C, int H, int W);
int fmri_ssim_pairs(const float* pred, const float* truth, int N, int M, int C, int H, int W, const int* pairs, int P,
                    float* out, void* ws, int64_t ws_bytes, void* stream);

/* ---- validation metrics of a batch in the engine's image layout (evaluation pass of the fused steps) ----------
 * fmri_image_metrics: out7[0..2] = PCC (PearsonCorrelation.forward over the whole batch, :276-292), mean SSIM
 *   (StructuralSimilarity.forward, size_average, :343-420: 11x11 Gaussian sigma 1.5, padding 5, C1 = 1e-4, C2 = 9e-4)
 *   and MSE (nn.MSELoss over the N C H W real elements) of pred16 against truth16, both fp16 [N][H][W][Cp] with
 *   channels 0..C-1 real (lanes C..Cp-1 may hold anything: they reach no sum), 16-byte aligned.  scale / shift: HOST
 *   float[C] each, or both NULL -- the metrics are then those of v * scale[c] + shift[c] (denormalize_image, :234-240),
 *   applied in fp32 to in-image pixels only (the padding stays 0).  Launch 1: one block per 16 x 16 tile of one pair,
 *   all channels, one 16-byte load per pixel of the 26 x 26 halo; window, filtered statistics and SSIM map in fp64
 *   (as fmri_ssim_pairs), plus the tile's fp64 sums of x, y, x^2, y^2, xy and (x - y)^2; 7 doubles per block into ws
 *   (fmri_image_metrics_ws_bytes(N, H, W) bytes; < 0: bad geometry).  Launch 2: one block folds them in a fixed order.
 *   acc4 (device double[4]: sums of pcc, ssim, mse over batches, and the batch count; may be NULL): launch 2 also adds
 *   this batch -- after clearing acc4 when acc_mode = 0, on top of it when acc_mode = 1 -- and writes the running means
 *   and the count to out7[3..6]; with acc4 NULL out7[3..6] are left alone.
 *   No atomics, no allocation, no host sync; two launches per call.  out7[0..2] is a bitwise function of the two
 *   tensors and (N, H, W, C, scale, shift) only: two calls are bit-identical with fmri_set_deterministic on or off.
 *   H or W < 11: FMRI_E_UNSUPPORTED, as fmri_ssim; Cp != 8: FMRI_E_UNSUPPORTED; ws_bytes too small: FMRI_E_WORKSPACE;
 *   nothing is launched then. */
int64_t fmri_image_metrics_ws_bytes(int N, int H, int W);
int fmri_image_metrics(const void* pred16, const void* truth16, int N, int H, int W, int C, int Cp,
                       const float* scale, const float* shift,      /* host float[C] each, or both NULL */
                       void* ws, int64_t ws_bytes, float* out7, double* acc4, int acc_mode, void* stream);

/* ---- n-way identification of a batch in the engine's image layout (objective_assessment, :752-816, on the device) ----
 * fmri_nway_scores: pred16 / truth16 fp16 [n][H][W][Cp], 16-byte aligned, channels 0..C-1 real (lanes C..Cp-1 may hold
 *   anything: they reach no sum), n >= 2, C <= 4.
 *   s_pcc[i * n + j] = PearsonCorrelation.forward(pred_i, truth_j) over one image, s_ssim[i * n + j] = the pair's mean
 *   SSIM: the definitions of fmri_pcc_matrix / fmri_ssim_pairs on the fp32 values of the fp16 elements (window, filtered
 *   statistics and SSIM map fp64; centring and norm fp64, the Gram fp32 MFMA chains of 16 k summed in fp64).  A pair's
 *   value is a bitwise function of its two images and (C, H, W) only -- not of i, j, n, the tile it falls into or
 *   fmri_set_deterministic -- so truth_j == truth_i bitwise gives S[i][j] == S[i][i] bitwise.  No atomics.
 *   cnt_m[i] = #{j != i : S_m[i][j] < S_m[i][i]} (NaN compares false); E_m = sum_i (cnt_m[i] / (n - 1))^(top - 1), the
 *   power by repeated multiplication and the sum in index order, both fp64 (top = 1: n).
 *   rng_state (device int64[2] of fmri_rng_normal, or NULL): distractor d[i][k], k < top - 1, is element
 *   e = i (top - 1) + k of stream sid at the state's offset under the mapping of fmri_rng_u32 on [0, n - 2],
 *   u = (w_e (n - 1)) >> 32, then d = u + (u >= i): uniform over the other images, with replacement, as random.choice
 *   in the reference (the same distribution, not the host's draws).  hit_m[i] = for all k: S_m[i][i] > S_m[i][d[i][k]]
 *   (top = 1: every image).  The offset is not moved.  distractors (int32 [n][top - 1], or NULL) receives d.
 *   acc6 (device double[6]): hits_pcc, hits_ssim, E_pcc, E_ssim, images, batches -- cleared first (acc_mode 0) or added
 *   to (1).  out8[0..3] = this batch's hits / n and E / n; out8[4..7] = acc6[0..3] / acc6[4], the score over the images
 *   so far (tp / dataset_size).  With rng_state NULL the two hit entries of out8 and acc6 are NaN.
 *   Five launches whatever n is (per-image statistics, Gram, pair SSIM blocked 16 pred x 8 truth per tile and channel,
 *   rows, fold); no allocation, no memset, no host sync.  ws: fmri_nway_ws_bytes(n, H, W) bytes (< 0: bad geometry),
 *   16-byte aligned.  Errors, before anything is launched: n < 2, top < 1, a NULL or misaligned required pointer or
 *   acc_mode outside {0, 1}: FMRI_E_BADARG; H or W < 11, Cp != 8 or C > 4: FMRI_E_UNSUPPORTED; ws_bytes too small:
 *   FMRI_E_WORKSPACE. */
int64_t fmri_nway_ws_bytes(int n, int H, int W);
int fmri_nway_scores(const void* pred16, const void* truth16, int n, int H, int W, int C, int Cp, int top,
                     const int64_t* rng_state /* device int64[2] or NULL */, int sid,
                     void* ws, int64_t ws_bytes,
                     float* s_pcc, float* s_ssim,        /* device fp32 [n][n], written */
                     int32_t* distractors,               /* device int32 [n][top-1] or NULL, written when given */
                     float* out8, double* acc6, int acc_mode, void* stream);

/* ---- uint8 image egress of a batch in the engine's image layout (the pictures the scripts write) --------------
 * fmri_images_u8: src16 fp16 [n][H][W][Cp], 16-byte aligned, channels 0..C-1 real (lanes C..Cp-1 may hold anything:
 *   they reach neither the range nor the output) -> normalised uint8 pixels, HWC.
 *   Arithmetic: torchvision 0.5.0's norm_ip / save_image as torch runs them on the CPU, every operation a separately
 *   rounded fp32 operation: lo, hi = min, max of the real elements; d = (float)((double)hi - (double)lo + 1e-5);
 *   y = (x + (-lo)) / d, a correctly rounded division; b = (uint8)clamp(y * 255 + 0.5, 0, 255), truncating.
 *   mode 0: save_image(F.interpolate(im, size=R), normalize=True) per image (evaluate(save=True),
 *     train/train_utils.py:728-735): one range per image; out [n][R][R][3] ([n][H][W][3] with R = 0), source index
 *     min((int)floorf(dst * ((float)H / R)), H - 1) (F.interpolate's default nearest mode).  0 < R < max(H, W):
 *     FMRI_E_UNSUPPORTED -- a smaller output drops pixels, and the scripts' range is that of the resized image.
 *   mode 1: make_grid(x, nrow, padding, normalize=True): one range over all n images; xmaps = min(nrow, n),
 *     ymaps = ceil(n / xmaps), out [ymaps (H + padding) + padding][xmaps (W + padding) + padding][3], image k at row
 *     (k / xmaps)(H + padding) + padding, column (k % xmaps)(W + padding) + padding, padding and empty cells 0;
 *     n == 1: the image alone, H x W.
 *   out: 4-byte aligned, with room for its byte count (fmri_images_u8_out_bytes; < 0: bad geometry) rounded up to a
 *   multiple of 4: the output is written as dwords, the up to three bytes behind its end as 0.
 *   slot_dev (device int64, or NULL: out as is): the output goes to out + (slot_dev[0] mod slot_mod) * slot_stride,
 *   the counter read ON THE DEVICE by the launch (slot_stride a multiple of 4) -- a ring whose slot follows a device
 *   counter such as fmri_trainlog_append's, in enqueue order.  present_dev (may be NULL): present_dev[slot] = 1
 *   (slot 0 without slot_dev).
 *   Two launches: one block per image writes its [lo, hi] to ws (fmri_images_u8_ws_bytes(n) bytes, 4-byte aligned;
 *   < 0: n < 1), one 16-byte load per pixel; the second is output-stationary, every lane decodes four consecutive
 *   bytes and issues one dword store, and in mode 1 every block folds the n ranges itself.  No atomics, no memset, no
 *   allocation, no host sync; the bytes are a function of the input and the geometry only (fmri_set_deterministic on
 *   or off).  A non-finite pixel gives unspecified bytes and moves no address.
 *   Errors, before anything is launched: Cp != 8 or C != 3: FMRI_E_UNSUPPORTED; a NULL or misaligned pointer, bad
 *   geometry, mode outside {0, 1}, slot_mod < 1 or a slot_stride that is no multiple of 4 with slot_dev:
 *   FMRI_E_BADARG; ws_bytes too small: FMRI_E_WORKSPACE; an output of 2^31 bytes or more: FMRI_E_UNSUPPORTED.
 * fmri_images_u8_open: one thread.  Unless opened_dev[0] == slot_dev[0] + 1 already: clears
 *   present_dev[k * present_stride + slot] for k < kinds, slot = slot_dev[0] mod slot_mod, and sets opened_dev[0] =
 *   slot_dev[0] + 1 -- the first call of a pass opens the slot, later calls of the same pass do nothing.  A ring's
 *   flags are cleared by this launch, not by a host memset that a replay would not repeat. */
int64_t fmri_images_u8_ws_bytes(int n);
int64_t fmri_images_u8_out_bytes(int n, int H, int W, int mode, int R, int nrow, int padding);
int fmri_images_u8(const void* src16, int n, int H, int W, int C, int Cp,
                   int mode,              /* 0: one range per image (save_image of one image); 1: one range over all n, grid */
                   int R,                 /* mode 0: output side, nearest-neighbour resize H x W -> R x R; 0 = no resize */
                   int nrow, int padding, /* mode 1 */
                   void* ws, int64_t ws_bytes, uint8_t* out,
                   const int64_t* slot_dev, int64_t slot_stride, int slot_mod,   /* ring addressing; NULL: out as is */
                   uint8_t* present_dev,  /* may be NULL: set to 1 at the addressed slot */
                   void* stream);
int fmri_images_u8_open(const int64_t* slot_dev, int slot_mod, int64_t* opened_dev /* device int64 */,
                        uint8_t* present_dev, int64_t present_stride, int kinds, void* stream);

/* ---- layout casts ------------------------------------------------------------------------------- */
int fmri_nchw_to_nhwc(const float* src, void* dst, int N, int C, int HW, int Cp, void* stream);
int fmri_nhwc_to_nchw(const void* src, float* dst, int N, int C, int HW, int Cp, float scale, void* stream);
int fmri_rows_f32_to_f16(const float* src, void* dst, int M, int C, int Cp, float scale, void* stream);
int fmri_rows_f16_to_f32(const void* src, float* dst, int M, int C, int Cp, float scale, void* stream);
int fmri_reduce_slabs(const float* slabs, int nslabs, int64_t slab_stride, int M, int C, int ld, const float* bias,
                      int act, float* out32, int ld32, void* out16, int ld16, void* stream);
int fmri_permute_chw(const float* src, float* dst, int C, int HW, int to_engine, float scale, int accumulate,
                     void* stream);

/* ---- batch norm (train mode, momentum 0.9; models/vae_gan.py:21,54,81,108,158) -------------------- */
/* reductions write per-block partials to a caller workspace of fmri_bn_ws_floats(M, C) floats (any smaller
 * size >= 2*C also works, with fewer blocks) and fold them into sums2C = [sum a | sum b], 2*C floats. */
int64_t fmri_bn_ws_floats(int M, int C);
int fmri_bn_stats(const void* x, int M, int C, float* sums2C, float* ws, int64_t ws_floats, void* stream);
int fmri_bn_finalize(const float* sums2C, int C, float count, const float* gamma, const float* beta, float eps,
                     float momentum, int updates, float* running_mean, float* running_var, float* mean, float* rstd,
                     float* scale, float* shift, int64_t* num_batches_tracked /* += updates, may be NULL */,
                     void* stream);
/* fmri_bn_stats + fmri_bn_finalize in two launches instead of three (the fold of the partial sums finalizes): the
 * forward of nn.BatchNorm2d/1d in train mode when no statistics are exchanged between ranks (models/vae_gan.py:21). */
int fmri_bn_stats_finalize(const void* x, int M, int C, float* sums2C, float* ws, int64_t ws_floats, float count,
                           const float* gamma, const float* beta, float eps, float momentum, int updates,
                           float* running_mean, float* running_var, float* mean, float* rstd, float* scale,
                           float* shift, int64_t* num_batches_tracked, void* stream);
/* BatchNorm over FEW rows in ONE launch per direction (the BatchNorm1d layers behind the dense layers,
 * models/vae_gan.py:81,108,158,200: M = batch rows): a block owns 32 channels for all rows -- statistics, finalize
 * (incl. the running statistics and num_batches_tracked, `updates` momentum updates), apply / the backward constants,
 * parameter gradients and dx.  fmri_bn_cols_fwd = fmri_bn_stats_finalize + fmri_bn_apply; fmri_bn_cols_bwd (nstreams 1
 * or 2 cotangent streams stacked along the rows, sums [nstreams][2][C], dbeta / dgamma += gscale * sums of stream
 * param_stream, may be NULL) = fmri_bn_bwd_reduce(2) + fmri_bn_bwd_apply(2).  Fixed summation order. */
int fmri_bn_cols_fwd(const void* x, void* y, int M, int C, float count, const float* gamma, const float* beta, float eps,
                     float momentum, int updates, float* running_mean, float* running_var, float* mean, float* rstd,
                     float* scale, float* shift, float* sums2C, int64_t* num_batches_tracked, int relu, void* stream);
/* fmri_bn_cols_fwd / fmri_bn_finalize for rows stored range-scaled, x_stored = (*in_scale) * x with *in_scale a power of
 * two (the latent batch behind fmri_latent_fwd_ranged; in_scale NULL = 1): eps is scaled by s^2, so the output equals
 * BatchNorm(x); mean / rstd / scale / shift describe the STORED rows (what the apply and backward kernels read) and the
 * running statistics receive mean / s and var / s^2 -- nn.BatchNorm1d behind `Decoder.fc` (models/vae_gan.py:107-109). */
int fmri_bn_cols_fwd_s(const void* x, void* y, int M, int C, float count, const float* gamma, const float* beta, float eps,
                       float momentum, int updates, float* running_mean, float* running_var, float* mean, float* rstd,
                       float* scale, float* shift, float* sums2C, int64_t* num_batches_tracked, int relu,
                       const float* in_scale, void* stream);
int fmri_bn_finalize_s(const float* sums2C, int C, float count, const float* gamma, const float* beta, float eps,
                       float momentum, int updates, float* running_mean, float* running_var, float* mean, float* rstd,
                       float* scale, float* shift, int64_t* num_batches_tracked, const float* in_scale, void* stream);
int fmri_bn_cols_bwd(const void* x, const void* dy, void* dx, int M, int C, int nstreams, float count, const float* mean,
                     const float* rstd, const float* gamma, const float* beta, int relu, float* sums, float* dbeta,
                     float* dgamma, float gscale, int param_stream, void* stream);
/* The statistics rows a contraction's epilogue wrote (fmri_igemm_ep: stat_part [rows][2][C] of ONE group) folded into
 * sums2C and finalized like fmri_bn_finalize; scratch: fmri_bn_fold_scratch_floats(C) floats (two-stage fold of long
 * row lists).  fmri_bn_fold only folds (data-parallel runs all-reduce sums2C before fmri_bn_finalize). */
int fmri_bn_fold_finalize(const float* stat_part, int rows, int C, float* scratch, float* sums2C, float count,
                          const float* gamma, const float* beta, float eps, float momentum, int updates,
                          float* running_mean, float* running_var, float* mean, float* rstd, float* scale, float* shift,
                          int64_t* num_batches_tracked, void* stream);
int fmri_bn_fold(const float* stat_part, int rows, int C, float* scratch, float* sums2C, void* stream);
int fmri_bn_fold_scratch_floats(int C);
/* BatchNorm-backward rows (fmri_epilogue.bn_x) of `groups` cotangent groups, stat_part [groups][rows_cap][2][C], folded
 * into sums [groups][2][C] = per group [sum g | sum g*xhat] (the sums4C layout of fmri_bn_bwd_apply2 for two groups);
 * dbeta / dgamma (may be NULL) += gscale * the sums of group param_group.  scratch: groups *
 * fmri_bn_fold_scratch_floats(C) floats. */
int fmri_bn_bwd_fold(const float* stat_part, int rows, int rows_cap, int C, int groups, float* scratch, float* sums,
                     float* dbeta, float* dgamma, float gscale, int param_group, void* stream);
int fmri_bn_apply(const void* x, void* y, int M, int C, const float* scale, const float* shift, int relu,
                  void* stream);
int fmri_bn_bwd_reduce(const void* x, const void* dy, int M, int C, const float* mean, const float* rstd,
                       const float* gamma, const float* beta, int relu, float* sums2C, float* ws,
                       int64_t ws_floats, float* dbeta /* += gscale * sums[0..C), may be NULL */,
                       float* dgamma /* += gscale * sums[C..2C), may be NULL */, float gscale, void* stream);
int fmri_bn_bwd_apply(const void* x, const void* dy, void* dx, int M, int C, float count, const float* mean,
                      const float* rstd, const float* gamma, const float* beta, int relu, const float* sums2C,
                      void* stream);
/* The same for TWO cotangent streams through one saved forward (the discriminator's logit and feature streams,
 * train/train_vgan_stage1.py:369-372 back-propagates both): dy2 / dx2 = [stream A rows | stream B rows], M rows each;
 * x, xhat and the ReLU mask are read / computed once.  sums4C = [A: sum g | A: sum g*xhat | B: sum g | B: sum g*xhat];
 * dbeta / dgamma (may be NULL) accumulate gscale * the sums of stream param_stream (0 = A, 1 = B); the workspace needs
 * 2 * fmri_bn_ws_floats. */
int fmri_bn_bwd_reduce2(const void* x, const void* dy2, int M, int C, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, int relu, float* sums4C, float* ws, int64_t ws_floats,
                        float* dbeta, float* dgamma, float gscale, int param_stream, void* stream);
int fmri_bn_bwd_apply2(const void* x, const void* dy2, void* dx2, int M, int C, float count, const float* mean,
                       const float* rstd, const float* gamma, const float* beta, int relu, const float* sums4C,
                       void* stream);
/* dpre = dy * act'(y) (ReLU / tanh); if colsum2C != NULL its first C floats receive the column sums of dpre and, with
 * dbias != NULL, dbias[c] += gscale * colsum[c] for c < dbias_n <= C (the bias gradient of the layer in front of the activation: autograd of
 * `nn.Conv2d(..., bias=True)` + Tanh, models/vae_gan.py:118-121) */
int fmri_act_bwd(const void* y, const void* dy, void* dpre, int M, int C, int act, float* colsum2C, float* ws,
                 int64_t ws_floats, float* dbias, int dbias_n, float gscale, void* stream);
/* dst[c] += scale * sum_{m < M} src[m*ld_row + c*ld_col], c < C; src fp16 (is_f16) or fp32.  Bias gradients of the dense
 * layers (column sums of the cotangent rows, what autograd's Linear backward reduces) in one launch, fixed-order sums. */
int fmri_colsum_acc(const void* src, int is_f16, int M, int C, int64_t ld_row, int64_t ld_col, float scale, float* dst,
                    void* stream);
/* The many-row form for contiguous fp16 rows [M][C], C % 8 == 0 (the bias gradient of discriminator.conv.0 over
 * 3B x 64 x 64 pixels): per-block partial sums in `ws` (fmri_bn_ws_floats(M, C) floats) + fold; sums2C receives
 * [sum x | sum x^2], dbias[c] += gscale * sum x[c] for c < dbias_n (dbias may be NULL). */
int fmri_colsum_rows(const void* x16, int M, int C, float* sums2C, float* ws, int64_t ws_floats, float* dbias,
                     int dbias_n, float gscale, void* stream);

/* ---- latent / losses (models/vae_gan.py:266-269, :302-320; train_vgan_stage1.py:368-404) ----------- */
int fmri_latent_fwd(const float* head, const float* eps, int B, int Z, int zp, void* z16, float* kl_rows,
                    float* kl_total, int sample, void* stream);
/* Range-safe `VaeGan.reparameterize` (models/vae_gan.py:266-269) for fp16 consumers: sigma = exp(0.5 logvar) leaves
 * fp16's range at logvar > 22.2, where the reference's fp32 arithmetic is still finite (it overflows at logvar > 88.7).
 *   phase & 1: z = eps * exp(0.5 logvar) + mu (sample) or mu -> z32 [B][Z] fp32, KL as fmri_latent_fwd,
 *              *zmax = max(*zmax, max |z|)   (the caller zeroes *zmax; data-parallel SyncBN runs all-reduce it with MAX)
 *   phase & 2: *zscale = s = the largest power of two <= 1 with s * (*zmax) <= cap (1 when *zmax <= cap or non-finite),
 *              z16 [B][zp] = fp16(s * z32), padding columns zero.
 * Consumers: the GEMM of `Decoder.fc` on z16, fmri_bn_cols_fwd_s / fmri_bn_finalize_s with in_scale = zscale; the data
 * gradient w.r.t. z is s times the one w.r.t. the stored rows, the weight gradient needs no correction.
 * fmri_rows_absmax: *zmax = max(*zmax, max |x|) for a caller-provided fp32 latent (then phase 2 with z32 = x). */
int fmri_latent_fwd_ranged(const float* head, const float* eps, int B, int Z, int zp, void* z16, float* kl_rows,
                           float* kl_total, int sample, float* z32, float* zmax, float* zscale, float cap, int phase,
                           void* stream);
int fmri_rows_absmax(const float* x, int64_t n, float* zmax, void* stream);
/* host only: the scale phase 2 derives from a batch maximum (the same function the kernel evaluates) */
float fmri_latent_range_scale(float zmax, float cap);
int fmri_latent_bwd(const float* head, const float* eps, const float* dz, int ldz, float dz_unscale, float kl_w,
                    const float* kl_dev, int B, int Z, float out_scale, void* dhead16, float* dhead32, int sample,
                    void* stream);
int fmri_feat_mse(const void* feat, int B, int F, float* mse_rows, float* mse_total, void* stream);
int fmri_pixel_sq(const void* x, const void* xt, int64_t npix, int C, int Cp, float* total, void* dxt, float gscale,
                  void* stream);
/* scal: float block, slots [0..2] += bce sums (orig, pred, sampled), [9] += sum (d bce / d logit)^2 */
int fmri_gan_head(const float* logit, int ldl, int B, float* prob, float* scal, void* stream);
/* fmri_gan_head / fmri_gan_head_bwd for a discriminator loss made of a subset of the three terms (bit 0 orig, 1 pred,
 * 2 sampled; 'dcgan' / 'vae': 5, train_vgan_stage1.py:375,382): slot [9] and the cotangent only see those parts. */
int fmri_gan_head_parts(const float* logit, int ldl, int B, float* prob, float* scal, int parts, void* stream);
int fmri_gan_head_bwd_parts(const float* logit, int ldl, int B, void* dlogit, int ldg, float gscale, const float* norm,
                            int parts, void* stream);
int fmri_wae_logloss(const float* logit, int ldl, int n, int one_minus, float w, float* total, float* prob,
                     void* dlogit, int ldg, float gscale, void* stream);
/* ---- MMD latent penalty with the inverse-multiquadratic kernel (the second WAE penalty of Tolstikhin et al., ICLR 2018;
 * the reference only has the adversarial one).  q: encoder latents [n][ldq], p: prior / target samples [n][ldp], fp32,
 * n >= 2 the GLOBAL batch, d = latent size (a multiple of 64, <= 1024, else FMRI_E_UNSUPPORTED); rows 16-byte aligned
 * (ldq, ldp multiples of 4).  Scales s (host array of 1..8 values; NULL -> {0.1, 0.2, 0.5, 1, 2, 5, 10}),
 * C_s = 2 d sigma2 s, k(a,b) = sum_s C_s / (C_s + |a-b|^2), kappa'(r) = -sum_s C_s / (C_s + r)^2:
 *     MMD_u = [ sum_{i!=j} k(p_i,p_j) + sum_{i!=j} k(q_i,q_j) ] / (n(n-1))  -  2/n^2 sum_{i,j} k(q_i,p_j)
 *     dMMD_u/dq_i = 4/(n(n-1)) sum_{j!=i} kappa'(r^qq_ij)(q_i-q_j)  -  4/n^2 sum_j kappa'(r^qp_ij)(q_i-p_j)
 * (the diagonal excluded by index; |a-b|^2 = |a|^2 + |b|^2 - 2 a.b from an fp32-input MFMA Gram tile, clamped at 0).
 * *total += w * MMD_u (total may be NULL); dq [n][ldd] fp32 = gscale * w * dMMD_u/dq (may be NULL: value only); p gets
 * no gradient.  ws: fmri_mmd_imq_ws_bytes(n, d) bytes of device workspace (< 0: unsupported geometry).  No atomics: the
 * column range is split over blocks whose partial sums a second pass adds in a fixed order, the statistic in fp64 --
 * two calls are bit-identical in either deterministic mode.  No allocation, no host sync: graph-capturable. */
int64_t fmri_mmd_imq_ws_bytes(int n, int d);
int fmri_mmd_imq(const float* q, int ldq, const float* p, int ldp, int n, int d, float sigma2, const float* scales,
                 int nscales, float w, float* total, float* dq, int ldd, float gscale, void* ws, int64_t ws_bytes,
                 void* stream);
/* ---- the WAE latent discriminator (models/vae_gan.py:499-529: Linear(z,H) ReLU [Linear(H,H) ReLU] x 3 Linear(H,1),
 * sigmoid left to fmri_wae_logloss) as one launch forward and one for the backward chain.  H = 512; Zp a multiple of
 * 64, 64 <= Zp <= 512 for fmri_mlp_fwd and 64 <= Zp <= 256 for fmri_mlp_bwd; anything else: FMRI_E_UNSUPPORTED, nothing
 * launched (use fmri_igemm layer by layer).  NULL w5[i] / hs4[i] / delta4[i], kp5[0] < Zp, kp5[i] / kpd4[i] < H, Z > Zp,
 * ldl < 1, M < 1: FMRI_E_BADARG.
 * fmri_mlp_fwd: z16 [M][Zp] fp16; w5[i] = layer i's packed fp16 weights in the forward orientation ([rows_pad][kp5[i]],
 *   row = output feature: what fmri_pack_weight produces for fmri_igemm), bias5[i] fp32 (may be NULL); hs4[i] receives
 *   the hidden activations h_{i+1} [M][H] fp16 (the backward pass needs them), logit [M] fp32 the pre-sigmoid output.
 *   hs4[i] and logit are written for rows [0, M) only: the four hs4 may be one [4][M][H] allocation.
 * fmri_mlp_bwd: dlogit16 [M][ldl] (column 0) -> delta4[i] = cotangent of the pre-activation of h_{i+1} ([M][H] fp16:
 *   the P operands of the layers' fmri_wgrad calls; written for rows [0, M) only, as is dz32), dbias5[i] += inv_scale *
 *   column sums (NULL dbias5 or entry: skip), dz32 [M][Z] fp32 = inv_scale * (delta1 . W0) (NULL: skip).  w4row = row 0
 *   of the output layer's forward-orientation matrix; wd4[i] = layer i's packed weights in the data-gradient
 *   orientation ([rows_pad][kpd4[i]], row = input feature); wd4[0] is read only when dz32 is given, and then its rows
 *   [0, Zp) are read whatever Z is: it must have at least Zp rows (only columns [0, Z) of the product
 *   are stored).  Replaces the autograd data path of
 *   train/train_wae_stage1.py:278-303.  Determinism: delta4 and dz32 are plain stores (bit-reproducible); the five
 *   dbias5 vectors are accumulated with fp32 atomics across the 32-row blocks, so their last bits depend on the
 *   arrival order of the blocks (run-to-run spread ~1e-7 relative; every other gradient of the engine is reduced in a
 *   fixed order). */
int fmri_mlp_fwd(const void* z16, int M, int Zp, int H, const void* const* w5, const int* kp5, const float* const* bias5,
                 void* const* hs4, float* logit, void* stream);
int fmri_mlp_bwd(const void* dlogit16, int ldl, int M, int Zp, int Z, int H, const void* const* hs4, const void* w4row,
                 const void* const* wd4, const int* kpd4, void* const* delta4, float* const* dbias5, float* dz32,
                 float inv_scale, void* stream);
/* scal slots: in [0..5] bce_o,bce_p,bce_s,kl,mse,nle and [9] dl2; out [6..8] loss_encoder/discriminator/decoder,
 * [10] nA = 1/rms(d bce/d logit), [11] nB = 1/rms(d mse/d feature), [12] nA/nB, [13] 1.0; flags = {train_dis, train_dec} */
int fmri_compose_gate(float* scal, int* flags, float batch, float nfeat, float lambda_mse, float equilibrium,
                      float margin, int gate_on, int force_dis, int force_dec, void* stream);
/* The same with the hyper-parameters on the DEVICE, hp4_dev = [lambda_mse, equilibrium, margin, beta] -- the values the
 * scripts decay every epoch (train_vgan_stage1.py:448-458); a step recorded into a HIP graph then follows the schedule --
 * and with the other loss compositions of train_vgan_stage1.py:359-388: mode 0 'vae-gan', 1 'beta-vae' (KL weight
 * beta / batch), 2 'dcgan' (pixel nle in place of the feature mse, discriminator loss bce_orig + bce_sampled), 3 'vae'
 * (dcgan's losses, decoder loss lambda * nle, train_dis starts False).  npix = reals per image (3*H*W).  Further
 * slots written: [16] nP = 1/rms(d nle/d x_tilde), [17] lambda*nA/nB, [18] 1 - lambda, [19] lambda*nA, [20] the factor
 * the decoder gradients carry (nP/lambda for 'vae', else nA), [21] the KL weight. */
int fmri_compose_gate_dev(float* scal, int* flags, float batch, float nfeat, float npix, const float* hp4_dev, int mode,
                          int gate_on, int force_dis, int force_dec, void* stream);
/* *counter_dev += 1 (the step count fmri_adam_dev derives its bias corrections from) */
int fmri_counter_inc(int* counter_dev, void* stream);
/* ---- counter-based random numbers (csrc/rng.hip; fmri_hip/rng.py) ---------------------------------------------------
 * What the reference draws on the host each batch -- `normal_()` in `reparameterize` (models/vae_gan.py), `randn` for z_p,
 * `0.5 * randn` for z_fake (train/train_wae_stage1.py:276) -- and the flip / shift draws of fmri_ingest_u8, made on the
 * device by Philox4x32-10 (Random123: multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten
 * rounds).  state: device int64[2] = [seed, offset], 8-byte aligned; key = (low, high 32 bits of seed); offset = Philox
 * blocks consumed so far, read on the DEVICE (a replayed HIP graph draws fresh numbers) and moved by fmri_rng_advance only.
 * Element e of a draw on stream id sid >= 0 is output word e % 4 of the block with counter
 *     (lo32(offset + e / 4), hi32(offset + e / 4), sid, 0).
 * Draws that share an offset must use different sids.  Enqueue-only, no allocation, no global state.
 *
 * fmri_rng_normal: out[r * ld + c] (fp32, r < rows, c < cols <= ld; columns >= cols are not touched) = scale * N(0, 1)
 *   for e = (row0 + r) * cols + c, row0 >= 0 the caller's first GLOBAL row: rank k of a data-parallel run passes
 *   row0 = k * rows and gets the rows the one-rank run at the global batch would have got.  Uniforms
 *   u = ((w >> 8) + 0.5) * 2^-24 in (0, 1); Box-Muller on (w0, w1) -> words 0, 1 and (w2, w3) -> words 2, 3:
 *   scale * sqrt(-2 ln u_a) * {cos, sin}(2 pi u_b), precise logf / log1pf / sincosf / sqrtf (the upper half of (0, 1) is
 *   evaluated through 1 - u, which fp32 holds exactly where it does not hold u).  |value| <= scale * sqrt(-2 ln 2^-25)
 *   ~ 5.89 * scale; max abs error against the real-valued map <= 1e-5 * scale.  rows * cols >= 2^31 or row0 > 2^40:
 *   FMRI_E_UNSUPPORTED.
 * fmri_rng_u32: out[i] (int32, i < n) = lo + (((uint64) w_i * (hi - lo + 1)) >> 32) in [lo, hi], w_i = word i % 4 of
 *   block i / 4 (lo = 0, hi = 1: flips; lo = -s, hi = s: shifts; lo = INT32_MIN, hi = INT32_MAX: the raw words).  A value's
 *   probability differs from 1 / (hi - lo + 1) by less than 2^-32, i.e. the relative bias is at most (hi - lo + 1) * 2^-32.
 *   n > 2^40: FMRI_E_UNSUPPORTED.
 * fmri_rng_advance: offset += nblocks (>= 0), one thread, a launch of its own behind the draws that share the offset
 *   (stream order keeps it behind their reads).  A draw of n elements from row0 = 0 consumes ceil(n / 4) blocks.
 * fmri_rng_u32_at: fmri_rng_u32 for the elements start .. start + n - 1 (start >= 0) of the same stream: out[i] is made
 *   from w_(start + i), word (start + i) % 4 of block (start + i) / 4.  Rank k of a data-parallel run passes start = k * n
 *   (flips) or 2 * k * n (shifts) and gets its slice of the one-rank draw at the global batch; start = 0 is fmri_rng_u32,
 *   bit for bit.  n or start > 2^40: FMRI_E_UNSUPPORTED. */
int fmri_rng_normal(const int64_t* state, float* out, int rows, int cols, int ld, int64_t row0, int sid, float scale,
                    void* stream);
int fmri_rng_u32(const int64_t* state, int32_t* out, int64_t n, int sid, int lo, int hi, void* stream);
int fmri_rng_advance(int64_t* state, int64_t nblocks, void* stream);
int fmri_rng_u32_at(const int64_t* state, int32_t* out, int64_t n, int64_t start, int sid, int lo, int hi,
                    void* stream);
/* ---- epoch sampler of a device-resident dataset (csrc/rng.hip; fmri_hip/feed.py) --------------------------------------
 * What `DataLoader(dataset, batch_size, shuffle=True)` does on the host for every batch of the reference's loops
 * (train/train_vgan_stage1.py:316 ff.): a fresh permutation of the N samples per epoch, B of them per step.  Here the
 * permutation is a keyed bijection evaluated per index on the device -- no buffer of N elements, no sort -- and the
 * position lives in device memory, so a step recorded into a HIP graph walks through whole epochs with no host work.
 *
 * pi(seed, epoch) on [0, N), 1 <= N < 2^31.  N = 1: pi(0) = 0.  Otherwise, with b = the bit length of N - 1,
 * k = ceil(b / 2) (1 .. 16), mask = 2^k - 1 (the domain 2^(2k) holds N and is below 4 N):
 *     x = i
 *     repeat:  L = x >> k,  R = x & mask
 *              for r = 0 .. 5:   f = output word 0 of Philox4x32-10 with key (lo32(seed), hi32(seed)) and counter
 *                                    ((r << 16) | R,  lo32(epoch),  16,  0x80000000 | hi32(epoch))
 *                                (L, R) = (R, L ^ (f & mask))
 *              x = (L << k) | R
 *     until x < N;   pi(i) = x
 * One pass of the loop body is a balanced Feistel network, a bijection of [0, 2^(2k)) whatever the round function is;
 * repeating it until the value falls below N ("cycle walking") follows the cycle of that bijection through i back into
 * [0, N) and therefore restricts it to a bijection of [0, N) -- fewer than 4 passes on average.  The fourth counter word
 * has its top bit set: fmri_rng_normal / fmri_rng_u32 always have 0 there, so no draw of theirs shares a block with the
 * sampler, whatever stream id a caller picks (16 is SID_PERM, kept apart from the steps' ids as well); epoch < 2^63.
 * Six rounds: with independent random round functions three rounds already make a Feistel network indistinguishable
 * from a random permutation for a reader of well under 2^(k/2) values and four do so for chosen inputs AND outputs
 * (Luby & Rackoff 1988), but an epoch reads the whole table, 2^(2k) values, where four rounds are known to show
 * (Patarin, "Generic attacks on Feistel schemes", 2001: order 2^k known values for four rounds, order 2^(2k) -- the
 * table itself -- from six on); two more rounds cost six instead of four Philox blocks per pass for B indices per
 * step -- a few hundred blocks where one noise draw takes thousands.  pi is a pure function of (seed, epoch, i, N).
 *
 * state: device int64[3] = [seed, epoch, cursor], 8-byte aligned, read on the device.
 * fmri_sampler_indices: idx_out[i] (int32, i < B) = pi(seed, epoch)((cursor + row0 + i) mod N).  row0 >= 0 is the
 *   caller's first row of the GLOBAL batch: rank k of W passes row0 = k * B and gets rows k * B .. of the one-rank batch
 *   of W * B.  row0 + B > N: FMRI_E_UNSUPPORTED.  Does not move the state.
 * fmri_sampler_advance: cursor += B_global; then, if fewer than B_global positions are left (N - cursor < B_global),
 *   epoch += 1 and cursor = 0.  One thread, a launch of its own behind the reads of the state (stream order), like
 *   fmri_rng_advance.  Drop-last: every batch has B_global samples and an epoch visits floor(N / B_global) * B_global
 *   DISTINCT samples; the N mod B_global positions at the end of the permutation are skipped in that epoch (another
 *   permutation, so other samples, in the next).  The reference's DataLoader (drop_last=False) runs a short last batch
 *   instead; a recorded step has a fixed batch size and cannot.  N < B_global: FMRI_E_UNSUPPORTED.
 * Both: enqueue-only, no allocation, no global state.  (seed, epoch, cursor) reproduces a run. */
int fmri_sampler_indices(const int64_t* state, int N, int B, int64_t row0, int32_t* idx_out, void* stream);
int fmri_sampler_advance(int64_t* state, int N, int B_global, void* stream);
/* ---- differentiable augmentation of the discriminator's inputs (csrc/diffaug.hip; fmri_hip/augment.py) -----------------
 * Zhao et al., "Differentiable Augmentation for Data-Efficient GAN Training" (NeurIPS 2020), policy colour + translation
 * + cutout: every image the discriminator sees, real or generated, goes through one random transform T_p, and the
 * generator's gradient is taken through it.  The reference has no counterpart; the contract is the formula below.
 *
 * Images: fp16 NHWC8 [N][H][W][8], square (H == W <= 128), real channels 0..2, 16-byte aligned.  table: fp32 [2B][8],
 * 16-byte aligned, one row p = [b, s, c, ty, tx, cy, cx, cut] per image (integers as exact floats).  Image i of the call
 * is image img0 + i (0 <= img0, img0 + N <= 3B) of the steps' [orig | pred | sampled] layout of B images each: orig b
 * and pred b use row b (they are compared feature by feature), sampled b uses row B + b.
 *
 * fmri_diffaug_fwd: dst = T_p(src), in this order on the values of the fp16 elements:
 *     u = x + b;   m = mean of u over the pixel's 3 channels,  v = (u - m) s + m;
 *     M = mean of v over the image's 3 H W real elements,      w = (v - M) c + M;
 *     o[y][x] = w[y + ty][x + tx] if that pixel lies inside the image, else 0;
 *     o[y][x] = 0 for y in rows and x in cols, rows = { clamp(cy - cut / 2 + i, 0, H - 1) : 0 <= i < cut } (integer
 *     division), cols likewise from cx; cut <= 0 cuts nothing;
 *     one rounding to fp16; lanes 3..7 of every output pixel are zeros.
 *   A stage whose parameter is neutral (b = 0, s = 1, c = 1) is skipped: the row [0,1,1,0,0,0,0,0] copies the real
 *   channels bit for bit.
 * fmri_diffaug_bwd: the adjoint of T_p's linear part on up to two cotangent streams of the same images in one launch
 *   (g_b / dst_b NULL: one):  mask g by the cutout window;  g1[y][x] = g[y - ty][x - tx] inside the image, else 0;
 *     g2 = c g1 + (1 - c) mean(g1 over the image's 3 H W elements);
 *     g3 = s g2 + (1 - s) (mean of g2 over the pixel's 3 channels);
 *   stored as fp16, finite values beyond +-65504 saturate (NaN stays NaN), lanes 3..7 zeros.
 * Both evaluate the colour stages and their sums in fp64 (the affine maps cancel near zero, where fp32 arithmetic misses
 * the fp16 rounding of the exact value by many ulps) and round once; sums run in a fixed order and there are no atomics:
 * the bits are a function of the inputs alone, with fmri_set_deterministic on or off.  src and dst may not overlap.
 * fmri_diffaug_params: table rows r < rows (fp32 [rows][8]) for the GLOBAL rows row0 + r of stream sid at the state's
 *   offset (fmri_rng_normal for the state; the offset is not moved; a row consumes 2 blocks).  With w0..w7 the elements
 *   8 (row0 + r) .. + 7 of the stream in the layout of fmri_rng_u32 and u(w) = (w >> 8) 2^-24:
 *     b = u(w0) - 0.5,  s = 2 u(w1),  c = u(w2) + 0.5                                   (policy_mask & 1: colour)
 *       (fp32 holds every value exactly but c from 1 on, where it is the fp32 sum rounded to nearest even)
 *     ty = -sh + ((w3 (2 sh + 1)) >> 32),  tx likewise from w4                          (policy_mask & 2: translation)
 *     cy = (w5 (H - cut mod 2 + 1)) >> 32,  cx likewise from w6,  column 7 = cut        (policy_mask & 4: cutout)
 *   w7 is unused; a policy that is off writes the neutral values of its columns (cut = 0).  Rank k of a data-parallel
 *   run passes row0 = k * B and gets its rows of the draw at the global batch.
 * Errors, before anything is launched or dereferenced: H != W or H > 128: FMRI_E_UNSUPPORTED; a NULL or misaligned
 * pointer, overlapping src / dst, N, H, B < 1, an image range outside [0, 3B), sh or cut outside [0, H], row0 < 0 or
 * > 2^40, sid < 0: FMRI_E_BADARG.  Enqueue-only, no allocation, no global state. */
int fmri_diffaug_params(const int64_t* state, float* table, int rows, int64_t row0, int sid, int H, int sh, int cut,
                        int policy_mask, void* stream);
int fmri_diffaug_fwd(const void* src16, void* dst16, int N, int H, int W, const float* table, int B, int img0,
                     void* stream);
int fmri_diffaug_bwd(const void* g_a, void* dst_a, const void* g_b, void* dst_b, int N, int H, int W, const float* table,
                     int B, int img0, void* stream);
/* ---- augmentation of the fMRI rows of the Stage-II / Stage-III steps (csrc/voxaug.hip; fmri_hip/voxaug.py) -------------
 * Trial noise, voxel dropout, a masked span of voxels (an "ROI") and gain jitter on the rows the cognitive encoder reads.
 * The reference has no counterpart; the contract is the formula below.  Batch row b, global row r = row0 + b (a rank k of
 * a data-parallel run passes row0 = k * B), voxel c < V, state [seed, offset] as for fmri_rng_normal:
 *
 *     y[b][c] = 0                                             if s_b <= c < s_b + L_b        (span mask)
 *             = 0                                             if dropped(b, c)
 *             = k_b * fma(sigma_b, n[r][c], g_b * x[b][c])    otherwise
 *
 *   in fp32 -- the product g x rounded, then the fma (left out where sigma_b == 0), then the product with k_b rounded --
 *   and then ONE rounding to fp16, the conversion of fmri_rows_f32_to_f16.  dst16 is fp16 [B][pad8(V)], columns V ..
 *   pad8(V) zero; dst32 (may be NULL) takes the fp32 value before that last rounding, [B][V].
 *   n[r][c]       element r V + c of stream sid_noise in the layout of fmri_rng_normal with cols = V: word (r V + c) % 4
 *                 of block offset + (r V + c) / 4, through the same Box-Muller -- bit for bit what
 *                 fmri_rng_normal(state, out, B, V, V, row0, sid_noise, 1) writes to out[b][c] at the same offset.
 *   dropped(b,c)  word (r V + c) % 4 of block offset + (r V + c) / 4 of stream sid_drop  <  (uint32)((double)p_b 2^32):
 *                 a comparison of integers.
 *   One step consumes (B_global V + 3) / 4 blocks, the two element streams alike.
 * table: fp32 [B][8], 16-byte aligned, row b = [g, sigma, p, k, s, L, 0, 0] (s, L integers as exact floats: V < 2^24).
 *   The neutral row [1, 0, 0, 1, 0, 0, 0, 0] gives bit for bit the rows of fmri_rows_f32_to_f16 at scale 1 (a negative
 *   zero included); a row with sigma == 0 / p == 0 evaluates no block of the noise / dropout stream.
 * fmri_voxaug_params: table rows b < rows from ONE Philox block per global row: block offset + row0 + b of stream
 *   sid_row, words w0 .. w3:
 *     the row is augmented iff prob >= 1 or w3 < (uint32)((double)prob 2^32); otherwise it is the neutral row;
 *     g = fma(gain, z0(w0, w1), 1), z0 the first Box-Muller output of the pair;  sigma and p as passed;
 *     k = 1 / (1 - p) in fp32 where rescale != 0 (inverted dropout), else 1 -- computed here, fmri_voxaug_apply reads it;
 *     s = (w2 (V - span_len + 1)) >> 32,  L = span_len.
 *   The offset is not moved; the row stream consumes B_global blocks.
 * Errors, before anything is launched or dereferenced: a NULL or misaligned pointer (state 8, table and dst16 16, src32
 * and dst32 4 bytes), dst32 overlapping src32, rows, B, V < 1, V >= 2^24, row0 < 0 or > 2^40, a negative stream id,
 * sid_noise == sid_drop, span_len outside [0, V], gain or sigma < 0, p outside [0, 1), prob outside [0, 1]:
 * FMRI_E_BADARG; B V > 2^31 - 1: FMRI_E_UNSUPPORTED.  Enqueue-only, no allocation, no global state. */
int fmri_voxaug_params(const int64_t* state, float* table, int rows, int64_t row0, int sid_row, int V, float gain,
                       float sigma, float p, int rescale, int span_len, float prob, void* stream);
int fmri_voxaug_apply(const float* src32, int V, int B, const float* table, const int64_t* state, int64_t row0,
                      int sid_noise, int sid_drop, void* dst16, float* dst32, void* stream);
/* starting cotangents of the two back-propagated streams, fp16, multiplied by gscale * (*norm) (norm: device float) */
int fmri_gan_head_bwd(const float* logit, int ldl, int B, void* dlogit, int ldg, float gscale, const float* norm,
                      void* stream);
int fmri_feat_mse_bwd(const void* feat, int B, int F, void* dfeat, float gscale, const float* norm, void* stream);
/* fmri_feat_mse / fmri_feat_mse_bwd for WIDE feature rows (the raw output of discriminator block 1 or 2, recon_level
 * 1 / 2: F = 131 072 / 65 536 at 64 px).  feat: fp16 [3B][F] (orig | pred | sampled rows), F a multiple of 8.  The unit of
 * work is a (row, column chunk) pair of fmri_feat_mse_wide_chunk() halves and the grid is sized from the device's CU
 * count, not from B.
 *   fmri_feat_mse_wide: per-chunk fp32 partial sums go to ws (>= fmri_feat_mse_wide_ws_floats(B, F) floats, caller-owned;
 *     FMRI_E_WORKSPACE if smaller) and are folded in index order by a one-block launch: mse_rows[b] (optional) = row
 *     sums, *mse_total (optional) += their sum.  No atomics: the bits are a function of (feat, B, F) alone, with
 *     fmri_set_deterministic on or off, whatever the grid.
 *   fmri_feat_mse_bwd_wide: dfeat rows [0, B) = +d, [B, 2B) = -d with d = fp16((f_o - f_p) * gscale * (*norm)) -- the
 *     bits fmri_feat_mse_bwd writes; rows [2B, 3B) are written (zeros) only if write_zero_rows, otherwise left untouched
 *     (a caller whose next kernel does not read them).
 * Enqueue-only, no allocation, no host sync. */
int fmri_feat_mse_wide_chunk(void);
int64_t fmri_feat_mse_wide_ws_floats(int B, int F);
int fmri_feat_mse_wide(const void* feat, int B, int F, float* mse_rows, float* mse_total, float* ws, int64_t ws_floats,
                       void* stream);
int fmri_feat_mse_bwd_wide(const void* feat, int B, int F, void* dfeat, float gscale, const float* norm,
                           int write_zero_rows, void* stream);
/* out = a * (*a_dev) * x + b * y   (fp16 tensors, fp32 math; y and a_dev may be NULL) */
int fmri_axpby_f16(const void* x, const void* y, void* out, int64_t n, float a, float b, const float* a_dev,
                   void* stream);

/* out = a * (*a_dev) * x + b * (*b_dev) * y */
int fmri_axpby2_f16(const void* x, const void* y, void* out, int64_t n, float a, float b, const float* a_dev,
                    const float* b_dev, void* stream);

/* device-side unit-RMS re-normalisation of an fp32 cotangent before an fp16 backward pass:
 *   fmri_sumsq : *acc += sum x^2 (all-reduce acc across ranks if data parallel)
 *   fmri_renorm: f = 1/sqrt(*sumsq/count); out16 = x*f*scale; *factor_out = (*factor_in)*f */
int fmri_sumsq(const float* x, int64_t n, float* acc, void* stream);
int fmri_renorm(const float* x, void* out16, int64_t n, float scale, const float* sumsq, float count,
                const float* factor_in, float* factor_out, void* stream);
/* The same with the sum of squares in double precision (8-byte aligned device double; zero_first: cleared by the launch
 * itself): the encoder cotangent of `VaeGan.loss`'s KL term (models/vae_gan.py:310) holds 0.5 * (exp(logvar) - 1), whose
 * square leaves fp32 at logvar > 44 while the reference's fp32 step is finite up to logvar 88 -- what the steps use. */
int fmri_sumsq_f64(const float* x, int64_t n, double* acc, int zero_first, void* stream);
int fmri_renorm_f64(const float* x, void* out16, int64_t n, float scale, const double* sumsq, float count,
                    const float* factor_in, float* factor_out, void* stream);

/* ---- optimizers over flat fp32 buffers (train_vgan_stage1.py:275-283; train_wae_stage1.py:221-224) ---
 * g_true = g * gscale / (*gdev) (gdev: device float or NULL), clamped to +-clamp if clamp > 0; the whole
 * update is skipped when flag != NULL and *flag == 0 (device-side equilibrium gate). */
int fmri_rmsprop(float* p, const float* g, float* sq, int64_t n, float lr, float alpha, float eps, float gscale,
                 const float* gdev, float clamp, const int* flag, void* stream);
int fmri_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps,
              float bc1, float bc2_sqrt, float gscale, const float* gdev, float clamp, const int* flag, void* stream);

/* The same updates with the learning rate (and Adam's step count, incremented with fmri_counter_inc BEFORE the call)
 * read from device memory: lr schedules (ExponentialLR / StepLR, train_vgan_stage1.py:448-450) and Adam's bias
 * correction then need no re-recording of a captured step. */
int fmri_rmsprop_dev(float* p, const float* g, float* sq, int64_t n, const float* lr_dev, float alpha, float eps,
                     float gscale, const float* gdev, float clamp, const int* flag, void* stream);
int fmri_adam_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev, float b1, float b2,
                  float eps, const int* t_dev, float gscale, const float* gdev, float clamp, const int* flag,
                  void* stream);

/* ---- one launch per sub-network between its weight gradients and its next forward pass (round 4) -----------------
 * What the reference does per parameter between `loss.backward()` and the next `model(x)` -- `.grad` accumulation,
 * `RMSprop.step()` (train_vgan_stage1.py:275-283, 425-432), and what the engine adds around it (slab sum and map of
 * a weight-gradient GEMM's output to the reference layout, the fp16 GEMM copy of the new weights) -- for EVERY
 * parameter of a sub-network in one launch, from a device-resident table:
 *   fmri_apply_entry_fill  fills one host-side row and returns the blocks it occupies (0: this tensor's layout map is
 *       not eligible -- keep fmri_unpack_grad / fmri_rmsprop_dev / fmri_pack_weight for the whole group; < 0: bad
 *       arguments).  flat_n > 0: a flat segment [w, w + flat_n) of 1-D parameters whose gradient `grad` the backward
 *       pass accumulated in place.  Otherwise: `gsrc` = packed gradient
 *       [nslabs][TA*A][ld] as fmri_wgrad wrote it, (sa, sta, sb, stb, A, TA, B, KW, py, px, step, TH, TW) the map of
 *       fmri_unpack_grad, `scale` its factor, `clear` != 0 to write zeros back over gsrc (outputs the weight-gradient
 *       kernel ADDS into), `pk` the fp16 [rows_pad][kpad] GEMM copy in gsrc's orientation or NULL.
 *   fmri_apply_batch  mode 1: w, sq <- RMSprop(w, sq, g * gscale / *gdev) exactly as fmri_rmsprop_dev (same operations,
 *       same order: bit-identical to the separate launches), skipped when *flag == 0; mode 0: gradients only, stored
 *       (not added) into `grad` in the reference layout; mode 2: zero the flat segments' `grad` (the start of a
 *       backward pass, instead of a memset of the whole gradient buffer); mode 3: as mode 1 with every gradient read
 *       from `grad` (reference layout, e.g. mode 0's result summed over the ranks by an all-reduce).
 *       gated != 0: the weight gradients behind gsrc were launched with fmri_wgrad_if under the same `flag` -- when it
 *       is 0 they added nothing and the `clear` pass is skipped as well. */
/* dst[c][r] = src[r][c] (fp16; r < R, c < C; leading dimensions multiples of 8, ld_dst >= R rounded up to 8; src holds
 * src_rows >= R rows, the rows from R on and the columns up to ld_src zero): the data-gradient orientation of a dense
 * layer's fp16 weight made from its forward orientation instead of a second pass over the fp32 master
 * (models/vae_gan.py:81,108,158,200: nn.Linear keeps ONE weight; the second GEMM layout is the engine's). */
int fmri_transpose_f16(const void* src, void* dst, int R, int C, int src_rows, int ld_src, int ld_dst, void* stream);
/* Batched form, one launch per sub-network from a device-resident table (fmri_transpose_entry_fill fills one host-side
 * row and returns the blocks it occupies, < 0 on bad arguments).  A row is one 2-D transpose: a dense weight's second
 * orientation, or ONE TAP of one output-parity class of a stride-2 transposed convolution's weight
 * (nn.Conv2d / nn.ConvTranspose2d keep one weight, models/vae_gan.py:18-20,46-53: the class blocks are the engine's):
 * `src` / `dst` point at the slices (16-byte aligned), `width` = source columns readable from `src` on to its row's end. */
int fmri_transpose_entry_bytes(void);
int fmri_transpose_entry_fill(void* host_entry, const void* src, void* dst, int R, int C, int src_rows, int width,
                              int ld_src, int ld_dst, int tile_begin);
int fmri_transpose_f16_batch(const void* table_dev, int n, int total_tiles, void* stream);
int fmri_apply_entry_bytes(void);
int fmri_apply_entry_fill(void* host_entry, const float* gsrc, float* w, float* sq, float* grad, void* pk, int64_t sa,
                          int64_t sta, int64_t sb, int64_t stb, int A, int TA, int B, int KW, int py, int px, int step,
                          int TH, int TW, int ld, int kpad, int nslabs, int64_t slab_stride, int clear, float scale,
                          int64_t flat_n, int tile_begin);
int fmri_apply_batch(const void* table_dev, int n, int total_tiles, int mode, const float* lr_dev, float alpha, float eps,
                     float gscale, const float* gdev, float clamp, const int* flag, int gated, void* stream);

/* ---- numerics monitor (opt-in; fmri_hip/monitor.py) ------------------------------------------------------------------
 * Statistics of one tensor segment.  Every field is order-independent or folded in a fixed order: two runs give the same
 * bits.  `sumsq` (double), `max`, `min` and `max_abs` cover the FINITE elements only (max = -inf, min = +inf, max_abs = 0
 * when there is none), `nonfinite` counts NaN / +-inf, `clamped` counts the elements that fminf(fmaxf(v, -clamp), clamp)
 * changes (0 when clamp <= 0), `written` is 1 once a statistics launch has filled the record (0: gated off / not run). */
typedef struct fmri_stat {
    double sumsq;
    float max, min, max_abs;
    int32_t nonfinite, clamped, written;
} fmri_stat;                                     /* 32 bytes */
/* One segment of fmri_tensor_stats: rows x cols fp32 values at x[r * ld + c], each taken as v = x * (scale / *div)
 * (div may be NULL: 1) -- the true-scale gradient of fmri_rmsprop_dev / fmri_adam_dev with scale = gscale, div = gdev.
 * `gate` (may be NULL): when *gate == 0 the segment is skipped and `out` is left as it is. */
typedef struct fmri_stat_seg {
    const float* x;
    int64_t rows, cols, ld;
    const float* div;
    const int* gate;
    fmri_stat* out;
    float scale, clamp;
} fmri_stat_seg;                                 /* 64 bytes */
#define FMRI_STAT_MAX_SEGS 8
#define FMRI_STAT_BLOCKS 256                     /* partial records per segment at most */
/* Up to FMRI_STAT_MAX_SEGS segments (host array, read before the call returns) in two launches: per-block partial records
 * into `ws` (fmri_tensor_stats_ws_bytes(nseg) bytes, 8-byte aligned), then a fixed-order fold into each segment's `out`. */
int fmri_tensor_stats_ws_bytes(int nseg);
int fmri_tensor_stats(const fmri_stat_seg* segs, int nseg, void* ws, void* stream);
/* fmri_apply_batch (modes 1 / 3) that also writes, per block, the statistics of the true-scale gradients it consumed
 * (before the clamp) and of the new weights: part[2 * b] = gradient, part[2 * b + 1] = weights, zero for a block that
 * updates nothing; `part` holds 2 * total_tiles records.  Same update, bit for bit.  fmri_stat_fold then folds the
 * records in a fixed order: out[0] <- the gradient records, out[1] <- the weight records, both only when `flag` is NULL
 * or *flag != 0. */
int fmri_apply_batch_stats(const void* table_dev, int n, int total_tiles, int mode, const float* lr_dev, float alpha,
                           float eps, float gscale, const float* gdev, float clamp, const int* flag, int gated,
                           fmri_stat* part, void* stream);
int fmri_stat_fold(const fmri_stat* part, int nrec, const int* flag, fmri_stat* out, void* stream);
/* fmri_bn_bwd_apply / fmri_bn_bwd_apply2 / fmri_bn_cols_bwd that also count, into cnt[0] and cnt[1] (caller-zeroed ints,
 * added to), the dx values the saturating fp16 store clipped to +-65504 and the NaN values it stored.  Same dx, bit for
 * bit; integer adds: deterministic. */
int fmri_bn_bwd_apply_cnt(const void* x, const void* dy, void* dx, int M, int C, float count, const float* mean,
                          const float* rstd, const float* gamma, const float* beta, int relu, const float* sums2C,
                          int* cnt, void* stream);
int fmri_bn_bwd_apply2_cnt(const void* x, const void* dy2, void* dx2, int M, int C, float count, const float* mean,
                           const float* rstd, const float* gamma, const float* beta, int relu, const float* sums4C,
                           int* cnt, void* stream);
int fmri_bn_cols_bwd_cnt(const void* x, const void* dy, void* dx, int M, int C, int nstreams, float count,
                         const float* mean, const float* rstd, const float* gamma, const float* beta, int relu,
                         float* sums, float* dbeta, float* dgamma, float gscale, int param_stream, int* cnt,
                         void* stream);

/* ---- epoch-end schedules and the per-step training log (csrc/schedule.hip; fmri_hip/schedule.py) -----------------------
 * What the reference's loops do around every step on the host -- the epoch-end block (train/train_vgan_stage1.py:447-458,
 * the same block in stages 2 / 3 and wae_vgan_stage1.py:456-467, `StepLR.step()` in train_wae_stage*.py) and the per-batch
 * loss log (train_vgan_stage1.py:391-394, 434-443) -- done on the device, where the epoch of a fed step lives
 * (fmri_sampler_advance), so that a step recorded into a HIP graph needs no host work at an epoch boundary.
 *
 * fmri_schedule: device-resident state, 8-byte aligned.  The values of epoch e are e iterations of
 *     lr[i] *= lr_gamma  where the NEW epoch index is a multiple of lr_step   (torch's chainable StepLR; ExponentialLR:
 *                                                                              lr_step = 1 -- a repeated product, not a power)
 *     margin *= decay_margin;  equilibrium *= decay_equilibrium;  if (margin > equilibrium) equilibrium = margin;
 *     lambda_mse *= decay_mse;  if (lambda_mse > 1) lambda_mse = 1;
 * from the base values, in double precision -- IEEE products, no contraction possible: the same doubles on the host and
 * on the device -- rounded to fp32 once, when handed to the kernels that read them. */
#define FMRI_SCHED_MAX_LR 4
typedef struct fmri_schedule {
    double lr_base[FMRI_SCHED_MAX_LR];           /* epoch-0 values */
    double margin_base, equilibrium_base, lambda_mse_base;
    double lr_gamma, decay_margin, decay_equilibrium, decay_mse;
    double lr[FMRI_SCHED_MAX_LR];                /* the values of epoch `applied_epoch` */
    double margin, equilibrium, lambda_mse;
    int64_t lr_step;                             /* >= 1 */
    int64_t applied_epoch;                       /* >= 0 */
} fmri_schedule;                                 /* 160 bytes */

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FMRI_HOST_DEVICE __host__ __device__
#else
#define FMRI_HOST_DEVICE
#endif
/* The arithmetic itself, shared by the kernel and the host entry point below (upper-case names: inline code of this
 * header, not symbols of the library).  FMRI_SCHEDULE_SEEK moves the state to `epoch` >= 0: nothing when it is there,
 * the difference iterated when it is behind, a restart from the base values when it is ahead (a feed set back to an
 * earlier epoch).  Its cost is linear in the number of epochs iterated. */
static inline FMRI_HOST_DEVICE void FMRI_SCHEDULE_RESTART(fmri_schedule* s) {
    for (int i = 0; i < FMRI_SCHED_MAX_LR; ++i) s->lr[i] = s->lr_base[i];
    s->margin = s->margin_base;
    s->equilibrium = s->equilibrium_base;
    s->lambda_mse = s->lambda_mse_base;
    s->applied_epoch = 0;
}
static inline FMRI_HOST_DEVICE void FMRI_SCHEDULE_EPOCH_END(fmri_schedule* s) {
    const int64_t e = s->applied_epoch + 1;
    if (e % s->lr_step == 0)
        for (int i = 0; i < FMRI_SCHED_MAX_LR; ++i) s->lr[i] *= s->lr_gamma;
    s->margin *= s->decay_margin;
    s->equilibrium *= s->decay_equilibrium;
    if (s->margin > s->equilibrium) s->equilibrium = s->margin;
    s->lambda_mse *= s->decay_mse;
    if (s->lambda_mse > 1.0) s->lambda_mse = 1.0;
    s->applied_epoch = e;
}
static inline FMRI_HOST_DEVICE void FMRI_SCHEDULE_SEEK(fmri_schedule* s, int64_t epoch) {
    if (epoch < s->applied_epoch) FMRI_SCHEDULE_RESTART(s);
    while (s->applied_epoch < epoch) FMRI_SCHEDULE_EPOCH_END(s);
}
/* host only: FMRI_SCHEDULE_SEEK on a schedule in HOST memory -- the function the kernel evaluates; out7 (may be NULL)
 * receives the fp32 roundings [lr[0..3], lambda_mse, equilibrium, margin].  lr_step < 1, epoch < 0: FMRI_E_BADARG. */
int fmri_schedule_seek_host(fmri_schedule* s, int64_t epoch, float* out7);
/* The first launch of a fed step, in front of the feed's draws (one thread): e = feed_state[1], the epoch of the batch
 * about to be drawn (feed_state: the [seed, epoch, cursor] of fmri_sampler_indices); with sched != NULL the schedule is
 * moved to e and its values are stored as fp32 to *lr_out[i] (each may be NULL: that optimizer is not scheduled) and
 * hp3_out[0..2] = [lambda_mse, equilibrium, margin] (the head of the hp4_dev of fmri_compose_gate_dev; may be NULL);
 * *epoch_out = e (may be NULL).  A negative e (never written by the sampler) is taken as 0; a schedule whose lr_step
 * is < 1 is left alone and nothing is stored.  sched and epoch_out both NULL: FMRI_E_BADARG. */
int fmri_epoch_begin(const int64_t* feed_state, fmri_schedule* sched, float* lr_out0, float* lr_out1, float* lr_out2,
                     float* lr_out3, float* hp3_out, int64_t* epoch_out, void* stream);
/* The last launch of a logged step (one wave): row (*counter mod capacity) of ring [capacity][K] fp32 receives the K
 * values at src_dev[k] (device array of K device addresses, K <= 64), read as kind_dev[k] = 0: fp32, 1: int32, 2: int64
 * (integers converted to fp32), then *counter += 1 (int64, 8-byte aligned, >= 0).  Plain stores, stream-ordered behind
 * the kernels that wrote the sources; no host sync. */
int fmri_trainlog_append(const void* const* src_dev, const int32_t* kind_dev, int K, float* ring, int64_t capacity,
                         int64_t* counter, void* stream);

/* ---- device-side training-state ring (csrc/state.hip; fmri_hip/state.py) --------------------------------------------
 * What `if not idx_epoch % 5: torch.save(model.state_dict(), ...)` of the scripts' epoch loops (train_vgan_stage1.py:596)
 * does on the host, for a step that runs from a recorded graph: ONE predicated launch that gathers every piece of
 * training state -- weights, BatchNorm statistics, optimizer state, generator and feed position, the log -- into a slot of
 * a device ring.  Whether the launch copies, and into which slot, is read on the device from the feed's state.
 *
 * A slot is a 64-byte header followed by the segments, each at a 16-byte boundary; a ring is `capacity` slots followed by
 * one more, the "manual" slot (index `capacity`).  The header, eight int64 written by one thread when a copy fires and read
 * by the host only: [FMRI_STATE_MAGIC, fingerprint, epoch, cursor, step, payload_bytes, 0, 0] -- epoch / cursor: the
 * feed's position at the launch, the position a resume continues from (-1 without a feed); step: *log_counter (-1
 * without one).
 *
 * One chunk (FMRI_STATE_CHUNK bytes of one segment) is what one 256-thread block moves: four 16-byte accesses per lane in
 * flight when the segment's live address is 16-byte aligned (plus a dword tail), dword by dword otherwise.  Nothing
 * outside a segment's bytes is written on either side.  Plain vector stores: no atomics, no memset, no allocation;
 * enqueue-only and capturable. */
#define FMRI_STATE_MAGIC 0x31544154534d4621ll    /* "!FMSTAT1" */
#define FMRI_STATE_HEADER 64
#define FMRI_STATE_CHUNK 16384
typedef struct fmri_state_seg {
    void* live;                                  /* device address of the tensor, a multiple of 4 */
    int64_t offset;                              /* of its bytes in a slot: a multiple of 16, >= FMRI_STATE_HEADER */
    int64_t bytes;                               /* a multiple of 4, >= 0 */
    int64_t chunk0;                              /* chunks of the segments in front of it (the prefix a block searches) */
} fmri_state_seg;                                /* 32 bytes */
/* host only: the slot layout of nseg segments of bytes[i] each -- offsets_out[i] (may be NULL) and, returned, the slot
 * size (a multiple of 16; 64 for nseg = 0).  nseg < 0, bytes NULL with nseg > 0, a negative byte count or one that is
 * not a multiple of 4: FMRI_E_BADARG (negative). */
int64_t fmri_state_layout(const int64_t* bytes, int nseg, int64_t* offsets_out);
/* The slot side's access policy of every later fmri_state_copy of the process: 1 non-temporal loads / stores (the
 * default; profiles/state_ring.md has the measurement it rests on), 0 plain ones; a negative value only asks.  Returns the
 * policy that was in force.  The live side is always plain: the next step reads those tensors. */
int fmri_state_nontemporal(int on);
/* segs_host: the table in host memory, checked here on every call -- live addresses multiples of 4, byte counts of 4,
 * offsets of 16, ascending and apart, inside a slot of slot_bytes, chunk0 the running chunk count -- and segs_dev its copy
 * in device memory, which the kernel reads.  ring: 16-byte aligned, ring_bytes >= (capacity + 1) * slot_bytes.
 * dir = 0 gathers live -> slot:
 *   feed_state != NULL (the [seed, epoch, cursor] of fmri_sampler_indices) and every >= 1: the launch copies only when
 *     cursor == 0, epoch >= 1 and (epoch - 1) % every == 0 -- the state at the end of epoch epoch - 1 where
 *     idx_epoch % every == 0 -- into slot ((epoch - 1) / every) % capacity (capacity >= 1).  Every block evaluates this
 *     from the same three words, which the launch does not write; when it is false every block returns at once and no
 *     byte of the ring changes.
 *   every == 0: unconditional, into the manual slot; feed_state (may be NULL) only fills the header's position.
 * dir = 1 scatters slot `capacity` -> live, unconditionally (feed_state must be NULL, every 0); the header is not read.
 * log_counter may be NULL.  Grid: min(chunks, 2048) blocks, grid-stride.  A table that fails the checks: FMRI_E_BADARG,
 * nothing is launched. */
int fmri_state_copy(const fmri_state_seg* segs_host, const fmri_state_seg* segs_dev, int nseg, void* ring,
                    int64_t ring_bytes, int64_t slot_bytes, int dir, const int64_t* feed_state, int every, int capacity,
                    uint64_t fingerprint, const int64_t* log_counter, void* stream);

/* ---- exponential moving average of the weights (csrc/ema.hip; fmri_hip/ema.py) -----------------------------------------
 * Averaged weights ("shadows") of a fused step, kept on the device: per step and per element, in fp32 and in this order,
 *     omd = 1.0f - d;  e = e + omd * (w - e)
 * with w the live value, e its shadow and d the step's decay, derived by every block of the launch from the same 16-byte
 * state block, which nothing in the launch writes (the step counter is advanced with fmri_counter_inc on &state->t,
 * behind the last update launch of a step):
 *     t < start:  d = 0 -- the shadow becomes a copy of the live value;
 *     otherwise:  s = t - start,  d = warmup ? min(decay, (float)((1.0 + s) / (10.0 + s))) : decay  (quotient in double).
 * A table lists the (live, shadow) pairs one launch covers; a chunk (FMRI_EMA_CHUNK floats of one segment) is what one
 * 256-thread block moves: four 16-byte accesses per lane and side in flight when both bases of the segment are 16-byte
 * aligned (plus a dword tail), dword by dword otherwise.  No byte outside [base, base + 4 n) of either side is touched.
 * Plain vector loads and stores: no atomics, no allocation; enqueue-only and capturable. */
#define FMRI_EMA_CHUNK 4096
typedef struct fmri_ema_seg {
    float* live;                                 /* device address of the tensor, a multiple of 4 */
    float* shadow;                               /* device address of its average, a multiple of 4 */
    int64_t n;                                   /* floats, >= 0 (0: the pointers are not looked at) */
    int64_t chunk0;                              /* chunks of the segments in front of it (the prefix a block searches) */
} fmri_ema_seg;                                  /* 32 bytes */
typedef struct fmri_ema_state {
    int32_t t;                                   /* steps averaged so far */
    int32_t start;                               /* steps t < start copy */
    float decay;                                 /* in [0, 1) */
    int32_t warmup;                              /* 0 / 1 */
} fmri_ema_state;                                /* 16 bytes */
/* host only: the decay d of step t, from the expression the kernel evaluates. */
float fmri_ema_decay_at(int32_t t, int32_t start, float decay, int32_t warmup);
/* One launch over all segments of the table.  segs_host: the table in host memory, checked here on every call -- n >= 0,
 * chunk0 the running chunk count, both addresses of a segment with n > 0 non-NULL multiples of 4 -- and segs_dev its copy
 * in device memory, which the kernel reads; state_dev: the fmri_ema_state in device memory, a multiple of 4.  Grid:
 * min(chunks, 2048) blocks, grid-stride; a table of empty segments launches nothing.  nseg < 0, a NULL table with
 * nseg > 0, a NULL state or a table that fails the checks: FMRI_E_BADARG, nothing is launched. */
int fmri_ema_update(const fmri_ema_seg* segs_host, const fmri_ema_seg* segs_dev, int nseg,
                    const fmri_ema_state* state_dev, void* stream);
/* live <-> shadow of every segment, moved as 32-bit words: bit for bit, NaN payloads included.  Checks as above. */
int fmri_ema_swap(const fmri_ema_seg* segs_host, const fmri_ema_seg* segs_dev, int nseg, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FMRI_HIP_H */
