/* C ABI of libfmri_hip.so, contrastive latent alignment (csrc/contrast.hip).  Part of the ABI of include/fmri_hip.h, which
 * includes this file: same conventions (device pointers, `stream` a hipStream_t, the fmri_err return codes).  fmri_hip/lib.py
 * derives the ctypes prototypes of these entry points from this file, as it does for fmri_hip.h. */
#ifndef FMRI_HIP_CONTRAST_H
#define FMRI_HIP_CONTRAST_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* ---- Contrastive latent alignment: the symmetric InfoNCE ("CLIP") loss between two paired latent batches, the
 * retrieval objective of the Stage-II / III steps (the reference has none).  q: the trained encoder's means [n][ldq],
 * t: the teacher's means [n][ldt], fp32, row i of q paired with row i of t; 2 <= n <= 4096 the GLOBAL batch, d = latent
 * size (a multiple of 64, <= 1024; else FMRI_E_UNSUPPORTED), 0.01 <= tau <= 1 (else FMRI_E_BADARG); rows 16-byte aligned
 * (ldq, ldt multiples of 4).  With a_i = q_i / |q_i|, b_j = t_j / |t_j|, s_ij = a_i . b_j / tau:
 *     L_row = (1/n) sum_i [ lse_j s_ij - s_ii ],   L_col = (1/n) sum_j [ lse_i s_ij - s_jj ]
 *     L = (L_row + L_col) / 2 if symmetric, else L_row
 *     G = dL/ds = ((P + Q) / 2 - I) / n if symmetric, else (P - I) / n    (P / Q: the row / column softmax of s)
 *     da_i = (1/tau) sum_j G_ij b_j,   dL/dq_i = (da_i - (a_i . da_i) a_i) / |q_i|
 * (s from an fp32-input MFMA Gram tile of the raw rows scaled by 1 / (|q_i| |t_j|), the cosine clamped to [-1, 1]).  A row
 * whose squared norm is 0 has a_i = 0 (b_j = 0): its logits are 0 and its dq_i = 0; nothing non-finite leaves the call
 * for finite inputs.
 * *total += w * L (total may be NULL); *top1 += (1/n) #{i : s_ii >= max_j s_ij} on the kernel's own fp32 logits (may be
 * NULL); dq [n][ldd] fp32 = gscale * w * dL/dq (may be NULL: values only, the second product is skipped); t gets no
 * gradient.  ws: fmri_latent_nce_ws_bytes(n, d) bytes of device workspace (< 0: unsupported geometry); it holds the
 * n x n logits between the log-sum-exp pass and the weight pass.  The log-sum-exps carry (max, sum) pairs per row and
 * column split, folded in index order (stable at tau = 0.01, where exp(s - 1/tau) underflows); the loss sum is fp64.  No
 * atomics, every partial written by one block: two calls are bit-identical in either deterministic mode.  No allocation,
 * no host sync: graph-capturable. */
int64_t fmri_latent_nce_ws_bytes(int n, int d);
int fmri_latent_nce(const float* q, int ldq, const float* t, int ldt, int n, int d, float tau, int symmetric, float w,
                    float* total, float* top1, float* dq, int ldd, float gscale, void* ws, int64_t ws_bytes,
                    void* stream);
#ifdef __cplusplus
}
#endif
#endif /* FMRI_HIP_CONTRAST_H */
