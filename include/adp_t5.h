/*
 * adp_t5.h -- extension of adp.h: the kernels of the frozen T5 text encoder (audio_diffusion_pytorch_amd/text.py, T5Encoder).
 * Exported by the same libadp_hip.so.  Forward only: the encoder is frozen, nothing here has a gradient.
 *
 *   h   = embed(ids)                                                        adp_t5_embed
 *   per block:  a = rmsnorm(h) ; qkv = a Wqkv^T ; o = attn(qkv) ; h = h + o Wo^T
 *               a = rmsnorm(h) ; f = relu(a Wi^T) ; h = h + f Wo2^T         adp_t5_rmsnorm, adp_t5_linear, adp_t5_attn
 *   out = rmsnorm(h)
 *
 * Conventions are adp_enc.h's: plain fp32 device pointers that need the alignment of a float only (ids: of an int64, bucket:
 * of an int32, mask: none), contiguous row-major tensors, int64 sizes, a hipStream_t passed as void*, 0 (ADP_OK) or a
 * negative ADP_ERR_* code, no allocation, no synchronisation, no atomics, bit-identical from call to call,
 * hipGraph-capturable.  fp32 in and out, fp32 accumulation; the matrix products run on the exact-f32 matrix-core instruction
 * (v_mfma_f32_32x32x2_f32).  Every access is a single element (no 16-byte access, so no alignment case) and every load is
 * predicated: a term outside a tensor is a zero the kernel writes itself, never an out-of-bounds read.
 *
 * Refusals (nothing is launched, nothing is written), checked in this order:
 *   ADP_ERR_NULL         a NULL pointer (res and mask may be NULL; ws may be NULL when adp_t5_linear_ws_bytes is 0, which
 *                        is known only after the sizes passed: that one NULL is reported after ADP_ERR_SHAPE)
 *   ADP_ERR_SHAPE        a size < 1; a size over the limits: fewer than 2^31 elements per tensor, B and H <= 65535
 *   ADP_ERR_UNSUPPORTED  adp_t5_attn: m > 512, dk not a multiple of 8 in [8, 128]
 */
#ifndef ADP_T5_H
#define ADP_T5_H
#include "adp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[t, :] = table[ids[t], :] for ids[t] in [0, V); an id outside that range writes a row of zeros and reads nothing.
 * ids int64 [T], table [V, d], out [T, d]. */
int adp_t5_embed(const int64_t* ids, const float* table, int64_t T, int64_t V, int64_t d, float* out, void* stream);

/* y[t, k] = x[t, k] * rsqrt(mean_k x[t, k]^2 + eps) * g[k]: no mean subtraction, no bias.  x [T, d], g [d], y [T, d]. */
int adp_t5_rmsnorm(const float* x, const float* g, int64_t T, int64_t d, float eps, float* y, void* stream);

/* y[t, n] = res[t, n] + act(sum_k x[t, k] w[n, k]),  act = max(., 0) when relu != 0, the identity otherwise; res NULL: no
 * residual term.  x [T, K], w [N, K], res [T, N], y [T, N]; res may be y itself (each element is read before it is written,
 * by the thread that writes it), x may not.  Any T, K, N >= 1.  When the 64 x 64 output tiles are too few to fill the chip,
 * the k sum is cut into segments of whole 32-element chunks, one workgroup each; their partials go through ws
 * (adp_t5_linear_ws_bytes, 0 when the sum is not cut) and a second launch adds them in increasing segment order. */
int64_t adp_t5_linear_ws_bytes(int64_t T, int64_t K, int64_t N);
int adp_t5_linear(const float* x, const float* w, const float* res, int64_t T, int64_t K, int64_t N, int64_t relu, float* y,
                  float* ws, void* stream);

/* Self-attention of one T5 block over the packed projections qkv [B, m, 3 H dk]: a token's row holds q (H dk values, head
 * major), then k, then v.  Per batch row b and head h, with q_i, k_j, v_j the dk-vectors of tokens i and j:
 *   S[i, j]  = q_i . k_j + rel_table[bucket[j - i + m - 1], h]      (no 1 / sqrt(dk): T5 folds it into its weights)
 *   S[i, j] += -FLT_MAX                                             where mask[b, j] == 0 (mask NULL: nowhere)
 *   P[i, :]  = softmax_j(S[i, :])  with the row maximum subtracted
 *   out[b, i, h dk : (h + 1) dk] = sum_j P[i, j] v_j
 * A masked key gets the weight 0 exactly; a row whose keys are all masked gets uniform weights.  rel_table [nb, H], bucket
 * int32 [2 m - 1] (a value outside [0, nb) contributes a bias of 0 and reads nothing), mask uint8 [B, m], out [B, m, H dk].
 * The keys are walked in tiles of 32 with a running maximum and sum (online softmax). */
int adp_t5_attn(const float* qkv, const float* rel_table, const int32_t* bucket, const uint8_t* mask, int64_t B, int64_t H,
                int64_t dk, int64_t m, int64_t nb, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
