/*
 * adp_gated.h -- extension of adp.h: the gated feed-forward GEMM of the T5 v1.1 / flan-T5 text encoder
 * (audio_diffusion_pytorch_amd/text.py, T5GatedEncoder).  Exported by the same libadp_hip.so.  Forward only: the encoder is
 * frozen, nothing here has a gradient.
 *
 *   per block:  a = rmsnorm(h) ; f = gelu_new(a Wi0^T) * (a Wi1^T) ; h = h + f Wo^T
 *               (rmsnorm and the Wo product are adp_t5.h's; the middle step is the one call declared here)
 *
 * Conventions are adp_t5.h's: plain fp32 device pointers that need the alignment of a float only, contiguous row-major
 * tensors, int64 sizes, a hipStream_t passed as void*, 0 (ADP_OK) or a negative ADP_ERR_* code, no allocation, no
 * synchronisation, no atomics, bit-identical from call to call, hipGraph-capturable.  fp32 in and out, fp32 accumulation on
 * the exact-f32 matrix-core instruction (v_mfma_f32_32x32x2_f32).  Every access is a single element and every load is
 * predicated: a term outside a tensor (a tail in T, K or F) is a zero the kernel writes itself, never an out-of-bounds read.
 *
 * Refusals (nothing is launched, nothing is written), checked in this order:
 *   ADP_ERR_NULL         a NULL pointer (ws may be NULL when the size query below gives 0, which is known only after the
 *                        sizes passed: that one NULL is reported after ADP_ERR_SHAPE)
 *   ADP_ERR_SHAPE        a size < 1; a size over the limits: fewer than 2^31 elements per tensor (the workspace included),
 *                        at most 65535 * 64 tokens
 *   ADP_ERR_UNSUPPORTED  an act other than ADP_GATED_ACT_GELU_NEW
 */
#ifndef ADP_GATED_H
#define ADP_GATED_H
#include "adp.h"

/* gelu_new(g) = 0.5 g (1 + tanh(sqrt(2 / pi) (g + 0.044715 g^3))), evaluated in this form in fp32 with tanhf: finite for
 * every finite g, exactly 0 for a large negative g.  The only activation built; the argument exists so that another gate
 * can be added without a change of the interface. */
#define ADP_GATED_ACT_GELU_NEW 1

#ifdef __cplusplus
extern "C" {
#endif

/* y[t, f] = act(sum_k x[t, k] w_gate[f, k]) * (sum_k x[t, k] w_up[f, k]).  x [T, K], w_gate and w_up [F, K], y [T, F]; any
 * T, K, F >= 1.  y must not overlap x, w_gate, w_up or ws.  One kernel stages x once and forms both products; a workgroup owns
 * 64 tokens x 32 features.  When those tiles are too few to fill the chip, the k sum is cut into segments of whole 32-element
 * chunks (never for K <= 128), one workgroup each; the raw partial products of both operands go through ws (the kernel's own
 * scratch, of which only the size is public: 0 when the sum is not cut) and a second launch adds them in increasing segment
 * order and applies act to the complete gate sum only. */
int64_t adp_gated_linear_ws_bytes(int64_t T, int64_t K, int64_t F);
int adp_gated_linear(const float* x, const float* w_gate, const float* w_up, int64_t T, int64_t K, int64_t F, int64_t act,
                     float* y, float* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif
