/*
 * adp_lt.h -- extension of adp.h: the two layers of the learned-transform front end (the reference's LTPlugin,
 * audio_diffusion_pytorch/components.py:113-159) and all their gradients.  Exported by the same libadp_hip.so.
 *
 *   encode = Conv1d(C, O, kernel K, stride s, padding p, padding_mode="reflect", bias=False)     [B, C, T] -> [B, O, L]
 *   decode = ConvTranspose1d(C, O, kernel K, stride s, padding p, bias=False)                    [B, C, L] -> [B, O, T]
 *
 * Both are dense over channels.  The two layers are each other's adjoints, so three kernels give the six operations:
 *
 *   operation                 entry point     mode              operands
 *   encode forward            adp_lt_conv     ADP_LT_REFLECT    x, encode weight [O, C, K]
 *   decode data gradient      adp_lt_conv     ADP_LT_ZERO       output gradient, decode weight [in, out, K] read as [O, C, K]
 *   decode forward            adp_lt_convt    ADP_LT_PLAIN      x, decode weight [C, O, K]
 *   encode data gradient      adp_lt_convt    ADP_LT_FOLD       output gradient, encode weight [out, in, K] read as [C, O, K]
 *   encode weight gradient    adp_lt_wgrad    ADP_LT_REFLECT    u = output gradient, v = layer input
 *   decode weight gradient    adp_lt_wgrad    ADP_LT_ZERO       u = layer input, v = output gradient ([in, out, K] result)
 *
 * Conventions are adp.h's: plain fp32 device pointers that need the alignment of a float only (16-byte accesses are
 * chosen by looking at the pointers and at the geometry), int64 sizes, a hipStream_t passed as void*, 0 (ADP_OK) or a
 * negative ADP_ERR_* code, no allocation, no synchronisation, hipGraph-capturable.  fp32 in and out, fp32 accumulation;
 * the tiled kernels run on the exact-f32 matrix-core instruction, and a per-output kernel takes every geometry whose
 * staged operands do not fit the tiled kernels' LDS plan (48 KiB for the signal segment: stride x (128 + K / stride) floats
 * per channel in adp_lt_conv) and every layer with fewer than 8 transform channels.
 *
 * Non-finite inputs: the tiled kernels mask reduction slots past the end of a sum (and the partial last tap group when K is
 * no multiple of stride) with a zero WEIGHT while the signal operand of the slot is a real sample of the same tile, so an Inf
 * or NaN sample can make neighbouring outputs of its tile NaN (0 * Inf) that torch would leave finite.  Finite inputs are
 * unaffected: the masked products are exact zeros.
 *
 * Refusals (nothing is launched, nothing is written):
 *   ADP_ERR_NULL         a NULL pointer
 *   ADP_ERR_SHAPE        a size < 1; an output length < 1; T <= pad with ADP_LT_REFLECT / ADP_LT_FOLD (a reflection needs
 *                        pad < T); adp_lt_convt's T that is not the layer's length (see there); a size over the limits:
 *                        B <= 65535, channels <= 65535, K and stride <= 65536, T and L < 2^31, fewer than 2^31 outputs
 *   ADP_ERR_UNSUPPORTED  pad < 0; an unknown mode
 */
#ifndef ADP_LT_H
#define ADP_LT_H
#include "adp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADP_LT_ZERO 0    /* adp_lt_conv / adp_lt_wgrad: the signal continues with zeros */
#define ADP_LT_REFLECT 1 /* ... with its mirror image, the edge sample not repeated (torch's "reflect") */
#define ADP_LT_PLAIN 0   /* adp_lt_convt: positions outside [0, T) are dropped */
#define ADP_LT_FOLD 1    /* ... are added to their mirror positions inside: the adjoint of ADP_LT_REFLECT */

/* L = (T + 2 pad - K) / stride + 1 of adp_lt_conv, and (L - 1) stride - 2 pad + K of adp_lt_convt; ADP_ERR_SHAPE when that
 * or an argument is not positive, ADP_ERR_UNSUPPORTED when pad < 0. */
int64_t adp_lt_conv_out_len(int64_t T, int64_t K, int64_t stride, int64_t pad);
int64_t adp_lt_convt_out_len(int64_t L, int64_t K, int64_t stride, int64_t pad);

/* y[n, o, l] = sum_c sum_k w[o, c, k] xp[n, c, l stride + k - pad],  xp = x continued as `mode` says (no padded copy exists:
 * the continuation is applied while a signal segment is staged in LDS).  x [B, C, T], w [O, C, K], y [B, O, L]. */
int adp_lt_conv(const float* x, const float* w, int64_t B, int64_t C, int64_t T, int64_t O, int64_t K, int64_t stride,
                int64_t pad, int64_t mode, float* y, void* stream);

/* out[n, o, t] = sum_c sum_j x[n, c, q - j] w[c, o, r + j stride],  t + pad = q stride + r.  x [B, C, L], w [C, O, K],
 * out [B, O, T].  ADP_LT_PLAIN: T must be adp_lt_convt_out_len(L, K, stride, pad).  ADP_LT_FOLD: T is the length of the
 * signal adp_lt_conv read, i.e. adp_lt_conv_out_len(T, K, stride, pad) must be L; the sums of the positions -pad..-1 and
 * T..T+pad-1 are added to positions pad..1 and T-2..T-1-pad (a second launch that owns those elements; no atomics). */
int adp_lt_convt(const float* x, const float* w, int64_t B, int64_t C, int64_t L, int64_t O, int64_t K, int64_t stride,
                 int64_t pad, int64_t mode, int64_t T, float* out, void* stream);

/* dw[a, b, k] = sum_n sum_l u[n, a, l] vp[n, b, l stride + k - pad].  u [B, A, L], v [B, Bc, T], dw [A, Bc, K];
 * L must be adp_lt_conv_out_len(T, K, stride, pad).  The (n, l) sum is cut into segments whose partials go through ws
 * (adp_lt_wgrad_ws_bytes) and are added by a second launch in increasing segment order: dw is WRITTEN, never accumulated
 * into, and bit-identical from call to call. */
int64_t adp_lt_wgrad_ws_bytes(int64_t B, int64_t A, int64_t Bc, int64_t L, int64_t K);
int adp_lt_wgrad(const float* u, const float* v, int64_t B, int64_t A, int64_t Bc, int64_t L, int64_t T, int64_t K,
                 int64_t stride, int64_t pad, int64_t mode, float* dw, float* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif
