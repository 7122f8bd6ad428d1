/*
 * adp_enc.h -- extension of adp.h: what the mel encoder (audio_diffusion_pytorch_amd/encoders.py, MelE1d) needs beyond the
 * conv families of adp.h.  Exported by the same libadp_hip.so.
 *
 *   down = Conv1d(R, M, kernel 2f + 1, stride f, padding f)          [B, R, L] -> [B, M, N],  N = (L - 1) / f + 1
 *
 * the overlapping strided downsample (adp_conv1d takes kernel = stride only), with its data and weight gradients, and the
 * tanh of the bottleneck with its gradient.  f is 2, 3 or 4.
 *
 * Conventions are adp.h's: plain fp32 device pointers that need the alignment of a float only, contiguous [B, C, L]
 * tensors, int64 sizes, a hipStream_t passed as void*, 0 (ADP_OK) or a negative ADP_ERR_* code, no allocation, no
 * synchronisation, hipGraph-capturable.  fp32 in and out, fp32 accumulation on the exact-f32 matrix-core instruction.  The
 * three conv kernels read and write single floats (no 16-byte access, so no alignment case); the tanh kernels use 16-byte
 * accesses when every pointer of the call is 16-byte aligned and single floats otherwise.  Every load is predicated: a term
 * outside a tensor is a zero the kernel writes itself, never an out-of-bounds read.
 *
 * Non-finite inputs: reduction slots past the end of a sum (channel and frame tails of a tile) carry a zero in BOTH operands,
 * except in adp_enc_down_wgrad, where the frames behind a segment's end carry a zero output gradient against real input
 * samples of the same row: an Inf or NaN sample there can make a weight gradient NaN that torch would leave finite.
 *
 * Refusals (nothing is launched, nothing is written), checked in this order:
 *   ADP_ERR_NULL         a NULL pointer
 *   ADP_ERR_SHAPE        a size < 1; a size over the limits: B <= 65535, channels <= 2^20, L < 2^31, fewer than 2^31
 *                        elements per tensor
 *   ADP_ERR_UNSUPPORTED  f outside 2..4
 */
#ifndef ADP_ENC_H
#define ADP_ENC_H
#include "adp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* N = (L - 1) / f + 1 = ceil(L / f): ADP_ERR_SHAPE when L < 1, ADP_ERR_UNSUPPORTED when f is outside 2..4. */
int64_t adp_enc_down_out_len(int64_t L, int64_t f);

/* y[b, m, n] = bias[m] + sum_r sum_{k < 2f+1} w[m, r, k] x[b, r, n f + k - f], terms outside [0, L) are zero.
 * x [B, R, L], w [M, R, 2f+1], bias [M], y [B, M, N]. */
int adp_enc_down_fwd(const float* x, const float* w, const float* bias, int64_t B, int64_t R, int64_t M, int64_t L,
                     int64_t f, float* y, void* stream);

/* dx[b, r, l] = sum_m sum_k w[m, r, k] dy[b, m, (l + f - k) / f] over the k for which the division is exact and the index
 * lies in [0, N).  dy [B, M, N], w [M, R, 2f+1], dx [B, R, L]: every element is written. */
int adp_enc_down_dgrad(const float* dy, const float* w, int64_t B, int64_t R, int64_t M, int64_t L, int64_t f, float* dx,
                       void* stream);

/* dw[m, r, k] = sum_b sum_n dy[b, m, n] x[b, r, n f + k - f],  dbias[m] = sum_b sum_n dy[b, m, n].
 * x [B, R, L], dy [B, M, N], dw [M, R, 2f+1], dbias [M].  The (b, n) sum is cut into segments whose partials go through ws
 * (adp_enc_down_wgrad_ws_bytes) and are added by a second launch in increasing segment order; dbias is a fixed-order sum of
 * its own.  No atomics: dw and dbias are WRITTEN, never accumulated into, and bit-identical from call to call. */
int64_t adp_enc_down_wgrad_ws_bytes(int64_t B, int64_t R, int64_t M, int64_t L, int64_t f);
int adp_enc_down_wgrad(const float* x, const float* dy, int64_t B, int64_t R, int64_t M, int64_t L, int64_t f, float* dw,
                       float* dbias, float* ws, void* stream);

/* z[i] = tanh(h[i]) and dh[i] = dz[i] (1 - z[i]^2) for i < n; n < 2^31. */
int adp_enc_tanh_fwd(const float* h, int64_t n, float* z, void* stream);
int adp_enc_tanh_bwd(const float* z, const float* dz, int64_t n, float* dh, void* stream);

#ifdef __cplusplus
}
#endif
#endif
