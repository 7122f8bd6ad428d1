/*
 * adp_spec.h -- extension of adp.h: the multi-resolution STFT loss of adp_stft_loss_* with row groups (stereo sum and
 * difference), an optional mel filterbank per resolution, and the FIR pre-filter that goes in front of it (spectral.py).
 * Exported by the same libadp_hip.so; implemented in csrc/spectral.hip on the FFT of csrc/stft_fft.h.
 *
 * Contract.  x and y are `rows` signals of `length` floats, rows contiguous.  Only x is differentiated.
 *
 *   pair = 0:  one group, the rows as they are.
 *   pair = 1:  rows is even, rows 2b and 2b + 1 are the two channels of item b.  Two groups of rows / 2 signals each:
 *              s_b = row(2b) + row(2b + 1) and d_b = row(2b) - row(2b + 1), formed where a kernel stages its span (two
 *              reads, one add or subtract); no sum or difference tensor exists in memory.  The same holds for y.
 *
 * Per group and resolution r = (N, hop, W) of `res` (host int64 triples, read at the call; N a power of two in [64, 4096],
 * 1 <= W <= N, hop >= 1, length > N / 2), with X and m = sqrt(max(|X|^2, eps)) exactly those of adp_stft_loss_fwd
 * (periodic Hann of length W centred in N, reflect padding N / 2, 1 + length / hop frames, N / 2 + 1 bins):
 *
 *   M = m                                    where n_bins[r] == 0 (or n_bins is NULL)
 *   M[j, t] = sum_k fb_r[j, k] m[k, t]       where n_bins[r] = J > 0: fb_r is float [J, N / 2 + 1], row-major, k increasing
 *   SC = ||M_y - M_x||_F / ||M_y||_F,  LM = mean |log M_x - log M_y|,  LIN = mean |M_x - M_y|     over the group's
 *        whole [signals, bins, frames] tensor
 *   value(group) = mean over r of (w_sc SC + w_log LM + w_lin LIN)
 *   loss = value(the group)                                         pair = 0
 *          (w_sum value(s) + w_diff value(d)) / 2                   pair = 1     (w_sum, w_diff are not read when pair = 0)
 *
 * `n_bins` is a host int64 array of nres entries (NULL: all zero), read at the call.  `fb` is a device array: the
 * filterbanks of the resolutions with n_bins[r] > 0, one behind the other in the order of `res`.  `mel_range` (device int32,
 * may be NULL) holds, in the same order, [J, 2] pairs [lo, hi): the bins a filter is walked over; a term outside is
 * skipped, so the range must hold every nonzero entry of the row (NULL: every bin).  `bin_range` (backward only; device
 * int32, may be NULL) holds per such resolution [N / 2 + 1, 2] pairs [lo, hi): the filters walked for a bin in the transposed
 * product.  Ranges are clamped to the valid indices.  A filter that is zero everywhere gives M = 0 and an infinite log: the
 * caller keeps such filterbanks out (spectral.py raises at construction).  n_bins[r] <= N / 2 - 1: the transposed
 * product's operand lives in LDS beside the magnitudes.
 *
 * Magnitudes never leave the chip: with a filterbank, the workgroup reads bins k and N - k of its transforms into
 * registers, and after a barrier the transform buffers hold the magnitudes the filter rows are walked over.
 *
 * adp_spec_loss_fwd writes loss[0] and keeps, in ws, the two norms per (group, resolution) that the backward reads.
 * adp_spec_loss_bwd writes dx (the shape of x) = gloss[0] * d loss / d x (gloss NULL: 1), the exact adjoint of the above;
 * with pair = 1 the last launch, which folds the reflect padding and sums the resolutions, also unmixes:
 * dx[2b] = g_s + g_d, dx[2b + 1] = g_s - g_d.  ws_fwd is the forward workspace of the same operands.
 *
 * With pair = 0 and no filterbank, loss and dx are those of adp_stft_loss_fwd / adp_stft_loss_bwd bit for bit.  x == y
 * gives loss 0.0 and dx all zero bit for bit.  No atomics; results are bit-identical from call to call.  gloss, fb and the
 * ranges are READ by the kernels: a launch captured in a hipGraph follows what they hold at the replay.
 *
 * adp_spec_fir: out[row, i] = sum_{j < ntaps} taps[j] * x[row, i + j - ntaps / 2], zeros outside [0, length), j increasing in
 * one chain of double-precision fused multiply-adds, rounded to float once (F.conv1d(row, taps, padding = ntaps / 2), a
 * cross-correlation, to within one rounding of the exact sum).  ntaps is odd, at most 255.
 * The adjoint with respect to x is the same call with the taps reversed.  One kernel: a workgroup stages 1024 outputs' span
 * (the run and ntaps - 1 halo samples) and the taps in LDS, with 16-byte loads where the row's offset allows and single
 * elements otherwise: the values do not depend on the pointers' alignment.  out must not overlap x.
 *
 * Conventions are adp.h's: pointers need the alignment of their element type only, int64 sizes, a hipStream_t passed as
 * void*, 0 (ADP_OK) or a negative ADP_ERR_* code, no allocation, no synchronisation, ordinary vector stores,
 * hipGraph-capturable; nothing outside the operands is touched.
 *
 * Refusals (nothing is launched, nothing is written), checked in this order:
 *   ADP_ERR_NULL         a NULL operand that is not optional (optional: n_bins, mel_range, bin_range, gloss; fb when no
 *                        resolution has a filterbank)
 *   ADP_ERR_SHAPE        rows < 1 or > 65535, length < 2 or >= 2^30, nres outside [1, 4], pair not 0 or 1, pair = 1 with
 *                        odd rows, length <= N / 2, n_bins[r] < 0;  fir: rows < 0, length < 0, ntaps even or outside
 *                        [1, 255], more than 2^31 - 1 workgroups  (fir with rows = 0 or length = 0 is ADP_OK, no launch)
 *   ADP_ERR_UNSUPPORTED  N not a power of two in [64, 4096], hop < 1, W outside [1, N], n_bins[r] > N / 2 - 1
 *   ADP_ERR_ALIGN        a float or int32 pointer that is not 4-byte aligned
 */
#ifndef ADP_SPEC_H
#define ADP_SPEC_H
#include "adp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the forward (backward = 0) or backward (backward = 1) workspace; host only, a negative ADP_ERR_* on refusal. */
int64_t adp_spec_loss_ws_bytes(int64_t rows, int64_t length, int64_t pair, int64_t nres, const int64_t* res,
                               const int64_t* n_bins, int64_t backward);

int adp_spec_loss_fwd(const float* x, const float* y, int64_t rows, int64_t length, int64_t pair, int64_t nres,
                      const int64_t* res, const int64_t* n_bins, const float* fb, const int32_t* mel_range, float w_sc,
                      float w_log, float w_lin, float eps, float w_sum, float w_diff, float* loss, float* ws, void* stream);

int adp_spec_loss_bwd(const float* x, const float* y, const float* gloss, const float* ws_fwd, int64_t rows, int64_t length,
                      int64_t pair, int64_t nres, const int64_t* res, const int64_t* n_bins, const float* fb,
                      const int32_t* mel_range, const int32_t* bin_range, float w_sc, float w_log, float w_lin, float eps,
                      float w_sum, float w_diff, float* dx, float* ws, void* stream);

/* out = the rows of x filtered by taps (device, ntaps floats); the adjoint is the call with reversed taps. */
int adp_spec_fir(const float* x, const float* taps, int64_t rows, int64_t length, int64_t ntaps, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
