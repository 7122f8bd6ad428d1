/*
 * adp_clip.h -- extension of adp.h: dynamic thresholding of a predicted clean signal (the reference's `clip`,
 * diffusion.py:36-54) and the v-sampler step that applies it.  Exported by the same libadp_hip.so.
 *
 * Contract.  A batch of `rows` items of `per` float values each, items contiguous.  For a threshold q in (0, 1] the scale of
 * item r is
 *
 *     s_r = max(quantile_q(|y_r|), min_scale)        y = x, or y = a0 x - b0 v when v is given (coef = device [a0, b0, ...])
 *
 * with torch.quantile's default (linear) rule.  The HOST forms the rank in float32, rank = float(q) * float(per - 1),
 * lo = floor(rank), w = rank - lo, and passes (lo, w); the kernels select the order statistics lo and hi = lo + (w > 0)
 * of |y_r| exactly and return lerp(sorted[lo], sorted[hi], w) by torch.lerp's formula
 * (w < 0.5 ? a + w (b - a) : b - (b - a)(1 - w)).  A row that holds a NaN gets a NaN scale.  per <= 2^24 (up to there
 * per - 1 is exact in float32; torch.quantile has the same limit).
 *
 * Selection: no sort.  The keys are the bit patterns of |y| (non-negative floats order like unsigned integers), 31 bits,
 * narrowed by three histogram passes over 11 + 10 + 10 bits.  A workgroup histograms its span of 4096 values of one row in
 * LDS and merges the non-empty bins into the row's histogram in the workspace with integer adds, so a result does not depend
 * on the order in which workgroups finish.  The bucket of a pass is chosen on the device, by every workgroup of the next
 * pass from the merged histogram (the host reads nothing).  lo and hi are adjacent ranks that may fall into different buckets
 * at any level: two prefixes are tracked, each with its own histogram once they differ.  y is never stored: every pass and
 * the step kernel form it from x and v by the same rounding sequence, y = fma(a0, x, -(b0 * v)).
 *
 * Launch sequence of adp_clip_scale: zero the workspace, pass 1, pass 2, pass 3, finalize (5 launches).  The workspace
 * needs no initialisation and nothing in it outlives the call; adp_clip_scale may be captured in a hipGraph and replayed
 * against the same workspace.
 *
 * Conventions are adp.h's: pointers need the alignment of their element type only (16-byte accesses where every pointer and
 * `per` allow them, single elements otherwise: the same values either way), int64 sizes, a hipStream_t passed as void*,
 * 0 (ADP_OK) or a negative ADP_ERR_* code, no allocation, no synchronisation, ordinary vector stores.  The only atomics are
 * the integer adds on the histograms.  Every load and store is predicated: nothing outside the operands is touched.
 *
 * Refusals (nothing is launched, nothing is written), checked in this order:
 *   ADP_ERR_NULL         a NULL pointer that the call needs (v may be NULL; coef only together with v; scale of
 *                        adp_clip_step may be NULL = static clamp to [-1, 1]; the history pointers only for order 1)
 *   ADP_ERR_SHAPE        rows < 0, per < 0, per > 2^24, lo outside [0, per), w outside [0, 1), w > 0 with lo = per - 1,
 *                        order not 1 or 2  (rows = 0 or per = 0 is ADP_OK and launches nothing)
 *   ADP_ERR_UNSUPPORTED  rows > 65535
 *   ADP_ERR_ALIGN        a pointer that is not 4-byte aligned
 */
#ifndef ADP_CLIP_H
#define ADP_CLIP_H
#include "adp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace adp_clip_scale needs for `rows` items of `per` values (host only; negative: an ADP_ERR_* code). */
int64_t adp_clip_ws_bytes(int64_t rows, int64_t per);

/* scale[r] = max(lerp(|y_r| sorted [lo], |y_r| sorted [lo + (w > 0)], w), min_scale), NaN where row r holds a NaN.
 * y = x where v is NULL (coef is not read), else y = a0 x - b0 v with coef = device [a0, b0, ...]. */
int adp_clip_scale(const float* x, const float* v, const float* coef, int64_t rows, int64_t per, int64_t lo, float w,
                   float min_scale, void* ws, float* scale, void* stream);

/* out = clamp(x, -s_r, s_r) / s_r per item (the reference's clip behind its quantile).  out may alias x. */
int adp_clip_apply(const float* x, const float* scale, int64_t rows, int64_t per, float* out, void* stream);

/* One thresholded v-sampler update.  x0 = a0 x - b0 v ; eps = b0 x + a0 v (from the raw v) ;
 * x0c = clamp(x0, -s_r, s_r) / s_r, or clamp(x0, -1, 1) where scale is NULL ;
 *   order 1: coef = device [a0, b0, a1, b1];          x_out = a1 x0c + b1 eps                       (history not touched)
 *   order 2: coef = device [a0, b0, a1, b1, ca, cb];  x_out = a1 x0c + b1 eps + ca (x0c - hist_x0) + cb (eps - hist_eps),
 *            history <- (x0c, eps); a row with ca = cb = 0 does not read the history.
 * Every output may alias its input: an element is read, then written, by the one lane that owns it. */
int adp_clip_step(const float* x, const float* v, const float* hist_x0, const float* hist_eps, const float* coef,
                  int64_t order, const float* scale, int64_t rows, int64_t per, float* x_out, float* hist_x0_out,
                  float* hist_eps_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
