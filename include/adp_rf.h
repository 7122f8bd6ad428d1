/*
 * adp_rf.h -- extension of adp.h: rectified flow (flow matching on the straight path between data and noise): the fused
 * noising of the training step and the sampler update.  Exported by the same libadp_hip.so.
 *
 * Contract.  A batch of `rows` items of `per` float values each, items contiguous, n = rows * per elements.  Time t lies in
 * [0, 1]; t = 1 is noise, t = 0 is data.
 *
 *   adp_rf_noise, with t = device [rows] and t_r = t[i / per] for element i:
 *
 *     x_t = (1 - t_r) x + t_r noise            u = noise - x
 *
 *   formed as x_t = fma(t_r, noise, fma(-t_r, x, x)) (two roundings; t_r = 0 returns x and t_r = 1 returns noise, bit for
 *   bit) and u = noise - x (one rounding).
 *
 *   adp_rf_step, with coef6 = device [a0, b0, c0, a1, c1, cb] (float32) = [1, t0, 1 - t0, t1, 1 - t1, cb] for a step from
 *   time t0 to time t1, each entry formed by the host in float64 and rounded once:
 *
 *     x0  = a0 x - b0 u                         (predicted data)
 *     eps = c0 u + x                            (predicted noise, always from the raw u)
 *     x0c = x0                                                  clip = 0
 *           clamp(x0, -s_r, s_r) / s_r,  r = i / per            clip = 1, scale given
 *           clamp(x0, -1, 1)                                    clip = 1, scale NULL
 *     w   = eps - x0c                           (the velocity actually used; u where nothing was clipped)
 *     x_out = c1 x0c + a1 eps                                   order 1, and order 2 where cb == 0
 *             c1 x0c + a1 eps + cb (w - hist)   hist_out = w    order 2
 *
 *   The rounding sequence is fixed: x0 = fma(a0, x, -(b0 * u)), which is adp_clip.h's, so a scale that adp_clip_scale
 *   selected from (x, u, coef6) is the quantile of exactly the values clamped here; eps = fma(c0, u, x); the division by
 *   s_r; w = eps - x0c; xn = fma(c1, x0c, a1 * eps); x_out = fma(cb, w - hist, xn).  Six float32 roundings on the longest
 *   path.  A NaN x0 or scale stays NaN.  Order 1 touches no history pointer.  An order-2 row with cb == 0 does not read
 *   hist (it still writes hist_out) and gives the bits of order 1: the first step of a run needs no initialised history.
 *
 * The kernels READ t and coef6: a launch captured in a hipGraph follows whatever was copied into them before the replay.
 * Every output may alias its input (x_t_out or u_out with x or noise; x_out with x; hist_out with hist): each element is
 * read, then written, by the one lane that owns it.
 *
 * Conventions are adp_sde.h's: pointers need the alignment of their element type only (16-byte accesses are used where
 * all tensor operands of the call allow them, single elements otherwise: the same values either way), int64 sizes, a
 * hipStream_t passed as void*, 0 (ADP_OK) or a negative ADP_ERR_* code, no allocation, no synchronisation, no atomics,
 * ordinary vector stores, hipGraph-capturable.  Every load and store is predicated: n need not be a multiple of 4, a group
 * of four elements may straddle items (t and scale are indexed per element), and nothing outside the operands is touched.
 * The values do not depend on n, on the launch geometry or on the pointers' alignment.
 *
 * Refusals (nothing is launched, nothing is written), checked in this order:
 *   ADP_ERR_NULL   adp_rf_noise: x, noise, t, x_t_out or u_out NULL.
 *                  adp_rf_step: x, u, coef6 or x_out NULL; with order = 2 also hist or hist_out NULL  (scale may be NULL)
 *   ADP_ERR_SHAPE  rows < 0, per < 0, rows * per beyond int64; adp_rf_step: order not 1 or 2, clip not 0 or 1, a scale
 *                  with clip = 0  (rows = 0 or per = 0 is ADP_OK and launches nothing)
 *   ADP_ERR_ALIGN  a pointer that is not 4-byte aligned (with order = 1 the history pointers are not looked at)
 */
#ifndef ADP_RF_H
#define ADP_RF_H
#include "adp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* x_t_out = (1 - t_r) x + t_r noise ; u_out = noise - x ; t = device [rows].  Outputs may alias inputs. */
int adp_rf_noise(const float* x, const float* noise, const float* t, int64_t rows, int64_t per, float* x_t_out,
                 float* u_out, void* stream);

/* One sampler update from time t0 to t1; coef6 = device [1, t0, 1 - t0, t1, 1 - t1, cb].
 * clip = 0: x0c = x0 (scale must be NULL).  clip = 1: x0c = clamp(x0, -s_r, s_r) / s_r, or clamp(x0, -1, 1) where scale is NULL.
 * order 1: hist and hist_out are not touched.  order 2: hist_out <- w; a row with cb == 0 does not read hist.
 * x_out may alias x, hist_out may alias hist. */
int adp_rf_step(const float* x, const float* u, const float* hist, const float* coef6, int64_t order, int64_t clip,
                const float* scale, int64_t rows, int64_t per, float* x_out, float* hist_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
