/*
 * adp_sde.h -- extension of adp.h: the stochastic (DDIM-eta) v-sampler step, whose noise is formed in registers from a
 * (seed, draw) row of adp_rng.h's generator.  Exported by the same libadp_hip.so.
 *
 * Contract.  A batch of `rows` items of `per` float values each, items contiguous, n = rows * per elements.  With
 * coef5 = device [a0, b0, a1, ce, cz] (float32) and z[i] = normal i of the stream of rng4 (adp_rng.h: Philox4x32-10 on
 * group g = i / 4, Box-Muller on the pairs of its words; bit-identical to what adp_randn writes for the same row):
 *
 *     x0  = a0 x - b0 v                eps = b0 x + a0 v                       (eps from the raw v)
 *     x0c = x0                                                  clip = 0
 *           clamp(x0, -s_r, s_r) / s_r,  r = i / per            clip = 1, scale given
 *           clamp(x0, -1, 1)                                    clip = 1, scale NULL
 *     x_out = a1 x0c + ce eps + cz z
 *
 * The host forms (ce, cz) for its eta; the kernel takes them as they are.  cz == 0 is the deterministic step: no noise is
 * formed and the words of rng4 are not read (rng4 may then be NULL).  A NULL rng4 under cz != 0 gives NaN in every element:
 * nothing is dereferenced.  x0 is formed by the rounding sequence of adp_clip.h, fma(a0, x, -(b0 * v)), so a scale that
 * adp_clip_scale selected from (x, v, coef5) is the quantile of exactly the values clamped here.  A NaN x0 or scale stays NaN.
 *
 * The kernels READ coef5 and rng4: a launch captured in a hipGraph follows whatever was copied into them before the replay.
 * x_out may alias x: each element is read, then written, by the one lane that owns it.
 *
 * Conventions are adp_rng.h's: pointers need the alignment of their element type only (16-byte accesses are used where
 * x, v and x_out all allow them, single elements otherwise: the same values either way), int64 sizes, a hipStream_t passed as
 * void*, 0 (ADP_OK) or a negative ADP_ERR_* code, no allocation, no synchronisation, no atomics, ordinary vector stores,
 * hipGraph-capturable.  Every load and store is predicated: n need not be a multiple of 4, a group of four elements may
 * straddle two items (scale is indexed per element), and nothing outside the operands is touched.  The values do not depend
 * on n, on the launch geometry or on the pointers' alignment.
 *
 * Refusals (nothing is launched, nothing is written), checked in this order:
 *   ADP_ERR_NULL   x, v, coef5 or x_out NULL  (scale may be NULL; rng4 as above)
 *   ADP_ERR_SHAPE  rows < 0, per < 0, rows * per beyond int64, clip not 0 or 1, a scale with clip = 0
 *                  (rows = 0 or per = 0 is ADP_OK and launches nothing)
 *   ADP_ERR_ALIGN  a pointer that is not 4-byte aligned
 */
#ifndef ADP_SDE_H
#define ADP_SDE_H
#include "adp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* coef5 = device [a0, b0, a1, ce, cz];  rng4 = the row of adp_rng.h;  z[i] = normal i of that row's stream.
 * clip = 0: x0c = x0 (scale must be NULL).  clip = 1: x0c = clamp(x0, -s_r, s_r) / s_r, or clamp(x0, -1, 1) where scale is NULL.
 * x_out may alias x.  A row with cz == 0 forms no noise and does not read rng4's words. */
int adp_v_step_eta(const float* x, const float* v, const float* coef5, const uint32_t* rng4, int64_t clip,
                   const float* scale, int64_t rows, int64_t per, float* x_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
