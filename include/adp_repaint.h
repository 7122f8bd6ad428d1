/*
 * adp_repaint.h -- extension of adp.h: RePaint inpainting (Lugmayr et al. 2022) for the v-objective, rectified flow and
 * Karras (EDM) diffusion: one resample -- the objective's own first-order sampler update, the jump back to the noisier level
 * and the known region -- as one kernel behind the net.  Exported by the same libadp_hip.so.
 *
 * Contract.  A batch of `rows` items of `per` float values each, items contiguous, n = rows * per elements.  A level is
 * x_l = a_l x0 + b_l noise, with (a, b) = (cos, sin)(sigma pi / 2) for v, (1 - t, t) for rf and (1, sigma) for K.  Each entry
 * point reads one device row: the objective's step coefficients for (level i -> level i + 1), exactly as its sampler's table
 * holds them, then (A, S, P, Q), every entry formed by the host in float64 and rounded once:
 *
 *   adp_repaint_v_step   row8  = (a0, b0, a1, b1,                 A, S, P, Q)     the row of adp_v_step / adp_clip_step
 *   adp_repaint_rf_step  row10 = (a0, b0, c0, a1, c1, cb,         A, S, P, Q)     the row of adp_rf_step; cb is not read
 *   adp_repaint_k_step   row12 = (a0, b0, e0, f0, c1, d1, s1, cb, A, S, P, Q)     the row of adp_edm_step; s1, cb are not read
 *
 * With z[i] = normal i of the stream of rng4 (adp_rng.h: Philox4x32-10 on group g = i / 4, Box-Muller on the pairs of its
 * words; bit-identical to what adp_randn writes for the same row), per element:
 *
 *   y = the first-order deterministic update of (x, p) by the step coefficients, x0 clipped by (clip, scale) as there:
 *         v,  clip = 0:  adp_v_step's bits            v,  clip = 1:  adp_clip_step's (order 1)
 *         rf:            adp_rf_step's (order 1)      K:             adp_edm_step's (order 1, s1 = 0), on the scaled state
 *   y = fma(S, z, A * y)               where S != 0     (the jump back: the forward transition q(x_i | x_{i+1}))
 *       A * y                          where S == 0 and A != 1
 *       y                              where S == 0 and A == 1     (the last resample of a step: it moves on)
 *   k = fma(P, source, Q * z)          where Q != 0     (the known region at the level the resample ends on)
 *       P * source                     where Q == 0     (P = 1: the source itself, bit for bit)
 *   x_out = mask ? k : y               mask: one byte per element, nonzero keeps the source
 *
 * The jump and the known region share z: the two uses never meet in one element.  A group of four elements forms its
 * normals only if it needs one: S != 0, or Q != 0 and an element of the group keeps the source.  A row with S == 0 and
 * Q == 0 does not read the words of rng4 (rng4 may then be NULL).  A NULL rng4 where a normal is needed puts NaN in the place of z:
 * nothing is dereferenced.  A NaN x0 or scale stays NaN.  Two float32 roundings follow the step's own on the path of y, two make k.
 *
 * The host chooses, for a resample that jumps back to level j = i:  A = a_i / a_{i+1}, S = sqrt(b_i^2 - (A b_{i+1})^2),
 * P = a_i, Q = b_i; for one that moves on (j = i + 1): A = 1, S = 0, P = a_{i+1}, Q = b_{i+1}.  On K's scaled state the
 * scale factors fold in: A = c_in(sigma_i) / g with g the factor the step row applied, S = c_in(sigma_i) sqrt(sigma_i^2 -
 * sigma_{i+1}^2), P = c_in(sigma_j), Q = c_in(sigma_j) sigma_j, and P = 1, Q = 0 on the last row of a run, which ends
 * unscaled.  The kernel takes the row as it is.
 *
 * The kernel READS row, rng4 and scale: a launch captured in a hipGraph follows whatever was copied into them before the
 * replay.  x_out may alias x: each element is read, then written, by the one lane that owns it.
 *
 * Conventions are adp_rf.h's and adp_edm.h's: pointers need the alignment of their element type only (16-byte accesses are
 * used where x, p, source and x_out are 16-byte aligned and mask is 4-byte aligned, single elements otherwise: the same
 * values either way), int64 sizes, a hipStream_t passed as void*, 0 (ADP_OK) or a negative ADP_ERR_* code, no allocation, no
 * synchronisation, no atomics, ordinary vector stores, hipGraph-capturable.  Every load and store is predicated: n need not
 * be a multiple of 4, a group of four elements may straddle items (scale is indexed per element), and nothing outside the
 * operands is touched.  The values do not depend on n, on the launch geometry or on the pointers' alignment.
 *
 * Refusals (nothing is launched, nothing is written), checked in this order:
 *   ADP_ERR_NULL   x, p, source, mask, row or x_out NULL  (scale may be NULL; rng4 as above)
 *   ADP_ERR_SHAPE  rows < 0, per < 0, rows * per beyond int64, clip not 0 or 1, a scale with clip = 0  (rows = 0 or per = 0
 *                  is ADP_OK and launches nothing)
 *   ADP_ERR_ALIGN  a float or rng4 pointer that is not 4-byte aligned  (mask is bytes: any address)
 */
#ifndef ADP_REPAINT_H
#define ADP_REPAINT_H
#include "adp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One resample under the v-objective: x, the net's v, row8 = device [a0, b0, a1, b1, A, S, P, Q]; rng4 = the row of adp_rng.h.
 * clip = 0: x0c = x0 (scale must be NULL).  clip = 1: x0c = clamp(x0, -s_r, s_r) / s_r, or clamp(x0, -1, 1) where scale is NULL.
 * x_out may alias x. */
int adp_repaint_v_step(const float* x, const float* v, const float* source, const uint8_t* mask, const float* row8,
                       const uint32_t* rng4, int64_t clip, const float* scale, int64_t rows, int64_t per, float* x_out,
                       void* stream);

/* One resample under rectified flow: x, the net's u, row10 = device [a0, b0, c0, a1, c1, cb, A, S, P, Q].  clip, scale, rng4
 * and aliasing as above. */
int adp_repaint_rf_step(const float* x, const float* u, const float* source, const uint8_t* mask, const float* row10,
                        const uint32_t* rng4, int64_t clip, const float* scale, int64_t rows, int64_t per, float* x_out,
                        void* stream);

/* One resample under Karras (EDM) diffusion on the scaled state: xs, the net's F, row12 = device [a0, b0, e0, f0, c1, d1, s1,
 * cb, A, S, P, Q].  clip, scale, rng4 and aliasing as above. */
int adp_repaint_k_step(const float* xs, const float* f, const float* source, const uint8_t* mask, const float* row12,
                       const uint32_t* rng4, int64_t clip, const float* scale, int64_t rows, int64_t per, float* xs_out,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
