/*
 * adp_edm.h -- extension of adp.h: Karras (EDM) diffusion, the preconditioned denoiser of Karras et al. 2022 on the
 * variance-exploding path x + sigma n: the fused noising of the training step and the sampler update.  Exported by the same
 * libadp_hip.so.
 *
 * Contract.  A batch of `rows` items of `per` float values each, items contiguous, n = rows * per elements.  With
 * sd = sigma_data and r = sqrt(sigma^2 + sd^2) the preconditioning is c_in = 1 / r, c_skip = sd^2 / r^2, c_out = sigma sd / r
 * and D = c_skip x + c_out F(c_in x, ln(sigma) / 4).  No entry point takes a logarithm: the caller forms ln(sigma) / 4.
 *
 *   adp_edm_noise, with sigma = device [rows] and s = sigma[i / per] for element i:
 *
 *     x_in   = c_in x + (c_in s) noise                      (what the net reads: unit variance for data of variance sd^2)
 *     target = (s / (sd r)) x - (sd / r) noise              (= (x - c_skip (x + s noise)) / c_out: the net's target)
 *
 *   The four per-item coefficients are formed in the kernel from s and sd, by correctly rounded float32 operations only
 *   (one product, one fused multiply-add, one square root, four divisions), in this sequence:
 *
 *     r = sqrt(fma(s, s, sd * sd))     c_in = 1 / r     c_n = s / r     t_x = c_n / sd     t_n = sd / r
 *     x_in = fma(c_in, x, c_n * noise)                  target = fma(t_x, x, -(t_n * noise))
 *
 *   Six float32 roundings on the longest path (sd * sd, the fused multiply-add, the square root, c_n, t_x and the closing
 *   multiply-add; the path through t_n * noise has six as well).  s = 0 gives x_in = x / sd and target = -noise
 *   (finite: nothing divides by s).  sigma_data is the float32 the call is given.
 *
 *   adp_edm_step, on the scaled state xs = c_in(sigma_i) x_i (what the net reads) and the net's output F, with
 *   coef8 = device [a0, b0, e0, f0, c1, d1, s1, cb] (float32), each entry formed by the host in float64 and rounded once,
 *   and z[i] = normal i of the stream of rng4 (adp_rng.h: Philox4x32-10 on group g = i / 4, Box-Muller on the pairs of its
 *   words; bit-identical to what adp_randn writes for the same row):
 *
 *     x0  = a0 xs - b0 F            a0 = sd^2 / r_i,     b0 = -sigma_i sd / r_i      (predicted data D)
 *     nh  = e0 xs + f0 F            e0 = sigma_i / r_i,  f0 = -sd / r_i              (predicted noise, always from the raw F)
 *     x0c = x0                                                  clip = 0
 *           clamp(x0, -s_r, s_r) / s_r,  r = i / per            clip = 1, scale given
 *           clamp(x0, -1, 1)                                    clip = 1, scale NULL
 *     xs_out = c1 x0c + d1 nh                                   order 1, and order 2 where cb == 0
 *              c1 x0c + d1 nh + cb (x0c - hist)   hist_out = x0c    order 2
 *              ... + s1 z                                       where s1 != 0
 *
 *   The host chooses c1 = g, d1 = g sigma_down, s1 = g sigma_up with g = c_in(sigma_{i+1}) (g = 1 on the last step, so a
 *   run ends unscaled); the kernel takes the row as it is.  The rounding sequence is fixed: x0 = fma(a0, xs, -(b0 * F)),
 *   which is adp_clip.h's, so a scale that adp_clip_scale selected from (xs, F, coef8) is the quantile of exactly the
 *   values clamped here; nh = fma(e0, xs, f0 * F); the division by s_r; xn = fma(c1, x0c, d1 * nh);
 *   xn = fma(cb, x0c - hist, xn); xs_out = fma(s1, z, xn).  Six float32 roundings on the longest path (b0 * F, x0,
 *   the division, xn and the two closing multiply-adds; four where cb == 0 and s1 == 0).  A NaN x0 or scale stays NaN.  Order 1 touches no history pointer.  An order-2 row with cb == 0 does
 *   not read hist (it still writes hist_out) and gives the bits of order 1: the first step of a run needs no initialised
 *   history.  s1 == 0 is the deterministic step: no noise is formed and the words of rng4 are not read (rng4 may then be
 *   NULL).  A NULL rng4 under s1 != 0 gives NaN in every element of xs_out: nothing is dereferenced.
 *
 * The kernels READ sigma, coef8 and rng4: a launch captured in a hipGraph follows whatever was copied into them before the
 * replay.  Every output may alias its input (x_in_out or target_out with x or noise; xs_out with xs; hist_out with hist):
 * each element is read, then written, by the one lane that owns it.
 *
 * Conventions are adp_rf.h's and adp_sde.h's: pointers need the alignment of their element type only (16-byte accesses are
 * used where all tensor operands of the call allow them, single elements otherwise: the same values either way), int64
 * sizes, a hipStream_t passed as void*, 0 (ADP_OK) or a negative ADP_ERR_* code, no allocation, no synchronisation, no
 * atomics, ordinary vector stores, hipGraph-capturable.  Every load and store is predicated: n need not be a multiple of 4,
 * a group of four elements may straddle items (sigma and scale are indexed per element), and nothing outside the operands
 * is touched.  The values do not depend on n, on the launch geometry or on the pointers' alignment.
 *
 * Refusals (nothing is launched, nothing is written), checked in this order:
 *   ADP_ERR_NULL   adp_edm_noise: x, noise, sigma, x_in_out or target_out NULL.
 *                  adp_edm_step: xs, f, coef8 or xs_out NULL; with order = 2 also hist or hist_out NULL  (scale may be
 *                  NULL; rng4 as above)
 *   ADP_ERR_SHAPE  rows < 0, per < 0, rows * per beyond int64; adp_edm_noise: sigma_data not > 0 (a NaN included);
 *                  adp_edm_step: order not 1 or 2, clip not 0 or 1, a scale with clip = 0  (rows = 0 or per = 0 is ADP_OK and
 *                  launches nothing)
 *   ADP_ERR_ALIGN  a pointer that is not 4-byte aligned (with order = 1 the history pointers are not looked at)
 */
#ifndef ADP_EDM_H
#define ADP_EDM_H
#include "adp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* x_in_out = c_in x + (c_in s) noise ; target_out = (s / (sd r)) x - (sd / r) noise ; sigma = device [rows], sd = sigma_data.
 * Outputs may alias inputs. */
int adp_edm_noise(const float* x, const float* noise, const float* sigma, float sigma_data, int64_t rows, int64_t per,
                  float* x_in_out, float* target_out, void* stream);

/* One sampler update on the scaled state; coef8 = device [a0, b0, e0, f0, c1, d1, s1, cb]; rng4 = the row of adp_rng.h.
 * clip = 0: x0c = x0 (scale must be NULL).  clip = 1: x0c = clamp(x0, -s_r, s_r) / s_r, or clamp(x0, -1, 1) where scale is NULL.
 * order 1: hist and hist_out are not touched.  order 2: hist_out <- x0c; a row with cb == 0 does not read hist.
 * A row with s1 == 0 forms no noise and does not read rng4's words.  xs_out may alias xs, hist_out may alias hist. */
int adp_edm_step(const float* xs, const float* f, const float* hist, const float* coef8, const uint32_t* rng4, int64_t order,
                 int64_t clip, const float* scale, int64_t rows, int64_t per, float* xs_out, float* hist_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
