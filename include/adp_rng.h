/*
 * adp_rng.h -- extension of adp.h: a counter-based normal generator whose seed and draw index live in a small DEVICE row,
 * and the VInpainter resample step that forms its noise from that row in registers.  Exported by the same libadp_hip.so.
 *
 * Generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011; the Random123
 * known-answer vectors).  Multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85.  One round,
 * with p0 = M0 * c0 and p1 = M1 * c2 (64-bit products):
 *
 *     (c0, c1, c2, c3) <- (hi(p1) ^ c1 ^ k0,  lo(p1),  hi(p0) ^ c3 ^ k1,  lo(p0))
 *
 * ten rounds; the key grows by the two increments after each of the first nine.
 *
 * Stream layout: elements are taken in groups of four.  rng4 = device [seed_lo, seed_hi, draw, 0] (four uint32; the last word
 * is reserved and not read).  Group g (a 64-bit index) of that row uses
 *
 *     counter (lo32(g), hi32(g), draw, 0)        key (seed_lo, seed_hi)
 *
 * and its four output words r0..r3 are words 4g .. 4g+3 of the stream (adp_philox_bits).  They become four normals by
 * Box-Muller on the pairs (r0, r1) and (r2, r3):
 *
 *     u = ((r >> 8) + 0.5) * 2^-24                         strictly inside (0, 1): no log(0)
 *     z_even = sqrt(-2 ln u_a) cos(2 pi u_b)               z_odd = sqrt(-2 ln u_a) sin(2 pi u_b)
 *
 * with the accurate logf, sqrtf and sincosf.  u_a has 25 significant bits, one more than a float holds: ln u_a is formed
 * as logf(h * 2^-25) + d / h, where h is the float nearest to the integer 2 (r >> 8) + 1 and d in {-1, 0, 1} is what the
 * rounding dropped (exact in integers), so that the radius keeps its accuracy where u_a is close to 1.  u_b is rounded to a
 * float.  Element 4g + k of a tensor is z_k; |z| <= sqrt(50 ln 2) = 5.89.  The values depend on the row alone -- not on n, on
 * the launch geometry or on the pointers' alignment.  The same row always gives the same values, on every backend.
 *
 * The kernels READ the row: a launch captured in a hipGraph follows whatever was copied into the row before the replay.
 *
 * Conventions are adp.h's: pointers need the alignment of their element type only (16-byte accesses are used where every
 * pointer of the call allows them, single elements otherwise: the same values either way), int64 sizes, a hipStream_t passed
 * as void*, 0 (ADP_OK) or a negative ADP_ERR_* code, no allocation, no synchronisation, no atomics, hipGraph-capturable.
 * Every load and store is predicated: n need not be a multiple of 4 and nothing outside the operands is touched.
 *
 * Refusals (nothing is launched, nothing is written), checked in this order:
 *   ADP_ERR_NULL   a NULL pointer
 *   ADP_ERR_SHAPE  n < 0  (n = 0 is ADP_OK and launches nothing)
 *   ADP_ERR_ALIGN  a uint32 or float pointer that is not 4-byte aligned
 */
#ifndef ADP_RNG_H
#define ADP_RNG_H
#include "adp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[i] = word i of the row's stream, i < n_words: the integer generator, testable exactly. */
int adp_philox_bits(const uint32_t* rng4, int64_t n_words, uint32_t* out, void* stream);

/* out[i] = normal i of the row's stream, i < n. */
int adp_randn(const uint32_t* rng4, int64_t n, float* out, void* stream);

/* adp_v_inpaint_step (adp.h) with noise[i] = normal i of the row's stream, formed in registers instead of read from memory:
 *   x_out[i] = mask[i] ? a1*source[i] + b1*z[i] : a1*(a0 x - b0 v) + b1*(b0 x + a0 v),   ab4 = device [a0, b0, a1, b1].
 * x_out may alias x: each element is read, then written, by the one lane that owns it. */
int adp_v_inpaint_step_rng(const float* x, const float* v, const float* source, const uint8_t* mask, const float* ab4,
                           const uint32_t* rng4, int64_t n, float* x_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
