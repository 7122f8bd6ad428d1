/*
 * adp_distill.h -- extension of adp.h: progressive distillation of a v-objective model (Salimans & Ho 2022): the
 * per-item linear combination that forms the teacher's mid point and the student's target, and the per-item weighted
 * squared error with its gradient.  Exported by the same libadp_hip.so.
 *
 * Contract.  A batch of `rows` items of `per` float values each, items contiguous, n = rows * per elements; r = i / per is
 * the item of element i.
 *
 *   adp_distill_comb, with coef = device [terms, rows] (planar: plane k holds one coefficient c_k per item):
 *
 *     out = c0_r x + c1_r p                     terms = 2 (q must be NULL)
 *     out = c0_r x + c1_r p + c2_r q            terms = 3
 *
 *   With phi = sigma pi / 2 a DDIM step of the v-objective is a rotation, x' = cos(d) x - sin(d) v for d = phi - phi'.
 *   Two teacher steps d1, d2 and the inversion of one student step D = d1 + d2 are both of this shape:
 *
 *     x_mid    = cos(d1) x_t - sin(d1) v1                                   (terms = 2, p = v1)
 *     v_target = c_x x_t + c_1 v1 + c_2 v2                                  (terms = 3, p = v1, q = v2)
 *     c_x = -sin(d1) sin(d2) / sin(D)    c_1 = cos(d2) sin(d1) / sin(D)    c_2 = sin(d2) / sin(D)
 *
 *   The coefficients are formed by the host in float64 and rounded once.  The rounding sequence is fixed:
 *   t = c0 * x ; t = fma(c1, p, t) ; out = fma(c2, q, t) -- three float32 roundings (two for terms = 2), and the
 *   two-term result is the three-term one's intermediate, bit for bit.  A NaN operand or coefficient stays NaN.
 *
 *   adp_distill_wmse_fwd, with w = device [rows] or NULL (every weight 1):
 *
 *     loss = (1 / n) sum_r w_r sum_e (v_pred - v_target)^2
 *
 *   Each lane accumulates s = fma(w_r d, d, s), d = v_pred - v_target, over the groups of four it owns, in element order;
 *   a block sums its lanes into one partial of the workspace, and one final block adds the partials in a fixed order in
 *   double: the same inputs give the same bits on every call, whatever the pointers' alignment, and w = NULL gives the bits
 *   of a w of ones.  The workspace holds adp_distill_wmse_ws_bytes(rows, per) bytes and needs no initialisation.
 *
 *   adp_distill_wmse_bwd, with gloss = device scalar or NULL (1):
 *
 *     dv = (gloss * 2 / n) * w_r * (v_pred - v_target)
 *
 *   formed as sc = gloss * 2 / (float)n once, then dv = (sc * w_r) * d.  dv may alias v_pred or v_target.
 *
 * The kernels READ coef, w and gloss: a launch captured in a hipGraph follows whatever was copied into them before the
 * replay.  adp_distill_comb's out may alias any of x, p, q: each element is read, then written, by the one lane that owns it.
 *
 * Conventions are adp_rf.h's: pointers need the alignment of their element type only (16-byte accesses are used where all
 * tensor operands of the call allow them, single elements otherwise: the same values either way), int64 sizes, a hipStream_t
 * passed as void*, 0 (ADP_OK) or a negative ADP_ERR_* code, no allocation, no synchronisation, no atomics, ordinary vector
 * stores, hipGraph-capturable.  Every load and store is predicated: n need not be a multiple of 4, a group of four elements
 * may straddle items, and nothing outside the operands is touched.
 *
 * Refusals (nothing is launched, nothing is written), checked in this order:
 *   ADP_ERR_NULL   adp_distill_comb: x, p, coef or out NULL; with terms = 3 also q NULL
 *                  adp_distill_wmse_fwd: v_pred, v_target, loss or ws NULL; adp_distill_wmse_bwd: v_pred, v_target or dv NULL
 *                  (w and gloss may be NULL)
 *   ADP_ERR_SHAPE  rows < 0, per < 0, rows * per beyond int64; adp_distill_comb: terms not 2 or 3, a q with terms = 2
 *                  (rows = 0 or per = 0 is ADP_OK and launches nothing: the loss is then not written)
 *   ADP_ERR_ALIGN  a pointer that is not 4-byte aligned
 * adp_distill_wmse_ws_bytes answers ADP_ERR_SHAPE for a refused shape.
 */
#ifndef ADP_DISTILL_H
#define ADP_DISTILL_H
#include "adp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out = c0_r x + c1_r p [+ c2_r q] ; coef = device [terms, rows], terms = 2 (q NULL) or 3.  out may alias x, p or q. */
int adp_distill_comb(const float* x, const float* p, const float* q, const float* coef, int64_t terms, int64_t rows,
                     int64_t per, float* out, void* stream);

/* bytes of the workspace adp_distill_wmse_fwd needs */
int64_t adp_distill_wmse_ws_bytes(int64_t rows, int64_t per);

/* loss = (1 / (rows * per)) sum_r w_r sum_e (v_pred - v_target)^2 ; w = device [rows] or NULL (ones).  Deterministic. */
int adp_distill_wmse_fwd(const float* v_pred, const float* v_target, const float* w, int64_t rows, int64_t per,
                         float* loss, float* ws, void* stream);

/* dv = gloss * 2 * w_r * (v_pred - v_target) / (rows * per) ; gloss = device scalar or NULL (1) ; w as above */
int adp_distill_wmse_bwd(const float* v_pred, const float* v_target, const float* w, const float* gloss, int64_t rows,
                         int64_t per, float* dv, void* stream);

#ifdef __cplusplus
}
#endif
#endif
