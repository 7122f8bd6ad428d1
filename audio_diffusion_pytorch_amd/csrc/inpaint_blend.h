// The arithmetic of one VInpainter resample for one element (diffusion.py:339-350), shared by adp_v_inpaint_step
// (elementwise.hip: the noise value is read from memory) and adp_v_inpaint_step_rng (rng.hip: it is formed in registers):
// rotate (x, v) from noise level i to level j, re-noise the source to level j, keep the source where the mask is set.
#pragma once
#include "adp_rt.h"

struct VInpaintCoef {
  float a0, b0, a1, b1;  // (a_i, b_i, a_j, b_j)
};

__device__ __forceinline__ float adp_v_inpaint_blend(const VInpaintCoef& c, float xv, float vv, float sv, float nz,
                                                     bool keep) {
  // The roundings are pinned, not left to contraction, which the compiler decides per call site: where no element keeps the
  // source the step must be adp_v_step's rotation bit for bit, in every kernel that inlines this.  v_step_kernel compiles
  // to one multiply-add per prediction and a plain product sum behind them; the emulator builds it with contraction off.
#pragma clang fp contract(off)
#ifdef ADP_EMULATE
  const float x_pred = c.a0 * xv - c.b0 * vv;
  const float n_pred = c.b0 * xv + c.a0 * vv;
#else
  const float x_pred = fmaf(c.a0, xv, -(c.b0 * vv));
  const float n_pred = fmaf(c.b0, xv, c.a0 * vv);
#endif
  const float xn = c.a1 * x_pred + c.b1 * n_pred;
  const float sn = c.a1 * sv + c.b1 * nz;
  return keep ? sn : xn;
}
