// The stochastic (DDIM-eta) v-sampler step (include/adp_sde.h): adp_clip_step's first-order update with a noise term whose
// values are formed in registers from a (seed, draw) row of the generator of include/adp_rng.h (csrc/philox.h).
//   adp_v_step_eta : x_out = a1 clip(a0 x - b0 v) + ce (b0 x + a0 v) + cz z,  2 reads, 1 write
// The shape is v_inpaint_rng_kernel's: one thread owns one group of four elements per pass -- one Philox call and two
// Box-Muller pairs -- in a grid-stride loop over the groups.  A row with cz == 0 skips the draw.  No LDS, no atomics, no
// cross-lane traffic; ordinary vector or single-element stores only.  The arithmetic of x0 and its clamps, the per-item
// scale of a group and the grid are csrc/sampler_update.h's, shared with clip.hip and rf.hip.
#include "adp_rt.h"
#include "adp.h"
#include "adp_sde.h"
#include "philox.h"
#include "sampler_update.h"

namespace {

using namespace philox;
using namespace upd;

// VEC: x, v and xo are 16-byte aligned.  CLIP_SCALE: element i takes scale[i / per]; a group may straddle items
// (item_values4).
template <int CLIP, bool VEC>
__global__ __launch_bounds__(256) void v_step_eta_kernel(const float* x, const float* v, const float* coef5,
                                                         const uint32_t* rng4, const float* scale, int64_t n, int64_t per,
                                                         float* xo) {
  const SdeCoef c{coef5[0], coef5[1], coef5[2], coef5[3], coef5[4]};
  const bool noisy = c.cz != 0.0f;  // (the same branch in every lane of the launch)
  RngRow r{0u, 0u, 0u};
  if (noisy && rng4) r = rng_row(rng4);
  const float nan = __uint_as_float(0x7FC00000u);
  const int64_t groups = rng_groups(n);
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t e = 4 * g;
    f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
    if (noisy) {
      if (rng4) {
        z = rng_normal4(r, g);
      } else {
        const f32x4 z_nan = {nan, nan, nan, nan};  // noise asked for without a row: loud, and nothing is dereferenced
        z = z_nan;
      }
    }
    float s[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (CLIP == CLIP_SCALE) item_values4(scale, e, n, per, s);
    if (VEC && e + 4 <= n) {
      const f32x4 xv = *(const f32x4*)(x + e), vv = *(const f32x4*)(v + e);
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        o[k] = sde_elem<CLIP>(c, s[k], clip_x0(c.a0, xv[k], c.b0, vv[k]), xv[k], vv[k], z[k], noisy);
      *(f32x4*)(xo + e) = o;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < n) {
          const float xv = x[e + k], vv = v[e + k];
          xo[e + k] = sde_elem<CLIP>(c, s[k], clip_x0(c.a0, xv, c.b0, vv), xv, vv, z[k], noisy);
        }
    }
  }
}

}  // namespace

extern "C" int adp_v_step_eta(const float* x, const float* v, const float* coef5, const uint32_t* rng4, int64_t clip,
                              const float* scale, int64_t rows, int64_t per, float* x_out, void* stream) {
  if (!x || !v || !coef5 || !x_out) return ADP_ERR_NULL;
  if (rows < 0 || per < 0 || (clip != 0 && clip != 1) || (clip == 0 && scale)) return ADP_ERR_SHAPE;
  if (count_overflows(rows, per)) return ADP_ERR_SHAPE;
  if (misaligned(x, 4) || misaligned(v, 4) || misaligned(coef5, 4) || misaligned(x_out, 4) ||
      (rng4 && misaligned(rng4, 4)) || (scale && misaligned(scale, 4)))
    return ADP_ERR_ALIGN;
  const int64_t n = rows * per;
  if (n == 0) return ADP_OK;
  const bool vec = !misaligned(x, 16) && !misaligned(v, 16) && !misaligned(x_out, 16);
  with_clip(clip, scale, [&](auto CLIP) {
    with_flag(vec, [&](auto VEC) {
      ADP_LAUNCH((v_step_eta_kernel<CLIP(), VEC()>), dim3(grid4(n)), dim3(256), stream, x, v, coef5, rng4, scale, n, per,
                 x_out);
    });
  });
  return ADP_LAUNCH_OK();
}
