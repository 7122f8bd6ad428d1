// The stochastic (DDIM-eta) v-sampler step (include/adp_sde.h): adp_clip_step's first-order update with a noise term whose
// values are formed in registers from a (seed, draw) row of the generator of include/adp_rng.h (csrc/philox.h).
//   adp_v_step_eta : x_out = a1 clip(a0 x - b0 v) + ce (b0 x + a0 v) + cz z,  2 reads, 1 write
// A pass of csrc/sampler_update.h's for_groups4 with that header's draw; a row with cz == 0 skips the draw.  The arithmetic
// of x0 and its clamps is that header's too, shared with clip.hip and rf.hip.
#include "adp_rt.h"
#include "adp.h"
#include "adp_sde.h"
#include "philox.h"
#include "sampler_update.h"

namespace {

using namespace upd;

// VEC: x, v and xo are 16-byte aligned.  CLIP_SCALE: element i takes scale[i / per]; a group may straddle items
// (item_values4).
template <int CLIP, bool VEC>
__global__ __launch_bounds__(256) void v_step_eta_kernel(const float* x, const float* v, const float* coef5,
                                                         const uint32_t* rng4, const float* scale, int64_t n, int64_t per,
                                                         float* xo) {
  const SdeCoef c{coef5[0], coef5[1], coef5[2], coef5[3], coef5[4]};
  const bool noisy = c.cz != 0.0f;  // (the same branch in every lane of the launch)
  const Normals normals(rng4, noisy);
  const In in[] = {x, v};
  const Out out[] = {xo};
  struct Group {
    f32x4 z;
    float s[4];
  };
  for_groups4<VEC>(
      in, out, n,
      [&](int64_t g, int64_t e, bool) {
        Group gv{{0.0f, 0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f, 1.0f}};
        if (noisy) gv.z = normals(g);
        if (CLIP == CLIP_SCALE) item_values4(scale, e, n, per, gv.s);
        return gv;
      },
      [&](const Group& gv, int k, const float(&a)[2], float(&o)[1]) {
        o[0] = sde_elem<CLIP>(c, gv.s[k], clip_x0(c.a0, a[0], c.b0, a[1]), a[0], a[1], gv.z[k], noisy);
      });
}

}  // namespace

extern "C" int adp_v_step_eta(const float* x, const float* v, const float* coef5, const uint32_t* rng4, int64_t clip,
                              const float* scale, int64_t rows, int64_t per, float* x_out, void* stream) {
  const int64_t n = flat_count({x, v, coef5, x_out}, {rng4, scale}, rows, per, clip_ok(clip, scale));
  if (n <= 0) return (int)n;
  const bool vec = aligned16({x, v, x_out});
  with_clip(clip, scale, [&](auto CLIP) {
    with_flag(vec, [&](auto VEC) {
      ADP_LAUNCH((v_step_eta_kernel<CLIP(), VEC()>), dim3(grid4(n)), dim3(256), stream, x, v, coef5, rng4, scale, n, per,
                 x_out);
    });
  });
  return ADP_LAUNCH_OK();
}
