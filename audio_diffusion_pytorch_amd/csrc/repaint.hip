// RePaint inpainting (include/adp_repaint.h): one resample of VRepainter / RFRepainter / KRepainter behind the net.
//   adp_repaint_{v,rf,k}_step : y = the objective's first-order update of (x, p) ; y = A y + S z (the jump back) ;
//                               x_out = mask ? P source + Q z : y                      3 reads + 1 byte, 1 write
// The pass of csrc/sampler_update.h's for_groups4, written out with the same guarantees (through for_groups4 the CLIP_SCALE
// forms need more scalar registers than there are) and kept in step with it by hand, with that header's draw, made only by the groups that need it.  A whole
// group also needs a 4-byte aligned mask, whose four bytes are then one word.  The three updates are that header's (the ones
// sde.hip, rf.hip and edm.hip launch) and inpaint_blend.h's rotation (adp_v_step's bits).
#include "adp_rt.h"
#include "adp.h"
#include "adp_repaint.h"
#include "inpaint_blend.h"
#include "philox.h"
#include "sampler_update.h"

namespace {

using namespace upd;

enum { OBJ_V = 0, OBJ_RF = 1, OBJ_K = 2 };

// The objective's step row (the first WORDS floats of `row`) and its first-order deterministic update of one element.
template <int OBJ>
struct Step;

template <>
struct Step<OBJ_V> {  // (a0, b0, a1, b1)
  static constexpr int WORDS = 4;
  float a0, b0, a1, b1;
  __device__ __forceinline__ explicit Step(const float* r) : a0(r[0]), b0(r[1]), a1(r[2]), b1(r[3]) {}
  // unclipped: adp_v_step's rotation (VSampler); clipped: adp_clip_step's first-order update (VThresholdSampler), which is
  // sde_elem with ce = b1 and no noise
  template <int CLIP>
  __device__ __forceinline__ float next(float s, float xv, float pv) const {
    if (CLIP == CLIP_NONE) return adp_v_inpaint_blend(VInpaintCoef{a0, b0, a1, b1}, xv, pv, 0.0f, 0.0f, false);
    return sde_elem<CLIP>(SdeCoef{a0, b0, a1, b1, 0.0f}, s, clip_x0(a0, xv, b0, pv), xv, pv, 0.0f, false);
  }
};

template <>
struct Step<OBJ_RF> {  // ops.rf_table's row; cb is not read (first order)
  static constexpr int WORDS = 6;
  RfCoef c;
  __device__ __forceinline__ explicit Step(const float* r) : c{r[0], r[1], r[2], r[3], r[4], 0.0f} {}
  template <int CLIP>
  __device__ __forceinline__ float next(float s, float xv, float pv) const {
    return rf_step_elem<CLIP, 1>(c, s, clip_x0(c.a0, xv, c.b0, pv), xv, pv, 0.0f, false).xn;
  }
};

template <>
struct Step<OBJ_K> {  // ops.edm_table's row; s1 and cb are not read (first order, eta = 0)
  static constexpr int WORDS = 8;
  EdmCoef c;
  __device__ __forceinline__ explicit Step(const float* r) : c{r[0], r[1], r[2], r[3], r[4], r[5], 0.0f, 0.0f} {}
  template <int CLIP>
  __device__ __forceinline__ float next(float s, float xv, float pv) const {
    return edm_step_elem<CLIP, 1>(c, s, clip_x0(c.a0, xv, c.b0, pv), xv, pv, 0.0f, 0.0f, false, false).xn;
  }
};

// (A, S, P, Q) behind the step row, and what of them the whole launch branches on
struct Blend {
  float A, S, P, Q;
  bool jump, rescale, renoise;  // S != 0 ; S == 0 and A != 1 ; Q != 0
  __device__ __forceinline__ explicit Blend(const float* r) : A(r[0]), S(r[1]), P(r[2]), Q(r[3]) {
    jump = S != 0.0f;
    rescale = !jump && A != 1.0f;
    renoise = Q != 0.0f;
  }
};

// One element, by the rounding sequence of the header: the step, the jump, the known region, the choice.
template <int OBJ, int CLIP>
__device__ __forceinline__ float repaint_elem(const Step<OBJ>& st, const Blend& b, float s, float xv, float pv, float sv,
                                              float z, bool keep) {
  float y = st.template next<CLIP>(s, xv, pv);
  if (b.jump)
    y = fma_rn(b.S, z, b.A * y);
  else if (b.rescale)
    y = b.A * y;
  const float k = b.renoise ? fma_rn(b.P, sv, b.Q * z) : b.P * sv;
  return keep ? k : y;
}

// VEC: x, p, src and xo are 16-byte aligned and mask is 4-byte aligned.  CLIP_SCALE: element i takes scale[i / per].
template <int OBJ, int CLIP, bool VEC>
__global__ __launch_bounds__(256) void repaint_step_kernel(const float* x, const float* p, const float* src,
                                                           const uint8_t* mask, const float* row, const uint32_t* rng4,
                                                           const float* scale, int64_t n, int64_t per, float* xo) {
  const Step<OBJ> st(row);
  const Blend b(row + Step<OBJ>::WORDS);  // (the same branches in every lane of the launch)
  const Normals normals(rng4, b.jump || b.renoise);
  const int64_t groups = groups4(n);
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t e = 4 * g;
    const bool whole = VEC && e + 4 <= n;
    bool keep[4] = {false, false, false, false};
    if (whole) {
      const uint32_t mw = *(const uint32_t*)(mask + e);
#pragma unroll
      for (int k = 0; k < 4; ++k) keep[k] = ((mw >> (8 * k)) & 0xFFu) != 0u;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < n) keep[k] = mask[e + k] != 0;
    }
    // a group draws only if it needs a normal: the jump does everywhere, the known region where an element keeps the source
    f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
    if (b.jump || (b.renoise && (keep[0] || keep[1] || keep[2] || keep[3]))) z = normals(g);
    float s[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (CLIP == CLIP_SCALE) item_values4(scale, e, n, per, s);
    if (whole) {
      const f32x4 xv = *(const f32x4*)(x + e), pv = *(const f32x4*)(p + e), sv = *(const f32x4*)(src + e);
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = repaint_elem<OBJ, CLIP>(st, b, s[k], xv[k], pv[k], sv[k], z[k], keep[k]);
      *(f32x4*)(xo + e) = o;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < n) xo[e + k] = repaint_elem<OBJ, CLIP>(st, b, s[k], x[e + k], p[e + k], src[e + k], z[k], keep[k]);
    }
  }
}

// the checks and the launch the three entry points share
template <int OBJ>
int repaint_step(const float* x, const float* p, const float* source, const uint8_t* mask, const float* row,
                 const uint32_t* rng4, int64_t clip, const float* scale, int64_t rows, int64_t per, float* x_out,
                 void* stream) {
  if (!mask) return ADP_ERR_NULL;  // (bytes: no alignment of its own)
  const int64_t n = flat_count({x, p, source, row, x_out}, {rng4, scale}, rows, per, clip_ok(clip, scale));
  if (n <= 0) return (int)n;
  const bool vec = aligned16({x, p, source, x_out}) && !misaligned(mask, 4);
  with_clip(clip, scale, [&](auto CLIP) {
    with_flag(vec, [&](auto VEC) {
      ADP_LAUNCH((repaint_step_kernel<OBJ, CLIP(), VEC()>), dim3(grid4(n)), dim3(256), stream, x, p, source, mask, row,
                 rng4, scale, n, per, x_out);
    });
  });
  return ADP_LAUNCH_OK();
}

}  // namespace

extern "C" int adp_repaint_v_step(const float* x, const float* v, const float* source, const uint8_t* mask,
                                  const float* row8, const uint32_t* rng4, int64_t clip, const float* scale, int64_t rows,
                                  int64_t per, float* x_out, void* stream) {
  return repaint_step<OBJ_V>(x, v, source, mask, row8, rng4, clip, scale, rows, per, x_out, stream);
}

extern "C" int adp_repaint_rf_step(const float* x, const float* u, const float* source, const uint8_t* mask,
                                   const float* row10, const uint32_t* rng4, int64_t clip, const float* scale, int64_t rows,
                                   int64_t per, float* x_out, void* stream) {
  return repaint_step<OBJ_RF>(x, u, source, mask, row10, rng4, clip, scale, rows, per, x_out, stream);
}

extern "C" int adp_repaint_k_step(const float* xs, const float* f, const float* source, const uint8_t* mask,
                                  const float* row12, const uint32_t* rng4, int64_t clip, const float* scale, int64_t rows,
                                  int64_t per, float* xs_out, void* stream) {
  return repaint_step<OBJ_K>(xs, f, source, mask, row12, rng4, clip, scale, rows, per, xs_out, stream);
}
