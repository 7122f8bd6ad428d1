// Counter-based normal generator (Philox4x32-10 + Box-Muller) and the VInpainter resample step that draws from it
// (include/adp_rng.h).  Seed and draw index are read from a 4-word DEVICE row, so one captured launch serves every draw:
// the host copies the next row in front of the replay.
//   adp_philox_bits        : the raw words of a row's stream (the integer generator, tested exactly)
//   adp_randn              : the normals of a row's stream, 1 write
//   adp_v_inpaint_step_rng : adp_v_inpaint_step with the noise formed in registers, 3 reads + 1 byte, 1 write
// One thread owns one group of four elements per pass: one Philox call (ten rounds of two 32x32->64 multiplies) and two
// Box-Muller pairs.  No LDS, no atomics, no cross-lane traffic; ordinary vector or single-element stores only.  The grid of
// such a kernel and the alignment predicate are csrc/sampler_update.h's, shared with sde.hip and rf.hip.
#include "adp_rt.h"
#include "adp.h"
#include "adp_rng.h"
#include "inpaint_blend.h"
#include "philox.h"
#include "sampler_update.h"

namespace {

using namespace philox;  // (csrc/philox.h: the generator itself, shared with sde.hip)
using namespace upd;     // (csrc/sampler_update.h: grid4 and misaligned)

// VEC: out is 16-byte aligned -> whole groups leave as one 16-byte store; the tail group and the unaligned case as single
// predicated stores
template <bool VEC>
__global__ __launch_bounds__(256) void philox_bits_kernel(const uint32_t* rng4, int64_t n, uint32_t* out) {
  const RngRow r = rng_row(rng4);
  const int64_t groups = rng_groups(n);
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const U32x4 w = rng_words(r, g);
    const int64_t e = 4 * g;
    if (VEC && e + 4 <= n) {
      *(U32x4*)(out + e) = w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < n) out[e + k] = w.w[k];
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void randn_kernel(const uint32_t* rng4, int64_t n, float* out) {
  const RngRow r = rng_row(rng4);
  const int64_t groups = rng_groups(n);
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const f32x4 z = rng_normal4(r, g);
    const int64_t e = 4 * g;
    if (VEC && e + 4 <= n) {
      *(f32x4*)(out + e) = z;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < n) out[e + k] = z[k];
    }
  }
}

// VEC: x, v, src and xo are 16-byte aligned and mask is 4-byte aligned.  A group none of whose elements keeps the source
// needs no noise and skips the draw (the values of the others do not depend on it).
template <bool VEC>
__global__ __launch_bounds__(256) void v_inpaint_rng_kernel(const float* x, const float* v, const float* src,
                                                            const uint8_t* mask, const float* ab4, const uint32_t* rng4,
                                                            int64_t n, float* xo) {
  const VInpaintCoef c{ab4[0], ab4[1], ab4[2], ab4[3]};
  const RngRow r = rng_row(rng4);
  const int64_t groups = rng_groups(n);
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t e = 4 * g;
    f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
    if (VEC && e + 4 <= n) {
      const f32x4 xv = *(const f32x4*)(x + e), vv = *(const f32x4*)(v + e), sv = *(const f32x4*)(src + e);
      const uint32_t m4 = *(const uint32_t*)(mask + e);
      if (m4 != 0u) z = rng_normal4(r, g);
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        o[k] = adp_v_inpaint_blend(c, xv[k], vv[k], sv[k], z[k], ((m4 >> (8 * k)) & 0xFFu) != 0u);
      *(f32x4*)(xo + e) = o;
    } else {
      bool keep[4], any = false;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        keep[k] = e + k < n && mask[e + k] != 0;
        any = any || keep[k];
      }
      if (any) z = rng_normal4(r, g);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < n) xo[e + k] = adp_v_inpaint_blend(c, x[e + k], v[e + k], src[e + k], z[k], keep[k]);
    }
  }
}

}  // namespace

extern "C" int adp_philox_bits(const uint32_t* rng4, int64_t n_words, uint32_t* out, void* stream) {
  if (!rng4 || !out) return ADP_ERR_NULL;
  if (n_words < 0) return ADP_ERR_SHAPE;
  if (misaligned(rng4, 4) || misaligned(out, 4)) return ADP_ERR_ALIGN;
  if (n_words == 0) return ADP_OK;
  if (!misaligned(out, 16))
    ADP_LAUNCH(philox_bits_kernel<true>, dim3(grid4(n_words)), dim3(256), stream, rng4, n_words, out);
  else
    ADP_LAUNCH(philox_bits_kernel<false>, dim3(grid4(n_words)), dim3(256), stream, rng4, n_words, out);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_randn(const uint32_t* rng4, int64_t n, float* out, void* stream) {
  if (!rng4 || !out) return ADP_ERR_NULL;
  if (n < 0) return ADP_ERR_SHAPE;
  if (misaligned(rng4, 4) || misaligned(out, 4)) return ADP_ERR_ALIGN;
  if (n == 0) return ADP_OK;
  if (!misaligned(out, 16))
    ADP_LAUNCH(randn_kernel<true>, dim3(grid4(n)), dim3(256), stream, rng4, n, out);
  else
    ADP_LAUNCH(randn_kernel<false>, dim3(grid4(n)), dim3(256), stream, rng4, n, out);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_v_inpaint_step_rng(const float* x, const float* v, const float* source, const uint8_t* mask,
                                      const float* ab4, const uint32_t* rng4, int64_t n, float* x_out, void* stream) {
  if (!x || !v || !source || !mask || !ab4 || !rng4 || !x_out) return ADP_ERR_NULL;
  if (n < 0) return ADP_ERR_SHAPE;
  if (misaligned(x, 4) || misaligned(v, 4) || misaligned(source, 4) || misaligned(ab4, 4) || misaligned(rng4, 4) ||
      misaligned(x_out, 4))
    return ADP_ERR_ALIGN;
  if (n == 0) return ADP_OK;
  const bool vec = !misaligned(x, 16) && !misaligned(v, 16) && !misaligned(source, 16) && !misaligned(x_out, 16) &&
                   !misaligned(mask, 4);
  if (vec)
    ADP_LAUNCH(v_inpaint_rng_kernel<true>, dim3(grid4(n)), dim3(256), stream, x, v, source, mask, ab4, rng4, n, x_out);
  else
    ADP_LAUNCH(v_inpaint_rng_kernel<false>, dim3(grid4(n)), dim3(256), stream, x, v, source, mask, ab4, rng4, n, x_out);
  return ADP_LAUNCH_OK();
}
