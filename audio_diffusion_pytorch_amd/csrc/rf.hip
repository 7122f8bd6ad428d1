// Rectified flow (include/adp_rf.h): the fused noising of the training step and the sampler update.
//   adp_rf_noise : x_t = (1 - t_r) x + t_r n ; u = n - x                                  2 reads, 2 writes
//   adp_rf_step  : x_out = c1 clip(a0 x - b0 u) + a1 (c0 u + x) [+ cb (w - hist)]         2 reads, 1 write (order 2: 3, 2)
// Both write out the pass of csrc/sampler_update.h's for_groups4, which states the geometry and its guarantees, and are
// kept in step with it by hand: through for_groups4 the noising measured up to 3 % and the step's order-2 forms up to 1.5 %
// slower.  The arithmetic of x0 and its clamps and the host checks are that header's too, shared with clip.hip and sde.hip.
#include "adp_rt.h"
#include "adp.h"
#include "adp_rf.h"
#include "sampler_update.h"

namespace {

using namespace upd;

// ---- noising.  fma(-t, x, x) is (1 - t) x in one rounding; t = 0 gives x and t = 1 gives n, bit for bit.
struct RfNoised {
  float xt, u;
};

__device__ __forceinline__ RfNoised rf_noise_elem(float t, float xv, float nv) {
  RfNoised r;
  r.xt = fma_rn(t, nv, fma_rn(-t, xv, xv));
  r.u = nv - xv;
  return r;
}

template <bool VEC>
__global__ __launch_bounds__(256) void rf_noise_kernel(const float* x, const float* noise, const float* t, int64_t n,
                                                       int64_t per, float* xt, float* uo) {
  const int64_t groups = groups4(n);
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t e = 4 * g;
    float tv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    item_values4(t, e, n, per, tv);
    if (VEC && e + 4 <= n) {
      const f32x4 xv = *(const f32x4*)(x + e), nv = *(const f32x4*)(noise + e);
      f32x4 a, b;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const RfNoised r = rf_noise_elem(tv[k], xv[k], nv[k]);
        a[k] = r.xt;
        b[k] = r.u;
      }
      *(f32x4*)(xt + e) = a;
      *(f32x4*)(uo + e) = b;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < n) {
          const RfNoised r = rf_noise_elem(tv[k], x[e + k], noise[e + k]);  // (both read before either store: aliasing)
          xt[e + k] = r.xt;
          uo[e + k] = r.u;
        }
    }
  }
}

// ---- the sampler update: rf_step_elem of sampler_update.h behind x0 = clip_x0(...)
// VEC: x, u, xo (and hist, ho for ORDER 2) are 16-byte aligned.  CLIP_SCALE: element i takes scale[i / per].
template <int CLIP, int ORDER, bool VEC>
__global__ __launch_bounds__(256) void rf_step_kernel(const float* x, const float* u, const float* hist, const float* coef6,
                                                      const float* scale, int64_t n, int64_t per, float* xo, float* ho) {
  const RfCoef c{coef6[0], coef6[1], coef6[2], coef6[3], coef6[4], coef6[5]};
  const bool multi = ORDER == 2 && c.cb != 0.0f;  // (the same branch in every lane of the launch)
  const int64_t groups = groups4(n);
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t e = 4 * g;
    float s[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (CLIP == CLIP_SCALE) item_values4(scale, e, n, per, s);
    if (VEC && e + 4 <= n) {
      const f32x4 xv = *(const f32x4*)(x + e), uv = *(const f32x4*)(u + e);
      f32x4 hv = {0.0f, 0.0f, 0.0f, 0.0f};
      if (multi) hv = *(const f32x4*)(hist + e);
      f32x4 o, w;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float x0 = clip_x0(c.a0, xv[k], c.b0, uv[k]);
        const RfStepped r = rf_step_elem<CLIP, ORDER>(c, s[k], x0, xv[k], uv[k], hv[k], multi);
        o[k] = r.xn;
        w[k] = r.w;
      }
      *(f32x4*)(xo + e) = o;
      if (ORDER == 2) *(f32x4*)(ho + e) = w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < n) {
          const float hv = multi ? hist[e + k] : 0.0f;
          const float xv = x[e + k], uv = u[e + k];
          const RfStepped r = rf_step_elem<CLIP, ORDER>(c, s[k], clip_x0(c.a0, xv, c.b0, uv), xv, uv, hv, multi);
          xo[e + k] = r.xn;
          if (ORDER == 2) ho[e + k] = r.w;
        }
    }
  }
}

}  // namespace

extern "C" int adp_rf_noise(const float* x, const float* noise, const float* t, int64_t rows, int64_t per, float* x_t_out,
                            float* u_out, void* stream) {
  const int64_t n = flat_count({x, noise, t, x_t_out, u_out}, {}, rows, per);
  if (n <= 0) return (int)n;
  const bool vec = aligned16({x, noise, x_t_out, u_out});
  with_flag(vec, [&](auto VEC) {
    ADP_LAUNCH((rf_noise_kernel<VEC()>), dim3(grid4(n)), dim3(256), stream, x, noise, t, n, per, x_t_out, u_out);
  });
  return ADP_LAUNCH_OK();
}

extern "C" int adp_rf_step(const float* x, const float* u, const float* hist, const float* coef6, int64_t order,
                           int64_t clip, const float* scale, int64_t rows, int64_t per, float* x_out, float* hist_out,
                           void* stream) {
  if (order == 2 && (!hist || !hist_out)) return ADP_ERR_NULL;
  if (order != 2) hist = nullptr, hist_out = nullptr;  // (the first-order kernels take no history)
  const bool own_ok = (order == 1 || order == 2) && clip_ok(clip, scale);
  const int64_t n = flat_count({x, u, coef6, x_out}, {scale, hist, hist_out}, rows, per, own_ok);
  if (n <= 0) return (int)n;
  const bool vec = aligned16({x, u, x_out, hist, hist_out});
  with_clip(clip, scale, [&](auto CLIP) {
    with_flag(order == 2, [&](auto ORDER2) {
      with_flag(vec, [&](auto VEC) {
        ADP_LAUNCH((rf_step_kernel<CLIP(), ORDER2() ? 2 : 1, VEC()>), dim3(grid4(n)), dim3(256), stream, x, u, hist, coef6,
                   scale, n, per, x_out, hist_out);
      });
    });
  });
  return ADP_LAUNCH_OK();
}
