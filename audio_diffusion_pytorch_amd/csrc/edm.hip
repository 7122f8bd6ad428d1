// Karras (EDM) diffusion (include/adp_edm.h): the fused noising of the training step and the sampler update on the scaled
// state xs = c_in(sigma) x.
//   adp_edm_noise : x_in = c_in x + (c_in sigma) n ; target = (sigma / (sd r)) x - (sd / r) n              2 reads, 2 writes
//   adp_edm_step  : xs_out = c1 clip(a0 xs - b0 F) + d1 (e0 xs + f0 F) [+ cb (x0c - hist)] [+ s1 z]        2 reads, 1 write
//                                                                                                 (order 2: 3 reads, 2 writes)
// The noising is a pass of csrc/sampler_update.h's for_groups4.  The step writes the same pass out, with the same
// guarantees and that header's draw: through for_groups4 its CLIP_SCALE, ORDER 2, VEC form needs more scalar registers than
// there are.  That loop is kept in step with for_groups4 by hand.  The arithmetic of x0 and its clamps is that header's
// too, shared with clip.hip, sde.hip and rf.hip.
#include "adp_rt.h"
#include "adp.h"
#include "adp_edm.h"
#include "philox.h"
#include "sampler_update.h"

namespace {

using namespace upd;

// ---- noising.  The four per-item coefficients by the sequence of the header: one product, one fused multiply-add, one
// square root and four divisions, each correctly rounded (the product build keeps hipcc's default, correctly rounded
// float32 division and square root), so the emulated build forms the same bits.
struct EdmNoiseCoef {
  float c_in, c_n, t_x, t_n;
};

__device__ __forceinline__ EdmNoiseCoef edm_noise_coef(float sigma, float sd) {
  const float r = sqrtf(fma_rn(sigma, sigma, sd * sd));
  EdmNoiseCoef c;
  c.c_in = 1.0f / r;
  c.c_n = sigma / r;
  c.t_x = c.c_n / sd;
  c.t_n = sd / r;
  return c;
}

struct EdmNoised {
  float x_in, target;
};

__device__ __forceinline__ EdmNoised edm_noise_elem(const EdmNoiseCoef& c, float xv, float nv) {
  EdmNoised r;
  r.x_in = fma_rn(c.c_in, xv, c.c_n * nv);
  r.target = fma_rn(c.t_x, xv, -(c.t_n * nv));
  return r;
}

template <bool VEC>
__global__ __launch_bounds__(256) void edm_noise_kernel(const float* x, const float* noise, const float* sigma, float sd,
                                                        int64_t n, int64_t per, float* xi, float* tg) {
  const In in[] = {x, noise};
  const Out out[] = {xi, tg};
  struct Group {
    EdmNoiseCoef c[4];
  };
  for_groups4<VEC>(
      in, out, n,
      [&](int64_t, int64_t e, bool) {
        float sv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        item_values4(sigma, e, n, per, sv);
        // the coefficients are a function of the item's sigma alone: formed for the group's first element and again only
        // where the walk met another value (a NaN sigma compares unequal and is formed again: the same NaN coefficients)
        Group v;
        v.c[0] = edm_noise_coef(sv[0], sd);
#pragma unroll
        for (int k = 1; k < 4; ++k) v.c[k] = sv[k] == sv[k - 1] ? v.c[k - 1] : edm_noise_coef(sv[k], sd);
        return v;
      },
      [&](const Group& v, int k, const float(&a)[2], float(&o)[2]) {
        const EdmNoised r = edm_noise_elem(v.c[k], a[0], a[1]);
        o[0] = r.x_in;
        o[1] = r.target;
      });
}

// ---- the sampler update: edm_step_elem of sampler_update.h behind x0 = clip_x0(...)
// VEC: xs, f, xo (and hist, ho for ORDER 2) are 16-byte aligned.  CLIP_SCALE: element i takes scale[i / per].
template <int CLIP, int ORDER, bool VEC>
__global__ __launch_bounds__(256) void edm_step_kernel(const float* x, const float* f, const float* hist,
                                                       const float* coef8, const uint32_t* rng4, const float* scale,
                                                       int64_t n, int64_t per, float* xo, float* ho) {
  const EdmCoef c{coef8[0], coef8[1], coef8[2], coef8[3], coef8[4], coef8[5], coef8[6], coef8[7]};
  const bool multi = ORDER == 2 && c.cb != 0.0f;  // (the same branches in every lane of the launch)
  const bool noisy = c.s1 != 0.0f;
  const Normals normals(rng4, noisy);
  const int64_t groups = groups4(n);
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t e = 4 * g;
    f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
    if (noisy) z = normals(g);
    float s[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (CLIP == CLIP_SCALE) item_values4(scale, e, n, per, s);
    if (VEC && e + 4 <= n) {
      const f32x4 xv = *(const f32x4*)(x + e), fv = *(const f32x4*)(f + e);
      f32x4 hv = {0.0f, 0.0f, 0.0f, 0.0f};
      if (multi) hv = *(const f32x4*)(hist + e);
      f32x4 o, w;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float x0 = clip_x0(c.a0, xv[k], c.b0, fv[k]);
        const EdmStepped r = edm_step_elem<CLIP, ORDER>(c, s[k], x0, xv[k], fv[k], hv[k], z[k], multi, noisy);
        o[k] = r.xn;
        w[k] = r.x0c;
      }
      *(f32x4*)(xo + e) = o;
      if (ORDER == 2) *(f32x4*)(ho + e) = w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < n) {
          const float hv = multi ? hist[e + k] : 0.0f;
          const float xv = x[e + k], fv = f[e + k];
          const float x0 = clip_x0(c.a0, xv, c.b0, fv);
          const EdmStepped r = edm_step_elem<CLIP, ORDER>(c, s[k], x0, xv, fv, hv, z[k], multi, noisy);
          xo[e + k] = r.xn;
          if (ORDER == 2) ho[e + k] = r.x0c;
        }
    }
  }
}

}  // namespace

extern "C" int adp_edm_noise(const float* x, const float* noise, const float* sigma, float sigma_data, int64_t rows,
                             int64_t per, float* x_in_out, float* target_out, void* stream) {
  const int64_t n = flat_count({x, noise, sigma, x_in_out, target_out}, {}, rows, per, sigma_data > 0.0f);
  if (n <= 0) return (int)n;
  const bool vec = aligned16({x, noise, x_in_out, target_out});
  with_flag(vec, [&](auto VEC) {
    ADP_LAUNCH((edm_noise_kernel<VEC()>), dim3(grid4(n)), dim3(256), stream, x, noise, sigma, sigma_data, n, per, x_in_out,
               target_out);
  });
  return ADP_LAUNCH_OK();
}

extern "C" int adp_edm_step(const float* xs, const float* f, const float* hist, const float* coef8, const uint32_t* rng4,
                            int64_t order, int64_t clip, const float* scale, int64_t rows, int64_t per, float* xs_out,
                            float* hist_out, void* stream) {
  if (order == 2 && (!hist || !hist_out)) return ADP_ERR_NULL;
  if (order != 2) hist = nullptr, hist_out = nullptr;  // (the first-order kernels take no history)
  const bool own_ok = (order == 1 || order == 2) && clip_ok(clip, scale);
  const int64_t n = flat_count({xs, f, coef8, xs_out}, {rng4, scale, hist, hist_out}, rows, per, own_ok);
  if (n <= 0) return (int)n;
  const bool vec = aligned16({xs, f, xs_out, hist, hist_out});
  with_clip(clip, scale, [&](auto CLIP) {
    with_flag(order == 2, [&](auto ORDER2) {
      with_flag(vec, [&](auto VEC) {
        ADP_LAUNCH((edm_step_kernel<CLIP(), ORDER2() ? 2 : 1, VEC()>), dim3(grid4(n)), dim3(256), stream, xs, f, hist, coef8,
                   rng4, scale, n, per, xs_out, hist_out);
      });
    });
  });
  return ADP_LAUNCH_OK();
}
