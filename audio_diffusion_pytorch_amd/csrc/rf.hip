// Rectified flow (include/adp_rf.h): the fused noising of the training step and the sampler update.
//   adp_rf_noise : x_t = (1 - t_r) x + t_r n ; u = n - x                                  2 reads, 2 writes
//   adp_rf_step  : x_out = c1 clip(a0 x - b0 u) + a1 (c0 u + x) [+ cb (w - hist)]         2 reads, 1 write (order 2: 3, 2)
// Both are bandwidth-bound elementwise passes of v_step_eta_kernel's shape (sde.hip): one thread owns one group of four
// elements per pass, in a grid-stride loop over the groups; 16-byte accesses where every tensor operand allows them, single
// elements otherwise.  The per-item values (t, scale) are found by one 64-bit division per group and a walk over the item
// boundaries inside it.  No LDS, no atomics, no cross-lane traffic; ordinary vector or single-element stores only.
#include "adp_rt.h"
#include "adp.h"
#include "adp_rf.h"

namespace {

#ifdef ADP_EMULATE
inline float rf_fma(float a, float b, float c) { return fmaf(a, b, c); }
#else
__device__ __forceinline__ float rf_fma(float a, float b, float c) { return __fmaf_rn(a, b, c); }
#endif

enum { CLIP_NONE = 0, CLIP_STATIC = 1, CLIP_SCALE = 2 };

// vals[k] = table[(e + k) / per] for the elements e + k < n of one group (e < n, so the walk stays below rows)
__device__ __forceinline__ void rf_item_values(const float* table, int64_t e, int64_t n, int64_t per, float* vals) {
  int64_t item = e / per, next = (item + 1) * per;
  float cur = table[item];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (e + k < n) {
      while (e + k >= next) {
        ++item;
        next += per;
        cur = table[item];
      }
      vals[k] = cur;
    }
  }
}

// ---- noising.  The multiply-adds are explicit: left to the compiler, the 16-byte and the single-element form could contract
// differently.  fma(-t, x, x) is (1 - t) x in one rounding; t = 0 gives x and t = 1 gives n, bit for bit.
struct RfNoised {
  float xt, u;
};

__device__ __forceinline__ RfNoised rf_noise_elem(float t, float xv, float nv) {
  RfNoised r;
  r.xt = rf_fma(t, nv, rf_fma(-t, xv, xv));
  r.u = nv - xv;
  return r;
}

template <bool VEC>
__global__ __launch_bounds__(256) void rf_noise_kernel(const float* x, const float* noise, const float* t, int64_t n,
                                                       int64_t per, float* xt, float* uo) {
  const int64_t groups = (n + 3) / 4;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t e = 4 * g;
    float tv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    rf_item_values(t, e, n, per, tv);
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

// ---- the sampler update
struct RfCoef {
  float a0, b0, c0, a1, c1, cb;
};

struct RfStepped {
  float xn, w;
};

// One element, by the rounding sequence of the header.  x0 is clip.hip's clip_x0 (fma(a0, x, -(b0 * u))): the scale was
// selected from those bits.  The clamps are clip.hip's as well: a NaN x0 or scale stays NaN.
template <int CLIP, int ORDER>
__device__ __forceinline__ RfStepped rf_step_elem(const RfCoef& c, float s, float xv, float uv, float hv, bool multi) {
  const float x0 = rf_fma(c.a0, xv, -(c.b0 * uv));
  const float eps = rf_fma(c.c0, uv, xv);
  float x0c = x0;
  if (CLIP == CLIP_STATIC) x0c = x0 < -1.0f ? -1.0f : (x0 > 1.0f ? 1.0f : x0);
  if (CLIP == CLIP_SCALE) x0c = (x0 < -s ? -s : (x0 > s ? s : x0)) / s;
  RfStepped r;
  r.xn = rf_fma(c.c1, x0c, c.a1 * eps);
  r.w = 0.0f;
  if (ORDER == 2) {
    r.w = eps - x0c;
    if (multi) r.xn = rf_fma(c.cb, r.w - hv, r.xn);
  }
  return r;
}

// VEC: x, u, xo (and hist, ho for ORDER 2) are 16-byte aligned.  CLIP_SCALE: element i takes scale[i / per].
template <int CLIP, int ORDER, bool VEC>
__global__ __launch_bounds__(256) void rf_step_kernel(const float* x, const float* u, const float* hist, const float* coef6,
                                                      const float* scale, int64_t n, int64_t per, float* xo, float* ho) {
  const RfCoef c{coef6[0], coef6[1], coef6[2], coef6[3], coef6[4], coef6[5]};
  const bool multi = ORDER == 2 && c.cb != 0.0f;  // (the same branch in every lane of the launch)
  const int64_t groups = (n + 3) / 4;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t e = 4 * g;
    float s[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (CLIP == CLIP_SCALE) rf_item_values(scale, e, n, per, s);
    if (VEC && e + 4 <= n) {
      const f32x4 xv = *(const f32x4*)(x + e), uv = *(const f32x4*)(u + e);
      f32x4 hv = {0.0f, 0.0f, 0.0f, 0.0f};
      if (multi) hv = *(const f32x4*)(hist + e);
      f32x4 o, w;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const RfStepped r = rf_step_elem<CLIP, ORDER>(c, s[k], xv[k], uv[k], hv[k], multi);
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
          const RfStepped r = rf_step_elem<CLIP, ORDER>(c, s[k], x[e + k], u[e + k], hv, multi);
          xo[e + k] = r.xn;
          if (ORDER == 2) ho[e + k] = r.w;
        }
    }
  }
}

// one group per thread and pass
unsigned rf_grid(int64_t n) {
  int64_t g = adp_cdiv(adp_cdiv(n, 4), 256);
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (unsigned)g;
}

inline bool misaligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

template <int CLIP, int ORDER>
void launch_step(bool vec, void* stream, const float* x, const float* u, const float* hist, const float* coef6,
                 const float* scale, int64_t n, int64_t per, float* xo, float* ho) {
  if (vec)
    ADP_LAUNCH((rf_step_kernel<CLIP, ORDER, true>), dim3(rf_grid(n)), dim3(256), stream, x, u, hist, coef6, scale, n, per, xo,
               ho);
  else
    ADP_LAUNCH((rf_step_kernel<CLIP, ORDER, false>), dim3(rf_grid(n)), dim3(256), stream, x, u, hist, coef6, scale, n, per,
               xo, ho);
}

template <int ORDER>
void launch_order(int64_t clip, bool vec, void* stream, const float* x, const float* u, const float* hist,
                  const float* coef6, const float* scale, int64_t n, int64_t per, float* xo, float* ho) {
  if (clip == 0)
    launch_step<CLIP_NONE, ORDER>(vec, stream, x, u, hist, coef6, scale, n, per, xo, ho);
  else if (!scale)
    launch_step<CLIP_STATIC, ORDER>(vec, stream, x, u, hist, coef6, scale, n, per, xo, ho);
  else
    launch_step<CLIP_SCALE, ORDER>(vec, stream, x, u, hist, coef6, scale, n, per, xo, ho);
}

}  // namespace

extern "C" int adp_rf_noise(const float* x, const float* noise, const float* t, int64_t rows, int64_t per, float* x_t_out,
                            float* u_out, void* stream) {
  if (!x || !noise || !t || !x_t_out || !u_out) return ADP_ERR_NULL;
  if (rows < 0 || per < 0) return ADP_ERR_SHAPE;
  if (per > 0 && rows > INT64_MAX / per) return ADP_ERR_SHAPE;
  if (misaligned(x, 4) || misaligned(noise, 4) || misaligned(t, 4) || misaligned(x_t_out, 4) || misaligned(u_out, 4))
    return ADP_ERR_ALIGN;
  const int64_t n = rows * per;
  if (n == 0) return ADP_OK;
  const bool vec = !misaligned(x, 16) && !misaligned(noise, 16) && !misaligned(x_t_out, 16) && !misaligned(u_out, 16);
  if (vec)
    ADP_LAUNCH((rf_noise_kernel<true>), dim3(rf_grid(n)), dim3(256), stream, x, noise, t, n, per, x_t_out, u_out);
  else
    ADP_LAUNCH((rf_noise_kernel<false>), dim3(rf_grid(n)), dim3(256), stream, x, noise, t, n, per, x_t_out, u_out);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_rf_step(const float* x, const float* u, const float* hist, const float* coef6, int64_t order,
                           int64_t clip, const float* scale, int64_t rows, int64_t per, float* x_out, float* hist_out,
                           void* stream) {
  if (!x || !u || !coef6 || !x_out) return ADP_ERR_NULL;
  if (order == 2 && (!hist || !hist_out)) return ADP_ERR_NULL;
  if (rows < 0 || per < 0 || (order != 1 && order != 2) || (clip != 0 && clip != 1) || (clip == 0 && scale))
    return ADP_ERR_SHAPE;
  if (per > 0 && rows > INT64_MAX / per) return ADP_ERR_SHAPE;
  if (misaligned(x, 4) || misaligned(u, 4) || misaligned(coef6, 4) || misaligned(x_out, 4) ||
      (scale && misaligned(scale, 4)) || (order == 2 && (misaligned(hist, 4) || misaligned(hist_out, 4))))
    return ADP_ERR_ALIGN;
  const int64_t n = rows * per;
  if (n == 0) return ADP_OK;
  bool vec = !misaligned(x, 16) && !misaligned(u, 16) && !misaligned(x_out, 16);
  if (order == 1) {
    launch_order<1>(clip, vec, stream, x, u, nullptr, coef6, scale, n, per, x_out, nullptr);
  } else {
    vec = vec && !misaligned(hist, 16) && !misaligned(hist_out, 16);
    launch_order<2>(clip, vec, stream, x, u, hist, coef6, scale, n, per, x_out, hist_out);
  }
  return ADP_LAUNCH_OK();
}
