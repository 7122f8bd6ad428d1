// What the sampler-update kernels share (clip.hip, sde.hip, rf.hip, edm.hip, repaint.hip, rng.hip), each decision stated once: the arithmetic of
// the predicted clean value and its clamps, whose bits include/adp_clip.h, adp_sde.h and adp_rf.h promise to be the ones
// adp_clip_scale ranked; the group-of-four geometry of the flat elementwise kernels; the host checks and the choice of a
// kernel instantiation.  Private to those sources.
#pragma once
#include <type_traits>

#include "adp_rt.h"

namespace upd {

// ---- arithmetic.  The multiply-adds are explicit: left to the compiler, the 16-byte and the single-element form of a kernel
// could contract differently and differ in the last bit.
__device__ __forceinline__ float fma_rn(float a, float b, float c) {
#ifdef ADP_EMULATE
  return fmaf(a, b, c);
#else
  return __fmaf_rn(a, b, c);
#endif
}

// THE predicted clean value: one product rounded, one fused multiply-add.  Every pass of the select and every step kernel
// (adp_clip_step, adp_v_step_eta, adp_rf_step) call this and nothing else, so that all of them see the same bits (a pass
// that rounded differently could send the select into an empty bucket, a step that did would clamp a value the scale was
// not selected from).
__device__ __forceinline__ float clip_x0(float a0, float x, float b0, float v) { return fma_rn(a0, x, -(b0 * v)); }

// clamp(y, -s, s) / s; a NaN y or s stays NaN (torch.clamp's behaviour, which fminf / fmaxf do not have)
__device__ __forceinline__ float clamp_div(float y, float s) {
  const float c = y < -s ? -s : (y > s ? s : y);
  return c / s;
}
__device__ __forceinline__ float clamp1(float y) { return y < -1.0f ? -1.0f : (y > 1.0f ? 1.0f : y); }

enum { CLIP_NONE = 0, CLIP_STATIC = 1, CLIP_SCALE = 2 };

// x0 clipped by mode: as it is, clamped to [-1, 1], or clamped to the item's scale s and divided by it
template <int CLIP>
__device__ __forceinline__ float clipped(float x0, float s) {
  return CLIP == CLIP_STATIC ? clamp1(x0) : CLIP == CLIP_SCALE ? clamp_div(x0, s) : x0;
}

// ---- the element updates of the three objectives, each stated once: sde.hip, rf.hip and edm.hip wrap them in their step
// kernels, repaint.hip puts the RePaint jump and the known region behind them.  Every caller forms x0 itself, by
// clip_x0(c.a0, x, c.b0, p) and nothing else, and hands it in: the one spelling a reader (and tests/test_clip_placement.py)
// finds in every source that clamps x0.
// v-objective (include/adp_sde.h): a1 clip(a0 x - b0 v) + ce (b0 x + a0 v) [+ cz z]
struct SdeCoef {
  float a0, b0, a1, ce, cz;
};

// One element behind x0 = clip_x0(c.a0, xv, c.b0, vv).  x0 and its clamps are clip_x0 and clipped above, the ones clip.hip's
// select ranks and adp_clip_step applies: the scale was selected from those bits, and a NaN x0 or scale stays NaN.
template <int CLIP>
__device__ __forceinline__ float sde_elem(const SdeCoef& c, float s, float x0, float xv, float vv, float z, bool noisy) {
  const float eps = fma_rn(c.b0, xv, c.a0 * vv);
  const float x0c = clipped<CLIP>(x0, s);
  const float xn = fma_rn(c.a1, x0c, c.ce * eps);
  return noisy ? fma_rn(c.cz, z, xn) : xn;
}

// rectified flow (include/adp_rf.h): c1 clip(a0 x - b0 u) + a1 (c0 u + x) [+ cb (w - hist)]
struct RfCoef {
  float a0, b0, c0, a1, c1, cb;
};

struct RfStepped {
  float xn, w;
};

// One element behind x0 = clip_x0(c.a0, xv, c.b0, uv), by the rounding sequence of the header.
template <int CLIP, int ORDER>
__device__ __forceinline__ RfStepped rf_step_elem(const RfCoef& c, float s, float x0, float xv, float uv, float hv,
                                                  bool multi) {
  const float eps = fma_rn(c.c0, uv, xv);
  const float x0c = clipped<CLIP>(x0, s);
  RfStepped r;
  r.xn = fma_rn(c.c1, x0c, c.a1 * eps);
  r.w = 0.0f;
  if (ORDER == 2) {
    r.w = eps - x0c;
    if (multi) r.xn = fma_rn(c.cb, r.w - hv, r.xn);
  }
  return r;
}

// Karras / EDM (include/adp_edm.h): c1 clip(a0 xs - b0 F) + d1 (e0 xs + f0 F) [+ cb (x0c - hist)] [+ s1 z]
struct EdmCoef {
  float a0, b0, e0, f0, c1, d1, s1, cb;
};

struct EdmStepped {
  float xn, x0c;
};

// One element behind x0 = clip_x0(c.a0, xv, c.b0, fv), by the rounding sequence of the header.
template <int CLIP, int ORDER>
__device__ __forceinline__ EdmStepped edm_step_elem(const EdmCoef& c, float s, float x0, float xv, float fv, float hv,
                                                    float z, bool multi, bool noisy) {
  const float nh = fma_rn(c.e0, xv, c.f0 * fv);
  EdmStepped r;
  r.x0c = clipped<CLIP>(x0, s);
  r.xn = fma_rn(c.c1, r.x0c, c.d1 * nh);
  if (ORDER == 2 && multi) r.xn = fma_rn(c.cb, r.x0c - hv, r.xn);
  if (noisy) r.xn = fma_rn(c.s1, z, r.xn);
  return r;
}

// ---- groups of four: one thread owns one group of four consecutive elements per pass, in a grid-stride loop.
// (philox::rng_groups spells the same count n / 4 + (n % 4 != 0) for rng.hip and sde.hip and stays: the compiler builds a
// different loop around each spelling, and neither family's device code is to change.)
__device__ __forceinline__ int64_t groups4(int64_t n) { return (n + 3) / 4; }

// vals[k] = table[(e + k) / per] for the elements e + k < n of the group at e (the others are left as they are): one 64-bit
// division per group, then a walk over the item boundaries inside it (e < n, so the walk stays below rows)
__device__ __forceinline__ void item_values4(const float* table, int64_t e, int64_t n, int64_t per, float* vals) {
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

// ---- host side
// blocks of 256 threads for n elements: one group per thread and pass
inline unsigned grid4(int64_t n) {
  int64_t g = adp_cdiv(adp_cdiv(n, 4), 256);
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (unsigned)g;
}

inline bool misaligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

// rows * per does not fit int64_t
inline bool count_overflows(int64_t rows, int64_t per) { return per > 0 && rows > INT64_MAX / per; }

// The choice of a kernel instantiation: f receives the run-time value as a std::integral_constant, to be read in a template
// argument as TAG().  Nested, they replace a ladder of if / else per template parameter.
template <class F>
inline void with_flag(bool on, F&& f) {
  if (on)
    f(std::true_type{});
  else
    f(std::false_type{});
}

// the clip mode of adp_v_step_eta and adp_rf_step from their (clip, scale) arguments
template <class F>
inline void with_clip(int64_t clip, const float* scale, F&& f) {
  if (clip == 0)
    f(std::integral_constant<int, CLIP_NONE>{});
  else if (!scale)
    f(std::integral_constant<int, CLIP_STATIC>{});
  else
    f(std::integral_constant<int, CLIP_SCALE>{});
}

}  // namespace upd
