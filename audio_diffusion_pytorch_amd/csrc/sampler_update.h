// What the sampler-update kernels share (clip.hip, sde.hip, rf.hip, edm.hip, repaint.hip, distill.hip, rng.hip), each
// decision stated once: the arithmetic of the predicted clean value and its clamps, whose bits include/adp_clip.h, adp_sde.h
// and adp_rf.h promise to be the ones adp_clip_scale ranked; the group-of-four pass of the flat elementwise kernels and its
// noise draw; the host checks and the choice of a kernel instantiation.  Private to those sources.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "adp_rt.h"
#include "philox.h"

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
// (philox::rng_groups spells the same count n / 4 + (n % 4 != 0) for rng.hip and stays: the compiler builds a different loop
// around each spelling, and that family's device code is not to change.)
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

// THE pass of the flat elementwise kernels over the n elements of NI float inputs and NO float outputs: v_step_eta_kernel,
// edm_noise_kernel and distill_comb_kernel call it.  rf.hip's two kernels, edm_step_kernel, repaint_step_kernel and
// distill.hip's two loss kernels write the same pass out, with the same guarantees, for the reason each file gives
// (scalar registers, or a measured time); a change here is made there by hand.  A whole group (VEC: every operand is
// 16-byte aligned; all four elements lie below n) moves as 16 bytes per operand, any other as single elements.
// What every caller gets:
//   - an operand that is not `on` is absent for the whole launch: never dereferenced, an input reads as 0.  A pass that
//     only accumulates takes one output that is off, `const Out none[] = {{nullptr, false}}`, and leaves it unwritten;
//   - group(g, e, whole) runs once per group, before any load, and returns what the group's elements share: the per-item
//     values, the draw;
//   - elem(shared, k, in, out) runs for each element e + k < n of the group, in element order, pass by pass;
//   - an output may be any input: a whole group loads every input before it stores any output, and the single-element
//     form reads every input of element k before it stores any output of element k.
// No LDS, no atomics, no cross-lane traffic; ordinary vector or single-element stores only.
struct In {
  const float* p;
  bool on;
  __device__ __forceinline__ In(const float* p, bool on = true) : p(p), on(on) {}
};
struct Out {
  float* p;
  bool on;
  __device__ __forceinline__ Out(float* p, bool on = true) : p(p), on(on) {}
};

template <bool VEC, int NI, int NO, class Group, class Elem>
__device__ __forceinline__ void for_groups4(const In (&in)[NI], const Out (&out)[NO], int64_t n, Group&& group,
                                            Elem&& elem) {
  const int64_t groups = groups4(n);
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t e = 4 * g;
    const bool whole = VEC && e + 4 <= n;
    const auto gv = group(g, e, whole);
    if (whole) {
      f32x4 iv[NI], ov[NO];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
        iv[i] = zero;
        if (in[i].on) iv[i] = *(const f32x4*)(in[i].p + e);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float a[NI], r[NO] = {};
#pragma unroll
        for (int i = 0; i < NI; ++i) a[i] = iv[i][k];
        elem(gv, k, a, r);
#pragma unroll
        for (int j = 0; j < NO; ++j) ov[j][k] = r[j];
      }
#pragma unroll
      for (int j = 0; j < NO; ++j)
        if (out[j].on) *(f32x4*)(out[j].p + e) = ov[j];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < n) {
          float a[NI], r[NO] = {};
#pragma unroll
          for (int i = 0; i < NI; ++i) a[i] = in[i].on ? in[i].p[e + k] : 0.0f;
          elem(gv, k, a, r);
#pragma unroll
          for (int j = 0; j < NO; ++j)
            if (out[j].on) out[j].p[e + k] = r[j];
        }
    }
  }
}

// The normals of a launch's rng row (include/adp_rng.h), formed in registers: one Philox call and two Box-Muller pairs per
// group.  `wanted` is the launch's own condition for reading the row at all.  Noise asked for without a row is four NaNs:
// loud, and nothing is dereferenced.
struct Normals {
  philox::RngRow row{0u, 0u, 0u};
  bool have;
  __device__ __forceinline__ Normals(const uint32_t* rng4, bool wanted) : have(rng4 != nullptr) {
    if (wanted && have) row = philox::rng_row(rng4);
  }
  __device__ __forceinline__ f32x4 operator()(int64_t g) const {
    if (have) return philox::rng_normal4(row, g);
    const float nan = __uint_as_float(0x7FC00000u);
    const f32x4 z_nan = {nan, nan, nan, nan};
    return z_nan;
  }
};

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

// The checks of a flat item-wise entry point (rows items of per values each), in the order of precedence they all keep:
// ADP_ERR_NULL for a missing required pointer; ADP_ERR_SHAPE for a negative size, for the entry's own conditions (own_ok)
// and for a count beyond int64_t; ADP_ERR_ALIGN for a required or a present optional pointer off a 4-byte boundary.
// Otherwise the element count n >= 0.  n == 0 launches nothing and ADP_OK is 0: a caller returns (int)n whenever n <= 0.
static_assert(ADP_OK == 0 && ADP_ERR_NULL < 0 && ADP_ERR_SHAPE < 0 && ADP_ERR_ALIGN < 0,
              "flat_count returns the codes and the count through one value");
inline int64_t flat_count(std::initializer_list<const void*> required, std::initializer_list<const void*> optional,
                          int64_t rows, int64_t per, bool own_ok = true) {
  for (const void* p : required)
    if (!p) return ADP_ERR_NULL;
  if (rows < 0 || per < 0 || !own_ok || count_overflows(rows, per)) return ADP_ERR_SHAPE;
  for (const void* p : required)
    if (misaligned(p, 4)) return ADP_ERR_ALIGN;
  for (const void* p : optional)
    if (misaligned(p, 4)) return ADP_ERR_ALIGN;  // (a null one is absent, and aligned)
  return rows * per;
}

// every pointer allows 16-byte accesses (a null one is absent and constrains nothing)
inline bool aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (misaligned(p, 16)) return false;
  return true;
}

// The choice of a kernel instantiation: f receives the run-time value as a std::integral_constant, to be read in a template
// argument as TAG().  Nested, they replace a ladder of if / else per template parameter.
template <class F>
inline void with_flag(bool on, F&& f) {
  if (on)
    f(std::true_type{});
  else
    f(std::false_type{});
}

// the (clip, scale) arguments of a sampler update: clip is 0 or 1, and a scale needs clip; then the clip mode from them
inline bool clip_ok(int64_t clip, const float* scale) { return (clip == 0 || clip == 1) && !(clip == 0 && scale); }

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
