// Dynamic thresholding (include/adp_clip.h): the exact per-item quantile of |x0| by a three-pass radix select, and the
// v-sampler step that clips the predicted clean signal with it.
//   adp_clip_scale : zero + 3 histogram passes (11 + 10 + 10 key bits) + finalize; x0 = a0 x - b0 v is formed on the fly
//                    by clip_x0 of csrc/sampler_update.h, which every kernel that clamps x0 calls as well
//   adp_clip_apply : out = clamp(x, -s, s) / s
//   adp_clip_step  : first / second order update on the clipped x0, in place on x and the history
// One workgroup histograms a span of CLIP_SPAN values of one row in LDS and merges its non-empty bins into the row's
// histogram with integer adds (order-independent: bit-identical from call to call).  The bucket choice after a pass is made
// by every workgroup of the next pass (clip_select), block 0 of the row records it for the passes behind.
#include "adp_rt.h"
#include "adp.h"
#include "adp_clip.h"
#include "sampler_update.h"

namespace {

using namespace upd;  // (csrc/sampler_update.h: clip_x0 and the clamps, shared with sde.hip and rf.hip)

constexpr int CLIP_SPAN = 4096;                       // values of a row per workgroup and pass
constexpr int CLIP_NB1 = 2048, CLIP_NB = 1024;        // bins of pass 1 (key bits 30..20) and of passes 2, 3 (10 bits each)
// workspace words per row: hist1 | hist2 lo, hi | hist3 lo, hi | sel1[4] sel2[4] nan[1] (padded)
constexpr int WS_H1 = 0, WS_H2 = CLIP_NB1, WS_H3 = WS_H2 + 2 * CLIP_NB, WS_SEL1 = WS_H3 + 2 * CLIP_NB, WS_SEL2 = WS_SEL1 + 4,
              WS_NAN = WS_SEL2 + 4, WS_ROW = WS_NAN + 8;
constexpr uint32_t KEY_INF = 0x7F800000u;

#ifdef ADP_EMULATE
inline void clip_count(uint32_t* p, uint32_t n) { *p += n; }  // (workgroups and lanes run one after another)
#else
__device__ __forceinline__ void clip_count(uint32_t* p, uint32_t n) { atomicAdd(p, n); }
#endif

// the key a pass ranks: the bits of |x0|, x0 from the one function the step kernels clamp (sampler_update.h)
template <bool HASV>
__device__ __forceinline__ uint32_t clip_key(float a0, float b0, float x, float v) {
  return __float_as_uint(HASV ? clip_x0(a0, x, b0, v) : x) & 0x7FFFFFFFu;
}

// the prefix and the rank inside it of the two order statistics after a pass
struct ClipSel {
  uint32_t p_lo, r_lo, p_hi, r_hi;
};

// Bucket choice: the bin of h_lo that holds rank r_lo and the bin of h_hi that holds rank r_hi (NB bins each; the two may be
// the same histogram), with the ranks inside those bins.  256 threads, NB / 256 consecutive bins each; the two running sums
// share one 64-bit scan (a row has at most 2^24 values: the low half cannot carry).  Result in sel4 (LDS) after the
// trailing barrier: [bin_lo, rank_lo, bin_hi, rank_hi]; zeros where a rank is not below the histogram's total.
template <int NB>
__device__ __forceinline__ void clip_select(const uint32_t* h_lo, const uint32_t* h_hi, uint32_t r_lo, uint32_t r_hi,
                                            uint64_t* scan256, uint32_t* sel4) {
  constexpr int PER = NB / 256;
  const int t = threadIdx.x;
  uint32_t a[PER], b[PER], sa = 0u, sb = 0u;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    a[k] = h_lo[t * PER + k];
    b[k] = h_hi[t * PER + k];
    sa += a[k];
    sb += b[k];
  }
  scan256[t] = (uint64_t)sa | ((uint64_t)sb << 32);
  if (t < 4) sel4[t] = 0u;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const uint64_t add = t >= off ? scan256[t - off] : 0ull;
    __syncthreads();
    scan256[t] += add;
    __syncthreads();
  }
  const uint64_t incl = scan256[t];
  uint32_t ea = (uint32_t)incl - sa, eb = (uint32_t)(incl >> 32) - sb;  // exclusive sums in front of this thread's bins
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (r_lo >= ea && r_lo - ea < a[k]) {
      sel4[0] = (uint32_t)(t * PER + k);
      sel4[1] = r_lo - ea;
    }
    if (r_hi >= eb && r_hi - eb < b[k]) {
      sel4[2] = (uint32_t)(t * PER + k);
      sel4[3] = r_hi - eb;
    }
    ea += a[k];
    eb += b[k];
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void clip_zero_kernel(uint32_t* ws, int64_t words) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) ws[i] = 0u;
}

// LEVEL 1: histogram of key bits 30..20 of the whole row, and the row's NaN count.
// LEVEL 2: choose the pass-1 buckets of ranks lo and hi (sel1), histogram key bits 19..10 of the keys inside each.
// LEVEL 3: choose the pass-2 buckets (sel2), histogram key bits 9..0.
// Grid (spans of the row, rows).  VEC: x, v 16-byte aligned and per % 4 == 0 (every row then starts 16-byte aligned).
template <int LEVEL, bool HASV, bool VEC>
__global__ __launch_bounds__(256) void clip_pass_kernel(const float* x, const float* v, const float* coef, int64_t per,
                                                        uint32_t lo, uint32_t hi, uint32_t* ws) {
  __shared__ uint32_t hist[CLIP_NB1];  // LEVEL 1: 2048 bins; LEVEL 2, 3: [lo prefix | hi prefix] x 1024 bins
  __shared__ uint64_t scan256[256];
  __shared__ uint32_t sel4[4];
  __shared__ uint32_t saw_nan;
  const int t = threadIdx.x;
  uint32_t* wsr = ws + (int64_t)blockIdx.y * WS_ROW;
  for (int i = t; i < CLIP_NB1; i += 256) hist[i] = 0u;
  if (t == 0) saw_nan = 0u;

  ClipSel s{0u, 0u, 0u, 0u};
  if (LEVEL == 2) {
    clip_select<CLIP_NB1>(wsr + WS_H1, wsr + WS_H1, lo, hi, scan256, sel4);
    s = ClipSel{sel4[0], sel4[1], sel4[2], sel4[3]};
  } else if (LEVEL == 3) {
    const ClipSel s1{wsr[WS_SEL1], wsr[WS_SEL1 + 1], wsr[WS_SEL1 + 2], wsr[WS_SEL1 + 3]};
    const uint32_t* h_lo = wsr + WS_H2;
    clip_select<CLIP_NB>(h_lo, s1.p_lo == s1.p_hi ? h_lo : h_lo + CLIP_NB, s1.r_lo, s1.r_hi, scan256, sel4);
    s = ClipSel{(s1.p_lo << 10) | sel4[0], sel4[1], (s1.p_hi << 10) | sel4[2], sel4[3]};
  } else {
    __syncthreads();
  }
  if (LEVEL >= 2 && blockIdx.x == 0 && t == 0) {
    uint32_t* out = wsr + (LEVEL == 2 ? WS_SEL1 : WS_SEL2);
    out[0] = s.p_lo;
    out[1] = s.r_lo;
    out[2] = s.p_hi;
    out[3] = s.r_hi;
  }

  float a0 = 0.0f, b0 = 0.0f;
  if (HASV) {
    a0 = coef[0];
    b0 = coef[1];
  }
  constexpr int PSHIFT = LEVEL == 2 ? 20 : 10;  // prefix = key >> PSHIFT, digit = the 10 bits below it
  auto count = [&](uint32_t key) {
    if (LEVEL == 1) {
      clip_count(&hist[key >> 20], 1u);
      if (key > KEY_INF) saw_nan = 1u;  // (every writer stores the same value)
    } else {
      const uint32_t p = key >> PSHIFT, d = (key >> (PSHIFT - 10)) & (CLIP_NB - 1);
      if (p == s.p_lo)
        clip_count(&hist[d], 1u);
      else if (p == s.p_hi)
        clip_count(&hist[CLIP_NB + d], 1u);
    }
  };
  const float* xr = x + (int64_t)blockIdx.y * per;
  const float* vr = HASV ? v + (int64_t)blockIdx.y * per : nullptr;
  const int64_t begin = (int64_t)blockIdx.x * CLIP_SPAN, end = begin + CLIP_SPAN < per ? begin + CLIP_SPAN : per;
  if (VEC) {
    for (int64_t i = begin + 4 * t; i < end; i += 4 * 256) {  // (per % 4 == 0: whole groups only)
      const f32x4 xv = *(const f32x4*)(xr + i);
      f32x4 vv = {0.0f, 0.0f, 0.0f, 0.0f};
      if (HASV) vv = *(const f32x4*)(vr + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) count(clip_key<HASV>(a0, b0, xv[k], vv[k]));
    }
  } else {
    for (int64_t i = begin + t; i < end; i += 256) count(clip_key<HASV>(a0, b0, xr[i], HASV ? vr[i] : 0.0f));
  }
  __syncthreads();
  uint32_t* g = wsr + (LEVEL == 1 ? WS_H1 : LEVEL == 2 ? WS_H2 : WS_H3);
  for (int i = t; i < CLIP_NB1; i += 256)
    if (hist[i] != 0u) clip_count(&g[i], hist[i]);
  if (LEVEL == 1 && t == 0 && saw_nan != 0u) clip_count(&wsr[WS_NAN], 1u);
}

// torch.lerp, every operation rounded on its own (no fused multiply-add: where the two keys are denormals a contraction
// would differ from the host's result in the last bits)
__device__ __forceinline__ float clip_lerp(float a, float b, float w) {
#ifndef ADP_EMULATE
#pragma clang fp contract(off)
#endif
  const float d = b - a;
  return w < 0.5f ? a + w * d : b - d * (1.0f - w);
}

// choose the pass-3 buckets: the two keys are complete.  One workgroup per row.
__global__ __launch_bounds__(256) void clip_final_kernel(const uint32_t* ws, float w, float floor_, float* scale) {
  __shared__ uint64_t scan256[256];
  __shared__ uint32_t sel4[4];
  const uint32_t* wsr = ws + (int64_t)blockIdx.x * WS_ROW;
  const ClipSel s2{wsr[WS_SEL2], wsr[WS_SEL2 + 1], wsr[WS_SEL2 + 2], wsr[WS_SEL2 + 3]};
  const uint32_t* h_lo = wsr + WS_H3;
  clip_select<CLIP_NB>(h_lo, s2.p_lo == s2.p_hi ? h_lo : h_lo + CLIP_NB, s2.r_lo, s2.r_hi, scan256, sel4);
  if (threadIdx.x != 0) return;
  const float a = __uint_as_float((s2.p_lo << 10) | sel4[0]), b = __uint_as_float((s2.p_hi << 10) | sel4[2]);
  const float q = clip_lerp(a, b, w);
  float s = q > floor_ ? q : floor_;
  if (wsr[WS_NAN] != 0u) s = __uint_as_float(0x7FC00000u);
  scale[blockIdx.x] = s;
}

// grid (blocks along the row, rows): the scale is uniform in a workgroup
template <bool VEC>
__global__ __launch_bounds__(256) void clip_apply_kernel(const float* x, const float* scale, int64_t per, float* out) {
  const float s = scale[blockIdx.y];
  const float* xr = x + (int64_t)blockIdx.y * per;
  float* o = out + (int64_t)blockIdx.y * per;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthreads = (int64_t)gridDim.x * 256;
  if (VEC) {
    for (int64_t i = 4 * tid; i < per; i += 4 * nthreads) {
      const f32x4 xv = *(const f32x4*)(xr + i);
      f32x4 y;
#pragma unroll
      for (int k = 0; k < 4; ++k) y[k] = clamp_div(xv[k], s);
      *(f32x4*)(o + i) = y;
    }
  } else {
    for (int64_t i = tid; i < per; i += nthreads) o[i] = clamp_div(xr[i], s);
  }
}

struct ClipStepCoef {
  float a0, b0, a1, b1, ca, cb;
};

// one element of the update; hx, he: previous (clipped x0, eps) in, this step's out.  DYN: divide by the item's scale
template <bool DYN, bool HIST>
__device__ __forceinline__ float clip_step_elem(const ClipStepCoef& c, float s, float xv, float vv, float& hx, float& he) {
  const float x0 = clip_x0(c.a0, xv, c.b0, vv);
  const float eps = fma_rn(c.b0, xv, c.a0 * vv);
  const float x0c = clipped<DYN ? CLIP_SCALE : CLIP_STATIC>(x0, s);
  float xn = fma_rn(c.a1, x0c, c.b1 * eps);
  if (HIST) xn = fma_rn(c.cb, eps - he, fma_rn(c.ca, x0c - hx, xn));
  hx = x0c;
  he = eps;
  return xn;
}

// ORDER2: the history is written; HIST: it is read as well.  VEC: every pointer 16-byte aligned and per % 4 == 0.
template <bool DYN, bool ORDER2, bool HIST, bool VEC>
__device__ __forceinline__ void clip_step_body(const ClipStepCoef& c, float s, const float* x, const float* v,
                                               const float* hx, const float* he, int64_t per, float* xo, float* hxo,
                                               float* heo) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthreads = (int64_t)gridDim.x * 256;
  if (VEC) {
    for (int64_t i = 4 * tid; i < per; i += 4 * nthreads) {
      const f32x4 xv = *(const f32x4*)(x + i), vv = *(const f32x4*)(v + i);
      f32x4 px = {0.0f, 0.0f, 0.0f, 0.0f}, pe = {0.0f, 0.0f, 0.0f, 0.0f}, xn;
      if (HIST) {
        px = *(const f32x4*)(hx + i);
        pe = *(const f32x4*)(he + i);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pxk = px[k], pek = pe[k];
        xn[k] = clip_step_elem<DYN, HIST>(c, s, xv[k], vv[k], pxk, pek);
        px[k] = pxk;
        pe[k] = pek;
      }
      *(f32x4*)(xo + i) = xn;
      if (ORDER2) {
        *(f32x4*)(hxo + i) = px;
        *(f32x4*)(heo + i) = pe;
      }
    }
  } else {
    for (int64_t i = tid; i < per; i += nthreads) {
      float px = 0.0f, pe = 0.0f;
      if (HIST) {
        px = hx[i];
        pe = he[i];
      }
      xo[i] = clip_step_elem<DYN, HIST>(c, s, x[i], v[i], px, pe);
      if (ORDER2) {
        hxo[i] = px;
        heo[i] = pe;
      }
    }
  }
}

// grid (blocks along the row, rows)
template <bool DYN, bool ORDER2, bool VEC>
__global__ __launch_bounds__(256) void clip_step_kernel(const float* x, const float* v, const float* hx, const float* he,
                                                        const float* coef, const float* scale, int64_t per, float* xo,
                                                        float* hxo, float* heo) {
  ClipStepCoef c{coef[0], coef[1], coef[2], coef[3], 0.0f, 0.0f};
  if (ORDER2) {
    c.ca = coef[4];
    c.cb = coef[5];
  }
  const float s = DYN ? scale[blockIdx.y] : 1.0f;
  const int64_t r = (int64_t)blockIdx.y * per;
  x += r;
  v += r;
  xo += r;
  if (ORDER2) {
    hx += r;
    he += r;
    hxo += r;
    heo += r;
  }
  if (ORDER2 && !(c.ca == 0.0f && c.cb == 0.0f))  // (the same branch in every lane of the launch)
    clip_step_body<DYN, true, true, VEC>(c, s, x, v, hx, he, per, xo, hxo, heo);
  else
    clip_step_body<DYN, ORDER2, false, VEC>(c, s, x, v, hx, he, per, xo, hxo, heo);
}

constexpr int64_t CLIP_MAX_PER = (int64_t)1 << 24, CLIP_MAX_ROWS = 65535;

// blocks along a row for the elementwise kernels: one group of four per thread and pass, capped so that rows * blocks stays
// a few waves of the chip
unsigned row_grid(int64_t per) {
  int64_t g = adp_cdiv(adp_cdiv(per, 4), 256);
  if (g > 1024) g = 1024;
  if (g < 1) g = 1;
  return (unsigned)g;
}

template <int LEVEL>
void launch_pass(bool hasv, bool vec, dim3 grid, void* stream, const float* x, const float* v, const float* coef,
                 int64_t per, uint32_t lo, uint32_t hi, uint32_t* ws) {
  if (hasv && vec)
    ADP_LAUNCH((clip_pass_kernel<LEVEL, true, true>), grid, dim3(256), stream, x, v, coef, per, lo, hi, ws);
  else if (hasv)
    ADP_LAUNCH((clip_pass_kernel<LEVEL, true, false>), grid, dim3(256), stream, x, v, coef, per, lo, hi, ws);
  else if (vec)
    ADP_LAUNCH((clip_pass_kernel<LEVEL, false, true>), grid, dim3(256), stream, x, v, coef, per, lo, hi, ws);
  else
    ADP_LAUNCH((clip_pass_kernel<LEVEL, false, false>), grid, dim3(256), stream, x, v, coef, per, lo, hi, ws);
}

}  // namespace

extern "C" int64_t adp_clip_ws_bytes(int64_t rows, int64_t per) {
  if (rows < 0 || per < 0 || per > CLIP_MAX_PER) return ADP_ERR_SHAPE;
  if (rows > CLIP_MAX_ROWS) return ADP_ERR_UNSUPPORTED;
  return rows * (int64_t)WS_ROW * (int64_t)sizeof(uint32_t);
}

extern "C" int adp_clip_scale(const float* x, const float* v, const float* coef, int64_t rows, int64_t per, int64_t lo,
                              float w, float min_scale, void* ws, float* scale, void* stream) {
  if (!x || !ws || !scale || (v && !coef)) return ADP_ERR_NULL;
  if (rows < 0 || per < 0 || per > CLIP_MAX_PER) return ADP_ERR_SHAPE;
  if (rows == 0 || per == 0) return ADP_OK;
  if (lo < 0 || lo >= per || !(w >= 0.0f && w < 1.0f) || (w > 0.0f && lo + 1 >= per)) return ADP_ERR_SHAPE;
  if (rows > CLIP_MAX_ROWS) return ADP_ERR_UNSUPPORTED;
  if (misaligned(x, 4) || (v && (misaligned(v, 4) || misaligned(coef, 4))) || misaligned(ws, 4) || misaligned(scale, 4))
    return ADP_ERR_ALIGN;
  const bool hasv = v != nullptr;
  const bool vec = !misaligned(x, 16) && !(v && misaligned(v, 16)) && per % 4 == 0;
  const uint32_t ulo = (uint32_t)lo, uhi = ulo + (w > 0.0f ? 1u : 0u);
  uint32_t* wsu = (uint32_t*)ws;
  const int64_t words = rows * WS_ROW;
  const dim3 grid((unsigned)adp_cdiv(per, CLIP_SPAN), (unsigned)rows);
  ADP_LAUNCH(clip_zero_kernel, dim3((unsigned)(adp_cdiv(words, 256) > 1024 ? 1024 : adp_cdiv(words, 256))), dim3(256), stream,
             wsu, words);
  launch_pass<1>(hasv, vec, grid, stream, x, v, coef, per, ulo, uhi, wsu);
  launch_pass<2>(hasv, vec, grid, stream, x, v, coef, per, ulo, uhi, wsu);
  launch_pass<3>(hasv, vec, grid, stream, x, v, coef, per, ulo, uhi, wsu);
  ADP_LAUNCH(clip_final_kernel, dim3((unsigned)rows), dim3(256), stream, (const uint32_t*)wsu, w, min_scale, scale);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_clip_apply(const float* x, const float* scale, int64_t rows, int64_t per, float* out, void* stream) {
  if (!x || !scale || !out) return ADP_ERR_NULL;
  if (rows < 0 || per < 0 || per > CLIP_MAX_PER) return ADP_ERR_SHAPE;
  if (rows == 0 || per == 0) return ADP_OK;
  if (rows > CLIP_MAX_ROWS) return ADP_ERR_UNSUPPORTED;
  if (misaligned(x, 4) || misaligned(scale, 4) || misaligned(out, 4)) return ADP_ERR_ALIGN;
  const dim3 grid(row_grid(per), (unsigned)rows);
  if (!misaligned(x, 16) && !misaligned(out, 16) && per % 4 == 0)
    ADP_LAUNCH(clip_apply_kernel<true>, grid, dim3(256), stream, x, scale, per, out);
  else
    ADP_LAUNCH(clip_apply_kernel<false>, grid, dim3(256), stream, x, scale, per, out);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_clip_step(const float* x, const float* v, const float* hist_x0, const float* hist_eps,
                             const float* coef, int64_t order, const float* scale, int64_t rows, int64_t per,
                             float* x_out, float* hist_x0_out, float* hist_eps_out, void* stream) {
  if (!x || !v || !coef || !x_out) return ADP_ERR_NULL;
  if (order == 2 && (!hist_x0 || !hist_eps || !hist_x0_out || !hist_eps_out)) return ADP_ERR_NULL;
  if (rows < 0 || per < 0 || per > CLIP_MAX_PER || (order != 1 && order != 2)) return ADP_ERR_SHAPE;
  if (rows == 0 || per == 0) return ADP_OK;
  if (rows > CLIP_MAX_ROWS) return ADP_ERR_UNSUPPORTED;
  if (misaligned(x, 4) || misaligned(v, 4) || misaligned(coef, 4) || misaligned(x_out, 4) || (scale && misaligned(scale, 4)))
    return ADP_ERR_ALIGN;
  bool vec = !misaligned(x, 16) && !misaligned(v, 16) && !misaligned(x_out, 16) && per % 4 == 0;
  if (order == 2) {
    if (misaligned(hist_x0, 4) || misaligned(hist_eps, 4) || misaligned(hist_x0_out, 4) || misaligned(hist_eps_out, 4))
      return ADP_ERR_ALIGN;
    vec = vec && !misaligned(hist_x0, 16) && !misaligned(hist_eps, 16) && !misaligned(hist_x0_out, 16) &&
          !misaligned(hist_eps_out, 16);
  }
  const dim3 grid(row_grid(per), (unsigned)rows);
  with_flag(scale != nullptr, [&](auto DYN) {
    with_flag(order == 2, [&](auto ORDER2) {
      with_flag(vec, [&](auto VEC) {
        ADP_LAUNCH((clip_step_kernel<DYN(), ORDER2(), VEC()>), grid, dim3(256), stream, x, v, hist_x0, hist_eps, coef, scale,
                   per, x_out, hist_x0_out, hist_eps_out);
      });
    });
  });
  return ADP_LAUNCH_OK();
}
