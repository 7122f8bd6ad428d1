// v-objective elementwise math and small helpers (HBM-bound streaming kernels, gfx950).
//   adp_v_noise  : diffusion.py:88-92   x_noisy = a x + b n ; v_target = a n - b x      (2 reads, 2 writes)
//   adp_mse_*    : diffusion.py:95      F.mse_loss(v_pred, v_target) and its gradient
//   adp_v_step   : diffusion.py:185-187 one VSampler update, 2 reads 1 write
//   adp_v_step2  : one VMultistepSampler update (two-step exponential integrator), 4 reads 3 writes
//   adp_arv_*    : diffusion.py:118-127, :231-235  autoregressive v-diffusion: one noise level per split of the window
//   adp_time_fourier_* : a_unet NumberEmbedder under TimeConditioningPlugin (components.py:74-76)
#include "adp_rt.h"
#ifndef ADP_EMULATE
#include <mutex>
#endif
#include "adp.h"
#include "adp_ar.h"
#include "inpaint_blend.h"

namespace {

constexpr float PI_F = 3.14159265358979323846f;

__global__ __launch_bounds__(256) void v_noise_kernel(const float* x, const float* noise, const float* sigma,
                                                      int64_t per, float* x_noisy, float* v_target) {
  const int64_t b = blockIdx.y;
  // angle = sigma * pi / 2 evaluated left to right in fp32, as the reference does (diffusion.py:78)
  const float angle = (sigma[b] * PI_F) / 2.0f;
  const float a = cosf(angle), bt = sinf(angle);
  const int64_t base = b * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256) {
    const float xv = x[base + i], nv = noise[base + i];
    x_noisy[base + i] = a * xv + bt * nv;
    v_target[base + i] = a * nv - bt * xv;
  }
}

constexpr int MSE_BLOCKS = 1024;

__global__ __launch_bounds__(256) void mse_partial_kernel(const float* p, const float* t, int64_t n, float* ws) {
  __shared__ float sh[4];
  float s = 0.0f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float d = p[i] - t[i];
    s = fmaf(d, d, s);
  }
  s = adp_block_sum<4>(s, sh);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

// one wave: lane l sums partials l, l + 64, ... in double (independent loads: a single thread walking all 1024 partials
// took 44 us), then the 64 lane sums are added in lane order by lane 0 -- fixed order, deterministic
__global__ __launch_bounds__(64) void mse_final_kernel(const float* ws, int nb, int64_t n, float* loss) {
  __shared__ double part[64];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 64) s += (double)ws[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double t = 0.0;
  for (int i = 0; i < 64; ++i) t += part[i];
  loss[0] = (float)(t / (double)n);
}

__global__ __launch_bounds__(256) void mse_bwd_kernel(const float* p, const float* t, const float* gloss, int64_t n,
                                                      float* dv) {
  const float sc = (gloss ? gloss[0] : 1.0f) * 2.0f / (float)n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    dv[i] = (p[i] - t[i]) * sc;
}

__global__ __launch_bounds__(256) void v_step_kernel(const float* x, const float* v, const float* ab4, int64_t n,
                                                     float* xo) {
  const float a0 = ab4[0], b0 = ab4[1], a1 = ab4[2], b1 = ab4[3];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float xv = x[i], vv = v[i];
    const float x_pred = a0 * xv - b0 * vv;
    const float n_pred = b0 * xv + a0 * vv;
    xo[i] = a1 * x_pred + b1 * n_pred;
  }
}

// one VMultistepSampler update (second-order two-step exponential integrator in the angle phi = sigma * pi / 2):
//   x0 = a0 x - b0 v ; eps = b0 x + a0 v
//   x_next = a1 x0 + b1 eps + ca (x0 - x0_prev) + cb (eps - eps_prev) ; history <- (x0, eps)
// coef6 = device [a0, b0, a1, b1, ca, cb].  A row with ca = cb = 0 (the first step) does NOT read the history: whatever an
// earlier run or the allocator left there (NaN included) cannot reach x.  Every output may alias its input: an element is
// read, then written, by the one lane that owns it.
struct VStep2Coef {
  float a0, b0, a1, b1, ca, cb;
};

template <bool HIST>
__device__ __forceinline__ float v_step2_elem(const VStep2Coef& c, float xv, float vv, float& hx, float& he) {
  const float x_pred = c.a0 * xv - c.b0 * vv;
  const float n_pred = c.b0 * xv + c.a0 * vv;
  float xn = c.a1 * x_pred + c.b1 * n_pred;
  if (HIST) xn += c.ca * (x_pred - hx) + c.cb * (n_pred - he);
  hx = x_pred;
  he = n_pred;
  return xn;
}

template <bool HIST>
__device__ __forceinline__ void v_step2_scalar_at(const VStep2Coef& c, const float* x, const float* v, const float* hx,
                                                  const float* he, int64_t i, float* xo, float* hxo, float* heo) {
  float px = 0.0f, pe = 0.0f;
  if (HIST) {
    px = hx[i];
    pe = he[i];
  }
  const float xn = v_step2_elem<HIST>(c, x[i], v[i], px, pe);
  xo[i] = xn;
  hxo[i] = px;
  heo[i] = pe;
}

// VEC: all seven pointers are 16-byte aligned -> 16-byte accesses on the first n & ~3 elements, scalar tail behind them
template <bool HIST, bool VEC>
__device__ __forceinline__ void v_step2_body(const VStep2Coef& c, const float* x, const float* v, const float* hx,
                                             const float* he, int64_t n, float* xo, float* hxo, float* heo) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthreads = (int64_t)gridDim.x * 256;
  const int64_t nv = VEC ? (n & ~(int64_t)3) : 0;
  for (int64_t i = 4 * tid; i < nv; i += 4 * nthreads) {
    const f32x4 xv = *(const f32x4*)(x + i), vv = *(const f32x4*)(v + i);
    f32x4 px = {0.0f, 0.0f, 0.0f, 0.0f}, pe = {0.0f, 0.0f, 0.0f, 0.0f}, xn;
    if (HIST) {
      px = *(const f32x4*)(hx + i);
      pe = *(const f32x4*)(he + i);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float pxk = px[k], pek = pe[k];
      xn[k] = v_step2_elem<HIST>(c, xv[k], vv[k], pxk, pek);
      px[k] = pxk;
      pe[k] = pek;
    }
    *(f32x4*)(xo + i) = xn;
    *(f32x4*)(hxo + i) = px;
    *(f32x4*)(heo + i) = pe;
  }
  for (int64_t i = nv + tid; i < n; i += nthreads) v_step2_scalar_at<HIST>(c, x, v, hx, he, i, xo, hxo, heo);
}

template <bool VEC>
__global__ __launch_bounds__(256) void v_step2_kernel(const float* x, const float* v, const float* hx, const float* he,
                                                      const float* coef6, int64_t n, float* xo, float* hxo,
                                                      float* heo) {
  const VStep2Coef c{coef6[0], coef6[1], coef6[2], coef6[3], coef6[4], coef6[5]};
  if (c.ca == 0.0f && c.cb == 0.0f)  // (the same branch in every lane of the launch)
    v_step2_body<false, VEC>(c, x, v, hx, he, n, xo, hxo, heo);
  else
    v_step2_body<true, VEC>(c, x, v, hx, he, n, xo, hxo, heo);
}

// one VInpainter resample step (diffusion.py:339-350): rotate (x, v) from noise level i to level j, re-noise the
// source to level j with the caller's draw, keep the source where mask is set (the arithmetic: inpaint_blend.h)
__global__ __launch_bounds__(256) void v_inpaint_kernel(const float* x, const float* v, const float* src,
                                                        const float* noise, const uint8_t* mask, const float* ab4,
                                                        int64_t n, float* xo) {
  const VInpaintCoef c{ab4[0], ab4[1], ab4[2], ab4[3]};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    xo[i] = adp_v_inpaint_blend(c, x[i], v[i], src[i], noise[i], mask[i] != 0);
}

// classifier-free guidance mix of the two halves of a batched [2B, ...] evaluation:
// out = o_masked + (o - o_masked) * scale,  o = y[:half], o_masked = y[half:]
__global__ __launch_bounds__(256) void cfg_mix_kernel(const float* y, int64_t half, float scale, float* out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < half; i += (int64_t)gridDim.x * 256) {
    const float o = y[i], om = y[half + i];
    out[i] = om + (o - om) * scale;
  }
}

// out[b, :] = pick[b] ? a[b, :] : bsrc[b, :]   (per-row select; CFG's training-time embedding mask and its batch
// doubling write through it)
__global__ __launch_bounds__(256) void select_rows_kernel(const float* a, const float* bsrc, const uint8_t* pick,
                                                          int64_t rows, int64_t per, float* out) {
  const int64_t n = rows * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / per;
    out[i] = pick[r] ? a[i] : bsrc[i];
  }
}

__global__ __launch_bounds__(256) void add_kernel(const float* a, const float* b, int64_t n, float* y) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = a[i] + b[i];
}

// out = a * x + b * y (y optional): gradient streams that meet with a constant factor (SkipCat's 2^-1/2 branch)
__global__ __launch_bounds__(256) void axpby_kernel(float a, const float* x, float b, const float* y, int64_t n,
                                                    float* out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = y ? fmaf(a, x[i], b * y[i]) : a * x[i];
}

// dst[r * dst_stride + c] = src[r * src_stride + c]: channel concat / split of [B, C, L] tensors seen as B rows
__global__ __launch_bounds__(256) void copy2d_kernel(const float* src, int64_t src_stride, float* dst,
                                                     int64_t dst_stride, int64_t rows, int64_t cols) {
  const int64_t n = rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cols, c = i - r * cols;
    dst[r * dst_stride + c] = src[r * src_stride + c];
  }
}

// space-to-depth of a [rows, L] tensor by factor f: out[(row * f + k), l] = x[row, l * f + k]  (a kernel = stride = f
// DownsampleItem with a factor the strided conv kernels do not cover becomes a 1x1 conv over the result)
__global__ __launch_bounds__(256) void unshuffle_kernel(const float* x, int64_t rows, int64_t Lo, int64_t f,
                                                        float* out) {
  const int64_t n = rows * Lo * f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / (Lo * f), p = i - row * (Lo * f);  // reads are coalesced
    const int64_t l = p / f, k = p - l * f;
    out[(row * f + k) * Lo + l] = x[i];
  }
}

// out[row, l] = sum_{k<f} x[row, l * f + k] (+ res[row, l]): gradient of a nearest upsample by any factor
__global__ __launch_bounds__(256) void pool_sum_kernel(const float* x, int64_t rows, int64_t Lo, int64_t f,
                                                       const float* res, float* out) {
  const int64_t n = rows * Lo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float* p = x + i * f;
    float s = 0.0f;
    for (int64_t k = 0; k < f; ++k) s += p[k];
    out[i] = res ? s + res[i] : s;
  }
}

__device__ __forceinline__ float act_f(float x, int act) {
  return act == 1 ? adp_silu(x) : (act == 2 ? adp_gelu(x) : x);
}
__device__ __forceinline__ float dact_f(float x, int act) {
  return act == 1 ? adp_dsilu(x) : (act == 2 ? adp_dgelu(x) : 1.0f);
}

__global__ __launch_bounds__(256) void act_fwd_kernel(const float* x, int64_t n, int act, float* y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = act_f(x[i], act);
}
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* x, const float* dy, int64_t n, int act,
                                                      int accumulate, float* dx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const float v = dy[i] * dact_f(x[i], act);
    dx[i] = accumulate ? dx[i] + v : v;
  }
}

// four[b, :] = [t, sin(f_0..f_{H-1}), cos(f_0..f_{H-1})],  f_h = ((t * w_h) * 2) * pi  (a_unet order of operations)
__global__ __launch_bounds__(256) void fourier_fwd_kernel(const float* t, const float* w, int64_t B, int64_t H,
                                                          float* four) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * H) return;
  const int64_t b = i / H, h = i % H;
  const float tv = t[b];
  const float f = ((tv * w[h]) * 2.0f) * PI_F;
  float* row = four + b * (2 * H + 1);
  if (h == 0) row[0] = tv;
  row[1 + h] = sinf(f);
  row[1 + H + h] = cosf(f);
}
__global__ __launch_bounds__(256) void fourier_bwd_kernel(const float* t, const float* w, const float* dfour,
                                                          int64_t B, int64_t H, int accumulate, float* dw) {
  const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (h >= H) return;
  float s = 0.0f;
  for (int64_t b = 0; b < B; ++b) {
    const float tv = t[b];
    const float f = ((tv * w[h]) * 2.0f) * PI_F;
    const float* row = dfour + b * (2 * H + 1);
    s += (row[1 + h] * cosf(f) - row[1 + H + h] * sinf(f)) * (tv * 2.0f * PI_F);
  }
  dw[h] = accumulate ? dw[h] + s : s;
}

// ---- fused AdamW step (optim.AdamW): gradient clipping at load, decoupled weight decay, moments, update, EMA lerp.
// Work is cut into chunks [tensor, first element, count] by the host (a 1 M-element conv weight and an 8-element bias
// balance); blocks stride over the chunk table.  Per chunk: scalar head up to the first 16-byte boundary of p, 16-byte
// accesses on the interior (two groups per lane in flight: ten independent loads before the first use), scalar tail.
// Gradients are slices of the flat gradient buffer, aligned to 4 bytes only: they are read through ld4_unaligned.
constexpr int OPT_MAX_PARTIALS = 1024;

// The tensors' addresses come out of a device table, so the compiler cannot tell that they are global memory and would use
// flat_ accesses (which also pass through the LDS aperture check and count on lgkmcnt): say so.
#ifdef ADP_EMULATE
#define OPT_GLOBAL
#else
#define OPT_GLOBAL __attribute__((address_space(1)))
#endif
typedef f32x4 f32x4_a4 __attribute__((aligned(4)));
__device__ __forceinline__ float opt_ld(const float* p) { return *(const OPT_GLOBAL float*)p; }
__device__ __forceinline__ void opt_st(float* p, float v) { *(OPT_GLOBAL float*)p = v; }
__device__ __forceinline__ f32x4 opt_ld4(const float* p) { return *(const OPT_GLOBAL f32x4*)p; }
__device__ __forceinline__ void opt_st4(float* p, f32x4 v) { *(OPT_GLOBAL f32x4*)p = v; }
// 4-byte aligned address: the compiler picks the widest load the target allows (global_load_dwordx4 on gfx950)
__device__ __forceinline__ f32x4 ld4_unaligned(const float* p) { return *(const OPT_GLOBAL f32x4_a4*)p; }

__device__ __forceinline__ int64_t opt_head(const void* p, int64_t cnt) {
  const int64_t h = (int64_t)((16 - ((uintptr_t)p & 15)) & 15) >> 2;  // elements up to the next 16-byte boundary
  return h < cnt ? h : cnt;
}

// block-wide sum of one double per thread in a fixed order (no 8-byte shuffles: an LDS tree); all threads get the result
__device__ __forceinline__ double opt_block_sum(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

__device__ __forceinline__ double opt_sq(double acc, float g) { return fma((double)g, (double)g, acc); }
__device__ __forceinline__ double opt_sq4(double acc, f32x4 g) {
  return opt_sq(opt_sq(opt_sq(opt_sq(acc, g[0]), g[1]), g[2]), g[3]);
}

__global__ __launch_bounds__(256) void sqnorm_partials_kernel(const float* const* ptrs, const int64_t* numels,
                                                              const int64_t* chunks, int64_t n_chunks,
                                                              double* partials) {
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t t = chunks[3 * c], start = chunks[3 * c + 1];
    int64_t cnt = chunks[3 * c + 2];
    if (start + cnt > numels[t]) cnt = numels[t] - start;  // (a table that disagrees with the tensors never reads past them)
    if (cnt <= 0) continue;
    const float* g = ptrs[t] + start;
    const int64_t head = opt_head(g, cnt);
    if (tid < head) acc = opt_sq(acc, opt_ld(g + tid));
    const int64_t nv = (cnt - head) & ~(int64_t)3;
    const float* gv = g + head;
    for (int64_t i = 4 * (int64_t)tid; i < nv; i += 2048) {
      const bool two = i + 1024 < nv;
      const f32x4 a = opt_ld4(gv + i);
      f32x4 b = {0.0f, 0.0f, 0.0f, 0.0f};
      if (two) b = opt_ld4(gv + i + 1024);
      acc = opt_sq4(opt_sq4(acc, a), b);
    }
    const int64_t j = head + nv + tid;
    if (j < cnt) acc = opt_sq(acc, opt_ld(g + j));
  }
  acc = opt_block_sum(acc, sh);
  if (tid == 0) partials[blockIdx.x] = acc;
}

struct AdamwScalars {
  float decay;         // 1 - lr * weight_decay
  float one_m_beta1;   // 1 - beta1
  float beta2;
  float one_m_beta2;   // 1 - beta2
  float inv_bc2_sqrt;  // 1 / sqrt(1 - beta2^step)
  float eps;
  float step_size;     // lr / (1 - beta1^step)
  float ema_w;         // 1 - ema_decay
};

// one element: every multiply-add is spelled fmaf and the compiler may not form others (it would fuse g * clip into the
// subtraction below in one path and not in the other), so the scalar and the 16-byte paths (and the emulated build) round alike
__device__ __forceinline__ void adamw_elem(const AdamwScalars& s, float clip, float& p, float g, float& m, float& v) {
#pragma clang fp contract(off)
  g *= clip;
  m = fmaf(g - m, s.one_m_beta1, m);
  v = fmaf(g * s.one_m_beta2, g, v * s.beta2);
  const float denom = fmaf(sqrtf(v), s.inv_bc2_sqrt, s.eps);
  p = fmaf(-s.step_size, m / denom, p * s.decay);
}

template <bool EMA>
__device__ __forceinline__ void adamw_scalar_at(const AdamwScalars& s, float clip, const adp_adamw_tensor& T, int64_t i) {
  float p = opt_ld(T.p + i), m = opt_ld(T.m + i), v = opt_ld(T.v + i);
  adamw_elem(s, clip, p, opt_ld(T.g + i), m, v);
  opt_st(T.p + i, p);
  opt_st(T.m + i, m);
  opt_st(T.v + i, v);
  if (EMA) {
    const float e = opt_ld(T.ema + i);
    opt_st(T.ema + i, fmaf(p - e, s.ema_w, e));
  }
}

template <bool EMA>
struct AdamwGroup4 {
  f32x4 p, g, m, v, e;
  __device__ __forceinline__ void load(const adp_adamw_tensor& T, int64_t i) {
    p = opt_ld4(T.p + i);
    g = ld4_unaligned(T.g + i);
    m = opt_ld4(T.m + i);
    v = opt_ld4(T.v + i);
    if (EMA) e = opt_ld4(T.ema + i);
  }
  __device__ __forceinline__ void update_store(const AdamwScalars& s, float clip, const adp_adamw_tensor& T, int64_t i) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float pk = p[k], mk = m[k], vk = v[k];
      adamw_elem(s, clip, pk, g[k], mk, vk);
      p[k] = pk;
      m[k] = mk;
      v[k] = vk;
      if (EMA) e[k] = fmaf(pk - e[k], s.ema_w, e[k]);
    }
    opt_st4(T.p + i, p);
    opt_st4(T.m + i, m);
    opt_st4(T.v + i, v);
    if (EMA) opt_st4(T.ema + i, e);
  }
};

template <bool EMA>
__device__ __forceinline__ void adamw_chunk(const AdamwScalars& s, float clip, const adp_adamw_tensor& T, int64_t cnt) {
  const int tid = threadIdx.x;
  // m, v (and the EMA tensor) must share p's 16-byte phase for the 16-byte path; allocations of their own always do
  uintptr_t phase = ((uintptr_t)T.p ^ (uintptr_t)T.m) | ((uintptr_t)T.p ^ (uintptr_t)T.v);
  if (EMA) phase |= (uintptr_t)T.p ^ (uintptr_t)T.ema;
  if (phase & 15) {
    for (int64_t i = tid; i < cnt; i += 256) adamw_scalar_at<EMA>(s, clip, T, i);
    return;
  }
  const int64_t head = opt_head(T.p, cnt);
  if (tid < head) adamw_scalar_at<EMA>(s, clip, T, tid);
  const int64_t nv = (cnt - head) & ~(int64_t)3;
  for (int64_t i = head + 4 * (int64_t)tid; i < head + nv; i += 2048) {
    const bool two = i + 1024 < head + nv;
    AdamwGroup4<EMA> a, b;
    a.load(T, i);
    if (two) b.load(T, i + 1024);
    a.update_store(s, clip, T, i);
    if (two) b.update_store(s, clip, T, i + 1024);
  }
  const int64_t j = head + nv + tid;
  if (j < cnt) adamw_scalar_at<EMA>(s, clip, T, j);
}

__global__ __launch_bounds__(256) void adamw_step_kernel(const adp_adamw_tensor* tensors, const int64_t* chunks,
                                                         int64_t n_chunks, AdamwScalars s, const double* partials,
                                                         int n_partials, float max_grad_norm, float* grad_norm_out) {
  __shared__ double sh[256];
  float clip = 1.0f;
  if (partials) {
    // every block adds the (at most 1024, L2-resident) partials in the same fixed order: one coefficient, no third launch
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += 256) acc += partials[i];
    const float norm = (float)sqrt(opt_block_sum(acc, sh));
    const float c = max_grad_norm / (norm + 1e-6f);
    clip = c > 1.0f ? 1.0f : c;  // (a NaN norm stays a NaN coefficient, as torch.clamp(max=1) keeps it)
    if (grad_norm_out && blockIdx.x == 0 && threadIdx.x == 0) grad_norm_out[0] = norm;
  }
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t t = chunks[3 * c], start = chunks[3 * c + 1];
    int64_t cnt = chunks[3 * c + 2];
    adp_adamw_tensor T = tensors[t];
    if (start + cnt > T.numel) cnt = T.numel - start;
    if (cnt <= 0) continue;
    T.p += start;
    T.g += start;
    T.m += start;
    T.v += start;
    if (T.ema) {
      T.ema += start;
      adamw_chunk<true>(s, clip, T, cnt);
    } else {
      adamw_chunk<false>(s, clip, T, cnt);
    }
  }
}

// ---- autoregressive v-diffusion (ARVDiffusion / ARVSampler): the window of T positions is cut into N splits of l = T / N
// positions and every split has its own noise level, which the net also reads as an extra input channel (the "sigma plane",
// [B, T]).  Work item = one (batch or batch-free, split, chunk of the split): blockIdx.x = (bs * gx + chunk).  A thread owns
// positions of ONE split and walks the channels (and, where the coefficients do not depend on the batch, the batch rows), so
// the per-split values are formed once per thread, not once per element.  VEC: l % 4 == 0 and every pointer is 16-byte
// aligned, so every (row, split) segment starts on a 16-byte boundary; else the scalar path.  Each element is read, then
// written, by the lane that owns it: x_out may be x.
template <bool VEC>
__global__ __launch_bounds__(256) void arv_noise_kernel(const float* x, const float* noise, const float* sigma, int64_t C,
                                                        int64_t T, int64_t N, int64_t gx, float* x_noisy, float* v_target,
                                                        float* plane) {
  const int64_t bs = blockIdx.x / gx, chunk = blockIdx.x - bs * gx;
  const int64_t b = bs / N, s = bs - b * N, l = T / N;
  const float sg = sigma[bs];
  // angle = sigma * pi / 2 evaluated left to right in fp32, as v_noise_kernel does
  const float angle = (sg * PI_F) / 2.0f;
  const float a = cosf(angle), bt = sinf(angle);
  const int64_t tid = chunk * 256 + threadIdx.x, nthreads = gx * 256;
  const int64_t seg = b * C * T + s * l;  // first element of channel 0's segment
  if (VEC) {
    for (int64_t j = 4 * tid; j < l; j += 4 * nthreads) {
      for (int64_t c = 0; c < C; ++c) {
        const int64_t i = seg + c * T + j;
        const f32x4 xv = *(const f32x4*)(x + i), nv = *(const f32x4*)(noise + i);
        f32x4 xn, vt;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          xn[k] = a * xv[k] + bt * nv[k];
          vt[k] = a * nv[k] - bt * xv[k];
        }
        *(f32x4*)(x_noisy + i) = xn;
        *(f32x4*)(v_target + i) = vt;
      }
      const f32x4 sv = {sg, sg, sg, sg};
      *(f32x4*)(plane + b * T + s * l + j) = sv;
    }
  } else {
    for (int64_t j = tid; j < l; j += nthreads) {
      for (int64_t c = 0; c < C; ++c) {
        const int64_t i = seg + c * T + j;
        const float xv = x[i], nv = noise[i];
        x_noisy[i] = a * xv + bt * nv;
        v_target[i] = a * nv - bt * xv;
      }
      plane[b * T + s * l + j] = sg;
    }
  }
}

struct ArvCoef {
  float a0, b0, a1, b1, sigma1;
};

__device__ __forceinline__ float arv_step_elem(const ArvCoef& c, float xv, float vv) {
  const float x_pred = c.a0 * xv - c.b0 * vv;  // (the operation order of v_step_kernel)
  const float n_pred = c.b0 * xv + c.a0 * vv;
  return c.a1 * x_pred + c.b1 * n_pred;
}

// blockIdx.x = s * gx + chunk: the coefficients are the split's, the same for every batch row and channel (rows = B * C)
template <bool VEC>
__global__ __launch_bounds__(256) void arv_step_kernel(const float* x, const float* v, const float* coef, int64_t B,
                                                       int64_t C, int64_t T, int64_t N, int64_t gx, float* xo,
                                                       float* plane) {
  const int64_t s = blockIdx.x / gx, chunk = blockIdx.x - s * gx;
  const int64_t l = T / N, rows = B * C;
  const float* row = coef + 5 * s;
  const ArvCoef c{row[0], row[1], row[2], row[3], row[4]};
  const int64_t tid = chunk * 256 + threadIdx.x, nthreads = gx * 256;
  if (VEC) {
    for (int64_t j = 4 * tid; j < l; j += 4 * nthreads) {
      for (int64_t r = 0; r < rows; ++r) {
        const int64_t i = r * T + s * l + j;
        const f32x4 xv = *(const f32x4*)(x + i), vv = *(const f32x4*)(v + i);
        f32x4 xn;
#pragma unroll
        for (int k = 0; k < 4; ++k) xn[k] = arv_step_elem(c, xv[k], vv[k]);
        *(f32x4*)(xo + i) = xn;
      }
      if (plane) {
        const f32x4 sv = {c.sigma1, c.sigma1, c.sigma1, c.sigma1};
        for (int64_t b = 0; b < B; ++b) *(f32x4*)(plane + b * T + s * l + j) = sv;
      }
    }
  } else {
    for (int64_t j = tid; j < l; j += nthreads) {
      for (int64_t r = 0; r < rows; ++r) {
        const int64_t i = r * T + s * l + j;
        xo[i] = arv_step_elem(c, x[i], v[i]);
      }
      if (plane)
        for (int64_t b = 0; b < B; ++b) plane[b * T + s * l + j] = c.sigma1;
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void arv_plane_kernel(const float* sigma, int64_t B, int64_t T, int64_t N, int64_t gx,
                                                        float* plane) {
  const int64_t s = blockIdx.x / gx, chunk = blockIdx.x - s * gx;
  const int64_t l = T / N;
  const float sg = sigma[s];
  const int64_t tid = chunk * 256 + threadIdx.x, nthreads = gx * 256;
  if (VEC) {
    const f32x4 sv = {sg, sg, sg, sg};
    for (int64_t j = 4 * tid; j < l; j += 4 * nthreads)
      for (int64_t b = 0; b < B; ++b) *(f32x4*)(plane + b * T + s * l + j) = sv;
  } else {
    for (int64_t j = tid; j < l; j += nthreads)
      for (int64_t b = 0; b < B; ++b) plane[b * T + s * l + j] = sg;
  }
}

// blocks per split: four positions per thread and pass; `units` splits (or batch x split pairs) share the launch
int64_t arv_grid(int64_t l, int64_t units) {
  int64_t gx = adp_cdiv(l, 256 * 4);
  const int64_t cap = adp_cdiv(4096, units);  // about the block count stream_grid allows
  if (gx > cap) gx = cap;
  return gx < 1 ? 1 : gx;
}

unsigned stream_grid(int64_t n) {
  int64_t g = adp_cdiv(n, 256 * 4);
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (unsigned)g;
}

}  // namespace

extern "C" int adp_version(void) { return 201; }

// ---- launch trace (profiling introspection; off by default, host-side only, per thread)
namespace {
thread_local bool g_trace_on = false;
thread_local char g_trace[4096];
thread_local size_t g_trace_len = 0;
#ifndef ADP_EMULATE
// The event list is process-wide (autograd runs the backward's launches on its own thread; the host code is
// serialised by the interpreter lock, so launches are appended in launch order).
constexpr int TRACE_EV_MAX = 8192;          // launches timed between two adp_launch_times calls
hipEvent_t g_ev[2 * TRACE_EV_MAX];
int g_ev_n = 0;                             // events recorded (two per launch)
std::mutex g_ev_mu;
#endif
}  // namespace

void adp_rt_note_launch(const char* kern, const char* site, void* stream) {
  if (!g_trace_on) return;
  const char* parts[4] = {g_trace_len ? "\n" : "", kern, "@", site};
  for (const char* p : parts)
    for (; *p && g_trace_len + 1 < sizeof(g_trace); ++p) g_trace[g_trace_len++] = *p;
  g_trace[g_trace_len] = 0;
#ifndef ADP_EMULATE
  std::lock_guard<std::mutex> lock(g_ev_mu);
  if (g_ev_n + 2 <= 2 * TRACE_EV_MAX) {
    hipEvent_t e;
    if (hipEventCreate(&e) == hipSuccess) {
      (void)hipEventRecord(e, (hipStream_t)stream);   // on the stream the kernel is launched on
      g_ev[g_ev_n++] = e;
    }
  }
#else
  (void)stream;
#endif
}

void adp_rt_launch_done(void* stream) {
#ifndef ADP_EMULATE
  if (!g_trace_on) return;
  std::lock_guard<std::mutex> lock(g_ev_mu);
  if ((g_ev_n & 1) == 0) return;
  hipEvent_t e;
  if (hipEventCreate(&e) == hipSuccess) {
    (void)hipEventRecord(e, (hipStream_t)stream);
    g_ev[g_ev_n++] = e;
  } else {  // keep the pairs aligned
    (void)hipEventDestroy(g_ev[--g_ev_n]);
  }
#else
  (void)stream;
#endif
}

extern "C" int64_t adp_launch_trace(int64_t enable, char* buf, int64_t cap) {
  int64_t n = 0;
  if (buf && cap > 0) {
    for (; n + 1 < cap && (size_t)n < g_trace_len; ++n) buf[n] = g_trace[n];
    buf[n] = 0;
  }
  g_trace_len = 0;
  g_trace[0] = 0;
  g_trace_on = enable != 0;
  return n;
}

extern "C" int64_t adp_launch_times(float* ms, int64_t cap) {
#ifndef ADP_EMULATE
  std::lock_guard<std::mutex> lock(g_ev_mu);
  const int pairs = g_ev_n / 2;
  int64_t n = 0;
  for (int i = 0; i < pairs; ++i) {
    float t = -1.0f;
    if (hipEventSynchronize(g_ev[2 * i + 1]) == hipSuccess) (void)hipEventElapsedTime(&t, g_ev[2 * i], g_ev[2 * i + 1]);
    if (ms && n < cap) ms[n++] = t;
    (void)hipEventDestroy(g_ev[2 * i]);
    (void)hipEventDestroy(g_ev[2 * i + 1]);
  }
  if (g_ev_n & 1) (void)hipEventDestroy(g_ev[g_ev_n - 1]);
  g_ev_n = 0;
  return n;
#else
  (void)ms;
  (void)cap;
  return 0;
#endif
}

extern "C" int adp_v_noise(const float* x, const float* noise, const float* sigma, int64_t B, int64_t per,
                           float* x_noisy, float* v_target, void* stream) {
  if (!x || !noise || !sigma || !x_noisy || !v_target) return ADP_ERR_NULL;
  if (B <= 0 || per <= 0 || B > 65535) return ADP_ERR_SHAPE;
  unsigned gx = stream_grid(per);
  ADP_LAUNCH(v_noise_kernel, dim3(gx, (unsigned)B), dim3(256), stream, x, noise, sigma, per, x_noisy, v_target);
  return ADP_LAUNCH_OK();
}

extern "C" int64_t adp_mse_ws_bytes(int64_t n) {
  (void)n;
  return MSE_BLOCKS * (int64_t)sizeof(float);
}

extern "C" int adp_mse_fwd(const float* v_pred, const float* v_target, int64_t n, float* loss, float* ws,
                           void* stream) {
  if (!v_pred || !v_target || !loss || !ws) return ADP_ERR_NULL;
  if (n <= 0) return ADP_ERR_SHAPE;
  int nb = (int)adp_cdiv(n, 256 * 8);
  if (nb > MSE_BLOCKS) nb = MSE_BLOCKS;
  ADP_LAUNCH(mse_partial_kernel, dim3((unsigned)nb), dim3(256), stream, v_pred, v_target, n, ws);
  ADP_LAUNCH(mse_final_kernel, dim3(1), dim3(64), stream, (const float*)ws, nb, n, loss);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_mse_bwd(const float* v_pred, const float* v_target, const float* gloss, int64_t n, float* dv,
                           void* stream) {
  if (!v_pred || !v_target || !dv) return ADP_ERR_NULL;
  if (n <= 0) return ADP_ERR_SHAPE;
  ADP_LAUNCH(mse_bwd_kernel, dim3(stream_grid(n)), dim3(256), stream, v_pred, v_target, gloss, n, dv);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_v_step(const float* x, const float* v, const float* ab4, int64_t n, float* x_out, void* stream) {
  if (!x || !v || !ab4 || !x_out) return ADP_ERR_NULL;
  if (n <= 0) return ADP_ERR_SHAPE;
  ADP_LAUNCH(v_step_kernel, dim3(stream_grid(n)), dim3(256), stream, x, v, ab4, n, x_out);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_v_step2(const float* x, const float* v, const float* hist_x0, const float* hist_eps,
                           const float* coef6, int64_t n, float* x_out, float* hist_x0_out, float* hist_eps_out,
                           void* stream) {
  if (!x || !v || !hist_x0 || !hist_eps || !coef6 || !x_out || !hist_x0_out || !hist_eps_out) return ADP_ERR_NULL;
  if (n <= 0) return ADP_ERR_SHAPE;
  const uintptr_t bits = (uintptr_t)x | (uintptr_t)v | (uintptr_t)hist_x0 | (uintptr_t)hist_eps | (uintptr_t)x_out |
                         (uintptr_t)hist_x0_out | (uintptr_t)hist_eps_out;
  if ((bits & 15) == 0)
    ADP_LAUNCH(v_step2_kernel<true>, dim3(stream_grid(n)), dim3(256), stream, x, v, hist_x0, hist_eps, coef6, n, x_out,
               hist_x0_out, hist_eps_out);
  else
    ADP_LAUNCH(v_step2_kernel<false>, dim3(stream_grid(n)), dim3(256), stream, x, v, hist_x0, hist_eps, coef6, n, x_out,
               hist_x0_out, hist_eps_out);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_arv_noise(const float* x, const float* noise, const float* sigma, int64_t B, int64_t C, int64_t T,
                             int64_t N, float* x_noisy, float* v_target, float* sigma_plane, void* stream) {
  if (!x || !noise || !sigma || !x_noisy || !v_target || !sigma_plane) return ADP_ERR_NULL;
  if (B <= 0 || C <= 0 || T <= 0 || N <= 0 || T % N != 0) return ADP_ERR_SHAPE;
  const int64_t l = T / N, gx = arv_grid(l, B * N);
  if (B * N * gx > 0x7fffffff) return ADP_ERR_SHAPE;
  const uintptr_t bits = (uintptr_t)x | (uintptr_t)noise | (uintptr_t)x_noisy | (uintptr_t)v_target | (uintptr_t)sigma_plane;
  if ((bits & 15) == 0 && l % 4 == 0)
    ADP_LAUNCH(arv_noise_kernel<true>, dim3((unsigned)(B * N * gx)), dim3(256), stream, x, noise, sigma, C, T, N, gx,
               x_noisy, v_target, sigma_plane);
  else
    ADP_LAUNCH(arv_noise_kernel<false>, dim3((unsigned)(B * N * gx)), dim3(256), stream, x, noise, sigma, C, T, N, gx,
               x_noisy, v_target, sigma_plane);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_arv_step(const float* x, const float* v, const float* coef, int64_t B, int64_t C, int64_t T, int64_t N,
                            float* x_out, float* sigma_plane_out, void* stream) {
  if (!x || !v || !coef || !x_out) return ADP_ERR_NULL;
  if (B <= 0 || C <= 0 || T <= 0 || N <= 0 || T % N != 0) return ADP_ERR_SHAPE;
  const int64_t l = T / N, gx = arv_grid(l, N);
  if (N * gx > 0x7fffffff) return ADP_ERR_SHAPE;
  const uintptr_t bits = (uintptr_t)x | (uintptr_t)v | (uintptr_t)x_out | (uintptr_t)sigma_plane_out;
  if ((bits & 15) == 0 && l % 4 == 0)
    ADP_LAUNCH(arv_step_kernel<true>, dim3((unsigned)(N * gx)), dim3(256), stream, x, v, coef, B, C, T, N, gx, x_out,
               sigma_plane_out);
  else
    ADP_LAUNCH(arv_step_kernel<false>, dim3((unsigned)(N * gx)), dim3(256), stream, x, v, coef, B, C, T, N, gx, x_out,
               sigma_plane_out);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_arv_plane(const float* sigma, int64_t B, int64_t T, int64_t N, float* sigma_plane, void* stream) {
  if (!sigma || !sigma_plane) return ADP_ERR_NULL;
  if (B <= 0 || T <= 0 || N <= 0 || T % N != 0) return ADP_ERR_SHAPE;
  const int64_t l = T / N, gx = arv_grid(l, N);
  if (N * gx > 0x7fffffff) return ADP_ERR_SHAPE;
  if (((uintptr_t)sigma_plane & 15) == 0 && l % 4 == 0)
    ADP_LAUNCH(arv_plane_kernel<true>, dim3((unsigned)(N * gx)), dim3(256), stream, sigma, B, T, N, gx, sigma_plane);
  else
    ADP_LAUNCH(arv_plane_kernel<false>, dim3((unsigned)(N * gx)), dim3(256), stream, sigma, B, T, N, gx, sigma_plane);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_v_inpaint_step(const float* x, const float* v, const float* source, const float* noise,
                                  const uint8_t* mask, const float* ab4, int64_t n, float* x_out, void* stream) {
  if (!x || !v || !source || !noise || !mask || !ab4 || !x_out) return ADP_ERR_NULL;
  if (n <= 0) return ADP_ERR_SHAPE;
  ADP_LAUNCH(v_inpaint_kernel, dim3(stream_grid(n)), dim3(256), stream, x, v, source, noise, mask, ab4, n, x_out);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_cfg_mix(const float* y, int64_t half, float scale, float* out, void* stream) {
  if (!y || !out) return ADP_ERR_NULL;
  if (half <= 0) return ADP_ERR_SHAPE;
  ADP_LAUNCH(cfg_mix_kernel, dim3(stream_grid(half)), dim3(256), stream, y, half, scale, out);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_select_rows(const float* a, const float* b, const uint8_t* pick, int64_t rows, int64_t per,
                               float* out, void* stream) {
  if (!a || !b || !pick || !out) return ADP_ERR_NULL;
  if (rows <= 0 || per <= 0) return ADP_ERR_SHAPE;
  ADP_LAUNCH(select_rows_kernel, dim3(stream_grid(rows * per)), dim3(256), stream, a, b, pick, rows, per, out);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_add(const float* a, const float* b, int64_t n, float* y, void* stream) {
  if (!a || !b || !y) return ADP_ERR_NULL;
  if (n <= 0) return ADP_ERR_SHAPE;
  ADP_LAUNCH(add_kernel, dim3(stream_grid(n)), dim3(256), stream, a, b, n, y);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_axpby(float a, const float* x, float b, const float* y, int64_t n, float* out, void* stream) {
  if (!x || !out) return ADP_ERR_NULL;
  if (n <= 0) return ADP_ERR_SHAPE;
  ADP_LAUNCH(axpby_kernel, dim3(stream_grid(n)), dim3(256), stream, a, x, b, y, n, out);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_copy2d(const float* src, int64_t src_stride, float* dst, int64_t dst_stride, int64_t rows,
                          int64_t cols, void* stream) {
  if (!src || !dst) return ADP_ERR_NULL;
  if (rows <= 0 || cols <= 0 || src_stride < cols || dst_stride < cols) return ADP_ERR_SHAPE;
  ADP_LAUNCH(copy2d_kernel, dim3(stream_grid(rows * cols)), dim3(256), stream, src, src_stride, dst, dst_stride, rows,
             cols);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_unshuffle(const float* x, int64_t rows, int64_t L, int64_t f, float* out, void* stream) {
  if (!x || !out) return ADP_ERR_NULL;
  if (rows <= 0 || L <= 0 || f < 1 || L % f != 0) return ADP_ERR_SHAPE;
  ADP_LAUNCH(unshuffle_kernel, dim3(stream_grid(rows * L)), dim3(256), stream, x, rows, L / f, f, out);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_pool_sum(const float* x, int64_t rows, int64_t Lout, int64_t f, const float* res, float* out,
                            void* stream) {
  if (!x || !out) return ADP_ERR_NULL;
  if (rows <= 0 || Lout <= 0 || f < 1) return ADP_ERR_SHAPE;
  ADP_LAUNCH(pool_sum_kernel, dim3(stream_grid(rows * Lout)), dim3(256), stream, x, rows, Lout, f, res, out);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_act_fwd(const float* x, int64_t n, int64_t act, float* y, void* stream) {
  if (!x || !y) return ADP_ERR_NULL;
  if (n <= 0 || act < 0 || act > 2) return ADP_ERR_SHAPE;
  ADP_LAUNCH(act_fwd_kernel, dim3((unsigned)adp_cdiv(n, 256)), dim3(256), stream, x, n, (int)act, y);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_act_bwd(const float* x, const float* dy, int64_t n, int64_t act, int64_t accumulate, float* dx,
                           void* stream) {
  if (!x || !dy || !dx) return ADP_ERR_NULL;
  if (n <= 0 || act < 0 || act > 2) return ADP_ERR_SHAPE;
  ADP_LAUNCH(act_bwd_kernel, dim3((unsigned)adp_cdiv(n, 256)), dim3(256), stream, x, dy, n, (int)act,
             (int)accumulate, dx);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_time_fourier_fwd(const float* t, const float* w, int64_t B, int64_t H, float* four, void* stream) {
  if (!t || !w || !four) return ADP_ERR_NULL;
  if (B <= 0 || H <= 0) return ADP_ERR_SHAPE;
  ADP_LAUNCH(fourier_fwd_kernel, dim3((unsigned)adp_cdiv(B * H, 256)), dim3(256), stream, t, w, B, H, four);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_time_fourier_bwd(const float* t, const float* w, const float* dfour, int64_t B, int64_t H,
                                    int64_t accumulate, float* dw, void* stream) {
  if (!t || !w || !dfour || !dw) return ADP_ERR_NULL;
  if (B <= 0 || H <= 0) return ADP_ERR_SHAPE;
  ADP_LAUNCH(fourier_bwd_kernel, dim3((unsigned)adp_cdiv(H, 256)), dim3(256), stream, t, w, dfour, B, H,
             (int)accumulate, dw);
  return ADP_LAUNCH_OK();
}

extern "C" int64_t adp_sqnorm_partials(const float* const* ptrs, const int64_t* numels, int64_t n_tensors,
                                       const int64_t* chunk_table, int64_t n_chunks, double* partials, void* stream) {
  if (!ptrs || !numels || !chunk_table || !partials) return ADP_ERR_NULL;
  if (n_tensors <= 0 || n_chunks <= 0) return ADP_ERR_SHAPE;
  const int64_t nb = n_chunks < OPT_MAX_PARTIALS ? n_chunks : OPT_MAX_PARTIALS;
  ADP_LAUNCH(sqnorm_partials_kernel, dim3((unsigned)nb), dim3(256), stream, ptrs, numels, chunk_table, n_chunks,
             partials);
  return ADP_LAUNCH_OK() == ADP_OK ? nb : ADP_ERR_LAUNCH;
}

extern "C" int adp_adamw_step(const adp_adamw_tensor* tensors, const int64_t* chunk_table, int64_t n_chunks, float decay,
                              float one_minus_beta1, float beta2, float one_minus_beta2, float inv_bc2_sqrt, float eps,
                              float step_size, float ema_weight, const double* partials, int64_t n_partials,
                              float max_grad_norm, float* grad_norm_out, void* stream) {
  if (!tensors || !chunk_table) return ADP_ERR_NULL;
  if (n_chunks <= 0 || (partials && (n_partials <= 0 || n_partials > OPT_MAX_PARTIALS))) return ADP_ERR_SHAPE;
  const AdamwScalars s{decay, one_minus_beta1, beta2, one_minus_beta2, inv_bc2_sqrt, eps, step_size, ema_weight};
  const int64_t nb = n_chunks < 4096 ? n_chunks : 4096;
  ADP_LAUNCH(adamw_step_kernel, dim3((unsigned)nb), dim3(256), stream, tensors, chunk_table, n_chunks, s, partials,
             (int)n_partials, max_grad_norm, grad_norm_out);
  return ADP_LAUNCH_OK();
}
