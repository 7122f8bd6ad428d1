// Progressive distillation (include/adp_distill.h): the per-item combination behind the teacher's mid point and the
// student's target, and the per-item weighted squared error with its gradient.
//   adp_distill_comb     : out = c0 x + c1 p [+ c2 q]                          2 or 3 reads, 1 write
//   adp_distill_wmse_fwd : loss = (1 / n) sum_r w_r sum_e (pred - target)^2    2 reads; partials, then one final block
//   adp_distill_wmse_bwd : dv = (gloss 2 / n) w_r (pred - target)              2 reads, 1 write
// All are bandwidth-bound elementwise passes of rf_noise_kernel's shape (rf.hip): one thread owns one group of four elements
// per pass, in a grid-stride loop over the groups; 16-byte accesses where every tensor operand allows them, single elements
// otherwise.  The per-item values (coefficients, weights) are found by item_values4.  No atomics; the one use of LDS is the
// block sum of the loss partials (adp_block_sum, as adp_mse_fwd's); ordinary vector or single-element stores only.  The walk,
// the grid and the host checks are csrc/sampler_update.h's.
#include "adp_rt.h"
#include "adp.h"
#include "adp_distill.h"
#include "sampler_update.h"

namespace {

using namespace upd;

// ---- the combination, by the rounding sequence of the header: the two-term value is the three-term one's intermediate
template <bool THREE>
__device__ __forceinline__ float comb_elem(float c0, float c1, float c2, float xv, float pv, float qv) {
  const float t = fma_rn(c1, pv, c0 * xv);
  return THREE ? fma_rn(c2, qv, t) : t;
}

// VEC: x, p, out (and q for THREE) are 16-byte aligned.  coef is planar [terms, rows]: plane k is a per-item table.
template <bool THREE, bool VEC>
__global__ __launch_bounds__(256) void distill_comb_kernel(const float* x, const float* p, const float* q,
                                                           const float* coef, int64_t rows, int64_t n, int64_t per,
                                                           float* out) {
  const int64_t groups = groups4(n);
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t e = 4 * g;
    float c0[4] = {0.0f, 0.0f, 0.0f, 0.0f}, c1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, c2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    item_values4(coef, e, n, per, c0);
    item_values4(coef + rows, e, n, per, c1);
    if (THREE) item_values4(coef + 2 * rows, e, n, per, c2);
    if (VEC && e + 4 <= n) {
      const f32x4 xv = *(const f32x4*)(x + e), pv = *(const f32x4*)(p + e);
      f32x4 qv = {0.0f, 0.0f, 0.0f, 0.0f};
      if (THREE) qv = *(const f32x4*)(q + e);
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = comb_elem<THREE>(c0[k], c1[k], c2[k], xv[k], pv[k], qv[k]);
      *(f32x4*)(out + e) = o;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < n) {
          const float qv = THREE ? q[e + k] : 0.0f;  // (every operand read before the store: aliasing)
          const float xv = x[e + k], pv = p[e + k];
          out[e + k] = comb_elem<THREE>(c0[k], c1[k], c2[k], xv, pv, qv);
        }
    }
  }
}

// ---- the weighted squared error.  A lane adds its elements in element order, pass by pass: the 16-byte and the
// single-element form accumulate the same sequence, so the partials do not depend on the pointers' alignment.
constexpr int WMSE_BLOCKS = 1024;

template <bool WEIGHTED, bool VEC>
__global__ __launch_bounds__(256) void distill_wmse_partial_kernel(const float* pr, const float* tg, const float* w,
                                                                   int64_t n, int64_t per, float* ws) {
  __shared__ float sh[4];
  float s = 0.0f;
  const int64_t groups = groups4(n);
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t e = 4 * g;
    float wv[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (WEIGHTED) item_values4(w, e, n, per, wv);
    if (VEC && e + 4 <= n) {
      const f32x4 a = *(const f32x4*)(pr + e), b = *(const f32x4*)(tg + e);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = a[k] - b[k];
        s = fma_rn(wv[k] * d, d, s);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < n) {
          const float d = pr[e + k] - tg[e + k];
          s = fma_rn(wv[k] * d, d, s);
        }
    }
  }
  s = adp_block_sum<4>(s, sh);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

// one wave: lane l sums partials l, l + 64, ... in double, then lane 0 adds the 64 lane sums in lane order (mse_final_kernel
// of elementwise.hip): a fixed order
__global__ __launch_bounds__(64) void distill_wmse_final_kernel(const float* ws, int nb, int64_t n, float* loss) {
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

template <bool WEIGHTED, bool VEC>
__global__ __launch_bounds__(256) void distill_wmse_bwd_kernel(const float* pr, const float* tg, const float* w,
                                                               const float* gloss, int64_t n, int64_t per, float* dv) {
  const float sc = (gloss ? gloss[0] : 1.0f) * 2.0f / (float)n;
  const int64_t groups = groups4(n);
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t e = 4 * g;
    float wv[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (WEIGHTED) item_values4(w, e, n, per, wv);
    if (VEC && e + 4 <= n) {
      const f32x4 a = *(const f32x4*)(pr + e), b = *(const f32x4*)(tg + e);
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = (sc * wv[k]) * (a[k] - b[k]);
      *(f32x4*)(dv + e) = o;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < n) {
          const float d = pr[e + k] - tg[e + k];  // (both read before the store: aliasing)
          dv[e + k] = (sc * wv[k]) * d;
        }
    }
  }
}

inline int wmse_blocks(int64_t n) {
  const unsigned g = grid4(n);
  return g > (unsigned)WMSE_BLOCKS ? WMSE_BLOCKS : (int)g;
}

}  // namespace

extern "C" int adp_distill_comb(const float* x, const float* p, const float* q, const float* coef, int64_t terms,
                                int64_t rows, int64_t per, float* out, void* stream) {
  if (!x || !p || !coef || !out) return ADP_ERR_NULL;
  if (terms == 3 && !q) return ADP_ERR_NULL;
  if (rows < 0 || per < 0 || (terms != 2 && terms != 3) || (terms == 2 && q)) return ADP_ERR_SHAPE;
  if (count_overflows(rows, per)) return ADP_ERR_SHAPE;
  if (misaligned(x, 4) || misaligned(p, 4) || (q && misaligned(q, 4)) || misaligned(coef, 4) || misaligned(out, 4))
    return ADP_ERR_ALIGN;
  const int64_t n = rows * per;
  if (n == 0) return ADP_OK;
  const bool vec = !misaligned(x, 16) && !misaligned(p, 16) && (!q || !misaligned(q, 16)) && !misaligned(out, 16);
  with_flag(terms == 3, [&](auto THREE) {
    with_flag(vec, [&](auto VEC) {
      ADP_LAUNCH((distill_comb_kernel<THREE(), VEC()>), dim3(grid4(n)), dim3(256), stream, x, p, q, coef, rows, n, per, out);
    });
  });
  return ADP_LAUNCH_OK();
}

extern "C" int64_t adp_distill_wmse_ws_bytes(int64_t rows, int64_t per) {
  if (rows < 0 || per < 0 || count_overflows(rows, per)) return ADP_ERR_SHAPE;
  return WMSE_BLOCKS * (int64_t)sizeof(float);
}

extern "C" int adp_distill_wmse_fwd(const float* v_pred, const float* v_target, const float* w, int64_t rows, int64_t per,
                                    float* loss, float* ws, void* stream) {
  if (!v_pred || !v_target || !loss || !ws) return ADP_ERR_NULL;
  if (rows < 0 || per < 0) return ADP_ERR_SHAPE;
  if (count_overflows(rows, per)) return ADP_ERR_SHAPE;
  if (misaligned(v_pred, 4) || misaligned(v_target, 4) || (w && misaligned(w, 4)) || misaligned(loss, 4) ||
      misaligned(ws, 4))
    return ADP_ERR_ALIGN;
  const int64_t n = rows * per;
  if (n == 0) return ADP_OK;
  const bool vec = !misaligned(v_pred, 16) && !misaligned(v_target, 16);
  const int nb = wmse_blocks(n);
  with_flag(w != nullptr, [&](auto WEIGHTED) {
    with_flag(vec, [&](auto VEC) {
      ADP_LAUNCH((distill_wmse_partial_kernel<WEIGHTED(), VEC()>), dim3((unsigned)nb), dim3(256), stream, v_pred, v_target,
                 w, n, per, ws);
    });
  });
  ADP_LAUNCH(distill_wmse_final_kernel, dim3(1), dim3(64), stream, (const float*)ws, nb, n, loss);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_distill_wmse_bwd(const float* v_pred, const float* v_target, const float* w, const float* gloss,
                                    int64_t rows, int64_t per, float* dv, void* stream) {
  if (!v_pred || !v_target || !dv) return ADP_ERR_NULL;
  if (rows < 0 || per < 0) return ADP_ERR_SHAPE;
  if (count_overflows(rows, per)) return ADP_ERR_SHAPE;
  if (misaligned(v_pred, 4) || misaligned(v_target, 4) || (w && misaligned(w, 4)) || (gloss && misaligned(gloss, 4)) ||
      misaligned(dv, 4))
    return ADP_ERR_ALIGN;
  const int64_t n = rows * per;
  if (n == 0) return ADP_OK;
  const bool vec = !misaligned(v_pred, 16) && !misaligned(v_target, 16) && !misaligned(dv, 16);
  with_flag(w != nullptr, [&](auto WEIGHTED) {
    with_flag(vec, [&](auto VEC) {
      ADP_LAUNCH((distill_wmse_bwd_kernel<WEIGHTED(), VEC()>), dim3(grid4(n)), dim3(256), stream, v_pred, v_target, w,
                 gloss, n, per, dv);
    });
  });
  return ADP_LAUNCH_OK();
}
