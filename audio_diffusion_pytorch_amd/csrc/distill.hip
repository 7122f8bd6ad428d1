// Progressive distillation (include/adp_distill.h): the per-item combination behind the teacher's mid point and the
// student's target, and the per-item weighted squared error with its gradient.
//   adp_distill_comb     : out = c0 x + c1 p [+ c2 q]                          2 or 3 reads, 1 write
//   adp_distill_wmse_fwd : loss = (1 / n) sum_r w_r sum_e (pred - target)^2    2 reads; partials, then one final block
//   adp_distill_wmse_bwd : dv = (gloss 2 / n) w_r (pred - target)              2 reads, 1 write
// The combination is a pass of csrc/sampler_update.h's for_groups4.  The two loss kernels write the same pass out (through
// for_groups4 their unweighted forms measured outside the parent's spread) and are kept in step with it by hand; the one use
// of LDS is the block sum of the loss partials (adp_block_sum, as adp_mse_fwd's).  The host checks are that header's too.
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
  const In in[] = {x, p, {q, THREE}};
  const Out outs[] = {out};
  struct Group {
    float c0[4], c1[4], c2[4];
  };
  for_groups4<VEC>(
      in, outs, n,
      [&](int64_t, int64_t e, bool) {
        Group c{{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
        item_values4(coef, e, n, per, c.c0);
        item_values4(coef + rows, e, n, per, c.c1);
        if (THREE) item_values4(coef + 2 * rows, e, n, per, c.c2);
        return c;
      },
      [&](const Group& c, int k, const float(&a)[3], float(&o)[1]) {
        o[0] = comb_elem<THREE>(c.c0[k], c.c1[k], c.c2[k], a[0], a[1], a[2]);
      });
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
  if (terms == 3 && !q) return ADP_ERR_NULL;
  const bool own_ok = (terms == 2 || terms == 3) && !(terms == 2 && q);
  const int64_t n = flat_count({x, p, coef, out}, {q}, rows, per, own_ok);
  if (n <= 0) return (int)n;
  const bool vec = aligned16({x, p, q, out});
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
  const int64_t n = flat_count({v_pred, v_target, loss, ws}, {w}, rows, per);
  if (n <= 0) return (int)n;
  const bool vec = aligned16({v_pred, v_target});
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
  const int64_t n = flat_count({v_pred, v_target, dv}, {w, gloss}, rows, per);
  if (n <= 0) return (int)n;
  const bool vec = aligned16({v_pred, v_target, dv});
  with_flag(w != nullptr, [&](auto WEIGHTED) {
    with_flag(vec, [&](auto VEC) {
      ADP_LAUNCH((distill_wmse_bwd_kernel<WEIGHTED(), VEC()>), dim3(grid4(n)), dim3(256), stream, v_pred, v_target, w,
                 gloss, n, per, dv);
    });
  });
  return ADP_LAUNCH_OK();
}
