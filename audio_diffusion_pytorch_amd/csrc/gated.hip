// The gated feed-forward GEMM of T5 v1.1 / flan-T5 (include/adp_gated.h): both projections of the gated feed-forward and
// the gate itself in one kernel.  fp32, exact-f32 matrix cores (v_mfma_f32_32x32x2_f32), forward only.
//
//   y[t, f] = act(sum_k x[t, k] w_gate[f, k]) * (sum_k x[t, k] w_up[f, k])        T x K x F, every operand k-contiguous
//
// The geometry is t5_linear_kernel's (csrc/t5.hip): 256 threads, k chunks of 32 staged as [64][32 + 1], the next chunk loaded
// into registers before the current chunk's matrix work and written to LDS after it, one 32 x 32 accumulator per wave.  A
// workgroup owns 64 tokens x 32 features: rows 0-31 of its weight tile are w_gate[f0 ..], rows 32-63 are w_up[f0 ..], so the
// activations are staged once for both products, wave column 0 accumulates the gate and wave column 1 the up product of the
// SAME 32 features.  Where the whole k sum is the workgroup's, the four waves drop their accumulators into the (now idle)
// staging LDS as four [32][33] tiles, and after one barrier each wave gates 16 of its token half's 32 rows and writes them
// as 32-float rows.  Where the k sum is cut over gridDim.z (the rule of t5_linear_plan: the 64 x 32 tiles alone are 64 .. 512
// workgroups on 256 CUs at the encoder's shapes), both raw partial products go to the workspace [segment][gate | up][T][F]
// and a second launch adds them in segment order and then applies the gate: act() is not linear, so it is applied only where
// the whole sum is known.  All loads are predicated and all tails (tokens, k, features) are zeros written into LDS.
#include <math.h>
#include <stdlib.h>
#include "adp_rt.h"
#include "adp_gated.h"

namespace {

constexpr int GL_T = 64;            // tokens per workgroup = rows of the weight tile (32 gate + 32 up)
constexpr int GL_F = 32;            // features per workgroup
constexpr int GL_KC = 32;           // k chunk between barriers
constexpr int GL_S = GL_KC + 1;     // the LDS row stride
constexpr int GL_PER = GL_T * GL_KC / 256;   // elements of one operand a thread stages per chunk

__device__ __forceinline__ f32x16 gl_zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.0f;
  return z;
}
// row of accumulator register r in a 32x32 fragment (the column is lane & 31)
__device__ __forceinline__ int gl_frag_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// 0.5 g (1 + tanh(sqrt(2 / pi) (g + 0.044715 g^3))): finite for every finite g (g^3 may be an infinity, tanh of it is +-1)
__device__ __forceinline__ float gl_gelu_new(float g) {
  return 0.5f * g * (1.0f + tanhf(0.7978845608028654f * (g + 0.044715f * g * g * g)));
}

// elements tid + 256 j of the [64][32] activation chunk: row (tid >> 5) + 8 j, k offset tid & 31
__device__ __forceinline__ void gl_fetch_x(const float* x, int64_t T, int64_t K, int64_t t0, int64_t k0, int64_t k_hi, int tid,
                                           float* reg) {
  const int64_t k = k0 + (tid & 31);
#pragma unroll
  for (int j = 0; j < GL_PER; ++j) {
    const int64_t t = t0 + (tid >> 5) + 8 * j;
    reg[j] = (t < T && k < k_hi) ? x[t * K + k] : 0.0f;
  }
}
// the same elements of the weight chunk: rows 0-31 (j < 4) are w_gate[f0 + row], rows 32-63 are w_up[f0 + row - 32]
__device__ __forceinline__ void gl_fetch_w(const float* wg, const float* wu, int64_t F, int64_t K, int64_t f0, int64_t k0,
                                           int64_t k_hi, int tid, float* reg) {
  const int64_t k = k0 + (tid & 31);
#pragma unroll
  for (int j = 0; j < GL_PER; ++j) {
    const int64_t f = f0 + (tid >> 5) + 8 * (j & 3);
    const float* w = (j < 4) ? wg : wu;
    reg[j] = (f < F && k < k_hi) ? w[f * K + k] : 0.0f;
  }
}

// DIRECT: the whole k sum is this workgroup's -- out is y and the gate is applied here; otherwise out is the partial buffer
// [segment][gate | up][T][F] and the gate is gated_sum_kernel's
template <bool DIRECT>
__global__ __launch_bounds__(256) void gated_linear_kernel(const float* x, const float* wg, const float* wu, int64_t T, int64_t K,
                                                           int64_t F, int64_t KS, float* out) {
  __shared__ float sm[2 * GL_T * GL_S];   // the two staged operands; in the DIRECT epilogue the four accumulator tiles
  float* xs = sm;
  float* wl = sm + GL_T * GL_S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1, h = lane >> 5, c = lane & 31;   // wn 0: the gate product, 1: the up product
  const int64_t f0 = (int64_t)blockIdx.x * GL_F, t0 = (int64_t)blockIdx.y * GL_T, sg = blockIdx.z;
  const int64_t k_lo = sg * KS, k_hi = (k_lo + KS < K) ? k_lo + KS : K;
  float xr[GL_PER], wr[GL_PER];
  gl_fetch_x(x, T, K, t0, k_lo, k_hi, tid, xr);
  gl_fetch_w(wg, wu, F, K, f0, k_lo, k_hi, tid, wr);
  f32x16 acc = gl_zero16();
  for (int64_t k0 = k_lo; k0 < k_hi; k0 += GL_KC) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < GL_PER; ++j) {
      xs[((tid >> 5) + 8 * j) * GL_S + (tid & 31)] = xr[j];
      wl[((tid >> 5) + 8 * j) * GL_S + (tid & 31)] = wr[j];
    }
    __syncthreads();
    if (k0 + GL_KC < k_hi) {   // the next chunk travels while this one is multiplied
      gl_fetch_x(x, T, K, t0, k0 + GL_KC, k_hi, tid, xr);
      gl_fetch_w(wg, wu, F, K, f0, k0 + GL_KC, k_hi, tid, wr);
    }
    const float* xa = xs + (wm * 32 + c) * GL_S + h;
    const float* wb = wl + (wn * 32 + c) * GL_S + h;
#pragma unroll
    for (int k2 = 0; k2 < GL_KC; k2 += 2) acc = adp_mfma32(xa[k2], wb[k2], acc);
  }
  const int64_t f = f0 + c;
  if (!DIRECT) {
    float* plane = out + (sg * 2 + wn) * T * F;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t t = t0 + wm * 32 + gl_frag_row(r, lane);
      if (t < T && f < F) plane[t * F + f] = acc[r];
    }
    return;
  }
  // tile `wave` of sm: this wave's 32 x 32 accumulator, [token][feature + 1]
  __syncthreads();   // every wave has read its last fragments of xs / wl
  float* mine = sm + wave * 32 * GL_S;
#pragma unroll
  for (int r = 0; r < 16; ++r) mine[gl_frag_row(r, lane) * GL_S + c] = acc[r];
  __syncthreads();
  const float* gt = sm + wm * 32 * GL_S;         // the gate tile of this token half (wave wm)
  const float* ut = sm + (wm + 2) * 32 * GL_S;   // its up tile (wave wm + 2)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = wn * 16 + 2 * i + h;         // the two waves of a token half take 16 rows each
    const int64_t t = t0 + wm * 32 + row;
    if (t < T && f < F) out[t * F + f] = gl_gelu_new(gt[row * GL_S + c]) * ut[row * GL_S + c];
  }
}

// y[i] = act(gate[0][i] + gate[1][i] + ...) * (up[0][i] + up[1][i] + ...), both sums in increasing segment order
__global__ __launch_bounds__(256) void gated_sum_kernel(const float* part, int64_t n, int ns, float* y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float g = part[i], u = part[n + i];
  for (int r = 1; r < ns; ++r) {
    g += part[(int64_t)(2 * r) * n + i];
    u += part[(int64_t)(2 * r + 1) * n + i];
  }
  y[i] = gl_gelu_new(g) * u;
}

// --------------------------------------------------------------------------------------------------------------- host
struct GatedPlan {
  int64_t KS;   // k elements per segment (whole chunks of GL_KC)
  int ns;       // segments
};

constexpr int64_t GL_MAX = ((int64_t)1 << 31) - 1;

// a, b >= 1: a * b <= GL_MAX without overflow
bool gl_fits(int64_t a, int64_t b) { return a <= GL_MAX / b; }

int gated_plan(int64_t T, int64_t K, int64_t F, GatedPlan* g) {
  if (T < 1 || K < 1 || F < 1) return ADP_ERR_SHAPE;
  if (T > GL_MAX || K > GL_MAX || F > GL_MAX || !gl_fits(T, K) || !gl_fits(F, K) || !gl_fits(T, F)) return ADP_ERR_SHAPE;
  if (adp_cdiv(T, GL_T) > 65535) return ADP_ERR_SHAPE;
  // about 512 workgroups over (tiles, segments); a segment is whole chunks of GL_KC and at least 128 long
  const int64_t tiles = adp_cdiv(T, GL_T) * adp_cdiv(F, GL_F);
  int64_t ns = adp_cdiv(512, tiles);
  if (ns > adp_cdiv(K, 128)) ns = adp_cdiv(K, 128);
  if (ns < 1) ns = 1;
  const int64_t KS = adp_cdiv(adp_cdiv(K, ns), GL_KC) * GL_KC;
  ns = adp_cdiv(K, KS);
  if (ns > 1 && 2 * ns * T > GL_MAX / F) return ADP_ERR_SHAPE;   // the partial buffer is a tensor like the others
  g->KS = KS;
  g->ns = (int)ns;
  return ADP_OK;
}

}  // namespace

extern "C" int64_t adp_gated_linear_ws_bytes(int64_t T, int64_t K, int64_t F) {
  GatedPlan g;
  const int rc = gated_plan(T, K, F, &g);
  if (rc != ADP_OK) return rc;
  return g.ns > 1 ? 2 * (int64_t)g.ns * T * F * (int64_t)sizeof(float) : 0;
}

extern "C" int adp_gated_linear(const float* x, const float* w_gate, const float* w_up, int64_t T, int64_t K, int64_t F,
                                int64_t act, float* y, float* ws, void* stream) {
  if (!x || !w_gate || !w_up || !y) return ADP_ERR_NULL;
  GatedPlan g;
  const int rc = gated_plan(T, K, F, &g);
  if (rc != ADP_OK) return rc;
  if (g.ns > 1 && !ws) return ADP_ERR_NULL;
  if (act != ADP_GATED_ACT_GELU_NEW) return ADP_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)adp_cdiv(F, GL_F), (unsigned)adp_cdiv(T, GL_T), (unsigned)g.ns);
  if (g.ns == 1) {
    ADP_LAUNCH(gated_linear_kernel<true>, grid, dim3(256), stream, x, w_gate, w_up, T, K, F, g.KS, y);
  } else {
    ADP_LAUNCH(gated_linear_kernel<false>, grid, dim3(256), stream, x, w_gate, w_up, T, K, F, g.KS, ws);
    ADP_LAUNCH(gated_sum_kernel, dim3((unsigned)adp_cdiv(T * F, 256)), dim3(256), stream, (const float*)ws, T * F, g.ns, y);
  }
  return ADP_LAUNCH_OK();
}
