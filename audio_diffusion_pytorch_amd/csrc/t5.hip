// The kernels of the frozen T5 text encoder (include/adp_t5.h): the embedding row gather, T5's RMS LayerNorm, the bias-free
// token GEMM with ReLU / residual epilogue, and self-attention with the relative-position bias.  fp32, exact-f32 matrix cores
// (v_mfma_f32_32x32x2_f32), forward only.
//
//   linear   y[t, n] = res[t, n] + act(sum_k x[t, k] w[n, k])          GEMM  T x K x N, both operands k-contiguous
//   attn     S^T = K Q^T + bias + mask ; P^T = softmax over keys ; O^T = V^T P^T      per (batch row, head, 32 queries)
//
// linear: 256 threads, a 64 x 64 block tile, one 32 x 32 accumulator per wave (the f32 instruction's issue interval equals its
// dependent latency, so one accumulator keeps the pipe full), k chunks of 32 staged as [64][32 + 1] (odd stride: the 32 rows a
// fragment reads fall on 32 banks).  The next chunk is loaded into registers before the current chunk's matrix work and
// written to LDS after it.  At the encoder's shapes (T = 64 .. 512 tokens against 768 x 768 .. 768 x 3072 weights) the tiles
// alone are 12 .. 200 workgroups on 256 CUs, so the k sum is cut over gridDim.z and the partials are added in segment order by
// a second launch that also applies the epilogue.
//
// attn: ONE wave per workgroup and 32 queries per wave.  The scores are computed TRANSPOSED (keys on the accumulator's rows,
// the query on its lane), so that everything a query's softmax needs sits in the two lanes c and c + 32: the row maximum and
// sum are 15 in-lane operations and one cross-half exchange, the running rescale of the online softmax is a per-lane
// multiply, and the probabilities P^T are already the B fragments of O^T = V^T P^T (register r of lane half h is key
// (r & 3) + 8 (r >> 2) + 4 h of the tile in both the accumulator layout and, by choice, in the k slot of the next product),
// so P never moves.  K tiles go through LDS ([32][dk + 1], coalesced loads); V^T fragments are read from global directly: the
// 32 lanes of a fragment read 32 consecutive floats of one token.  O^T is transposed through LDS for row-contiguous stores.
// All loads are predicated and all tails (tokens, features, rows below a tile) are zeros written into LDS or registers.
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include "adp_rt.h"
#include "adp_t5.h"

namespace {

constexpr int TL_T = 64;            // linear: block tile edge
constexpr int TL_KC = 32;           // linear: k chunk between barriers
constexpr int TL_S = TL_KC + 1;     // its LDS row stride
constexpr int TL_PER = TL_T * TL_KC / 256;   // elements of one operand a thread stages per chunk
constexpr int TA_Q = 32;            // attn: queries per wave = keys per tile
constexpr int TA_MAXD = 128;        // attn: dk limit
constexpr int TA_S = TA_MAXD + 1;   // its LDS row stride
constexpr int TA_MAXM = 512;        // attn: token limit

__device__ __forceinline__ f32x16 t5_zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.0f;
  return z;
}
// row of accumulator register r in a 32x32 fragment (the column is lane & 31)
__device__ __forceinline__ int t5_frag_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// --------------------------------------------------------------------------------------------------------------- embed
__global__ __launch_bounds__(256) void t5_embed_kernel(const int64_t* ids, const float* table, int64_t V, int64_t d, float* out) {
  const int64_t t = blockIdx.x, id = ids[t];
  const bool ok = id >= 0 && id < V;
  for (int64_t c = threadIdx.x; c < d; c += 256) out[t * d + c] = ok ? table[id * d + c] : 0.0f;
}

// ------------------------------------------------------------------------------------------------------------- rmsnorm
// one workgroup per row: a thread-strided sum of squares in a fixed order, the wave and block sums, then the scaled row
__global__ __launch_bounds__(256) void t5_rmsnorm_kernel(const float* x, const float* g, int64_t d, float eps, float* y) {
  __shared__ float sh[4];
  const float* xr = x + (int64_t)blockIdx.x * d;
  float* yr = y + (int64_t)blockIdx.x * d;
  float s = 0.0f;
  for (int64_t c = threadIdx.x; c < d; c += 256) s += xr[c] * xr[c];
  s = adp_block_sum<4>(s, sh);
  const float r = rsqrtf(s / (float)d + eps);
  for (int64_t c = threadIdx.x; c < d; c += 256) yr[c] = xr[c] * r * g[c];
}

// -------------------------------------------------------------------------------------------------------------- linear
struct T5LinPlan {
  int64_t KS;   // k elements per segment (whole chunks of TL_KC)
  int ns;       // segments
};

// elements tid + 256 j of a [64][32] operand chunk: row (tid >> 5) + 8 j, k offset tid & 31
__device__ __forceinline__ void t5_lin_fetch(const float* a, int64_t rows, int64_t K, int64_t r0, int64_t k0, int64_t k_hi,
                                             int tid, float* reg) {
  const int64_t k = k0 + (tid & 31);
#pragma unroll
  for (int j = 0; j < TL_PER; ++j) {
    const int64_t r = r0 + (tid >> 5) + 8 * j;
    reg[j] = (r < rows && k < k_hi) ? a[r * K + k] : 0.0f;
  }
}

// DIRECT: the whole k sum is this workgroup's -- out is y and the epilogue is applied here; otherwise out is the partial
// buffer [segment][T][N] and the epilogue is t5_linear_sum_kernel's
template <bool DIRECT>
__global__ __launch_bounds__(256) void t5_linear_kernel(const float* x, const float* w, const float* res, int64_t T, int64_t K,
                                                        int64_t N, int64_t KS, int relu, float* out) {
  __shared__ float xs[TL_T * TL_S];
  __shared__ float wl[TL_T * TL_S];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1, h = lane >> 5, c = lane & 31;
  const int64_t n0 = (int64_t)blockIdx.x * TL_T, t0 = (int64_t)blockIdx.y * TL_T, sg = blockIdx.z;
  const int64_t k_lo = sg * KS, k_hi = (k_lo + KS < K) ? k_lo + KS : K;
  float xr[TL_PER], wr[TL_PER];
  t5_lin_fetch(x, T, K, t0, k_lo, k_hi, tid, xr);
  t5_lin_fetch(w, N, K, n0, k_lo, k_hi, tid, wr);
  f32x16 acc = t5_zero16();
  for (int64_t k0 = k_lo; k0 < k_hi; k0 += TL_KC) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TL_PER; ++j) {
      xs[((tid >> 5) + 8 * j) * TL_S + (tid & 31)] = xr[j];
      wl[((tid >> 5) + 8 * j) * TL_S + (tid & 31)] = wr[j];
    }
    __syncthreads();
    if (k0 + TL_KC < k_hi) {   // the next chunk travels while this one is multiplied
      t5_lin_fetch(x, T, K, t0, k0 + TL_KC, k_hi, tid, xr);
      t5_lin_fetch(w, N, K, n0, k0 + TL_KC, k_hi, tid, wr);
    }
    const float* xa = xs + (wm * 32 + c) * TL_S + h;
    const float* wb = wl + (wn * 32 + c) * TL_S + h;
#pragma unroll
    for (int k2 = 0; k2 < TL_KC; k2 += 2) acc = adp_mfma32(xa[k2], wb[k2], acc);
  }
  const int64_t n = n0 + wn * 32 + c;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t t = t0 + wm * 32 + t5_frag_row(r, lane);
    if (t < T && n < N) {
      float v = acc[r];
      if (DIRECT) {
        if (relu) v = fmaxf(v, 0.0f);
        if (res) v += res[t * N + n];
        out[t * N + n] = v;
      } else {
        out[(sg * T + t) * N + n] = v;
      }
    }
  }
}

// y[i] = res[i] + act(part[0][i] + part[1][i] + ...) in increasing segment order
__global__ __launch_bounds__(256) void t5_linear_sum_kernel(const float* part, const float* res, int64_t n, int ns, int relu,
                                                            float* y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = part[i];
  for (int r = 1; r < ns; ++r) s += part[(int64_t)r * n + i];
  if (relu) s = fmaxf(s, 0.0f);
  if (res) s += res[i];
  y[i] = s;
}

// ---------------------------------------------------------------------------------------------------------------- attn
// DT: 32-feature tiles of the output, ceil(dk / 32)
template <int DT>
__global__ __launch_bounds__(64) void t5_attn_kernel(const float* qkv, const float* rel_table, const int32_t* bucket,
                                                     const uint8_t* mask, int64_t H, int64_t dk, int64_t m, int64_t nb,
                                                     float* out) {
  __shared__ float qs[TA_Q * TA_S];
  __shared__ float ks[TA_Q * TA_S];      // the K tile; at the end the transposed output tile
  __shared__ float biasv[2 * TA_MAXM];   // rel_table[bucket[j], h] for j = key - query + m - 1
  __shared__ float madd[TA_MAXM];        // the mask's addend per key
  const int lane = threadIdx.x, c = lane & 31;
  const int64_t b = blockIdx.z, h = blockIdx.y, q0 = (int64_t)blockIdx.x * TA_Q;
  const int64_t HD = H * dk, row = 3 * HD;
  const float* base = qkv + b * m * row + h * dk;   // q of token 0; k is HD further, v 2 HD
  const int D = (int)dk, M = (int)m;
  for (int j = lane; j < 2 * M - 1; j += 64) {
    const int32_t bk = bucket[j];
    biasv[j] = (bk >= 0 && bk < nb) ? rel_table[(int64_t)bk * H + h] : 0.0f;
  }
  for (int j = lane; j < M; j += 64) madd[j] = (mask && mask[b * m + j] == 0) ? -FLT_MAX : 0.0f;
  for (int i = lane; i < TA_Q * D; i += 64) {
    const int q = i / D, d = i - q * D;
    qs[q * TA_S + d] = (q0 + q < m) ? base[(q0 + q) * row + d] : 0.0f;
  }
  // a query row behind the end computes on row m - 1's bias (finite values, never stored)
  const int qc = (int)((q0 + c < m) ? q0 + c : m - 1);
  float m_run = -INFINITY, l_run = 0.0f;
  f32x16 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = t5_zero16();
  for (int kt0 = 0; kt0 < M; kt0 += TA_Q) {
    __syncthreads();
    for (int i = lane; i < TA_Q * D; i += 64) {
      const int kk = i / D, d = i - kk * D;
      ks[kk * TA_S + d] = (kt0 + kk < M) ? base[(int64_t)(kt0 + kk) * row + HD + d] : 0.0f;
    }
    __syncthreads();
    // S^T[key, query]: A = K[key = c][d], B = Q^T[d][query = c], the lane halves take even and odd d
    f32x16 s = t5_zero16();
    const float* ka = ks + c * TA_S + (lane >> 5);
    const float* qb = qs + c * TA_S + (lane >> 5);
    for (int d2 = 0; d2 < D; d2 += 2) s = adp_mfma32(ka[d2], qb[d2], s);
    float tm = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt0 + t5_frag_row(r, lane);
      s[r] = (key < M) ? (s[r] + biasv[key - qc + M - 1]) + madd[key] : -INFINITY;   // a key behind the end: weight 0
      tm = fmaxf(tm, s[r]);
    }
    tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
    // every tile holds a key in [0, m): tm is finite (-FLT_MAX at the least), so is m_new, and no difference below is a NaN
    const float m_new = fmaxf(m_run, tm);
    const float alpha = expf(m_run - m_new);
    float ps = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = expf(s[r] - m_new);
      ps += s[r];
    }
    ps += __shfl_xor(ps, 32, 64);
    l_run = l_run * alpha + ps;
    m_run = m_new;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
    // O^T[d, query] += V^T[d][key] P^T[key][query]: k slot (lane >> 5) of step r is the key register r of that lane half holds
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt0 + t5_frag_row(r, lane);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const int d = dt * 32 + c;
        const float v = (key < M && d < D) ? base[(int64_t)key * row + 2 * HD + d] : 0.0f;
        o[dt] = adp_mfma32(v, s[r], o[dt]);
      }
    }
  }
  const float inv = 1.0f / l_run;   // l_run >= 1: the row maximum itself contributes exp(0)
  __syncthreads();
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = dt * 32 + t5_frag_row(r, lane);
      if (d < D) ks[c * TA_S + d] = o[dt][r] * inv;
    }
  __syncthreads();
  for (int i = lane; i < TA_Q * D; i += 64) {
    const int q = i / D, d = i - q * D;
    if (q0 + q < m) out[(b * m + q0 + q) * HD + h * dk + d] = ks[q * TA_S + d];
  }
}

// --------------------------------------------------------------------------------------------------------------- host
constexpr int64_t T5_MAX = ((int64_t)1 << 31) - 1;

// a, b >= 1: a * b <= T5_MAX without overflow
bool t5_fits(int64_t a, int64_t b) { return a <= T5_MAX / b; }

int t5_linear_plan(int64_t T, int64_t K, int64_t N, T5LinPlan* g) {
  if (T < 1 || K < 1 || N < 1) return ADP_ERR_SHAPE;
  if (T > T5_MAX || K > T5_MAX || N > T5_MAX || !t5_fits(T, K) || !t5_fits(N, K) || !t5_fits(T, N)) return ADP_ERR_SHAPE;
  if (adp_cdiv(T, TL_T) > 65535) return ADP_ERR_SHAPE;
  // about 512 workgroups over (tiles, segments); a segment is whole chunks of TL_KC and at least 128 long
  const int64_t tiles = adp_cdiv(T, TL_T) * adp_cdiv(N, TL_T);
  int64_t ns = adp_cdiv(512, tiles);
  if (ns > adp_cdiv(K, 128)) ns = adp_cdiv(K, 128);
  if (ns < 1) ns = 1;
  const int64_t KS = adp_cdiv(adp_cdiv(K, ns), TL_KC) * TL_KC;
  ns = adp_cdiv(K, KS);
  if (ns > 1 && ns * T > T5_MAX / N) return ADP_ERR_SHAPE;
  g->KS = KS;
  g->ns = (int)ns;
  return ADP_OK;
}

}  // namespace

extern "C" int adp_t5_embed(const int64_t* ids, const float* table, int64_t T, int64_t V, int64_t d, float* out, void* stream) {
  if (!ids || !table || !out) return ADP_ERR_NULL;
  if (T < 1 || V < 1 || d < 1) return ADP_ERR_SHAPE;
  if (T > T5_MAX || V > T5_MAX || d > T5_MAX || !t5_fits(T, d) || !t5_fits(V, d)) return ADP_ERR_SHAPE;
  ADP_LAUNCH(t5_embed_kernel, dim3((unsigned)T), dim3(256), stream, ids, table, V, d, out);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_t5_rmsnorm(const float* x, const float* g, int64_t T, int64_t d, float eps, float* y, void* stream) {
  if (!x || !g || !y) return ADP_ERR_NULL;
  if (T < 1 || d < 1) return ADP_ERR_SHAPE;
  if (T > T5_MAX || d > T5_MAX || !t5_fits(T, d)) return ADP_ERR_SHAPE;
  ADP_LAUNCH(t5_rmsnorm_kernel, dim3((unsigned)T), dim3(256), stream, x, g, d, eps, y);
  return ADP_LAUNCH_OK();
}

extern "C" int64_t adp_t5_linear_ws_bytes(int64_t T, int64_t K, int64_t N) {
  T5LinPlan g;
  const int rc = t5_linear_plan(T, K, N, &g);
  if (rc != ADP_OK) return rc;
  return g.ns > 1 ? (int64_t)g.ns * T * N * (int64_t)sizeof(float) : 0;
}

extern "C" int adp_t5_linear(const float* x, const float* w, const float* res, int64_t T, int64_t K, int64_t N, int64_t relu,
                             float* y, float* ws, void* stream) {
  if (!x || !w || !y) return ADP_ERR_NULL;
  T5LinPlan g;
  const int rc = t5_linear_plan(T, K, N, &g);
  if (rc != ADP_OK) return rc;
  if (g.ns > 1 && !ws) return ADP_ERR_NULL;
  const dim3 grid((unsigned)adp_cdiv(N, TL_T), (unsigned)adp_cdiv(T, TL_T), (unsigned)g.ns);
  const int act = relu != 0;
  if (g.ns == 1) {
    ADP_LAUNCH(t5_linear_kernel<true>, grid, dim3(256), stream, x, w, res, T, K, N, g.KS, act, y);
  } else {
    ADP_LAUNCH(t5_linear_kernel<false>, grid, dim3(256), stream, x, w, res, T, K, N, g.KS, act, ws);
    ADP_LAUNCH(t5_linear_sum_kernel, dim3((unsigned)adp_cdiv(T * N, 256)), dim3(256), stream, (const float*)ws, res, T * N, g.ns,
               act, y);
  }
  return ADP_LAUNCH_OK();
}

extern "C" int adp_t5_attn(const float* qkv, const float* rel_table, const int32_t* bucket, const uint8_t* mask, int64_t B,
                           int64_t H, int64_t dk, int64_t m, int64_t nb, float* out, void* stream) {
  if (!qkv || !rel_table || !bucket || !out) return ADP_ERR_NULL;
  if (B < 1 || H < 1 || dk < 1 || m < 1 || nb < 1) return ADP_ERR_SHAPE;
  if (B > 65535 || H > 65535 || dk > T5_MAX || m > T5_MAX || nb > T5_MAX || !t5_fits(nb, H)) return ADP_ERR_SHAPE;
  if (!t5_fits(H, dk) || !t5_fits(3 * H * dk, m) || !t5_fits(3 * H * dk * m, B)) return ADP_ERR_SHAPE;
  if (m > TA_MAXM || dk < 8 || dk > TA_MAXD || dk % 8 != 0) return ADP_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)adp_cdiv(m, TA_Q), (unsigned)H, (unsigned)B);
  const int64_t dt = adp_cdiv(dk, 32);
  if (dt == 1) ADP_LAUNCH(t5_attn_kernel<1>, grid, dim3(64), stream, qkv, rel_table, bucket, mask, H, dk, m, nb, out);
  else if (dt == 2) ADP_LAUNCH(t5_attn_kernel<2>, grid, dim3(64), stream, qkv, rel_table, bucket, mask, H, dk, m, nb, out);
  else if (dt == 3) ADP_LAUNCH(t5_attn_kernel<3>, grid, dim3(64), stream, qkv, rel_table, bucket, mask, H, dk, m, nb, out);
  else ADP_LAUNCH(t5_attn_kernel<4>, grid, dim3(64), stream, qkv, rel_table, bucket, mask, H, dk, m, nb, out);
  return ADP_LAUNCH_OK();
}
