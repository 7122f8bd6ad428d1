// The mel encoder's own kernels (include/adp_enc.h): the overlapping strided downsample Conv1d(R, M, 2f + 1, stride f,
// padding f) with its data and weight gradients, and the bottleneck's tanh.  fp32, exact-f32 matrix cores
// (v_mfma_f32_32x32x2_f32).  With K = 2f + 1 and N = ceil(L / f):
//
//   down_fwd    y[b, m, n]   = bias[m] + sum_{r, k} w[m, r, k] x[b, r, n f + k - f]     GEMM  M x (R K) x N       per batch row
//   down_dgrad  dx[b, r, qf+p] = sum_{m, j} w[m, r, p + j f] dy[b, m, q + 1 - j]        GEMM  R x (M J_p) x Q     per phase p
//   down_wgrad  dw[m, r, k]  = sum_{b, n} dy[b, m, n] x[b, r, n f + k - f]              GEMM  M x (B N) x (R K)
//
// Every tiled kernel: 256 threads, a 64 x 64 block tile, one 32 x 32 accumulator per wave (the f32 instruction's issue
// interval equals its dependent latency, so one accumulator keeps the pipe full); down_dgrad holds one accumulator per
// output phase p = l % f, whose taps are k = p, p + f (and 2 f for p = 0): J_0 = 3, J_p = 2, K in all, so the block uses
// every weight it stages once.  The two lanes halves of an MFMA (its two reduction slots) take an even and an odd CHANNEL
// (down_fwd, down_dgrad) or frame (down_wgrad), so that the tap index is a compile-time constant of the unrolled loop.
// Layouts in LDS:
//   down_fwd    the input segment of a channel in POLYPHASE order, element i = q f + r at [r][q]: the 32 lanes of a B
//               fragment (consecutive outputs n, one tap k = j f + r) read [r][n + j], consecutive words; the natural
//               order would put them f words apart.  Weights [64][8 K + 1].
//   down_dgrad  dy rows in natural order with one neighbour on each side, weights [64 r][8 K + 1] staged from the
//               contiguous span w[m, r0 .. r0 + 63, :].
//   down_wgrad  dy as [64 m][32 + 1], the input segments of the channels a column tile touches in natural order.
// All loads are predicated and all tails (channels, frames, rows below a tile) are zeros written into LDS.
#include <stdlib.h>
#include "adp_rt.h"
#include "adp_enc.h"

namespace {

constexpr int EN_T = 64;          // block tile edge
constexpr int EN_CH = 8;          // channels per reduction chunk between barriers (even: the lane halves split them)
constexpr int EN_NQ = EN_T + 3;   // staged row of down_fwd / down_dgrad: 64 positions + 2 neighbours, odd
constexpr int EW_NCH = 32;        // frames per reduction chunk of down_wgrad
constexpr int EW_US = EW_NCH + 1;

__device__ __forceinline__ f32x16 en_zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.0f;
  return z;
}
// row of accumulator register r in a 32x32 fragment (the column is lane & 31)
__device__ __forceinline__ int en_frag_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// ------------------------------------------------------------------------------------------------------------ down_fwd
template <int F>
__global__ __launch_bounds__(256) void enc_down_fwd_kernel(const float* x, const float* w, const float* bias, int64_t R,
                                                           int64_t M, int64_t L, int64_t N, float* y) {
  constexpr int K = 2 * F + 1, CK = EN_CH * K, WS = CK + 1, SEGN = F * EN_NQ;
  __shared__ float seg[EN_CH * SEGN];
  __shared__ float wl[EN_T * WS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1, h = lane >> 5, c = lane & 31;
  const int64_t b = blockIdx.z, m0 = (int64_t)blockIdx.y * EN_T, n0 = (int64_t)blockIdx.x * EN_T;
  const int64_t tb = n0 * F - F;   // input position of segment element 0
  f32x16 acc = en_zero16();
  for (int64_t c0 = 0; c0 < R; c0 += EN_CH) {
    const int cn = (int)((R - c0 < EN_CH) ? R - c0 : EN_CH);
    __syncthreads();
    for (int i = tid; i < EN_CH * SEGN; i += 256) {
      const int cl = i / SEGN, p = i - cl * SEGN;
      const int64_t t = tb + p;
      const float v = (cl < cn && t >= 0 && t < L) ? x[((b * R + c0 + cl) * L) + t] : 0.0f;
      seg[cl * SEGN + (p % F) * EN_NQ + p / F] = v;
    }
    for (int i = tid; i < EN_T * CK; i += 256) {
      const int mi = i / CK, kk = i - mi * CK;
      wl[mi * WS + kk] = (m0 + mi < M && kk < cn * K) ? w[((m0 + mi) * R + c0) * K + kk] : 0.0f;
    }
    __syncthreads();
    const float* wa = wl + (wm * 32 + c) * WS + h * K;
    const float* sb = seg + h * SEGN + wn * 32 + c;
#pragma unroll
    for (int i2 = 0; i2 < EN_CH / 2; ++i2)
#pragma unroll
      for (int k = 0; k < K; ++k)
        acc = adp_mfma32(wa[i2 * 2 * K + k], sb[i2 * 2 * SEGN + (k % F) * EN_NQ + k / F], acc);
  }
  const int64_t n = n0 + wn * 32 + c;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t m = m0 + wm * 32 + en_frag_row(r, lane);
    if (m < M && n < N) y[(b * M + m) * N + n] = acc[r] + bias[m];
  }
}

// ---------------------------------------------------------------------------------------------------------- down_dgrad
template <int F>
__global__ __launch_bounds__(256) void enc_down_dgrad_kernel(const float* dy, const float* w, int64_t R, int64_t M, int64_t L,
                                                             int64_t N, float* dx) {
  constexpr int K = 2 * F + 1, CK = EN_CH * K, WS = CK + 1;
  __shared__ float dys[EN_CH * EN_NQ];
  __shared__ float wl[EN_T * WS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave & 1, wq = wave >> 1, h = lane >> 5, c = lane & 31;
  const int64_t b = blockIdx.z, r0 = (int64_t)blockIdx.y * EN_T, q0 = (int64_t)blockIdx.x * EN_T;
  f32x16 acc[F];
#pragma unroll
  for (int p = 0; p < F; ++p) acc[p] = en_zero16();
  for (int64_t mc0 = 0; mc0 < M; mc0 += EN_CH) {
    const int mn = (int)((M - mc0 < EN_CH) ? M - mc0 : EN_CH);
    __syncthreads();
    for (int i = tid; i < EN_CH * EN_NQ; i += 256) {   // element qi of a row is dy at frame q0 - 1 + qi
      const int ml = i / EN_NQ, qi = i - ml * EN_NQ;
      const int64_t n = q0 - 1 + qi;
      dys[i] = (ml < mn && n >= 0 && n < N) ? dy[(b * M + mc0 + ml) * N + n] : 0.0f;
    }
    for (int i = tid; i < EN_CH * EN_T * K; i += 256) {  // w[m, r0 .. r0 + 63, :] is one contiguous span
      const int ml = i / (EN_T * K), e = i - ml * (EN_T * K);
      const int ri = e / K, k = e - ri * K;
      wl[ri * WS + ml * K + k] = (ml < mn && r0 + ri < R) ? w[((mc0 + ml) * R + r0) * K + e] : 0.0f;
    }
    __syncthreads();
    const float* wa = wl + (wr * 32 + c) * WS + h * K;
    const float* db = dys + h * EN_NQ + wq * 32 + c + 2;
#pragma unroll
    for (int i2 = 0; i2 < EN_CH / 2; ++i2)
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int p = 0; p < F; ++p)
          if (p + j * F < K) acc[p] = adp_mfma32(wa[i2 * 2 * K + p + j * F], db[i2 * 2 * EN_NQ - j], acc[p]);
  }
  const int64_t q = q0 + wq * 32 + c;
#pragma unroll
  for (int p = 0; p < F; ++p) {
    const int64_t l = q * F + p;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      const int64_t r = r0 + wr * 32 + en_frag_row(rr, lane);
      if (r < R && l < L) dx[(b * R + r) * L + l] = acc[p][rr];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------- down_wgrad
struct EncWPlan {
  int64_t SL;   // frames per segment (whole chunks of EW_NCH)
  int sl, segs; // segments per batch row, in all
};

template <int F>
__global__ __launch_bounds__(256) void enc_down_wgrad_kernel(const float* x, const float* dy, int64_t R, int64_t M, int64_t L,
                                                             int64_t N, EncWPlan g, float* part) {
  constexpr int K = 2 * F + 1, SEGW = (EW_NCH + 1) * F + 1, NB = (EN_T - 1) / K + 2;   // NB: channels 64 columns can touch
  __shared__ float vs[NB * SEGW];
  __shared__ float us[EN_T * EW_US];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wc = wave >> 1, h = lane >> 5, c = lane & 31;
  const int64_t m0 = (int64_t)blockIdx.x * EN_T, col0 = (int64_t)blockIdx.y * EN_T, RK = R * K;
  const int64_t sg = blockIdx.z, b = sg / g.sl, n_lo = (sg % g.sl) * g.SL;
  const int64_t n_hi = (n_lo + g.SL < N) ? n_lo + g.SL : N;
  const int64_t r_lo = col0 / K;
  const int64_t clast = (col0 + EN_T - 1 < RK - 1) ? col0 + EN_T - 1 : RK - 1;
  const int nb = (int)(clast / K - r_lo) + 1;
  const int64_t col = col0 + wc * 32 + c;
  int colo = 0;
  if (col < RK) {
    const int64_t r = col / K;
    colo = (int)(r - r_lo) * SEGW + (int)(col - r * K);
  }
  f32x16 acc = en_zero16();
  for (int64_t nc0 = n_lo; nc0 < n_hi; nc0 += EW_NCH) {
    __syncthreads();
    for (int i = tid; i < EN_T * EW_NCH; i += 256) {
      const int mi = i / EW_NCH, ni = i - mi * EW_NCH;
      us[mi * EW_US + ni] = (m0 + mi < M && nc0 + ni < n_hi) ? dy[(b * M + m0 + mi) * N + nc0 + ni] : 0.0f;
    }
    const int64_t tb = nc0 * F - F;
    for (int i = tid; i < nb * SEGW; i += 256) {
      const int bi = i / SEGW, p = i - bi * SEGW;
      const int64_t t = tb + p;
      vs[i] = (t >= 0 && t < L) ? x[(b * R + r_lo + bi) * L + t] : 0.0f;
    }
    __syncthreads();
    const float* ua = us + (wm * 32 + c) * EW_US + h;
    const float* vb = vs + colo + h * F;
#pragma unroll
    for (int n2 = 0; n2 < EW_NCH; n2 += 2) acc = adp_mfma32(ua[n2], vb[n2 * F], acc);
  }
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int64_t m = m0 + wm * 32 + en_frag_row(rr, lane);
    if (m < M && col < RK) part[(sg * M + m) * RK + col] = acc[rr];
  }
}

// dw[i] = part[0][i] + part[1][i] + ... in increasing segment order
__global__ __launch_bounds__(256) void enc_down_wgrad_sum_kernel(const float* part, int64_t n, int segs, float* dw) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = part[i];
  for (int r = 1; r < segs; ++r) s += part[(int64_t)r * n + i];
  dw[i] = s;
}

// dbias[m] = sum over (b, n) of dy[b, m, n]: one workgroup per channel, a fixed thread-strided order, then the wave and block sums
__global__ __launch_bounds__(256) void enc_down_dbias_kernel(const float* dy, int64_t B, int64_t M, int64_t N, float* dbias) {
  __shared__ float sh[4];
  const int64_t m = blockIdx.x, total = B * N;
  float s = 0.0f;
  for (int64_t i = threadIdx.x; i < total; i += 256) {
    const int64_t b = i / N, n = i - b * N;
    s += dy[(b * M + m) * N + n];
  }
  s = adp_block_sum<4>(s, sh);
  if (threadIdx.x == 0) dbias[m] = s;
}

// ---------------------------------------------------------------------------------------------------------------- tanh
// VEC: every pointer is 16-byte aligned -- thread i < n / 4 takes elements 4 i .. 4 i + 3, the threads behind them the tail
template <bool VEC>
__global__ __launch_bounds__(256) void enc_tanh_fwd_kernel(const float* hh, int64_t n, float* z) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (VEC) {
    const int64_t n4 = n / 4;
    if (i < n4) {
      f32x4 v = ((const f32x4*)hh)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = tanhf(v[e]);
      ((f32x4*)z)[i] = v;
    } else if (4 * n4 + (i - n4) < n) {
      const int64_t j = 4 * n4 + (i - n4);
      z[j] = tanhf(hh[j]);
    }
  } else if (i < n) {
    z[i] = tanhf(hh[i]);
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void enc_tanh_bwd_kernel(const float* z, const float* dz, int64_t n, float* dh) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (VEC) {
    const int64_t n4 = n / 4;
    if (i < n4) {
      const f32x4 zv = ((const f32x4*)z)[i], g = ((const f32x4*)dz)[i];
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = g[e] * (1.0f - zv[e] * zv[e]);
      ((f32x4*)dh)[i] = v;
    } else if (4 * n4 + (i - n4) < n) {
      const int64_t j = 4 * n4 + (i - n4);
      dh[j] = dz[j] * (1.0f - z[j] * z[j]);
    }
  } else if (i < n) {
    dh[i] = dz[i] * (1.0f - z[i] * z[i]);
  }
}

// --------------------------------------------------------------------------------------------------------------- host
constexpr int64_t EN_MAX = ((int64_t)1 << 31) - 1;
constexpr int64_t EN_MAX_CH = (int64_t)1 << 20;

bool en_aligned(const void* a) { return ((uintptr_t)a & 15) == 0; }

int64_t en_out_len(int64_t L, int64_t f) { return (L - 1) / f + 1; }

// extents first (ADP_ERR_SHAPE), then the factor (ADP_ERR_UNSUPPORTED)
int en_check(int64_t B, int64_t R, int64_t M, int64_t L, int64_t f) {
  if (B < 1 || R < 1 || M < 1 || L < 1) return ADP_ERR_SHAPE;
  if (B > 65535 || R > EN_MAX_CH || M > EN_MAX_CH || L > EN_MAX) return ADP_ERR_SHAPE;
  if (f < 2 || f > 4) return ADP_ERR_UNSUPPORTED;
  // (B R and B M are below 2^36: the products are compared by division, nothing overflows)
  if (B * R > EN_MAX / L || B * M > EN_MAX / en_out_len(L, f) || M * R * (2 * f + 1) > EN_MAX) return ADP_ERR_SHAPE;
  return ADP_OK;
}

int en_wgrad_plan(int64_t B, int64_t R, int64_t M, int64_t L, int64_t f, EncWPlan* g) {
  const int rc = en_check(B, R, M, L, f);
  if (rc != ADP_OK) return rc;
  const int64_t N = en_out_len(L, f), RK = R * (2 * f + 1);
  // about 512 workgroups over (tiles of dw, batch row, segment); segments are whole chunks of EW_NCH frames
  const int64_t tiles = adp_cdiv(M, EN_T) * adp_cdiv(RK, EN_T);
  int64_t sl = adp_cdiv(512, tiles * B);
  if (sl > adp_cdiv(N, EW_NCH)) sl = adp_cdiv(N, EW_NCH);
  if (sl < 1) sl = 1;
  const int64_t SL = adp_cdiv(adp_cdiv(N, sl), EW_NCH) * EW_NCH;
  sl = adp_cdiv(N, SL);
  if (B * sl > 65535 || adp_cdiv(RK, EN_T) > 65535) return ADP_ERR_SHAPE;
  g->SL = SL;
  g->sl = (int)sl;
  g->segs = (int)(B * sl);
  return ADP_OK;
}

}  // namespace

extern "C" int64_t adp_enc_down_out_len(int64_t L, int64_t f) {
  if (L < 1 || L > EN_MAX) return ADP_ERR_SHAPE;
  if (f < 2 || f > 4) return ADP_ERR_UNSUPPORTED;
  return en_out_len(L, f);
}

extern "C" int adp_enc_down_fwd(const float* x, const float* w, const float* bias, int64_t B, int64_t R, int64_t M, int64_t L,
                                int64_t f, float* y, void* stream) {
  if (!x || !w || !bias || !y) return ADP_ERR_NULL;
  const int rc = en_check(B, R, M, L, f);
  if (rc != ADP_OK) return rc;
  const int64_t N = en_out_len(L, f);
  if (adp_cdiv(M, EN_T) > 65535) return ADP_ERR_SHAPE;
  const dim3 grid((unsigned)adp_cdiv(N, EN_T), (unsigned)adp_cdiv(M, EN_T), (unsigned)B);
  if (f == 2) ADP_LAUNCH(enc_down_fwd_kernel<2>, grid, dim3(256), stream, x, w, bias, R, M, L, N, y);
  else if (f == 3) ADP_LAUNCH(enc_down_fwd_kernel<3>, grid, dim3(256), stream, x, w, bias, R, M, L, N, y);
  else ADP_LAUNCH(enc_down_fwd_kernel<4>, grid, dim3(256), stream, x, w, bias, R, M, L, N, y);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_enc_down_dgrad(const float* dy, const float* w, int64_t B, int64_t R, int64_t M, int64_t L, int64_t f,
                                  float* dx, void* stream) {
  if (!dy || !w || !dx) return ADP_ERR_NULL;
  const int rc = en_check(B, R, M, L, f);
  if (rc != ADP_OK) return rc;
  const int64_t N = en_out_len(L, f);   // = ceil(L / f): the number of output positions per phase
  if (adp_cdiv(R, EN_T) > 65535) return ADP_ERR_SHAPE;
  const dim3 grid((unsigned)adp_cdiv(N, EN_T), (unsigned)adp_cdiv(R, EN_T), (unsigned)B);
  if (f == 2) ADP_LAUNCH(enc_down_dgrad_kernel<2>, grid, dim3(256), stream, dy, w, R, M, L, N, dx);
  else if (f == 3) ADP_LAUNCH(enc_down_dgrad_kernel<3>, grid, dim3(256), stream, dy, w, R, M, L, N, dx);
  else ADP_LAUNCH(enc_down_dgrad_kernel<4>, grid, dim3(256), stream, dy, w, R, M, L, N, dx);
  return ADP_LAUNCH_OK();
}

extern "C" int64_t adp_enc_down_wgrad_ws_bytes(int64_t B, int64_t R, int64_t M, int64_t L, int64_t f) {
  EncWPlan g;
  const int rc = en_wgrad_plan(B, R, M, L, f, &g);
  if (rc != ADP_OK) return rc;
  return (int64_t)g.segs * M * R * (2 * f + 1) * (int64_t)sizeof(float);
}

extern "C" int adp_enc_down_wgrad(const float* x, const float* dy, int64_t B, int64_t R, int64_t M, int64_t L, int64_t f,
                                  float* dw, float* dbias, float* ws, void* stream) {
  if (!x || !dy || !dw || !dbias || !ws) return ADP_ERR_NULL;
  EncWPlan g;
  const int rc = en_wgrad_plan(B, R, M, L, f, &g);
  if (rc != ADP_OK) return rc;
  const int64_t N = en_out_len(L, f), cnt = M * R * (2 * f + 1);
  const dim3 grid((unsigned)adp_cdiv(M, EN_T), (unsigned)adp_cdiv(R * (2 * f + 1), EN_T), (unsigned)g.segs);
  if (f == 2) ADP_LAUNCH(enc_down_wgrad_kernel<2>, grid, dim3(256), stream, x, dy, R, M, L, N, g, ws);
  else if (f == 3) ADP_LAUNCH(enc_down_wgrad_kernel<3>, grid, dim3(256), stream, x, dy, R, M, L, N, g, ws);
  else ADP_LAUNCH(enc_down_wgrad_kernel<4>, grid, dim3(256), stream, x, dy, R, M, L, N, g, ws);
  ADP_LAUNCH(enc_down_wgrad_sum_kernel, dim3((unsigned)adp_cdiv(cnt, 256)), dim3(256), stream, (const float*)ws, cnt, g.segs, dw);
  ADP_LAUNCH(enc_down_dbias_kernel, dim3((unsigned)M), dim3(256), stream, dy, B, M, N, dbias);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_enc_tanh_fwd(const float* h, int64_t n, float* z, void* stream) {
  if (!h || !z) return ADP_ERR_NULL;
  if (n < 1 || n > EN_MAX) return ADP_ERR_SHAPE;
  if (en_aligned(h) && en_aligned(z)) {
    ADP_LAUNCH(enc_tanh_fwd_kernel<true>, dim3((unsigned)adp_cdiv(n / 4 + n % 4, 256)), dim3(256), stream, h, n, z);
  } else {
    ADP_LAUNCH(enc_tanh_fwd_kernel<false>, dim3((unsigned)adp_cdiv(n, 256)), dim3(256), stream, h, n, z);
  }
  return ADP_LAUNCH_OK();
}

extern "C" int adp_enc_tanh_bwd(const float* z, const float* dz, int64_t n, float* dh, void* stream) {
  if (!z || !dz || !dh) return ADP_ERR_NULL;
  if (n < 1 || n > EN_MAX) return ADP_ERR_SHAPE;
  if (en_aligned(z) && en_aligned(dz) && en_aligned(dh)) {
    ADP_LAUNCH(enc_tanh_bwd_kernel<true>, dim3((unsigned)adp_cdiv(n / 4 + n % 4, 256)), dim3(256), stream, z, dz, n, dh);
  } else {
    ADP_LAUNCH(enc_tanh_bwd_kernel<false>, dim3((unsigned)adp_cdiv(n, 256)), dim3(256), stream, z, dz, n, dh);
  }
  return ADP_LAUNCH_OK();
}
