// The learned-transform front end (include/adp_lt.h): a strided convolution over a reflect- or zero-continued signal, the
// strided transposed convolution, and the weight gradient of both.  fp32, exact-f32 matrix cores (v_mfma_f32_32x32x2_f32).
//
//   lt_conv   y[n, o, l]   = sum_{c, k} w[o, c, k] xp[n, c, l s + k - p]          GEMM  O x (C K) x L        per batch row
//   lt_convt  out[n, o, t] = sum_{c, j} x[n, c, q - j] w[c, o, r + j s]           GEMM  Q x (C J) x (O s)    t + p = q s + r
//   lt_wgrad  dw[a, b, k]  = sum_{n, l} u[n, a, l] vp[n, b, l s + k - p]          GEMM  A x (B L) x (Bc K)
//
// The "im2col" operand of every one of them is a strided window of a signal segment that a workgroup stages in LDS once;
// the continuation (reflect / zero) is applied by the staging loop, so no padded copy exists.  Layouts in LDS:
//   lt_conv   the segment in POLYPHASE order, element i = q s + r of a channel at [r][q] with an odd row length NQ: the 32
//             lanes of a B fragment (consecutive frames l, one tap k = j s + r) read [r][l + j], consecutive words -- the
//             natural order would put them s words apart, all on one bank for s = 32.  Weights [64][32 + 1].
//   lt_convt  x rows in natural order (A fragment: consecutive q), weights as [c j][o r] (B fragment: consecutive r, and
//             the store of a fragment row is consecutive in t).
//   lt_wgrad  u as [a][32 + 1], the v segment in natural order (B fragment: consecutive taps k).
// Every tiled kernel: 256 threads, wave tile 32 x 64 (two accumulators share the A fragment), a k-chunk of 32 between
// barriers.  The per-output kernels behind them read global memory directly and take every geometry.
#include <stdlib.h>
#include "adp_rt.h"
#include "adp_lt.h"

namespace {

constexpr int LT_CAP = 12288;   // LDS floats of the staged signal operand (48 KiB)
constexpr int LT_KC = 32;       // reduction chunk between barriers
constexpr int LT_WS = LT_KC + 1;
constexpr int LT_MIN_ROWS = 8; // narrower operands (rows / columns of the 32-wide fragment they fill) go to the per-output kernels

struct LtGeom {
  int64_t B, C, T, O, K, s, p, L;
  int mode;
  int J, NQ, cc, sh;            // taps per phase ceil(K / s); lt_conv: polyphase row length, channels per staged chunk, and
                                // the segment's shift: it starts sh = p % 4 elements early, on a 16-byte boundary of the row
};

// xp[t] of one signal row: t in [-p, T + p) by reflection (p < T, so one reflection is enough), zero outside that range
// (only masked fragment columns read there); zero mode: zero outside [0, T)
__device__ __forceinline__ float lt_fetch(const float* row, int64_t t, int64_t T, int64_t p, int mode) {
  if (mode == ADP_LT_REFLECT) {
    if (t < -p || t >= T + p) return 0.0f;
    if (t < 0) t = -t;
    else if (t >= T) t = 2 * (T - 1) - t;
    return row[t];
  }
  return (t >= 0 && t < T) ? row[t] : 0.0f;
}

__device__ __forceinline__ f32x16 lt_zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.0f;
  return z;
}
// row of accumulator register r in a 32x32 fragment (the column is lane & 31)
__device__ __forceinline__ int lt_frag_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// ------------------------------------------------------------------------------------------------------------- lt_conv
constexpr int LC_BO = 64, LC_BL = 128;

template <bool VEC>
__global__ __launch_bounds__(256) void lt_conv_tile_kernel(const float* x, const float* w, LtGeom g, float* y) {
  __shared__ float seg[LT_CAP] __attribute__((aligned(16)));
  __shared__ float wl[LC_BO * LT_WS];
  __shared__ int offt[LT_KC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wo = wave & 1, wh = wave >> 1;
  const int K = (int)g.K, s = (int)g.s, NQ = g.NQ, C = (int)g.C;
  const int64_t n = blockIdx.z, o0 = (int64_t)blockIdx.y * LC_BO, l0 = (int64_t)blockIdx.x * LC_BL;
  const int64_t tb = l0 * g.s - g.p - g.sh;
  const int segn = s * NQ;
  f32x16 acc0 = lt_zero16(), acc1 = lt_zero16();
  for (int c0 = 0; c0 < C; c0 += g.cc) {
    const int cn = (C - c0 < g.cc) ? C - c0 : g.cc;
    __syncthreads();
    for (int cl = 0; cl < cn; ++cl) {
      const float* row = x + (n * C + c0 + cl) * g.T;
      float* sc = seg + cl * segn;
      if (VEC) {  // s, T, p + sh multiples of 4, x 16-byte aligned: four elements share q and lie inside the row together
        for (int i = tid * 4; i < segn; i += 1024) {
          const int q = i / s, r = i - q * s;
          const int64_t t = tb + i;
          f32x4 v;
          if (t >= 0 && t + 3 < g.T) {
            v = *(const f32x4*)(row + t);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = lt_fetch(row, t + e, g.T, g.p, g.mode);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) sc[(r + e) * NQ + q] = v[e];
        }
      } else {
        for (int i = tid; i < segn; i += 256) {
          const int q = i / s, r = i - q * s;
          sc[r * NQ + q] = lt_fetch(row, tb + i, g.T, g.p, g.mode);
        }
      }
    }
    const int ck = cn * K;
    for (int kk0 = 0; kk0 < ck; kk0 += LT_KC) {
      __syncthreads();
      for (int i = tid; i < LC_BO * LT_KC; i += 256) {
        const int oi = i >> 5, kq = i & 31;
        wl[oi * LT_WS + kq] = (o0 + oi < g.O && kk0 + kq < ck) ? w[((o0 + oi) * C + c0) * K + kk0 + kq] : 0.0f;
      }
      if (tid < LT_KC) {
        const int kk = kk0 + tid;
        int off = 0;
        if (kk < ck) {
          const int cl = kk / K, k = kk - cl * K + g.sh;
          const int j = k / s, r = k - j * s;
          off = cl * segn + r * NQ + j;
        }
        offt[tid] = off;
      }
      __syncthreads();
      const float* wa = wl + (wo * 32 + (lane & 31)) * LT_WS + (lane >> 5);
      const float* sb = seg + wh * 64 + (lane & 31);
#pragma unroll
      for (int k2 = 0; k2 < LT_KC; k2 += 2) {
        const float a = wa[k2];
        const int off = offt[k2 + (lane >> 5)];
        acc0 = adp_mfma32(a, sb[off], acc0);
        acc1 = adp_mfma32(a, sb[off + 32], acc1);
      }
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int64_t l = l0 + wh * 64 + h * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t o = o0 + wo * 32 + lt_frag_row(r, lane);
      if (o < g.O && l < g.L) y[(n * g.O + o) * g.L + l] = h ? acc1[r] : acc0[r];
    }
  }
}

__global__ __launch_bounds__(256) void lt_conv_plain_kernel(const float* x, const float* w, LtGeom g, float* y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= g.B * g.O * g.L) return;
  const int64_t l = i % g.L, no = i / g.L, o = no % g.O, n = no / g.O;
  const int64_t tb = l * g.s - g.p;
  float acc = 0.0f;
  for (int64_t c = 0; c < g.C; ++c) {
    const float* row = x + (n * g.C + c) * g.T;
    const float* wr = w + (o * g.C + c) * g.K;
    float part = 0.0f;
    for (int64_t k = 0; k < g.K; ++k) part = fmaf(wr[k], lt_fetch(row, tb + k, g.T, g.p, g.mode), part);
    acc += part;
  }
  y[i] = acc;
}

// ------------------------------------------------------------------------------------------------------------ lt_convt
constexpr int LD_BQ = 128, LD_BM = 64;

struct LtTGeom {
  int64_t B, C, L, O, K, s, p, T, qf, OS;   // qf: q of output 0; OS = O s (fragment columns m = o s + r)
  int mode, J, XW;                          // XW: staged x row = LD_BQ + J - 1 columns
};

// the full (uncropped) transposed convolution at position t of the reflect-extended axis, t >= -p
__device__ __forceinline__ float lt_convt_at(const float* x, const float* w, const LtTGeom& g, int64_t n, int64_t o, int64_t t) {
  const int64_t u = t + g.p, q = u / g.s, r = u - q * g.s;
  float acc = 0.0f;
  for (int64_t c = 0; c < g.C; ++c) {
    const float* xr = x + (n * g.C + c) * g.L;
    const float* wr = w + (c * g.O + o) * g.K;
    float part = 0.0f;
    for (int64_t j = 0, k = r; k < g.K; ++j, k += g.s) {
      const int64_t l = q - j;
      if (l < 0) break;
      if (l < g.L) part = fmaf(xr[l], wr[k], part);
    }
    acc += part;
  }
  return acc;
}

template <bool VEC>
__global__ __launch_bounds__(256) void lt_convt_tile_kernel(const float* x, const float* w, LtTGeom g, float* out) {
  __shared__ float xs[LT_CAP];
  __shared__ float wl[LT_KC * LD_BM] __attribute__((aligned(16)));
  __shared__ int offx[LT_KC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int J = g.J, XW = g.XW, C = (int)g.C, K = (int)g.K, s = (int)g.s;
  const int64_t n = blockIdx.z, m0 = (int64_t)blockIdx.y * LD_BM, q0 = g.qf + (int64_t)blockIdx.x * LD_BQ;
  const int64_t qb = q0 - (J - 1);
  const int CJ = C * J;
  // the weight column this thread stages: m = o s + r, fixed for the kernel (VEC: four consecutive r of one o)
  const int mi = VEC ? (tid & 15) * 4 : (tid & 63);
  const int64_t m = m0 + mi;
  const int64_t wo = m / s;
  const int wr = (int)(m - wo * s);
  f32x16 acc0 = lt_zero16(), acc1 = lt_zero16();
  for (int kk0 = 0; kk0 < CJ; kk0 += LT_KC) {
    const int c_lo = kk0 / J;
    int c_hi = (kk0 + LT_KC - 1) / J;
    if (c_hi > C - 1) c_hi = C - 1;
    const int nx = (c_hi - c_lo + 1) * XW;
    __syncthreads();
    for (int i = tid; i < nx; i += 256) {
      const int ci = i / XW, qi = i - ci * XW;
      const int64_t l = qb + qi;
      xs[i] = (l >= 0 && l < g.L) ? x[(n * C + c_lo + ci) * g.L + l] : 0.0f;
    }
    if (VEC) {  // s and K multiples of 4, w 16-byte aligned: r .. r + 3 belong to one o and one j
      for (int kq = tid >> 4; kq < LT_KC; kq += 16) {
        const int kk = kk0 + kq, c = kk / J, j = kk - c * J, k = wr + j * s;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (kk < CJ && m < g.OS && k < K) v = *(const f32x4*)(w + ((int64_t)c * g.O + wo) * K + k);
        *(f32x4*)(wl + kq * LD_BM + mi) = v;
      }
    } else {
      for (int kq = tid >> 6; kq < LT_KC; kq += 4) {
        const int kk = kk0 + kq, c = kk / J, j = kk - c * J, k = wr + j * s;
        wl[kq * LD_BM + mi] = (kk < CJ && m < g.OS && k < K) ? w[((int64_t)c * g.O + wo) * K + k] : 0.0f;
      }
    }
    if (tid < LT_KC) {
      const int kk = kk0 + tid;
      int off = 0;
      if (kk < CJ) {
        const int c = kk / J, j = kk - c * J;
        off = (c - c_lo) * XW + (J - 1) - j;
      }
      offx[tid] = off;
    }
    __syncthreads();
    const float* xa = xs + wave * 32 + (lane & 31);
    const float* wb = wl + (lane >> 5) * LD_BM + (lane & 31);
#pragma unroll
    for (int k2 = 0; k2 < LT_KC; k2 += 2) {
      const float a = xa[offx[k2 + (lane >> 5)]];
      acc0 = adp_mfma32(a, wb[k2 * LD_BM], acc0);
      acc1 = adp_mfma32(a, wb[k2 * LD_BM + 32], acc1);
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int64_t mc = m0 + h * 32 + (lane & 31);
    const int64_t o = mc / s;
    const int64_t r = mc - o * s;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t q = q0 + wave * 32 + lt_frag_row(i, lane);
      const int64_t t = q * s + r - g.p;
      if (mc < g.OS && t >= 0 && t < g.T) out[(n * g.O + o) * g.T + t] = h ? acc1[i] : acc0[i];
    }
  }
}

// ADP_LT_FOLD behind the tiled kernel: the owner of border position t adds the mirrored sums (left: t = 1 .. p from -t;
// right: t = T-1-p .. T-2 from 2 (T-1) - t).  A position in both ranges belongs to its left thread.
__global__ __launch_bounds__(256) void lt_convt_fold_kernel(const float* x, const float* w, LtTGeom g, float* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= g.B * g.O * 2 * g.p) return;
  const int64_t e = i % (2 * g.p), no = i / (2 * g.p), o = no % g.O, n = no / g.O;
  const bool left = e < g.p;
  const int64_t t = left ? 1 + e : g.T - 1 - g.p + (e - g.p);
  const bool in_left = t >= 1 && t <= g.p, in_right = t >= g.T - 1 - g.p && t <= g.T - 2;
  if (!left && in_left) return;
  float add = 0.0f;
  if (in_left) add += lt_convt_at(x, w, g, n, o, -t);
  if (in_right) add += lt_convt_at(x, w, g, n, o, 2 * (g.T - 1) - t);
  out[(n * g.O + o) * g.T + t] += add;
}

__global__ __launch_bounds__(256) void lt_convt_plain_kernel(const float* x, const float* w, LtTGeom g, float* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= g.B * g.O * g.T) return;
  const int64_t t = i % g.T, no = i / g.T, o = no % g.O, n = no / g.O;
  float acc = lt_convt_at(x, w, g, n, o, t);
  if (g.mode == ADP_LT_FOLD) {
    if (t >= 1 && t <= g.p) acc += lt_convt_at(x, w, g, n, o, -t);
    if (t >= g.T - 1 - g.p && t <= g.T - 2) acc += lt_convt_at(x, w, g, n, o, 2 * (g.T - 1) - t);
  }
  out[i] = acc;
}

// ------------------------------------------------------------------------------------------------------------ lt_wgrad
constexpr int LW_BA = 64, LW_BC = 128, LW_LCH = 32;

struct LtWGeom {
  int64_t B, A, Bc, L, T, K, s, p, BK;      // BK = Bc K (columns of dw)
  int mode, sl, SL, segs, SEGW;             // segments per batch row, frames per segment; staged v row (LW_LCH - 1) s + K
};

__global__ __launch_bounds__(256) void lt_wgrad_tile_kernel(const float* u, const float* v, LtWGeom g, float* part) {
  __shared__ float vs[LT_CAP];
  __shared__ float us[LW_BA * LT_WS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wa = wave & 1, wc = wave >> 1;
  const int K = (int)g.K, s = (int)g.s, SEGW = g.SEGW;
  const int64_t a0 = (int64_t)blockIdx.x * LW_BA, col0 = (int64_t)blockIdx.y * LW_BC;
  const int seg = blockIdx.z;
  const int64_t n = seg / g.sl, l_lo = (int64_t)(seg % g.sl) * g.SL;
  const int64_t l_hi = (l_lo + g.SL < g.L) ? l_lo + g.SL : g.L;
  const int b_lo = (int)(col0 / K);
  int64_t clast = col0 + LW_BC - 1;
  if (clast > g.BK - 1) clast = g.BK - 1;
  const int nb = (int)(clast / K) - b_lo + 1;
  int colo[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int64_t col = col0 + wc * 64 + h * 32 + (lane & 31);
    colo[h] = 0;
    if (col < g.BK) {
      const int b = (int)(col / K), k = (int)(col - (int64_t)b * K);
      colo[h] = (b - b_lo) * SEGW + k;
    }
  }
  f32x16 acc0 = lt_zero16(), acc1 = lt_zero16();
  for (int64_t lc0 = l_lo; lc0 < l_hi; lc0 += LW_LCH) {
    __syncthreads();
    for (int i = tid; i < LW_BA * LW_LCH; i += 256) {
      const int ai = i >> 5, li = i & 31;
      us[ai * LT_WS + li] = (a0 + ai < g.A && lc0 + li < l_hi) ? u[(n * g.A + a0 + ai) * g.L + lc0 + li] : 0.0f;
    }
    const int64_t tb = lc0 * g.s - g.p;
    for (int bi = 0; bi < nb; ++bi) {
      const float* row = v + (n * g.Bc + b_lo + bi) * g.T;
      for (int i = tid; i < SEGW; i += 256) vs[bi * SEGW + i] = lt_fetch(row, tb + i, g.T, g.p, g.mode);
    }
    __syncthreads();
    const float* ua = us + (wa * 32 + (lane & 31)) * LT_WS + (lane >> 5);
    const float* vb = vs + (lane >> 5) * s;
#pragma unroll
    for (int l2 = 0; l2 < LW_LCH; l2 += 2) {
      const float a = ua[l2];
      acc0 = adp_mfma32(a, vb[colo[0] + l2 * s], acc0);
      acc1 = adp_mfma32(a, vb[colo[1] + l2 * s], acc1);
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int64_t col = col0 + wc * 64 + h * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t a = a0 + wa * 32 + lt_frag_row(r, lane);
      if (a < g.A && col < g.BK) part[((int64_t)seg * g.A + a) * g.BK + col] = h ? acc1[r] : acc0[r];
    }
  }
}

__global__ __launch_bounds__(256) void lt_wgrad_plain_kernel(const float* u, const float* v, LtWGeom g, float* part) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= g.A * g.BK) return;
  const int64_t a = i / g.BK, col = i - a * g.BK, b = col / g.K, k = col - b * g.K;
  const int seg = blockIdx.y;
  const int64_t n = seg / g.sl, l_lo = (int64_t)(seg % g.sl) * g.SL;
  const int64_t l_hi = (l_lo + g.SL < g.L) ? l_lo + g.SL : g.L;
  const float* ur = u + (n * g.A + a) * g.L;
  const float* row = v + (n * g.Bc + b) * g.T;
  float acc = 0.0f;
  for (int64_t l = l_lo; l < l_hi; ++l) acc = fmaf(ur[l], lt_fetch(row, l * g.s + k - g.p, g.T, g.p, g.mode), acc);
  part[(int64_t)seg * g.A * g.BK + i] = acc;
}

// dw[i] = part[0][i] + part[1][i] + ... in increasing segment order
__global__ __launch_bounds__(256) void lt_wgrad_sum_kernel(const float* part, int64_t n, int segs, float* dw) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = part[i];
  for (int r = 1; r < segs; ++r) s += part[(int64_t)r * n + i];
  dw[i] = s;
}

// --------------------------------------------------------------------------------------------------------------- host
constexpr int64_t LT_MAX_LEN = ((int64_t)1 << 31) - 1;

bool lt_aligned(const void* a) { return ((uintptr_t)a & 15) == 0; }
// ADP_LT_TILED=0 sends every call to the per-output kernels (A/B and test knob)
bool lt_tiled_on() { return adp_knob_on("ADP_LT_TILED", true); }

int lt_check_common(int64_t B, int64_t Ca, int64_t Cb, int64_t K, int64_t s, int64_t p) {
  if (B < 1 || Ca < 1 || Cb < 1 || K < 1 || s < 1) return ADP_ERR_SHAPE;
  if (p < 0) return ADP_ERR_UNSUPPORTED;
  if (B > 65535 || Ca > 65535 || Cb > 65535 || K > 65536 || s > 65536 || p > LT_MAX_LEN) return ADP_ERR_SHAPE;
  return ADP_OK;
}

int64_t lt_conv_len(int64_t T, int64_t K, int64_t s, int64_t p) {
  if (T < 1 || T > LT_MAX_LEN || T + 2 * p < K) return ADP_ERR_SHAPE;
  return (T + 2 * p - K) / s + 1;
}

int lt_wgrad_plan(int64_t B, int64_t A, int64_t Bc, int64_t L, int64_t K, LtWGeom* g) {
  if (B < 1 || A < 1 || Bc < 1 || L < 1 || K < 1) return ADP_ERR_SHAPE;
  if (B > 65535 || A > 65535 || Bc > 65535 || K > 65536 || L > LT_MAX_LEN) return ADP_ERR_SHAPE;
  // about 512 workgroups over (tiles of dw, batch row, segment); segments are whole chunks of LW_LCH frames
  const int64_t tiles = adp_cdiv(A, LW_BA) * adp_cdiv(Bc * K, LW_BC);
  int64_t sl = adp_cdiv(512, tiles * B);
  if (sl > adp_cdiv(L, LW_LCH)) sl = adp_cdiv(L, LW_LCH);
  if (sl < 1) sl = 1;
  const int64_t SL = adp_cdiv(adp_cdiv(L, sl), LW_LCH) * LW_LCH;
  sl = adp_cdiv(L, SL);
  if (B * sl > 65535) return ADP_ERR_SHAPE;
  g->B = B; g->A = A; g->Bc = Bc; g->L = L; g->K = K; g->BK = Bc * K;
  g->sl = (int)sl;
  g->SL = (int)SL;
  g->segs = (int)(B * sl);
  return ADP_OK;
}

}  // namespace

extern "C" int64_t adp_lt_conv_out_len(int64_t T, int64_t K, int64_t stride, int64_t pad) {
  if (K < 1 || stride < 1) return ADP_ERR_SHAPE;
  if (pad < 0) return ADP_ERR_UNSUPPORTED;
  return lt_conv_len(T, K, stride, pad);
}

extern "C" int64_t adp_lt_convt_out_len(int64_t L, int64_t K, int64_t stride, int64_t pad) {
  if (L < 1 || K < 1 || stride < 1) return ADP_ERR_SHAPE;
  if (pad < 0) return ADP_ERR_UNSUPPORTED;
  const int64_t T = (L - 1) * stride - 2 * pad + K;
  return T < 1 ? ADP_ERR_SHAPE : T;
}

extern "C" int adp_lt_conv(const float* x, const float* w, int64_t B, int64_t C, int64_t T, int64_t O, int64_t K,
                           int64_t stride, int64_t pad, int64_t mode, float* y, void* stream) {
  if (!x || !w || !y) return ADP_ERR_NULL;
  const int rc = lt_check_common(B, C, O, K, stride, pad);
  if (rc != ADP_OK) return rc;
  if (mode != ADP_LT_ZERO && mode != ADP_LT_REFLECT) return ADP_ERR_UNSUPPORTED;
  const int64_t L = lt_conv_len(T, K, stride, pad);
  if (L < 1) return ADP_ERR_SHAPE;
  if (mode == ADP_LT_REFLECT && T <= pad) return ADP_ERR_SHAPE;
  if (B * O * L > LT_MAX_LEN) return ADP_ERR_SHAPE;
  LtGeom g;
  g.B = B; g.C = C; g.T = T; g.O = O; g.K = K; g.s = stride; g.p = pad; g.L = L;
  g.mode = (int)mode;
  const bool vec = stride % 4 == 0 && T % 4 == 0 && lt_aligned(x);
  g.sh = vec ? (int)(pad % 4) : 0;
  g.J = (int)adp_cdiv(K + g.sh, stride);
  g.NQ = (LC_BL + g.J - 1) | 1;
  const int64_t segn = stride * g.NQ;
  // tiled: one channel's polyphase segment fits, and the output rows fill at least a quarter of a fragment
  if (lt_tiled_on() && segn <= LT_CAP && O >= LT_MIN_ROWS) {
    g.cc = (int)(LT_CAP / segn < C ? LT_CAP / segn : C);
    const dim3 grid((unsigned)adp_cdiv(L, LC_BL), (unsigned)adp_cdiv(O, LC_BO), (unsigned)B);
    if (vec) ADP_LAUNCH(lt_conv_tile_kernel<true>, grid, dim3(256), stream, x, w, g, y);
    else ADP_LAUNCH(lt_conv_tile_kernel<false>, grid, dim3(256), stream, x, w, g, y);
  } else {
    g.cc = 0;
    ADP_LAUNCH(lt_conv_plain_kernel, dim3((unsigned)adp_cdiv(B * O * L, 256)), dim3(256), stream, x, w, g, y);
  }
  return ADP_LAUNCH_OK();
}

extern "C" int adp_lt_convt(const float* x, const float* w, int64_t B, int64_t C, int64_t L, int64_t O, int64_t K,
                            int64_t stride, int64_t pad, int64_t mode, int64_t T, float* out, void* stream) {
  if (!x || !w || !out) return ADP_ERR_NULL;
  const int rc = lt_check_common(B, C, O, K, stride, pad);
  if (rc != ADP_OK) return rc;
  if (mode != ADP_LT_PLAIN && mode != ADP_LT_FOLD) return ADP_ERR_UNSUPPORTED;
  if (L < 1 || L > LT_MAX_LEN || T < 1 || T > LT_MAX_LEN) return ADP_ERR_SHAPE;
  if (mode == ADP_LT_PLAIN) {
    if (T != (L - 1) * stride - 2 * pad + K) return ADP_ERR_SHAPE;
  } else {
    if (T <= pad || lt_conv_len(T, K, stride, pad) != L) return ADP_ERR_SHAPE;
  }
  if (B * O * T > LT_MAX_LEN) return ADP_ERR_SHAPE;
  LtTGeom g;
  g.B = B; g.C = C; g.L = L; g.O = O; g.K = K; g.s = stride; g.p = pad; g.T = T;
  g.qf = pad / stride;
  g.OS = O * stride;
  g.mode = (int)mode;
  g.J = (int)adp_cdiv(K, stride);
  g.XW = LD_BQ + g.J - 1;
  const int64_t Q = (pad + T - 1) / stride - g.qf + 1;
  const int64_t chans = LT_KC / g.J + 2;   // channels a reduction chunk of LT_KC (c, j) pairs can touch
  if (lt_tiled_on() && chans * g.XW <= LT_CAP && g.OS >= LT_MIN_ROWS && adp_cdiv(g.OS, LD_BM) <= 65535) {
    const dim3 grid((unsigned)adp_cdiv(Q, LD_BQ), (unsigned)adp_cdiv(g.OS, LD_BM), (unsigned)B);
    const bool vec = stride % 4 == 0 && K % 4 == 0 && lt_aligned(w);
    if (vec) ADP_LAUNCH(lt_convt_tile_kernel<true>, grid, dim3(256), stream, x, w, g, out);
    else ADP_LAUNCH(lt_convt_tile_kernel<false>, grid, dim3(256), stream, x, w, g, out);
    if (mode == ADP_LT_FOLD && pad > 0)
      ADP_LAUNCH(lt_convt_fold_kernel, dim3((unsigned)adp_cdiv(B * O * 2 * pad, 256)), dim3(256), stream, x, w, g, out);
  } else {
    ADP_LAUNCH(lt_convt_plain_kernel, dim3((unsigned)adp_cdiv(B * O * T, 256)), dim3(256), stream, x, w, g, out);
  }
  return ADP_LAUNCH_OK();
}

extern "C" int64_t adp_lt_wgrad_ws_bytes(int64_t B, int64_t A, int64_t Bc, int64_t L, int64_t K) {
  LtWGeom g;
  const int rc = lt_wgrad_plan(B, A, Bc, L, K, &g);
  if (rc != ADP_OK) return rc;
  return (int64_t)g.segs * A * g.BK * (int64_t)sizeof(float);
}

extern "C" int adp_lt_wgrad(const float* u, const float* v, int64_t B, int64_t A, int64_t Bc, int64_t L, int64_t T,
                            int64_t K, int64_t stride, int64_t pad, int64_t mode, float* dw, float* ws, void* stream) {
  if (!u || !v || !dw || !ws) return ADP_ERR_NULL;
  int rc = lt_check_common(B, A, Bc, K, stride, pad);
  if (rc != ADP_OK) return rc;
  if (mode != ADP_LT_ZERO && mode != ADP_LT_REFLECT) return ADP_ERR_UNSUPPORTED;
  if (L < 1 || lt_conv_len(T, K, stride, pad) != L) return ADP_ERR_SHAPE;
  if (mode == ADP_LT_REFLECT && T <= pad) return ADP_ERR_SHAPE;
  LtWGeom g;
  rc = lt_wgrad_plan(B, A, Bc, L, K, &g);
  if (rc != ADP_OK) return rc;
  if (A * g.BK > LT_MAX_LEN) return ADP_ERR_SHAPE;
  g.T = T; g.s = stride; g.p = pad;
  g.mode = (int)mode;
  const int64_t segw = (LW_LCH - 1) * stride + K;
  g.SEGW = (int)segw;
  int64_t nb = (LW_BC - 1) / K + 2;        // channels of v the columns of one tile can touch
  if (nb > Bc) nb = Bc;
  const int64_t ctiles = adp_cdiv(g.BK, LW_BC);
  if (lt_tiled_on() && nb * segw <= LT_CAP && A >= LT_MIN_ROWS && ctiles <= 65535) {
    const dim3 grid((unsigned)adp_cdiv(A, LW_BA), (unsigned)ctiles, (unsigned)g.segs);
    ADP_LAUNCH(lt_wgrad_tile_kernel, grid, dim3(256), stream, u, v, g, ws);
  } else {
    const dim3 grid((unsigned)adp_cdiv(A * g.BK, 256), (unsigned)g.segs);
    ADP_LAUNCH(lt_wgrad_plain_kernel, grid, dim3(256), stream, u, v, g, ws);
  }
  ADP_LAUNCH(lt_wgrad_sum_kernel, dim3((unsigned)adp_cdiv(A * g.BK, 256)), dim3(256), stream, (const float*)ws, A * g.BK,
             g.segs, dw);
  return ADP_LAUNCH_OK();
}
