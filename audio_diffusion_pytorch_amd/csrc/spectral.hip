// Grouped / mel-scaled multi-resolution STFT loss and its FIR pre-filter (spectral.py; C-ABI and contract in
// include/adp_spec.h).  The loss is the one of resample.hip (adp_stft_loss_*: same plan, same transforms, same per-bin
// arithmetic, same reductions -- with one group and no filterbank the results are its bits) with three additions:
//
//   pair:  a logical row is the sum or the difference of the two channels of an item, formed where a kernel stages its span;
//          partial sums and norms are kept per group, and the fold launch of the backward unmixes the two gradients.
//   mel:   after the transforms every thread takes the magnitudes of its bins (k and N - k of the x and the y transform)
//          into registers; after a barrier the transform buffers hold the magnitudes [frame][bin] (x in `bre`, y in `bim`)
//          and one thread per (filter, frame) walks the filter's [lo, hi) bins.  The backward leaves dL/dM per (frame,
//          filter) in the free tail of `bre` and every bin gathers its (at most two, for triangles) filters from there.
//   fir:   out[i] = sum_j taps[j] x[i + j - T/2] from an LDS-staged span, accumulated in double and rounded once.
#include "adp_rt.h"
#include "adp_spec.h"
#include "stft_fft.h"

namespace {

constexpr int SP_MAXR = 4;            // resolutions per call
constexpr int SP_NORMS = 4 * SP_MAXR; // forward workspace head: ||M_y - M_x||, ||M_y|| per (group, resolution)

struct SpecPlan {
  int nres, pair, groups;
  int n[SP_MAXR], logn[SP_MAXR], hop[SP_MAXR], win[SP_MAXR];
  int frames[SP_MAXR];       // 1 + L / h
  int fpb[SP_MAXR];          // frames per forward workgroup
  int chunks[SP_MAXR];       // forward workgroups per row
  int nb[SP_MAXR];           // filters of the resolution's filterbank (0: none)
  int64_t part_off[SP_MAXR]; // float offset of the resolution's forward partials in the forward workspace
  int64_t gp_off[SP_MAXR];   // float offset of the resolution's padded-row gradient in the backward workspace
  int64_t fb_off[SP_MAXR];   // float offset of the resolution's filterbank in fb
  int64_t mr_off[SP_MAXR];   // int offset of its [nb, 2] filter ranges
  int64_t br_off[SP_MAXR];   // int offset of its [N/2 + 1, 2] bin ranges
  int64_t rows, rpg, length; // signals, signals per group
  float w_sc, w_log, w_lin, eps;
  float wg[2];               // w_sum, w_diff
};

// sample j of logical row (group g, item b): the row itself, or the sum / difference of the item's two channels
struct SpecRow {
  const float* a;
  int64_t L;
  int mode;  // 0: a[j]; 1: a[j] + a[j + L]; 2: a[j] - a[j + L]
  __device__ __forceinline__ float operator()(int64_t j) const {
    if (mode == 0) return a[j];
    const float u = a[j], v = a[j + L];
    return mode == 1 ? u + v : u - v;
  }
};

__device__ __forceinline__ SpecRow spec_row(const float* base, const SpecPlan& p, int64_t lr) {
  SpecRow s;
  s.L = p.length;
  if (!p.pair) {
    s.a = base + lr * p.length;
    s.mode = 0;
  } else {
    const int64_t g = lr / p.rpg, b = lr - g * p.rpg;
    s.a = base + 2 * b * p.length;
    s.mode = g ? 2 : 1;
  }
  return s;
}

template <int LOGN, bool MEL>
__global__ __launch_bounds__(256) void spec_fwd_kernel(const float* x, const float* y, const float* fb,
                                                       const int32_t* mrange, SpecPlan p, int r, float* ws) {
  using C = StftCfg<LOGN>;
  constexpr int N = C::N, NP = C::PAIRS, NK = N / 2 + 1, NF = 2 * NP, ITER = (NP * NK + 255) / 256;
  __shared__ float xs[C::XCAP];
  __shared__ float ys[C::XCAP];
  __shared__ float bre[2 * NP * N];  // transforms [0, NP): pairs of x frames; [NP, 2 NP): the same pairs of y frames
  __shared__ float bim[2 * NP * N];
  __shared__ float twr[N / 4];
  __shared__ float twi[N / 4];
  __shared__ float win[N];
  __shared__ float red[4][4];
  const int tid = threadIdx.x;
  const int hop = p.hop[r], fpb = p.fpb[r];
  const int64_t row = blockIdx.y, L = p.length;
  const int f0 = blockIdx.x * fpb;
  const int nf = (p.frames[r] - f0 < fpb) ? p.frames[r] - f0 : fpb;
  const float eps = p.eps;
  st_tables<LOGN>(twr, twi, win, p.win[r]);
  const int64_t s0 = (int64_t)f0 * hop - N / 2;  // original-signal index of the span's first (padded) sample
  const int span = (nf - 1) * hop + N;
  const SpecRow xr = spec_row(x, p, row), yr = spec_row(y, p, row);
  for (int i = tid; i < span; i += 256) {
    const int64_t src = st_reflect(s0 + i, L);
    xs[i] = xr(src);
    ys[i] = yr(src);
  }
  __syncthreads();
  float s_d = 0.0f, s_y = 0.0f, s_log = 0.0f, s_lin = 0.0f;
  for (int fb0 = 0; fb0 < nf; fb0 += 2 * NP) {
    for (int i = tid; i < 2 * NP * N; i += 256) {
      const int s = i >> LOGN, n = i & (N - 1);
      const int ta = fb0 + 2 * (s % NP);  // frames ta, ta + 1 of x (s < NP) or of y
      const float* src = s < NP ? xs : ys;
      bre[i] = ta < nf ? win[n] * src[ta * hop + n] : 0.0f;
      bim[i] = ta + 1 < nf ? win[n] * src[(ta + 1) * hop + n] : 0.0f;
    }
    __syncthreads();
    st_fft<LOGN, 2 * NP>(bre, bim, twr, twi);
    if constexpr (!MEL) {
      for (int i = tid; i < NP * NK; i += 256) {
        const int s = i / NK, k = i - s * NK;
        const int ta = fb0 + 2 * s;
        if (ta >= nf) continue;
        float X[2][2], Y[2][2];  // [frame ta / ta + 1][re, im]
        st_split<LOGN>(bre + s * N, bim + s * N, k, X[0][0], X[0][1], X[1][0], X[1][1]);
        st_split<LOGN>(bre + (NP + s) * N, bim + (NP + s) * N, k, Y[0][0], Y[0][1], Y[1][0], Y[1][1]);
        for (int e = 0; e < 2 && ta + e < nf; ++e) {
          const float mx = sqrtf(fmaxf(X[e][0] * X[e][0] + X[e][1] * X[e][1], eps));
          const float my = sqrtf(fmaxf(Y[e][0] * Y[e][0] + Y[e][1] * Y[e][1], eps));
          const float d = my - mx;
          s_d = fmaf(d, d, s_d);
          s_y = fmaf(my, my, s_y);
          s_log += fabsf(logf(mx) - logf(my));
          s_lin += fabsf(mx - my);
        }
      }
      __syncthreads();
    } else {
      float mg[ITER][4];  // m_x of frames ta, ta + 1, then m_y
#pragma unroll
      for (int q = 0; q < ITER; ++q) {
        const int i = tid + q * 256;
        if (i < NP * NK) {
          const int s = i / NK, k = i - s * NK;
          float X[2][2], Y[2][2];
          st_split<LOGN>(bre + s * N, bim + s * N, k, X[0][0], X[0][1], X[1][0], X[1][1]);
          st_split<LOGN>(bre + (NP + s) * N, bim + (NP + s) * N, k, Y[0][0], Y[0][1], Y[1][0], Y[1][1]);
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            mg[q][e] = sqrtf(fmaxf(X[e][0] * X[e][0] + X[e][1] * X[e][1], eps));
            mg[q][2 + e] = sqrtf(fmaxf(Y[e][0] * Y[e][0] + Y[e][1] * Y[e][1], eps));
          }
        }
      }
      __syncthreads();  // every bin of every transform is in registers: the buffers become the magnitudes [frame][bin]
#pragma unroll
      for (int q = 0; q < ITER; ++q) {
        const int i = tid + q * 256;
        if (i < NP * NK) {
          const int s = i / NK, k = i - s * NK;
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            bre[(2 * s + e) * NK + k] = mg[q][e];
            bim[(2 * s + e) * NK + k] = mg[q][2 + e];
          }
        }
      }
      __syncthreads();
      const int nb = p.nb[r];
      const int cnt = (nf - fb0 < NF) ? nf - fb0 : NF;
      const float* fbr = fb + p.fb_off[r];
      const int32_t* mr = mrange ? mrange + p.mr_off[r] : nullptr;
      for (int i = tid; i < nb * NF; i += 256) {
        const int m = i / NF, e = i - m * NF;
        if (e >= cnt) continue;
        int lo = mr ? mr[2 * m] : 0, hi = mr ? mr[2 * m + 1] : NK;
        lo = lo < 0 ? 0 : lo;
        hi = hi > NK ? NK : hi;
        const float* fr = fbr + (int64_t)m * NK;
        const float* gx = bre + e * NK;
        const float* gy = bim + e * NK;
        float mx = 0.0f, my = 0.0f;
        for (int k = lo; k < hi; ++k) {
          const float w = fr[k];
          mx = fmaf(w, gx[k], mx);
          my = fmaf(w, gy[k], my);
        }
        const float d = my - mx;
        s_d = fmaf(d, d, s_d);
        s_y = fmaf(my, my, s_y);
        s_log += fabsf(logf(mx) - logf(my));
        s_lin += fabsf(mx - my);
      }
      __syncthreads();
    }
  }
  s_d = adp_wave_sum(s_d);
  s_y = adp_wave_sum(s_y);
  s_log = adp_wave_sum(s_log);
  s_lin = adp_wave_sum(s_lin);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = s_d;
    red[tid >> 6][1] = s_y;
    red[tid >> 6][2] = s_log;
    red[tid >> 6][3] = s_lin;
  }
  __syncthreads();
  if (tid < 4) {
    float* out = ws + p.part_off[r] + (row * p.chunks[r] + blockIdx.x) * 4;
    out[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  }
}

// one wave: every (group, resolution)'s partials in double, lane-strided then in lane order (fixed order), -> loss and norms
__global__ __launch_bounds__(64) void spec_final_kernel(float* ws, SpecPlan p, float* loss) {
  __shared__ double part[64];
  const int tid = threadIdx.x;
  double total[2] = {0.0, 0.0};
  for (int g = 0; g < p.groups; ++g) {
    for (int r = 0; r < p.nres; ++r) {
      const int64_t nb = p.rpg * p.chunks[r];
      const float* src = ws + p.part_off[r] + (int64_t)g * nb * 4;
      double q[4];
      for (int c = 0; c < 4; ++c) {
        double s = 0.0;
        for (int64_t i = tid; i < nb; i += 64) s += (double)src[i * 4 + c];
        part[tid] = s;
        __syncthreads();
        double t = 0.0;
        for (int i = 0; i < 64; ++i) t += part[i];
        q[c] = t;
        __syncthreads();
      }
      const int bins = p.nb[r] ? p.nb[r] : p.n[r] / 2 + 1;
      const double count = (double)p.rpg * (double)p.frames[r] * (double)bins;
      const double nd = sqrt(q[0]), ny = sqrt(q[1]);
      total[g] += (double)p.w_sc * (nd / ny) + (double)p.w_log * (q[2] / count) + (double)p.w_lin * (q[3] / count);
      if (tid == 0) {
        ws[2 * (g * SP_MAXR + r)] = (float)nd;
        ws[2 * (g * SP_MAXR + r) + 1] = (float)ny;
      }
    }
  }
  if (tid == 0) {
    if (p.groups == 1)
      loss[0] = (float)(total[0] / (double)p.nres);
    else
      loss[0] = (float)(0.5 * ((double)p.wg[0] * (total[0] / (double)p.nres) + (double)p.wg[1] * (total[1] / (double)p.nres)));
  }
}

template <int LOGN, bool MEL>
__global__ __launch_bounds__(256) void spec_bwd_kernel(const float* x, const float* y, const float* gloss,
                                                       const float* norms, const float* fb, const int32_t* mrange,
                                                       const int32_t* brange, SpecPlan p, int r, float* ws) {
  using C = StftCfg<LOGN>;
  constexpr int N = C::N, NP = C::PAIRS, NK = N / 2 + 1, NF = 2 * NP, PB = C::PB, NACC = PB / 256;
  constexpr int ITER = (NP * NK + 255) / 256, DOFF = NF * NK;  // dL/dM [frame][filter] behind the x magnitudes in bre
  __shared__ float bre[2 * NP * N];  // as in the forward: x pairs, then the same y pairs
  __shared__ float bim[2 * NP * N];
  __shared__ float twr[N / 4];
  __shared__ float twi[N / 4];
  __shared__ float win[N];
  const int tid = threadIdx.x;
  const int hop = p.hop[r], F = p.frames[r];
  const int64_t row = blockIdx.y, L = p.length, Lp = L + N;
  const int64_t q0 = (int64_t)blockIdx.x * PB;  // first padded sample owned by this workgroup
  const float eps = p.eps;
  st_tables<LOGN>(twr, twi, win, p.win[r]);
  // dL/dM = c_sc (M_x - M_y) + c_log sign(log M_x - log M_y) / M_x + c_lin sign(M_x - M_y)
  const int grp = p.pair ? (int)(row / p.rpg) : 0;
  float scale = (gloss ? gloss[0] : 1.0f) / (float)p.nres;
  if (p.pair) scale *= 0.5f * p.wg[grp];
  const float nd = norms[2 * (grp * SP_MAXR + r)], ny = norms[2 * (grp * SP_MAXR + r) + 1];
  const float count = (float)((double)p.rpg * (double)F * (double)(MEL ? p.nb[r] : NK));
  const float c_sc = nd > 0.0f ? scale * p.w_sc / (nd * ny) : 0.0f;
  const float c_log = scale * p.w_log / count, c_lin = scale * p.w_lin / count;
  // frames t with t*h <= q0 + PB - 1 and t*h + N - 1 >= q0
  const int64_t lo = q0 - N + 1;
  const int t_lo = lo <= 0 ? 0 : (int)((lo + hop - 1) / hop);
  const int t_hi = (int)((q0 + PB - 1) / hop < F - 1 ? (q0 + PB - 1) / hop : F - 1);
  const SpecRow xr = spec_row(x, p, row), yr = spec_row(y, p, row);
  float acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j) acc[j] = 0.0f;
  __syncthreads();
  for (int t = t_lo; t <= t_hi; t += 2 * NP) {
    for (int i = tid; i < 2 * NP * N; i += 256) {
      const int s = i >> LOGN, n = i & (N - 1);
      const int ta = t + 2 * (s % NP);  // frames ta, ta + 1 of x (s < NP) or of y
      const SpecRow& src = s < NP ? xr : yr;
      bre[i] = ta <= t_hi ? win[n] * src(st_reflect((int64_t)ta * hop + n - N / 2, L)) : 0.0f;
      bim[i] = ta + 1 <= t_hi ? win[n] * src(st_reflect((int64_t)(ta + 1) * hop + n - N / 2, L)) : 0.0f;
    }
    __syncthreads();
    st_fft<LOGN, 2 * NP>(bre, bim, twr, twi);
    if constexpr (!MEL) {
      // G of frames ta, ta + 1, and P = S_ta + i S_ta+1 (S: the Hermitian extension of G), conjugated, into the x transform;
      // bins k and N-k are read and overwritten by the same thread
      for (int i = tid; i < NP * NK; i += 256) {
        const int s = i / NK, k = i - s * NK;
        const int ta = t + 2 * s;
        if (ta > t_hi) continue;
        float* re = bre + s * N;
        float* im = bim + s * N;
        float X[2][2], Y[2][2], G[2][2];  // [frame ta / ta + 1][re, im]
        st_split<LOGN>(re, im, k, X[0][0], X[0][1], X[1][0], X[1][1]);
        st_split<LOGN>(bre + (NP + s) * N, bim + (NP + s) * N, k, Y[0][0], Y[0][1], Y[1][0], Y[1][1]);
        for (int e = 0; e < 2; ++e) {
          const float px = X[e][0] * X[e][0] + X[e][1] * X[e][1];
          const float mx = sqrtf(fmaxf(px, eps)), my = sqrtf(fmaxf(Y[e][0] * Y[e][0] + Y[e][1] * Y[e][1], eps));
          const float dl = logf(mx) - logf(my), dm = mx - my;
          const float sl = (float)((dl > 0.0f) - (dl < 0.0f)), sm = (float)((dm > 0.0f) - (dm < 0.0f));
          const float gm = c_sc * dm + c_log * sl / mx + c_lin * sm;
          const float g = (px >= eps && ta + e <= t_hi) ? gm / mx : 0.0f;
          G[e][0] = g * X[e][0];
          G[e][1] = g * X[e][1];
        }
        if (k == 0 || k == N / 2) {
          re[k] = G[0][0];
          im[k] = -G[1][0];
        } else {
          re[k] = 0.5f * (G[0][0] - G[1][1]);
          im[k] = -0.5f * (G[0][1] + G[1][0]);
          re[N - k] = 0.5f * (G[0][0] + G[1][1]);
          im[N - k] = 0.5f * (G[0][1] - G[1][0]);
        }
      }
    } else {
      float XR[ITER][4];  // X of frames ta, ta + 1: re, im, re, im
      float MG[ITER][4];  // m_x of the two frames, then m_y
#pragma unroll
      for (int q = 0; q < ITER; ++q) {
        const int i = tid + q * 256;
        if (i < NP * NK) {
          const int s = i / NK, k = i - s * NK;
          float Y[2][2];
          st_split<LOGN>(bre + s * N, bim + s * N, k, XR[q][0], XR[q][1], XR[q][2], XR[q][3]);
          st_split<LOGN>(bre + (NP + s) * N, bim + (NP + s) * N, k, Y[0][0], Y[0][1], Y[1][0], Y[1][1]);
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            MG[q][e] = sqrtf(fmaxf(XR[q][2 * e] * XR[q][2 * e] + XR[q][2 * e + 1] * XR[q][2 * e + 1], eps));
            MG[q][2 + e] = sqrtf(fmaxf(Y[e][0] * Y[e][0] + Y[e][1] * Y[e][1], eps));
          }
        }
      }
      __syncthreads();  // every bin is in registers: the buffers become the magnitudes [frame][bin]
#pragma unroll
      for (int q = 0; q < ITER; ++q) {
        const int i = tid + q * 256;
        if (i < NP * NK) {
          const int s = i / NK, k = i - s * NK;
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            bre[(2 * s + e) * NK + k] = MG[q][e];
            bim[(2 * s + e) * NK + k] = MG[q][2 + e];
          }
        }
      }
      __syncthreads();
      const int nb = p.nb[r];
      const float* fbr = fb + p.fb_off[r];
      const int32_t* mr = mrange ? mrange + p.mr_off[r] : nullptr;
      const int32_t* br = brange ? brange + p.br_off[r] : nullptr;
      float* D = bre + DOFF;  // [NF][nb], nb <= N/2 - 1: inside bre, behind the magnitudes and behind transform NP - 1
      for (int i = tid; i < nb * NF; i += 256) {
        const int m = i / NF, e = i - m * NF;
        int lo_k = mr ? mr[2 * m] : 0, hi_k = mr ? mr[2 * m + 1] : NK;
        lo_k = lo_k < 0 ? 0 : lo_k;
        hi_k = hi_k > NK ? NK : hi_k;
        const float* fr = fbr + (int64_t)m * NK;
        const float* gx = bre + e * NK;
        const float* gy = bim + e * NK;
        float mx = 0.0f, my = 0.0f;
        for (int k = lo_k; k < hi_k; ++k) {
          const float w = fr[k];
          mx = fmaf(w, gx[k], mx);
          my = fmaf(w, gy[k], my);
        }
        const float dl = logf(mx) - logf(my), dm = mx - my;
        const float sl = (float)((dl > 0.0f) - (dl < 0.0f)), sm = (float)((dm > 0.0f) - (dm < 0.0f));
        D[e * nb + m] = t + e <= t_hi ? c_sc * dm + c_log * sl / mx + c_lin * sm : 0.0f;
      }
      __syncthreads();
      // dL/dm_x[k] = sum_j fb[j, k] dL/dM[j]; P lands in transforms [0, NP) of bre / bim: below D, over magnitudes no one reads
#pragma unroll
      for (int q = 0; q < ITER; ++q) {
        const int i = tid + q * 256;
        if (i < NP * NK) {
          const int s = i / NK, k = i - s * NK;
          const int ta = t + 2 * s;
          int lo_j = br ? br[2 * k] : 0, hi_j = br ? br[2 * k + 1] : nb;
          lo_j = lo_j < 0 ? 0 : lo_j;
          hi_j = hi_j > nb ? nb : hi_j;
          float G[2][2];
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const float* De = D + (2 * s + e) * nb;
            float gm = 0.0f;
            for (int j = lo_j; j < hi_j; ++j) gm = fmaf(fbr[(int64_t)j * NK + k], De[j], gm);
            const float px = XR[q][2 * e] * XR[q][2 * e] + XR[q][2 * e + 1] * XR[q][2 * e + 1];
            const float g = (px >= eps && ta + e <= t_hi) ? gm / MG[q][e] : 0.0f;
            G[e][0] = g * XR[q][2 * e];
            G[e][1] = g * XR[q][2 * e + 1];
          }
          float* re = bre + s * N;
          float* im = bim + s * N;
          if (k == 0 || k == N / 2) {
            re[k] = G[0][0];
            im[k] = -G[1][0];
          } else {
            re[k] = 0.5f * (G[0][0] - G[1][1]);
            im[k] = -0.5f * (G[0][1] + G[1][0]);
            re[N - k] = 0.5f * (G[0][0] + G[1][1]);
            im[N - k] = 0.5f * (G[0][1] - G[1][0]);
          }
        }
      }
    }
    __syncthreads();
    // FFT(conj P) = conj(IFFT_unnormalised(P)): real part = gradient of frame ta, minus the imaginary part = of ta + 1
    st_fft<LOGN, NP>(bre, bim, twr, twi);
#pragma unroll
    for (int j = 0; j < NACC; ++j) {
      const int64_t q = q0 + tid + j * 256;
      for (int s = 0; s < NP; ++s) {
        const int ta = t + 2 * s;
        const int64_t na = q - (int64_t)ta * hop, nb2 = na - hop;
        if (ta <= t_hi && na >= 0 && na < N) acc[j] = fmaf(win[na], bre[s * N + na], acc[j]);
        if (ta + 1 <= t_hi && nb2 >= 0 && nb2 < N) acc[j] = fmaf(win[nb2], -bim[s * N + nb2], acc[j]);
      }
    }
    __syncthreads();
  }
  float* gp = ws + p.gp_off[r] + row * Lp;
#pragma unroll
  for (int j = 0; j < NACC; ++j) {
    const int64_t q = q0 + tid + j * 256;
    if (q < Lp) gp[q] = acc[j];
  }
}

// the gradient of logical row lr at sample i: sum over resolutions of the padded-row gradient at i + N/2 and at its
// reflect-pad mirrors
__device__ __forceinline__ float spec_fold(const float* ws, const SpecPlan& p, int64_t lr, int64_t i) {
  const int64_t L = p.length;
  float g = 0.0f;
  for (int r = 0; r < p.nres; ++r) {
    const int64_t c = p.n[r] / 2;
    const float* gp = ws + p.gp_off[r] + lr * (L + p.n[r]);
    g += gp[i + c];
    if (i >= 1 && i <= c) g += gp[c - i];
    if (i >= L - 1 - c && i <= L - 2) g += gp[2 * (L - 1) - i + c];
  }
  return g;
}

// dx[row, i]: the fold, and with pair the unmix dx[2b] = g_s + g_d, dx[2b + 1] = g_s - g_d
__global__ __launch_bounds__(256) void spec_fold_kernel(const float* ws, SpecPlan p, float* dx) {
  const int64_t L = p.length;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = blockIdx.y;
  if (i >= L) return;
  if (!p.pair) {
    dx[row * L + i] = spec_fold(ws, p, row, i);
  } else {
    const int64_t b = row >> 1;
    const float gs = spec_fold(ws, p, b, i), gd = spec_fold(ws, p, p.rpg + b, i);
    dx[row * L + i] = (row & 1) ? gs - gd : gs + gd;
  }
}

// validates the call and fills the plan; workspace sizes in floats
int spec_plan(int64_t rows, int64_t length, int64_t pair, int64_t nres, const int64_t* res, const int64_t* n_bins,
              float w_sc, float w_log, float w_lin, float eps, float w_sum, float w_diff, SpecPlan* p, int64_t* fwd_floats,
              int64_t* bwd_floats) {
  if (nres < 1 || nres > SP_MAXR || rows < 1 || rows > 65535 || length < 2 || length >= ((int64_t)1 << 30))
    return ADP_ERR_SHAPE;
  if ((pair != 0 && pair != 1) || (pair && (rows & 1))) return ADP_ERR_SHAPE;
  p->nres = (int)nres;
  p->pair = (int)pair;
  p->groups = pair ? 2 : 1;
  p->rows = rows;
  p->rpg = pair ? rows / 2 : rows;
  p->length = length;
  p->w_sc = w_sc;
  p->w_log = w_log;
  p->w_lin = w_lin;
  p->eps = eps;
  p->wg[0] = w_sum;
  p->wg[1] = w_diff;
  int64_t fo = SP_NORMS, bo = 0, fbo = 0, mro = 0, bro = 0;
  for (int r = 0; r < nres; ++r) {
    const int64_t N = res[3 * r], h = res[3 * r + 1], W = res[3 * r + 2], J = n_bins ? n_bins[r] : 0;
    int logn = 0;
    while (logn < 13 && ((int64_t)1 << logn) < N) ++logn;
    if (((int64_t)1 << logn) != N || logn < 6 || logn > 12) return ADP_ERR_UNSUPPORTED;
    if (h < 1 || W < 1 || W > N) return ADP_ERR_UNSUPPORTED;
    if (length <= N / 2 || J < 0) return ADP_ERR_SHAPE;  // reflect padding needs N/2 < L
    if (J > N / 2 - 1) return ADP_ERR_UNSUPPORTED;
    const int64_t F = 1 + length / h;
    const int64_t per_pass = N >= 512 ? 2 : 1024 / N;  // 2 * StftCfg<LOGN>::PAIRS
    int64_t fpb = 1 + ST_SPAN_EXTRA / h;
    if (fpb > 16 * per_pass) fpb = 16 * per_pass;
    p->n[r] = (int)N;
    p->logn[r] = logn;
    p->hop[r] = (int)h;
    p->win[r] = (int)W;
    p->frames[r] = (int)F;
    p->fpb[r] = (int)fpb;
    p->chunks[r] = (int)adp_cdiv(F, fpb);
    p->nb[r] = (int)J;
    p->part_off[r] = fo;
    fo += rows * p->chunks[r] * 4;
    p->gp_off[r] = bo;
    bo += rows * (length + N);
    p->fb_off[r] = fbo;
    p->mr_off[r] = mro;
    p->br_off[r] = bro;
    if (J > 0) {
      fbo += J * (N / 2 + 1);
      mro += 2 * J;
      bro += 2 * (N / 2 + 1);
    }
  }
  if (fwd_floats) *fwd_floats = fo;
  if (bwd_floats) *bwd_floats = bo;
  return ADP_OK;
}

// whether a resolution of the call has a filterbank (read before the plan: the NULL answers come first)
bool spec_has_mel(int64_t nres, const int64_t* n_bins) {
  if (!n_bins || nres < 1 || nres > SP_MAXR) return false;  // (a bad nres is refused by the plan; n_bins has nres entries)
  for (int64_t r = 0; r < nres; ++r)
    if (n_bins[r] > 0) return true;
  return false;
}

inline bool spec_off4(const void* q) { return ((uintptr_t)q & 3) != 0; }

#define ADP_SPEC_DISPATCH(LAUNCH)                                  \
  switch (p.logn[r]) {                                             \
    case 6: if (p.nb[r]) LAUNCH(6, true); else LAUNCH(6, false); break;     \
    case 7: if (p.nb[r]) LAUNCH(7, true); else LAUNCH(7, false); break;     \
    case 8: if (p.nb[r]) LAUNCH(8, true); else LAUNCH(8, false); break;     \
    case 9: if (p.nb[r]) LAUNCH(9, true); else LAUNCH(9, false); break;     \
    case 10: if (p.nb[r]) LAUNCH(10, true); else LAUNCH(10, false); break;  \
    case 11: if (p.nb[r]) LAUNCH(11, true); else LAUNCH(11, false); break;  \
    default: if (p.nb[r]) LAUNCH(12, true); else LAUNCH(12, false); break;  \
  }

// ---- FIR
constexpr int FIR_RUN = 1024;    // outputs per workgroup
constexpr int FIR_MAXT = 255;    // taps
constexpr int FIR_XCAP = FIR_RUN + FIR_MAXT - 1 + 3;

__global__ __launch_bounds__(256) void spec_fir_kernel(const float* x, const float* taps, int64_t length, int T,
                                                       int64_t chunks, float* out) {
  __shared__ float xs[FIR_XCAP];
  __shared__ float hs[FIR_MAXT];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x / chunks;
  const int64_t o0 = (blockIdx.x - row * chunks) * FIR_RUN;
  const int run = length - o0 < FIR_RUN ? (int)(length - o0) : FIR_RUN;
  const int span = run + T - 1;
  const int64_t g0 = o0 - T / 2;  // row index of the span's first sample (may be < 0)
  const float* xr = x + row * length;
  for (int j = tid; j < T; j += 256) hs[j] = taps[j];
  // the elements in front of the first 16-byte boundary, then groups of four: one 16-byte load where the whole group lies in
  // the row, single elements (zeros outside the row) otherwise
  const int64_t word = (int64_t)((uintptr_t)xr >> 2) + g0;  // the span's first sample, in 4-byte words of address space
  const int head = (int)((4 - (word & 3)) & 3);
  for (int i = tid; i < head && i < span; i += 256) {
    const int64_t g = g0 + i;
    xs[i] = (g >= 0 && g < length) ? xr[g] : 0.0f;
  }
  const int nq = span > head ? (span - head + 3) / 4 : 0;
  for (int q = tid; q < nq; q += 256) {
    const int i = head + 4 * q;
    const int64_t g = g0 + i;
    if (g >= 0 && g + 3 < length && i + 3 < span) {
      const f32x4 v = *(const f32x4*)(xr + g);
      xs[i] = v[0];
      xs[i + 1] = v[1];
      xs[i + 2] = v[2];
      xs[i + 3] = v[3];
    } else {
      for (int u = 0; u < 4; ++u)
        if (i + u < span) xs[i + u] = (g + u >= 0 && g + u < length) ? xr[g + u] : 0.0f;
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < FIR_RUN / 256; ++u) {
    const int o = tid + u * 256;
    if (o < run) {
      double a = 0.0;  // every product is exact in double; one rounding to float at the end
      for (int j = 0; j < T; ++j) a = fma((double)hs[j], (double)xs[o + j], a);
      out[row * length + o0 + o] = (float)a;
    }
  }
}

}  // namespace

extern "C" int64_t adp_spec_loss_ws_bytes(int64_t rows, int64_t length, int64_t pair, int64_t nres, const int64_t* res,
                                          const int64_t* n_bins, int64_t backward) {
  if (!res) return ADP_ERR_NULL;
  SpecPlan p;
  int64_t f = 0, b = 0;
  const int rc = spec_plan(rows, length, pair, nres, res, n_bins, 1.0f, 1.0f, 0.0f, 1e-8f, 1.0f, 1.0f, &p, &f, &b);
  if (rc != ADP_OK) return rc;
  return (backward ? b : f) * (int64_t)sizeof(float);
}

extern "C" int adp_spec_loss_fwd(const float* x, const float* y, int64_t rows, int64_t length, int64_t pair, int64_t nres,
                                 const int64_t* res, const int64_t* n_bins, const float* fb, const int32_t* mel_range,
                                 float w_sc, float w_log, float w_lin, float eps, float w_sum, float w_diff, float* loss,
                                 float* ws, void* stream) {
  if (!x || !y || !res || !loss || !ws || (spec_has_mel(nres, n_bins) && !fb)) return ADP_ERR_NULL;
  SpecPlan p;
  const int rc = spec_plan(rows, length, pair, nres, res, n_bins, w_sc, w_log, w_lin, eps, w_sum, w_diff, &p, nullptr,
                           nullptr);
  if (rc != ADP_OK) return rc;
  if (spec_off4(x) || spec_off4(y) || spec_off4(fb) || spec_off4(mel_range) || spec_off4(loss) || spec_off4(ws))
    return ADP_ERR_ALIGN;
  for (int r = 0; r < p.nres; ++r) {
    const dim3 grid((unsigned)p.chunks[r], (unsigned)rows);
#define ADP_SPEC_FWD(LG, MEL) \
  ADP_LAUNCH((spec_fwd_kernel<LG, MEL>), grid, dim3(256), stream, x, y, fb, mel_range, p, r, ws)
    ADP_SPEC_DISPATCH(ADP_SPEC_FWD)
#undef ADP_SPEC_FWD
  }
  ADP_LAUNCH(spec_final_kernel, dim3(1), dim3(64), stream, ws, p, loss);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_spec_loss_bwd(const float* x, const float* y, const float* gloss, const float* ws_fwd, int64_t rows,
                                 int64_t length, int64_t pair, int64_t nres, const int64_t* res, const int64_t* n_bins,
                                 const float* fb, const int32_t* mel_range, const int32_t* bin_range, float w_sc, float w_log,
                                 float w_lin, float eps, float w_sum, float w_diff, float* dx, float* ws, void* stream) {
  if (!x || !y || !ws_fwd || !res || !dx || !ws || (spec_has_mel(nres, n_bins) && !fb)) return ADP_ERR_NULL;
  SpecPlan p;
  const int rc = spec_plan(rows, length, pair, nres, res, n_bins, w_sc, w_log, w_lin, eps, w_sum, w_diff, &p, nullptr,
                           nullptr);
  if (rc != ADP_OK) return rc;
  if (spec_off4(x) || spec_off4(y) || spec_off4(gloss) || spec_off4(ws_fwd) || spec_off4(fb) || spec_off4(mel_range) ||
      spec_off4(bin_range) || spec_off4(dx) || spec_off4(ws))
    return ADP_ERR_ALIGN;
  for (int r = 0; r < p.nres; ++r) {
    const int64_t pb = p.n[r] >= 1024 ? 2 * (int64_t)p.n[r] : 2048;  // StftCfg<LOGN>::PB
    const dim3 grid((unsigned)adp_cdiv(length + p.n[r], pb), (unsigned)rows);
#define ADP_SPEC_BWD(LG, MEL)                                                                                      \
  ADP_LAUNCH((spec_bwd_kernel<LG, MEL>), grid, dim3(256), stream, x, y, gloss, ws_fwd, fb, mel_range, bin_range, p, r, \
             ws)
    ADP_SPEC_DISPATCH(ADP_SPEC_BWD)
#undef ADP_SPEC_BWD
  }
  ADP_LAUNCH(spec_fold_kernel, dim3((unsigned)adp_cdiv(length, 256), (unsigned)rows), dim3(256), stream, ws, p, dx);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_spec_fir(const float* x, const float* taps, int64_t rows, int64_t length, int64_t ntaps, float* out,
                            void* stream) {
  if (!x || !taps || !out) return ADP_ERR_NULL;
  if (rows < 0 || length < 0 || ntaps < 1 || ntaps > FIR_MAXT || !(ntaps & 1)) return ADP_ERR_SHAPE;
  const int64_t chunks = adp_cdiv(length, FIR_RUN);
  if (rows > 0 && chunks > 0x7fffffff / rows) return ADP_ERR_SHAPE;
  if (spec_off4(x) || spec_off4(taps) || spec_off4(out)) return ADP_ERR_ALIGN;
  if (rows == 0 || length == 0) return ADP_OK;
  ADP_LAUNCH(spec_fir_kernel, dim3((unsigned)(rows * chunks)), dim3(256), stream, x, taps, length, (int)ntaps, chunks, out);
  return ADP_LAUNCH_OK();
}
