// The packed-pair LDS FFT shared by the STFT kernels (resample.hip: the STFT loss and the mel spectrogram; spectral.hip: the
// grouped / mel-scaled STFT loss).  Two consecutive real frames a, b of ONE signal are packed as z = a + i b into one N-point
// complex FFT and separated afterwards (st_split).  The FFT is a Stockham radix-4 (one radix-2 pass first when log2 N is odd)
// over LDS: every thread takes its butterflies' operands into registers, barrier, writes them back, barrier.  Twiddles (N/4
// entries, W^2 and W^3 by complex products) and the window are computed into LDS by each workgroup.  Workgroups of 256 threads.
#pragma once
#include "adp_rt.h"

namespace {

constexpr int ST_SPAN_EXTRA = 2048; // staged input floats per signal beyond one frame (forward)

template <int LOGN>
struct StftCfg {
  static constexpr int N = 1 << LOGN;
  static constexpr int PAIRS = N >= 512 ? 1 : 512 / N;  // frame pairs per FFT pass (2 PAIRS transforms: >= 256 butterflies)
  static constexpr int XCAP = N + ST_SPAN_EXTRA;        // staged floats per signal (forward)
  static constexpr int PB = N >= 1024 ? 2 * N : 2048;   // padded samples per backward workgroup
};

__device__ __forceinline__ int64_t st_reflect(int64_t i, int64_t L) {
  if (i < 0) i = -i;
  if (i >= L) i = 2 * (L - 1) - i;
  return i;
}

// twr/twi[m] = e^{-2 pi i m / N}, m < N/4; win = periodic Hann of length W centred in N (torch.stft's zero padding)
template <int LOGN>
__device__ void st_tables(float* twr, float* twi, float* win, int W) {
  constexpr int N = 1 << LOGN;
  const int off = (N - W) / 2;
  for (int m = threadIdx.x; m < N / 4; m += 256) {
    const float a = (float)m * (6.28318530717958647692f / (float)N);
    twr[m] = cosf(a);
    twi[m] = -sinf(a);
  }
  for (int n = threadIdx.x; n < N; n += 256) {
    const int m = n - off;
    win[n] = (m >= 0 && m < W) ? 0.5f - 0.5f * cosf((float)m * (6.28318530717958647692f / (float)W)) : 0.0f;
  }
}

// in-place forward FFT of NB consecutive N-point complex sequences (re/im) by the whole workgroup; starts after a barrier
// that published the input, ends with a barrier
template <int LOGN, int NB>
__device__ void st_fft(float* re, float* im, const float* twr, const float* twi) {
  constexpr int N = 1 << LOGN;
  const int tid = threadIdx.x;
  int Ns = 1;
  if (LOGN & 1) {  // radix-2 pass with unit twiddles
    constexpr int NBF = NB * N / 2;
    constexpr int PER = (NBF + 255) / 256;
    float ar[PER][2], ai[PER][2];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int g = tid + q * 256;
      if (g < NBF) {
        const int base = (g >> (LOGN - 1)) << LOGN, j = g & (N / 2 - 1);
        const float r0 = re[base + j], i0 = im[base + j], r1 = re[base + j + N / 2], i1 = im[base + j + N / 2];
        ar[q][0] = r0 + r1; ai[q][0] = i0 + i1;
        ar[q][1] = r0 - r1; ai[q][1] = i0 - i1;
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int g = tid + q * 256;
      if (g < NBF) {
        const int base = (g >> (LOGN - 1)) << LOGN, j = g & (N / 2 - 1);
        re[base + 2 * j] = ar[q][0]; im[base + 2 * j] = ai[q][0];
        re[base + 2 * j + 1] = ar[q][1]; im[base + 2 * j + 1] = ai[q][1];
      }
    }
    __syncthreads();
    Ns = 2;
  }
  constexpr int NBF = NB * N / 4;
  constexpr int PER = (NBF + 255) / 256;
  for (; Ns < N; Ns *= 4) {
    float vr[PER][4], vi[PER][4];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int g = tid + q * 256;
      if (g < NBF) {
        const int base = (g >> (LOGN - 2)) << LOGN, j = g & (N / 4 - 1), k = j & (Ns - 1);
        const int t = k * (N / (4 * Ns));
        const float w1r = twr[t], w1i = twi[t];
        const float w2r = w1r * w1r - w1i * w1i, w2i = 2.0f * w1r * w1i;
        const float w3r = w1r * w2r - w1i * w2i, w3i = w1r * w2i + w1i * w2r;
        const float x0r = re[base + j], x0i = im[base + j];
        const float u1r = re[base + j + N / 4], u1i = im[base + j + N / 4];
        const float u2r = re[base + j + N / 2], u2i = im[base + j + N / 2];
        const float u3r = re[base + j + 3 * N / 4], u3i = im[base + j + 3 * N / 4];
        const float x1r = u1r * w1r - u1i * w1i, x1i = u1r * w1i + u1i * w1r;
        const float x2r = u2r * w2r - u2i * w2i, x2i = u2r * w2i + u2i * w2r;
        const float x3r = u3r * w3r - u3i * w3i, x3i = u3r * w3i + u3i * w3r;
        const float a0r = x0r + x2r, a0i = x0i + x2i, a1r = x0r - x2r, a1i = x0i - x2i;
        const float a2r = x1r + x3r, a2i = x1i + x3i;
        const float a3r = x1i - x3i, a3i = x3r - x1r;  // (x1 - x3) * (-i)
        vr[q][0] = a0r + a2r; vi[q][0] = a0i + a2i;
        vr[q][1] = a1r + a3r; vi[q][1] = a1i + a3i;
        vr[q][2] = a0r - a2r; vi[q][2] = a0i - a2i;
        vr[q][3] = a1r - a3r; vi[q][3] = a1i - a3i;
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int g = tid + q * 256;
      if (g < NBF) {
        const int base = (g >> (LOGN - 2)) << LOGN, j = g & (N / 4 - 1), k = j & (Ns - 1);
        const int d = base + (j - k) * 4 + k;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          re[d + r * Ns] = vr[q][r];
          im[d + r * Ns] = vi[q][r];
        }
      }
    }
    __syncthreads();
  }
}

// bin k (<= N/2) of the two real frames packed in one transform Z
template <int LOGN>
__device__ __forceinline__ void st_split(const float* re, const float* im, int k, float& xr, float& xi, float& yr,
                                         float& yi) {
  constexpr int N = 1 << LOGN;
  const int kc = (N - k) & (N - 1);
  const float zr = re[k], zi = im[k], cr = re[kc], ci = -im[kc];
  xr = 0.5f * (zr + cr);
  xi = 0.5f * (zi + ci);
  yr = 0.5f * (zi - ci);
  yi = -0.5f * (zr - cr);
}

}  // namespace
