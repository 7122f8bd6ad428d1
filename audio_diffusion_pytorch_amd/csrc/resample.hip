// Windowed-sinc polyphase resampler (utils.resample / downsample / upsample of
// /root/reference/audio_diffusion_pytorch/utils.py:82-117; the DiffusionUpsampler path, models.py:149-153, :163;
// SURVEY.md 8f-1).  The reference pads the waveform, runs ONE strided conv1d with `fo` output channels (one per
// output phase) and interleaves the phases with a rearrange "(b c) k l -> b c (l k)"; here the padding, the
// interleave and the final crop are index arithmetic inside one streaming kernel:
//
//   out[row, l*fo + k] = sum_{j < J} kern[k*J + j] * xpad[row, l*fi + j],   xpad[i] = x[i - width] or 0
//
// A workgroup owns 256 consecutive outputs of one row; the input span they touch ((256/fo)*fi + J samples) and the
// fo x J coefficient table are staged in LDS with coalesced loads, then every lane runs its J-tap dot product from
// LDS (lanes of one phase read consecutive addresses, a phase's coefficients are broadcast).
#include "adp_rt.h"
#include "adp.h"
#include "stft_fft.h"

namespace {

constexpr int RS_OUT = 256;      // outputs per workgroup
constexpr int RS_XCAP = 6144;    // floats of input span staged in LDS
constexpr int RS_KCAP = 4096;    // floats of coefficient table staged in LDS

__global__ __launch_bounds__(256) void resample_kernel(const float* x, const float* kern, int64_t length, int fi, int fo,
                                                       int J, int width, int64_t out_len, float* out) {
  __shared__ float xs[RS_XCAP];
  __shared__ float ks[RS_KCAP];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.y;
  const int64_t o0 = (int64_t)blockIdx.x * RS_OUT;
  const int64_t o_last = (o0 + RS_OUT - 1 < out_len - 1) ? o0 + RS_OUT - 1 : out_len - 1;
  const int64_t l_lo = o0 / fo, l_hi = o_last / fo;
  const int64_t i0 = l_lo * fi - width;                       // first input index of the span (may be < 0)
  const int span = (int)((l_hi - l_lo) * fi + J);
  const float* xr = x + row * length;
  for (int i = tid; i < span; i += 256) {
    const int64_t g = i0 + i;
    xs[i] = (g >= 0 && g < length) ? xr[g] : 0.0f;              // the zero padding of F.pad
  }
  for (int i = tid; i < fo * J; i += 256) ks[i] = kern[i];
  __syncthreads();
  const int64_t o = o0 + tid;
  if (o >= out_len) return;
  const int64_t l = o / fo;
  const int k = (int)(o - l * fo);
  const float* xp = xs + (l - l_lo) * fi;
  const float* kp = ks + k * J;
  float acc = 0.0f;
  for (int j = 0; j < J; ++j) acc = fmaf(kp[j], xp[j], acc);
  out[row * out_len + o] = acc;
}

}  // namespace

extern "C" int adp_resample(const float* x, const float* kern, int64_t rows, int64_t length, int64_t fi, int64_t fo,
                            int64_t J, int64_t width, int64_t out_len, float* out, void* stream) {
  if (!x || !kern || !out) return ADP_ERR_NULL;
  if (rows <= 0 || length <= 0 || fi < 1 || fo < 1 || J < 1 || width < 0 || out_len <= 0) return ADP_ERR_SHAPE;
  if (rows > 65535 || length >= (int64_t)1 << 40) return ADP_ERR_SHAPE;
  // every output must be one the reference's conv produces: l <= (length + 2*width + fi - J) / fi
  if ((out_len - 1) / fo > (length + 2 * width + fi - J) / fi) return ADP_ERR_SHAPE;
  if (fo * J > RS_KCAP || ((RS_OUT - 1) / fo + 1) * fi + J > RS_XCAP) return ADP_ERR_UNSUPPORTED;
  dim3 grid((unsigned)adp_cdiv(out_len, RS_OUT), (unsigned)rows);
  ADP_LAUNCH(resample_kernel, grid, dim3(256), stream, x, kern, length, (int)fi, (int)fo, (int)J, (int)width, out_len, out);
  return ADP_LAUNCH_OK();
}

// ------------------------------------------------------------------------------------------------------------------
// Multi-resolution STFT loss (losses.py; auraloss's MultiResolutionSTFTLoss with its defaults).  Per resolution
// (N = fft size, h = hop, W = window length) and signal row:
//
//   X[t, k] = sum_n wt[n] * xpad[t*h + n] * e^{-2 pi i k n / N},   k <= N/2,  t < 1 + L/h
//   wt      = periodic Hann of length W, zero-padded and centred in N;  xpad = x reflect-padded by N/2 on each side
//   m       = sqrt(max(|X|^2, eps));   SC = ||m_y - m_x||_F / ||m_y||_F;   LM = mean|log m_x - log m_y|;
//   LIN     = mean|m_x - m_y|;         loss = mean over resolutions of (w_sc SC + w_log LM + w_lin LIN)
//
// Transform: two consecutive real frames a, b of ONE signal are packed as z = a + i b into one N-point complex FFT and
// separated afterwards (A[k] = (Z[k] + conj Z[N-k]) / 2, B[k] = -i (Z[k] - conj Z[N-k]) / 2): the same work as two
// N/2-point complex FFTs plus their split steps.  x and y go through identical arithmetic, so x == y gives m_x == m_y
// bit for bit (a zero loss and a zero gradient).  The FFT is a Stockham radix-4 (one radix-2 pass first when log2 N
// is odd) over LDS: every thread takes its butterflies' operands into registers, barrier, writes them back, barrier.
// Twiddles (N/4 entries, W^2 and W^3 by complex products) and the window are computed into LDS by each workgroup: no
// host->device copy, so the first call may sit inside a stream capture.
//
// Forward: one launch per resolution.  A workgroup owns up to `fpb` consecutive frames of one row, stages their input
// span of both signals in LDS (reflect padding = index arithmetic), runs 2 PAIRS frames per FFT pass and leaves four partial
// sums (sum (m_y - m_x)^2, sum m_y^2, sum |log m_x - log m_y|, sum |m_x - m_y|) in the workspace; magnitudes never leave
// the chip.  One single-wave launch reduces every resolution's partials in double in a fixed order, writes the loss and
// keeps ||m_y - m_x|| and ||m_y|| per resolution for the backward pass.
//
// Backward (exact adjoint, input gradient only): one launch per resolution.  A workgroup owns PB consecutive samples of
// the PADDED row and computes every frame that touches them: FFTs of the packed frame pairs of x and y, G = dL/dm * X / m
// from the saved norms, the onesided inverse of a frame pair as one complex FFT of the conjugated S_a + i S_b (S: the
// Hermitian extension of G, S[0] = Re G[0], S[N/2] = Re G[N/2], S[k] = G[k]/2, S[N-k] = conj G[k]/2; 1.5 transforms per
// frame in all), window, and an overlap-add by gather into registers (frames in
// increasing order; boundary frames are recomputed by both neighbours, no atomics).  A last launch folds the reflect-pad
// edges back onto the mirrored samples and sums the resolutions, in a fixed order.  Everything is deterministic.
namespace {

constexpr int ST_MAXR = 4;          // resolutions per call

struct StftPlan {
  int nres;
  int n[ST_MAXR], logn[ST_MAXR], hop[ST_MAXR], win[ST_MAXR];
  int frames[ST_MAXR];       // 1 + L / h
  int fpb[ST_MAXR];          // frames per forward workgroup
  int chunks[ST_MAXR];       // forward workgroups per row
  int64_t part_off[ST_MAXR]; // float offset of the resolution's forward partials in the forward workspace
  int64_t gp_off[ST_MAXR];   // float offset of the resolution's padded-row gradient in the backward workspace
  int64_t rows, length;
  float w_sc, w_log, w_lin, eps;
};

constexpr int ST_NORMS = 2 * ST_MAXR;  // forward workspace head: ||m_y - m_x||, ||m_y|| per resolution

template <int LOGN>
__global__ __launch_bounds__(256) void stft_fwd_kernel(const float* x, const float* y, StftPlan p, int r, float* ws) {
  using C = StftCfg<LOGN>;
  constexpr int N = C::N, NP = C::PAIRS, NK = N / 2 + 1;
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
  const float* xr = x + row * L;
  const float* yr = y + row * L;
  for (int i = tid; i < span; i += 256) {
    const int64_t src = st_reflect(s0 + i, L);
    xs[i] = xr[src];
    ys[i] = yr[src];
  }
  __syncthreads();
  float s_d = 0.0f, s_y = 0.0f, s_log = 0.0f, s_lin = 0.0f;
  for (int fb = 0; fb < nf; fb += 2 * NP) {
    for (int i = tid; i < 2 * NP * N; i += 256) {
      const int s = i >> LOGN, n = i & (N - 1);
      const int ta = fb + 2 * (s % NP);  // frames ta, ta + 1 of x (s < NP) or of y
      const float* src = s < NP ? xs : ys;
      bre[i] = ta < nf ? win[n] * src[ta * hop + n] : 0.0f;
      bim[i] = ta + 1 < nf ? win[n] * src[(ta + 1) * hop + n] : 0.0f;
    }
    __syncthreads();
    st_fft<LOGN, 2 * NP>(bre, bim, twr, twi);
    for (int i = tid; i < NP * NK; i += 256) {
      const int s = i / NK, k = i - s * NK;
      const int ta = fb + 2 * s;
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

// one wave: every resolution's partials in double, lane-strided then in lane order (fixed order), -> loss and norms
__global__ __launch_bounds__(64) void stft_final_kernel(float* ws, StftPlan p, float* loss) {
  __shared__ double part[64];
  const int tid = threadIdx.x;
  double total = 0.0;
  for (int r = 0; r < p.nres; ++r) {
    const int64_t nb = p.rows * p.chunks[r];
    const float* src = ws + p.part_off[r];
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
    const double count = (double)p.rows * (double)p.frames[r] * (double)(p.n[r] / 2 + 1);
    const double nd = sqrt(q[0]), ny = sqrt(q[1]);
    total += (double)p.w_sc * (nd / ny) + (double)p.w_log * (q[2] / count) + (double)p.w_lin * (q[3] / count);
    if (tid == 0) {
      ws[2 * r] = (float)nd;
      ws[2 * r + 1] = (float)ny;
    }
  }
  if (tid == 0) loss[0] = (float)(total / (double)p.nres);
}

template <int LOGN>
__global__ __launch_bounds__(256) void stft_bwd_kernel(const float* x, const float* y, const float* gloss,
                                                       const float* norms, StftPlan p, int r, float* ws) {
  using C = StftCfg<LOGN>;
  constexpr int N = C::N, NP = C::PAIRS, NK = N / 2 + 1, PB = C::PB, NACC = PB / 256;
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
  // dL/dm = c_sc (m_x - m_y) + c_log sign(log m_x - log m_y) / m_x + c_lin sign(m_x - m_y)
  const float scale = (gloss ? gloss[0] : 1.0f) / (float)p.nres;
  const float nd = norms[2 * r], ny = norms[2 * r + 1];
  const float count = (float)((double)p.rows * (double)F * (double)NK);
  const float c_sc = nd > 0.0f ? scale * p.w_sc / (nd * ny) : 0.0f;
  const float c_log = scale * p.w_log / count, c_lin = scale * p.w_lin / count;
  // frames t with t*h <= q0 + PB - 1 and t*h + N - 1 >= q0
  const int64_t lo = q0 - N + 1;
  const int t_lo = lo <= 0 ? 0 : (int)((lo + hop - 1) / hop);
  const int t_hi = (int)((q0 + PB - 1) / hop < F - 1 ? (q0 + PB - 1) / hop : F - 1);
  const float* xr = x + row * L;
  const float* yr = y + row * L;
  float acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j) acc[j] = 0.0f;
  __syncthreads();
  for (int t = t_lo; t <= t_hi; t += 2 * NP) {
    for (int i = tid; i < 2 * NP * N; i += 256) {
      const int s = i >> LOGN, n = i & (N - 1);
      const int ta = t + 2 * (s % NP);  // frames ta, ta + 1 of x (s < NP) or of y
      const float* src = s < NP ? xr : yr;
      bre[i] = ta <= t_hi ? win[n] * src[st_reflect((int64_t)ta * hop + n - N / 2, L)] : 0.0f;
      bim[i] = ta + 1 <= t_hi ? win[n] * src[st_reflect((int64_t)(ta + 1) * hop + n - N / 2, L)] : 0.0f;
    }
    __syncthreads();
    st_fft<LOGN, 2 * NP>(bre, bim, twr, twi);
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
    __syncthreads();
    // FFT(conj P) = conj(IFFT_unnormalised(P)): real part = gradient of frame ta, minus the imaginary part = of ta + 1
    st_fft<LOGN, NP>(bre, bim, twr, twi);
#pragma unroll
    for (int j = 0; j < NACC; ++j) {
      const int64_t q = q0 + tid + j * 256;
      for (int s = 0; s < NP; ++s) {
        const int ta = t + 2 * s;
        const int64_t na = q - (int64_t)ta * hop, nb = na - hop;
        if (ta <= t_hi && na >= 0 && na < N) acc[j] = fmaf(win[na], bre[s * N + na], acc[j]);
        if (ta + 1 <= t_hi && nb >= 0 && nb < N) acc[j] = fmaf(win[nb], -bim[s * N + nb], acc[j]);
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

// dx[row, i] = sum over resolutions of the padded-row gradient at i + N/2 and at its reflect-pad mirrors
__global__ __launch_bounds__(256) void stft_fold_kernel(const float* ws, StftPlan p, float* dx) {
  const int64_t L = p.length;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = blockIdx.y;
  if (i >= L) return;
  float g = 0.0f;
  for (int r = 0; r < p.nres; ++r) {
    const int64_t c = p.n[r] / 2;
    const float* gp = ws + p.gp_off[r] + row * (L + p.n[r]);
    g += gp[i + c];
    if (i >= 1 && i <= c) g += gp[c - i];
    if (i >= L - 1 - c && i <= L - 2) g += gp[2 * (L - 1) - i + c];
  }
  dx[row * L + i] = g;
}

// validates the resolutions (N, h, W triples) and fills the plan; workspace sizes in floats
int stft_plan(int64_t rows, int64_t length, int64_t nres, const int64_t* res, float w_sc, float w_log, float w_lin,
              float eps, StftPlan* p, int64_t* fwd_floats, int64_t* bwd_floats) {
  if (!res) return ADP_ERR_NULL;
  if (nres < 1 || nres > ST_MAXR || rows < 1 || rows > 65535 || length < 2 || length >= ((int64_t)1 << 30))
    return ADP_ERR_SHAPE;
  p->nres = (int)nres;
  p->rows = rows;
  p->length = length;
  p->w_sc = w_sc;
  p->w_log = w_log;
  p->w_lin = w_lin;
  p->eps = eps;
  int64_t fo = ST_NORMS, bo = 0;
  for (int r = 0; r < nres; ++r) {
    const int64_t N = res[3 * r], h = res[3 * r + 1], W = res[3 * r + 2];
    int logn = 0;
    while (logn < 13 && ((int64_t)1 << logn) < N) ++logn;
    if (((int64_t)1 << logn) != N || logn < 6 || logn > 12) return ADP_ERR_UNSUPPORTED;
    if (h < 1 || W < 1 || W > N) return ADP_ERR_UNSUPPORTED;
    if (length <= N / 2) return ADP_ERR_SHAPE;  // reflect padding needs N/2 < L
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
    p->part_off[r] = fo;
    fo += rows * p->chunks[r] * 4;
    p->gp_off[r] = bo;
    bo += rows * (length + N);
  }
  if (fwd_floats) *fwd_floats = fo;
  if (bwd_floats) *bwd_floats = bo;
  return ADP_OK;
}

#define ADP_STFT_DISPATCH(LAUNCH)    \
  switch (p.logn[r]) {               \
    case 6: LAUNCH(6); break;        \
    case 7: LAUNCH(7); break;        \
    case 8: LAUNCH(8); break;        \
    case 9: LAUNCH(9); break;        \
    case 10: LAUNCH(10); break;      \
    case 11: LAUNCH(11); break;      \
    default: LAUNCH(12); break;      \
  }

}  // namespace

extern "C" int64_t adp_stft_loss_ws_bytes(int64_t rows, int64_t length, int64_t nres, const int64_t* res,
                                          int64_t backward) {
  StftPlan p;
  int64_t f = 0, b = 0;
  const int rc = stft_plan(rows, length, nres, res, 1.0f, 1.0f, 0.0f, 1e-8f, &p, &f, &b);
  if (rc != ADP_OK) return rc;
  return (backward ? b : f) * (int64_t)sizeof(float);
}

extern "C" int adp_stft_loss_fwd(const float* x, const float* y, int64_t rows, int64_t length, int64_t nres,
                                 const int64_t* res, float w_sc, float w_log, float w_lin, float eps, float* loss,
                                 float* ws, void* stream) {
  if (!x || !y || !loss || !ws) return ADP_ERR_NULL;
  StftPlan p;
  const int rc = stft_plan(rows, length, nres, res, w_sc, w_log, w_lin, eps, &p, nullptr, nullptr);
  if (rc != ADP_OK) return rc;
  for (int r = 0; r < p.nres; ++r) {
    const dim3 grid((unsigned)p.chunks[r], (unsigned)rows);
#define ADP_STFT_FWD(LG) ADP_LAUNCH(stft_fwd_kernel<LG>, grid, dim3(256), stream, x, y, p, r, ws)
    ADP_STFT_DISPATCH(ADP_STFT_FWD)
#undef ADP_STFT_FWD
  }
  ADP_LAUNCH(stft_final_kernel, dim3(1), dim3(64), stream, ws, p, loss);
  return ADP_LAUNCH_OK();
}

extern "C" int adp_stft_loss_bwd(const float* x, const float* y, const float* gloss, const float* ws_fwd, int64_t rows,
                                 int64_t length, int64_t nres, const int64_t* res, float w_sc, float w_log, float w_lin,
                                 float eps, float* dx, float* ws, void* stream) {
  if (!x || !y || !ws_fwd || !dx || !ws) return ADP_ERR_NULL;
  StftPlan p;
  const int rc = stft_plan(rows, length, nres, res, w_sc, w_log, w_lin, eps, &p, nullptr, nullptr);
  if (rc != ADP_OK) return rc;
  for (int r = 0; r < p.nres; ++r) {
    const int64_t pb = p.n[r] >= 1024 ? 2 * (int64_t)p.n[r] : 2048;  // StftCfg<LOGN>::PB
    const dim3 grid((unsigned)adp_cdiv(length + p.n[r], pb), (unsigned)rows);
#define ADP_STFT_BWD(LG) ADP_LAUNCH(stft_bwd_kernel<LG>, grid, dim3(256), stream, x, y, gloss, ws_fwd, p, r, ws)
    ADP_STFT_DISPATCH(ADP_STFT_BWD)
#undef ADP_STFT_BWD
  }
  ADP_LAUNCH(stft_fold_kernel, dim3((unsigned)adp_cdiv(length, 256), (unsigned)rows), dim3(256), stream, ws, p, dx);
  return ADP_LAUNCH_OK();
}

// ------------------------------------------------------------------------------------------------------------------
// Mel spectrogram (vocoder.MelSpectrogram; the reference's components.MelSpectrogram with torchaudio's documented
// defaults).  Per row of T samples:
//
//   xpad  = x reflect-padded by pad = (N - hop) / 2 on each side
//   X[t]  = FFT_N(wt * xpad[t*hop .. t*hop + N)),  wt = periodic Hann of length W centred in N,  t < 1 + (T + 2 pad - N) / hop
//   mel[m, t] = sum_k fb[k, m] |X[t, k]|,  k <= N/2 in increasing order            (fb: [N/2 + 1, n_mels], built by the host)
//   normalize:      mel = 2 (mel / max over the whole tensor)^(1/4) - 1            (a zero maximum gives -1 everywhere)
//   normalize_log:  mel = log(max(mel, 1e-5))                                       (after normalize)
//
// One launch: a workgroup owns up to `fpb` consecutive frames of one row, stages their span in LDS, runs 4 PAIRS frames per
// FFT pass (the STFT loss's packed-pair transform, st_fft / st_split above), leaves the magnitudes in LDS and forms the
// filterbank product from there: one thread per (mel, frame), walking `range[m] = [lo, hi)` (the bins where the column of
// fb is not zero: a triangle) or every bin when no ranges are given; skipped terms are exact zeros, so the sum is the dense
// product.  With `normalize` every workgroup also leaves its maximum in the workspace and a second launch takes the maximum
// of those and applies the pointwise map: no atomics, no host value, bit-identical from call to call.
namespace {

constexpr int MEL_NORMALIZE = 1, MEL_LOG = 2;
constexpr float MEL_LOG_FLOOR = 1e-5f;
constexpr float MEL_LOG_OF_FLOOR = -11.512925464970229f;  // log(1e-5) rounded once: what every clamped value returns

struct MelPlan {
  int n, logn, hop, win, pad, n_mels, frames, fpb, chunks;
  int64_t rows, length;
};

template <int LOGN>
__global__ __launch_bounds__(256) void mel_kernel(const float* x, const float* fb, const int32_t* range, MelPlan p, int mode,
                                                  float* out, float* part) {
  using C = StftCfg<LOGN>;
  constexpr int N = C::N, NP = 2 * C::PAIRS, NF = 2 * NP, NK = N / 2 + 1;  // NP packed pairs = NF frames per pass
  __shared__ float xs[C::XCAP];
  __shared__ float bre[NP * N];
  __shared__ float bim[NP * N];
  __shared__ float twr[N / 4];
  __shared__ float twi[N / 4];
  __shared__ float win[N];
  __shared__ float mag[NF * NK];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int hop = p.hop, fpb = p.fpb, n_mels = p.n_mels, F = p.frames;
  const int64_t row = blockIdx.y, L = p.length;
  const int f0 = blockIdx.x * fpb;
  const int nf = (F - f0 < fpb) ? F - f0 : fpb;
  st_tables<LOGN>(twr, twi, win, p.win);
  const int64_t s0 = (int64_t)f0 * hop - p.pad;  // original-signal index of the span's first (padded) sample
  const int span = (nf - 1) * hop + N;
  const float* xr = x + row * L;
  for (int i = tid; i < span; i += 256) xs[i] = xr[st_reflect(s0 + i, L)];
  __syncthreads();
  float vmax = 0.0f;
  for (int fbase = 0; fbase < nf; fbase += NF) {
    for (int i = tid; i < NP * N; i += 256) {
      const int s = i >> LOGN, n = i & (N - 1);
      const int ta = fbase + 2 * s;
      bre[i] = ta < nf ? win[n] * xs[ta * hop + n] : 0.0f;
      bim[i] = ta + 1 < nf ? win[n] * xs[(ta + 1) * hop + n] : 0.0f;
    }
    __syncthreads();
    st_fft<LOGN, NP>(bre, bim, twr, twi);
    for (int i = tid; i < NP * NK; i += 256) {
      const int s = i / NK, k = i - s * NK;
      float ar, ai, br, bi;
      st_split<LOGN>(bre + s * N, bim + s * N, k, ar, ai, br, bi);
      mag[(2 * s) * NK + k] = sqrtf(ar * ar + ai * ai);
      mag[(2 * s + 1) * NK + k] = sqrtf(br * br + bi * bi);
    }
    __syncthreads();
    const int cnt = (nf - fbase < NF) ? nf - fbase : NF;
    for (int i = tid; i < n_mels * NF; i += 256) {
      const int m = i / NF, e = i - m * NF;
      if (e >= cnt) continue;
      const int lo = range ? range[2 * m] : 0, hi = range ? range[2 * m + 1] : NK;
      const float* mg = mag + e * NK;
      float acc = 0.0f;
      for (int k = lo; k < hi; ++k) acc = fmaf(fb[(int64_t)k * n_mels + m], mg[k], acc);
      vmax = fmaxf(vmax, acc);
      if (mode == MEL_LOG) acc = acc > MEL_LOG_FLOOR ? logf(acc) : MEL_LOG_OF_FLOOR;
      out[(row * n_mels + m) * F + f0 + fbase + e] = acc;
    }
    __syncthreads();
  }
  if (mode & MEL_NORMALIZE) {
    vmax = adp_wave_max(vmax);
    if ((tid & 63) == 0) red[tid >> 6] = vmax;
    __syncthreads();
    if (tid == 0) part[row * p.chunks + blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  }
}

// mel = 2 (mel / max)^(1/4) - 1, then the log; every workgroup takes the maximum of all forward workgroups' maxima itself
__global__ __launch_bounds__(256) void mel_norm_kernel(float* out, int64_t n, const float* part, int nparts, int mode) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  float vmax = 0.0f;
  for (int i = tid; i < nparts; i += 256) vmax = fmaxf(vmax, part[i]);
  vmax = adp_wave_max(vmax);
  if ((tid & 63) == 0) red[tid >> 6] = vmax;
  __syncthreads();
  vmax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) {
    // in double: 2 r^(1/4) - 1 cancels near r = 1/16 and the log behind it magnifies every rounding made on the way
    const double r = vmax > 0.0f ? (double)out[i] / (double)vmax : 0.0;
    double v = 2.0 * sqrt(sqrt(r)) - 1.0;
    float o = (float)v;
    if (mode & MEL_LOG) o = v > (double)MEL_LOG_FLOOR ? (float)log(v) : MEL_LOG_OF_FLOOR;
    out[i] = o;
  }
}

int mel_plan(int64_t rows, int64_t length, int64_t n_fft, int64_t hop, int64_t win, int64_t n_mels, MelPlan* p) {
  if (rows < 1 || rows > 65535 || length < 1 || length >= ((int64_t)1 << 30) || n_mels < 1 || n_mels > 65535)
    return ADP_ERR_SHAPE;
  int logn = 0;
  while (logn < 13 && ((int64_t)1 << logn) < n_fft) ++logn;
  if (((int64_t)1 << logn) != n_fft || logn < 6 || logn > 12) return ADP_ERR_UNSUPPORTED;
  if (hop < 1 || hop > n_fft || win < 1 || win > n_fft) return ADP_ERR_UNSUPPORTED;
  const int64_t pad = (n_fft - hop) / 2;
  if (length <= pad || length + 2 * pad < n_fft) return ADP_ERR_SHAPE;  // reflect padding; at least one frame
  const int64_t F = 1 + (length + 2 * pad - n_fft) / hop;
  const int64_t per_pass = n_fft >= 512 ? 4 : 2048 / n_fft;  // 4 * StftCfg<LOGN>::PAIRS
  int64_t fpb = 1 + ST_SPAN_EXTRA / hop;
  if (fpb > 8 * per_pass) fpb = 8 * per_pass;
  if (adp_cdiv(F, fpb) > 0x7fffffff / 4 || F >= ((int64_t)1 << 30)) return ADP_ERR_SHAPE;
  p->n = (int)n_fft;
  p->logn = logn;
  p->hop = (int)hop;
  p->win = (int)win;
  p->pad = (int)pad;
  p->n_mels = (int)n_mels;
  p->frames = (int)F;
  p->fpb = (int)fpb;
  p->chunks = (int)adp_cdiv(F, fpb);
  p->rows = rows;
  p->length = length;
  return ADP_OK;
}

}  // namespace

extern "C" int64_t adp_mel_frames(int64_t length, int64_t n_fft, int64_t hop) {
  if (n_fft < 1 || hop < 1 || hop > n_fft || length < 1) return ADP_ERR_SHAPE;
  const int64_t pad = (n_fft - hop) / 2;
  if (length + 2 * pad < n_fft) return ADP_ERR_SHAPE;
  return 1 + (length + 2 * pad - n_fft) / hop;
}

extern "C" int64_t adp_mel_spectrogram_ws_bytes(int64_t rows, int64_t length, int64_t n_fft, int64_t hop, int64_t win,
                                                int64_t n_mels) {
  MelPlan p;
  const int rc = mel_plan(rows, length, n_fft, hop, win, n_mels, &p);
  if (rc != ADP_OK) return rc;
  return rows * p.chunks * (int64_t)sizeof(float);
}

extern "C" int adp_mel_spectrogram(const float* x, const float* fb, const int32_t* range, int64_t rows, int64_t length,
                                   int64_t n_fft, int64_t hop, int64_t win, int64_t n_mels, int64_t normalize,
                                   int64_t normalize_log, float* out, float* ws, void* stream) {
  if (!x || !fb || !out || (normalize && !ws)) return ADP_ERR_NULL;
  MelPlan p;
  const int rc = mel_plan(rows, length, n_fft, hop, win, n_mels, &p);
  if (rc != ADP_OK) return rc;
  const int mode = (normalize ? MEL_NORMALIZE : 0) | (normalize_log ? MEL_LOG : 0);
  const dim3 grid((unsigned)p.chunks, (unsigned)rows);
#define ADP_MEL(LG) ADP_LAUNCH(mel_kernel<LG>, grid, dim3(256), stream, x, fb, range, p, mode, out, ws)
  switch (p.logn) {
    case 6: ADP_MEL(6); break;
    case 7: ADP_MEL(7); break;
    case 8: ADP_MEL(8); break;
    case 9: ADP_MEL(9); break;
    case 10: ADP_MEL(10); break;
    case 11: ADP_MEL(11); break;
    default: ADP_MEL(12); break;
  }
#undef ADP_MEL
  if (normalize) {
    const int64_t n = rows * n_mels * p.frames;
    const int64_t blocks = adp_cdiv(n, 256) < 1024 ? adp_cdiv(n, 256) : 1024;
    ADP_LAUNCH(mel_norm_kernel, dim3((unsigned)blocks), dim3(256), stream, out, n, (const float*)ws,
               (int)(rows * p.chunks), mode);
  }
  return ADP_LAUNCH_OK();
}

// ------------------------------------------------------------------------------------------------------------------
// to_flat of the vocoder: ConvTranspose1d(M, 1, kernel K, stride hop, padding pad, no bias) and its weight gradient.
//
//   flat[n, t] = sum_m sum_j spec[n, m, q - j] * w[m, r + j hop],   t + pad = q hop + r (0 <= r < hop),  j < ceil(K / hop)
//   dW[m, k]   = sum_n sum_l spec[n, m, l] * g[n, l hop + k - pad]
//
// Forward: a workgroup owns TF_TT consecutive outputs of one row; the weight rows and the spectrogram columns they touch
// go through LDS in chunks of `mc` mel channels (weights are read once per workgroup, coalesced).  When hop, pad and K are
// multiples of 4, four consecutive outputs share q and read their four weights as one 16-byte LDS access and are stored as
// one 16-byte access; any other geometry runs the per-output path.
// Weight gradient: thread = 4 consecutive taps k of TW_MR mel channels (32 register accumulators), the (n, l) sum is split
// into `segs` segments over the grid, every segment WRITES its partial to the workspace and a second launch adds the
// segments in increasing order: deterministic, nothing accumulated into the caller's buffer.
namespace {

constexpr int TF_TT = 2048;     // outputs per forward workgroup (8 per thread)
constexpr int TF_CAP = 12288;   // LDS floats of a forward workgroup (weights + spectrogram columns of one chunk)
constexpr int TW_MR = 8;        // mel channels per weight-gradient thread

struct TflatPlan {
  int64_t N, M, L, K, hop, pad, Lout;
  int J, NL, mc, vec;
  int sl, lc, segs;             // weight gradient: l-chunks per batch row, their length, segments = N * sl
  int64_t slots;                // weight gradient: threads needed = ceil(K / 4) * ceil(M / TW_MR)
};

template <bool VEC>
__global__ __launch_bounds__(256) void tflat_fwd_kernel(const float* spec, const float* w, TflatPlan p, float* out) {
  __shared__ float lds[TF_CAP];
  const int tid = threadIdx.x;
  const int K = (int)p.K, hop = (int)p.hop, pad = (int)p.pad, J = p.J, NL = p.NL, M = (int)p.M;
  const int64_t L = p.L, Lout = p.Lout, n = blockIdx.y;
  const int64_t t0 = (int64_t)blockIdx.x * TF_TT;
  const int64_t lb = (t0 + pad) / hop - (J - 1);  // spectrogram column held at index 0 of a staged row
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.0f;
  for (int m0 = 0; m0 < M; m0 += p.mc) {
    const int mcn = (M - m0 < p.mc) ? M - m0 : p.mc;
    float* wl = lds;
    float* sl = lds + mcn * K;
    __syncthreads();
    if (VEC) {
      for (int i = tid * 4; i < mcn * K; i += 1024) *(f32x4*)(wl + i) = *(const f32x4*)(w + (int64_t)m0 * K + i);
    } else {
      for (int i = tid; i < mcn * K; i += 256) wl[i] = w[(int64_t)m0 * K + i];
    }
    for (int i = tid; i < mcn * NL; i += 256) {
      const int mi = i / NL, li = i - mi * NL;
      const int64_t l = lb + li;
      sl[i] = (l >= 0 && l < L) ? spec[(n * M + m0 + mi) * L + l] : 0.0f;
    }
    __syncthreads();
    float part[8];  // this chunk's share, added to the total once: a blocked sum (shorter rounding chains)
#pragma unroll
    for (int i = 0; i < 8; ++i) part[i] = 0.0f;
    if (VEC) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int64_t u = t0 + (g * 256 + tid) * 4 + pad;
        const int64_t q = u / hop;
        const int r = (int)(u - q * hop), qi = (int)(q - lb);
        for (int mi = 0; mi < mcn; ++mi) {
          for (int j = 0; j < J; ++j) {
            const int k = r + j * hop;
            if (k >= K) break;
            const f32x4 wv = *(const f32x4*)(wl + mi * K + k);
            const float s = sl[mi * NL + qi - j];
#pragma unroll
            for (int c = 0; c < 4; ++c) part[g * 4 + c] = fmaf(s, wv[c], part[g * 4 + c]);
          }
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t u = t0 + i * 256 + tid + pad;
        const int64_t q = u / hop;
        const int r = (int)(u - q * hop), qi = (int)(q - lb);
        for (int mi = 0; mi < mcn; ++mi) {
          for (int j = 0; j < J; ++j) {
            const int k = r + j * hop;
            if (k >= K) break;
            part[i] = fmaf(sl[mi * NL + qi - j], wl[mi * K + k], part[i]);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += part[i];
  }
  float* o = out + n * Lout;
  if (VEC) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int64_t t = t0 + (g * 256 + tid) * 4;
      if (t < Lout) *(f32x4*)(o + t) = f32x4{acc[g * 4], acc[g * 4 + 1], acc[g * 4 + 2], acc[g * 4 + 3]};  // Lout % 4 == 0
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int64_t t = t0 + i * 256 + tid;
      if (t < Lout) o[t] = acc[i];
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void tflat_wgrad_kernel(const float* spec, const float* g, TflatPlan p, float* part) {
  const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot >= p.slots) return;
  const int K = (int)p.K, M = (int)p.M;
  const int K4 = (K + 3) / 4;
  const int mg = (int)(slot / K4), k0 = (int)(slot - (int64_t)mg * K4) * 4;
  const int m0 = mg * TW_MR;
  const int seg = blockIdx.y;
  const int64_t n = seg / p.sl;
  const int64_t l_lo = (int64_t)(seg % p.sl) * p.lc;
  const int64_t l_hi = (l_lo + p.lc < p.L) ? l_lo + p.lc : p.L;
  const float* gr = g + n * p.Lout;
  const float* sr = spec + (n * M + m0) * p.L;
  float acc[TW_MR][4];
#pragma unroll
  for (int i = 0; i < TW_MR; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[i][c] = 0.0f;
  for (int64_t l = l_lo; l < l_hi; ++l) {
    const int64_t t = l * p.hop + k0 - p.pad;
    float gv[4];
    if (VEC) {  // t % 4 == 0 and Lout % 4 == 0: the four taps are inside or outside together
      const f32x4 v = (t >= 0 && t < p.Lout) ? *(const f32x4*)(gr + t) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int c = 0; c < 4; ++c) gv[c] = v[c];
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) gv[c] = (k0 + c < K && t + c >= 0 && t + c < p.Lout) ? gr[t + c] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < TW_MR; ++i) {
      const float s = (m0 + i < M) ? sr[(int64_t)i * p.L + l] : 0.0f;
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[i][c] = fmaf(s, gv[c], acc[i][c]);
    }
  }
  float* dst = part + (int64_t)seg * M * K;
#pragma unroll
  for (int i = 0; i < TW_MR; ++i) {
    if (m0 + i >= M) break;
    float* d = dst + (int64_t)(m0 + i) * K + k0;
    if (VEC) {
      *(f32x4*)d = f32x4{acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
    } else {
      for (int c = 0; c < 4 && k0 + c < K; ++c) d[c] = acc[i][c];
    }
  }
}

// dW[i] = part[0][i] + part[1][i] + ... in increasing segment order
__global__ __launch_bounds__(256) void tflat_wgrad_sum_kernel(const float* part, int64_t mk, int segs, float* dw) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= mk) return;
  float s = part[i];
  for (int r = 1; r < segs; ++r) s += part[(int64_t)r * mk + i];
  dw[i] = s;
}

// the 16-byte paths need 16-byte aligned bases (rows are multiples of 4 floats there)
bool tflat_aligned(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

int tflat_plan(int64_t N, int64_t M, int64_t L, int64_t K, int64_t hop, TflatPlan* p) {
  if (N < 1 || N > 65535 || M < 1 || M > 65535 || L < 1 || L >= ((int64_t)1 << 30)) return ADP_ERR_SHAPE;
  if (hop < 1 || K < hop || K > 65536) return ADP_ERR_UNSUPPORTED;
  const int64_t pad = (K - hop) / 2;
  const int64_t Lout = (L - 1) * hop - 2 * pad + K;
  if (Lout < 1 || Lout >= ((int64_t)1 << 40)) return ADP_ERR_SHAPE;
  const int64_t J = adp_cdiv(K, hop);
  const int64_t NL = (TF_TT - 1) / hop + J + 1;
  if (K + NL > TF_CAP) return ADP_ERR_UNSUPPORTED;
  int64_t mc = TF_CAP / (K + NL);
  if (mc > M) mc = M;
  p->N = N; p->M = M; p->L = L; p->K = K; p->hop = hop; p->pad = pad; p->Lout = Lout;
  p->J = (int)J;
  p->NL = (int)NL;
  p->mc = (int)mc;
  p->vec = (hop % 4 == 0 && pad % 4 == 0 && K % 4 == 0) ? 1 : 0;
  p->slots = adp_cdiv(K, 4) * adp_cdiv(M, TW_MR);
  // about 256 workgroups over (slots, batch row, l-chunk); chunks of at least 16 spectrogram columns
  const int64_t gx = adp_cdiv(p->slots, 256);
  int64_t sl = adp_cdiv(256, gx * N);
  if (sl > adp_cdiv(L, 16)) sl = adp_cdiv(L, 16);
  if (sl < 1) sl = 1;
  const int64_t lc = adp_cdiv(L, sl);
  sl = adp_cdiv(L, lc);
  if (N * sl > 65535) return ADP_ERR_SHAPE;
  p->sl = (int)sl;
  p->lc = (int)lc;
  p->segs = (int)(N * sl);
  return ADP_OK;
}

}  // namespace

extern "C" int64_t adp_tflat_out_len(int64_t L, int64_t K, int64_t hop) {
  if (L < 1 || hop < 1 || K < hop) return ADP_ERR_SHAPE;
  return (L - 1) * hop - 2 * ((K - hop) / 2) + K;
}

extern "C" int adp_tflat_fwd(const float* spec, const float* w, int64_t N, int64_t M, int64_t L, int64_t K, int64_t hop,
                             float* out, void* stream) {
  if (!spec || !w || !out) return ADP_ERR_NULL;
  TflatPlan p;
  const int rc = tflat_plan(N, M, L, K, hop, &p);
  if (rc != ADP_OK) return rc;
  const dim3 grid((unsigned)adp_cdiv(p.Lout, TF_TT), (unsigned)N);
  if (p.vec && tflat_aligned(w, out)) ADP_LAUNCH(tflat_fwd_kernel<true>, grid, dim3(256), stream, spec, w, p, out);
  else ADP_LAUNCH(tflat_fwd_kernel<false>, grid, dim3(256), stream, spec, w, p, out);
  return ADP_LAUNCH_OK();
}

extern "C" int64_t adp_tflat_wgrad_ws_bytes(int64_t N, int64_t M, int64_t L, int64_t K, int64_t hop) {
  TflatPlan p;
  const int rc = tflat_plan(N, M, L, K, hop, &p);
  if (rc != ADP_OK) return rc;
  return (int64_t)p.segs * M * K * (int64_t)sizeof(float);
}

extern "C" int adp_tflat_wgrad(const float* spec, const float* g, int64_t N, int64_t M, int64_t L, int64_t K, int64_t hop,
                               float* dw, float* ws, void* stream) {
  if (!spec || !g || !dw || !ws) return ADP_ERR_NULL;
  TflatPlan p;
  const int rc = tflat_plan(N, M, L, K, hop, &p);
  if (rc != ADP_OK) return rc;
  const dim3 grid((unsigned)adp_cdiv(p.slots, 256), (unsigned)p.segs);
  if (p.vec && tflat_aligned(g, ws)) ADP_LAUNCH(tflat_wgrad_kernel<true>, grid, dim3(256), stream, spec, g, p, ws);
  else ADP_LAUNCH(tflat_wgrad_kernel<false>, grid, dim3(256), stream, spec, g, p, ws);
  ADP_LAUNCH(tflat_wgrad_sum_kernel, dim3((unsigned)adp_cdiv(M * K, 256)), dim3(256), stream, (const float*)ws, M * K, p.segs,
             dw);
  return ADP_LAUNCH_OK();
}
