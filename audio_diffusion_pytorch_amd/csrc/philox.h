// The counter-based normal generator of include/adp_rng.h as device functions: Philox4x32-10 on a (seed, draw) row and
// Box-Muller on its words.  Private to the kernel sources that form a row's stream in registers (rng.hip: adp_randn and
// the VInpainter step; sde.hip, edm.hip: the stochastic sampler steps; repaint.hip: the RePaint resample), so that all of them
// give the same bits for the same row.
#pragma once
#include "adp_rt.h"

namespace philox {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

struct alignas(16) U32x4 {
  uint32_t w[4];
};

struct RngRow {
  uint32_t seed_lo, seed_hi, draw;
};

__device__ __forceinline__ RngRow rng_row(const uint32_t* rng4) { return RngRow{rng4[0], rng4[1], rng4[2]}; }

// Philox4x32-10 on counter (lo32(g), hi32(g), draw, 0) under key (seed_lo, seed_hi): words 4g .. 4g+3 of the row's stream
__device__ __forceinline__ U32x4 rng_words(const RngRow& r, int64_t g) {
  uint32_t c0 = (uint32_t)((uint64_t)g & 0xFFFFFFFFu), c1 = (uint32_t)((uint64_t)g >> 32), c2 = r.draw, c3 = 0u;
  uint32_t k0 = r.seed_lo, k1 = r.seed_hi;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  return U32x4{{c0, c1, c2, c3}};
}

// Box-Muller on one pair of words: u = ((r >> 8) + 0.5) 2^-24 for both; (sqrt(-2 ln u_a) cos(2 pi u_b), ... sin(2 pi u_b)).
// u_a = m 2^-25 with m = 2 (ra >> 8) + 1 a 25-bit odd integer: h is the float nearest to m, d = m - h in {-1, 0, 1} (exact in
// integers), ln u_a = logf(h 2^-25) + d / h up to (d / h)^2 / 2 < 2^-49.  Without the d term the radius would be off by up
// to 1e-4 where u_a is within 2^-16 of 1.
__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& z_cos, float& z_sin) {
  const uint32_t m = 2u * (ra >> 8) + 1u;
  const float h = (float)m;
  const int d = (int)m - (int)(uint32_t)h;
  const float ln_u = logf(h * 0x1p-25f) + (float)d / h;
  const float radius = sqrtf(-2.0f * ln_u);
  const float ub = ((float)(rb >> 8) + 0.5f) * 0x1p-24f;
  float s, c;
  sincosf(6.28318530717958647692f * ub, &s, &c);
  z_cos = radius * c;
  z_sin = radius * s;
}

// the draw: normals 4g .. 4g+3 of the row's stream
__device__ __forceinline__ f32x4 rng_normal4(const RngRow& r, int64_t g) {
  const U32x4 w = rng_words(r, g);
  float z0, z1, z2, z3;
  box_muller(w.w[0], w.w[1], z0, z1);
  box_muller(w.w[2], w.w[3], z2, z3);
  const f32x4 z = {z0, z1, z2, z3};
  return z;
}

__device__ __forceinline__ int64_t rng_groups(int64_t n) { return n / 4 + (n % 4 != 0); }

}  // namespace philox
