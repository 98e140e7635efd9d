// Philox4x32-10 (Salmon et al., SC'11) and the standard-normal draw built on it: one definition for the Rademacher probe, the SDE sampler's
// noise (ode.hip) and the validation objective (fm_valid.hip), so a named draw (seed, counter, element) has the same bits wherever it is inlined.
#pragma once
#include "common.h"

constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(PHILOX_M0, c[0]), lo0 = PHILOX_M0 * c[0], hi1 = __umulhi(PHILOX_M1, c[2]), lo1 = PHILOX_M1 * c[2];
    const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += PHILOX_W0; k1 += PHILOX_W1;
  }
}

// One Philox block = four words = four normals.  Word w gives u = ((w >> 9) + 0.5) 2^-23 = (2 (w >> 9) + 1) 2^-24: an odd 24-bit integer times
// a power of two, exact in f32 and strictly inside (0, 1).  Box-Muller on (u0, u1) and (u2, u3): r = sqrt(-2 ln u_a), the angle 2 pi u_b rounded
// once, z = (r cos, r sin).  Every product is a named rounding (no contraction), so the draw has the same bits wherever it is inlined.
constexpr float SDE_TWO_PI = 6.283185307179586f;

__device__ __forceinline__ float philox_u01(unsigned w) { return (float)(((w >> 9) << 1) | 1u) * 0x1p-24f; }

__device__ __forceinline__ void box_muller(unsigned wa, unsigned wb, float& z0, float& z1) {
  const float r = sqrtf(__fmul_rn(-2.f, logf(philox_u01(wa))));
  float s, c;
  sincosf(__fmul_rn(SDE_TWO_PI, philox_u01(wb)), &s, &c);
  z0 = __fmul_rn(r, c);
  z1 = __fmul_rn(r, s);
}

// the four normals of elements 4 v .. 4 v + 3 of the draw (seed = (k0, k1), counter = (c0, c1))
__device__ __forceinline__ void philox_normal4(long v, unsigned k0, unsigned k1, unsigned c0, unsigned c1, float (&z)[4]) {
  unsigned c[4] = {c0, c1, (unsigned)((unsigned long)v & 0xffffffffu), (unsigned)((unsigned long)v >> 32)};
  philox4x32_10(c, k0, k1);
  box_muller(c[0], c[1], z[0], z[1]);
  box_muller(c[2], c[3], z[2], z[3]);
}
