// The project's counter-based normal stream: Philox4x32-10 (Salmon et al., "Parallel Random Numbers: As Easy as 1, 2, 3", 2011)
// and Box-Muller in fp32.  Every normal is a pure function of (seed of the sample, draw index, element index):
//   key      (seed & 0xffffffff, seed >> 32)
//   element  g = offset + e,  blk = g >> 2,  lane = g & 3
//   counter  (blk & 0xffffffff, blk >> 32, draw & 0xffffffff, draw >> 32)
//   x0..x3   ten rounds, multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85
//   u1 = ((x >> 8) + 1) 2^-24 in (0, 1],  u2 = (x >> 8) 2^-24 in [0, 1)          (exact in fp32)
//   lanes 0..3 = ra cospi(2 u2a), ra sinpi(2 u2a), rb cospi(2 u2b), rb sinpi(2 u2b),  r = sqrt(-2 log u1)
// Plain C++ that compiles for the device and for the host (tests compile it with the host compiler alone).  The host has no
// sinpif / cospif everywhere, so there the two are taken from the fp64 sin / cos and rounded: the integer part is the same bit
// for bit, the normals agree to fp32 rounding.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define APTP_PHILOX_HD __host__ __device__ inline
#else
#define APTP_PHILOX_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

APTP_PHILOX_HD void aptp_philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// the four words of block blk of draw `draw` of the sample whose seed is `seed`
APTP_PHILOX_HD void aptp_philox_block(uint64_t seed, uint64_t draw, uint64_t blk, uint32_t x[4]) {
  x[0] = (uint32_t)blk; x[1] = (uint32_t)(blk >> 32); x[2] = (uint32_t)draw; x[3] = (uint32_t)(draw >> 32);
  aptp_philox4x32_10(x, (uint32_t)seed, (uint32_t)(seed >> 32));
}

APTP_PHILOX_HD float aptp_philox_u1(uint32_t x) { return (float)((x >> 8) + 1u) * 5.9604644775390625e-8f; }   // 2^-24
APTP_PHILOX_HD float aptp_philox_u2(uint32_t x) { return (float)(x >> 8) * 5.9604644775390625e-8f; }

APTP_PHILOX_HD float aptp_philox_cospi2(float u2) {
#if defined(__HIP_DEVICE_COMPILE__)
  return cospif(2.f * u2);
#else
  return (float)cos(6.283185307179586476925 * (double)u2);
#endif
}

APTP_PHILOX_HD float aptp_philox_sinpi2(float u2) {
#if defined(__HIP_DEVICE_COMPILE__)
  return sinpif(2.f * u2);
#else
  return (float)sin(6.283185307179586476925 * (double)u2);
#endif
}

APTP_PHILOX_HD float aptp_philox_radius(uint32_t x) { return sqrtf(-2.f * logf(aptp_philox_u1(x))); }

// the four normals of a block
APTP_PHILOX_HD void aptp_philox_normals4(const uint32_t x[4], float z[4]) {
  const float ra = aptp_philox_radius(x[0]), rb = aptp_philox_radius(x[2]);
  const float ua = aptp_philox_u2(x[1]), ub = aptp_philox_u2(x[3]);
  z[0] = ra * aptp_philox_cospi2(ua);
  z[1] = ra * aptp_philox_sinpi2(ua);
  z[2] = rb * aptp_philox_cospi2(ub);
  z[3] = rb * aptp_philox_sinpi2(ub);
}

// one normal of a block: the same statements on the pair of words that lane uses
APTP_PHILOX_HD float aptp_philox_normal1(const uint32_t x[4], int lane) {
  const float r = aptp_philox_radius((lane & 2) ? x[2] : x[0]), u = aptp_philox_u2((lane & 2) ? x[3] : x[1]);
  return r * ((lane & 1) ? aptp_philox_sinpi2(u) : aptp_philox_cospi2(u));
}
