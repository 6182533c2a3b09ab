// The arithmetic of a seeded training batch (csrc/train_noise.hip), on the stream of philox_normal.h unchanged.
// A training sample has an int64 seed and the call a draw d in [0, 2^59) (an epoch or a global step); sub-draw k of the call is
// Philox draw 8 d + k of that seed:
//   k = 0  transform (host, data.draw_crop_flip_seeded): words x0, x1, x2 of block 0:
//          top = (x0 (H1 - R + 1)) >> 32, left = (x1 (W1 - R + 1)) >> 32 in uint64, flip = x2 >> 31
//   k = 1  VAE posterior eps      element e = c hw + y w + x of the sample's NCHW [4, h, w]
//   k = 2  noise                  same indexing
//   k = 3  offset noise           element c (one block: the four channels)
//   k = 4  input perturbation     same indexing as k = 1
//   k = 5  timestep               word x0 of block 0: t = (x0 T) >> 32 in uint64, T = max_scheduler_steps
//   k = 6  router assignment      Gumbel noise of the optimal-transport assignment (gumbel_relax.h): element = column
//   k = 7  router relaxation      Gumbel noise of the relaxation itself (gumbel_relax.h): same indexing
// fp32, contraction off, in this order (z_k the normal of sub-draw k, s the scale, (sa, so) row t of the [T, 2] table of
// sqrt(alphas_cumprod), sqrt(1 - alphas_cumprod)):
//   x0     = s fmaf(expf(0.5f clamp(logvar, -30, 20)), z1, mean)   (moments given)   |   x0 = latents_in   (latents given)
//            the one fused multiply-add of the map, written out: aptp_latent_dist's mean + std eps compiles to one, so a seeded
//            x0 equals what that kernel gives for the same eps bit for bit
//   n      = z2 + noise_offset z3[c]                               (n = z2 when noise_offset == 0)
//   m      = n + input_perturbation z4                             (m = n when input_perturbation == 0)
//   noisy  = sa x0 + so m
//   target = n  (epsilon)   |   sa n - so x0  (v_prediction)
// Plain C++ for the device and the host, as philox_normal.h is: the kernel calls nothing else for arithmetic and the host test
// compiles this file with the host compiler alone.
#pragma once
#include "philox_normal.h"

// every product and sum below is rounded on its own
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define APTP_TN_DRAWS 8                // sub-draws reserved per call
#define APTP_TN_TRANSFORM 0
#define APTP_TN_EPS 1
#define APTP_TN_NOISE 2
#define APTP_TN_OFFSET 3
#define APTP_TN_PERTURB 4
#define APTP_TN_TIMESTEP 5

APTP_PHILOX_HD uint64_t aptp_tn_subdraw(uint64_t draw, int k) { return (uint64_t)APTP_TN_DRAWS * draw + (uint64_t)k; }

// an integer in [0, n) from one word: each value for floor(2^32 / n) or ceil(2^32 / n) words
APTP_PHILOX_HD int64_t aptp_tn_choice(uint32_t x, int64_t n) { return (int64_t)(((uint64_t)x * (uint64_t)n) >> 32); }

// what a sample's elements share: the timestep, its table row and the four offset normals (zero when there is no offset)
struct AptpTnSample {
  int64_t t;
  float sa, so;
  float z3[4];
};

APTP_PHILOX_HD void aptp_tn_sample(uint64_t seed, uint64_t draw, int64_t T, const float* sqrt_table, bool with_offset,
                                   AptpTnSample* s) {
  uint32_t x[4];
  aptp_philox_block(seed, aptp_tn_subdraw(draw, APTP_TN_TIMESTEP), 0, x);
  s->t = aptp_tn_choice(x[0], T);
  s->sa = sqrt_table[2 * s->t];
  s->so = sqrt_table[2 * s->t + 1];
  s->z3[0] = s->z3[1] = s->z3[2] = s->z3[3] = 0.f;
  if (with_offset) {
    aptp_philox_block(seed, aptp_tn_subdraw(draw, APTP_TN_OFFSET), 0, x);
    aptp_philox_normals4(x, s->z3);
  }
}

// the host values of a call
struct AptpTnKnobs {
  float scale, noise_offset, input_perturbation;
  int v_prediction;
};

APTP_PHILOX_HD float aptp_tn_x0(float mean, float logvar, float z1, float scale) {
  const float lv = fminf(fmaxf(logvar, -30.f), 20.f);
  const float sd = expf(0.5f * lv);
  return scale * fmaf(sd, z1, mean);
}

// one element: x0 as given or formed by aptp_tn_x0; z3c the offset normal of its channel; z4 is not read without a perturbation
APTP_PHILOX_HD void aptp_tn_element(const AptpTnKnobs& k, const AptpTnSample& s, float x0, float z2, float z3c, float z4,
                                    float* noisy, float* target, float* n_out) {
  const float n = k.noise_offset != 0.f ? z2 + k.noise_offset * z3c : z2;
  const float m = k.input_perturbation != 0.f ? n + k.input_perturbation * z4 : n;
  *noisy = s.sa * x0 + s.so * m;
  *target = k.v_prediction ? s.sa * n - s.so * x0 : n;
  *n_out = n;
}

// four elements of one channel: the same statements
APTP_PHILOX_HD void aptp_tn_element4(const AptpTnKnobs& k, const AptpTnSample& s, const float x0[4], const float z2[4], float z3c,
                                     const float z4[4], float noisy[4], float target[4], float n_out[4]) {
  for (int j = 0; j < 4; ++j) aptp_tn_element(k, s, x0[j], z2[j], z3c, z4[j], &noisy[j], &target[j], &n_out[j]);
}

// element e of a sample's [4, h, w], everything from the seed: the form the element-wise path and the host use.  mean / logvar
// are read only with from_moments, x0_in only without.
APTP_PHILOX_HD void aptp_tn_element_of(const AptpTnKnobs& k, const AptpTnSample& s, uint64_t seed, uint64_t draw, int64_t e,
                                       int64_t hw, bool from_moments, float mean, float logvar, float x0_in, float* x0,
                                       float* noisy, float* target, float* n_out) {
  const uint64_t blk = (uint64_t)e >> 2;
  const int lane = (int)(e & 3);
  uint32_t x[4];
  float z4 = 0.f;
  if (from_moments) {
    aptp_philox_block(seed, aptp_tn_subdraw(draw, APTP_TN_EPS), blk, x);
    *x0 = aptp_tn_x0(mean, logvar, aptp_philox_normal1(x, lane), k.scale);
  } else {
    *x0 = x0_in;
  }
  aptp_philox_block(seed, aptp_tn_subdraw(draw, APTP_TN_NOISE), blk, x);
  const float z2 = aptp_philox_normal1(x, lane);
  if (k.input_perturbation != 0.f) {
    aptp_philox_block(seed, aptp_tn_subdraw(draw, APTP_TN_PERTURB), blk, x);
    z4 = aptp_philox_normal1(x, lane);
  }
  aptp_tn_element(k, s, *x0, z2, s.z3[(int)(e / hw)], z4, noisy, target, n_out);
}
