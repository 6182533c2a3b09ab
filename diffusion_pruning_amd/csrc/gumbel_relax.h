// The router's Gumbel-sigmoid relaxation on seeded noise (csrc/gumbel_relax.hip), on the stream of philox_normal.h
// unchanged.  Row r of a call has an int64 seed, the call a Philox draw; element e of the row reads ONE word of that stream:
//   word  = word (e & 3) of aptp_philox_block(seed, draw, e >> 2)
//   e     = c for width column c of the input;  e = nw + j for the depth entry at SORTED position j (where the noise is
//           applied, before the depth_order scatter)
//   draw  of a sample row:   aptp_tn_subdraw(d, k), d the batch's draw (train_noise.h), k = 6 the noise of the optimal-transport
//                            assignment, k = 7 the noise of the relaxation itself
//         of a codebook row: 2^63 | noise_step, seed = router_seed + code index (sample draws are below 2^62: no collision)
//   u     = aptp_philox_u1(word) in (0, 1], exact;   G = -logf(1e-20f - logf(u))
//           (the reference's -log(-log(U + eps) + eps): u + 1e-20 rounds to u for every u of this form)
// fp32, contraction off, every sum in index order (T the temperature, `base` the offset):
//   width  w = sigmoid((z + G + base) / T);  non-zero-width rule: a segment with no w >= 0.5f gets +0.5f on its first entry
//   depth  sm = softmax(zd),  p = flip(cumsum(sm)),  x = logf(p + 1e-6f) - log1pf(-(p - 1e-6f)),
//          d_sorted = sigmoid((x + G + base) / T),  out[nw + depth_order[j]] = d_sorted[j]
// backward: d out / d z with the noise and the bump as constants -- s (1 - s) / T on the un-bumped sigmoid, the logit's
//   1 / (p + 1e-6) + 1 / (1 - (p - 1e-6)), the transpose of flip-cumsum, the softmax backward.  Everything but z is recomputed.
// Plain C++ for the device and the host, as philox_normal.h and train_noise.h are.
#pragma once
#include "train_noise.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define APTP_TN_ROUTER_ASSIGN 6        // the two sub-draws train_noise.h leaves free
#define APTP_TN_ROUTER_RELAX 7
#define APTP_GR_CODEBOOK_BIT 0x8000000000000000ull

// the Philox draw of a call from the value in device memory: the batch's draw, or the count of steps run for the codebook
APTP_PHILOX_HD uint64_t aptp_gr_draw(uint64_t d, int sub, bool codebook) {
  return codebook ? (APTP_GR_CODEBOOK_BIT | d) : aptp_tn_subdraw(d, sub);
}

APTP_PHILOX_HD uint32_t aptp_gr_word(uint64_t seed, uint64_t draw, uint64_t e) {
  uint32_t x[4];
  aptp_philox_block(seed, draw, e >> 2, x);
  const int lane = (int)(e & 3);
  return lane == 0 ? x[0] : (lane == 1 ? x[1] : (lane == 2 ? x[2] : x[3]));
}

APTP_PHILOX_HD float aptp_gr_gumbel_of(uint32_t word) { return -logf(1e-20f - logf(aptp_philox_u1(word))); }

APTP_PHILOX_HD float aptp_gr_gumbel(uint64_t seed, uint64_t draw, uint64_t e) { return aptp_gr_gumbel_of(aptp_gr_word(seed, draw, e)); }

APTP_PHILOX_HD float aptp_gr_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// one relaxed entry from its logit and its noise
APTP_PHILOX_HD float aptp_gr_relax(float logit, float G, float base, float T) { return aptp_gr_sigmoid((logit + G + base) / T); }

// d relax / d logit from the relaxed (un-bumped) value
APTP_PHILOX_HD float aptp_gr_relax_grad(float s, float T) { return (1.0f - s) * s / T; }

// the non-zero-width rule of one segment w[lo, hi): true where no entry reaches 0.5 (the caller then adds 0.5f to w[lo])
APTP_PHILOX_HD bool aptp_gr_segment_dead(const float* w, int lo, int hi) {
  int alive = 0;
  for (int c = lo; c < hi; ++c) alive += w[c] >= 0.5f ? 1 : 0;
  return alive == 0;
}

// the depth chain of one row, walked in index order: sm, p, d_sorted are nd floats each (sm the softmax, p the flipped cumsum)
APTP_PHILOX_HD void aptp_gr_depth_forward(const float* zd, int nd, uint64_t seed, uint64_t draw, int nw, float T, float base,
                                          float* sm, float* p, float* d_sorted) {
  float m = -INFINITY;
  for (int k = 0; k < nd; ++k) m = fmaxf(m, zd[k]);
  float sum = 0.f;
  for (int k = 0; k < nd; ++k) { sm[k] = expf(zd[k] - m); sum += sm[k]; }
  float run = 0.f;
  for (int k = 0; k < nd; ++k) {
    sm[k] = sm[k] / sum;
    run += sm[k];
    p[nd - 1 - k] = run;
  }
  for (int j = 0; j < nd; ++j) {
    const float x = logf(p[j] + 1e-6f) - log1pf(-(p[j] - 1e-6f));
    d_sorted[j] = aptp_gr_relax(x, aptp_gr_gumbel(seed, draw, (uint64_t)nw + (uint64_t)j), base, T);
  }
}

// its backward: g[j] the gradient w.r.t. d_sorted[j] on entry, overwritten; dzd nd floats
APTP_PHILOX_HD void aptp_gr_depth_backward(float* g, const float* sm, const float* p, const float* d_sorted, int nd, float T, float* dzd) {
  // d_sorted -> x -> p
  for (int j = 0; j < nd; ++j)
    g[j] = g[j] * aptp_gr_relax_grad(d_sorted[j], T) * (1.0f / (p[j] + 1e-6f) + 1.0f / (1.0f - (p[j] - 1e-6f)));
  // p[j] = c[nd - 1 - j], c = cumsum(sm): d sm[k] = sum_{i >= k} d c[i] = sum_{j <= nd - 1 - k} g[j], a running sum over j
  float run = 0.f, dot = 0.f;
  for (int j = 0; j < nd; ++j) {
    run += g[j];
    dzd[nd - 1 - j] = run;
  }
  for (int k = 0; k < nd; ++k) dot += sm[k] * dzd[k];
  for (int k = 0; k < nd; ++k) dzd[k] = sm[k] * (dzd[k] - dot);
}
