// Seeded training batches on the device:
//   aptp_train_noise   VAE moments (or latents) and per-sample seeds -> noisy latents, target and timesteps in ONE launch; every
//                      value a pure function of (seed of the sample, draw, element), whatever batch the sample sits in.  The draw
//                      map and every arithmetic statement are csrc/train_noise.h; this file only moves data.
// Memory- and launch-bound: blockIdx.y is the sample; its timestep, table row and offset normals are formed by one lane per
// workgroup and shared through LDS.  With hw % 4 == 0 and 16-byte aligned tensors a lane owns an aligned group of four elements
// of one channel (at most three Philox evaluations, 16-byte loads and stores); otherwise one element per lane with the same
// statements, so both paths give the same bits.  No reductions, no atomics: bit-equal from run to run and capture to replay.
#include "aptp_common.h"
#include "train_noise.h"

#pragma clang fp contract(off)

namespace {

struct TrainNoiseK {
  const float* moments; const float* latents_in; const float* table;
  const int64_t* seeds; const int64_t* draw_dev;
  float* noisy; float* target; int64_t* timesteps; float* latents_out; float* noise_out;
  int64_t draw, hw, T;
  AptpTnKnobs knobs;
};

template <bool VEC>
__global__ __launch_bounds__(256) void train_noise_kernel(const TrainNoiseK p) {
  __shared__ AptpTnSample shared;
  const int64_t row = blockIdx.y;
  const uint64_t seed = (uint64_t)p.seeds[row];
  const uint64_t draw = (uint64_t)p.draw + (p.draw_dev ? (uint64_t)p.draw_dev[0] : 0ull);
  if (threadIdx.x == 0) {
    aptp_tn_sample(seed, draw, p.T, p.table, p.knobs.noise_offset != 0.f, &shared);
    if (blockIdx.x == 0) p.timesteps[row] = shared.t;
  }
  __syncthreads();
  const AptpTnSample s = shared;
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n4 = 4 * p.hw;                                // elements of a sample
  const int64_t e = VEC ? 4 * k : k;
  if (e >= n4) return;
  const int64_t i = row * n4 + e;                             // into [B, 4, h, w]
  const int c = (int)(e / p.hw);
  const int64_t im = row * 2 * n4 + e;                        // the mean in [B, 8, h, w]; the logvar is 4 hw further on
  if constexpr (VEC) {
    uint32_t x[4];
    float x0[4], z2[4], z4[4] = {0.f, 0.f, 0.f, 0.f}, noisy[4], target[4], n[4];
    if (p.moments) {
      const float4 mean = *reinterpret_cast<const float4*>(p.moments + im);
      const float4 logvar = *reinterpret_cast<const float4*>(p.moments + im + n4);
      float z1[4];
      aptp_philox_block(seed, aptp_tn_subdraw(draw, APTP_TN_EPS), (uint64_t)k, x);
      aptp_philox_normals4(x, z1);
      x0[0] = aptp_tn_x0(mean.x, logvar.x, z1[0], p.knobs.scale);
      x0[1] = aptp_tn_x0(mean.y, logvar.y, z1[1], p.knobs.scale);
      x0[2] = aptp_tn_x0(mean.z, logvar.z, z1[2], p.knobs.scale);
      x0[3] = aptp_tn_x0(mean.w, logvar.w, z1[3], p.knobs.scale);
    } else {
      const float4 v = *reinterpret_cast<const float4*>(p.latents_in + i);
      x0[0] = v.x; x0[1] = v.y; x0[2] = v.z; x0[3] = v.w;
    }
    aptp_philox_block(seed, aptp_tn_subdraw(draw, APTP_TN_NOISE), (uint64_t)k, x);
    aptp_philox_normals4(x, z2);
    if (p.knobs.input_perturbation != 0.f) {
      aptp_philox_block(seed, aptp_tn_subdraw(draw, APTP_TN_PERTURB), (uint64_t)k, x);
      aptp_philox_normals4(x, z4);
    }
    aptp_tn_element4(p.knobs, s, x0, z2, s.z3[c], z4, noisy, target, n);
    *reinterpret_cast<float4*>(p.noisy + i) = make_float4(noisy[0], noisy[1], noisy[2], noisy[3]);
    *reinterpret_cast<float4*>(p.target + i) = make_float4(target[0], target[1], target[2], target[3]);
    if (p.latents_out) *reinterpret_cast<float4*>(p.latents_out + i) = make_float4(x0[0], x0[1], x0[2], x0[3]);
    if (p.noise_out) *reinterpret_cast<float4*>(p.noise_out + i) = make_float4(n[0], n[1], n[2], n[3]);
  } else {
    float mean = 0.f, logvar = 0.f, x0_in = 0.f, x0, noisy, target, n;
    if (p.moments) { mean = p.moments[im]; logvar = p.moments[im + n4]; }
    else x0_in = p.latents_in[i];
    aptp_tn_element_of(p.knobs, s, seed, draw, e, p.hw, p.moments != nullptr, mean, logvar, x0_in, &x0, &noisy, &target, &n);
    p.noisy[i] = noisy;
    p.target[i] = target;
    if (p.latents_out) p.latents_out[i] = x0;
    if (p.noise_out) p.noise_out[i] = n;
  }
}

}  // namespace

extern "C" int aptp_train_noise(const AptpTrainNoiseParams* p, aptp_stream_t stream) {
  APTP_CHECK(p, "train_noise: null pointer");
  APTP_CHECK(p->sqrt_table && p->seeds_dev && p->noisy && p->target && p->timesteps,
             "train_noise: null pointer (sqrt_table, seeds_dev, noisy, target, timesteps)");
  APTP_CHECK((p->moments != nullptr) != (p->latents_in != nullptr), "train_noise: give exactly one of moments and latents_in");
  APTP_CHECK(p->B >= 1 && p->B <= 65535, "train_noise: B = %d outside 1..65535", p->B);
  APTP_CHECK(p->h >= 1 && p->w >= 1 && (int64_t)p->h * p->w <= (1ll << 36) / p->B, "train_noise: bad extents h = %d, w = %d", p->h, p->w);
  APTP_CHECK(p->T >= 1, "train_noise: T = %d is below 1", p->T);
  APTP_CHECK(p->draw >= 0 && p->draw < (1ll << 59), "train_noise: draw %lld outside [0, 2^59)", (long long)p->draw);
  APTP_CHECK(p->prediction == APTP_TRAIN_NOISE_EPSILON || p->prediction == APTP_TRAIN_NOISE_V_PREDICTION,
             "train_noise: unknown prediction %d", p->prediction);
  const void* f32[] = {p->moments, p->latents_in, p->sqrt_table, p->noisy, p->target, p->latents_out, p->noise_out};
  bool aligned16 = true;
  for (const void* q : f32) {
    APTP_CHECK(((uintptr_t)q % 4) == 0, "train_noise: pointer alignment");
    aligned16 = aligned16 && (q == p->sqrt_table || ((uintptr_t)q % 16) == 0);
  }
  APTP_CHECK(((uintptr_t)p->seeds_dev % 8) == 0 && ((uintptr_t)p->draw_dev % 8) == 0 && ((uintptr_t)p->timesteps % 8) == 0,
             "train_noise: pointer alignment");
  TrainNoiseK k;
  k.moments = p->moments; k.latents_in = p->latents_in; k.table = p->sqrt_table; k.seeds = p->seeds_dev; k.draw_dev = p->draw_dev;
  k.noisy = p->noisy; k.target = p->target; k.timesteps = p->timesteps; k.latents_out = p->latents_out; k.noise_out = p->noise_out;
  k.draw = p->draw; k.hw = (int64_t)p->h * p->w; k.T = p->T;
  k.knobs.scale = p->scale; k.knobs.noise_offset = p->noise_offset; k.knobs.input_perturbation = p->input_perturbation;
  k.knobs.v_prediction = p->prediction == APTP_TRAIN_NOISE_V_PREDICTION ? 1 : 0;
  // a lane owns four elements where they are one channel's and sit at a 16-byte address in every tensor and every sample
  const bool vec = k.hw % 4 == 0 && aligned16;
  const int64_t lanes = vec ? k.hw : 4 * k.hw;
  const int64_t blocks = (lanes + 255) / 256;
  APTP_CHECK(blocks < (1ll << 31), "train_noise: too many elements");
  const dim3 grid((unsigned)blocks, (unsigned)p->B), block(256);
  if (vec) hipLaunchKernelGGL(train_noise_kernel<true>, grid, block, 0, (hipStream_t)stream, k);
  else hipLaunchKernelGGL(train_noise_kernel<false>, grid, block, 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
