// AdamW of optim.hip with both moments kept as block-wise 8-bit codes (`use_8bit_adam` of the fine-tune recipe).
// Per element 10 B read (p, g, two codes) and 8 B written (p, two codes, bf16 operand) plus two fp32 scales per 256 elements:
// 18.03 B against the 30 B of the fp32 pass.  The format -- two maps of 256 values, absmax per block of 256 elements -- is the
// one tests/adamw8_model.py defines; the arithmetic on p is packed_pass.h's adamw_element on the DEQUANTISED old moments, and
// p moves by the unquantised new ones.
//
// Geometry: optim.hip's.  In trip i of a workgroup wave w's 64 float4 cover elements base + i * 1024 + w * 256 .. + 255 of the
// item: exactly one quantisation block, so each absmax is a cross-lane max of one wave (no LDS, no barrier) and a wave stores
// its own two scales.  All four trips are loaded before the first arithmetic; the 16 new (m, v) pairs of a thread stay in
// registers across the reduction.  Both maps sit in LDS (2 KB); a code is found by bisection over the sorted map (eight reads)
// and one comparison of the two neighbours.
#include "packed_pass.h"

using namespace packed_pass;

namespace {

constexpr int QBLOCK = 256;                     // elements per quantisation block = 64 lanes x 4
static_assert(ELEMS_PER_BLOCK % QBLOCK == 0 && QBLOCK == APTP_WAVE * 4, "one wave, one trip = one quantisation block");

struct Adam8K {
  const AptpAdamW8Item* items; const int32_t* starts; int n_items;
  float lr, beta1, beta2, eps, wd;
  const float* step; const float* gate; float gscale; float warmup; const float* gscale_dev;      // as AdamK of optim.hip
  const float* qs; const float* qu;             // signed map (first moment), unsigned map (second moment)
  const float* lr_dev;                          // LR_DEV only, as AdamK of optim.hip
};

// a nearest code of x in the ascending map q[0..255] (LDS): the last value <= x by bisection, then the closer of it and its
// successor.  x below q[0] gives 0; a NaN gives 0 (its block's absmax is NaN already).
__device__ __forceinline__ uint32_t nearest_code(const float* q, float x) {
  int lo = 0;
#pragma unroll
  for (int s = 128; s >= 1; s >>= 1)
    if (q[lo + s] <= x) lo += s;
  const int hi = lo < 255 ? lo + 1 : 255;
  return (uint32_t)((q[hi] - x) < (x - q[lo]) ? hi : lo);
}

// |x| for the block's max; a non-finite x becomes +inf, which fmaxf keeps (it drops a NaN) and the kernel stores as a NaN
__device__ __forceinline__ float for_max(float x) { return non_finite(x) ? __builtin_inff() : fabsf(x); }

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
  return x;
}

__device__ __forceinline__ float quad_max(const float4& a) { return fmaxf(fmaxf(for_max(a.x), for_max(a.y)), fmaxf(for_max(a.z), for_max(a.w))); }

__device__ __forceinline__ uint32_t quad_codes(const float* q, const float4& a, float inv) {
  return nearest_code(q, a.x * inv) | nearest_code(q, a.y * inv) << 8 | nearest_code(q, a.z * inv) << 16 | nearest_code(q, a.w * inv) << 24;
}

__device__ __forceinline__ float4 dequant_quad(const float* q, uint32_t c, float absmax) {
  return float4{q[c & 255] * absmax, q[(c >> 8) & 255] * absmax, q[(c >> 16) & 255] * absmax, q[c >> 24] * absmax};
}

template <bool LR_DEV>                          // as adamw_many_kernel of optim.hip
__global__ __launch_bounds__(256) void adamw8_many_kernel(const Adam8K k) {
  __shared__ float qs[256], qu[256];
  const int b = blockIdx.x;
  const int lo = item_of_block(k.starts, k.n_items, b);
  if (k.gate && non_finite(k.gate[0])) return;  // the NaN guard of adamw_many_kernel: uniform over the grid, before any barrier
  qs[threadIdx.x] = k.qs[threadIdx.x];
  qu[threadIdx.x] = k.qu[threadIdx.x];
  const AptpAdamW8Item it = k.items[lo];
  const float gscale = k.gscale_dev ? k.gscale * k.gscale_dev[0] : k.gscale;
  const float lr = LR_DEV ? k.lr_dev[0] : warmup_lr(k.lr, k.step[0], k.warmup);
  const AdamCoef c = adam_coef(lr, k.wd, k.beta1, k.beta2, k.eps, gscale, k.step[0] + 1.0f);
  const int64_t base = (int64_t)(b - k.starts[lo]) * ELEMS_PER_BLOCK;
  __bf16* sh = (__bf16*)it.shadow;
  const int wave = threadIdx.x / APTP_WAVE;

  // every load of the four trips first.  A lane beyond n holds p = g = 0 and the zero codes: its moments are 0, old and new.
  float4 p[4], g[4];
  uint32_t cm[4], cv[4];
  float am[4], av[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t e = base + ((int64_t)i * THREADS + threadIdx.x) * 4;
    const int64_t qb = (base + (int64_t)i * THREADS * 4) / QBLOCK + wave;      // the wave's quantisation block in this trip
    p[i] = float4{0.f, 0.f, 0.f, 0.f}; g[i] = p[i];
    cm[i] = 0x7f7f7f7fu; cv[i] = 0u; am[i] = 0.f; av[i] = 0.f;
    if (qb * QBLOCK < it.n) { am[i] = it.absmax_m[qb]; av[i] = it.absmax_v[qb]; }
    if (whole_quad(e, it.n)) {
      p[i] = *reinterpret_cast<const float4*>(it.p + e);
      g[i] = *reinterpret_cast<const float4*>(it.g + e);
      cm[i] = *reinterpret_cast<const uint32_t*>(it.m8 + e);
      cv[i] = *reinterpret_cast<const uint32_t*>(it.v8 + e);
    } else {
      float* pp = reinterpret_cast<float*>(&p[i]);
      float* gg = reinterpret_cast<float*>(&g[i]);
#pragma unroll
      for (int j = 0; j < 3; ++j)                // at most three elements of a quad that is not whole
        if (e + j < it.n) {
          pp[j] = it.p[e + j]; gg[j] = it.g[e + j];
          cm[i] = (cm[i] & ~(255u << (8 * j))) | (uint32_t)it.m8[e + j] << (8 * j);
          cv[i] |= (uint32_t)it.v8[e + j] << (8 * j);
        }
    }
  }
  __syncthreads();                               // the maps

#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t e = base + ((int64_t)i * THREADS + threadIdx.x) * 4;
    const int64_t qb = (base + (int64_t)i * THREADS * 4) / QBLOCK + wave;
    float4 m = dequant_quad(qs, cm[i], am[i]);
    float4 v = dequant_quad(qu, cv[i], av[i]);
    adamw_quad(c, p[i], g[i], m, v);
    // the block's scales: a wave-level max; +inf stands for "not finite" and becomes the NaN that poisons the block visibly
    float sm = wave_max(quad_max(m)), sv = wave_max(quad_max(v));
    if (non_finite(sm)) sm = __builtin_nanf("");
    if (non_finite(sv)) sv = __builtin_nanf("");
    const float im = sm > 0.f ? 1.0f / sm : 0.f, iv = sv > 0.f ? 1.0f / sv : 0.f;      // absmax 0 (or NaN): no division, x = 0
    const uint32_t qm = quad_codes(qs, m, im), qv = quad_codes(qu, v, iv);
    if ((threadIdx.x & (APTP_WAVE - 1)) == 0 && qb * QBLOCK < it.n) { it.absmax_m[qb] = sm; it.absmax_v[qb] = sv; }
    if (whole_quad(e, it.n)) {
      *reinterpret_cast<float4*>(it.p + e) = p[i];
      *reinterpret_cast<uint32_t*>(it.m8 + e) = qm;
      *reinterpret_cast<uint32_t*>(it.v8 + e) = qv;
      if (sh) {
        uint2 q; q.x = pack_bf16x2(p[i].x, p[i].y); q.y = pack_bf16x2(p[i].z, p[i].w);
        *reinterpret_cast<uint2*>(sh + e) = q;
      }
    } else {
      const float* pp = reinterpret_cast<const float*>(&p[i]);
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (e + j < it.n) {
          it.p[e + j] = pp[j];
          it.m8[e + j] = (uint8_t)(qm >> (8 * j));
          it.v8[e + j] = (uint8_t)(qv >> (8 * j));
          if (sh) sh[e + j] = (__bf16)pp[j];
        }
    }
  }
}

}  // namespace

extern "C" int aptp_adamw8_blocks(int64_t n) { return blocks_of(n); }

extern "C" int aptp_adamw8_many(const AptpAdamW8Params* p, const float* grad_scale_dev, aptp_stream_t stream) {
  return aptp_adamw8_many_lr(p, grad_scale_dev, nullptr, stream);
}

extern "C" int aptp_adamw8_many_lr(const AptpAdamW8Params* p, const float* grad_scale_dev, const float* lr_dev, aptp_stream_t stream) {
  APTP_CHECK(p && p->items_dev && p->starts_dev && p->step_dev && p->n_items >= 1 && p->total_blocks >= 1, "adamw8_many: bad arguments");
  APTP_CHECK(p->qmap_signed_dev && p->qmap_unsigned_dev, "adamw8_many: null code map");
  APTP_CHECK((lr_dev || p->lr >= 0.f) && p->beta1 >= 0.f && p->beta1 < 1.f && p->beta2 >= 0.f && p->beta2 < 1.f && p->eps > 0.f, "adamw8_many: hyper-parameters");
  APTP_CHECK(p->grad_scale >= 0.f, "adamw8_many: grad_scale");
  APTP_CHECK(p->warmup_steps >= 0.f, "adamw8_many: warmup_steps");
  APTP_CHECK(((uintptr_t)grad_scale_dev & 3) == 0, "adamw8_many: misaligned grad_scale_dev");
  APTP_CHECK(((uintptr_t)lr_dev & 3) == 0, "adamw8_many: misaligned lr_dev");
  APTP_CHECK(!lr_dev || p->warmup_steps == 0.f, "adamw8_many: lr_dev and warmup_steps > 0 (the schedule that writes lr_dev owns the warm-up)");
  APTP_CHECK((((uintptr_t)p->qmap_signed_dev | (uintptr_t)p->qmap_unsigned_dev) & 3) == 0, "adamw8_many: misaligned code map");
  if (p->items_host) {                          // the host's copy of the table: what the kernel will dereference is checked here
    int64_t blocks = 0;
    for (int i = 0; i < p->n_items; ++i) {
      const AptpAdamW8Item& it = p->items_host[i];
      APTP_CHECK(it.p && it.g && it.m8 && it.v8 && it.absmax_m && it.absmax_v, "adamw8_many: item %d: null pointer", i);
      APTP_CHECK(it.n >= 1, "adamw8_many: item %d: n must be >= 1", i);
      APTP_CHECK((((uintptr_t)it.p | (uintptr_t)it.g) & 15) == 0 && ((uintptr_t)it.shadow & 7) == 0,
                 "adamw8_many: item %d: p and g must be 16-byte aligned, the operand 8-byte aligned", i);
      APTP_CHECK((((uintptr_t)it.m8 | (uintptr_t)it.v8) & 3) == 0, "adamw8_many: item %d: the code arrays must be 4-byte aligned", i);
      APTP_CHECK((((uintptr_t)it.absmax_m | (uintptr_t)it.absmax_v) & 3) == 0, "adamw8_many: item %d: the scale arrays must be 4-byte aligned", i);
      blocks += aptp_adamw8_blocks(it.n);
    }
    APTP_CHECK(blocks == p->total_blocks, "adamw8_many: total_blocks %d, the items need %lld", (int)p->total_blocks, (long long)blocks);
  }
  Adam8K k{p->items_dev, p->starts_dev, p->n_items, p->lr, p->beta1, p->beta2, p->eps, p->weight_decay, p->step_dev,
           p->gate_dev, p->grad_scale == 0.f ? 1.0f : p->grad_scale, p->warmup_steps, grad_scale_dev,
           p->qmap_signed_dev, p->qmap_unsigned_dev, lr_dev};
  const dim3 grid((unsigned)p->total_blocks), block(256);
  if (lr_dev) hipLaunchKernelGGL(adamw8_many_kernel<true>, grid, block, 0, (hipStream_t)stream, k);
  else hipLaunchKernelGGL(adamw8_many_kernel<false>, grid, block, 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
