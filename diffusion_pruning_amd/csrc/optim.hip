// AdamW over the packed trainable state of an expert (packed_train.PackedTrainer) as ONE launch, with the bf16 operand the
// GEMM kernels read ("shadow") written by the same pass.  Replaces torch's multi-tensor fused AdamW (34 launches, 3.4 ms at
// 396 M parameters) plus the multi-tensor fp32 -> bf16 cast of the shadows (25 launches, 0.8 ms): per parameter 16 B read
// (p, g, m, v) and 14 B written (p, m, v, shadow) in one pass -- HBM-bound, 11.9 GB per step for this expert.
//
// Same arithmetic as torch.optim.AdamW (decoupled weight decay, bias correction, fp32 throughout; torch/optim/adamw.py,
// the `capturable` fused form: step count read from device memory):
//   p <- p * (1 - lr * wd);  m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g^2
//   p <- p - (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// (one body, packed_pass.h's adamw_element, shared with the router's optimizer in router_optim.hip).
// The table of tensors lives in device memory (built once; the gradient addresses are those of the captured backward).
// Below it: aptp_grad_accumulate, the sum of a window of micro-batch gradients that such a step is applied to.
#include "packed_pass.h"

using namespace packed_pass;

namespace {

struct AdamK {
  const AptpAdamWItem* items; const int32_t* starts; int n_items;
  float lr, beta1, beta2, eps, wd;
  const float* step;                            // device scalar: number of steps taken BEFORE this one
  const float* gate;                            // optional device scalar: the step is applied only when it is finite
  float gscale;                                 // gradients are multiplied by this first (1 / world size of a summed exchange)
  float warmup;                                 // 0 = off; else the rate ramps linearly over this many optimizer steps
  const float* gscale_dev;                      // optional device scalar (the clip coefficient of grad_norm.hip): one more factor of gscale
  const float* lr_dev;                          // LR_DEV only: the rate itself (what aptp_lr_schedule stored); lr and warmup are not read
};

// LR_DEV: the rate is one more uniform scalar load instead of warmup_lr; the instantiation without it is the kernel as it was
template <bool LR_DEV>
__global__ __launch_bounds__(256) void adamw_many_kernel(const AdamK k) {
  const int b = blockIdx.x;
  const int lo = item_of_block(k.starts, k.n_items, b);
  // NaN guard of a replayed graph (reference: pdm/training/trainer.py:921-929 skips the batch whose backward produced
  // NaNs): a non-finite loss leaves parameters, moments and operands untouched; the caller advances the step count by
  // the same predicate.  Uniform over the grid: one scalar load.
  if (k.gate && non_finite(k.gate[0])) return;
  const AptpAdamWItem it = k.items[lo];
  // the warm-up is counted in optimizer steps.  Uniform; W = 0 leaves lr as passed.  So is the clip: one scalar load, one product.
  const float gscale = k.gscale_dev ? k.gscale * k.gscale_dev[0] : k.gscale;
  const float lr = LR_DEV ? k.lr_dev[0] : warmup_lr(k.lr, k.step[0], k.warmup);
  const AdamCoef c = adam_coef(lr, k.wd, k.beta1, k.beta2, k.eps, gscale, k.step[0] + 1.0f);
  const int64_t base = (int64_t)(b - k.starts[lo]) * ELEMS_PER_BLOCK;
  __bf16* sh = (__bf16*)it.shadow;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t e = base + ((int64_t)i * THREADS + threadIdx.x) * 4;
    if (whole_quad(e, it.n)) {
      float4 p = *reinterpret_cast<const float4*>(it.p + e);
      const float4 g = *reinterpret_cast<const float4*>(it.g + e);
      float4 m = *reinterpret_cast<const float4*>(it.m + e);
      float4 v = *reinterpret_cast<const float4*>(it.v + e);
      adamw_quad(c, p, g, m, v);
      *reinterpret_cast<float4*>(it.p + e) = p;
      *reinterpret_cast<float4*>(it.m + e) = m;
      *reinterpret_cast<float4*>(it.v + e) = v;
      if (sh) {
        uint2 q; q.x = pack_bf16x2(p.x, p.y); q.y = pack_bf16x2(p.z, p.w);
        *reinterpret_cast<uint2*>(sh + e) = q;
      }
    } else {
      for (int64_t x = e; x < it.n && x < e + 4; ++x) {
        float p = it.p[x], m = it.m[x], v = it.v[x];
        adamw_element(c, p, it.g[x], m, v);
        it.p[x] = p; it.m[x] = m; it.v[x] = v;
        if (sh) sh[x] = (__bf16)p;
      }
    }
  }
}

}  // namespace

extern "C" int aptp_adamw_blocks(int64_t n) { return blocks_of(n); }

extern "C" int aptp_adamw_many(const AptpAdamWParams* p, aptp_stream_t stream) { return aptp_adamw_many_scaled(p, nullptr, stream); }

extern "C" int aptp_adamw_many_scaled(const AptpAdamWParams* p, const float* grad_scale_dev, aptp_stream_t stream) {
  return aptp_adamw_many_lr(p, grad_scale_dev, nullptr, stream);
}

extern "C" int aptp_adamw_many_lr(const AptpAdamWParams* p, const float* grad_scale_dev, const float* lr_dev, aptp_stream_t stream) {
  APTP_CHECK(p && p->items_dev && p->starts_dev && p->step_dev && p->n_items >= 1 && p->total_blocks >= 1, "adamw_many: bad arguments");
  APTP_CHECK((lr_dev || p->lr >= 0.f) && p->beta1 >= 0.f && p->beta1 < 1.f && p->beta2 >= 0.f && p->beta2 < 1.f && p->eps > 0.f, "adamw_many: hyper-parameters");
  APTP_CHECK(p->grad_scale >= 0.f, "adamw_many: grad_scale");
  APTP_CHECK(p->warmup_steps >= 0.f, "adamw_many: warmup_steps");
  APTP_CHECK(((uintptr_t)grad_scale_dev & 3) == 0, "adamw_many: misaligned grad_scale_dev");
  APTP_CHECK(((uintptr_t)lr_dev & 3) == 0, "adamw_many: misaligned lr_dev");
  APTP_CHECK(!lr_dev || p->warmup_steps == 0.f, "adamw_many: lr_dev and warmup_steps > 0 (the schedule that writes lr_dev owns the warm-up)");
  AdamK k{p->items_dev, p->starts_dev, p->n_items, p->lr, p->beta1, p->beta2, p->eps, p->weight_decay, p->step_dev,
          p->gate_dev, p->grad_scale == 0.f ? 1.0f : p->grad_scale, p->warmup_steps, grad_scale_dev, lr_dev};
  const dim3 grid((unsigned)p->total_blocks), block(256);
  if (lr_dev) hipLaunchKernelGGL(adamw_many_kernel<true>, grid, block, 0, (hipStream_t)stream, k);
  else hipLaunchKernelGGL(adamw_many_kernel<false>, grid, block, 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}

// ---- gradient accumulation over the micro-batches of an optimizer window ------------------------------------------------------
// acc and g are the accumulator and the gradient arena of an expert (fp32, up to ~0.9 G elements: int64 indices).  Pure HBM
// streaming: 8 B (STORE) or 12 B (ADD, FINAL) per element, nothing to reuse.  A block takes ELEMS_PER_BLOCK elements per trip --
// its 4 float4 loads per operand are issued before the first add -- and the grid is capped, the rest is a grid stride: the
// whole-arena launch of an SD-2.1 expert would otherwise be ~10^5 blocks of one trip each.
namespace {

constexpr int ACCUM_MAX_BLOCKS = 2048;          // 256 CUs x 8 resident blocks of 256 threads

template <int MODE>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ acc, float* __restrict__ g, const int64_t n) {
  const int64_t n4 = n & ~(int64_t)3;           // the float4 part; acc and g are 16-byte aligned
  const int64_t stride = (int64_t)gridDim.x * ELEMS_PER_BLOCK;
  for (int64_t base = (int64_t)blockIdx.x * ELEMS_PER_BLOCK; base < n4; base += stride) {
    float4 a[4], b[4];
    int64_t e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      e[i] = base + ((int64_t)i * 256 + threadIdx.x) * 4;
      if (e[i] < n4) {
        b[i] = *reinterpret_cast<const float4*>(g + e[i]);
        if (MODE != APTP_GRAD_ACCUM_STORE) a[i] = *reinterpret_cast<const float4*>(acc + e[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (e[i] < n4) {
        float4 r = b[i];
        if (MODE != APTP_GRAD_ACCUM_STORE) { r.x = a[i].x + b[i].x; r.y = a[i].y + b[i].y; r.z = a[i].z + b[i].z; r.w = a[i].w + b[i].w; }
        *reinterpret_cast<float4*>((MODE == APTP_GRAD_ACCUM_FINAL ? g : acc) + e[i]) = r;
      }
    }
  }
  if (blockIdx.x == 0 && n4 + threadIdx.x < n) {        // scalar tail: at most 3 elements
    const int64_t x = n4 + threadIdx.x;
    const float gv = g[x];
    if (MODE == APTP_GRAD_ACCUM_STORE) acc[x] = gv;
    else if (MODE == APTP_GRAD_ACCUM_ADD) acc[x] = acc[x] + gv;
    else g[x] = acc[x] + gv;
  }
}

}  // namespace

extern "C" int aptp_grad_accumulate_blocks(int64_t n) {
  if (n <= 0) return 0;
  const int64_t b = (n + ELEMS_PER_BLOCK - 1) / ELEMS_PER_BLOCK;
  return (int)(b < ACCUM_MAX_BLOCKS ? b : ACCUM_MAX_BLOCKS);
}

extern "C" int aptp_grad_accumulate(const AptpGradAccumParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->acc && p->g, "grad_accumulate: null pointer");
  APTP_CHECK(p->n >= 1, "grad_accumulate: n must be >= 1");
  APTP_CHECK(p->mode >= APTP_GRAD_ACCUM_STORE && p->mode <= APTP_GRAD_ACCUM_FINAL, "grad_accumulate: mode %d", (int)p->mode);
  APTP_CHECK(((uintptr_t)p->acc & 15) == 0 && ((uintptr_t)p->g & 15) == 0, "grad_accumulate: acc and g must be 16-byte aligned");
  APTP_CHECK(p->acc != p->g, "grad_accumulate: acc and g are the same buffer");
  const dim3 grid((unsigned)aptp_grad_accumulate_blocks(p->n)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (p->mode == APTP_GRAD_ACCUM_STORE) hipLaunchKernelGGL(grad_accumulate_kernel<APTP_GRAD_ACCUM_STORE>, grid, block, 0, s, p->acc, p->g, p->n);
  else if (p->mode == APTP_GRAD_ACCUM_ADD) hipLaunchKernelGGL(grad_accumulate_kernel<APTP_GRAD_ACCUM_ADD>, grid, block, 0, s, p->acc, p->g, p->n);
  else hipLaunchKernelGGL(grad_accumulate_kernel<APTP_GRAD_ACCUM_FINAL>, grid, block, 0, s, p->acc, p->g, p->n);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
