// What the table-driven passes over the packed trainable state share (optim.hip, router_optim.hip, ema.hip; the item lookup
// also serves pack_ops.hip): block geometry, item lookup, finiteness predicate and THE AdamW element.  No state.  DESIGN 6s.
//
// The helpers hand back indices and predicates; every load and store stays in the kernel's own body.  A trip loop shared as a
// template over lambdas compiles to flat_* memory instructions (the compiler no longer sees that the pointers of an item are
// global once they pass through a closure), so the four-trip loop is written out per kernel.
#pragma once
#include "aptp_common.h"

namespace packed_pass {

constexpr int THREADS = 256;
constexpr int ELEMS_PER_BLOCK = THREADS * 4 * 4;         // 4096: every thread takes 4 float4, THREADS * 4 elements apart

// blocks of an item of n elements (aptp_adamw_blocks, aptp_group_adamw_blocks; the EMA tables use the former)
constexpr int blocks_of(int64_t n) { return n <= 0 ? 0 : (int)((n + ELEMS_PER_BLOCK - 1) / ELEMS_PER_BLOCK); }

// the item that block b belongs to: starts[i] = first block of item i, starts[n_items] = grid size (starts[lo] <= b < starts[hi])
__device__ __forceinline__ int item_of_block(const int32_t* starts, int n_items, int b) {
  int lo = 0, hi = n_items;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (starts[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

// Trip i (0..3) of a block: the thread's float4 starts at element e = base + ((int64_t)i * THREADS + threadIdx.x) * 4 of the item.
// The kernels spell this out: behind a helper, in either of two forms tried, one kernel or another gets other index arithmetic
// and other register counts than it had.
// the four elements at e all belong to an item of n elements (else: the scalar tail e .. min(n, e + 4))
__device__ __forceinline__ bool whole_quad(int64_t e, int64_t n) { return e + 3 < n; }

// torch.isfinite: what the host side of a gated step counts with (PackedAdamW.finish_step, PackedEMA.step)
__device__ __forceinline__ bool non_finite(float x) { return !(fabsf(x) <= 3.402823466e38f); }

// AdamW of torch.optim.AdamW (decoupled weight decay, bias correction, fp32 throughout) for the step that makes the count t
struct AdamCoef { float beta1, beta2, eps, gscale, step_size, bc2_sqrt, decay; };

__device__ __forceinline__ AdamCoef adam_coef(float lr, float wd, float beta1, float beta2, float eps, float gscale, float t) {
  const float bc1 = 1.0f - powf(beta1, t), bc2 = 1.0f - powf(beta2, t);
  return AdamCoef{beta1, beta2, eps, gscale, lr / bc1, sqrtf(bc2), 1.0f - lr * wd};
}

// constant_with_warmup: rate lr * min(1, k / W) at the step that follows k applied ones (the first runs at 0); W = 0 leaves lr
__device__ __forceinline__ float warmup_lr(float lr, float applied, float warmup) {
  return warmup > 0.0f ? lr * fminf(1.0f, applied / warmup) : lr;
}

// the one body of the formula (float4 lanes and scalar tails of both AdamW kernels); g is the raw gradient
__device__ __forceinline__ void adamw_element(const AdamCoef& c, float& p, float g, float& m, float& v) {
  g *= c.gscale;
  p *= c.decay;
  m = c.beta1 * m + (1.0f - c.beta1) * g;
  v = c.beta2 * v + (1.0f - c.beta2) * g * g;
  p -= c.step_size * m / (sqrtf(v) / c.bc2_sqrt + c.eps);
}

__device__ __forceinline__ void adamw_quad(const AdamCoef& c, float4& p, const float4& g, float4& m, float4& v) {
  adamw_element(c, p.x, g.x, m.x, v.x); adamw_element(c, p.y, g.y, m.y, v.y);
  adamw_element(c, p.z, g.z, m.z, v.z); adamw_element(c, p.w, g.w, m.w, v.w);
}

}  // namespace packed_pass
