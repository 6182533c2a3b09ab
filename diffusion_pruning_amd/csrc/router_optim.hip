// AdamW over the router's trainable state (hyper-net + quantizer: a few dozen small fp32 tensors) as ONE entry point whose
// schedule lives in device memory, so a captured pruning step (GraphedPrunerStep) follows the recipe of
// configs/pruning/sd-2-1_cc3m.yaml without a recapture: two parameter groups with their own rate and weight decay,
// `constant_with_warmup`, the NaN batch skip of pdm/training/trainer.py:921-929, and a step count PER TENSOR.
//
// Per element the arithmetic is adamw_many_kernel's (optim.hip), one body for both: packed_pass.h's adamw_element
// (torch.optim.AdamW: decoupled weight decay, bias correction, fp32 throughout):
//   p <- p * (1 - lr * wd);  m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g^2
//   p <- p - (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// with t = step_i + 1 (the item's own count: torch keeps one `step` per parameter and skips a parameter without a gradient, so a
// codebook that gets none during the hyper-net pre-training starts its bias correction at the phase switch) and
// lr = lr_g * min(1, applied / W_g) for W_g > 0 (LambdaLR's constant_with_warmup counted in APPLIED steps; the first runs at 0).
//
// No block of a grid reads a count that another block of the same grid advances: three small launches.
//   1. scan    every gradient element (and the gate): anything non-finite raises counters[2]
//   2. update  reads counters[2], counters[0], step_i; applies the step or leaves p, m, v alone; zeroes the gradients when asked
//   3. advance one block: step_i += 1 for every item and applied += 1, or skipped += 1; clears counters[2]
#include "packed_pass.h"

using namespace packed_pass;

namespace {

struct GroupAdamK {
  const AptpGroupAdamWItem* items; const int32_t* starts; int n_items;
  const AptpAdamWGroup* groups; int n_groups;
  float* counters;                              // {applied, skipped, bad-gradient flag, reserved}
  float beta1, beta2, eps, gscale;
  int zero_grad;
  const float* gate;                            // optional device scalar: the step is applied only when it is finite
  const float* gscale_dev;                      // optional device scalar (the clip coefficient of grad_norm.hip): one more factor of gscale
};

__global__ __launch_bounds__(256) void group_adamw_scan_kernel(const GroupAdamK k) {
  const int b = blockIdx.x;
  if (b >= k.starts[k.n_items]) return;
  const int lo = item_of_block(k.starts, k.n_items, b);
  const AptpGroupAdamWItem it = k.items[lo];
  const int64_t base = (int64_t)(b - k.starts[lo]) * ELEMS_PER_BLOCK;
  bool bad = false;
  if (b == 0 && threadIdx.x == 0 && k.gate) bad = non_finite(k.gate[0]);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t e = base + ((int64_t)i * THREADS + threadIdx.x) * 4;
    if (whole_quad(e, it.n)) {
      const float4 g = *reinterpret_cast<const float4*>(it.g + e);
      bad = bad || non_finite(g.x) || non_finite(g.y) || non_finite(g.z) || non_finite(g.w);
    } else {
      for (int64_t x = e; x < it.n && x < e + 4; ++x) bad = bad || non_finite(it.g[x]);
    }
  }
  if (bad) k.counters[2] = 1.0f;                // every writer stores the same value
}

__global__ __launch_bounds__(256) void group_adamw_update_kernel(const GroupAdamK k) {
  const int b = blockIdx.x;
  if (b >= k.starts[k.n_items]) return;
  const int lo = item_of_block(k.starts, k.n_items, b);
  const AptpGroupAdamWItem it = k.items[lo];
  if (it.group < 0 || it.group >= k.n_groups) return;
  const bool skip = k.counters[2] != 0.0f;      // uniform over the grid: written by the scan, cleared by the advance launch
  if (skip && !k.zero_grad) return;
  const AptpAdamWGroup gr = k.groups[it.group];
  const float gscale = k.gscale_dev ? k.gscale * k.gscale_dev[0] : k.gscale;      // uniform: one scalar load, one product
  const AdamCoef c = adam_coef(warmup_lr(gr.lr, k.counters[0], gr.warmup_steps), gr.weight_decay, k.beta1, k.beta2, k.eps, gscale,
                               it.step[0] + 1.0f);
  const int64_t base = (int64_t)(b - k.starts[lo]) * ELEMS_PER_BLOCK;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t e = base + ((int64_t)i * THREADS + threadIdx.x) * 4;
    if (whole_quad(e, it.n)) {
      if (!skip) {
        float4 p = *reinterpret_cast<const float4*>(it.p + e);
        const float4 g = *reinterpret_cast<const float4*>(it.g + e);
        float4 m = *reinterpret_cast<const float4*>(it.m + e);
        float4 v = *reinterpret_cast<const float4*>(it.v + e);
        adamw_quad(c, p, g, m, v);
        *reinterpret_cast<float4*>(it.p + e) = p;
        *reinterpret_cast<float4*>(it.m + e) = m;
        *reinterpret_cast<float4*>(it.v + e) = v;
      }
      if (k.zero_grad) *reinterpret_cast<float4*>(it.g + e) = zero4;
    } else {
      for (int64_t x = e; x < it.n && x < e + 4; ++x) {
        if (!skip) {
          float p = it.p[x], m = it.m[x], v = it.v[x];
          adamw_element(c, p, it.g[x], m, v);
          it.p[x] = p; it.m[x] = m; it.v[x] = v;
        }
        if (k.zero_grad) it.g[x] = 0.0f;
      }
    }
  }
}

// one block: every thread reads the flag before any thread clears it
__global__ __launch_bounds__(256) void group_adamw_advance_kernel(const GroupAdamK k) {
  const bool skip = k.counters[2] != 0.0f;
  __syncthreads();
  if (!skip)
    for (int i = threadIdx.x; i < k.n_items; i += 256) {
      float* s = k.items[i].step;
      s[0] = s[0] + 1.0f;
    }
  if (threadIdx.x == 0) {
    if (skip) k.counters[1] = k.counters[1] + 1.0f; else k.counters[0] = k.counters[0] + 1.0f;
    k.counters[2] = 0.0f;
  }
}

}  // namespace

extern "C" int aptp_group_adamw_blocks(int64_t n) { return blocks_of(n); }

extern "C" int aptp_group_adamw(const AptpGroupAdamWParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->items_dev && p->starts_dev && p->groups_dev && p->counters_dev, "group_adamw: null pointer");
  APTP_CHECK(p->n_items >= 1 && p->n_groups >= 1 && p->total_blocks >= 1, "group_adamw: n_items, n_groups and total_blocks must be >= 1");
  APTP_CHECK(p->beta1 >= 0.f && p->beta1 < 1.f && p->beta2 >= 0.f && p->beta2 < 1.f && p->eps > 0.f, "group_adamw: hyper-parameters");
  APTP_CHECK(p->grad_scale >= 0.f, "group_adamw: grad_scale");
  APTP_CHECK(((uintptr_t)p->items_dev & 7) == 0 && ((uintptr_t)p->starts_dev & 3) == 0 && ((uintptr_t)p->groups_dev & 3) == 0 &&
             ((uintptr_t)p->counters_dev & 15) == 0 && ((uintptr_t)p->gate_dev & 3) == 0 && ((uintptr_t)p->grad_scale_dev & 3) == 0,
             "group_adamw: misaligned table");
  if (p->items_host) {                          // the host's copy of the table: what the kernels will dereference is checked here
    int64_t blocks = 0;
    for (int i = 0; i < p->n_items; ++i) {
      const AptpGroupAdamWItem& it = p->items_host[i];
      APTP_CHECK(it.p && it.g && it.m && it.v && it.step, "group_adamw: item %d: null pointer", i);
      APTP_CHECK(it.n >= 1, "group_adamw: item %d: n must be >= 1", i);
      APTP_CHECK(it.group >= 0 && it.group < p->n_groups, "group_adamw: item %d: group %d of %d", i, (int)it.group, (int)p->n_groups);
      APTP_CHECK((((uintptr_t)it.p | (uintptr_t)it.g | (uintptr_t)it.m | (uintptr_t)it.v) & 15) == 0 && ((uintptr_t)it.step & 3) == 0,
                 "group_adamw: item %d: p, g, m and v must be 16-byte aligned", i);
      blocks += aptp_group_adamw_blocks(it.n);
    }
    APTP_CHECK(blocks == p->total_blocks, "group_adamw: total_blocks %d, the items need %lld", (int)p->total_blocks, (long long)blocks);
  }
  GroupAdamK k{p->items_dev, p->starts_dev, p->n_items, p->groups_dev, p->n_groups, p->counters_dev, p->beta1, p->beta2, p->eps,
               p->grad_scale == 0.f ? 1.0f : p->grad_scale, p->zero_grad != 0, p->gate_dev,
               p->grad_scale_dev};
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)p->total_blocks), block(256);
  hipLaunchKernelGGL(group_adamw_scan_kernel, grid, block, 0, s, k);
  hipLaunchKernelGGL(group_adamw_update_kernel, grid, block, 0, s, k);
  hipLaunchKernelGGL(group_adamw_advance_kernel, dim3(1), block, 0, s, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
