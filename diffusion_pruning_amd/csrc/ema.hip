// Exponential moving average of the packed trainable state of an expert (packed_train.PackedEMA) as ONE launch over a device
// table, gated and counted on the device like the AdamW pass next to it (optim.hip), plus the exchange of the averaged and the
// trained values that lets the validation graphs and the checkpoint export read the average at the addresses they already know.
// Pure HBM streaming, nothing to reuse: UPDATE reads p and ema and writes ema (12 B per element), SWAP reads and writes both
// (16 B) and writes the bf16 operand of a weight (18 B).
//
// The decay is the rule of diffusers' EMAModel (diffusers/training_utils.py: get_decay, step), evaluated in fp32 from the
// device-side count of applied EMA steps:
//   n = count + 1;  s = max(0, n - update_after_step - 1)
//   s <= 0:  d = 0                                  (the first applied step copies the parameters)
//   else     base = use_warmup ? 1 - (1 + s / inv_gamma)^(-power) : (1 + s) / (10 + s)
//            d = max(min_decay, min(base, decay))
//   ema <- ema - (1 - d) * (ema - p)
// 1 - d == 1 stores p itself: ema - (ema - p) is p only up to a rounding of the difference.
#include "packed_pass.h"

using namespace packed_pass;                    // the tables are laid out by aptp_adamw_blocks

namespace {

struct EmaK {
  const AptpEmaItem* items; const int32_t* starts; int n_items;
  const float* count;                           // device scalar: EMA steps applied BEFORE this call
  const float* gate;                            // optional device scalar: the update is applied only when it is finite
  float decay, min_decay, update_after, inv_gamma, power;
  int use_warmup;
  float* cur_decay;                             // optional device scalar: the decay this call used
};

__device__ __forceinline__ float ema_decay(const EmaK& k) {
  const float n = k.count[0] + 1.0f;
  const float s = fmaxf(0.0f, n - k.update_after - 1.0f);
  if (s <= 0.0f) return 0.0f;
  const float base = k.use_warmup ? 1.0f - powf(1.0f + s / k.inv_gamma, -k.power) : (1.0f + s) / (10.0f + s);
  return fmaxf(k.min_decay, fminf(base, k.decay));
}

template <int MODE>
__global__ __launch_bounds__(256) void ema_many_kernel(const EmaK k) {
  const int b = blockIdx.x;
  float omd = 0.0f;
  if (MODE == APTP_EMA_UPDATE) {
    // same predicate as the AdamW pass: a non-finite loss leaves the average (and the reported decay) untouched; the caller
    // advances the count by the same predicate.  Uniform over the grid: one scalar load.
    if (k.gate && non_finite(k.gate[0])) return;
    const float d = ema_decay(k);
    omd = 1.0f - d;
    if (b == 0 && threadIdx.x == 0 && k.cur_decay) k.cur_decay[0] = d;
  }
  const int lo = item_of_block(k.starts, k.n_items, b);
  const AptpEmaItem it = k.items[lo];
  const int64_t base = (int64_t)(b - k.starts[lo]) * ELEMS_PER_BLOCK;
  const bool copy = omd == 1.0f;
  __bf16* sh = (__bf16*)it.shadow;
  float4 p[4], a[4];
  int64_t e[4];
  // the block's loads are requested before its first store
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    e[i] = base + ((int64_t)i * THREADS + threadIdx.x) * 4;
    if (whole_quad(e[i], it.n)) {
      p[i] = *reinterpret_cast<const float4*>(it.p + e[i]);
      a[i] = *reinterpret_cast<const float4*>(it.ema + e[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (whole_quad(e[i], it.n)) {
      if (MODE == APTP_EMA_UPDATE) {
        float4 r = p[i];
        if (!copy) {
          r.x = a[i].x - omd * (a[i].x - p[i].x); r.y = a[i].y - omd * (a[i].y - p[i].y);
          r.z = a[i].z - omd * (a[i].z - p[i].z); r.w = a[i].w - omd * (a[i].w - p[i].w);
        }
        *reinterpret_cast<float4*>(it.ema + e[i]) = r;
      } else {
        *reinterpret_cast<float4*>(it.p + e[i]) = a[i];
        *reinterpret_cast<float4*>(it.ema + e[i]) = p[i];
        if (sh) {
          uint2 q; q.x = pack_bf16x2(a[i].x, a[i].y); q.y = pack_bf16x2(a[i].z, a[i].w);
          *reinterpret_cast<uint2*>(sh + e[i]) = q;
        }
      }
    } else {
      for (int64_t x = e[i]; x < it.n && x < e[i] + 4; ++x) {         // scalar tail: at most 3 elements of the item
        const float pv = it.p[x], av = it.ema[x];
        if (MODE == APTP_EMA_UPDATE) {
          it.ema[x] = copy ? pv : av - omd * (av - pv);
        } else {
          it.p[x] = av; it.ema[x] = pv;
          if (sh) sh[x] = (__bf16)av;
        }
      }
    }
  }
}

}  // namespace

extern "C" int aptp_ema_many(const AptpEmaParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->items_dev && p->starts_dev, "ema_many: null table");
  APTP_CHECK(p->n_items >= 1 && p->total_blocks >= 1, "ema_many: n_items %d, total_blocks %d", (int)p->n_items, (int)p->total_blocks);
  APTP_CHECK(p->mode == APTP_EMA_UPDATE || p->mode == APTP_EMA_SWAP, "ema_many: mode %d", (int)p->mode);
  APTP_CHECK(p->mode == APTP_EMA_SWAP || p->count_dev, "ema_many: UPDATE needs count_dev");
  APTP_CHECK(p->decay >= 0.f && p->decay <= 1.f, "ema_many: decay outside [0, 1]");
  APTP_CHECK(p->min_decay >= 0.f && p->min_decay <= p->decay, "ema_many: min_decay outside [0, decay]");
  APTP_CHECK(p->update_after_step >= 0, "ema_many: update_after_step %d", (int)p->update_after_step);
  APTP_CHECK(p->inv_gamma > 0.f, "ema_many: inv_gamma must be > 0");
  APTP_CHECK(p->power > 0.f, "ema_many: power must be > 0");
  const EmaK k{p->items_dev, p->starts_dev, p->n_items, p->count_dev, p->gate_dev, p->decay, p->min_decay,
               (float)p->update_after_step, p->inv_gamma, p->power, p->use_warmup != 0, p->cur_decay_dev};
  const dim3 grid((unsigned)p->total_blocks), block(256);
  if (p->mode == APTP_EMA_UPDATE) hipLaunchKernelGGL(ema_many_kernel<APTP_EMA_UPDATE>, grid, block, 0, (hipStream_t)stream, k);
  else hipLaunchKernelGGL(ema_many_kernel<APTP_EMA_SWAP>, grid, block, 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
