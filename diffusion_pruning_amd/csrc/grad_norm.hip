// Global L2 norm of the gradients of a packed-pass table and the clip coefficient of torch.nn.utils.clip_grad_norm_
// (max_grad_norm of the diffusers training scripts), left in DEVICE memory where the AdamW passes of optim.hip and
// router_optim.hip read it (their grad_scale_dev): the gradients are never rewritten, a captured step clips with no
// host round trip, and the norm is there to report.  4 B read per element, HBM-bound.  DESIGN 6t.
//
// Two launches, no atomics; no block reads what another block of the same grid writes (router_optim.hip's rule).
// THE SUMMATION ORDER IS PART OF THE CONTRACT (tests/grad_norm_model.py restates it; every replay gives the same bits):
//   partial   grid = total_blocks, 256 threads; block b belongs to item `lo` (packed_pass.h: item_of_block) and covers its
//             elements base .. base + 4096, base = (b - starts[lo]) * 4096.  Thread t starts s = 0.0 (fp64) and, for trip
//             i = 0, 1, 2, 3 with e = base + (i * 256 + t) * 4: a whole quad (e + 3 < n) adds g[e]^2, g[e+1]^2, g[e+2]^2, g[e+3]^2 in
//             that order, else the elements e .. min(n, e + 4) in index order.  Every product is (double)g * (double)g -- exact,
//             so contraction to an FMA changes no bit -- and every sum is one fp64 addition.
//   block sum inside each wave of 64 a butterfly: for off = 32, 16, 8, 4, 2, 1: s = s + (s of lane ^ off); the four wave sums w0..w3 go
//             through LDS and thread 0 forms ((w0 + w1) + w2) + w3 = partials[b].
//   finalise  one block of 256 threads: thread j starts s = 0.0 and adds partials[j], partials[j + 256], ... in that order; the block
//             sum as above gives S.  Thread 0, in fp64:
//               total = sqrt(S) * grad_scale                      (grad_scale widened from fp32; 0 = 1)
//               r     = max_norm / (total + 1e-6)                 (torch's formula; max_norm widened from fp32)
//               coef  = 1 unless r < 1 (so also for a null max_norm_dev, +inf or NaN), else max(r, 0); rounded to fp32
//               the verdict is finite iff (float)total and the gate (when given) are: then verdict = (float)total, else NaN and
//               coef = 1.0f (no optimizer multiplies by NaN if a caller forgets the gate)
//               clipped_count += 1 when the verdict is finite and the fp32 coef < 1
//             and writes out = {(float)total, coef, verdict, clipped_count} with one 16-byte store.
#include "packed_pass.h"

using namespace packed_pass;

namespace {

struct GradNormK {
  const AptpGradNormItem* items; const int32_t* starts; int n_items, total_blocks;
  double* partials;
  float gscale;
  const float* max_norm;
  const float* gate;
  float* out;
};

// the fixed tree of both kernels; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double s, double* wave_sums) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_xor(s, off);
  if ((threadIdx.x & (APTP_WAVE - 1)) == 0) wave_sums[threadIdx.x / APTP_WAVE] = s;
  __syncthreads();
  return ((wave_sums[0] + wave_sums[1]) + wave_sums[2]) + wave_sums[3];
}

__device__ __forceinline__ void add_square(double& s, float g) { s = s + (double)g * (double)g; }

__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const GradNormK k) {
  __shared__ double wave_sums[THREADS / APTP_WAVE];
  const int b = blockIdx.x;
  const int lo = item_of_block(k.starts, k.n_items, b);
  const AptpGradNormItem it = k.items[lo];
  const int64_t base = (int64_t)(b - k.starts[lo]) * ELEMS_PER_BLOCK;
  // the four loads go out before the first product; a trip without a whole quad contributes zeros here (s + 0.0 is s) and its
  // elements through the scalar tail below, in the trip's own place
  float4 q[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t e = base + ((int64_t)i * THREADS + threadIdx.x) * 4;
    q[i] = whole_quad(e, it.n) ? *reinterpret_cast<const float4*>(it.g + e) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t e = base + ((int64_t)i * THREADS + threadIdx.x) * 4;
    if (whole_quad(e, it.n)) {
      add_square(s, q[i].x); add_square(s, q[i].y); add_square(s, q[i].z); add_square(s, q[i].w);
    } else {
      for (int64_t x = e; x < it.n && x < e + 4; ++x) add_square(s, it.g[x]);
    }
  }
  s = block_sum(s, wave_sums);
  if (threadIdx.x == 0) k.partials[b] = s;
}

__global__ __launch_bounds__(256) void grad_norm_finalise_kernel(const GradNormK k) {
  __shared__ double wave_sums[THREADS / APTP_WAVE];
  double s = 0.0;
  // the adds are one dependent chain in the contract's order; the loads are not: eight go out before their adds (an SD-2.1 expert
  // has ~1.2e5 partials, ~480 per thread, and one load's latency per add is what this kernel would otherwise cost)
  int j = threadIdx.x;
  for (; j < k.total_blocks - 7 * THREADS; j += 8 * THREADS) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = k.partials[j + u * THREADS];
#pragma unroll
    for (int u = 0; u < 8; ++u) s = s + v[u];
  }
  for (; j < k.total_blocks; j += THREADS) s = s + k.partials[j];
  s = block_sum(s, wave_sums);
  if (threadIdx.x != 0) return;
  const double total = sqrt(s) * (double)k.gscale;
  const float total_f = (float)total;
  float coef = 1.0f;
  if (k.max_norm) {
    const double r = (double)k.max_norm[0] / (total + 1e-6);
    if (r < 1.0) coef = (float)(r < 0.0 ? 0.0 : r);
  }
  const bool finite = !non_finite(total_f) && !(k.gate && non_finite(k.gate[0]));
  float clipped = k.out[3];
  if (!finite) coef = 1.0f;
  else if (coef < 1.0f) clipped = clipped + 1.0f;
  *reinterpret_cast<float4*>(k.out) = make_float4(total_f, coef, finite ? total_f : __builtin_nanf(""), clipped);
}

}  // namespace

extern "C" int aptp_grad_norm_blocks(int64_t n) { return blocks_of(n); }

extern "C" int aptp_grad_norm(const AptpGradNormParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->items_dev && p->starts_dev && p->partials_dev && p->out_dev, "grad_norm: null pointer");
  APTP_CHECK(p->n_items >= 1 && p->total_blocks >= 1, "grad_norm: n_items and total_blocks must be >= 1");
  APTP_CHECK(p->grad_scale >= 0.f, "grad_norm: grad_scale");
  APTP_CHECK(((uintptr_t)p->items_dev & 7) == 0 && ((uintptr_t)p->starts_dev & 3) == 0 && ((uintptr_t)p->partials_dev & 7) == 0 &&
             ((uintptr_t)p->out_dev & 15) == 0 && ((uintptr_t)p->max_norm_dev & 3) == 0 && ((uintptr_t)p->gate_dev & 3) == 0,
             "grad_norm: misaligned table, partials_dev (8 bytes), out_dev (16 bytes), max_norm_dev or gate_dev");
  GradNormK k{p->items_dev, p->starts_dev, p->n_items, p->total_blocks, p->partials_dev, p->grad_scale == 0.f ? 1.0f : p->grad_scale,
              p->max_norm_dev, p->gate_dev, p->out_dev};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(grad_norm_partial_kernel, dim3((unsigned)p->total_blocks), dim3(THREADS), 0, s, k);
  hipLaunchKernelGGL(grad_norm_finalise_kernel, dim3(1), dim3(THREADS), 0, s, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
