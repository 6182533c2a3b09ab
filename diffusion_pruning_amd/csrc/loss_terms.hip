// All loss terms of one validation step in three launches (Pruner.validate / FineTuner.validate, pdm/training/trainer.py:1026-1095,
// 1767-1818): the min-SNR weighted diffusion term, the output-distillation term and the nine block terms, their weighted sum,
// and running totals over the batches of a validation run -- kept on the device, read by the host once per run.
//
//   1  partial   a "unit" is an unweighted term or one sample of the weighted term.  Unit u owns aptp_mse_nblocks(unit rows, C)
//                consecutive workgroups and, inside that range, walks its vectors exactly as mse_partial_kernel does with a grid
//                of that size: same grid stride, same per-thread order, same in-block fold
//   2  finish    one workgroup per unit: thread t sums the unit's partials t, t + 256, ..; the fixed tree; * inv_n
//   3  combine   one workgroup; thread 0 forms the weighted term, the groups, the total and the running totals in index order
//
// So a unit's value has the bits aptp_mse gives the same view (tests/test_loss_terms_gpu.py), and the validation losses are the
// training step's losses on the same tensors.  As in loss_ops.hip there is no atomic, no ticket and no cross-workgroup protocol
// (its header says why: replayed next to other graphs such reductions returned wrong sums); launch order is the only dependency.
// HBM-bound: every operand is read once, 16 bytes per lane, and nothing but a few hundred floats is written.
#include "aptp_common.h"

namespace {

constexpr int MAX_UNITS = 1024;      // staged in LDS by the combine launch

struct LtTerm {
  const void* a; const void* b;
  int64_t lda, ldb;
  int64_t unit_rows;     // rows of one unit
  int64_t nvec;          // unit_rows * CO
  int32_t CO;            // C / 8
  int32_t nblk;          // workgroups (= partials) per unit
  int32_t unit0;         // first unit of this term
  int32_t n_units;       // 1, or the B samples of the weighted term
  int32_t a_f32, b_f32, group, weighted;
  float inv_n, scale;
};

struct LtK {
  LtTerm t[APTP_LOSS_TERMS_MAX];
  int32_t blk0[APTP_LOSS_TERMS_MAX + 1];     // block prefix per term (host-computed); blk0[n_terms] = total
  int32_t n_terms, n_groups, n_units, total_blocks;
  float coef[APTP_LOSS_TERMS_MAX], gdiv[APTP_LOSS_TERMS_MAX];
  const float* w;
  float* partial;        // [total_blocks] partials, then [n_units] unit values
  float* out; float* sample_out; float* running;
};

template <bool F32>
__device__ __forceinline__ void lt_load8(const void* base, int64_t row, int64_t ld, int o, float* f) {
  if (F32) {
    const float4* p = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + row * ld + (int64_t)o * 8);
    const float4 x = p[0], y = p[1];
    f[0] = x.x; f[1] = x.y; f[2] = x.z; f[3] = x.w; f[4] = y.x; f[5] = y.y; f[6] = y.z; f[7] = y.w;
  } else {
    const uint4 q = *reinterpret_cast<const uint4*>(reinterpret_cast<const __bf16*>(base) + row * ld + (int64_t)o * 8);
    unpack_bf16x8(q, f);
  }
}

// the loop of mse_partial_kernel with blockIdx.x -> lb, gridDim.x -> nblk and the unit's first row added
template <bool AF32, bool BF32>
__device__ __forceinline__ float lt_accumulate(const void* a, int64_t lda, const void* b, int64_t ldb, int64_t row0, int64_t nvec,
                                               int CO, int lb, int nblk) {
  float acc = 0.f;
  for (int64_t v = (int64_t)lb * 256 + threadIdx.x; v < nvec; v += (int64_t)nblk * 256) {
    const int64_t r = v / CO;
    const int o = (int)(v - r * CO);
    float x[8], y[8];
    lt_load8<AF32>(a, row0 + r, lda, o, x);
    lt_load8<BF32>(b, row0 + r, ldb, o, y);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float d = x[e] - y[e]; s += d * d; }
    acc += s;
  }
  return acc;
}

__global__ __launch_bounds__(256) void loss_terms_partial_kernel(const LtK p) {
  __shared__ float red[4];
  int t = 0;
  while (t + 1 < p.n_terms && (int)blockIdx.x >= p.blk0[t + 1]) ++t;       // <= 16 entries
  const LtTerm& T = p.t[t];
  const int local = (int)blockIdx.x - p.blk0[t];
  const int unit = local / T.nblk;
  const int lb = local - unit * T.nblk;
  const int64_t row0 = (int64_t)unit * T.unit_rows;
  float acc;
  if (T.a_f32) {
    acc = T.b_f32 ? lt_accumulate<true, true>(T.a, T.lda, T.b, T.ldb, row0, T.nvec, T.CO, lb, T.nblk)
                  : lt_accumulate<true, false>(T.a, T.lda, T.b, T.ldb, row0, T.nvec, T.CO, lb, T.nblk);
  } else {
    acc = T.b_f32 ? lt_accumulate<false, true>(T.a, T.lda, T.b, T.ldb, row0, T.nvec, T.CO, lb, T.nblk)
                  : lt_accumulate<false, false>(T.a, T.lda, T.b, T.ldb, row0, T.nvec, T.CO, lb, T.nblk);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) p.partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup per unit: mse_finish_kernel over the unit's nblk <= 1024 partials
__global__ __launch_bounds__(256) void loss_terms_finish_kernel(const LtK p) {
  __shared__ float red[256];
  const int u = (int)blockIdx.x;
  int t = 0;
  while (t + 1 < p.n_terms && u >= p.t[t + 1].unit0) ++t;
  const LtTerm& T = p.t[t];
  const float* part = p.partial + p.blk0[t] + (int64_t)(u - T.unit0) * T.nblk;
  float a = 0.f;
  for (int i = threadIdx.x; i < T.nblk; i += 256) a += part[i];
  red[threadIdx.x] = a;
  __syncthreads();
#pragma unroll
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) p.partial[p.total_blocks + u] = red[0] * T.inv_n;
}

// one workgroup: the unit values (and the sample weights) go through LDS, then thread 0 adds everything up in index order
__global__ __launch_bounds__(256) void loss_terms_combine_kernel(const LtK p) {
  __shared__ float val[MAX_UNITS];
  __shared__ float sw[MAX_UNITS];
  const float* uv = p.partial + p.total_blocks;
  for (int u = threadIdx.x; u < p.n_units; u += 256) val[u] = uv[u];
  for (int t = 0; t < p.n_terms; ++t) {
    const LtTerm& T = p.t[t];
    if (!T.weighted) continue;
    for (int b = threadIdx.x; b < T.n_units; b += 256) {
      sw[b] = p.w[b];
      if (p.sample_out) p.sample_out[b] = uv[T.unit0 + b];
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float g[APTP_LOSS_TERMS_MAX];
#pragma unroll
  for (int i = 0; i < APTP_LOSS_TERMS_MAX; ++i) g[i] = 0.f;
  for (int t = 0; t < p.n_terms; ++t) {
    const LtTerm& T = p.t[t];
    float v;
    if (T.weighted) {
      v = 0.f;
      for (int b = 0; b < T.n_units; ++b) v += sw[b] * val[T.unit0 + b];
      v *= 1.0f / (float)T.n_units;
    } else {
      v = val[T.unit0];
    }
#pragma unroll
    for (int i = 0; i < APTP_LOSS_TERMS_MAX; ++i)
      if (i == T.group) g[i] += v * T.scale;
  }
  float total = 0.f;
#pragma unroll
  for (int i = 0; i < APTP_LOSS_TERMS_MAX; ++i) {
    if (i < p.n_groups) {
      if (p.gdiv[i] != 0.f) g[i] = g[i] / p.gdiv[i];
      total += p.coef[i] * g[i];
      p.out[i] = g[i];
      if (p.running) p.running[i] += g[i];
    }
  }
  p.out[p.n_groups] = total;
  if (p.running) {
    p.running[p.n_groups] += total;
    p.running[p.n_groups + 1] += 1.0f;
  }
}

// validates the table and lays out units and workgroups; with `quiet` a bad table gives false without touching the error string
bool lt_plan(const AptpLossTermsParams* p, LtK* k, bool quiet) {
#define LT_REQUIRE(cond, ...)                 \
  do {                                        \
    if (!(cond)) {                            \
      if (!quiet) aptp_set_error(__VA_ARGS__); \
      return false;                           \
    }                                         \
  } while (0)
  LT_REQUIRE(p, "loss_terms: null parameter block");
  LT_REQUIRE(p->n_terms >= 1 && p->n_terms <= APTP_LOSS_TERMS_MAX, "loss_terms: n_terms must be 1..%d (got %d)", APTP_LOSS_TERMS_MAX, p->n_terms);
  LT_REQUIRE(p->n_groups >= 1 && p->n_groups <= APTP_LOSS_TERMS_MAX, "loss_terms: n_groups must be 1..%d (got %d)", APTP_LOSS_TERMS_MAX, p->n_groups);
  int64_t blocks = 0;
  int units = 0, weighted = 0;
  for (int i = 0; i < p->n_terms; ++i) {
    const AptpLossTerm& s = p->terms[i];
    LtTerm& T = k->t[i];
    LT_REQUIRE(s.a && s.b, "loss_terms: term %d: null operand", i);
    LT_REQUIRE(s.rows > 0 && s.C > 0 && s.C % 8 == 0, "loss_terms: term %d: C must be a positive multiple of 8 (got %d)", i, s.C);
    LT_REQUIRE(s.lda >= s.C && s.ldb >= s.C && s.lda % 8 == 0 && s.ldb % 8 == 0,
               "loss_terms: term %d: leading dimensions (multiples of 8, >= C)", i);
    LT_REQUIRE(((uintptr_t)s.a & 15) == 0 && ((uintptr_t)s.b & 15) == 0, "loss_terms: term %d: operands must be 16-byte aligned", i);
    LT_REQUIRE(s.group >= 0 && s.group < p->n_groups, "loss_terms: term %d: group %d of %d", i, s.group, p->n_groups);
    LT_REQUIRE(s.rows_per_sample >= 0, "loss_terms: term %d: rows_per_sample", i);
    T.a = s.a; T.b = s.b; T.lda = s.lda; T.ldb = s.ldb;
    T.a_f32 = s.a_f32 != 0; T.b_f32 = s.b_f32 != 0; T.group = s.group; T.scale = s.scale;
    T.weighted = s.rows_per_sample > 0;
    T.unit_rows = s.rows;
    T.n_units = 1;
    if (T.weighted) {
      LT_REQUIRE(s.rows % s.rows_per_sample == 0, "loss_terms: term %d: rows %lld is no multiple of rows_per_sample %lld", i,
                 (long long)s.rows, (long long)s.rows_per_sample);
      LT_REQUIRE(p->w, "loss_terms: term %d is weighted and w is null", i);
      LT_REQUIRE(++weighted == 1, "loss_terms: at most one weighted term");
      LT_REQUIRE(s.rows / s.rows_per_sample <= MAX_UNITS - APTP_LOSS_TERMS_MAX, "loss_terms: term %d: more than %d samples", i,
                 MAX_UNITS - APTP_LOSS_TERMS_MAX);
      T.unit_rows = s.rows_per_sample;
      T.n_units = (int32_t)(s.rows / s.rows_per_sample);
    }
    T.CO = s.C / 8;
    T.nvec = T.unit_rows * T.CO;
    T.nblk = aptp_mse_nblocks(T.unit_rows, s.C);
    T.inv_n = 1.0f / ((float)T.unit_rows * (float)s.C);
    T.unit0 = units;
    k->blk0[i] = (int32_t)blocks;
    units += T.n_units;
    blocks += (int64_t)T.nblk * T.n_units;
  }
  k->blk0[p->n_terms] = (int32_t)blocks;
  k->n_terms = p->n_terms; k->n_groups = p->n_groups; k->n_units = units; k->total_blocks = (int32_t)blocks;
  return true;
#undef LT_REQUIRE
}

}  // namespace

extern "C" int aptp_loss_terms_nblocks(const AptpLossTermsParams* p) {
  LtK k = {};
  return lt_plan(p, &k, true) ? k.total_blocks : 0;
}

extern "C" int aptp_loss_terms_scratch_floats(const AptpLossTermsParams* p) {
  LtK k = {};
  return lt_plan(p, &k, true) ? k.total_blocks + k.n_units : 0;
}

extern "C" int aptp_loss_terms(const AptpLossTermsParams* p, aptp_stream_t stream) {
  LtK k = {};
  if (!lt_plan(p, &k, false)) return APTP_EINVAL;
  APTP_CHECK(p->partial && p->out, "loss_terms: partial / out");
  for (int i = 0; i < APTP_LOSS_TERMS_MAX; ++i) { k.coef[i] = p->group_coef[i]; k.gdiv[i] = p->group_div[i]; }
  k.w = p->w; k.partial = p->partial; k.out = p->out; k.sample_out = p->sample_out; k.running = p->running;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(loss_terms_partial_kernel, dim3(k.total_blocks), dim3(256), 0, s, k);
  hipLaunchKernelGGL(loss_terms_finish_kernel, dim3(k.n_units), dim3(256), 0, s, k);
  hipLaunchKernelGGL(loss_terms_combine_kernel, dim3(1), dim3(256), 0, s, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
