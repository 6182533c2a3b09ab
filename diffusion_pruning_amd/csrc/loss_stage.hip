// The loss stage of a training step whose batch may be short (FineTuner.step, pdm/training/trainer.py:1736-1763, behind a loader
// that drops undecodable samples, pdm/utils/data_utils.py:175-179): every term per sample, a 0 / 1 mask over the samples, the mean
// over the samples present -- and all gradients w.r.t. the first operands from ONE launch.
//
//   forward, the three-launch shape of loss_terms.hip:
//   1  partial   a unit is one (term, sample).  Unit u owns aptp_mse_nblocks(rows_per_sample, C) consecutive workgroups and walks
//                its vectors as mse_partial_kernel does with a grid of that size: same stride, same per-thread order, same fold
//   2  finish    one workgroup per unit: mse_finish_kernel over the unit's partials; * inv_n
//   3  combine   one workgroup.  Thread t < n_terms reads valid, w and the unit values of term t from GLOBAL memory (16 terms of
//                1024 samples do not fit the LDS budget of loss_terms.hip) and forms n and its term in sample order; thread 0
//                then forms the groups, the total and n in index order.  n is a sum of 0s and 1s (exact), so every thread has
//                the same n and every value the bits one thread walking all terms would give it
//   backward, one launch: a workgroup belongs to one (gradient item, sample); its coefficients are formed once per workgroup in
//   fp64 from device scalars (g, n = out[G + 1], valid[b], w[b]), so a replayed graph follows the mask without host work
//
// No atomics, no tickets: launch order is the only dependency (loss_ops.hip says why).  Rows of samples that are not valid are
// never multiplied into anything: forward skips their unit values, backward writes their gradient rows as zeros without reading
// the operands.  HBM-bound: every operand is read once per direction, 16 bytes per lane, strided operands where they lie.
#include "aptp_common.h"

namespace {

struct LsTerm {
  const void* a; const void* b;
  int64_t lda, ldb;
  int64_t unit_rows;     // rows of one sample
  int64_t nvec;          // unit_rows * CO
  int32_t CO;            // C / 8
  int32_t nblk;          // workgroups (= partials) per unit
  int32_t a_f32, b_f32, group, weighted;
  float inv_n, scale;
};

struct LsGrad {
  void* grad_out; int64_t ldg;
  int32_t t0, t1;        // t1 = -1: one term
  int32_t nbs;           // workgroups per sample
  int32_t pad;
};

struct LsK {
  LsTerm t[APTP_LOSS_TERMS_MAX];
  LsGrad gr[APTP_LOSS_TERMS_MAX];
  int32_t blk0[APTP_LOSS_TERMS_MAX + 1];     // forward workgroup prefix per term; blk0[n_terms] = total
  int32_t gblk0[APTP_LOSS_TERMS_MAX + 1];    // backward workgroup prefix per gradient item
  int32_t n_terms, n_groups, n_grads, B, total_blocks, sample_term;
  float coef[APTP_LOSS_TERMS_MAX], gdiv[APTP_LOSS_TERMS_MAX];
  const float* valid; const float* w; const float* g;
  float* partial;        // [total_blocks] partials, then [n_terms * B] unit values, term-major
  float* out; float* sample_out;
};

__device__ __forceinline__ void ls_load8(const void* base, int64_t row, int64_t ld, int o, bool f32, float* f) {
  if (f32) {
    const float4* p = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + row * ld + (int64_t)o * 8);
    const float4 x = p[0], y = p[1];
    f[0] = x.x; f[1] = x.y; f[2] = x.z; f[3] = x.w; f[4] = y.x; f[5] = y.y; f[6] = y.z; f[7] = y.w;
  } else {
    const uint4 q = *reinterpret_cast<const uint4*>(reinterpret_cast<const __bf16*>(base) + row * ld + (int64_t)o * 8);
    unpack_bf16x8(q, f);
  }
}

// the loop of mse_partial_kernel with blockIdx.x -> lb, gridDim.x -> nblk and the sample's first row added
template <bool AF32, bool BF32>
__device__ __forceinline__ float ls_accumulate(const void* a, int64_t lda, const void* b, int64_t ldb, int64_t row0, int64_t nvec,
                                               int CO, int lb, int nblk) {
  float acc = 0.f;
  for (int64_t v = (int64_t)lb * 256 + threadIdx.x; v < nvec; v += (int64_t)nblk * 256) {
    const int64_t r = v / CO;
    const int o = (int)(v - r * CO);
    float x[8], y[8];
    ls_load8(a, row0 + r, lda, o, AF32, x);
    ls_load8(b, row0 + r, ldb, o, BF32, y);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float d = x[e] - y[e]; s += d * d; }
    acc += s;
  }
  return acc;
}

__global__ __launch_bounds__(256) void loss_stage_partial_kernel(const LsK p) {
  __shared__ float red[4];
  int t = 0;
  while (t + 1 < p.n_terms && (int)blockIdx.x >= p.blk0[t + 1]) ++t;       // <= 16 entries
  const LsTerm& T = p.t[t];
  const int local = (int)blockIdx.x - p.blk0[t];
  const int unit = local / T.nblk;                                         // the sample
  const int lb = local - unit * T.nblk;
  const int64_t row0 = (int64_t)unit * T.unit_rows;
  float acc;
  if (T.a_f32) {
    acc = T.b_f32 ? ls_accumulate<true, true>(T.a, T.lda, T.b, T.ldb, row0, T.nvec, T.CO, lb, T.nblk)
                  : ls_accumulate<true, false>(T.a, T.lda, T.b, T.ldb, row0, T.nvec, T.CO, lb, T.nblk);
  } else {
    acc = T.b_f32 ? ls_accumulate<false, true>(T.a, T.lda, T.b, T.ldb, row0, T.nvec, T.CO, lb, T.nblk)
                  : ls_accumulate<false, false>(T.a, T.lda, T.b, T.ldb, row0, T.nvec, T.CO, lb, T.nblk);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) p.partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup per unit (blockIdx.x = term * B + sample): mse_finish_kernel over the unit's nblk <= 1024 partials
__global__ __launch_bounds__(256) void loss_stage_finish_kernel(const LsK p) {
  __shared__ float red[256];
  const int u = (int)blockIdx.x;
  const int t = u / p.B;
  const LsTerm& T = p.t[t];
  const float* part = p.partial + p.blk0[t] + (int64_t)(u - t * p.B) * T.nblk;
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

__global__ __launch_bounds__(256) void loss_stage_combine_kernel(const LsK p) {
  __shared__ float tv[APTP_LOSS_TERMS_MAX];
  __shared__ float nv;
  const float* uv = p.partial + p.total_blocks;
  if (p.sample_out) {
    const float* su = uv + (int64_t)p.sample_term * p.B;
    for (int b = threadIdx.x; b < p.B; b += 256) p.sample_out[b] = p.valid[b] != 0.f ? su[b] : 0.f;
  }
  if ((int)threadIdx.x < p.n_terms) {
    const LsTerm& T = p.t[threadIdx.x];
    const float* u = uv + (int64_t)threadIdx.x * p.B;
    float n = 0.f, s = 0.f;
    if (T.weighted) {
#pragma unroll 8
      for (int b = 0; b < p.B; ++b) {
        const float vb = p.valid[b], x = u[b], wb = p.w[b];
        if (vb != 0.f) { n += vb; s += wb * x; }
      }
    } else {
#pragma unroll 8
      for (int b = 0; b < p.B; ++b) {
        const float vb = p.valid[b], x = u[b];
        if (vb != 0.f) { n += vb; s += x; }
      }
    }
    tv[threadIdx.x] = n != 0.f ? s * (1.0f / n) : 0.f;
    if (threadIdx.x == 0) nv = n;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float g[APTP_LOSS_TERMS_MAX];
#pragma unroll
  for (int i = 0; i < APTP_LOSS_TERMS_MAX; ++i) g[i] = 0.f;
  for (int t = 0; t < p.n_terms; ++t) {
    const float v = tv[t] * p.t[t].scale;
#pragma unroll
    for (int i = 0; i < APTP_LOSS_TERMS_MAX; ++i)
      if (i == p.t[t].group) g[i] += v;
  }
  float total = 0.f;
#pragma unroll
  for (int i = 0; i < APTP_LOSS_TERMS_MAX; ++i) {
    if (i < p.n_groups) {
      if (p.gdiv[i] != 0.f) g[i] = g[i] / p.gdiv[i];
      total += p.coef[i] * g[i];
      p.out[i] = g[i];
    }
  }
  p.out[p.n_groups] = total;
  p.out[p.n_groups + 1] = nv;
}

// c_t[b] of the header, g included; fp64 so that the value is rounded once
__device__ __forceinline__ float ls_coef(const LsK& p, int t, int b, double n, double g) {
  const LsTerm& T = p.t[t];
  const double gd = p.gdiv[T.group] != 0.f ? (double)p.gdiv[T.group] : 1.0;
  const double w = T.weighted ? (double)p.w[b] : 1.0;
  const double E = (double)T.unit_rows * (double)T.CO * 8.0;
  return (float)(g * 2.0 * (double)p.coef[T.group] * (double)T.scale * w / (n * E * gd));
}

__global__ __launch_bounds__(256) void loss_stage_bwd_kernel(const LsK p) {
  int i = 0;
  while (i + 1 < p.n_grads && (int)blockIdx.x >= p.gblk0[i + 1]) ++i;
  const LsGrad& G = p.gr[i];
  const LsTerm& T0 = p.t[G.t0];
  const int local = (int)blockIdx.x - p.gblk0[i];
  const int b = local / G.nbs;
  const int lb = local - b * G.nbs;
  const int64_t row0 = (int64_t)b * T0.unit_rows;
  const int CO = T0.CO;
  const bool af32 = T0.a_f32 != 0;
  const float n = p.out[p.n_groups + 1];
  const bool live = n != 0.f && p.valid[b] != 0.f;
  if (!live) {
    // a sample that is not there: zeros, and neither operand is read
    for (int64_t v = (int64_t)lb * 256 + threadIdx.x; v < T0.nvec; v += (int64_t)G.nbs * 256) {
      const int64_t r = v / CO;
      const int o = (int)(v - r * CO);
      if (af32) {
        float4* d = reinterpret_cast<float4*>(reinterpret_cast<float*>(G.grad_out) + (row0 + r) * G.ldg + (int64_t)o * 8);
        d[0] = make_float4(0.f, 0.f, 0.f, 0.f);
        d[1] = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        *reinterpret_cast<uint4*>(reinterpret_cast<__bf16*>(G.grad_out) + (row0 + r) * G.ldg + (int64_t)o * 8) = make_uint4(0u, 0u, 0u, 0u);
      }
    }
    return;
  }
  const double gup = (double)p.g[0];
  const float c0 = ls_coef(p, G.t0, b, (double)n, gup);
  const bool two = G.t1 >= 0;
  const float c1 = two ? ls_coef(p, G.t1, b, (double)n, gup) : 0.f;
  const void* b0 = T0.b;
  const int64_t ldb0 = T0.ldb;
  const bool b0f32 = T0.b_f32 != 0;
  const void* b1 = two ? p.t[G.t1].b : nullptr;
  const int64_t ldb1 = two ? p.t[G.t1].ldb : 0;
  const bool b1f32 = two && p.t[G.t1].b_f32 != 0;
  for (int64_t v = (int64_t)lb * 256 + threadIdx.x; v < T0.nvec; v += (int64_t)G.nbs * 256) {
    const int64_t r = v / CO;
    const int o = (int)(v - r * CO);
    float x[8], y[8];
    ls_load8(T0.a, row0 + r, T0.lda, o, af32, x);
    ls_load8(b0, row0 + r, ldb0, o, b0f32, y);
    if (two) {
      float z[8];
      ls_load8(b1, row0 + r, ldb1, o, b1f32, z);
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = c0 * (x[e] - y[e]) + c1 * (x[e] - z[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = c0 * (x[e] - y[e]);
    }
    if (af32) {
      float4* d = reinterpret_cast<float4*>(reinterpret_cast<float*>(G.grad_out) + (row0 + r) * G.ldg + (int64_t)o * 8);
      d[0] = make_float4(x[0], x[1], x[2], x[3]);
      d[1] = make_float4(x[4], x[5], x[6], x[7]);
    } else {
      *reinterpret_cast<uint4*>(reinterpret_cast<__bf16*>(G.grad_out) + (row0 + r) * G.ldg + (int64_t)o * 8) = pack_bf16x8(x);
    }
  }
}

constexpr int BWD_VEC_PER_BLOCK = 1024;     // 4 vectors per thread before a sample gets another workgroup
constexpr int BWD_MAX_NBS = 64;

// validates the table and lays out units and workgroups; with `quiet` a bad table gives false without touching the error string
bool ls_plan(const AptpLossStageParams* p, LsK* k, bool quiet, bool bwd) {
#define LS_REQUIRE(cond, ...)                  \
  do {                                         \
    if (!(cond)) {                             \
      if (!quiet) aptp_set_error(__VA_ARGS__); \
      return false;                            \
    }                                          \
  } while (0)
  LS_REQUIRE(p, "loss_stage: null parameter block");
  LS_REQUIRE(p->n_terms >= 1 && p->n_terms <= APTP_LOSS_TERMS_MAX, "loss_stage: n_terms must be 1..%d (got %d)", APTP_LOSS_TERMS_MAX, p->n_terms);
  LS_REQUIRE(p->n_groups >= 1 && p->n_groups <= APTP_LOSS_TERMS_MAX, "loss_stage: n_groups must be 1..%d (got %d)", APTP_LOSS_TERMS_MAX, p->n_groups);
  int64_t blocks = 0, B = 0;
  int sample_term = -1;
  for (int i = 0; i < p->n_terms; ++i) {
    const AptpLossStageTerm& s = p->terms[i];
    LsTerm& T = k->t[i];
    LS_REQUIRE(s.a && s.b, "loss_stage: term %d: null operand", i);
    LS_REQUIRE(s.rows > 0 && s.C > 0 && s.C % 8 == 0, "loss_stage: term %d: C must be a positive multiple of 8 (got %d)", i, s.C);
    LS_REQUIRE(s.lda >= s.C && s.ldb >= s.C && s.lda % 8 == 0 && s.ldb % 8 == 0,
               "loss_stage: term %d: leading dimensions (multiples of 8, >= C)", i);
    LS_REQUIRE(((uintptr_t)s.a & 15) == 0 && ((uintptr_t)s.b & 15) == 0, "loss_stage: term %d: operands must be 16-byte aligned", i);
    LS_REQUIRE(s.group >= 0 && s.group < p->n_groups, "loss_stage: term %d: group %d of %d", i, s.group, p->n_groups);
    LS_REQUIRE(s.rows_per_sample > 0 && s.rows % s.rows_per_sample == 0,
               "loss_stage: term %d: rows %lld is no positive multiple of rows_per_sample %lld", i, (long long)s.rows,
               (long long)s.rows_per_sample);
    const int64_t Bi = s.rows / s.rows_per_sample;
    LS_REQUIRE(Bi <= APTP_LOSS_STAGE_MAX_B, "loss_stage: term %d: more than %d samples", i, APTP_LOSS_STAGE_MAX_B);
    LS_REQUIRE(i == 0 || Bi == B, "loss_stage: term %d has %lld samples, term 0 has %lld: B differs", i, (long long)Bi, (long long)B);
    B = Bi;
    LS_REQUIRE(!s.weighted || p->w, "loss_stage: term %d is weighted and w is null", i);
    LS_REQUIRE(s.rows_per_sample * (int64_t)(s.C / 8) < ((int64_t)1 << 40), "loss_stage: term %d: sample too large", i);
    if (s.weighted && sample_term < 0) sample_term = i;
    T.a = s.a; T.b = s.b; T.lda = s.lda; T.ldb = s.ldb;
    T.a_f32 = s.a_f32 != 0; T.b_f32 = s.b_f32 != 0; T.group = s.group; T.scale = s.scale; T.weighted = s.weighted != 0;
    T.unit_rows = s.rows_per_sample;
    T.CO = s.C / 8;
    T.nvec = T.unit_rows * T.CO;
    T.nblk = aptp_mse_nblocks(T.unit_rows, s.C);
    T.inv_n = 1.0f / ((float)T.unit_rows * (float)s.C);
    k->blk0[i] = (int32_t)blocks;
    blocks += (int64_t)T.nblk * B;
  }
  LS_REQUIRE(p->valid, "loss_stage: valid is null");
  k->blk0[p->n_terms] = (int32_t)blocks;
  k->n_terms = p->n_terms; k->n_groups = p->n_groups; k->B = (int32_t)B; k->total_blocks = (int32_t)blocks;
  k->sample_term = sample_term < 0 ? 0 : sample_term;
  k->n_grads = 0;
  if (!bwd) return true;
  LS_REQUIRE(p->n_grads >= 1 && p->n_grads <= APTP_LOSS_TERMS_MAX, "loss_stage: n_grads must be 1..%d (got %d)", APTP_LOSS_TERMS_MAX, p->n_grads);
  int64_t gblocks = 0;
  for (int i = 0; i < p->n_grads; ++i) {
    const AptpLossStageGrad& s = p->grads[i];
    LsGrad& G = k->gr[i];
    LS_REQUIRE(s.term0 >= 0 && s.term0 < p->n_terms && s.term1 >= -1 && s.term1 < p->n_terms && s.term1 != s.term0,
               "loss_stage: gradient %d: term index (%d, %d) of %d", i, s.term0, s.term1, p->n_terms);
    const AptpLossStageTerm& t0 = p->terms[s.term0];
    if (s.term1 >= 0) {
      const AptpLossStageTerm& t1 = p->terms[s.term1];
      LS_REQUIRE(t1.a == t0.a && t1.lda == t0.lda && t1.rows == t0.rows && t1.rows_per_sample == t0.rows_per_sample && t1.C == t0.C &&
                     (t1.a_f32 != 0) == (t0.a_f32 != 0),
                 "loss_stage: gradient %d: terms %d and %d have different first operands", i, s.term0, s.term1);
    }
    const int64_t ldg = s.ldg ? s.ldg : t0.lda;
    LS_REQUIRE(s.grad_out && ((uintptr_t)s.grad_out & 15) == 0, "loss_stage: gradient %d: grad_out must be 16-byte aligned and not null", i);
    LS_REQUIRE(ldg >= t0.C && ldg % 8 == 0, "loss_stage: gradient %d: leading dimension (multiple of 8, >= C)", i);
    const int64_t nvec = t0.rows_per_sample * (int64_t)(t0.C / 8);
    int64_t nbs = (nvec + BWD_VEC_PER_BLOCK - 1) / BWD_VEC_PER_BLOCK;
    nbs = nbs < 1 ? 1 : (nbs > BWD_MAX_NBS ? BWD_MAX_NBS : nbs);
    G.grad_out = s.grad_out; G.ldg = ldg; G.t0 = s.term0; G.t1 = s.term1; G.nbs = (int32_t)nbs; G.pad = 0;
    k->gblk0[i] = (int32_t)gblocks;
    gblocks += nbs * B;
  }
  k->gblk0[p->n_grads] = (int32_t)gblocks;
  k->n_grads = p->n_grads;
  return true;
#undef LS_REQUIRE
}

void ls_fill(const AptpLossStageParams* p, LsK* k) {
  for (int i = 0; i < APTP_LOSS_TERMS_MAX; ++i) { k->coef[i] = p->group_coef[i]; k->gdiv[i] = p->group_div[i]; }
  k->valid = p->valid; k->w = p->w; k->g = p->g; k->partial = p->partial; k->out = p->out; k->sample_out = p->sample_out;
}

}  // namespace

extern "C" int aptp_loss_stage_nblocks(const AptpLossStageParams* p) {
  LsK k = {};
  return ls_plan(p, &k, true, false) ? k.total_blocks : 0;
}

extern "C" int aptp_loss_stage_scratch_floats(const AptpLossStageParams* p) {
  LsK k = {};
  return ls_plan(p, &k, true, false) ? k.total_blocks + k.n_terms * k.B : 0;
}

extern "C" int aptp_loss_stage_bwd_nblocks(const AptpLossStageParams* p) {
  LsK k = {};
  return ls_plan(p, &k, true, true) ? k.gblk0[k.n_grads] : 0;
}

extern "C" int aptp_loss_stage(const AptpLossStageParams* p, aptp_stream_t stream) {
  LsK k = {};
  if (!ls_plan(p, &k, false, false)) return APTP_EINVAL;
  APTP_CHECK(p->partial && p->out, "loss_stage: partial / out");
  ls_fill(p, &k);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(loss_stage_partial_kernel, dim3(k.total_blocks), dim3(256), 0, s, k);
  hipLaunchKernelGGL(loss_stage_finish_kernel, dim3(k.n_terms * k.B), dim3(256), 0, s, k);
  hipLaunchKernelGGL(loss_stage_combine_kernel, dim3(1), dim3(256), 0, s, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}

extern "C" int aptp_loss_stage_bwd(const AptpLossStageParams* p, aptp_stream_t stream) {
  LsK k = {};
  if (!ls_plan(p, &k, false, true)) return APTP_EINVAL;
  APTP_CHECK(p->out && p->g, "loss_stage: backward needs out (n = out[G + 1], written by aptp_loss_stage) and g");
  ls_fill(p, &k);
  hipLaunchKernelGGL(loss_stage_bwd_kernel, dim3(k.gblk0[k.n_grads]), dim3(256), 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
