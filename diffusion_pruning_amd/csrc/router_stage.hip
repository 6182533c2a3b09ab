// The router's batch-coupled stage for a pruning step whose batch may be short (Pruner.step, pdm/training/trainer.py:1129-1249,
// behind a loader that drops undecodable samples, pdm/utils/data_utils.py:175-179): the Sinkhorn assignment of the quantiser
// (pdm/models/vq/quantizer.py:263-340), the contrastive loss (pdm/losses/contrastive_loss.py:5-22) and the three MAC losses
// (trainer.py:1227-1238), each over the samples PRESENT, with a 0 / 1 mask read from device memory at launch time.
//
//   aptp_sinkhorn_assign, one launch of one workgroup: Q lives in global memory ([B, K], 256 KB at the largest size: more than the
//        LDS), every pass is "one thread per sample walks its K entries" or "column sums over the samples" with a barrier between
//   aptp_router_stage, three launches:
//   1  unit     one workgroup per sample: the two row norms, the normalised rows Â_i and Ẑ_i
//   2  row      one workgroup per sample i: the two Gram rows over V (a wave per j, lanes over the features, the own row in LDS),
//               both row softmaxes, P_i. and T_i. for the backward, and the row's part of the BCE sum
//   3  combine  one workgroup: n, the contrastive mean, mean / max / unbiased std of the ratios, the resource term, the total
//   aptp_router_stage_bwd, two launches:
//   1  dscore   one workgroup per sample i: BCE backward and the row-softmax backward -> dS_i.
//   2  darch    one workgroup per sample i: dÂ_i = sum_j (dS_ij + dS_ji) Â_j / tau (tau folded into dS), the normalisation's
//               backward, and d_ratios[i]
//
// No atomics, no tickets: launch order is the only dependency, every sum has one fixed order (a thread's strided walk, the
// 64-lane shuffle fold, the four waves in index order).  A sample that is not valid is SKIPPED -- its workgroup returns, its
// index is never a j -- so what its rows hold reaches no output; the backward writes its gradient rows as zeros without reading
// the operands.  Latency-bound at the design point (B <= 128, K = 8, E = 1634, D = 768): plain fp32 loads, nothing vectorised.
#include "aptp_common.h"

namespace {

constexpr int NT = 256;
constexpr int FEAT_MAX = APTP_ROUTER_STAGE_MAX_FEATURES;
constexpr int PER_THREAD = FEAT_MAX / NT;

// sum over the workgroup in a fixed order; every thread gets the value.  red: 4 floats of LDS, reusable right after the call
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// the same for the few fp64 sums of the combine launch: a tree over 256 LDS slots, one fixed order
__device__ __forceinline__ double block_sum_f64(double v, double* buf) {
  __syncthreads();
  buf[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) buf[threadIdx.x] += buf[threadIdx.x + w];
    __syncthreads();
  }
  return buf[0];
}

__device__ __forceinline__ float block_max(float v, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// ---- (a) the masked Sinkhorn assignment ----------------------------------------------------------------------------------
struct SkK {
  const float* scores; int64_t ld;
  const float* valid; int64_t* idx; float* q;
  int32_t B, K, iters;
  float eps;
};

// first maximum of K values; a NaN counts as the maximum (torch.argmax)
__device__ __forceinline__ int first_argmax(const float* row, int K) {
  float best = row[0];
  int at = 0;
  for (int k = 1; k < K; ++k) {
    const float v = row[k];
    if (v > best || (v != v && best == best)) { best = v; at = k; }
  }
  return at;
}

// col[k] = sum over the valid samples of q[b][k], in one fixed order: thread (k, sub) walks b = sub, sub + nsub, ..; the nsub
// partials of a column are added in index order
__device__ __forceinline__ void column_sums(const SkK& p, int KP, float* part, float* col) {
  const int k = (int)threadIdx.x % KP, sub = (int)threadIdx.x / KP, nsub = NT / KP;
  __syncthreads();                                       // the rows other threads wrote in the pass before
  float a = 0.f;
  if (k < p.K)
    for (int b = sub; b < p.B; b += nsub)
      if (p.valid[b] != 0.f) a += p.q[(int64_t)b * p.K + k];
  part[threadIdx.x] = a;
  __syncthreads();
  if (sub == 0 && k < p.K) {
    float s = 0.f;
    for (int i = 0; i < nsub; ++i) s += part[i * KP + k];
    col[k] = s;
  }
  __syncthreads();
}

__global__ __launch_bounds__(NT) void sinkhorn_assign_kernel(const SkK p) {
  __shared__ float part[NT];
  __shared__ float col[APTP_SINKHORN_MAX_K];
  __shared__ float red[4];
  const int K = p.K;
  int KP = 1;
  while (KP < K) KP <<= 1;
  float cnt = 0.f;
  for (int b = threadIdx.x; b < p.B; b += NT) {
    const float vb = p.valid[b];
    if (vb != 0.f) {
      cnt += vb;
      for (int k = 0; k < K; ++k) p.q[(int64_t)b * K + k] = expf(p.scores[(int64_t)b * p.ld + k] / p.eps);
    }
  }
  const float n = block_sum(cnt, red);                   // a sum of 0s and 1s: exact in any order
  if (n != 0.f) {
    column_sums(p, KP, part, col);
    float total = 0.f;
    for (int k = 0; k < K; ++k) total += col[k];
    for (int b = threadIdx.x; b < p.B; b += NT)
      if (p.valid[b] != 0.f)
        for (int k = 0; k < K; ++k) p.q[(int64_t)b * K + k] /= total;
    for (int it = 0; it < p.iters; ++it) {
      column_sums(p, KP, part, col);
      for (int b = threadIdx.x; b < p.B; b += NT) {
        if (p.valid[b] == 0.f) continue;
        float* row = p.q + (int64_t)b * K;
        float s = 0.f;
        for (int k = 0; k < K; ++k) {
          const float v = row[k] / col[k] / (float)K;
          row[k] = v;
          s += v;
        }
        for (int k = 0; k < K; ++k) row[k] = row[k] / s / n;
      }
    }
  }
  // every thread finishes the samples it owned in the passes above: no barrier needed before the last pass
  for (int b = threadIdx.x; b < p.B; b += NT) {
    float* row = p.q + (int64_t)b * K;
    if (n != 0.f && p.valid[b] != 0.f) {
      for (int k = 0; k < K; ++k) row[k] *= n;
      p.idx[b] = first_argmax(row, K);
    } else {
      // not there: the argmax of its own raw scores (the quantiser's eval branch), and its Q row is zeros
      p.idx[b] = first_argmax(p.scores + (int64_t)b * p.ld, K);
      for (int k = 0; k < K; ++k) row[k] = 0.f;
    }
  }
}

// ---- (b) the masked router stage ---------------------------------------------------------------------------------------------
struct RsK {
  const float* text; int64_t ld_text;
  const float* arch; int64_t ld_arch;
  const float* ratios; const float* valid; const float* g;
  float* ahat; float* zhat;        // [B, E], [B, D]
  float* P; float* T; float* dS;   // [B, B] each; only V x V is written or read
  float* na; float* rowloss;       // [B]
  float* top;                      // [2]: the largest valid ratio and d resource / d mean, as the combine launch formed them
  float* out; float* d_arch; int64_t ld_darch; float* d_ratios;
  int32_t B, E, D, resource_type;
  float tau_a, tau_z;
  double p;
  float w_res, w_con, w_std, w_max;
};

__device__ __forceinline__ float unit_row(const float* src, float* dst, int N, float* red) {
  float ss = 0.f;
  for (int e = threadIdx.x; e < N; e += NT) { const float v = src[e]; ss += v * v; }
  const float norm = sqrtf(block_sum(ss, red));
  for (int e = threadIdx.x; e < N; e += NT) dst[e] = src[e] / norm;
  return norm;
}

__global__ __launch_bounds__(NT) void router_unit_kernel(const RsK p) {
  __shared__ float red[4];
  const int i = (int)blockIdx.x;
  if (p.valid[i] == 0.f) return;
  const float na = unit_row(p.arch + (int64_t)i * p.ld_arch, p.ahat + (int64_t)i * p.E, p.E, red);
  unit_row(p.text + (int64_t)i * p.ld_text, p.zhat + (int64_t)i * p.D, p.D, red);
  if (threadIdx.x == 0) p.na[i] = na;
}

// s[j] = (own . unit[j]) / tau for the valid j: wave w takes j = w, w + 4, ..; the lanes walk the features
__device__ __forceinline__ void gram_row(const float* own, const float* unit, int N, const float* valid, int B, float tau, float* s) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int j = wave; j < B; j += NT / 64) {
    if (valid[j] == 0.f) continue;                       // (uniform over the wave)
    const float* u = unit + (int64_t)j * N;
    float a = 0.f;
    for (int e = lane; e < N; e += 64) a += own[e] * u[e];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    if (lane == 0) s[j] = a / tau;
  }
}

struct RowSoftmax { float m, sum, logsum; };

__device__ __forceinline__ RowSoftmax row_softmax(const float* s, const float* valid, int B, float* red) {
  float m = -INFINITY;
  for (int j = threadIdx.x; j < B; j += NT)
    if (valid[j] != 0.f) m = fmaxf(m, s[j]);
  m = block_max(m, red);
  float a = 0.f;
  for (int j = threadIdx.x; j < B; j += NT)
    if (valid[j] != 0.f) a += expf(s[j] - m);
  RowSoftmax r;
  r.m = m;
  r.sum = block_sum(a, red);
  r.logsum = logf(r.sum);
  return r;
}

__global__ __launch_bounds__(NT) void router_row_kernel(const RsK p) {
  __shared__ float own_a[FEAT_MAX];
  __shared__ float own_z[FEAT_MAX];
  __shared__ float sa[APTP_ROUTER_STAGE_MAX_B];
  __shared__ float sz[APTP_ROUTER_STAGE_MAX_B];
  __shared__ float red[4];
  const int i = (int)blockIdx.x, B = p.B;
  if (p.valid[i] == 0.f) return;
  for (int e = threadIdx.x; e < p.E; e += NT) own_a[e] = p.ahat[(int64_t)i * p.E + e];
  for (int e = threadIdx.x; e < p.D; e += NT) own_z[e] = p.zhat[(int64_t)i * p.D + e];
  __syncthreads();
  gram_row(own_a, p.ahat, p.E, p.valid, B, p.tau_a, sa);
  gram_row(own_z, p.zhat, p.D, p.valid, B, p.tau_z, sz);
  __syncthreads();
  const RowSoftmax A = row_softmax(sa, p.valid, B, red);
  const RowSoftmax Z = row_softmax(sz, p.valid, B, red);
  float acc = 0.f;
  for (int j = threadIdx.x; j < B; j += NT) {
    if (p.valid[j] == 0.f) continue;
    const float ea = expf(sa[j] - A.m);
    const float P = ea / A.sum, T = expf(sz[j] - Z.m) / Z.sum;
    float one_minus = 1.0f - P;
    if (P > 0.5f) {
      // at most one j of a row: 1 - P from the other exponentials of the row, not from a difference of nearly equal numbers
      float others = 0.f;
      for (int k = 0; k < B; ++k)
        if (k != j && p.valid[k] != 0.f) others += expf(sa[k] - A.m);
      one_minus = others / A.sum;
    }
    const float logP = fmaxf((sa[j] - A.m) - A.logsum, -100.f);
    const float log1mP = fmaxf(logf(one_minus), -100.f);             // F.binary_cross_entropy's clamp
    acc += T * logP + (1.0f - T) * log1mP;
    p.P[(int64_t)i * B + j] = P;
    p.T[(int64_t)i * B + j] = T;
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) p.rowloss[i] = acc;
}

// The statistics of the <= 1024 ratios are scalars that a difference then cancels (|mean - p|, the deviation of nearly equal
// ratios): they are accumulated in fp64 by this one workgroup and rounded to fp32 once, as loss_stage.hip forms its coefficients
__global__ __launch_bounds__(NT) void router_combine_kernel(const RsK p) {
  __shared__ float red[4];
  __shared__ double red64[NT];
  const int B = p.B;
  float cnt = 0.f, l = 0.f, rm = -INFINITY;
  double rs = 0.0;
  for (int b = threadIdx.x; b < B; b += NT) {
    const float vb = p.valid[b];
    if (vb != 0.f) {
      const float r = p.ratios[b];
      cnt += vb; l += p.rowloss[b]; rs += (double)r; rm = fmaxf(rm, r);
    }
  }
  const float n = block_sum(cnt, red);
  if (n == 0.f) {
    if (threadIdx.x < 8) p.out[threadIdx.x] = 0.f;
    return;
  }
  l = block_sum(l, red);
  rs = block_sum_f64(rs, red64);
  rm = block_max(rm, red);
  const double mean = rs / (double)n;
  double ss = 0.0;
  float at = 0.f;
  for (int b = threadIdx.x; b < B; b += NT) {
    if (p.valid[b] != 0.f) {
      const float r = p.ratios[b];
      const double d = (double)r - mean;
      ss += d * d;
      at += r == rm ? 1.f : 0.f;
    }
  }
  ss = block_sum_f64(ss, red64);
  at = block_sum(at, red);
  if (threadIdx.x != 0) return;
  const float contrastive = -l / (n * n);
  double res, dres;                                    // the derivative on the branch the value took: the backward reads it
  if (p.resource_type == APTP_RESOURCE_LOG) {
    res = mean > p.p ? log(mean / p.p) : log(p.p / mean);
    dres = mean > p.p ? 1.0 / mean : -1.0 / mean;
  } else if (p.resource_type == APTP_RESOURCE_MAE) {
    res = fabs(mean - p.p);
    dres = mean > p.p ? 1.0 : (mean < p.p ? -1.0 : 0.0);
  } else {
    res = (mean - p.p) * (mean - p.p);
    dres = 2.0 * (mean - p.p);
  }
  const float resource = (float)res;
  const float max_loss = (float)(1.0 - (double)rm);
  const float std_loss = (float)-sqrt(ss / ((double)n - 1.0));     // n = 1: 0 / 0, the NaN torch.std gives
  p.out[0] = contrastive;
  p.out[1] = resource;
  p.out[2] = max_loss;
  p.out[3] = std_loss;
  p.out[4] = p.w_res * resource + p.w_con * contrastive + p.w_std * std_loss + p.w_max * max_loss;
  p.out[5] = (float)mean;
  p.out[6] = n;
  p.out[7] = at;
  p.top[0] = rm;
  p.top[1] = (float)dres;
}

__global__ __launch_bounds__(NT) void router_dscore_kernel(const RsK p) {
  __shared__ float dp[APTP_ROUTER_STAGE_MAX_B];
  __shared__ float red[4];
  const int i = (int)blockIdx.x, B = p.B;
  const float n = p.out[6];
  if (n == 0.f || p.valid[i] == 0.f) return;
  const float c = p.g[0] * p.w_con / (n * n);
  float dot = 0.f;
  for (int j = threadIdx.x; j < B; j += NT) {
    if (p.valid[j] == 0.f) continue;
    const float P = p.P[(int64_t)i * B + j], T = p.T[(int64_t)i * B + j];
    const float d = (P - T) / fmaxf(P * (1.0f - P), 1e-12f) * c;     // binary_cross_entropy_backward
    dp[j] = d;
    dot += d * P;
  }
  dot = block_sum(dot, red);
  for (int j = threadIdx.x; j < B; j += NT)
    if (p.valid[j] != 0.f) p.dS[(int64_t)i * B + j] = p.P[(int64_t)i * B + j] * (dp[j] - dot) / p.tau_a;
}

__global__ __launch_bounds__(NT) void router_darch_kernel(const RsK p) {
  __shared__ float cj[APTP_ROUTER_STAGE_MAX_B];
  __shared__ float red[4];
  const int i = (int)blockIdx.x, B = p.B, E = p.E;
  const float n = p.out[6];
  float* drow = p.d_arch + (int64_t)i * p.ld_darch;
  if (n == 0.f || p.valid[i] == 0.f) {
    // a sample that is not there: zeros, and no operand is read
    for (int e = threadIdx.x; e < E; e += NT) drow[e] = 0.f;
    if (threadIdx.x == 0) p.d_ratios[i] = 0.f;
    return;
  }
  for (int j = threadIdx.x; j < B; j += NT)
    cj[j] = p.valid[j] != 0.f ? p.dS[(int64_t)i * B + j] + p.dS[(int64_t)j * B + i] : 0.f;
  __syncthreads();
  float acc[PER_THREAD];
#pragma unroll
  for (int k = 0; k < PER_THREAD; ++k) acc[k] = 0.f;
  for (int j = 0; j < B; ++j) {
    if (p.valid[j] == 0.f) continue;
    const float c = cj[j];
    const float* u = p.ahat + (int64_t)j * E;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
      const int e = (int)threadIdx.x + k * NT;
      if (e < E) acc[k] += c * u[e];
    }
  }
  const float* own = p.ahat + (int64_t)i * E;
  float dot = 0.f;
#pragma unroll
  for (int k = 0; k < PER_THREAD; ++k) {
    const int e = (int)threadIdx.x + k * NT;
    if (e < E) dot += acc[k] * own[e];
  }
  dot = block_sum(dot, red);
  const float na = p.na[i];
#pragma unroll
  for (int k = 0; k < PER_THREAD; ++k) {
    const int e = (int)threadIdx.x + k * NT;
    if (e < E) drow[e] = (acc[k] - own[e] * dot) / na;
  }
  if (threadIdx.x != 0) return;
  const float g = p.g[0], r = p.ratios[i], mean = p.out[5], sd = -p.out[3], at = p.out[7];
  const float dres = p.top[1];
  float d = p.w_res * dres / n;
  // torch's std backward: nothing flows where the deviation is exactly 0 (the single-architecture baseline)
  if (sd != 0.f) d += p.w_std * (-(r - mean) / ((n - 1.0f) * sd));
  // the maximum itself (1 - max_loss is not it, bit for bit): shared evenly among the samples that attain it (torch.max)
  if (r == p.top[0]) d += p.w_max * (-1.0f / at);
  p.d_ratios[i] = g * d;
}

bool rs_plan(const AptpRouterStageParams* p, RsK* k, bool bwd) {
#define RS_REQUIRE(cond, ...)      \
  do {                             \
    if (!(cond)) {                 \
      aptp_set_error(__VA_ARGS__); \
      return false;                \
    }                              \
  } while (0)
  RS_REQUIRE(p, "router_stage: null parameter block");
  RS_REQUIRE(p->B >= 1 && p->B <= APTP_ROUTER_STAGE_MAX_B, "router_stage: B must be 1..%d (got %d)", APTP_ROUTER_STAGE_MAX_B, p->B);
  RS_REQUIRE(p->E >= 1 && p->E <= APTP_ROUTER_STAGE_MAX_FEATURES, "router_stage: E must be 1..%d (got %d)", APTP_ROUTER_STAGE_MAX_FEATURES, p->E);
  RS_REQUIRE(p->D >= 1 && p->D <= APTP_ROUTER_STAGE_MAX_FEATURES, "router_stage: D must be 1..%d (got %d)", APTP_ROUTER_STAGE_MAX_FEATURES, p->D);
  RS_REQUIRE(p->text && p->arch && p->ratios && p->valid, "router_stage: null operand (text / arch / ratios / valid)");
  RS_REQUIRE(p->work && p->out, "router_stage: null work / out");
  RS_REQUIRE(p->ld_text >= p->D && p->ld_arch >= p->E, "router_stage: row pitch below the row length");
  RS_REQUIRE(p->resource_type == APTP_RESOURCE_LOG || p->resource_type == APTP_RESOURCE_MAE || p->resource_type == APTP_RESOURCE_MSE,
             "router_stage: unknown resource type %d", p->resource_type);
  RS_REQUIRE(p->tau_arch > 0.f && p->tau_text > 0.f, "router_stage: temperatures must be positive");
  if (bwd) {
    RS_REQUIRE(p->g, "router_stage: backward needs g");
    RS_REQUIRE(p->d_arch && p->d_ratios, "router_stage: null d_arch / d_ratios");
    RS_REQUIRE(p->ld_darch >= p->E, "router_stage: d_arch pitch below E");
  }
#undef RS_REQUIRE
  const int64_t B = p->B, E = p->E, D = p->D;
  float* w = p->work;
  k->text = p->text; k->ld_text = p->ld_text; k->arch = p->arch; k->ld_arch = p->ld_arch;
  k->ratios = p->ratios; k->valid = p->valid; k->g = p->g;
  k->ahat = w; w += B * E;
  k->zhat = w; w += B * D;
  k->P = w; w += B * B;
  k->T = w; w += B * B;
  k->dS = w; w += B * B;
  k->na = w; w += B;
  k->rowloss = w; w += B;
  k->top = w;
  k->out = p->out; k->d_arch = p->d_arch; k->ld_darch = p->ld_darch; k->d_ratios = p->d_ratios;
  k->B = p->B; k->E = p->E; k->D = p->D; k->resource_type = p->resource_type;
  k->tau_a = p->tau_arch; k->tau_z = p->tau_text; k->p = p->p;
  k->w_res = p->w_resource; k->w_con = p->w_contrastive; k->w_std = p->w_std; k->w_max = p->w_max;
  return true;
}

}  // namespace

extern "C" int64_t aptp_router_stage_work_floats(int32_t B, int32_t E, int32_t D) {
  if (B < 1 || B > APTP_ROUTER_STAGE_MAX_B || E < 1 || E > APTP_ROUTER_STAGE_MAX_FEATURES || D < 1 || D > APTP_ROUTER_STAGE_MAX_FEATURES)
    return 0;
  return (int64_t)B * E + (int64_t)B * D + 3 * (int64_t)B * B + 2 * (int64_t)B + 2;
}

extern "C" int aptp_sinkhorn_assign(const AptpSinkhornParams* p, aptp_stream_t stream) {
  APTP_CHECK(p, "sinkhorn_assign: null parameter block");
  APTP_CHECK(p->B >= 1 && p->B <= APTP_ROUTER_STAGE_MAX_B, "sinkhorn_assign: B must be 1..%d (got %d)", APTP_ROUTER_STAGE_MAX_B, p->B);
  APTP_CHECK(p->K >= 1 && p->K <= APTP_SINKHORN_MAX_K, "sinkhorn_assign: K must be 1..%d (got %d)", APTP_SINKHORN_MAX_K, p->K);
  APTP_CHECK(p->iters >= 0 && p->iters <= 1000, "sinkhorn_assign: iters must be 0..1000 (got %d)", p->iters);
  APTP_CHECK(p->eps > 0.f, "sinkhorn_assign: eps must be positive");
  APTP_CHECK(p->scores && p->valid && p->idx && p->q, "sinkhorn_assign: null pointer (scores / valid / idx / q)");
  APTP_CHECK(p->ld >= p->K, "sinkhorn_assign: row pitch below K");
  SkK k;
  k.scores = p->scores; k.ld = p->ld; k.valid = p->valid; k.idx = p->idx; k.q = p->q;
  k.B = p->B; k.K = p->K; k.iters = p->iters; k.eps = p->eps;
  hipLaunchKernelGGL(sinkhorn_assign_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}

extern "C" int aptp_router_stage(const AptpRouterStageParams* p, aptp_stream_t stream) {
  RsK k = {};
  if (!rs_plan(p, &k, false)) return APTP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(router_unit_kernel, dim3(k.B), dim3(NT), 0, s, k);
  hipLaunchKernelGGL(router_row_kernel, dim3(k.B), dim3(NT), 0, s, k);
  hipLaunchKernelGGL(router_combine_kernel, dim3(1), dim3(NT), 0, s, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}

extern "C" int aptp_router_stage_bwd(const AptpRouterStageParams* p, aptp_stream_t stream) {
  RsK k = {};
  if (!rs_plan(p, &k, true)) return APTP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(router_dscore_kernel, dim3(k.B), dim3(NT), 0, s, k);
  hipLaunchKernelGGL(router_darch_kernel, dim3(k.B), dim3(NT), 0, s, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
