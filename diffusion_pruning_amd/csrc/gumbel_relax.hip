// The router's Gumbel-sigmoid relaxation in training mode as ONE launch forward and ONE backward, drawing its own noise on the
// project's Philox stream (the stream, the draw map and the arithmetic in gumbel_relax.h):
//   aptp_gumbel_relax      z fp32 [R, E] -> out fp32 [R, E] = [w | d] of StructureVectorQuantizer.gumbel_sigmoid_trick
//   aptp_gumbel_relax_bwd  dout fp32 [R, E] -> dz fp32 [R, E], everything but z recomputed from the seeds
//   aptp_philox_gumbel     the raw noise G (and / or the words behind it) fp32 [R, n] of the same (seeds, draw, sub, offset)
// Latency-bound (R <= 128 rows of E ~ 1.6 k at the design point): one workgroup of 256 threads per row, the row staged in LDS.
//   pass 1    the threads walk the width columns: one Philox word, two logs and one exp each; meanwhile ONE lane walks the depth
//             chain (nd <= 64: softmax, cumsum, flip, logit, sigmoid) in index order on LDS arrays and scatters it by depth_order
//   barrier
//   pass 2    one thread per segment counts its live entries in index order and adds 0.5 to the first entry of a dead one
//   barrier
//   pass 3    the row goes out with ordinary stores
// No atomics, no tickets, no reductions across lanes: the same bits at every replay.  The seeds and the draw are read from
// device memory at launch time; the codebook bit and the sub-draw are applied HERE (aptp_gr_draw), not by the caller.
#include "aptp_common.h"
#include "gumbel_relax.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;

struct GrK {
  const float* z; float* out; const float* dout; float* dz;
  const int64_t* seeds; const int64_t* draw;
  const int32_t* seg_start; const int32_t* depth_order;
  int32_t nw, nd, n_seg, sub, codebook, nzw;
  float T, base;
};

__global__ __launch_bounds__(NT) void gumbel_relax_kernel(const GrK p) {
  __shared__ float row[APTP_GUMBEL_RELAX_MAX_E];
  __shared__ float sm[APTP_GUMBEL_RELAX_MAX_ND], pr[APTP_GUMBEL_RELAX_MAX_ND], ds[APTP_GUMBEL_RELAX_MAX_ND];
  const int E = p.nw + p.nd;
  const int64_t r = blockIdx.x;
  const float* z = p.z + r * E;
  const uint64_t seed = (uint64_t)p.seeds[r];
  const uint64_t draw = aptp_gr_draw((uint64_t)p.draw[0], p.sub, p.codebook != 0);
  for (int c = threadIdx.x; c < p.nw; c += NT) row[c] = aptp_gr_relax(z[c], aptp_gr_gumbel(seed, draw, (uint64_t)c), p.base, p.T);
  if (threadIdx.x == NT - 1 && p.nd > 0) {
    aptp_gr_depth_forward(z + p.nw, p.nd, seed, draw, p.nw, p.T, p.base, sm, pr, ds);
    for (int j = 0; j < p.nd; ++j) row[p.nw + p.depth_order[j]] = ds[j];          // (a permutation of [0, nd): checked on the host)
  }
  __syncthreads();
  if (p.nzw)
    for (int s = threadIdx.x; s < p.n_seg; s += NT) {
      const int lo = p.seg_start[s], hi = p.seg_start[s + 1];
      if (aptp_gr_segment_dead(row, lo, hi)) row[lo] += 0.5f;
    }
  __syncthreads();
  float* out = p.out + r * E;
  for (int e = threadIdx.x; e < E; e += NT) out[e] = row[e];
}

__global__ __launch_bounds__(NT) void gumbel_relax_bwd_kernel(const GrK p) {
  __shared__ float sm[APTP_GUMBEL_RELAX_MAX_ND], pr[APTP_GUMBEL_RELAX_MAX_ND], ds[APTP_GUMBEL_RELAX_MAX_ND];
  __shared__ float g[APTP_GUMBEL_RELAX_MAX_ND], dzd[APTP_GUMBEL_RELAX_MAX_ND];
  const int E = p.nw + p.nd;
  const int64_t r = blockIdx.x;
  const float* z = p.z + r * E;
  const float* dout = p.dout + r * E;
  float* dz = p.dz + r * E;
  const uint64_t seed = (uint64_t)p.seeds[r];
  const uint64_t draw = aptp_gr_draw((uint64_t)p.draw[0], p.sub, p.codebook != 0);
  // the bump is a constant: the derivative is the un-bumped sigmoid's, recomputed from z and the seed
  for (int c = threadIdx.x; c < p.nw; c += NT) {
    const float s = aptp_gr_relax(z[c], aptp_gr_gumbel(seed, draw, (uint64_t)c), p.base, p.T);
    dz[c] = dout[c] * aptp_gr_relax_grad(s, p.T);
  }
  if (threadIdx.x == NT - 1 && p.nd > 0) {
    aptp_gr_depth_forward(z + p.nw, p.nd, seed, draw, p.nw, p.T, p.base, sm, pr, ds);
    for (int j = 0; j < p.nd; ++j) g[j] = dout[p.nw + p.depth_order[j]];
    aptp_gr_depth_backward(g, sm, pr, ds, p.nd, p.T, dzd);
    for (int k = 0; k < p.nd; ++k) dz[p.nw + k] = dzd[k];
  }
}

struct PgK {
  float* out; uint32_t* words;
  const int64_t* seeds; const int64_t* draw;
  int64_t n, offset;
  int32_t sub, codebook;
};

__global__ __launch_bounds__(NT) void philox_gumbel_kernel(const PgK p) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= p.n) return;
  const int64_t r = blockIdx.y;
  const uint64_t draw = aptp_gr_draw((uint64_t)p.draw[0], p.sub, p.codebook != 0);
  const uint32_t w = aptp_gr_word((uint64_t)p.seeds[r], draw, (uint64_t)p.offset + (uint64_t)i);
  if (p.out) p.out[r * p.n + i] = aptp_gr_gumbel_of(w);
  if (p.words) p.words[r * p.n + i] = w;
}

bool gr_plan(const AptpGumbelRelaxParams* p, GrK* k, bool bwd) {
#define GR_REQUIRE(cond, ...)      \
  do {                             \
    if (!(cond)) {                 \
      aptp_set_error(__VA_ARGS__); \
      return false;                \
    }                              \
  } while (0)
  GR_REQUIRE(p, "gumbel_relax: null parameter block");
  GR_REQUIRE(p->R >= 1 && p->R <= APTP_GUMBEL_RELAX_MAX_R, "gumbel_relax: R must be 1..%d (got %d)", APTP_GUMBEL_RELAX_MAX_R, p->R);
  GR_REQUIRE(p->nw >= 0 && p->nd >= 0 && p->nd <= APTP_GUMBEL_RELAX_MAX_ND, "gumbel_relax: nd must be 0..%d and nw >= 0 (got nw = %d, nd = %d)",
             APTP_GUMBEL_RELAX_MAX_ND, p->nw, p->nd);
  GR_REQUIRE(p->nw <= APTP_GUMBEL_RELAX_MAX_E && p->nw + p->nd >= 1 && p->nw + p->nd <= APTP_GUMBEL_RELAX_MAX_E,
             "gumbel_relax: E = nw + nd must be 1..%d (got %d + %d)", APTP_GUMBEL_RELAX_MAX_E, p->nw, p->nd);
  GR_REQUIRE(p->n_seg >= 0 && p->n_seg <= APTP_GUMBEL_RELAX_MAX_SEG && (p->n_seg > 0) == (p->nw > 0),
             "gumbel_relax: n_seg must be 0..%d, and 0 exactly when nw is (got %d for nw = %d)", APTP_GUMBEL_RELAX_MAX_SEG, p->n_seg, p->nw);
  GR_REQUIRE(p->sub == APTP_TN_ROUTER_ASSIGN || p->sub == APTP_TN_ROUTER_RELAX, "gumbel_relax: sub must be 6 or 7 (got %d)", p->sub);
  GR_REQUIRE(p->T > 0.f, "gumbel_relax: the temperature must be positive");
  GR_REQUIRE(p->z && p->seeds && p->draw, "gumbel_relax: null operand (z / seeds / draw)");
  GR_REQUIRE(bwd || p->out, "gumbel_relax: null out");
  GR_REQUIRE(!bwd || (p->dout && p->dz), "gumbel_relax: backward needs dout and dz");
  GR_REQUIRE(p->seg_start && p->seg_start_host, "gumbel_relax: null seg_start (device table / host copy)");
  GR_REQUIRE(p->nd == 0 || (p->depth_order && p->depth_order_host), "gumbel_relax: null depth_order (device table / host copy)");
  // the tables are device memory the kernel indexes LDS with: what they hold is checked on the host copy the caller keeps
  GR_REQUIRE(p->seg_start_host[0] == 0 && p->seg_start_host[p->n_seg] == p->nw, "gumbel_relax: seg_start must run from 0 to nw = %d (got %d .. %d)",
             p->nw, p->seg_start_host[0], p->seg_start_host[p->n_seg]);
  for (int s = 0; s < p->n_seg; ++s)
    GR_REQUIRE(p->seg_start_host[s] < p->seg_start_host[s + 1], "gumbel_relax: segment %d is empty or seg_start decreases", s);
  uint64_t seen = 0;
  for (int j = 0; j < p->nd; ++j) {
    const int32_t o = p->depth_order_host[j];
    GR_REQUIRE(o >= 0 && o < p->nd, "gumbel_relax: depth_order[%d] = %d outside [0, %d)", j, o, p->nd);
    GR_REQUIRE(!((seen >> o) & 1ull), "gumbel_relax: depth_order names %d twice", o);
    seen |= 1ull << o;
  }
#undef GR_REQUIRE
  k->z = p->z; k->out = p->out; k->dout = p->dout; k->dz = p->dz;
  k->seeds = p->seeds; k->draw = p->draw; k->seg_start = p->seg_start; k->depth_order = p->depth_order;
  k->nw = p->nw; k->nd = p->nd; k->n_seg = p->n_seg; k->sub = p->sub; k->codebook = p->codebook; k->nzw = p->non_zero_width;
  k->T = p->T; k->base = p->base;
  return true;
}

}  // namespace

extern "C" int aptp_gumbel_relax(const AptpGumbelRelaxParams* p, aptp_stream_t stream) {
  GrK k = {};
  if (!gr_plan(p, &k, false)) return APTP_EINVAL;
  hipLaunchKernelGGL(gumbel_relax_kernel, dim3(p->R), dim3(NT), 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}

extern "C" int aptp_gumbel_relax_bwd(const AptpGumbelRelaxParams* p, aptp_stream_t stream) {
  GrK k = {};
  if (!gr_plan(p, &k, true)) return APTP_EINVAL;
  hipLaunchKernelGGL(gumbel_relax_bwd_kernel, dim3(p->R), dim3(NT), 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}

extern "C" int aptp_philox_gumbel(const AptpPhiloxGumbelParams* p, aptp_stream_t stream) {
  APTP_CHECK(p, "philox_gumbel: null parameter block");
  APTP_CHECK(p->R >= 1 && p->R <= APTP_GUMBEL_RELAX_MAX_R, "philox_gumbel: R must be 1..%d (got %d)", APTP_GUMBEL_RELAX_MAX_R, p->R);
  APTP_CHECK(p->n >= 1 && p->n <= (1ll << 31), "philox_gumbel: n must be 1..2^31 (got %lld)", (long long)p->n);
  APTP_CHECK(p->offset >= 0 && p->offset <= (1ll << 62), "philox_gumbel: offset %lld outside [0, 2^62]", (long long)p->offset);
  APTP_CHECK(p->sub == APTP_TN_ROUTER_ASSIGN || p->sub == APTP_TN_ROUTER_RELAX, "philox_gumbel: sub must be 6 or 7 (got %d)", p->sub);
  APTP_CHECK((p->out || p->words) && p->seeds && p->draw, "philox_gumbel: null pointer (out and words / seeds / draw)");
  PgK k;
  k.out = p->out; k.words = p->words; k.seeds = p->seeds; k.draw = p->draw;
  k.n = p->n; k.offset = p->offset; k.sub = p->sub; k.codebook = p->codebook;
  const dim3 grid((unsigned)((p->n + NT - 1) / NT), (unsigned)p->R);
  hipLaunchKernelGGL(philox_gumbel_kernel, grid, dim3(NT), 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
