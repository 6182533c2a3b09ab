// The two ends of the MPNet prompt encoder (transformers MPNetEmbeddings and the masked mean of sentence-transformers'
// all-mpnet-base-v2, pdm/utils/data_utils.py:130-155):
//   aptp_embed_ln      position id from the ids, word row + position row in fp32, LayerNorm, one rounding to the stream;
//   aptp_masked_mean   sum over the valid tokens / max(number of valid tokens, 1e-9), fp32, fixed summation order.
#include "aptp_common.h"

namespace {

constexpr int ENT = 128;     // threads of embed_ln: 8 channels per thread and pass, at most 2 passes (C <= 2048)

struct EmbK {
  const int64_t* ids; const float* word; const float* pos; const float* gamma; const float* beta;
  void* out; int64_t ldo;
  int L, C, vocab, pos_rows, pad, out_f32;
  float eps;
};

__device__ __forceinline__ float block_sum_128(float v, float* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();                       // red is free (an earlier call's readers are past it)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1];
}

// One workgroup per token row.  The position id is the number of non-pad ids of the sample up to and including this row,
// plus pad (a pad token: pad itself) -- transformers' create_position_ids_from_input_ids.  An id outside [0, vocab) or a
// position outside the table is never used as an index: the row is written as NaN.
__global__ __launch_bounds__(ENT) void embed_ln_kernel(const EmbK p) {
  __shared__ float red[2];
  __shared__ int cnt_s[2];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int l = (int)(row % p.L);
  const int64_t* srow = p.ids + (row - l);
  const int64_t id = srow[l];
  int cnt = 0;
  for (int j = tid; j <= l; j += ENT) cnt += srow[j] != p.pad;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
  if ((tid & 63) == 0) cnt_s[tid >> 6] = cnt;
  __syncthreads();
  const int pos_id = (id != p.pad ? cnt_s[0] + cnt_s[1] : 0) + p.pad;
  const bool ok = id >= 0 && id < p.vocab && pos_id >= 0 && pos_id < p.pos_rows;
  const float* wr = p.word + (ok ? id : 0) * (int64_t)p.C;
  const float* pr = p.pos + (int64_t)(ok ? pos_id : 0) * p.C;

  float v[2][8];
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int c = 8 * (tid + ENT * u);
    if (c < p.C) {
      const float4 t0 = *reinterpret_cast<const float4*>(wr + c), t1 = *reinterpret_cast<const float4*>(wr + c + 4);
      const float4 q0 = *reinterpret_cast<const float4*>(pr + c), q1 = *reinterpret_cast<const float4*>(pr + c + 4);
      v[u][0] = __fadd_rn(t0.x, q0.x); v[u][1] = __fadd_rn(t0.y, q0.y); v[u][2] = __fadd_rn(t0.z, q0.z); v[u][3] = __fadd_rn(t0.w, q0.w);
      v[u][4] = __fadd_rn(t1.x, q1.x); v[u][5] = __fadd_rn(t1.y, q1.y); v[u][6] = __fadd_rn(t1.z, q1.z); v[u][7] = __fadd_rn(t1.w, q1.w);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[u][e];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[u][e] = 0.f;
    }
  }
  const float mean = block_sum_128(s, red) / (float)p.C;
  float vs = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (8 * (tid + ENT * u) < p.C) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = v[u][e] - mean; vs += d * d; }
    }
  }
  const float rstd = 1.0f / sqrtf(block_sum_128(vs, red) / (float)p.C + p.eps);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int c = 8 * (tid + ENT * u);
    if (c >= p.C) continue;
    float y[8];
    const float4 g0 = *reinterpret_cast<const float4*>(p.gamma + c), g1 = *reinterpret_cast<const float4*>(p.gamma + c + 4);
    const float4 b0 = *reinterpret_cast<const float4*>(p.beta + c), b1 = *reinterpret_cast<const float4*>(p.beta + c + 4);
    const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = ok ? (v[u][e] - mean) * rstd * g[e] + bb[e] : __builtin_nanf("");
    if (p.out_f32) {
      float4* dst = reinterpret_cast<float4*>(reinterpret_cast<float*>(p.out) + row * p.ldo + c);
      dst[0] = make_float4(y[0], y[1], y[2], y[3]);
      dst[1] = make_float4(y[4], y[5], y[6], y[7]);
    } else {
      *reinterpret_cast<uint4*>(reinterpret_cast<__bf16*>(p.out) + row * p.ldo + c) = pack_bf16x8(y);
    }
  }
}

// Masked mean: a workgroup takes 256 channels of one sample; its 256 threads are 4 token slices x 64 channel quads.  Slice s
// sums the tokens s, s + 4, ... in order; the four partial sums are then added in slice order: one fixed order, no atomics.
struct MeanK {
  const void* x; int64_t sxb, sxl; const float* mask; float* out;
  int L, C, x_f32;
};

__global__ __launch_bounds__(256) void masked_mean_kernel(const MeanK p) {
  __shared__ float part[4][64][5];
  const int tid = threadIdx.x, cq = tid & 63, sl = tid >> 6;
  const int b = blockIdx.x;
  const int c = blockIdx.y * 256 + 4 * cq;
  const float* mrow = p.mask ? p.mask + (int64_t)b * p.L : nullptr;
  float a[4] = {0.f, 0.f, 0.f, 0.f}, n = 0.f;
  for (int l = sl; l < p.L; l += 4) {
    const float m = mrow ? mrow[l] : 1.0f;
    n += m;
    if (m == 0.f || c >= p.C) continue;              // a padded row is not read
    float x[4];
    if (p.x_f32) {
      const float4 t = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p.x) + (int64_t)b * p.sxb + (int64_t)l * p.sxl + c);
      x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    } else {
      union { uint2 q; __bf16 h[4]; } u;
      u.q = *reinterpret_cast<const uint2*>(reinterpret_cast<const __bf16*>(p.x) + (int64_t)b * p.sxb + (int64_t)l * p.sxl + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = (float)u.h[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = __builtin_fmaf(x[e], m, a[e]);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) part[sl][cq][e] = a[e];
  part[sl][cq][4] = n;
  __syncthreads();
  if (sl != 0 || c >= p.C) return;
  float den = 0.f, s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    den += part[k][cq][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] += part[k][cq][e];
  }
  den = fmaxf(den, 1e-9f);
  *reinterpret_cast<float4*>(p.out + (int64_t)b * p.C + c) = make_float4(s[0] / den, s[1] / den, s[2] / den, s[3] / den);
}

}  // namespace

extern "C" int aptp_embed_ln(const AptpEmbedLnParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->ids && p->word && p->pos && p->gamma && p->beta && p->out, "embed_ln: null pointer");
  APTP_CHECK(p->B > 0 && p->L > 0 && p->vocab > 0 && p->C > 0 && p->C % 8 == 0 && p->C <= 16 * ENT,
             "embed_ln: bad extents (C must be a multiple of 8, <= %d)", 16 * ENT);
  APTP_CHECK(p->pad_id >= 0 && (int64_t)p->L + p->pad_id < p->pos_rows, "embed_ln: %d tokens with pad id %d need %d position rows, have %d",
             p->L, p->pad_id, p->L + p->pad_id + 1, p->pos_rows);
  APTP_CHECK(p->ldo >= p->C && p->ldo % 8 == 0, "embed_ln: ldo (%lld) must be >= C and a multiple of 8", (long long)p->ldo);
  APTP_CHECK((int64_t)p->B * p->L < (1ll << 31), "embed_ln: B * L too large");
  APTP_CHECK(p->eps > 0.f, "embed_ln: eps must be positive");
  APTP_CHECK(((uintptr_t)p->ids % 8) == 0 && ((uintptr_t)p->word % 16) == 0 && ((uintptr_t)p->pos % 16) == 0 &&
             ((uintptr_t)p->gamma % 16) == 0 && ((uintptr_t)p->beta % 16) == 0 && ((uintptr_t)p->out % 16) == 0, "embed_ln: pointer alignment");
  EmbK k;
  k.ids = p->ids; k.word = p->word; k.pos = p->pos; k.gamma = p->gamma; k.beta = p->beta; k.out = p->out; k.ldo = p->ldo;
  k.L = p->L; k.C = p->C; k.vocab = p->vocab; k.pos_rows = p->pos_rows; k.pad = p->pad_id; k.out_f32 = p->out_f32; k.eps = p->eps;
  hipLaunchKernelGGL(embed_ln_kernel, dim3((unsigned)(p->B * p->L)), dim3(ENT), 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}

extern "C" int aptp_masked_mean(const AptpMaskedMeanParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->x && p->out, "masked_mean: null pointer");
  APTP_CHECK(p->B > 0 && p->L > 0 && p->C > 0 && p->C % 4 == 0, "masked_mean: bad extents (C must be a multiple of 4)");
  APTP_CHECK(p->x_stride_l >= p->C && p->x_stride_l % 4 == 0 && p->x_stride_b >= 0 && p->x_stride_b % 4 == 0,
             "masked_mean: strides must be multiples of 4 elements, the row stride >= C");
  APTP_CHECK(((uintptr_t)p->x % (p->x_f32 ? 16 : 8)) == 0 && ((uintptr_t)p->out % 16) == 0 && ((uintptr_t)p->mask % 4) == 0,
             "masked_mean: pointer alignment");
  APTP_CHECK((p->C + 255) / 256 <= 65535, "masked_mean: C too large");
  MeanK k;
  k.x = p->x; k.sxb = p->x_stride_b; k.sxl = p->x_stride_l; k.mask = p->mask; k.out = p->out;
  k.L = p->L; k.C = p->C; k.x_f32 = p->x_f32 ? 1 : 0;
  hipLaunchKernelGGL(masked_mean_kernel, dim3((unsigned)p->B, (unsigned)((p->C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
