// Flash-style attention backward, head_dim 64, bf16 operands, fp32 accumulation (gfx950).
//
// With P = softmax(QK^T * scale) recomputed from the forward's log-sum-exp (no N x N tensor is stored):
//   delta[q] = sum_d dO[q,d] * O[q,d]
//   dV = P^T dO;   dP = dO V^T;   dS = P o (dP - delta);   dQ = scale * dS K;   dK = scale * dS^T Q
// Three kernels, none of which needs a cross-workgroup reduction (deterministic):
//   attn_delta_kernel   one thread per (b, q, head)
//   attn_dq_kernel      workgroup = 128 queries (4 waves x 32), sweeps key tiles;   mirrors the forward's data flow
//   attn_dkdv_kernel    workgroup = 128 keys (4 waves x 32), sweeps query tiles
// MFMA operand plumbing is the forward kernel's: the "row on the lane" product is computed transposed
// (mfma_f32_32x32x16_bf16 with the LDS tile as A operand and register-resident fragments as B operand), so each lane
// owns ONE query (dQ kernel) or ONE key (dK/dV kernel) and the score accumulator, converted to bf16, is directly the
// B operand of the following product; the second view of an operand tile (d on the MFMA row index) is a hardware-transposed read
// of the same row-major LDS image (ds_read_b64_tr_b16), in the 16-row order the accumulators hold their rows in.
#include "aptp_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

struct AttnBwdK {
  const __bf16* q; int64_t qsb, qsl;
  const __bf16* k; int64_t ksb, ksl;
  const __bf16* v; int64_t vsb, vsl;
  const __bf16* o; int64_t osb, osl;
  const __bf16* dout; int64_t dosb, dosl;
  __bf16* dq; int64_t dqsb, dqsl;
  __bf16* dk; int64_t dksb, dksl;
  __bf16* dv; int64_t dvsb, dvsl;
  const float* lse; float* delta;   // [B, H, Lq]
  int B, H, Lq, Lk;
  float scale, c;                   // c = scale * log2(e)
  float* part; int nsplit;          // dK/dV kernel: query range split over nsplit workgroups, fp32 partials [nsplit][B][H][Lk][128]
};

__global__ __launch_bounds__(256) void attn_delta_kernel(const AttnBwdK p) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)p.B * p.Lq * p.H;
  if (idx >= total) return;
  const int h = (int)(idx % p.H);
  const int64_t bq = idx / p.H;
  const int q = (int)(bq % p.Lq), b = (int)(bq / p.Lq);
  const __bf16* op = p.o + (int64_t)b * p.osb + (int64_t)q * p.osl + h * 64;
  const __bf16* dp = p.dout + (int64_t)b * p.dosb + (int64_t)q * p.dosl + h * 64;
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    union { u32x4 v; __bf16 e[8]; } a, d;
    a.v = *reinterpret_cast<const u32x4*>(op + i * 8);
    d.v = *reinterpret_cast<const u32x4*>(dp + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc += (float)a.e[e] * (float)d.e[e];
  }
  p.delta[((int64_t)b * p.H + h) * p.Lq + q] = acc;
}

// One row-major LDS image per operand tile serves BOTH MFMA views (round 4; the second, software-transposed image with its eight
// scattered 4-byte stores per thread is gone): [64 rows][64 d], 16-byte chunk c of row r at chunk c ^ xs_row(r).
//   rows on the MFMA row index:  ds_read_b128 (frag_rm)       -- the 8 even rows of a lane group have distinct xs_row: conflict-free
//   d on the MFMA row index:     ds_read_b64_tr_b16 (frag_trh) -- the 4 rows of a block cover disjoint 64-byte spans of the bank line
__device__ __forceinline__ int xs_row(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }

// stage a [64 rows][64 d] tile held as row pairs (2*pair, 2*pair+1; 16-byte chunk `chunk`)
__device__ __forceinline__ void stage_tile(__bf16* rm, const u32x4 r0, const u32x4 r1, int pair, int chunk) {
  const int sw = chunk ^ xs_row(2 * pair);          // (rows 2p and 2p+1 share xs_row)
  *reinterpret_cast<u32x4*>(rm + (2 * pair) * 64 + sw * 8) = r0;
  *reinterpret_cast<u32x4*>(rm + (2 * pair + 1) * 64 + sw * 8) = r1;
}

__device__ __forceinline__ u32x4 load_row16(const __bf16* base, int64_t stride, int row, int nrows, int chunk) {
  const int rc = row < nrows ? row : nrows - 1;
  u32x4 v = *reinterpret_cast<const u32x4*>(base + (int64_t)rc * stride + chunk * 8);
  return row < nrows ? v : (u32x4){0u, 0u, 0u, 0u};
}

// A-operand fragment of the image with ROWS on the MFMA row index: lane (row = base + lq, hh), k-step s -> chunk 2s + hh
__device__ __forceinline__ bf16x8 frag_rm(const __bf16* img, int row, int s, int hh) {
  const int sw = (2 * s + hh) ^ xs_row(row);
  return *reinterpret_cast<const bf16x8*>(img + row * 64 + sw * 8);
}
// A-operand fragment of the same image with d on the MFMA row index (d = 32u + (lane & 31)), k = the 16 rows of slot (t, s2) in
// the order the score accumulators hold them: element j <-> row 32t + 16s2 + (j & 3) + 8(j >> 2) + 4hh.  Two hardware-transposed
// reads: lane (hh, gb = (lane >> 4) & 1, q_ = (lane >> 2) & 3, p_ = lane & 3) addresses row 32t + 16s2 + 4hh + q_ (+ 8), columns
// 32u + 16gb + 4p_ .. +3 and receives column 32u + 16gb + (lane & 15) of the block's four rows.  EXEC must be all ones.
__device__ __forceinline__ bf16x8 frag_trh(const __bf16* img, int u, int t, int s2, int lane) {
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const int q_ = (lane >> 2) & 3, p_ = lane & 3, gb = (lane >> 4) & 1, hh = lane >> 5;
  const int row = 32 * t + 16 * s2 + 4 * hh + q_;
  const int ch = 4 * u + 2 * gb + (p_ >> 1);
  const __bf16* a0 = img + row * 64 + ((ch ^ xs_row(row)) * 8) + 4 * (p_ & 1);
  const __bf16* a1 = img + (row + 8) * 64 + ((ch ^ xs_row(row + 8)) * 8) + 4 * (p_ & 1);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a1));
  const s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, both);
}

__global__ __launch_bounds__(256) void attn_dq_kernel(const AttnBwdK p) {
  __shared__ __attribute__((aligned(16))) __bf16 Ks[64 * 64], Vs[64 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 31, hh = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y;
  const int q0 = blockIdx.x * 128 + wave * 32;
  const int qrow = q0 + lq;
  const bool qok = qrow < p.Lq;
  const int qc = qok ? qrow : p.Lq - 1;
  const __bf16* qp = p.q + (int64_t)b * p.qsb + (int64_t)h * 64;
  const __bf16* dop = p.dout + (int64_t)b * p.dosb + (int64_t)h * 64;
  const __bf16* kp = p.k + (int64_t)b * p.ksb + (int64_t)h * 64;
  const __bf16* vp = p.v + (int64_t)b * p.vsb + (int64_t)h * 64;
  bf16x8 qf[4], dof[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    u32x4 a = *reinterpret_cast<const u32x4*>(qp + (int64_t)qc * p.qsl + 16 * s + 8 * hh);
    u32x4 d = *reinterpret_cast<const u32x4*>(dop + (int64_t)qc * p.dosl + 16 * s + 8 * hh);
    a = qok ? a : (u32x4){0u, 0u, 0u, 0u};
    d = qok ? d : (u32x4){0u, 0u, 0u, 0u};
    qf[s] = __builtin_bit_cast(bf16x8, a);
    dof[s] = __builtin_bit_cast(bf16x8, d);
  }
  const int64_t sidx = ((int64_t)b * p.H + h) * p.Lq + qc;
  const float lse = qok ? p.lse[sidx] : 0.f;
  const float delta = qok ? p.delta[sidx] : 0.f;

  const int chunk = tid & 7, pair = tid >> 3;
  u32x4 kr[2], vr[2];
  auto load_kv = [&](int tile) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      kr[i] = load_row16(kp, p.ksl, tile * 64 + 2 * pair + i, p.Lk, chunk);
      vr[i] = load_row16(vp, p.vsl, tile * 64 + 2 * pair + i, p.Lk, chunk);
    }
  };
  f32x16 dqacc[2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int r = 0; r < 16; ++r) dqacc[u][r] = 0.f;

  const int ntiles = (p.Lk + 63) / 64;
  load_kv(0);
  for (int tile = 0; tile < ntiles; ++tile) {
    __syncthreads();
    stage_tile(Ks, kr[0], kr[1], pair, chunk);
    stage_tile(Vs, vr[0], vr[1], pair, chunk);
    __syncthreads();
    if (tile + 1 < ntiles) load_kv(tile + 1);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x16 sacc, dpacc;
#pragma unroll
      for (int r = 0; r < 16; ++r) { sacc[r] = 0.f; dpacc[r] = 0.f; }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rm(Ks, 32 * t + lq, s, hh), qf[s], sacc, 0, 0, 0);
        dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rm(Vs, 32 * t + lq, s, hh), dof[s], dpacc, 0, 0, 0);
      }
      // sacc[r] = S^T[key = 64*tile + 32t + (r&3) + 8(r>>2) + 4hh][q]; rows past Lk hold K = 0, so their dS meets K^T = 0
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[r], p.c, -lse));   // raw v_exp_f32 (argument <= ~0, as in the forward)
        sacc[r] = pv * (dpacc[r] - delta);
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        bf16x8 dsf;
#pragma unroll
        for (int j = 0; j < 8; ++j) dsf[j] = (__bf16)sacc[8 * s2 + j];
#pragma unroll
        for (int u = 0; u < 2; ++u)
          dqacc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_trh(Ks, u, t, s2, lane), dsf, dqacc[u], 0, 0, 0);
      }
    }
  }
  if (qok) {
    __bf16* dqp = p.dq + (int64_t)b * p.dqsb + (int64_t)qrow * p.dqsl + (int64_t)h * 64;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = 32 * u + 8 * g + 4 * hh;
        uint2 w;
        w.x = pack_bf16x2(dqacc[u][4 * g + 0] * p.scale, dqacc[u][4 * g + 1] * p.scale);
        w.y = pack_bf16x2(dqacc[u][4 * g + 2] * p.scale, dqacc[u][4 * g + 3] * p.scale);
        *reinterpret_cast<uint2*>(dqp + d) = w;
      }
  }
}

__global__ __launch_bounds__(256, 2) void attn_dkdv_kernel(const AttnBwdK p) {
  __shared__ __attribute__((aligned(16))) __bf16 Qs[64 * 64], Ds[64 * 64];
  __shared__ __attribute__((aligned(16))) float lse_s[64], delta_s[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lk = lane & 31, hh = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y;
  const int nkt = (p.Lk + 127) / 128;
  const int kt = blockIdx.x % nkt, sp = blockIdx.x / nkt;       // key tile, slice of the query range
  const int k0 = kt * 128 + wave * 32;
  const int krow = k0 + lk;
  const bool kok = krow < p.Lk;
  const int kc = kok ? krow : p.Lk - 1;
  const __bf16* qp = p.q + (int64_t)b * p.qsb + (int64_t)h * 64;
  const __bf16* dop = p.dout + (int64_t)b * p.dosb + (int64_t)h * 64;
  const __bf16* kp = p.k + (int64_t)b * p.ksb + (int64_t)h * 64;
  const __bf16* vp = p.v + (int64_t)b * p.vsb + (int64_t)h * 64;
  bf16x8 kf[4], vf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    u32x4 a = *reinterpret_cast<const u32x4*>(kp + (int64_t)kc * p.ksl + 16 * s + 8 * hh);
    u32x4 d = *reinterpret_cast<const u32x4*>(vp + (int64_t)kc * p.vsl + 16 * s + 8 * hh);
    a = kok ? a : (u32x4){0u, 0u, 0u, 0u};
    d = kok ? d : (u32x4){0u, 0u, 0u, 0u};
    kf[s] = __builtin_bit_cast(bf16x8, a);
    vf[s] = __builtin_bit_cast(bf16x8, d);
  }
  const int chunk = tid & 7, pair = tid >> 3;
  u32x4 qr[2], dr[2];
  float sreg = 0.f;
  const float* lse_g = p.lse + ((int64_t)b * p.H + h) * p.Lq;
  const float* delta_g = p.delta + ((int64_t)b * p.H + h) * p.Lq;
  auto load_q = [&](int tile) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      qr[i] = load_row16(qp, p.qsl, tile * 64 + 2 * pair + i, p.Lq, chunk);
      dr[i] = load_row16(dop, p.dosl, tile * 64 + 2 * pair + i, p.Lq, chunk);
    }
    if (tid < 128) {
      const int qi = tile * 64 + (tid & 63);
      const int qic = qi < p.Lq ? qi : p.Lq - 1;
      const float v = (tid < 64 ? lse_g : delta_g)[qic];
      sreg = qi < p.Lq ? v : 0.f;
    }
  };
  f32x16 dkacc[2], dvacc[2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dkacc[u][r] = 0.f; dvacc[u][r] = 0.f; }

  const int ntiles_all = (p.Lq + 63) / 64;
  const int tile0 = (int)(((int64_t)ntiles_all * sp) / p.nsplit), ntiles = (int)(((int64_t)ntiles_all * (sp + 1)) / p.nsplit);
  if (tile0 < ntiles) load_q(tile0);
  for (int tile = tile0; tile < ntiles; ++tile) {
    __syncthreads();
    stage_tile(Qs, qr[0], qr[1], pair, chunk);
    stage_tile(Ds, dr[0], dr[1], pair, chunk);
    if (tid < 64) lse_s[tid] = sreg;
    else if (tid < 128) delta_s[tid - 64] = sreg;
    __syncthreads();
    if (tile + 1 < ntiles) load_q(tile + 1);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x16 sacc, dpacc;
#pragma unroll
      for (int r = 0; r < 16; ++r) { sacc[r] = 0.f; dpacc[r] = 0.f; }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rm(Qs, 32 * t + lk, s, hh), kf[s], sacc, 0, 0, 0);
        dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rm(Ds, 32 * t + lk, s, hh), vf[s], dpacc, 0, 0, 0);
      }
      // sacc[r] = S[q = 64*tile + 32t + (r&3) + 8(r>>2) + 4hh][key]; query rows past Lq hold Q = dO = 0, lse = delta = 0
      f32x16 pacc;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 l4 = *reinterpret_cast<const float4*>(lse_s + 32 * t + 8 * g + 4 * hh);
        const float4 d4 = *reinterpret_cast<const float4*>(delta_s + 32 * t + 8 * g + 4 * hh);
        const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * g + i;
          const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[r], p.c, -lv[i]));   // raw v_exp_f32 (argument <= ~0)
          pacc[r] = pv;
          sacc[r] = pv * (dpacc[r] - dv[i]);
        }
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        bf16x8 pf, dsf;
#pragma unroll
        for (int j = 0; j < 8; ++j) { pf[j] = (__bf16)pacc[8 * s2 + j]; dsf[j] = (__bf16)sacc[8 * s2 + j]; }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          dvacc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_trh(Ds, u, t, s2, lane), pf, dvacc[u], 0, 0, 0);
          dkacc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_trh(Qs, u, t, s2, lane), dsf, dkacc[u], 0, 0, 0);
        }
      }
    }
  }
  if (kok && p.nsplit > 1) {
    // partial sums of this slice of the query range (fp32, dK already scaled): [sp][b][h][key][dk 64 | dv 64]
    float* pp = p.part + ((((int64_t)sp * p.B + b) * p.H + h) * p.Lk + krow) * 128;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = 32 * u + 8 * g + 4 * hh;
        *reinterpret_cast<float4*>(pp + d) = make_float4(dkacc[u][4 * g + 0] * p.scale, dkacc[u][4 * g + 1] * p.scale,
                                                         dkacc[u][4 * g + 2] * p.scale, dkacc[u][4 * g + 3] * p.scale);
        *reinterpret_cast<float4*>(pp + 64 + d) = make_float4(dvacc[u][4 * g + 0], dvacc[u][4 * g + 1], dvacc[u][4 * g + 2], dvacc[u][4 * g + 3]);
      }
  } else if (kok) {
    __bf16* dkp = p.dk + (int64_t)b * p.dksb + (int64_t)krow * p.dksl + (int64_t)h * 64;
    __bf16* dvp = p.dv + (int64_t)b * p.dvsb + (int64_t)krow * p.dvsl + (int64_t)h * 64;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = 32 * u + 8 * g + 4 * hh;
        uint2 w;
        w.x = pack_bf16x2(dkacc[u][4 * g + 0] * p.scale, dkacc[u][4 * g + 1] * p.scale);
        w.y = pack_bf16x2(dkacc[u][4 * g + 2] * p.scale, dkacc[u][4 * g + 3] * p.scale);
        *reinterpret_cast<uint2*>(dkp + d) = w;
        w.x = pack_bf16x2(dvacc[u][4 * g + 0], dvacc[u][4 * g + 1]);
        w.y = pack_bf16x2(dvacc[u][4 * g + 2], dvacc[u][4 * g + 3]);
        *reinterpret_cast<uint2*>(dvp + d) = w;
      }
  }
}

// dK, dV = sum over the query slices of the partials (slice order: deterministic); one thread per (b, h, key, 4 channels of 128)
__global__ __launch_bounds__(256) void attn_dkdv_fold_kernel(const AttnBwdK p) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)p.B * p.H * p.Lk * 32;
  if (idx >= total) return;
  const int c4 = (int)(idx & 31);
  const int64_t row = idx >> 5;                                   // (b * H + h) * Lk + key
  const int key = (int)(row % p.Lk);
  const int64_t bh = row / p.Lk;
  const int h = (int)(bh % p.H), b = (int)(bh / p.H);
  const int64_t slab = (int64_t)p.B * p.H * p.Lk * 128;
  const float* src = p.part + row * 128 + c4 * 4;
  float4 a = *reinterpret_cast<const float4*>(src);
  for (int s = 1; s < p.nsplit; ++s) {
    const float4 t = *reinterpret_cast<const float4*>(src + s * slab);
    a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
  }
  uint2 w; w.x = pack_bf16x2(a.x, a.y); w.y = pack_bf16x2(a.z, a.w);
  __bf16* dst = c4 < 16 ? p.dk + (int64_t)b * p.dksb + (int64_t)key * p.dksl + (int64_t)h * 64 + c4 * 4
                        : p.dv + (int64_t)b * p.dvsb + (int64_t)key * p.dvsl + (int64_t)h * 64 + (c4 - 16) * 4;
  *reinterpret_cast<uint2*>(dst) = w;
}

}  // namespace

// Few keys (cross-attention: 77) leave the dK/dV kernel with one key tile per (b, head) -- 20 workgroups sweeping 4096 queries
// each at SD-2.1 level 64 (152 us against 15 us for the forward).  The query range is then split over `q_split` workgroups.
extern "C" int aptp_attention_bwd_q_split(const AptpAttentionBwdParams* p) {
  if (!p || p->Lk <= 0 || p->Lq <= 0) return 1;
  const int64_t wgs = (int64_t)((p->Lk + 127) / 128) * p->heads * p->B;
  const int ntiles = (p->Lq + 63) / 64;
  // measured (tools/bench_attn_bwd.py, B = 4, 77 keys; us for 1 / 2 / 4 / 8 / 16 slices): 4096 queries x 5 heads 156 / 96 / 65 / 52 / 57;
  // 1024 x 10 heads 51 / 39 / 33 / 37 / 42; 256 x 20 heads 23 / 24 / 31: about 160 workgroups, and only for long query ranges
  if (wgs >= 128 || ntiles < 16) return 1;
  int64_t s = (160 + wgs / 2) / wgs;
  const int cap = ntiles / 2;                                     // at least two query tiles per slice
  s = s > cap ? cap : s;
  return (int)(s < 1 ? 1 : s);
}

extern "C" size_t aptp_attention_bwd_workspace_bytes(const AptpAttentionBwdParams* p, int32_t q_split) {
  if (!p || q_split <= 1) return 0;
  return (size_t)q_split * p->B * p->heads * p->Lk * 128 * sizeof(float);
}

extern "C" int aptp_attention_bwd(const AptpAttentionBwdParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->q && p->k && p->v && p->o && p->dout && p->dq && p->dk && p->dv && p->lse && p->delta, "attention_bwd: null pointer");
  APTP_CHECK(p->B > 0 && p->heads > 0 && p->Lq > 0 && p->Lk > 0 && p->heads <= 65535 && p->B <= 65535, "attention_bwd: bad extents");
  const int64_t strides[] = {p->q_stride_b, p->q_stride_l, p->k_stride_b, p->k_stride_l, p->v_stride_b, p->v_stride_l,
                             p->o_stride_b, p->o_stride_l, p->dout_stride_b, p->dout_stride_l, p->dq_stride_b, p->dq_stride_l,
                             p->dk_stride_b, p->dk_stride_l, p->dv_stride_b, p->dv_stride_l};
  for (int64_t s : strides) APTP_CHECK(s % 8 == 0, "attention_bwd: strides must be multiples of 8 elements");
  const void* ptrs[] = {p->q, p->k, p->v, p->o, p->dout, p->dq, p->dk, p->dv};
  for (const void* q : ptrs) APTP_CHECK(((uintptr_t)q % 16) == 0, "attention_bwd: pointers must be 16-byte aligned");
  const int64_t row_strides[] = {p->q_stride_l, p->k_stride_l, p->v_stride_l, p->o_stride_l, p->dout_stride_l,
                                 p->dq_stride_l, p->dk_stride_l, p->dv_stride_l};
  for (int64_t s : row_strides) APTP_CHECK(s >= (int64_t)p->heads * 64, "attention_bwd: row stride < heads*64");
  // P is recomputed as exp2(S*c - lse) from the forward's lse, and the forward takes scale > 0 only (rejects NaN too)
  APTP_CHECK(p->scale > 0.f, "attention_bwd: scale must be positive");
  AttnBwdK k;
  k.q = (const __bf16*)p->q; k.qsb = p->q_stride_b; k.qsl = p->q_stride_l;
  k.k = (const __bf16*)p->k; k.ksb = p->k_stride_b; k.ksl = p->k_stride_l;
  k.v = (const __bf16*)p->v; k.vsb = p->v_stride_b; k.vsl = p->v_stride_l;
  k.o = (const __bf16*)p->o; k.osb = p->o_stride_b; k.osl = p->o_stride_l;
  k.dout = (const __bf16*)p->dout; k.dosb = p->dout_stride_b; k.dosl = p->dout_stride_l;
  k.dq = (__bf16*)p->dq; k.dqsb = p->dq_stride_b; k.dqsl = p->dq_stride_l;
  k.dk = (__bf16*)p->dk; k.dksb = p->dk_stride_b; k.dksl = p->dk_stride_l;
  k.dv = (__bf16*)p->dv; k.dvsb = p->dv_stride_b; k.dvsl = p->dv_stride_l;
  k.lse = p->lse; k.delta = p->delta;
  k.B = p->B; k.H = p->heads; k.Lq = p->Lq; k.Lk = p->Lk;
  k.scale = p->scale; k.c = p->scale * 1.44269504088896340736f;
  k.nsplit = p->q_split > 1 ? p->q_split : 1;
  k.part = (float*)p->workspace;
  APTP_CHECK(k.nsplit == 1 || (p->workspace && ((uintptr_t)p->workspace % 16) == 0 && k.nsplit <= (p->Lq + 63) / 64),
             "attention_bwd: q_split needs a 16-byte aligned workspace of aptp_attention_bwd_workspace_bytes and <= the query tiles");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = (int64_t)p->B * p->Lq * p->heads;
  hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, k);
  hipLaunchKernelGGL(attn_dq_kernel, dim3((p->Lq + 127) / 128, p->heads, p->B), dim3(256), 0, s, k);
  hipLaunchKernelGGL(attn_dkdv_kernel, dim3(((p->Lk + 127) / 128) * k.nsplit, p->heads, p->B), dim3(256), 0, s, k);
  if (k.nsplit > 1) {
    const int64_t n = (int64_t)p->B * p->heads * p->Lk * 32;
    hipLaunchKernelGGL(attn_dkdv_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, k);
  }
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
