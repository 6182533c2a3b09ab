// Bidirectional self-attention with an additive relative-position bias and a key padding mask, head width 64: the
// self-attention of MPNet (transformers MPNetSelfAttention; all-mpnet-base-v2: 12 heads, scale 1/8, L <= 512):
//   o = softmax(q k^T * scale + relbias[h][j - i + L - 1] + keymask[b][j]) v,
// a masked key weighted exactly 0, fp32 softmax statistics, bf16 in / out.
//
// The work is many short sequences (a training batch is 64 x 20-40 tokens, dataset filtering 2048 x the longest caption), so
// the unit is the (sample, head) pair: one workgroup (4 waves) per pair and 128-query block, i.e. ONE workgroup per pair up
// to L = 128.  Keys are walked in chunks of 128 with an online softmax, so K (row-major) and V (transposed) of one chunk
// sit in LDS (36 KB) whatever L is; up to L = 128 there is one chunk and the rescaling multiplies by exp2(-inf) = 0 once.
//   kend               1 + the last valid key of the sample (L without a mask).  Chunks, key tiles and query strips at or
//                      past kend are never computed: with a prefix mask the cost follows the caption, not the padding.
//                      Query rows at or past kend are padding (their own mask is 0) and are written as zeros.
//   S[16 q][16 keys]   mfma_f32_16x16x32_bf16 over the 64 channels, Q fragments from global memory (kept in registers over
//                      the chunks), K fragments from LDS; the chunk's tiles stay in registers (8 x 4 fp32 per lane);
//   softmax            score * scale*log2(e) + bias*log2(e) (LDS table over j - i) + 0 / -inf per key (LDS); the running maximum
//                      of a row whose keys so far are all masked is -inf and is replaced by 0 in the exponent, so such a chunk
//                      adds exactly 0 and nothing is NaN; the last valid key (kend - 1) makes every row sum positive;
//   O[16 q][64 c]     += P V: P (bf16) through the wave's LDS strip, 32 keys per MFMA; an odd tile count writes one zero tile.
// K and V rows of masked keys are staged as zeros, so a masked key's V never meets an MFMA (not even as 0 * inf).
#include "aptp_common.h"

namespace {

constexpr int D = 64;        // head width
constexpr int LMAX = 512;    // longest sequence
constexpr int KCH = 128;     // keys per chunk
constexpr int QBLK = 128;    // query rows per workgroup (two 16-row strips per wave)
constexpr int KLD = 72;      // K image row stride (bf16): 144 B rows keep the 16-byte fragment reads aligned
constexpr int TLD = 136;     // V^T and P image row stride (bf16): 272 B rows
constexpr float LOG2E = 1.44269504088896340736f;

struct BiasK {
  const __bf16* q; int64_t qsb, qsl;
  const __bf16* k; int64_t ksb, ksl;
  const __bf16* v; int64_t vsb, vsl;
  __bf16* o; int64_t osb, osl;
  const float* rb;     // [heads][2L - 1]
  const float* km;     // [B][L] or null
  int heads, L, nqb;
  float c;             // scale * log2(e)
};

__global__ __launch_bounds__(256) void attn_bias_kernel(const BiasK p) {
  __shared__ __attribute__((aligned(16))) __bf16 Ks[KCH * KLD];
  __shared__ __attribute__((aligned(16))) __bf16 Vt[D * TLD];
  __shared__ __attribute__((aligned(16))) __bf16 Ps[4 * 16 * TLD];
  __shared__ float Bs[2 * LMAX];     // relbias[h][:] * log2(e)
  __shared__ float Km[KCH];          // 0 (valid key) or -inf (masked or past kend), this chunk
  __shared__ int kend_s;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g4 = lane >> 4;
  const int qb = blockIdx.x % p.nqb, pair = blockIdx.x / p.nqb;
  const int b = pair / p.heads, h = pair - b * p.heads;
  const int L = p.L;

  const __bf16* qp = p.q + (int64_t)b * p.qsb + h * D;
  const __bf16* kp = p.k + (int64_t)b * p.ksb + h * D;
  const __bf16* vp = p.v + (int64_t)b * p.vsb + h * D;
  const float* mrow = p.km ? p.km + (int64_t)b * L : nullptr;

  // ---- kend and the bias table --------------------------------------------------------------------------------------------
  if (tid == 0) kend_s = 0;
  __syncthreads();
  {
    int ke = mrow ? 0 : L;
    if (mrow)
      for (int j = tid; j < L; j += 256)
        if (mrow[j] != 0.f) ke = j + 1;                      // j ascends: the thread's last hit is its largest
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const int o = __shfl_xor(ke, off);
      ke = o > ke ? o : ke;
    }
    if (lane == 0) atomicMax(&kend_s, ke);
    const float* rb = p.rb + (int64_t)h * (2 * L - 1);
    for (int e = tid; e < 2 * L - 1; e += 256) Bs[e] = rb[e] * LOG2E;
  }
  __syncthreads();
  const int kend = kend_s;
  const int qbase = qb * QBLK;

  // ---- per-strip state: strip u of this wave holds query rows q0[u] .. q0[u] + 15 ------------------------------------------
  bf16x8 qf[2][2];
  f32x4 oacc[2][D / 16];
  float mrun[2][4], lrun[2][4];
  bool act[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int q0 = qbase + 16 * (wave + 4 * u);
    act[u] = q0 < L && q0 < kend;
    const int qr = q0 + l16 < L ? q0 + l16 : L - 1;
    const __bf16* src = qp + (int64_t)qr * p.qsl + 8 * g4;
    if (act[u]) {
      qf[u][0] = *reinterpret_cast<const bf16x8*>(src);
      qf[u][1] = *reinterpret_cast<const bf16x8*>(src + 32);
    } else {
      qf[u][0] = qf[u][1] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    }
#pragma unroll
    for (int db = 0; db < D / 16; ++db) oacc[u][db] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) { mrun[u][r] = -INFINITY; lrun[u][r] = 0.f; }
  }

  __bf16* const pw = Ps + wave * 16 * TLD;
  const int nch = qbase < kend ? (kend + KCH - 1) / KCH : 0;      // a block of padding rows computes nothing
  for (int ch = 0; ch < nch; ++ch) {
    const int k0 = ch * KCH;
    const int nk = kend - k0 < KCH ? kend - k0 : KCH;
    const int nt = (nk + 15) >> 4;
    const int np = (nk + 31) & ~31;
    // ---- K -> Ks[key][c], V -> Vt[c][key]; masked keys and rows past nk are zeros ------------------------------------------
    for (int e = tid; e < np * (D / 8); e += 256) {
      const int r = e >> 3, c0 = (e & 7) * 8;
      uint4 kq = make_uint4(0u, 0u, 0u, 0u), vq = make_uint4(0u, 0u, 0u, 0u);
      if (r < nk && (!mrow || mrow[k0 + r] != 0.f)) {
        kq = *reinterpret_cast<const uint4*>(kp + (int64_t)(k0 + r) * p.ksl + c0);
        vq = *reinterpret_cast<const uint4*>(vp + (int64_t)(k0 + r) * p.vsl + c0);
      }
      *reinterpret_cast<uint4*>(Ks + r * KLD + c0) = kq;
      union { uint4 q; __bf16 x[8]; } uv;
      uv.q = vq;
#pragma unroll
      for (int j = 0; j < 8; ++j) Vt[(c0 + j) * TLD + r] = uv.x[j];
    }
    if (tid < KCH) Km[tid] = (tid < nk && (!mrow || mrow[k0 + tid] != 0.f)) ? 0.f : -INFINITY;
    __syncthreads();

#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (!act[u]) continue;
      const int q0 = qbase + 16 * (wave + 4 * u);
      // S tiles of the chunk: sacc[t][r] = S[q0 + 4 g4 + r][k0 + 16 t + l16]
      f32x4 sacc[KCH / 16];
#pragma unroll
      for (int t = 0; t < KCH / 16; ++t) {
        sacc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (t < nt) {
          const __bf16* kr = Ks + (16 * t + l16) * KLD + 8 * g4;
          sacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[u][0], *reinterpret_cast<const bf16x8*>(kr), sacc[t], 0, 0, 0);
          sacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[u][1], *reinterpret_cast<const bf16x8*>(kr + 32), sacc[t], 0, 0, 0);
        }
      }
      // scaled, biased, masked scores (exp2 domain) and the chunk's row maxima (rows 4 g4 + r; a row's 16 lanes share g4)
      float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      int bi[4];                                    // bias index of key k0 + l16 for row r: key - q + L - 1, q clamped to L - 1
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = q0 + 4 * g4 + r;
        bi[r] = k0 + l16 - (q < L ? q : L - 1) + L - 1;
      }
#pragma unroll
      for (int t = 0; t < KCH / 16; ++t) {
        if (t < nt) {
          const float kmv = Km[16 * t + l16];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            // a select, not a sum: past key L - 1 the table index leaves the 2L - 1 entries that were written
            const float sv = kmv == 0.f ? sacc[t][r] * p.c + Bs[bi[r] + 16 * t] : -INFINITY;
            sacc[t][r] = sv;
            mx[r] = fmaxf(mx[r], sv);
          }
        }
      }
      float alpha[4], muse[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], off));
        const float mnew = fmaxf(mrun[u][r], mx[r]);
        muse[r] = mnew == -INFINITY ? 0.f : mnew;       // every key so far masked: exponent -inf - 0, weights exactly 0
        alpha[r] = exp2f(mrun[u][r] - muse[r]);         // first chunk: exp2(-inf) = 0
        mrun[u][r] = mnew;
      }
      // P = exp2(S - max) (masked: exactly 0), row sums in fp32, P as bf16 into the wave's strip of LDS
      float rs[4] = {0.f, 0.f, 0.f, 0.f};
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the previous strip's P reads are done
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int t = 0; t < KCH / 16; ++t) {
        if (t < nt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float pr = exp2f(sacc[t][r] - muse[r]);
            rs[r] += pr;
            pw[(4 * g4 + r) * TLD + 16 * t + l16] = (__bf16)pr;
          }
        } else if (t == nt && (nt & 1)) {
#pragma unroll
          for (int r = 0; r < 4; ++r) pw[(4 * g4 + r) * TLD + 16 * t + l16] = (__bf16)0.f;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) rs[r] += __shfl_xor(rs[r], off);
        lrun[u][r] = lrun[u][r] * alpha[r] + rs[r];
#pragma unroll
        for (int db = 0; db < D / 16; ++db) oacc[u][db][r] *= alpha[r];
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // P of this strip is visible to the whole wave
      __builtin_amdgcn_wave_barrier();
      // O += P V over 32-key steps: A = P[l16][32 kc + 8 g4 + j], B = V[32 kc + 8 g4 + j][16 db + l16] = Vt row
      const int nkc = (nt + 1) >> 1;
      for (int kc = 0; kc < nkc; ++kc) {
        const bf16x8 pf = *reinterpret_cast<const bf16x8*>(pw + l16 * TLD + 32 * kc + 8 * g4);
#pragma unroll
        for (int db = 0; db < D / 16; ++db) {
          const bf16x8 vf = *reinterpret_cast<const bf16x8*>(Vt + (16 * db + l16) * TLD + 32 * kc + 8 * g4);
          oacc[u][db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, oacc[u][db], 0, 0, 0);
        }
      }
    }
    __syncthreads();       // the chunk's K, V and mask images are free
  }

  // oacc[u][db][r] = O[q0 + 4 g4 + r][16 db + l16]; padding rows (strips at or past kend) are written as zeros
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int q0 = qbase + 16 * (wave + 4 * u);
    if (q0 >= L) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + 4 * g4 + r;
      if (q >= L) continue;
      const float inv = lrun[u][r] > 0.f ? 1.0f / lrun[u][r] : 0.f;
      __bf16* dst = p.o + (int64_t)b * p.osb + (int64_t)q * p.osl + h * D + l16;
#pragma unroll
      for (int db = 0; db < D / 16; ++db) dst[16 * db] = (__bf16)(oacc[u][db][r] * inv);
    }
  }
}

// ---- fp32 PARITY instantiation (never benchmarked): exact-fp32 arithmetic, one thread per query row, the valid keys in order
// through the same exp2-domain online softmax; K and V rows are read from global memory.  A row with no valid key is zeros.
struct BiasF {
  const float* q; int64_t qsb, qsl;
  const float* k; int64_t ksb, ksl;
  const float* v; int64_t vsb, vsl;
  float* o; int64_t osb, osl;
  const float* rb;
  const float* km;
  int heads, L, nqb;
  float scale;
};

__global__ __launch_bounds__(QBLK) void attn_bias_f32_kernel(const BiasF p) {
  const int qb = blockIdx.x % p.nqb, pair = blockIdx.x / p.nqb;
  const int b = pair / p.heads, h = pair - b * p.heads;
  const int i = qb * QBLK + threadIdx.x;
  const int L = p.L;
  if (i >= L) return;
  float q[D], acc[D];
  const float* qr = p.q + (int64_t)b * p.qsb + (int64_t)i * p.qsl + h * D;
#pragma unroll
  for (int d = 0; d < D; d += 4) {
    const float4 t = *reinterpret_cast<const float4*>(qr + d);
    q[d] = t.x; q[d + 1] = t.y; q[d + 2] = t.z; q[d + 3] = t.w;
    acc[d] = acc[d + 1] = acc[d + 2] = acc[d + 3] = 0.f;
  }
  float m_run = -INFINITY, l_run = 0.f;
  const float* kb = p.k + (int64_t)b * p.ksb + h * D;
  const float* vb = p.v + (int64_t)b * p.vsb + h * D;
  const float* rb = p.rb + (int64_t)h * (2 * L - 1) + (L - 1 - i);
  const float* mrow = p.km ? p.km + (int64_t)b * L : nullptr;
  for (int j = 0; j < L; ++j) {
    if (mrow && mrow[j] == 0.f) continue;
    const float* kr = kb + (int64_t)j * p.ksl;
    float sdot = 0.f;
#pragma unroll
    for (int d = 0; d < D; d += 4) {
      const float4 t = *reinterpret_cast<const float4*>(kr + d);
      sdot += q[d] * t.x; sdot += q[d + 1] * t.y; sdot += q[d + 2] * t.z; sdot += q[d + 3] * t.w;
    }
    const float sv = (sdot * p.scale + rb[j]) * LOG2E;
    const float m_new = fmaxf(m_run, sv);
    const float alpha = exp2f(m_run - m_new);            // -inf on the first key -> 0
    const float pr = exp2f(sv - m_new);
    l_run = l_run * alpha + pr;
    m_run = m_new;
    const float* vr = vb + (int64_t)j * p.vsl;
#pragma unroll
    for (int d = 0; d < D; d += 4) {
      const float4 t = *reinterpret_cast<const float4*>(vr + d);
      acc[d] = acc[d] * alpha + pr * t.x; acc[d + 1] = acc[d + 1] * alpha + pr * t.y;
      acc[d + 2] = acc[d + 2] * alpha + pr * t.z; acc[d + 3] = acc[d + 3] * alpha + pr * t.w;
    }
  }
  const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;
  float* dst = p.o + (int64_t)b * p.osb + (int64_t)i * p.osl + h * D;
#pragma unroll
  for (int d = 0; d < D; d += 4) *reinterpret_cast<float4*>(dst + d) = make_float4(acc[d] * inv, acc[d + 1] * inv, acc[d + 2] * inv, acc[d + 3] * inv);
}

}  // namespace

extern "C" int aptp_attention_bias(const AptpAttentionBiasParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->q && p->k && p->v && p->o && p->relbias, "attention_bias: null pointer");
  APTP_CHECK(p->B > 0 && p->heads > 0, "attention_bias: bad extents (B %d, heads %d)", p->B, p->heads);
  APTP_CHECK(p->L >= 1 && p->L <= LMAX, "attention_bias: L %d outside [1, %d]", p->L, LMAX);
  const int nqb = (p->L + QBLK - 1) / QBLK;
  APTP_CHECK((int64_t)p->B * p->heads * nqb < (1ll << 31), "attention_bias: B * heads too large");
  APTP_CHECK(p->scale > 0.f && p->scale < 1e30f, "attention_bias: scale must be positive and finite");
  const int64_t sl[4] = {p->q_stride_l, p->k_stride_l, p->v_stride_l, p->o_stride_l};
  const int64_t sb[4] = {p->q_stride_b, p->k_stride_b, p->v_stride_b, p->o_stride_b};
  const void* ptr[4] = {p->q, p->k, p->v, p->o};
  const int vec = p->io_f32 ? 4 : 8;        // elements per 16 bytes
  for (int i = 0; i < 4; ++i) {
    APTP_CHECK(sl[i] >= (int64_t)p->heads * D && sl[i] % vec == 0,
               "attention_bias: row stride %lld must be >= heads * 64 and a multiple of %d", (long long)sl[i], vec);
    APTP_CHECK(sb[i] >= 0 && sb[i] % vec == 0, "attention_bias: batch stride %lld must be a non-negative multiple of %d",
               (long long)sb[i], vec);
    APTP_CHECK(((uintptr_t)ptr[i] % 16) == 0, "attention_bias: pointers must be 16-byte aligned");
  }
  APTP_CHECK(((uintptr_t)p->relbias % 4) == 0 && ((uintptr_t)p->key_mask % 4) == 0, "attention_bias: relbias / key_mask alignment");
  const dim3 grid((unsigned)(p->B * p->heads * nqb));
  if (p->io_f32) {
    BiasF k;
    k.q = (const float*)p->q; k.qsb = p->q_stride_b; k.qsl = p->q_stride_l;
    k.k = (const float*)p->k; k.ksb = p->k_stride_b; k.ksl = p->k_stride_l;
    k.v = (const float*)p->v; k.vsb = p->v_stride_b; k.vsl = p->v_stride_l;
    k.o = (float*)p->o; k.osb = p->o_stride_b; k.osl = p->o_stride_l;
    k.rb = p->relbias; k.km = p->key_mask;
    k.heads = p->heads; k.L = p->L; k.nqb = nqb; k.scale = p->scale;
    hipLaunchKernelGGL(attn_bias_f32_kernel, grid, dim3(QBLK), 0, (hipStream_t)stream, k);
    APTP_LAUNCH_CHECK();
    return APTP_OK;
  }
  BiasK k;
  k.q = (const __bf16*)p->q; k.qsb = p->q_stride_b; k.qsl = p->q_stride_l;
  k.k = (const __bf16*)p->k; k.ksb = p->k_stride_b; k.ksl = p->k_stride_l;
  k.v = (const __bf16*)p->v; k.vsb = p->v_stride_b; k.vsl = p->v_stride_l;
  k.o = (__bf16*)p->o; k.osb = p->o_stride_b; k.osl = p->o_stride_l;
  k.rb = p->relbias; k.km = p->key_mask;
  k.heads = p->heads; k.L = p->L; k.nqb = nqb; k.c = p->scale * LOG2E;
  hipLaunchKernelGGL(attn_bias_kernel, grid, dim3(256), 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
