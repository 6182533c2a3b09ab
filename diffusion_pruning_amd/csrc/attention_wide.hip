// Single-head attention of width 512: the self-attention of AutoencoderKL's decoder mid-block (diffusers Attention with
// heads = 1, dim_head = 512, upcast_softmax): o = softmax(q k^T * scale) v, fp32 softmax statistics, bf16 in / out.
//
// Flash layout (S never leaves the chip, both contractions on mfma_f32_16x16x32_bf16, the O accumulator in registers).
// Workgroup = 4 waves = 32 query rows of one sample; keys walk in tiles of 32:
//   S[32 q][32 keys]    wave w computes the 16 x 16 block (q half w >> 1, key half w & 1) over all 512 channels: its Q
//                       fragments (16 rows x 512) stay in registers for the whole sweep, its K fragments are 16-byte
//                       loads straight from global memory (each K row is read by two waves of the workgroup: L1 / L2);
//   softmax             S goes through LDS; 8 threads per query row take the row maximum, the exp2 terms (-> P, bf16, LDS),
//                       the row sum and the rescale factor alpha of the running state;
//   O^T[512 c][32 q]   += V^T P^T: wave w owns channels [128 w, 128 w + 128) for all 32 queries (2 x 8 accumulator tiles,
//                       64 fp32 per lane); V^T comes from an LDS image the workgroup writes transposed (key pairs packed).
// Query tiles of 32 rows (not 64): at the decoder's 256 px point (B = 8, L = 1,024) that is 256 workgroups, one per CU,
// where 64-row tiles would leave half the chip idle; a 64-row tile would also need 128 fp32 accumulators per lane.
// Ragged ends: query rows past Lq load a clamped row and store nothing; keys past Lk load a clamped (finite) row and get
// score -inf, so their P is exactly 0.  Every tile holds >= 1 valid key, so the running maximum is finite after tile 0.
#include "attention_short.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int D = 512;       // head width
constexpr int QT = 32;       // query rows per workgroup
constexpr int KT = 32;       // keys per tile
constexpr int VLD = 40;      // V^T image row stride (bf16): 80 B rows keep the 16-byte fragment reads aligned
constexpr int PLD = 40;      // P image row stride (bf16)
constexpr int SLD = 33;      // S image row stride (fp32)

struct WideK : AttnView<__bf16> {
  int Lq, Lk;
  float c;   // scale * log2(e)
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_wide_kernel(const WideK p) {
  __shared__ __attribute__((aligned(16))) __bf16 Vt[D * VLD];
  __shared__ __attribute__((aligned(16))) __bf16 Ps[QT * PLD];
  __shared__ float Ss[QT * SLD];
  __shared__ float As[QT];
  __shared__ float Ls[QT];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g4 = lane >> 4;
  const int b = blockIdx.y;
  const int q0 = blockIdx.x * QT;

  const __bf16* qp = p.q + (int64_t)b * p.qsb;
  const __bf16* kp = p.k + (int64_t)b * p.ksb;
  const __bf16* vp = p.v + (int64_t)b * p.vsb;

  // ---- Q fragments (A operand: lane holds Q[q][32 s + 8 g4 + j]) -------------------------------------------------
  const int qb = wave >> 1, kb = wave & 1;
  bf16x8 qf[D / 32];
  {
    const int qrow = q0 + 16 * qb + l16;
    const int qc = qrow < p.Lq ? qrow : p.Lq - 1;
    const __bf16* src = qp + (int64_t)qc * p.qsl + 8 * g4;
#pragma unroll
    for (int s = 0; s < D / 32; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(src + 32 * s);
  }

  // ---- softmax role: row sr, keys 4 * sl .. + 3 -------------------------------------------------------------------
  const int sr = tid >> 3, sl = tid & 7;
  float m_run = -INFINITY, l_run = 0.f;

  // ---- V staging role: key pair vk (keys 2 vk, 2 vk + 1), 8-channel chunks vc + 16 i ---------------------------------
  const int vk = tid & 15, vc = tid >> 4;

  f32x4 oacc[2][8];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) oacc[rb][cb] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int ntiles = (p.Lk + KT - 1) / KT;
  for (int tile = 0; tile < ntiles; ++tile) {
    const int key0 = tile * KT;
    // V rows of this tile into registers (clamped rows past Lk: finite values that meet P = 0)
    u32x4 vreg[4][2];
    {
      const int ka = key0 + 2 * vk, kb2 = ka + 1;
      const int kac = ka < p.Lk ? ka : p.Lk - 1, kbc = kb2 < p.Lk ? kb2 : p.Lk - 1;
      const __bf16* va = vp + (int64_t)kac * p.vsl;
      const __bf16* vb = vp + (int64_t)kbc * p.vsl;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c0 = 8 * (vc + 16 * i);
        vreg[i][0] = *reinterpret_cast<const u32x4*>(va + c0);
        vreg[i][1] = *reinterpret_cast<const u32x4*>(vb + c0);
      }
    }
    // ---- S block of this wave --------------------------------------------------------------------------------------
    f32x4 sacc = {0.f, 0.f, 0.f, 0.f};
    {
      const int key = key0 + 16 * kb + l16;
      const int kc = key < p.Lk ? key : p.Lk - 1;
      const __bf16* src = kp + (int64_t)kc * p.ksl + 8 * g4;
#pragma unroll
      for (int s = 0; s < D / 32; ++s) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(src + 32 * s);
        sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[s], kf, sacc, 0, 0, 0);
      }
    }
    __syncthreads();   // the previous tile's readers of Ss / Ps / Vt / As are done
#pragma unroll
    for (int r = 0; r < 4; ++r) Ss[(16 * qb + 4 * g4 + r) * SLD + 16 * kb + l16] = sacc[r];
    // V^T image: dword (V[2 vk][c], V[2 vk + 1][c]) -> Vt[c][2 vk .. 2 vk + 1]
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c0 = 8 * (vc + 16 * i);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t a = vreg[i][0][e >> 1], bb = vreg[i][1][e >> 1];
        const uint32_t w = (e & 1) ? ((a >> 16) | (bb & 0xffff0000u)) : ((a & 0xffffu) | (bb << 16));
        *reinterpret_cast<uint32_t*>(Vt + (c0 + e) * VLD + 2 * vk) = w;
      }
    }
    __syncthreads();
    // ---- online softmax: 8 threads per query row ----------------------------------------------------------------
    {
      float sv[4];
      float mx = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kk = 4 * sl + j;
        sv[j] = key0 + kk < p.Lk ? Ss[sr * SLD + kk] * p.c : -INFINITY;
        mx = fmaxf(mx, sv[j]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 1));
      mx = fmaxf(mx, __shfl_xor(mx, 2));
      mx = fmaxf(mx, __shfl_xor(mx, 4));
      const float m_new = fmaxf(m_run, mx);
      const float alpha = exp2f(m_run - m_new);            // m_run = -inf on the first tile -> 0
      float pr[4], rs = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pr[j] = exp2f(sv[j] - m_new);                        // masked keys: exp2(-inf) = 0
        rs += pr[j];
      }
      rs += __shfl_xor(rs, 1);
      rs += __shfl_xor(rs, 2);
      rs += __shfl_xor(rs, 4);
      l_run = l_run * alpha + rs;
      m_run = m_new;
      uint2 pk;
      pk.x = pack_bf16x2(pr[0], pr[1]);
      pk.y = pack_bf16x2(pr[2], pr[3]);
      *reinterpret_cast<uint2*>(Ps + sr * PLD + 4 * sl) = pk;
      if (sl == 0) As[sr] = alpha;
    }
    __syncthreads();
    // ---- O^T += V^T P^T ---------------------------------------------------------------------------------------------
    bf16x8 pf[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      pf[rb] = *reinterpret_cast<const bf16x8*>(Ps + (16 * rb + l16) * PLD + 8 * g4);
      const float al = As[16 * rb + l16];
#pragma unroll
      for (int cb = 0; cb < 8; ++cb) oacc[rb][cb] *= al;
    }
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) {
      const bf16x8 vf = *reinterpret_cast<const bf16x8*>(Vt + (128 * wave + 16 * cb + l16) * VLD + 8 * g4);
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) oacc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[rb], oacc[rb][cb], 0, 0, 0);
    }
  }

  if (sl == 0) Ls[sr] = l_run;
  __syncthreads();
  // oacc[rb][cb][r] = O[q = 16 rb + l16][c = 128 wave + 16 cb + 4 g4 + r]
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int q = q0 + 16 * rb + l16;
    if (q >= p.Lq) continue;
    const float inv = 1.0f / Ls[16 * rb + l16];
    __bf16* dst = p.o + (int64_t)b * p.osb + (int64_t)q * p.osl + 128 * wave + 4 * g4;
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) {
      uint2 pk;
      pk.x = pack_bf16x2(oacc[rb][cb][0] * inv, oacc[rb][cb][1] * inv);
      pk.y = pack_bf16x2(oacc[rb][cb][2] * inv, oacc[rb][cb][3] * inv);
      *reinterpret_cast<uint2*>(dst + 16 * cb) = pk;
    }
  }
}

// ---- fp32 PARITY instantiation (never benchmarked): exact-fp32 arithmetic, same tiling of keys and the same exp2-domain
// online softmax.  Workgroup = 16 query rows; the Q tile sits in LDS, K and V are read from global memory; scores are
// plain channel-order dot products, one thread per (query, key) pair; each thread owns two output channels of all 16 rows.
struct WideF : AttnView<float> {
  int Lq, Lk;
  float c;
};

constexpr int FQ = 16;

__global__ __launch_bounds__(256) void attn_wide_f32_kernel(const WideF p) {
  __shared__ float Qs[FQ * D];
  __shared__ float Sf[FQ][KT + 1];
  __shared__ float Af[FQ];
  __shared__ float Lf[FQ];
  const int tid = threadIdx.x, b = blockIdx.y, q0 = blockIdx.x * FQ;
  for (int e = tid; e < FQ * D; e += 256) {
    const int r = e / D, d = e - r * D;
    const int qr = q0 + r < p.Lq ? q0 + r : p.Lq - 1;
    Qs[e] = p.q[(int64_t)b * p.qsb + (int64_t)qr * p.qsl + d];
  }
  float acc[FQ][2];
#pragma unroll
  for (int r = 0; r < FQ; ++r) acc[r][0] = acc[r][1] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;     // (meaningful in threads 0..FQ-1)
  const float* kb = p.k + (int64_t)b * p.ksb;
  const float* vb = p.v + (int64_t)b * p.vsb;
  __syncthreads();
  for (int key0 = 0; key0 < p.Lk; key0 += KT) {
    const int nk = p.Lk - key0 < KT ? p.Lk - key0 : KT;
    for (int e = tid; e < FQ * KT; e += 256) {
      const int r = e & (FQ - 1), kk = e / FQ;
      if (kk < nk) {
        const float* kr = kb + (int64_t)(key0 + kk) * p.ksl;
        const float* qr = Qs + r * D;
        float s = 0.f;
        for (int d = 0; d < D; ++d) s += qr[d] * kr[d];
        Sf[r][kk] = s * p.c;
      }
    }
    __syncthreads();
    if (tid < FQ) {
      float mx = -INFINITY;
      for (int kk = 0; kk < nk; ++kk) mx = fmaxf(mx, Sf[tid][kk]);
      const float m_new = fmaxf(m_run, mx);
      const float alpha = exp2f(m_run - m_new);
      float rs = 0.f;
      for (int kk = 0; kk < nk; ++kk) {
        const float pr = exp2f(Sf[tid][kk] - m_new);
        Sf[tid][kk] = pr;
        rs += pr;
      }
      l_run = l_run * alpha + rs;
      m_run = m_new;
      Af[tid] = alpha;
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = tid + 256 * h;
#pragma unroll
      for (int r = 0; r < FQ; ++r) acc[r][h] *= Af[r];
      for (int kk = 0; kk < nk; ++kk) {
        const float vv = vb[(int64_t)(key0 + kk) * p.vsl + c];
#pragma unroll
        for (int r = 0; r < FQ; ++r) acc[r][h] += Sf[r][kk] * vv;
      }
    }
    __syncthreads();
  }
  if (tid < FQ) Lf[tid] = l_run;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < FQ; ++r) {
    if (q0 + r >= p.Lq) break;
    float* dst = p.o + (int64_t)b * p.osb + (int64_t)(q0 + r) * p.osl;
    const float inv = 1.0f / Lf[r];
    dst[tid] = acc[r][0] * inv;
    dst[tid + 256] = acc[r][1] * inv;
  }
}

}  // namespace

extern "C" int aptp_attention_wide(const AptpAttentionWideParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->q && p->k && p->v && p->o, "attention_wide: null pointer");
  APTP_CHECK(p->B > 0 && p->Lq > 0 && p->Lk > 0, "attention_wide: bad extents (B %d, Lq %d, Lk %d)", p->B, p->Lq, p->Lk);
  APTP_CHECK(p->B <= 65535, "attention_wide: B %d > 65535", p->B);
  if (int rc = attn_check_view(p, "attention_wide", D, "512")) return rc;
  const float c = p->scale * 1.44269504088896340736f;
  if (p->io_f32) {
    WideF k;
    k.fill(p); k.Lq = p->Lq; k.Lk = p->Lk; k.c = c;
    hipLaunchKernelGGL(attn_wide_f32_kernel, dim3((p->Lq + FQ - 1) / FQ, p->B), dim3(256), 0, (hipStream_t)stream, k);
  } else {
    WideK k;
    k.fill(p); k.Lq = p->Lq; k.Lk = p->Lk; k.c = c;
    hipLaunchKernelGGL(attn_wide_kernel, dim3((p->Lq + QT - 1) / QT, p->B), dim3(256), 0, (hipStream_t)stream, k);
  }
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
