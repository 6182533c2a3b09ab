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
//                      Every query row below L is written.  Query rows at or past kend are padding (their own mask is 0):
//                      a 16-row strip that STARTS at or past kend -- so every strip of a 128-row query block with
//                      qbase >= kend -- is written as exact zeros; the rows past kend inside the strip that straddles
//                      kend are computed like any other row and hold ordinary attention values (what the fp32 parity
//                      kernel below computes for every row below L).  Callers must not read meaning into padding rows.
//   S[16 q][16 keys]   mfma_f32_16x16x32_bf16 over the 64 channels, Q fragments from global memory (kept in registers over
//                      the chunks), K fragments from LDS; the chunk's tiles stay in registers (8 x 4 fp32 per lane);
//   softmax            score * scale*log2(e) + bias*log2(e) (LDS table over j - i) + 0 / -inf per key (LDS); the running maximum
//                      of a row whose keys so far are all masked is -inf and is replaced by 0 in the exponent, so such a chunk
//                      adds exactly 0 and nothing is NaN; the last valid key (kend - 1) makes every row sum positive;
//   O[16 q][64 c]     += P V: P (bf16) through the wave's LDS strip, 32 keys per MFMA; an odd tile count writes one zero tile.
// K and V rows of masked keys are staged as zeros, so a masked key's V never meets an MFMA (not even as 0 * inf).
#include "attention_short.h"

namespace {

using namespace attn_short;

constexpr int LMAX = 512;    // longest sequence
constexpr int KCH = KIMG;    // keys per chunk: one LDS image
constexpr int QBLK = 128;    // query rows per workgroup (two 16-row strips per wave)
constexpr float LOG2E = 1.44269504088896340736f;

struct BiasK : AttnView<__bf16> {
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

  // the wave index and kend (below) as scalars: strip, chunk and per-tile tests are then uniform branches, not exec masks
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
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
  const int kend = __builtin_amdgcn_readfirstlane(kend_s);
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
    if (act[u]) load_q(qf[u], qp, p.qsl, q0, L, l16, g4);
    else qf[u][0] = qf[u][1] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
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
    // masked keys and rows past nk are zeros in the K and V images and -inf in the mask image
    const auto valid = [&](int r) { return r < nk && (!mrow || mrow[k0 + r] != 0.f); };
    stage_kv(Ks, Vt, kp, p.ksl, vp, p.vsl, k0, nk, tid, valid);
    if (tid < KCH) Km[tid] = valid(tid) ? 0.f : -INFINITY;
    __syncthreads();

#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (!act[u]) continue;
      const int q0 = qbase + 16 * (wave + 4 * u);
      // S tiles of the chunk: sacc[t][r] = S[q0 + 4 g4 + r][k0 + 16 t + l16]
      f32x4 sacc[NT];
      s_tiles(sacc, qf[u], Ks, nt, l16, g4);
      // scaled, biased, masked scores (exp2 domain) and the chunk's row maxima
      float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      int bi[4];                                    // bias index of key k0 + l16 for row r: key - q + L - 1, q clamped to L - 1
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = q0 + 4 * g4 + r;
        bi[r] = k0 + l16 - (q < L ? q : L - 1) + L - 1;
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
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
        const float mnew = fmaxf(mrun[u][r], row_max(mx[r]));
        muse[r] = mnew == -INFINITY ? 0.f : mnew;       // every key so far masked: exponent -inf - 0, weights exactly 0
        alpha[r] = exp2f(mrun[u][r] - muse[r]);         // first chunk: exp2(-inf) = 0
        mrun[u][r] = mnew;
      }
      float rs[4];
      write_p(pw, rs, sacc, muse, nt, l16, g4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        lrun[u][r] = lrun[u][r] * alpha[r] + rs[r];
#pragma unroll
        for (int db = 0; db < D / 16; ++db) oacc[u][db][r] *= alpha[r];
      }
      pv_acc(oacc[u], pw, Vt, nt, l16, g4);
    }
    __syncthreads();       // the chunk's K, V and mask images are free
  }

  // every row below L is stored; strips that start at or past kend never accumulated anything and come out as exact zeros
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int q0 = qbase + 16 * (wave + 4 * u);
    if (q0 >= L) continue;
    store_rows(p.o + (int64_t)b * p.osb + h * D, p.osl, oacc[u], q0, L, l16, g4,
               [&](int r) { return lrun[u][r] > 0.f ? 1.0f / lrun[u][r] : 0.f; });
  }
}

// ---- fp32 PARITY instantiation (never benchmarked): row_f32 over the valid keys.  A row with no valid key is zeros.
struct BiasF : AttnView<float> {
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
  const float* rb = p.rb + (int64_t)h * (2 * L - 1) + (L - 1 - i);
  const float* mrow = p.km ? p.km + (int64_t)b * L : nullptr;
  row_f32(p, b, h, i, L, [&](int j) { return mrow && mrow[j] == 0.f; },
          [&](float sdot, int j) { return (sdot * p.scale + rb[j]) * LOG2E; },
          [](float l_run) { return l_run > 0.f ? 1.0f / l_run : 0.f; });
}

}  // namespace

extern "C" int aptp_attention_bias(const AptpAttentionBiasParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->q && p->k && p->v && p->o && p->relbias, "attention_bias: null pointer");
  APTP_CHECK(p->B > 0 && p->heads > 0, "attention_bias: bad extents (B %d, heads %d)", p->B, p->heads);
  APTP_CHECK(p->L >= 1 && p->L <= LMAX, "attention_bias: L %d outside [1, %d]", p->L, LMAX);
  const int nqb = (p->L + QBLK - 1) / QBLK;
  APTP_CHECK((int64_t)p->B * p->heads * nqb < (1ll << 31), "attention_bias: B * heads too large");
  if (int rc = attn_check_view(p, "attention_bias", (int64_t)p->heads * D, "heads * 64")) return rc;
  APTP_CHECK(((uintptr_t)p->relbias % 4) == 0 && ((uintptr_t)p->key_mask % 4) == 0, "attention_bias: relbias / key_mask alignment");
  const dim3 grid((unsigned)(p->B * p->heads * nqb));
  if (p->io_f32) {
    BiasF k;
    k.fill(p); k.rb = p->relbias; k.km = p->key_mask;
    k.heads = p->heads; k.L = p->L; k.nqb = nqb; k.scale = p->scale;
    hipLaunchKernelGGL(attn_bias_f32_kernel, grid, dim3(QBLK), 0, (hipStream_t)stream, k);
  } else {
    BiasK k;
    k.fill(p); k.rb = p->relbias; k.km = p->key_mask;
    k.heads = p->heads; k.L = p->L; k.nqb = nqb; k.c = p->scale * LOG2E;
    hipLaunchKernelGGL(attn_bias_kernel, grid, dim3(256), 0, (hipStream_t)stream, k);
  }
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
