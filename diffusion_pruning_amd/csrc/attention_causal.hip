// Causal self-attention of short sequences with head width 64: the self-attention of CLIP's text encoder
// (transformers CLIPAttention with the causal mask and no padding mask; SD-2.1: 16 heads, L = 77, scale 1/8):
// o = softmax(q k^T * scale + causal) v, key j > query i weighted exactly 0, fp32 softmax statistics, bf16 in / out.
//
// One workgroup (4 waves) per (sample, head).  L <= 128, so the whole K (row-major) and V (transposed) of the pair sit in LDS
// (K rows and V columns past L are zeros).  Wave w takes the 16-query strips w, w + 4, ...; for strip s:
//   S[16 q][16 keys]   key tiles 0..s only (tiles right of the diagonal tile hold no key <= any query of the strip and are
//                      never computed), mfma_f32_16x16x32_bf16 over the 64 channels: Q fragments from global memory, K
//                      fragments from LDS; all s + 1 tiles stay in registers (at most 8 x 4 fp32 per lane);
//   softmax            keys above the diagonal (and past L) get score -inf before the row maximum, so they never reach it and
//                      contribute exp2(-inf) = 0 to the row sum; key 0 is valid for every row, the maximum is finite;
//   O[16 q][64 c]     += P V: P (bf16) goes through the wave's LDS strip, 32 keys per MFMA; when s + 1 is odd the tile
//                      after the diagonal is written as zeros so the last 32-key step adds nothing from it.
// Query rows past L (the end of the last strip) load row L - 1 and store nothing.
#include "attention_short.h"

namespace {

using namespace attn_short;

constexpr int LMAX = KIMG;   // longest sequence: K and V of a (sample, head) pair are one LDS image

struct CausalK : AttnView<__bf16> {
  int heads, L;
  float c;   // scale * log2(e)
};

__global__ __launch_bounds__(256) void attn_causal_kernel(const CausalK p) {
  __shared__ __attribute__((aligned(16))) __bf16 Ks[LMAX * KLD];
  __shared__ __attribute__((aligned(16))) __bf16 Vt[D * TLD];
  __shared__ __attribute__((aligned(16))) __bf16 Ps[4 * 16 * TLD];

  // the wave index as a scalar: the strip index s and every per-tile test (t <= s) are then uniform branches, not exec masks
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, g4 = lane >> 4;
  const int b = blockIdx.x / p.heads, h = blockIdx.x - b * p.heads;
  const int L = p.L;

  const __bf16* qp = p.q + (int64_t)b * p.qsb + h * D;
  const __bf16* kp = p.k + (int64_t)b * p.ksb + h * D;
  const __bf16* vp = p.v + (int64_t)b * p.vsb + h * D;

  stage_kv(Ks, Vt, kp, p.ksl, vp, p.vsl, 0, L, tid, [&](int r) { return r < L; });
  __syncthreads();

  __bf16* const pw = Ps + wave * 16 * TLD;
  const int nstrips = (L + 15) >> 4;
  for (int s = wave; s < nstrips; s += 4) {
    const int q0 = 16 * s;
    bf16x8 qf[2];
    load_q(qf, qp, p.qsl, q0, L, l16, g4);
    // S tiles 0..s: sacc[t][r] = S[q0 + 4 g4 + r][16 t + l16]
    f32x4 sacc[NT];
    s_tiles(sacc, qf, Ks, s + 1, l16, g4);
    // masked, scaled scores and the row maxima
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t <= s) {
        const int key = 16 * t + l16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int q = q0 + 4 * g4 + r;
          const float sv = (key <= q && key < L) ? sacc[t][r] * p.c : -INFINITY;
          sacc[t][r] = sv;
          mx[r] = fmaxf(mx[r], sv);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) mx[r] = row_max(mx[r]);
    float rs[4];
    write_p(pw, rs, sacc, mx, s + 1, l16, g4);
    f32x4 oacc[D / 16];
#pragma unroll
    for (int db = 0; db < D / 16; ++db) oacc[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
    pv_acc(oacc, pw, Vt, s + 1, l16, g4);
    store_rows(p.o + (int64_t)b * p.osb + h * D, p.osl, oacc, q0, L, l16, g4, [&](int r) { return 1.0f / rs[r]; });
  }
}

// ---- fp32 PARITY instantiation (never benchmarked): row_f32 over the keys 0..i of row i
struct CausalF : AttnView<float> {
  int heads, L;
  float c;
};

__global__ __launch_bounds__(LMAX) void attn_causal_f32_kernel(const CausalF p) {
  const int i = threadIdx.x;
  const int b = blockIdx.x / p.heads, h = blockIdx.x - b * p.heads;
  if (i >= p.L) return;
  row_f32(p, b, h, i, i + 1, [](int) { return false; }, [&](float sdot, int) { return sdot * p.c; },
          [](float l_run) { return 1.0f / l_run; });
}

}  // namespace

extern "C" int aptp_attention_causal(const AptpAttentionCausalParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->q && p->k && p->v && p->o, "attention_causal: null pointer");
  APTP_CHECK(p->B > 0 && p->heads > 0, "attention_causal: bad extents (B %d, heads %d)", p->B, p->heads);
  APTP_CHECK(p->L >= 1 && p->L <= LMAX, "attention_causal: L %d outside [1, %d]", p->L, LMAX);
  APTP_CHECK((int64_t)p->B * p->heads < (1ll << 31), "attention_causal: B * heads too large");
  if (int rc = attn_check_view(p, "attention_causal", (int64_t)p->heads * D, "heads * 64")) return rc;
  const float c = p->scale * 1.44269504088896340736f;
  const dim3 grid((unsigned)(p->B * p->heads));
  if (p->io_f32) {
    CausalF k;
    k.fill(p); k.heads = p->heads; k.L = p->L; k.c = c;
    hipLaunchKernelGGL(attn_causal_f32_kernel, grid, dim3(LMAX), 0, (hipStream_t)stream, k);
  } else {
    CausalK k;
    k.fill(p); k.heads = p->heads; k.L = p->L; k.c = c;
    hipLaunchKernelGGL(attn_causal_kernel, grid, dim3(256), 0, (hipStream_t)stream, k);
  }
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
