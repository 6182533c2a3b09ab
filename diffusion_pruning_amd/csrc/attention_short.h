// What the attention kernels outside the U-Net share.  All three entry points (attention_causal.hip, attention_bias.hip,
// attention_wide.hip) take q, k, v, o as strided views: the view, its fill and its host-side check are here once.  The two
// short-sequence kernels of head width 64 (causal: CLIP text; relative bias: MPNet) are built from the same blocks -- K / V
// staging into LDS, the S tiles of a 16-query strip, the P strip, P V and the row store, plus the fp32 parity row -- which
// live in attn_short below; each kernel keeps what really differs: which scores are -inf, what is added to them, and whether
// the softmax is one-shot or online over chunks.
#pragma once
#include "aptp_common.h"

// q, k, v, o of one launch: element (b, l, c) at ptr + b * sb + l * sl + c
template <typename T>
struct AttnView {
  const T* q; int64_t qsb, qsl;
  const T* k; int64_t ksb, ksl;
  const T* v; int64_t vsb, vsl;
  T* o; int64_t osb, osl;
  template <typename P>     // P: any of the public attention parameter blocks
  void fill(const P* p) {
    q = (const T*)p->q; qsb = p->q_stride_b; qsl = p->q_stride_l;
    k = (const T*)p->k; ksb = p->k_stride_b; ksl = p->k_stride_l;
    v = (const T*)p->v; vsb = p->v_stride_b; vsl = p->v_stride_l;
    o = (T*)p->o; osb = p->o_stride_b; osl = p->o_stride_l;
  }
};

// The view checks of an attention entry point `name`, after its own null and extent checks: scale, and per tensor the row
// stride (>= min_row, printed as min_row_text), the batch stride and the 16-byte alignment that the vector loads rely on.
template <typename P>
static int attn_check_view(const P* p, const char* name, int64_t min_row, const char* min_row_text) {
  APTP_CHECK(p->scale > 0.f && p->scale < 1e30f, "%s: scale must be positive and finite", name);
  const int64_t sl[4] = {p->q_stride_l, p->k_stride_l, p->v_stride_l, p->o_stride_l};
  const int64_t sb[4] = {p->q_stride_b, p->k_stride_b, p->v_stride_b, p->o_stride_b};
  const void* ptr[4] = {p->q, p->k, p->v, p->o};
  const int vec = p->io_f32 ? 4 : 8;        // elements per 16 bytes
  for (int i = 0; i < 4; ++i) {
    APTP_CHECK(sl[i] >= min_row && sl[i] % vec == 0, "%s: row stride %lld must be >= %s and a multiple of %d", name,
               (long long)sl[i], min_row_text, vec);
    APTP_CHECK(sb[i] >= 0 && sb[i] % vec == 0, "%s: batch stride %lld must be a non-negative multiple of %d", name,
               (long long)sb[i], vec);
    APTP_CHECK(((uintptr_t)ptr[i] % 16) == 0, "%s: pointers must be 16-byte aligned", name);
  }
  return APTP_OK;
}

namespace attn_short {

constexpr int D = 64;          // head width
constexpr int KIMG = 128;      // keys of one LDS image of K and V
constexpr int NT = KIMG / 16;  // its 16-key tiles
constexpr int KLD = 72;        // K image row stride (bf16): 144 B rows keep the 16-byte fragment reads aligned
constexpr int TLD = 136;       // V^T and P image row stride (bf16): 272 B rows

// K -> Ks[key][c], V -> Vt[c][key] for the keys k0 + r, r in [0, n) rounded up to 32, by the 256 threads of the workgroup;
// rows with !valid(r) -- past n, or masked -- are zeros (P = 0 must not meet a non-finite V, not even as 0 * inf)
template <typename Valid>
__device__ __forceinline__ void stage_kv(__bf16* Ks, __bf16* Vt, const __bf16* kp, int64_t ksl, const __bf16* vp, int64_t vsl,
                                         int k0, int n, int tid, Valid valid) {
  const int np = (n + 31) & ~31;
  for (int e = tid; e < np * (D / 8); e += 256) {
    const int r = e >> 3, c0 = (e & 7) * 8;
    uint4 kq = make_uint4(0u, 0u, 0u, 0u), vq = make_uint4(0u, 0u, 0u, 0u);
    if (valid(r)) {
      kq = *reinterpret_cast<const uint4*>(kp + (int64_t)(k0 + r) * ksl + c0);
      vq = *reinterpret_cast<const uint4*>(vp + (int64_t)(k0 + r) * vsl + c0);
    }
    *reinterpret_cast<uint4*>(Ks + r * KLD + c0) = kq;
    union { uint4 q; __bf16 x[8]; } u;
    u.q = vq;
#pragma unroll
    for (int j = 0; j < 8; ++j) Vt[(c0 + j) * TLD + r] = u.x[j];
  }
}

// Q fragments of the strip at q0 (A operand: lane holds Q[q0 + l16][32 ks + 8 g4 + j]); rows past L load row L - 1
__device__ __forceinline__ void load_q(bf16x8 (&qf)[2], const __bf16* qp, int64_t qsl, int q0, int L, int l16, int g4) {
  const int qr = q0 + l16 < L ? q0 + l16 : L - 1;
  const __bf16* src = qp + (int64_t)qr * qsl + 8 * g4;
  qf[0] = *reinterpret_cast<const bf16x8*>(src);
  qf[1] = *reinterpret_cast<const bf16x8*>(src + 32);
}

// S tiles 0 .. nt - 1 of a strip against the K image: sacc[t][r] = S[row 4 g4 + r][image key 16 t + l16]; the tiles from nt
// on are never computed and stay zero
__device__ __forceinline__ void s_tiles(f32x4 (&sacc)[NT], const bf16x8 (&qf)[2], const __bf16* Ks, int nt, int l16, int g4) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    sacc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (t < nt) {
      const __bf16* kr = Ks + (16 * t + l16) * KLD + 8 * g4;
      sacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[0], *reinterpret_cast<const bf16x8*>(kr), sacc[t], 0, 0, 0);
      sacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[1], *reinterpret_cast<const bf16x8*>(kr + 32), sacc[t], 0, 0, 0);
    }
  }
}

// maximum / sum over the 16 lanes that hold one row of a tile (rows 4 g4 + r; a row's 16 lanes share g4)
__device__ __forceinline__ float row_max(float v) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off);
  return v;
}

// P = exp2(S - m) (masked: exactly 0) of tiles 0 .. nt - 1 as bf16 into the wave's strip pw of LDS, the row sums in fp32 into
// rs; when nt is odd, tile nt is written as zeros so that the last 32-key step of P V adds nothing from it
__device__ __forceinline__ void write_p(__bf16* pw, float (&rs)[4], const f32x4 (&sacc)[NT], const float (&m)[4], int nt,
                                        int l16, int g4) {
#pragma unroll
  for (int r = 0; r < 4; ++r) rs[r] = 0.f;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the previous strip's P reads are done
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t < nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pr = exp2f(sacc[t][r] - m[r]);
        rs[r] += pr;
        pw[(4 * g4 + r) * TLD + 16 * t + l16] = (__bf16)pr;
      }
    } else if (t == nt && (nt & 1)) {
#pragma unroll
      for (int r = 0; r < 4; ++r) pw[(4 * g4 + r) * TLD + 16 * t + l16] = (__bf16)0.f;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) rs[r] = row_sum(rs[r]);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // P of this strip is visible to the whole wave
  __builtin_amdgcn_wave_barrier();
}

// O += P V over the 32-key steps that cover nt tiles: A = P[l16][32 kc + 8 g4 + j], B = V[32 kc + 8 g4 + j][16 db + l16] = Vt row
__device__ __forceinline__ void pv_acc(f32x4 (&oacc)[D / 16], const __bf16* pw, const __bf16* Vt, int nt, int l16, int g4) {
  const int nkc = (nt + 1) >> 1;
  for (int kc = 0; kc < nkc; ++kc) {
    const bf16x8 pf = *reinterpret_cast<const bf16x8*>(pw + l16 * TLD + 32 * kc + 8 * g4);
#pragma unroll
    for (int db = 0; db < D / 16; ++db) {
      const bf16x8 vf = *reinterpret_cast<const bf16x8*>(Vt + (16 * db + l16) * TLD + 32 * kc + 8 * g4);
      oacc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, oacc[db], 0, 0, 0);
    }
  }
}

// oacc[db][r] = O[q0 + 4 g4 + r][16 db + l16] times inv(r) -> the head's rows of o (op: its row 0), rows past L not stored
template <typename Inv>
__device__ __forceinline__ void store_rows(__bf16* op, int64_t osl, const f32x4 (&oacc)[D / 16], int q0, int L, int l16, int g4,
                                           Inv inv) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + 4 * g4 + r;
    if (q >= L) continue;
    const float iv = inv(r);
    __bf16* dst = op + (int64_t)q * osl + l16;
#pragma unroll
    for (int db = 0; db < D / 16; ++db) dst[16 * db] = (__bf16)(oacc[db][r] * iv);
  }
}

// ---- fp32 PARITY row (never benchmarked): exact-fp32 arithmetic, one thread per query row i of pair (b, h), the keys j in
// [0, nkeys) without skip(j) in order through the exp2-domain online softmax, score(q . k_j, j) in that domain; K and V rows
// are read from global memory (the active lanes of a wave read the same row at the same time).  o = acc * inv(row sum).
template <typename Skip, typename Score, typename Inv>
__device__ __forceinline__ void row_f32(const AttnView<float>& p, int b, int h, int i, int nkeys, Skip skip, Score score, Inv inv) {
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
  for (int j = 0; j < nkeys; ++j) {
    if (skip(j)) continue;
    const float* kr = kb + (int64_t)j * p.ksl;
    float sdot = 0.f;
#pragma unroll
    for (int d = 0; d < D; d += 4) {
      const float4 t = *reinterpret_cast<const float4*>(kr + d);
      sdot += q[d] * t.x; sdot += q[d + 1] * t.y; sdot += q[d + 2] * t.z; sdot += q[d + 3] * t.w;
    }
    const float sv = score(sdot, j);
    const float m_new = fmaxf(m_run, sv);
    const float alpha = exp2f(m_run - m_new);            // -inf on the first key -> 0
    const float pr = exp2f(sv - m_new);
    l_run = l_run * alpha + pr;
    m_run = m_new;
    const float* vr = vb + (int64_t)j * p.vsl;
#pragma unroll
    for (int d = 0; d < D; d += 4) {
      const float4 t = *reinterpret_cast<const float4*>(vr + d);
      // acc * alpha + pr * v with the second product fused, spelled out: left to contraction, the compiler is free to fuse
      // either product, and the two forms round differently
      acc[d] = __builtin_fmaf(pr, t.x, acc[d] * alpha); acc[d + 1] = __builtin_fmaf(pr, t.y, acc[d + 1] * alpha);
      acc[d + 2] = __builtin_fmaf(pr, t.z, acc[d + 2] * alpha); acc[d + 3] = __builtin_fmaf(pr, t.w, acc[d + 3] * alpha);
    }
  }
  const float iv = inv(l_run);
  float* dst = p.o + (int64_t)b * p.osb + (int64_t)i * p.osl + h * D;
#pragma unroll
  for (int d = 0; d < D; d += 4) *reinterpret_cast<float4*>(dst + d) = make_float4(acc[d] * iv, acc[d + 1] * iv, acc[d + 2] * iv, acc[d + 3] * iv);
}

}  // namespace attn_short
