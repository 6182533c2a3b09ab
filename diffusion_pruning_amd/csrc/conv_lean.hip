// Lean implicit-GEMM kernel for the 3x3 convolutions of the masked U-Net (ResnetBlock2D conv1 / conv2 with the fused 1x1
// shortcut, Downsample2D, Upsample2D -- reference call sites pdm/models/unet/blocks.py:331,362 and unet.py:375-475).  The 54
// 3x3 launches of the headline step are 38 % of its time (profiles/r4_bench_per_step_breakdown.txt), and round 4's SQ counters
// (profiles/r4_tile_pmc.txt, tile 34) show a wave of conv_gemm_dma_kernel issuing ~55 VALU + ~58 SALU instructions per
// 20-MFMA K-step: set_tap recomputes bounds, multiplies and 64-bit row pointers at every tap change, and every LDS-DMA pass pays
// a 64-bit pointer add.  This is the diet lin_gemm.hip applied to the linear layers, for the convolutions:
//   * tap table: in the prologue each lane computes, once per staged row, the 32-bit byte offset of all 9 taps and of the x2
//     entry (stride, nearest / zero-insertion upsampling and the padding folded in; 0x80000000 marks a tap that reads zeros).
//     The operands are read with buffer loads to LDS (buffer_load_dwordx4 ... lds): scalar resource + 32-bit per-lane offset +
//     scalar offset, the channel step (+128 B) and the weights' K-tile both in the scalar offset.  A tap change is a register
//     select, a channel step changes one SGPR, and a sentinel offset lies past the resource's extent, so the load returns zeros
//     -- the same zero rows conv_gemm_dma_kernel streams from its zero page;
//   * everything requested up front: next-launch prefetch first (slice bounds from the host), then the first D operand
//     stages, then -- before anything waits -- the epilogue's bias, row bias, gate, beta correction and residual inputs
//     (LeanEpiIn, in the transposed layout the epilogue uses them in);
//   * one-pass transposed epilogue (lean_epilogue in conv_gemm_core.h).
// Same tiles, wave grids, LDS image (XOR-swizzled 128-byte rows, swizzle applied to the source chunk), MFMA mapping, K order
// (taps, channel steps, x2 segment), ring / ping-pong schedules, split-K slab layout, in-kernel combine and XCD decode orders
// as conv_gemm_dma_kernel: for the same tile and split the output is bit-identical to it (tests/test_conv_lean_gpu.py).
// fp32 I/O, GEGLU, folded LayerNorm, row statistics and the depth lerp (soft depth gates: training graphs only; see
// lean_epilogue) stay with the general kernel (aptp_conv_lean_eligible).
#include "conv_gemm_core.h"

namespace {
using namespace aptp_cg;

constexpr unsigned ZERO_OFF = 0x80000000u;   // past every operand's extent (< 2^31 bytes, checked on the host): reads zeros
constexpr int NTAB = 10;                     // 9 filter taps + the x2 entry

// 16 bytes per lane, global -> LDS (buffer_load_dwordx4 ... lds): resource + 32-bit lane offset + scalar offset, lane l lands at
// lds + 16 l.  (Device pass only: the host pass of this builtin inside the kernel's lambdas silently drops the kernel's launch stub.)
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, __bf16* lds, unsigned voff, int soff) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr)lds, 16, voff, soff, 0, 0);
#endif
}

template <int BM, int BN, int WM, int WN, int STAGES, bool PP, int KU>
__global__ __launch_bounds__(WM * WN * 64) void conv_lean_kernel(const KParams p) {
  constexpr int NW = WM * WN, NT = NW * 64, RPP = NT / 8;     // RPP: tile rows one LDS-DMA pass of the workgroup covers
  constexpr int WTM = BM / WM, WTN = BN / WN, MF = WTM / 16, NF = WTN / 16;
  constexpr int A_PASS = BM / RPP, B_PASS = (BN + RPP - 1) / RPP;
  constexpr int B_FULL = BN / RPP, NLD_LO = A_PASS + B_FULL, NLD_HI = A_PASS + B_PASS;
  static_assert(NW == 4 || NW == 8, "4 or 8 waves");
  static_assert(BM % RPP == 0 && WTM % 16 == 0 && WTN % 16 == 0 && BN % 8 == 0, "tile shape");
  static_assert(NW * 16 * (WTN + 4) * 4 <= STAGES * (BM + BN) * BK * 2, "epilogue transpose buffer");

  __shared__ __attribute__((aligned(16))) __bf16 smem[STAGES * (BM + BN) * BK];
  __shared__ unsigned pf_scratch[64];
  __bf16* As = smem;
  __bf16* Bs = smem + STAGES * BM * BK;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
  int tm, tn, kz;
  decode_block(p, tiles_m, tiles_n, tm, tn, kz);
  const int m0 = tm * BM, n0 = tn * BN;
  const int kt_begin = p.fd_sk.div(p.nK * kz);
  const int kt_end = p.fd_sk.div(p.nK * (kz + 1));

  // ---- next launch's weights towards this XCD's L2: requested FIRST, ahead of the operand stages (see prefetch_hosted) ----
  prefetch_hosted(p, tid, NT, pf_scratch);

  // ---- tap table: byte offset of every tap of this lane's staged rows (source chunk schunk already included) ----
  const int rowbase = tid >> 3;
  const unsigned schunk = (unsigned)((tid & 7) ^ ((rowbase >> 1) & 7));   // source chunk that lands in this lane's LDS slot
  unsigned tab[A_PASS][NTAB];
#pragma unroll
  for (int i = 0; i < A_PASS; ++i) {
    const int m = m0 + rowbase + RPP * i;
    if (m < p.M) {
      const int b = p.fd_hw.div(m), rem = m - b * p.HW;
      const int oy = p.fd_wout.div(rem), ox = rem - oy * p.Wout;
      const int iy0 = oy * p.stride - 1, ix0 = ox * p.stride - 1, pix0 = b * p.Hin * p.Win;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        int iy = iy0 + t / 3, ix = ix0 + t % 3;
        const bool ok = (unsigned)iy < (unsigned)p.HinE && (unsigned)ix < (unsigned)p.WinE && !(p.zins & (iy | ix));
        iy >>= p.ups; ix >>= p.ups;
        tab[i][t] = ok ? ((unsigned)(pix0 + iy * p.Win + ix) * (unsigned)p.ldx) * 2u + schunk * 16u : ZERO_OFF;   // < 2^31
      }
      tab[i][9] = p.x2 ? ((unsigned)m * (unsigned)p.ldx2) * 2u + schunk * 16u : ZERO_OFF;
    } else {
#pragma unroll
      for (int t = 0; t < NTAB; ++t) tab[i][t] = ZERO_OFF;     // rows past M multiply zeros (never stored)
    }
  }
  unsigned boff[B_PASS];
#pragma unroll
  for (int i = 0; i < B_PASS; ++i) {
    int n = n0 + rowbase + RPP * i;
    n = n < p.N ? n : p.N - 1;                                  // columns past N accumulate garbage that is never stored
    boff[i] = (unsigned)(n * (unsigned)p.Ktot) * 2u + schunk * 16u;
  }
  // the padding of the last channel step: a per-lane predicate, once
  const bool tail_bad = (int)((p.ncc - 1) * BK + schunk * 8) >= p.Cin;
  const bool tail_bad2 = (int)((p.ncc2 - 1) * BK + schunk * 8) >= p.Cin2;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(p.x), 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t x2r =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(p.x2 ? p.x2 : p.x), 0, p.x2 ? p.x2_bytes : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(p.w), 0, p.w_bytes, 0x00020000);

  // K walk of the NEXT tile to request: global K-tile l_kt = (tap l_tap, channel step l_cc); l_tap == 9: the x2 segment
  int l_kt = kt_begin, l_tap = 0, l_cc = kt_begin;
  if (kt_begin != 0) {                    // (workgroup-uniform; only K-slices past the first pay the division)
    l_tap = kt_begin / p.ncc;
    if (l_tap > 9) l_tap = 9;
    l_cc = kt_begin - l_tap * p.ncc;
  }
  // The table is consumed in order (tap 0, 1, ..., 8, x2): a tap change shifts it down by one entry -- register moves with
  // compile-time indices, so it stays in VGPRs (a runtime-indexed select is folded into an indexed load from scratch memory).
  // tab[i][0] is always the current tap's offset.
  auto next_tap = [&]() {
#pragma unroll
    for (int i = 0; i < A_PASS; ++i)
#pragma unroll
      for (int t = 0; t + 1 < NTAB; ++t) tab[i][t] = tab[i][t + 1];
  };
  for (int t = 0; t < l_tap; ++t) next_tap();     // (a K-slice that starts past tap 0)

  auto issue_tile = [&](int stage) {
    const bool seg2 = l_tap == 9;                                          // wave-uniform
    const int ncur = seg2 ? p.ncc2 : p.ncc;
    const bool pad = l_cc == ncur - 1 && (seg2 ? tail_bad2 : tail_bad);   // this lane's chunk of the last channel step
    const int sa = __builtin_amdgcn_readfirstlane(l_cc * (BK * 2));
    const int sb = __builtin_amdgcn_readfirstlane(l_kt * (BK * 2));
#pragma unroll
    for (int i = 0; i < A_PASS; ++i) {
      __bf16* dst = As + (stage * BM + wave * 8 + RPP * i) * BK;          // wave-uniform; lane l lands at dst + l * 16 B
      if (seg2) dma16(x2r, dst, pad ? ZERO_OFF : tab[i][0], sa);
      else dma16(xr, dst, pad ? ZERO_OFF : tab[i][0], sa);
    }
#pragma unroll
    for (int i = 0; i < B_PASS; ++i) {
      if (wave * 8 + RPP * i < BN) {                                       // wave-uniform: the last pass may be partial
        __bf16* dst = Bs + (stage * BN + wave * 8 + RPP * i) * BK;
        dma16(wr, dst, boff[i], sb);
      }
    }
    ++l_kt;
    if (++l_cc == ncur) {                 // next tap (wave-uniform branch)
      l_cc = 0;
      if (l_tap < 9) {
        ++l_tap;
        next_tap();
      }
    }
  };

  f32x4 acc[MF][NF];
  zero_acc(acc);
  const int frow = lane & 15, fq = lane >> 4;
  auto compute = [&](int stage) {         // (local on purpose: see the note on the MFMA block in conv_gemm_kloop.h)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 af[MF], wf[NF];
#pragma unroll
      for (int i = 0; i < MF; ++i) {
        const int r = wm * WTM + i * 16 + frow;
        af[i] = *reinterpret_cast<const bf16x8*>(As + (stage * BM + r) * BK + ((s * 4 + fq) ^ ((r >> 1) & 7)) * 8);
      }
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int r = wn * WTN + j * 16 + frow;
        wf[j] = *reinterpret_cast<const bf16x8*>(Bs + (stage * BN + r) * BK + ((s * 4 + fq) ^ ((r >> 1) & 7)) * 8);
      }
#pragma unroll
      for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
    }
  };

  // ---- prologue: the first D stages, then the epilogue's inputs (un-split launches; a split's combining workgroup asks later) ----
  constexpr int D = PP ? STAGES - 2 : (KU == 2 ? STAGES - 2 : STAGES - 1);
  constexpr int DW = KU == 2 ? D - 2 : D - 1;                      // tiles still in flight at a wait of the loop
  static_assert(STAGES >= 2 && D >= 1, "ring");
  static_assert(!PP || NW == 8, "ping-pong: 8 waves");
  static_assert(KU == 1 || !PP, "two K-tiles per barrier: ring schedule only");
  const bool hi = (NLD_HI != NLD_LO) && (wave * 8 + RPP * (B_PASS - 1) < BN);   // wave-uniform: this wave takes the partial pass
  auto wait_ring = [&](bool full) { ring_wait<NLD_LO, NLD_HI, DW>(hi, full); };
  const int n = kt_end - kt_begin;
  const int pre = n < D ? n : D;
  for (int t = 0; t < pre; ++t) issue_tile(t);
  LeanEpiIn<WTM, WTN> ein;
  if (p.split_k == 1) lean_epi_load<WTM, WTN>(p, m0, n0, wm, wn, lane, ein);

  if (n > 0) {
    // (the epilogue inputs requested above are younger than the operand stages: they only make the first counted wait stricter)
    wait_ring(pre == D);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if constexpr (PP) kloop_pp<STAGES, D>(n, wave >> 2, issue_tile, compute, wait_ring);
    else if constexpr (KU == 2) kloop_ku2<STAGES, D>(n, issue_tile, compute, wait_ring);
    else kloop_ring<STAGES, D>(n, issue_tile, compute, wait_ring);
  }

  // ---- split-K: slabs for the reduce launch, or the in-kernel combine ----
  if (p.split_k > 1 && p.counters) {
    if (!splitk_combine<NT, MF, NF>(p, acc, tm * tiles_n + tn, kz, tid, reinterpret_cast<int*>(smem))) return;
    lean_epi_load<WTM, WTN>(p, m0, n0, wm, wn, lane, ein);
  } else if (p.split_k > 1) {
    store_splitk_slab(p, acc, kz, m0 + wm * WTM, n0 + wn * WTN, frow, fq);
    return;
  }
  __syncthreads();                        // every wave is done reading the operand stages
  lean_epilogue<MF, NF, WTM, WTN>(p, acc, m0, n0, wm, wn, lane, ein, reinterpret_cast<float*>(smem) + wave * 16 * (WTN + 4));
}

template <int BM, int BN, int WM, int WN, int STAGES, bool PP, int KU>
void launch_lean(KParams k, hipStream_t s) {
  const int grid = ((k.M + BM - 1) / BM) * ((k.N + BN - 1) / BN) * k.split_k;
  set_prefetch_slices(k, grid);
  hipLaunchKernelGGL((conv_lean_kernel<BM, BN, WM, WN, STAGES, PP, KU>), dim3(grid), dim3(WM * WN * 64), 0, s, k);
}

}  // namespace

namespace aptp_cg {

// Which launches the lean kernel takes: 3x3 / pad-1 convolutions (stride 1 or 2, any upsampling, optional x2 segment) with the
// coalesced bf16 epilogue, on the tiles of the headline step's 3x3 launches.  Everything else stays with conv_gemm_dma_kernel,
// tile 19 (128x160, 8 waves, 2 stages) included: its 74 KB ring leaves room for two workgroups per CU, i.e. 128 VGPRs per wave,
// and the up-front epilogue inputs do not fit that (measured 0.74-0.81x; requested after the K loop, with the epilogue
// spilling, 0.86-1.02x).
bool aptp_conv_lean_eligible(const KParams& k, int tile) {
  if (k.KH != 3 || k.KW != 3 || k.pad != 1 || (k.stride != 1 && k.stride != 2)) return false;
  if (k.io_f32 || k.out_f32 || !k.epi16 || k.ln_stats || k.rstat_out || k.depth) return false;
  if (k.act != APTP_ACT_NONE && k.act != APTP_ACT_SILU) return false;
  if (k.Nout < 8 || k.ncc < 1) return false;
  return tile_known(tile) && kTiles[tile].c3;        // the rows of conv_gemm_tiles.h flagged C3
}

// The lean kernel of a C3 row, with the row's own geometry, ring and schedule.  A row without the flag instantiates nothing.
template <bool C3, int BM, int BN, int WM, int WN, int STAGES, bool PP, int KU>
static bool launch_lean_row(const KParams& k, hipStream_t s) {
  if constexpr (C3) launch_lean<BM, BN, WM, WN, STAGES, PP, KU>(k, s);
  return C3;
}

int aptp_launch_conv_lean(const KParams& k, int tile, hipStream_t s) {
  switch (tile) {
#define X(NAME, FAMILY, BM, BN, WM, WN, STAGES, KU, KS, LIN, C3) case APTP_TILE_##NAME: \
    if (launch_lean_row<C3 != 0, BM, BN, WM, WN, STAGES, TileFamily::FAMILY == TileFamily::PP, KU>(k, s)) return APTP_OK; break;
    APTP_CONV_GEMM_TILES(X)
#undef X
  }
  aptp_set_error("conv_lean: tile %d has no lean instantiation", tile); return APTP_EINVAL;
}

}  // namespace aptp_cg
