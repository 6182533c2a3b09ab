// The K loop that conv_gemm_dma_kernel / conv3x3_halo_kernel (conv_gemm.hip), conv_lean_kernel (conv_lean.hip) and
// lin_gemm_kernel (lin_gemm.hip) share: the counted vmcnt wait, the three ring schedules, the host-sized next-launch prefetch
// and the split-K slab store.  Included by conv_gemm_core.h (after KParams); every function is inlined into the kernels of the
// including file.
// What stays in each kernel is what differs between them: address generation (issue_tile), the prologue -- the first D tiles,
// the epilogue inputs requested behind them, the first wait and the first barrier -- and the epilogue.
// The MFMA block stays there too (the `compute` lambda: swizzled fragment reads + MF x NF x 2 MFMAs), although it is the same
// text in every kernel.  Hoisted into a function here -- pointers by value or by reference, generic or LDS-typed -- the
// registers and the v_mfma count stay what they are, but the compiler's wait-count pass no longer tells the fragment reads
// from the LDS-DMA still in flight and puts an s_waitcnt vmcnt(0) in front of them, in 3 of the 6 conv_lean_kernel
// instantiations and at 40 more places in lin_gemm.hip: the ring is drained at every K-step.  Measured on the headline
// forward: 210.5 -> 203.6 steps/s with the conv_lean.hip change alone, 210.5 -> 209.6 with the lin_gemm.hip one.
#pragma once

namespace aptp_cg {

typedef __attribute__((address_space(3))) void* lds_ptr;
typedef const __attribute__((address_space(1))) void* gbl_ptr;

template <int MF, int NF>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[MF][NF]) {
#pragma unroll
  for (int i = 0; i < MF; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// Counted wait of the ring: the tile(s) of the next step have landed, DW newer tiles stay in flight (vmcnt retires in order).
// A wave issues NLD_LO LDS-DMA instructions per tile, or NLD_HI if it takes part in a partial last row pass (`hi`,
// wave-uniform): each waits on its own count.  !full (prologue shorter than the ring, or the loop's tail) and DW == 0 drain.
// Younger requests of the prologue (epilogue inputs, statistics) only make a counted wait stricter for the operand tiles.
template <int NLD_LO, int NLD_HI, int DW>
__device__ __forceinline__ void ring_wait(bool hi, bool full) {
  static_assert(DW >= 0 && NLD_HI * DW <= 63, "vmcnt immediate");
  if constexpr (DW > 0) {
    if (full) {
      if (hi) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD_HI * DW) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD_LO * DW) : "memory");
      return;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// The three schedules below run n K-tiles through a ring of STAGES stages after the kernel's prologue has requested the first
// min(n, D) tiles into stages 0.., waited for the first step's tile(s) and met one barrier.  issue(stage) requests the next
// tile of the kernel's K walk, compute(stage) multiplies one, wait(full) is the kernel's ring_wait.  The waits are counted and
// the barriers raw (s_barrier has no implicit vmcnt(0)), so tiles stay in flight across every barrier.

// STAGES-deep ring, D = STAGES - 1 tiles in flight across the barriers: the operand round trip (~1-2k cycles) is several K-steps
// long at these tile sizes, so one tile ahead is not enough.
//   iteration kt: issue tile kt+D into stage (kt+D)%S == (kt-1)%S (last read before the previous barrier),
//                 compute stage kt%S, wait until tile kt+1 has landed (D-1 newer tiles stay in flight), barrier.
template <int STAGES, int D, class Issue, class Compute, class Wait>
__device__ __forceinline__ void kloop_ring(int n, Issue& issue, Compute& compute, Wait& wait) {
  static_assert(D == STAGES - 1 && D >= 1, "ring");
  int cur = 0, nxt = D % STAGES;         // stage of tile kt, stage of tile kt+D
  for (int kt = 0; kt < n; ++kt) {
    const bool more = kt + D < n;
    if (more) issue(nxt);
    compute(cur);
    asm volatile("" ::: "memory");
    wait(more);                                                // tail: everything still in flight is needed soon
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // this wave's LDS reads of `cur` are done
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    cur = cur + 1 == STAGES ? 0 : cur + 1;
    nxt = nxt + 1 == STAGES ? 0 : nxt + 1;
  }
}

// Two K-tiles per synchronisation point (an effective K-step of 128): iteration i issues tiles 2i+D and 2i+D+1 into the two
// stages read in iteration i-1, runs the MFMAs of tiles 2i and 2i+1, waits until tiles 2i+2 and 2i+3 have landed (D-2 newer
// tiles stay in flight; D == 2: plain double buffering of 128-wide steps) and meets ONE barrier: half the s_waitcnt / s_barrier
// stops of the ring above.
template <int STAGES, int D, class Issue, class Compute, class Wait>
__device__ __forceinline__ void kloop_ku2(int n, Issue& issue, Compute& compute, Wait& wait) {
  static_assert(STAGES >= 4 && STAGES % 2 == 0 && D == STAGES - 2, "pairs of stages");
  int cur = 0, nxt = D;
  for (int kt = 0; kt < n; kt += 2) {
    const int ni = n - (kt + D);          // tiles left to request: two per iteration while >= 2
    if (ni >= 1) issue(nxt);
    if (ni >= 2) issue(nxt + 1);
    compute(cur);
    if (kt + 1 < n) compute(cur + 1);
    asm volatile("" ::: "memory");
    wait(ni >= 2);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    cur = cur + 2 == STAGES ? 0 : cur + 2;
    nxt = nxt + 2 == STAGES ? 0 : nxt + 2;
  }
}

// Ping-pong schedule (8 waves = two groups of four, grp = wave >> 2; waves w and w+4 share a SIMD).  Every K-step is two slots
// separated by workgroup barriers: in slot L a wave issues its share of the LDS-DMA for tile k+D, in slot C it reads the
// fragments of tile k from LDS and runs the MFMAs.  Group 1 runs one slot behind group 0, so on every SIMD one wave drives the
// matrix pipe (and the LDS read port) while the other drives the load path.  In the lockstep loops the three engines take
// turns (in-kernel stamps, 128x160 tile: DMA issue 490-550, LDS reads + MFMA 470-525, waits 400-550 cycles per K-step).
//   RAW: a wave waits for its own DMA rows of tile k+1 at the end of C(k); group 0 reads tile k+1 two barriers later,
//        group 1 three.
//   WAR: tile k+D lands in the stage of tile k+D-S = k-2 (S = D+2), last read by group 1 in its C(k-2), which ends one
//        barrier before group 0's L(k) starts.  (S = D+1 would let group 0's DMA overwrite the stage group 1 is still
//        reading in the same slot.)
template <int STAGES, int D, class Issue, class Compute, class Wait>
__device__ __forceinline__ void kloop_pp(int n, int grp, Issue& issue, Compute& compute, Wait& wait) {
  static_assert(STAGES >= 3 && D == STAGES - 2, "ping-pong: ring of >= 3 stages");
  if (grp == 1) {                       // stagger: group 1 starts one slot late
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  int cur = 0, nxt = D % STAGES;
  for (int kt = 0; kt < n; ++kt) {
    // ---- slot L(kt): the load path ----
    const bool more = kt + D < n;
    if (more) issue(nxt);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    // ---- slot C(kt): LDS reads + MFMAs ----
    __builtin_amdgcn_s_setprio(1);
    compute(cur);
    __builtin_amdgcn_s_setprio(0);
    asm volatile("" ::: "memory");
    wait(more);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    cur = cur + 1 == STAGES ? 0 : cur + 1;
    nxt = nxt + 1 == STAGES ? 0 : nxt + 1;
  }
  if (grp == 0) {                       // group 0 pairs group 1's last barrier
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
}

// Next launch's weights towards this XCD's L2, slice bounds from the host (set_prefetch_slices: no division on the device): one
// dword per 64-byte line into a scratch row, by LDS-DMA -- no VGPRs, nothing waits on them but the counted vmcnt of the main loop.
// Call it BEFORE the operand tiles are requested: an LDS-DMA into the scratch row that is still pending when the K loop starts
// makes the compiler's wait-count pass put a vmcnt(0) in front of the loop's fragment reads (it cannot tell the scratch row
// from the operand stages), which serialises the ring.
__device__ __forceinline__ void prefetch_hosted(const KParams& p, int tid, int nt, unsigned* scratch) {
  if (!p.pf_ptr) return;
  const int xcd = blockIdx.x & 7;
  const int x0 = (int)(((int64_t)p.pf_lines * xcd) >> 3), x1 = (int)(((int64_t)p.pf_lines * (xcd + 1)) >> 3);
  const int l0 = x0 + (int)(blockIdx.x >> 3) * p.pf_per;
  const int l1 = l0 + p.pf_per < x1 ? l0 + p.pf_per : x1;
  for (int l = l0 + tid; l < l1; l += nt)
    __builtin_amdgcn_global_load_lds((gbl_ptr)(p.pf_ptr + (int64_t)l * 64), (lds_ptr)scratch, 4, 0, 0);
}

// host side of prefetch_hosted for a launch of `grid` workgroups: the lines of the xcd-th eighth of the buffer are dealt to the
// workgroups of that XCD (as aptp_prefetch_slice does on the device)
inline void set_prefetch_slices(KParams& k, int grid) {
  k.pf_lines = 0; k.pf_per = 0;
  if (!k.pf_ptr) return;
  const int nper = (grid + 7) >> 3;                   // workgroups per XCD under round-robin dispatch (upper bound)
  k.pf_lines = (int)(k.pf_bytes >> 6);
  const int per_xcd = (k.pf_lines + 7) >> 3;
  k.pf_per = (per_xcd + nper - 1) / nper;
  if (k.pf_per < 1) k.pf_per = 1;
}

// Split-K with a reduce launch: this workgroup's fp32 accumulators to slab kz of the workspace, in the accumulator layout
//   acc[i][j][r] = out[m_base + i*16 + frow][n_base + j*16 + fq*4 + r]
template <int MF, int NF>
__device__ __forceinline__ void store_splitk_slab(const KParams& p, const f32x4 (&acc)[MF][NF], int kz, int m_base, int n_base, int frow,
                                                  int fq) {
  float* ws = p.ws + (int64_t)kz * p.M * p.ws_ld;
#pragma unroll
  for (int i = 0; i < MF; ++i) {
    const int m = m_base + i * 16 + frow;
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      const int n = n_base + j * 16 + fq * 4;
      if (n >= p.N) continue;
      float4 o; o.x = acc[i][j][0]; o.y = acc[i][j][1]; o.z = acc[i][j][2]; o.w = acc[i][j][3];
      *reinterpret_cast<float4*>(ws + (int64_t)m * p.ws_ld + n) = o;
    }
  }
}

}  // namespace aptp_cg
