// Seeded normal noise on the device:
//   aptp_philox_normal   out[r, e] = scale z (+ base[r, e]),  z the project's counter-based normal stream (philox_normal.h) of
//                        (seeds[r], draw, offset + e), or -- raw -- the uint32 word behind it.  The seeds, a draw increment and a
//                        scale factor are read from device memory, so one captured launch follows a denoise loop.
// Memory-bound and tiny: one lane per aligned block of four elements (one Philox evaluation, one 16-byte store; 8 bytes for
// bf16), single elements -- the same statements on the one lane they need -- for a row's head and tail and wherever an address is
// not aligned.  No reductions, no atomics: bit-equal from run to run and from capture to replay.
#include "aptp_common.h"
#include "philox_normal.h"

// base + scale z is a multiply, then an add: two roundings, as the tensor expression has them
#pragma clang fp contract(off)

namespace {

struct PhiloxK {
  void* out; const float* base;
  const int64_t* seeds; const int64_t* draw_dev; const float* scale_dev;
  int64_t n, offset, draw;
  int64_t head, nblk;            // per row: head single elements, nblk blocks of four, the rest single again
  float scale;
  int kind;                      // APTP_PHILOX_F32 / BF16 / RAW
};

template <int KIND>
__device__ __forceinline__ void store1(const PhiloxK& p, int64_t i, float v, uint32_t w) {
  if constexpr (KIND == APTP_PHILOX_F32) reinterpret_cast<float*>(p.out)[i] = v;
  else if constexpr (KIND == APTP_PHILOX_BF16) reinterpret_cast<__bf16*>(p.out)[i] = (__bf16)v;
  else reinterpret_cast<uint32_t*>(p.out)[i] = w;
}

template <int KIND>
__global__ __launch_bounds__(256) void philox_normal_kernel(const PhiloxK p) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t tail0 = p.head + 4 * p.nblk;                 // first element of the tail
  if (k >= p.head + p.nblk + (p.n - tail0)) return;
  const int64_t row = blockIdx.y;
  const uint64_t seed = (uint64_t)p.seeds[row];
  const uint64_t draw = (uint64_t)p.draw + (p.draw_dev ? (uint64_t)p.draw_dev[0] : 0ull);
  const float scale = p.scale_dev ? p.scale * p.scale_dev[0] : p.scale;
  const bool vec = k >= p.head && k < p.head + p.nblk;
  const int64_t e = k < p.head ? k : (vec ? p.head + 4 * (k - p.head) : tail0 + (k - p.head - p.nblk));
  const uint64_t g = (uint64_t)p.offset + (uint64_t)e;
  const int64_t i = row * p.n + e;
  uint32_t x[4];
  aptp_philox_block(seed, draw, g >> 2, x);
  if (vec) {                                                  // (g & 3 == 0 and every address 16-byte aligned: see the host side)
    if constexpr (KIND == APTP_PHILOX_RAW) {
      *reinterpret_cast<uint4*>(reinterpret_cast<uint32_t*>(p.out) + i) = make_uint4(x[0], x[1], x[2], x[3]);
    } else {
      float z[4], v[4];
      aptp_philox_normals4(x, z);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = scale * z[j];
      if (p.base) {
        const float4 bv = *reinterpret_cast<const float4*>(p.base + i);
        v[0] = bv.x + v[0]; v[1] = bv.y + v[1]; v[2] = bv.z + v[2]; v[3] = bv.w + v[3];
      }
      if constexpr (KIND == APTP_PHILOX_F32) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.out) + i) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        uint2 q;
        q.x = pack_bf16x2(v[0], v[1]);
        q.y = pack_bf16x2(v[2], v[3]);
        *reinterpret_cast<uint2*>(reinterpret_cast<__bf16*>(p.out) + i) = q;
      }
    }
  } else {
    const int lane = (int)(g & 3);
    const uint32_t w = lane == 0 ? x[0] : (lane == 1 ? x[1] : (lane == 2 ? x[2] : x[3]));
    float v = 0.f;
    if constexpr (KIND != APTP_PHILOX_RAW) {
      v = scale * aptp_philox_normal1(x, lane);
      if (p.base) v = p.base[i] + v;
    }
    store1<KIND>(p, i, v, w);
  }
}

}  // namespace

extern "C" int aptp_philox_normal(const AptpPhiloxNormalParams* p, aptp_stream_t stream) {
  APTP_CHECK(p, "philox_normal: null pointer");
  APTP_CHECK(p->out && p->seeds_dev, "philox_normal: null pointer (out, seeds_dev)");
  APTP_CHECK(p->out_kind == APTP_PHILOX_F32 || p->out_kind == APTP_PHILOX_BF16 || p->out_kind == APTP_PHILOX_RAW,
             "philox_normal: unknown out_kind %d", p->out_kind);
  APTP_CHECK(p->b >= 1 && p->b <= 65535 && p->n >= 1 && p->n <= (1ll << 40) / p->b, "philox_normal: bad extents b = %d, n = %lld",
             p->b, (long long)p->n);
  APTP_CHECK(p->offset >= 0 && p->offset <= (1ll << 62), "philox_normal: offset %lld outside [0, 2^62]", (long long)p->offset);
  APTP_CHECK(p->draw >= 0, "philox_normal: draw %lld is negative", (long long)p->draw);
  APTP_CHECK(p->out_kind != APTP_PHILOX_RAW || (!p->base && !p->scale_dev), "philox_normal: the raw words take no base and no scale");
  const int esz = p->out_kind == APTP_PHILOX_BF16 ? 2 : 4;
  APTP_CHECK(((uintptr_t)p->out % esz) == 0 && ((uintptr_t)p->base % 4) == 0 && ((uintptr_t)p->seeds_dev % 8) == 0 &&
             ((uintptr_t)p->draw_dev % 8) == 0 && ((uintptr_t)p->scale_dev % 4) == 0, "philox_normal: pointer alignment");
  PhiloxK k;
  k.out = p->out; k.base = p->base; k.seeds = p->seeds_dev; k.draw_dev = p->draw_dev; k.scale_dev = p->scale_dev;
  k.n = p->n; k.offset = p->offset; k.draw = p->draw; k.scale = p->scale; k.kind = p->out_kind;
  // a lane owns a whole block where the block starts at a multiple of four of offset + e AND the four elements sit at an
  // aligned address in every row: the head runs up to the first such element, and rows must keep the alignment
  const int64_t head = (4 - (p->offset & 3)) & 3;
  const uintptr_t oalign = 4 * (uintptr_t)esz;
  bool aligned = head < p->n && (((uintptr_t)p->out + (uintptr_t)head * esz) % oalign) == 0 &&
                 (!p->base || (((uintptr_t)p->base + (uintptr_t)head * 4) % 16) == 0) && (p->b == 1 || p->n % 4 == 0);
  k.head = aligned ? head : 0;
  k.nblk = aligned ? (p->n - head) / 4 : 0;
  const int64_t threads = k.head + k.nblk + (p->n - k.head - 4 * k.nblk);
  const int64_t blocks = (threads + 255) / 256;
  APTP_CHECK(blocks < (1ll << 31), "philox_normal: too many elements");
  const dim3 grid((unsigned)blocks, (unsigned)p->b), block(256);
  if (p->out_kind == APTP_PHILOX_F32)
    hipLaunchKernelGGL(philox_normal_kernel<APTP_PHILOX_F32>, grid, block, 0, (hipStream_t)stream, k);
  else if (p->out_kind == APTP_PHILOX_BF16)
    hipLaunchKernelGGL(philox_normal_kernel<APTP_PHILOX_BF16>, grid, block, 0, (hipStream_t)stream, k);
  else
    hipLaunchKernelGGL(philox_normal_kernel<APTP_PHILOX_RAW>, grid, block, 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
