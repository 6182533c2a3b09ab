// aptp_mmd_rbf: the MMD statistic of CMMD (cmmd-pytorch/distance.py:28-64) without the n x n, n x m and m x m matrices.
//
//   launch 1  squared norms of the rows of x and y (the diagonal of the Gram matrices in the reference), one wave per row;
//   launch 2  one workgroup per 128 x 128 tile of one of the three kernel matrices (xx, yy, xy in one grid): the Gram tile with
//             exact-fp32 MFMAs (v_mfma_f32_16x16x4_f32, operands through LDS in K-steps of 32, the next step's global loads in
//             flight during the multiplies), then d^2 = |a|^2 + |b|^2 - 2 a.b and 1 - k = -expm1(-gamma d^2) per element, summed
//             per lane, per wave (butterfly) and per workgroup in a fixed order: ONE fp32 partial per tile;
//   launch 3  one workgroup adds the partials of each matrix in fp64 (thread-strided, then a fixed tree) and forms the statistic.
// 4 waves as 2 x 2, wave tile 64 x 64 = 4 x 4 fragments: 64 MFMAs (2048 cycles) per 8 LDS reads of 16 bytes: MFMA-bound.
#include "aptp_common.h"

namespace {

constexpr int TM = 128, BKF = 32, PITCH = BKF + 4;    // pitch 36 floats: the 16 rows of a fragment read 16 distinct 16-byte slots

struct MmdK {
  const float* x; int64_t ldx; const float* y; int64_t ldy;
  int n, m, D, tn, tm;           // tn / tm: 128-row tiles of x / y
  float gamma, scale;
  float* sq;                     // [n + m] squared norms
  float* part;                   // [tn*tn + tm*tm + tn*tm] tile partials: xx, yy, xy
  double* out;
};

__global__ __launch_bounds__(256) void mmd_sqnorm_kernel(const MmdK p) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.n + p.m) return;
  const float* r = row < p.n ? p.x + (int64_t)row * p.ldx : p.y + (int64_t)(row - p.n) * p.ldy;
  float a = 0.f;
  for (int c = 4 * lane; c < p.D; c += 256) {
    const float4 t = *reinterpret_cast<const float4*>(r + c);
    a += t.x * t.x + t.y * t.y + t.z * t.z + t.w * t.w;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off);
  if (lane == 0) p.sq[row] = a;
}

__global__ __launch_bounds__(256) void mmd_tile_kernel(const MmdK p) {
  __shared__ __attribute__((aligned(16))) float As[TM * PITCH], Bs[TM * PITCH];
  __shared__ float wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  // which matrix, which tile
  int t = blockIdx.x;
  const int nxx = p.tn * p.tn, nyy = p.tm * p.tm;
  const float *a, *b, *sqa, *sqb;
  int64_t lda, ldb;
  int na, nb, ta, tb;
  if (t < nxx) { a = b = p.x; lda = ldb = p.ldx; na = nb = p.n; sqa = sqb = p.sq; ta = t / p.tn; tb = t - ta * p.tn; }
  else if (t < nxx + nyy) { t -= nxx; a = b = p.y; lda = ldb = p.ldy; na = nb = p.m; sqa = sqb = p.sq + p.n; ta = t / p.tm; tb = t - ta * p.tm; }
  else { t -= nxx + nyy; a = p.x; b = p.y; lda = p.ldx; ldb = p.ldy; na = p.n; nb = p.m; sqa = p.sq; sqb = p.sq + p.n; ta = t / p.tm; tb = t - ta * p.tm; }
  const int a0 = ta * TM, b0 = tb * TM;

  // global -> registers -> LDS: thread (row = tid >> 3 (+ 32 i), float4 column = tid & 7), 4 passes per operand
  const int lr = tid >> 3, lc = (tid & 7) * 4;
  float4 ra[4], rb[4];
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = lr + 32 * i, k = k0 + lc;
      const bool kon = k < p.D;                        // (D is a multiple of 4: a float4 is inside the row or outside it)
      ra[i] = (kon && a0 + r < na) ? *reinterpret_cast<const float4*>(a + (int64_t)(a0 + r) * lda + k) : make_float4(0.f, 0.f, 0.f, 0.f);
      rb[i] = (kon && b0 + r < nb) ? *reinterpret_cast<const float4*>(b + (int64_t)(b0 + r) * ldb + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<float4*>(As + (lr + 32 * i) * PITCH + lc) = ra[i];
      *reinterpret_cast<float4*>(Bs + (lr + 32 * i) * PITCH + lc) = rb[i];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15, fq = lane >> 4;
  const int nk = (p.D + BKF - 1) / BKF;
  gload(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();                                   // the previous step's fragment reads are done
    lstore();
    __syncthreads();
    if (kt + 1 < nk) gload((kt + 1) * BKF);
    // exact-fp32 MFMA 16x16x4: a lane supplies one value per operand, k = lane >> 4.  The float4 at columns 16 h + 4 fq of a row
    // feeds element e to the (h, e)-th of eight MFMAs, the same column for both operands: the sum over the 32 columns is complete
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4 af[4], bf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const f32x4*>(As + (wm * 64 + i * 16 + frow) * PITCH + h * 16 + fq * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) bf[j] = *reinterpret_cast<const f32x4*>(Bs + (wn * 64 + j * 16 + frow) * PITCH + h * 16 + fq * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j][e], af[i][e], acc[i][j], 0, 0, 0);
    }
  }

  // acc[i][j][e] = a-row (wm 64 + 16 i + frow) . b-row (wn 64 + 16 j + 4 fq + e)
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ia = a0 + wm * 64 + i * 16 + frow;
    const float na2 = ia < na ? sqa[ia] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int jb = b0 + wn * 64 + j * 16 + fq * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (ia < na && jb + e < nb) {
          const float d2 = (na2 + sqb[jb + e]) - 2.0f * acc[i][j][e];
          s += -expm1f(-p.gamma * d2);
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) wsum[wave] = s;
  __syncthreads();
  if (tid == 0) p.part[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

__global__ __launch_bounds__(256) void mmd_finish_kernel(const MmdK p) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const int cnt[3] = {p.tn * p.tn, p.tm * p.tm, p.tn * p.tm};
  const double den[3] = {(double)p.n * p.n, (double)p.m * p.m, (double)p.n * p.m};
  double mean[3];
  int base = 0;
  for (int q = 0; q < 3; ++q) {
    double a = 0.0;
    for (int i = tid; i < cnt[q]; i += 256) a += (double)p.part[base + i];
    base += cnt[q];
    __syncthreads();
    red[tid] = a;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
      if (tid < w) red[tid] += red[tid + w];
      __syncthreads();
    }
    mean[q] = red[0] / den[q];
  }
  if (tid == 0) {
    // k_xx + k_yy - 2 k_xy with k = 1 - (1 - k)
    p.out[0] = (double)p.scale * (2.0 * mean[2] - mean[0] - mean[1]);
    p.out[1] = mean[0]; p.out[2] = mean[1]; p.out[3] = mean[2];
  }
}

inline int64_t tiles_of(int n) { return (n + TM - 1) / TM; }
inline int64_t sq_floats(int n, int m) { return ((int64_t)n + m + 3) / 4 * 4; }

}  // namespace

extern "C" int64_t aptp_mmd_rbf_workspace_bytes(int32_t n, int32_t m) {
  if (n < 1 || m < 1) return 0;
  const int64_t tn = tiles_of(n), tm = tiles_of(m);
  return 4 * (sq_floats(n, m) + tn * tn + tm * tm + tn * tm);
}

extern "C" int aptp_mmd_rbf(const AptpMmdRbfParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->x && p->y && p->workspace && p->out, "mmd_rbf: null pointer");
  APTP_CHECK(p->n >= 1 && p->m >= 1 && p->D >= 4 && p->D % 4 == 0, "mmd_rbf: bad extents (n, m >= 1, D a positive multiple of 4)");
  APTP_CHECK(p->ldx >= p->D && p->ldx % 4 == 0 && p->ldy >= p->D && p->ldy % 4 == 0, "mmd_rbf: row strides must be >= D and multiples of 4");
  APTP_CHECK(p->sigma > 0.f && p->sigma == p->sigma && p->scale == p->scale, "mmd_rbf: sigma must be positive");
  APTP_CHECK(((uintptr_t)p->x % 16) == 0 && ((uintptr_t)p->y % 16) == 0 && ((uintptr_t)p->workspace % 16) == 0 && ((uintptr_t)p->out % 8) == 0,
             "mmd_rbf: pointer alignment");
  const int64_t tn = tiles_of(p->n), tm = tiles_of(p->m);
  const int64_t tiles = tn * tn + tm * tm + tn * tm;
  APTP_CHECK(tiles < (1ll << 31) && (int64_t)p->n + p->m < (1ll << 31), "mmd_rbf: too many rows");
  MmdK k;
  k.x = p->x; k.ldx = p->ldx; k.y = p->y; k.ldy = p->ldy; k.n = p->n; k.m = p->m; k.D = p->D; k.tn = (int)tn; k.tm = (int)tm;
  k.gamma = 1.0f / (2.0f * p->sigma * p->sigma); k.scale = p->scale;
  k.sq = reinterpret_cast<float*>(p->workspace); k.part = k.sq + sq_floats(p->n, p->m); k.out = p->out;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mmd_sqnorm_kernel, dim3((unsigned)((p->n + p->m + 3) / 4)), dim3(256), 0, s, k);
  hipLaunchKernelGGL(mmd_tile_kernel, dim3((unsigned)tiles), dim3(256), 0, s, k);
  hipLaunchKernelGGL(mmd_finish_kernel, dim3(1), dim3(256), 0, s, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
