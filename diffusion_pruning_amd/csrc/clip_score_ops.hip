// The device path of the CLIP score (pdm/utils/clip_utils.py:141-263) outside the two towers:
//   aptp_image_patches_pil   OpenAI CLIP's preprocess -- Resize(S, BICUBIC) on a PIL image, CenterCrop(S), ToTensor, Normalize --
//                            on uint8 images, bit-exact with PIL's 8-bit resampler, and the unfold of the patch convolution;
//   aptp_eos_pool_ln         final_layer_norm of the one row per prompt that the text projection reads (the EOS row);
//   aptp_paired_cosine       cos(a_i, b_i) per pair and their fp64 sum in a fixed order.
#include "aptp_common.h"

namespace {

// PIL's ImagingResample for 8-bit images (Resample.c): coefficients in PRECISION_BITS = 32 - 8 - 2 fixed point, an int32
// accumulator that starts at one half, an arithmetic shift, a clamp to [0, 255]
constexpr int PIL_BITS = 22;

__device__ __forceinline__ int pil_clip8(int acc) {
  const int v = acc >> PIL_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

struct ResampleHK {
  const uint8_t* x; uint8_t* out;
  const int32_t* bounds; const int32_t* weights;
  int64_t total;              // B * H * W1
  int W, W1, kmax;
};

// horizontal pass: one thread per pixel (b, y, ox) of the scratch image, its three channels together
__global__ __launch_bounds__(256) void pil_resample_h_kernel(const ResampleHK p) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.total) return;
  const int ox = (int)(idx % p.W1);
  const int64_t row = idx / p.W1;                    // (b, y)
  int x0 = p.bounds[2 * ox], n = p.bounds[2 * ox + 1];
  // a table that does not belong to this image must not move a read outside the row
  x0 = x0 < 0 ? 0 : (x0 > p.W - 1 ? p.W - 1 : x0);
  n = n < 0 ? 0 : (n > p.kmax ? p.kmax : n);
  n = n > p.W - x0 ? p.W - x0 : n;
  const uint8_t* src = p.x + (row * p.W + x0) * 3;
  const int32_t* k = p.weights + (int64_t)ox * p.kmax;
  int a0 = 1 << (PIL_BITS - 1), a1 = a0, a2 = a0;
  for (int j = 0; j < n; ++j) {
    const int w = k[j];
    a0 += (int)src[3 * j] * w;
    a1 += (int)src[3 * j + 1] * w;
    a2 += (int)src[3 * j + 2] * w;
  }
  uint8_t* dst = p.out + idx * 3;
  dst[0] = (uint8_t)pil_clip8(a0);
  dst[1] = (uint8_t)pil_clip8(a1);
  dst[2] = (uint8_t)pil_clip8(a2);
}

struct PilPatchK {
  const uint8_t* src;         // [B, H, W1, 3]: the horizontal pass's output, or the input when the width does not change
  void* out; int64_t ldo, total;
  const int32_t* bounds; const int32_t* weights;     // vertical table, null when the height does not change
  int H, W1, kmax, top, left;
  int S, P, G, K, out_f32;
  float mean[3], std[3];
};

// vertical pass + centre crop + ToTensor + Normalize + unfold: one thread per output element, row (b, gy, gx), column
// k = (c, py, px) or padding (aptp_image_patches' layout)
__global__ __launch_bounds__(256) void pil_patches_kernel(const PilPatchK p) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.total) return;
  const int k = (int)(idx % p.ldo);
  const int64_t row = idx / p.ldo;
  float v = 0.f;
  if (k < p.K) {
    const int PP = p.P * p.P;
    const int c = k / PP, r = k - c * PP, py = r / p.P, px = r - py * p.P;
    const int gg = (int)(row % (p.G * p.G));
    const int64_t b = row / (p.G * p.G);
    const int gy = gg / p.G, gx = gg - gy * p.G;
    const int oy = gy * p.P + py + p.top, ox = gx * p.P + px + p.left;      // in the resized image
    const uint8_t* col = p.src + (b * p.H * p.W1 + ox) * 3 + c;
    const int64_t sy = (int64_t)p.W1 * 3;
    int u;
    if (p.bounds) {
      int y0 = p.bounds[2 * oy], n = p.bounds[2 * oy + 1];
      y0 = y0 < 0 ? 0 : (y0 > p.H - 1 ? p.H - 1 : y0);
      n = n < 0 ? 0 : (n > p.kmax ? p.kmax : n);
      n = n > p.H - y0 ? p.H - y0 : n;
      const int32_t* w = p.weights + (int64_t)oy * p.kmax;
      int acc = 1 << (PIL_BITS - 1);
      for (int j = 0; j < n; ++j) acc += (int)col[(y0 + j) * sy] * w[j];
      u = pil_clip8(acc);
    } else {
      u = col[oy * sy];
    }
    // ToTensor (uint8 -> fp32, an IEEE division by 255) and Normalize ((v - mean) / std), both in fp32 as torchvision does
    v = ((float)u / 255.0f - p.mean[c]) / p.std[c];
  }
  if (p.out_f32) reinterpret_cast<float*>(p.out)[idx] = v;
  else reinterpret_cast<__bf16*>(p.out)[idx] = (__bf16)v;
}

struct EosK {
  const int64_t* ids; const void* x; int64_t x_stride_b, x_stride_l;
  const float* gamma; const float* beta;
  float* out; void* out_act; int64_t ldo_act; int32_t* index_out;
  int B, L, C, mode, eos, x_f32, act_f32;
  float eps;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

constexpr int EOS_MAX_C = 2048;      // 64 lanes x 4 passes x 8 channels held in registers

// one wave per prompt: the pooling position from the ids, then a two-pass LayerNorm of that one row
__global__ __launch_bounds__(256) void eos_pool_ln_kernel(const EosK p) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= p.B) return;
  const int64_t* ids = p.ids + (int64_t)b * p.L;
  int at;
  if (p.mode == APTP_EOS_ARGMAX) {
    // first index of the largest id: (id, index) pairs ordered by larger id, then smaller index
    int64_t best = INT64_MIN;
    int bi = 0x7fffffff;
    for (int l = lane; l < p.L; l += 64) {
      const int64_t v = ids[l];
      if (v > best) { best = v; bi = l; }          // l ascends within a lane: the first of equals stays
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const int64_t ov = __shfl_xor(best, off);
      const int oi = __shfl_xor(bi, off);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    at = bi;
  } else {
    int bi = 0x7fffffff;
    for (int l = lane; l < p.L; l += 64)
      if (ids[l] == (int64_t)p.eos && l < bi) bi = l;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const int oi = __shfl_xor(bi, off);
      bi = oi < bi ? oi : bi;
    }
    at = bi == 0x7fffffff ? 0 : bi;                // no EOS in the row: index 0, as (ids == eos).int().argmax() gives
  }
  if (p.index_out && lane == 0) p.index_out[b] = at;

  const int64_t off = (int64_t)b * p.x_stride_b + (int64_t)at * p.x_stride_l;
  float v[4][8];
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = 8 * (lane + 64 * u);
    if (c < p.C) {
      if (p.x_f32) {
        const float* xr = reinterpret_cast<const float*>(p.x) + off + c;
        const float4 t0 = *reinterpret_cast<const float4*>(xr), t1 = *reinterpret_cast<const float4*>(xr + 4);
        v[u][0] = t0.x; v[u][1] = t0.y; v[u][2] = t0.z; v[u][3] = t0.w;
        v[u][4] = t1.x; v[u][5] = t1.y; v[u][6] = t1.z; v[u][7] = t1.w;
      } else {
        unpack_bf16x8(*reinterpret_cast<const uint4*>(reinterpret_cast<const __bf16*>(p.x) + off + c), v[u]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[u][e];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[u][e] = 0.f;
    }
  }
  const float mean = wave_sum(s) / (float)p.C;
  float vs = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (8 * (lane + 64 * u) < p.C) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = v[u][e] - mean; vs += d * d; }
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(vs) / (float)p.C + p.eps);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = 8 * (lane + 64 * u);
    if (c >= p.ldo_act && c >= p.C) continue;
    float y[8];
    if (c < p.C) {
      const float4 g0 = *reinterpret_cast<const float4*>(p.gamma + c), g1 = *reinterpret_cast<const float4*>(p.gamma + c + 4);
      const float4 b0 = *reinterpret_cast<const float4*>(p.beta + c), b1 = *reinterpret_cast<const float4*>(p.beta + c + 4);
      const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
      const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) y[e] = (v[u][e] - mean) * rstd * g[e] + bb[e];
      float4* dst = reinterpret_cast<float4*>(p.out + (int64_t)b * p.C + c);
      dst[0] = make_float4(y[0], y[1], y[2], y[3]);
      dst[1] = make_float4(y[4], y[5], y[6], y[7]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) y[e] = 0.f;      // columns [C, ldo_act) of the GEMM operand are zeros
    }
    if (p.out_act && c < p.ldo_act) {
      if (p.act_f32) {
        float4* dst = reinterpret_cast<float4*>(reinterpret_cast<float*>(p.out_act) + (int64_t)b * p.ldo_act + c);
        dst[0] = make_float4(y[0], y[1], y[2], y[3]);
        dst[1] = make_float4(y[4], y[5], y[6], y[7]);
      } else {
        *reinterpret_cast<uint4*>(reinterpret_cast<__bf16*>(p.out_act) + (int64_t)b * p.ldo_act + c) = pack_bf16x8(y);
      }
    }
  }
}

struct CosK { const float* a; int64_t lda; const float* b; int64_t ldb; float* cos_out; double* sum_out; int n, D, accumulate; };

// one wave per pair: lane-strided float4 reads of both rows, three butterfly sums (fixed order)
__global__ __launch_bounds__(256) void paired_cosine_kernel(const CosK p) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.n) return;
  const float* a = p.a + (int64_t)row * p.lda;
  const float* b = p.b + (int64_t)row * p.ldb;
  float ab = 0.f, aa = 0.f, bb = 0.f;
  for (int c = 4 * lane; c < p.D; c += 256) {
    const float4 s = *reinterpret_cast<const float4*>(a + c), t = *reinterpret_cast<const float4*>(b + c);
    ab += s.x * t.x + s.y * t.y + s.z * t.z + s.w * t.w;
    aa += s.x * s.x + s.y * s.y + s.z * s.z + s.w * s.w;
    bb += t.x * t.x + t.y * t.y + t.z * t.z + t.w * t.w;
  }
  ab = wave_sum(ab); aa = wave_sum(aa); bb = wave_sum(bb);
  if (lane == 0) p.cos_out[row] = ab / (sqrtf(aa) * sqrtf(bb));
}

// one workgroup: thread t adds cos[t], cos[t + 256], ... in fp64, then a tree over the 256 partials -- the same order every run
__global__ __launch_bounds__(256) void cosine_sum_kernel(const CosK p) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < p.n; i += 256) s += (double)p.cos_out[i];
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) *p.sum_out = p.accumulate ? *p.sum_out + red[0] : red[0];
}

// Python's round() of d / 2 for d >= 0: halves go to the even neighbour (torchvision's CenterCrop)
int round_half_even_div2(int d) {
  const int n = d / 2;
  return (d & 1) ? n + (n & 1) : n;
}

// window of PIL's bicubic filter for a resize in -> out: (int)ceil(2 * max(in / out, 1)) * 2 + 1 (precompute_coeffs' ksize)
int pil_bicubic_ksize(int in, int out) {
  double scale = (double)in / (double)out;
  if (scale < 1.0) scale = 1.0;
  const double support = 2.0 * scale;
  int c = (int)support;
  if ((double)c < support) ++c;
  return 2 * c + 1;
}

}  // namespace

extern "C" int aptp_image_patches_pil_size(int32_t H, int32_t W, int32_t S, int32_t* H1, int32_t* W1, int32_t* top, int32_t* left) {
  APTP_CHECK(H > 0 && W > 0 && S > 0 && H <= 16384 && W <= 16384 && S <= 16384,
             "image_patches_pil: bad extents (the shorter side of an image must not be 0; sizes at most 16384)");
  const int h1 = H <= W ? S : (int)((int64_t)S * H / W), w1 = W <= H ? S : (int)((int64_t)S * W / H);
  APTP_CHECK(h1 <= 65536 && w1 <= 65536, "image_patches_pil: aspect ratio too large (resized to %d x %d)", h1, w1);
  if (H1) *H1 = h1;
  if (W1) *W1 = w1;
  if (top) *top = round_half_even_div2(h1 - S);
  if (left) *left = round_half_even_div2(w1 - S);
  return APTP_OK;
}

extern "C" int aptp_image_patches_pil(const AptpImagePatchesPilParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->x && p->out, "image_patches_pil: null pointer");
  APTP_CHECK(p->B > 0 && p->P > 0 && p->P <= 256 && p->S > 0 && p->S % p->P == 0,
             "image_patches_pil: bad extents (S must be a positive multiple of P)");
  int32_t H1, W1, top, left;
  if (int rc = aptp_image_patches_pil_size(p->H, p->W, p->S, &H1, &W1, &top, &left)) return rc;
  const int K = 3 * p->P * p->P;
  APTP_CHECK(p->ldo == (int64_t)((K + 63) / 64) * 64, "image_patches_pil: ldo (%lld) must be ceil(3 P^2 / 64) * 64 = %d", (long long)p->ldo, (K + 63) / 64 * 64);
  for (int c = 0; c < 3; ++c) APTP_CHECK(p->std[c] > 0.f, "image_patches_pil: std must be positive");
  const bool horiz = W1 != p->W, vert = H1 != p->H;
  if (horiz) {
    APTP_CHECK(p->xbounds && p->xweights && p->scratch, "image_patches_pil: the width changes (%d -> %d): xbounds, xweights and scratch are needed", p->W, W1);
    APTP_CHECK(p->xk >= pil_bicubic_ksize(p->W, W1) && p->xk <= 65536,
               "image_patches_pil: window of %d taps is wider than the horizontal table's declared maximum %d", pil_bicubic_ksize(p->W, W1), p->xk);
    APTP_CHECK(((uintptr_t)p->xbounds % 4) == 0 && ((uintptr_t)p->xweights % 4) == 0, "image_patches_pil: pointer alignment");
  }
  if (vert) {
    APTP_CHECK(p->ybounds && p->yweights, "image_patches_pil: the height changes (%d -> %d): ybounds and yweights are needed", p->H, H1);
    APTP_CHECK(p->yk >= pil_bicubic_ksize(p->H, H1) && p->yk <= 65536,
               "image_patches_pil: window of %d taps is wider than the vertical table's declared maximum %d", pil_bicubic_ksize(p->H, H1), p->yk);
    APTP_CHECK(((uintptr_t)p->ybounds % 4) == 0 && ((uintptr_t)p->yweights % 4) == 0, "image_patches_pil: pointer alignment");
  }
  APTP_CHECK(((uintptr_t)p->out % 16) == 0, "image_patches_pil: pointer alignment");
  const int G = p->S / p->P;
  const int64_t rows = (int64_t)p->B * G * G;
  APTP_CHECK(rows < (1ll << 31) && rows * p->ldo < (1ll << 39) && (int64_t)p->B * p->H * W1 < (1ll << 37), "image_patches_pil: too large");
  if (horiz) {
    ResampleHK h;
    h.x = p->x; h.out = reinterpret_cast<uint8_t*>(p->scratch); h.bounds = p->xbounds; h.weights = p->xweights;
    h.total = (int64_t)p->B * p->H * W1; h.W = p->W; h.W1 = W1; h.kmax = p->xk;
    hipLaunchKernelGGL(pil_resample_h_kernel, dim3((unsigned)((h.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h);
    APTP_LAUNCH_CHECK();
  }
  PilPatchK k;
  k.src = horiz ? reinterpret_cast<const uint8_t*>(p->scratch) : p->x;
  k.out = p->out; k.ldo = p->ldo; k.total = rows * p->ldo;
  k.bounds = vert ? p->ybounds : nullptr; k.weights = vert ? p->yweights : nullptr;
  k.H = p->H; k.W1 = W1; k.kmax = p->yk; k.top = top; k.left = left;
  k.S = p->S; k.P = p->P; k.G = G; k.K = K; k.out_f32 = p->out_f32 ? 1 : 0;
  for (int c = 0; c < 3; ++c) { k.mean[c] = p->mean[c]; k.std[c] = p->std[c]; }
  hipLaunchKernelGGL(pil_patches_kernel, dim3((unsigned)((k.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}

extern "C" int aptp_eos_pool_ln(const AptpEosPoolLnParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->ids && p->x && p->gamma && p->beta && p->out, "eos_pool_ln: null pointer");
  APTP_CHECK(p->B > 0 && p->L > 0 && p->C > 0 && p->C % 8 == 0 && p->C <= EOS_MAX_C,
             "eos_pool_ln: bad extents (C must be a multiple of 8, <= %d)", EOS_MAX_C);
  APTP_CHECK(p->eos_mode == APTP_EOS_ARGMAX || p->eos_mode == APTP_EOS_FIRST, "eos_pool_ln: eos_mode %d (0 = argmax, 1 = first_eos)", p->eos_mode);
  APTP_CHECK(p->x_stride_l >= p->C && p->x_stride_l % 8 == 0 && p->x_stride_b >= 0 && p->x_stride_b % 8 == 0,
             "eos_pool_ln: x strides must be multiples of 8, the row stride >= C");
  APTP_CHECK(!p->out_act || (p->ldo_act >= p->C && p->ldo_act % 8 == 0 && p->ldo_act <= EOS_MAX_C),
             "eos_pool_ln: ldo_act (%lld) must be >= C, a multiple of 8 and <= %d", (long long)p->ldo_act, EOS_MAX_C);
  APTP_CHECK(p->eps > 0.f, "eos_pool_ln: eps must be positive");
  APTP_CHECK(((uintptr_t)p->ids % 8) == 0 && ((uintptr_t)p->x % 16) == 0 && ((uintptr_t)p->gamma % 16) == 0 && ((uintptr_t)p->beta % 16) == 0 &&
             ((uintptr_t)p->out % 16) == 0 && ((uintptr_t)p->out_act % 16) == 0 && ((uintptr_t)p->index_out % 4) == 0, "eos_pool_ln: pointer alignment");
  EosK k;
  k.ids = p->ids; k.x = p->x; k.x_stride_b = p->x_stride_b; k.x_stride_l = p->x_stride_l; k.gamma = p->gamma; k.beta = p->beta;
  k.out = p->out; k.out_act = p->out_act; k.ldo_act = p->out_act ? p->ldo_act : 0; k.index_out = p->index_out;
  k.B = p->B; k.L = p->L; k.C = p->C; k.mode = p->eos_mode; k.eos = p->eos_token_id; k.x_f32 = p->x_f32 ? 1 : 0; k.act_f32 = p->act_f32 ? 1 : 0;
  k.eps = p->eps;
  hipLaunchKernelGGL(eos_pool_ln_kernel, dim3((unsigned)((p->B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}

extern "C" int aptp_paired_cosine(const AptpPairedCosineParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->a && p->b && p->cos_out && p->sum_out, "paired_cosine: null pointer");
  APTP_CHECK(p->n > 0 && p->D > 0 && p->D % 4 == 0, "paired_cosine: bad extents (D must be a multiple of 4)");
  APTP_CHECK(p->lda >= p->D && p->lda % 4 == 0 && p->ldb >= p->D && p->ldb % 4 == 0, "paired_cosine: row strides must be >= D and multiples of 4");
  APTP_CHECK(((uintptr_t)p->a % 16) == 0 && ((uintptr_t)p->b % 16) == 0 && ((uintptr_t)p->cos_out % 4) == 0 && ((uintptr_t)p->sum_out % 8) == 0,
             "paired_cosine: pointer alignment");
  CosK k;
  k.a = p->a; k.lda = p->lda; k.b = p->b; k.ldb = p->ldb; k.cos_out = p->cos_out; k.sum_out = p->sum_out; k.n = p->n; k.D = p->D;
  k.accumulate = p->accumulate ? 1 : 0;
  hipLaunchKernelGGL(paired_cosine_kernel, dim3((unsigned)((p->n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  hipLaunchKernelGGL(cosine_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
