// The two ends of the CLIP image encoder and the row normalisation of its embeddings:
//   aptp_image_patches   bicubic resize (F.interpolate semantics) + mean / std normalisation + the unfold of the patch
//                        convolution, images in, GEMM operand rows out (cmmd-pytorch/embedding.py:26-30, 57-65);
//   aptp_vit_embed_ln    [class_embedding | patch GEMM output] + position_embedding, pre_layrnorm, one rounding to the stream
//                        (transformers CLIPVisionEmbeddings + CLIPVisionTransformer.pre_layrnorm);
//   aptp_l2_normalize    rows of an fp32 matrix divided by their norm (embedding.py:70, pdm/utils/clip_utils.py:160-161).
#include "aptp_common.h"

namespace {

struct PatchK {
  const float* x; void* out; int64_t ldo, total;
  int H, W, S, P, G, K, nchw, resize, out_f32;
  int64_t sb, sy, sx, sc;            // element strides of x by sample, row, column, channel
  float scale_y, scale_x;
  float mean[3], std[3];
};

// F.interpolate(mode="bicubic", align_corners=False): source coordinate scale * (dst + 0.5) - 0.5 (not clamped), the four taps
// at floor - 1 .. floor + 2 with indices clamped to the image, Keys' kernel with A = -0.75
__device__ __forceinline__ void cubic_coeffs(float t, float c[4]) {
  const float A = -0.75f;
  const float x0 = t + 1.0f, x3 = (1.0f - t) + 1.0f, x2 = 1.0f - t;
  c[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
  c[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
  c[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
  c[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// one thread per output element: row (b, gy, gx), column k = (c, py, px) or padding
__global__ __launch_bounds__(256) void image_patches_kernel(const PatchK p) {
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
    const int oy = gy * p.P + py, ox = gx * p.P + px;
    const float* xb = p.x + b * p.sb + c * p.sc;
    if (!p.resize) {
      v = xb[oy * p.sy + ox * p.sx];
    } else {
      const float ry = p.scale_y * ((float)oy + 0.5f) - 0.5f, rx = p.scale_x * ((float)ox + 0.5f) - 0.5f;
      const float fy = floorf(ry), fx = floorf(rx);
      const int iy = (int)fy, ix = (int)fx;
      float cy[4], cx[4];
      cubic_coeffs(ry - fy, cy);
      cubic_coeffs(rx - fx, cx);
      int64_t ofx[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) ofx[j] = clampi(ix - 1 + j, p.W - 1) * p.sx;
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float* xr = xb + clampi(iy - 1 + i, p.H - 1) * p.sy;
        const float h = xr[ofx[0]] * cx[0] + xr[ofx[1]] * cx[1] + xr[ofx[2]] * cx[2] + xr[ofx[3]] * cx[3];
        acc += h * cy[i];
      }
      v = (acc - p.mean[c]) / p.std[c];
    }
  }
  if (p.out_f32) reinterpret_cast<float*>(p.out)[idx] = v;
  else reinterpret_cast<__bf16*>(p.out)[idx] = (__bf16)v;
}

constexpr int ENT = 128;     // threads of vit_embed_ln: 8 channels per thread and pass, at most 2 passes (C <= 2048)

struct VitK {
  const float* patches; int64_t ldp;
  const float* cls; const float* pos; const float* gamma; const float* beta;
  void* out; int64_t ldo;
  int T, C, out_f32;
  float eps;
};

__device__ __forceinline__ float block_sum_128(float v, float* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();                       // red is free (an earlier call's readers are past it)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1];
}

// One workgroup per token row (embed_ln_kernel's skeleton: two-pass statistics on values held in registers)
__global__ __launch_bounds__(ENT) void vit_embed_ln_kernel(const VitK p) {
  __shared__ float red[2];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int t = (int)(row % p.T);
  const int64_t b = row / p.T;
  const float* src = t == 0 ? p.cls : p.patches + (b * (p.T - 1) + (t - 1)) * p.ldp;
  const float* pr = p.pos + (int64_t)t * p.C;

  float v[2][8];
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int c = 8 * (tid + ENT * u);
    if (c < p.C) {
      const float4 t0 = *reinterpret_cast<const float4*>(src + c), t1 = *reinterpret_cast<const float4*>(src + c + 4);
      const float4 q0 = *reinterpret_cast<const float4*>(pr + c), q1 = *reinterpret_cast<const float4*>(pr + c + 4);
      v[u][0] = __fadd_rn(t0.x, q0.x); v[u][1] = __fadd_rn(t0.y, q0.y); v[u][2] = __fadd_rn(t0.z, q0.z); v[u][3] = __fadd_rn(t0.w, q0.w);
      v[u][4] = __fadd_rn(t1.x, q1.x); v[u][5] = __fadd_rn(t1.y, q1.y); v[u][6] = __fadd_rn(t1.z, q1.z); v[u][7] = __fadd_rn(t1.w, q1.w);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[u][e];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[u][e] = 0.f;
    }
  }
  const float mean = block_sum_128(s, red) / (float)p.C;
  float vs = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (8 * (tid + ENT * u) < p.C) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = v[u][e] - mean; vs += d * d; }
    }
  }
  const float rstd = 1.0f / sqrtf(block_sum_128(vs, red) / (float)p.C + p.eps);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int c = 8 * (tid + ENT * u);
    if (c >= p.C) continue;
    float y[8];
    const float4 g0 = *reinterpret_cast<const float4*>(p.gamma + c), g1 = *reinterpret_cast<const float4*>(p.gamma + c + 4);
    const float4 b0 = *reinterpret_cast<const float4*>(p.beta + c), b1 = *reinterpret_cast<const float4*>(p.beta + c + 4);
    const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = (v[u][e] - mean) * rstd * g[e] + bb[e];
    if (p.out_f32) {
      float4* dst = reinterpret_cast<float4*>(reinterpret_cast<float*>(p.out) + row * p.ldo + c);
      dst[0] = make_float4(y[0], y[1], y[2], y[3]);
      dst[1] = make_float4(y[4], y[5], y[6], y[7]);
    } else {
      *reinterpret_cast<uint4*>(reinterpret_cast<__bf16*>(p.out) + row * p.ldo + c) = pack_bf16x8(y);
    }
  }
}

struct L2K { const float* x; int64_t ldx; float* out; int64_t ldo; int n, D; };

// one wave per row: lane-strided float4 reads, butterfly sum (fixed order), division by the norm
__global__ __launch_bounds__(256) void l2_normalize_kernel(const L2K p) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.n) return;
  const float* x = p.x + (int64_t)row * p.ldx;
  float a = 0.f;
  for (int c = 4 * lane; c < p.D; c += 256) {
    const float4 t = *reinterpret_cast<const float4*>(x + c);
    a += t.x * t.x + t.y * t.y + t.z * t.z + t.w * t.w;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off);
  const float nrm = sqrtf(a);
  float* y = p.out + (int64_t)row * p.ldo;
  for (int c = 4 * lane; c < p.D; c += 256) {
    const float4 t = *reinterpret_cast<const float4*>(x + c);
    *reinterpret_cast<float4*>(y + c) = make_float4(t.x / nrm, t.y / nrm, t.z / nrm, t.w / nrm);
  }
}

}  // namespace

extern "C" int aptp_image_patches(const AptpImagePatchesParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->x && p->out, "image_patches: null pointer");
  APTP_CHECK(p->B > 0 && p->H > 0 && p->W > 0 && p->S > 0 && p->P > 0 && p->P <= 256 && p->S % p->P == 0 && p->S <= 16384 && p->H <= 16384 && p->W <= 16384,
             "image_patches: bad extents (S must be a positive multiple of P, sizes at most 16384)");
  const int K = 3 * p->P * p->P;
  APTP_CHECK(p->ldo == (int64_t)((K + 63) / 64) * 64, "image_patches: ldo (%lld) must be ceil(3 P^2 / 64) * 64 = %d", (long long)p->ldo, (K + 63) / 64 * 64);
  APTP_CHECK(p->resize || (p->nchw && p->H == p->S && p->W == p->S), "image_patches: resize = 0 takes [B, 3, S, S] pixel_values");
  for (int c = 0; c < 3; ++c) APTP_CHECK(!p->resize || p->std[c] > 0.f, "image_patches: std must be positive");
  APTP_CHECK(((uintptr_t)p->x % 4) == 0 && ((uintptr_t)p->out % 16) == 0, "image_patches: pointer alignment");
  const int G = p->S / p->P;
  const int64_t rows = (int64_t)p->B * G * G;
  APTP_CHECK(rows < (1ll << 31) && rows * p->ldo < (1ll << 39), "image_patches: output too large");
  PatchK k;
  k.x = p->x; k.out = p->out; k.ldo = p->ldo; k.total = rows * p->ldo;
  k.H = p->H; k.W = p->W; k.S = p->S; k.P = p->P; k.G = G; k.K = K; k.nchw = p->nchw ? 1 : 0; k.resize = p->resize ? 1 : 0;
  k.out_f32 = p->out_f32 ? 1 : 0;
  const int64_t HW = (int64_t)p->H * p->W;
  k.sb = 3 * HW;
  if (k.nchw) { k.sc = HW; k.sy = p->W; k.sx = 1; } else { k.sc = 1; k.sy = 3 * (int64_t)p->W; k.sx = 3; }
  k.scale_y = (float)p->H / (float)p->S; k.scale_x = (float)p->W / (float)p->S;
  for (int c = 0; c < 3; ++c) { k.mean[c] = p->mean[c]; k.std[c] = p->std[c]; }
  hipLaunchKernelGGL(image_patches_kernel, dim3((unsigned)((k.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}

extern "C" int aptp_vit_embed_ln(const AptpVitEmbedLnParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->patches && p->cls && p->pos && p->gamma && p->beta && p->out, "vit_embed_ln: null pointer");
  APTP_CHECK(p->B > 0 && p->T > 1 && p->C > 0 && p->C % 8 == 0 && p->C <= 16 * ENT,
             "vit_embed_ln: bad extents (T >= 2, C must be a multiple of 8, <= %d)", 16 * ENT);
  APTP_CHECK(p->ldp >= p->C && p->ldp % 4 == 0, "vit_embed_ln: ldp (%lld) must be >= C and a multiple of 4", (long long)p->ldp);
  APTP_CHECK(p->ldo >= p->C && p->ldo % 8 == 0, "vit_embed_ln: ldo (%lld) must be >= C and a multiple of 8", (long long)p->ldo);
  APTP_CHECK((int64_t)p->B * p->T < (1ll << 31), "vit_embed_ln: B * T too large");
  APTP_CHECK(p->eps > 0.f, "vit_embed_ln: eps must be positive");
  APTP_CHECK(((uintptr_t)p->patches % 16) == 0 && ((uintptr_t)p->cls % 16) == 0 && ((uintptr_t)p->pos % 16) == 0 &&
             ((uintptr_t)p->gamma % 16) == 0 && ((uintptr_t)p->beta % 16) == 0 && ((uintptr_t)p->out % 16) == 0, "vit_embed_ln: pointer alignment");
  VitK k;
  k.patches = p->patches; k.ldp = p->ldp; k.cls = p->cls; k.pos = p->pos; k.gamma = p->gamma; k.beta = p->beta;
  k.out = p->out; k.ldo = p->ldo; k.T = p->T; k.C = p->C; k.out_f32 = p->out_f32 ? 1 : 0; k.eps = p->eps;
  hipLaunchKernelGGL(vit_embed_ln_kernel, dim3((unsigned)(p->B * p->T)), dim3(ENT), 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}

extern "C" int aptp_l2_normalize(const AptpL2NormalizeParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->x && p->out, "l2_normalize: null pointer");
  APTP_CHECK(p->n > 0 && p->D > 0 && p->D % 4 == 0, "l2_normalize: bad extents (D must be a multiple of 4)");
  APTP_CHECK(p->ldx >= p->D && p->ldx % 4 == 0 && p->ldo >= p->D && p->ldo % 4 == 0, "l2_normalize: row strides must be >= D and multiples of 4");
  APTP_CHECK(((uintptr_t)p->x % 16) == 0 && ((uintptr_t)p->out % 16) == 0, "l2_normalize: pointer alignment");
  L2K k;
  k.x = p->x; k.ldx = p->ldx; k.out = p->out; k.ldo = p->ldo; k.n = p->n; k.D = p->D;
  hipLaunchKernelGGL(l2_normalize_kernel, dim3((unsigned)((p->n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
