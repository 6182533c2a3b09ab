// Everything a denoise step does after the U-Net call, in one launch:
//   aptp_guided_step   classifier-free guidance g = u + s (t - u), optionally rescaled to the text branch's per-sample standard
//                      deviation (Lin et al. 2023, section 3.4), then the DDIM, PNDM / PLMS or DPM-Solver++ (2M) update of
//                      pipeline.py's DDIMSchedulerLite.step_coef / PNDMSchedulerLite.step / DPMSolverMultistepSchedulerLite.step,
//                      statement for statement in fp32.  The per-step scheduler state is read from device memory, so one
//                      captured launch serves every step of a loop.
// Memory-bound and tiny: a flat grid of 16-byte accesses with a scalar tail, or -- with the rescale, which needs two standard
// deviations per sample first -- one workgroup per sample and fixed-order reductions (no floating-point atomics: bit-equal
// from run to run and from capture to replay).
#include "aptp_common.h"

// the torch statements round after every operation; keep the same roundings instead of contracting them into FMAs
#pragma clang fp contract(off)

namespace {

struct StepK {
  const void* noise; const float* sample; float* out;
  const float* coef; const int64_t* slot; const float* w; const float* flags;
  float* E; float* saved;      // (DPM-Solver++: saved is the previous data prediction)
  int64_t n, total;            // elements per sample, b * n
  int noise_f32, do_cfg, pndm, dpm, v_pred;
  float scale, phi;
};

// the scheduler's scalars of this step, formed per thread from the device tables exactly as the tensor expressions form them
struct StepCoef {
  float c0, c1, c2, c3;        // DDIM: sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), sqrt(1 - a_prev); PNDM: sqrt(a_t), sqrt(1 - a_t), sqrt(a_p / a_t), a_p - a_t
  float denom;                 // PNDM: a_t sqrt(1 - a_p) + sqrt(a_t (1 - a_t) a_p)
  float c4;                    // DPM-Solver++: c0 .. c4 = alpha_s, sigma_s, c_x, c_0, c_1 of the table row
  float w[5], f0, f1;
  int slot;
};

__device__ __forceinline__ StepCoef load_coef(const StepK& p) {
  StepCoef c;
  c.c4 = p.dpm ? p.coef[4] : 0.f;
  if (!p.pndm) {
    c.c0 = p.coef[0]; c.c1 = p.coef[1]; c.c2 = p.coef[2]; c.c3 = p.coef[3];
    c.denom = 1.f; c.f0 = c.f1 = 0.f; c.slot = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) c.w[k] = 0.f;
    return c;
  }
  const float a_t = p.coef[0], a_p = p.coef[1];
  c.c0 = sqrtf(a_t);
  c.c1 = sqrtf(1.f - a_t);
  c.c2 = sqrtf(a_p / a_t);
  c.c3 = a_p - a_t;
  c.denom = a_t * sqrtf(1.f - a_p) + sqrtf(a_t * (1.f - a_t) * a_p);
#pragma unroll
  for (int k = 0; k < 5; ++k) c.w[k] = p.w[k];
  c.f0 = p.flags[0]; c.f1 = p.flags[1];
  const int64_t s = p.slot[0];
  c.slot = s < 0 ? 0 : (s > 4 ? 4 : (int)s);             // whatever the table says, the write stays inside the ring
  return c;
}

__device__ __forceinline__ float load_noise(const StepK& p, int64_t i) {
  return p.noise_f32 ? reinterpret_cast<const float*>(p.noise)[i] : (float)reinterpret_cast<const __bf16*>(p.noise)[i];
}

__device__ __forceinline__ void load_noise4(const StepK& p, int64_t i, float* f) {
  if (p.noise_f32) {
    const float4 v = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p.noise) + i);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  } else {
    union { uint2 q; __bf16 h[4]; } u;
    u.q = *reinterpret_cast<const uint2*>(reinterpret_cast<const __bf16*>(p.noise) + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = (float)u.h[j];
  }
}

// guidance without the rescale
__device__ __forceinline__ float guide(const StepK& p, float u, float t) { return p.do_cfg ? u + p.scale * (t - u) : u; }

template <int V>
__device__ __forceinline__ void ld(const float* ptr, float* f) {
  if constexpr (V == 4) {
    const float4 v = *reinterpret_cast<const float4*>(ptr);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  } else {
    f[0] = ptr[0];
  }
}

template <int V>
__device__ __forceinline__ void st(float* ptr, const float* f) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(ptr) = make_float4(f[0], f[1], f[2], f[3]);
  else ptr[0] = f[0];
}

// the scheduler update of V consecutive elements whose guided model output is g; E and saved are updated in place
template <int V>
__device__ __forceinline__ void update(const StepK& p, const StepCoef& c, int64_t i, const float* g) {
  float x[V], o[V];
  ld<V>(p.sample + i, x);
  if (p.dpm) {
    float pv[V], x0[V];
    ld<V>(p.saved + i, pv);                                          // this lane's own elements, read before they are replaced
#pragma unroll
    for (int j = 0; j < V; ++j) {
      x0[j] = p.v_pred ? c.c0 * x[j] - c.c1 * g[j] : (x[j] - c.c1 * g[j]) / c.c0;
      o[j] = (c.c2 * x[j] + c.c3 * x0[j]) + c.c4 * pv[j];
    }
    st<V>(p.saved + i, x0);
  } else if (!p.pndm) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float x0, eps;
      if (p.v_pred) {
        x0 = c.c0 * x[j] - c.c1 * g[j];
        eps = c.c0 * g[j] + c.c1 * x[j];
      } else {
        eps = g[j];
        x0 = (x[j] - c.c1 * eps) / c.c0;
      }
      o[j] = c.c2 * x0 + c.c3 * eps;
    }
  } else {
    float sv[V], comb[V];
    ld<V>(p.saved + i, sv);
#pragma unroll
    for (int j = 0; j < V; ++j) comb[j] = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      float e[V];
      float* row = p.E + (int64_t)k * p.total + i;
      if (k == c.slot) {                                             // this call's output goes into the ring and into the sum
#pragma unroll
        for (int j = 0; j < V; ++j) e[j] = g[j];
        st<V>(row, g);
      } else {
        ld<V>(row, e);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) comb[j] = comb[j] + c.w[k] * e[j];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      sv[j] = sv[j] + c.f1 * (x[j] - sv[j]);                         // call 0 remembers the sample
      const float base = x[j] + c.f0 * (sv[j] - x[j]);               // call 1 restarts from it
      float cb = comb[j];
      if (p.v_pred) cb = c.c0 * cb + c.c1 * base;
      o[j] = c.c2 * base - c.c3 * cb / c.denom;
    }
    st<V>(p.saved + i, sv);
  }
  st<V>(p.out + i, o);
}

// flat grid over the b * n elements: nvec groups of four, then total - 4 nvec single elements
__global__ __launch_bounds__(256) void guided_step_flat_kernel(const StepK p, const int64_t nvec) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t ntail = p.total - 4 * nvec;
  if (tid >= nvec + ntail) return;
  const StepCoef c = load_coef(p);
  if (tid < nvec) {
    const int64_t i = 4 * tid;
    float u[4], t[4], g[4];
    load_noise4(p, i, u);
    if (p.do_cfg) load_noise4(p, p.total + i, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = guide(p, u[j], p.do_cfg ? t[j] : 0.f);
    update<4>(p, c, i, g);
  } else {
    const int64_t i = 4 * nvec + (tid - nvec);
    const float u = load_noise(p, i);
    const float g = guide(p, u, p.do_cfg ? load_noise(p, p.total + i) : 0.f);
    update<1>(p, c, i, &g);
  }
}

constexpr int RS_THREADS = 1024;
constexpr int RS_WAVES = RS_THREADS / APTP_WAVE;

// sum of (a, b) over the workgroup in a fixed order: lanes by xor-butterfly, then the waves one after another in LDS
__device__ __forceinline__ void block_sum2(double& a, double& b, double* lds) {
#pragma unroll
  for (int off = APTP_WAVE / 2; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, APTP_WAVE);
    b += __shfl_xor(b, off, APTP_WAVE);
  }
  const int wave = threadIdx.x / APTP_WAVE, lane = threadIdx.x % APTP_WAVE;
  __syncthreads();                                        // (the previous call's readers are done with lds)
  if (lane == 0) { lds[2 * wave] = a; lds[2 * wave + 1] = b; }
  __syncthreads();
  a = 0.0; b = 0.0;
#pragma unroll
  for (int wv = 0; wv < RS_WAVES; ++wv) { a += lds[2 * wv]; b += lds[2 * wv + 1]; }
}

// guidance with the rescale: one workgroup per sample.  Pass 1 the means of the text branch and of g, pass 2 their squared
// deviations (two passes: no cancellation whatever the mean), pass 3 the update.  The row is read three times, out of L2.
template <int V>
__global__ __launch_bounds__(RS_THREADS) void guided_step_rescale_kernel(const StepK p) {
  __shared__ double lds[2 * RS_WAVES];
  const int64_t row = (int64_t)blockIdx.x * p.n;
  const int64_t nv = p.n / V;                             // (V == 4 only when it divides n)
  double st = 0.0, sg = 0.0;
  for (int64_t j = threadIdx.x; j < nv; j += RS_THREADS) {
    float u[V], t[V];
    if constexpr (V == 4) { load_noise4(p, row + 4 * j, u); load_noise4(p, p.total + row + 4 * j, t); }
    else { u[0] = load_noise(p, row + j); t[0] = load_noise(p, p.total + row + j); }
#pragma unroll
    for (int e = 0; e < V; ++e) { st += (double)t[e]; sg += (double)guide(p, u[e], t[e]); }
  }
  block_sum2(st, sg, lds);
  const double mt = st / (double)p.n, mg = sg / (double)p.n;
  double qt = 0.0, qg = 0.0;
  for (int64_t j = threadIdx.x; j < nv; j += RS_THREADS) {
    float u[V], t[V];
    if constexpr (V == 4) { load_noise4(p, row + 4 * j, u); load_noise4(p, p.total + row + 4 * j, t); }
    else { u[0] = load_noise(p, row + j); t[0] = load_noise(p, p.total + row + j); }
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const double dt = (double)t[e] - mt, dg = (double)guide(p, u[e], t[e]) - mg;
      qt += dt * dt; qg += dg * dg;
    }
  }
  block_sum2(qt, qg, lds);
  // unbiased, as torch's .std; the ratio is applied in fp32 like the tensor expression
  const float std_t = (float)sqrt(qt / (double)(p.n - 1)), std_g = (float)sqrt(qg / (double)(p.n - 1));
  const float ratio = std_t / std_g;
  const StepCoef c = load_coef(p);
  for (int64_t j = threadIdx.x; j < nv; j += RS_THREADS) {
    float u[V], t[V], g[V];
    if constexpr (V == 4) { load_noise4(p, row + 4 * j, u); load_noise4(p, p.total + row + 4 * j, t); }
    else { u[0] = load_noise(p, row + j); t[0] = load_noise(p, p.total + row + j); }
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float g0 = guide(p, u[e], t[e]);
      g[e] = p.phi * (g0 * ratio) + (1.f - p.phi) * g0;
    }
    update<V>(p, c, row + (int64_t)V * j, g);
  }
}

}  // namespace

extern "C" int aptp_guided_step(const AptpGuidedStepParams* p, aptp_stream_t stream) {
  APTP_CHECK(p, "guided_step: null pointer");
  APTP_CHECK(p->scheduler != APTP_STEP_DPMPP || (p->coef && p->saved && ((uintptr_t)p->coef % 4) == 0 && ((uintptr_t)p->saved % 4) == 0),
             "guided_step: DPM-Solver needs coef (5 floats) and prev (passed as saved), both 4-byte aligned");
  APTP_CHECK(p->noise && p->sample && p->out && p->coef, "guided_step: null pointer");
  APTP_CHECK(p->noise_dtype == APTP_STEP_NOISE_BF16 || p->noise_dtype == APTP_STEP_NOISE_F32,
             "guided_step: noise_dtype %d is neither bf16 (%d) nor fp32 (%d)", p->noise_dtype, APTP_STEP_NOISE_BF16, APTP_STEP_NOISE_F32);
  APTP_CHECK(p->scheduler == APTP_STEP_DDIM || p->scheduler == APTP_STEP_PNDM || p->scheduler == APTP_STEP_DPMPP,
             "guided_step: unknown scheduler %d", p->scheduler);
  APTP_CHECK(p->prediction == APTP_STEP_EPSILON || p->prediction == APTP_STEP_V_PREDICTION, "guided_step: unknown prediction type %d",
             p->prediction);
  APTP_CHECK(p->do_cfg == 0 || p->do_cfg == 1, "guided_step: do_cfg is %d (0 or 1)", p->do_cfg);
  APTP_CHECK(p->b >= 1 && p->n >= 1 && p->b <= 65535 && p->n <= (1ll << 40) / p->b, "guided_step: bad extents b = %d, n = %lld", p->b,
             (long long)p->n);
  APTP_CHECK(p->noise_rows == (p->do_cfg ? 2 * p->b : p->b), "guided_step: noise has %d rows, expected %d (b = %d, do_cfg = %d)",
             p->noise_rows, p->do_cfg ? 2 * p->b : p->b, p->b, p->do_cfg);
  APTP_CHECK(p->guidance_rescale >= 0.f && p->guidance_rescale <= 1.f, "guided_step: guidance_rescale %g outside [0, 1]",
             (double)p->guidance_rescale);
  const bool rescale = p->guidance_rescale > 0.f;
  APTP_CHECK(!rescale || p->do_cfg, "guided_step: guidance_rescale needs classifier-free guidance (do_cfg)");
  APTP_CHECK(!rescale || p->n >= 2, "guided_step: guidance_rescale needs n >= 2 for an unbiased standard deviation, got %lld",
             (long long)p->n);
  const bool f32 = p->noise_dtype == APTP_STEP_NOISE_F32, pndm = p->scheduler == APTP_STEP_PNDM, dpm = p->scheduler == APTP_STEP_DPMPP;
  APTP_CHECK(((uintptr_t)p->noise % (f32 ? 4 : 2)) == 0 && ((uintptr_t)p->sample % 4) == 0 && ((uintptr_t)p->out % 4) == 0 &&
             ((uintptr_t)p->coef % 4) == 0, "guided_step: pointer alignment");
  if (pndm) {
    APTP_CHECK(p->slot && p->w && p->flags && p->E && p->saved, "guided_step: PNDM needs slot, w, flags, E and saved");
    APTP_CHECK(((uintptr_t)p->slot % 8) == 0 && ((uintptr_t)p->w % 4) == 0 && ((uintptr_t)p->flags % 4) == 0 &&
               ((uintptr_t)p->E % 4) == 0 && ((uintptr_t)p->saved % 4) == 0, "guided_step: pointer alignment (PNDM state)");
  }
  StepK k;
  k.noise = p->noise; k.sample = p->sample; k.out = p->out;
  k.coef = p->coef; k.slot = p->slot; k.w = p->w; k.flags = p->flags; k.E = p->E; k.saved = p->saved;
  k.n = p->n; k.total = (int64_t)p->b * p->n;
  k.noise_f32 = f32; k.do_cfg = p->do_cfg; k.pndm = pndm; k.dpm = dpm; k.v_pred = p->prediction == APTP_STEP_V_PREDICTION;
  k.scale = p->guidance_scale; k.phi = p->guidance_rescale;
  // groups of four need every base the kernel forms to be aligned: 16 bytes for fp32, 8 for four bf16
  const int64_t unit = rescale ? p->n : k.total;          // rows start at multiples of this many elements
  const uintptr_t nalign = f32 ? 16 : 8;
  bool aligned = ((uintptr_t)p->noise % nalign) == 0 && ((uintptr_t)p->sample % 16) == 0 && ((uintptr_t)p->out % 16) == 0;
  if (p->do_cfg) aligned = aligned && k.total % 4 == 0;   // the text half starts b * n elements in
  if (pndm) aligned = aligned && ((uintptr_t)p->E % 16) == 0 && ((uintptr_t)p->saved % 16) == 0 && k.total % 4 == 0;
  if (dpm) aligned = aligned && ((uintptr_t)p->saved % 16) == 0;   // prev is indexed like sample
  if (rescale) aligned = aligned && unit % 4 == 0;
  if (rescale) {
    if (aligned)
      hipLaunchKernelGGL(guided_step_rescale_kernel<4>, dim3((unsigned)p->b), dim3(RS_THREADS), 0, (hipStream_t)stream, k);
    else
      hipLaunchKernelGGL(guided_step_rescale_kernel<1>, dim3((unsigned)p->b), dim3(RS_THREADS), 0, (hipStream_t)stream, k);
  } else {
    const int64_t nvec = aligned ? k.total / 4 : 0;
    const int64_t threads = nvec + (k.total - 4 * nvec);
    const int64_t blocks = (threads + 255) / 256;
    APTP_CHECK(blocks < (1ll << 31), "guided_step: too many elements");
    hipLaunchKernelGGL(guided_step_flat_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, k, nvec);
  }
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
