// The learning-rate curves of the recipes' `lr_scheduler` (transformers.optimization.get_scheduler; diffusers' optimization.py has
// the same expressions) as a function of the count of APPLIED optimizer steps (csrc/lr_schedule.hip).  The step that
// follows k applied ones runs at lr * m(k): the first at m(0), and a skipped step does not advance k -- the convention of
// packed_pass.h's warmup_lr.  W = num_warmup_steps, T = num_training_steps, both in optimizer steps.
//   every kind but constant, k < W:  m = k / max(1, W)
//   constant                         m = 1
//   constant_with_warmup             m = 1                                                            (k >= W)
//   linear                           m = max(0, (T - k) / max(1, T - W))
//   cosine                           m = max(0, 0.5 (1 + cos(pi num_cycles 2 prog))),  prog = (k - W) / max(1, T - W);  rises again past T
//   cosine_with_restarts             m = 0 for prog >= 1, else max(0, 0.5 (1 + cos(pi ((num_cycles prog) mod 1))))
//   polynomial                       m = lr_end / lr_init for k > T, else ((lr_init - lr_end) (1 - (k - W) / (T - W))^power + lr_end) / lr_init
// m is evaluated in fp64, operation by operation as the library's Python does; the stored rate is (float)((double)lr * m), with two
// exceptions that exist so that switching between this path and the older ones changes no bit: constant stores lr itself and
// constant_with_warmup stores warmup_lr's own fp32 expression lr * fminf(1, k / W).
// Plain C++ for the device and the host, as train_noise.h is: the kernel calls nothing else for arithmetic.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define APTP_LRS_HD __host__ __device__ inline
#else
#define APTP_LRS_HD inline
#endif

// every product and sum below is rounded on its own
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define APTP_LRS_CONSTANT 0
#define APTP_LRS_CONSTANT_WITH_WARMUP 1
#define APTP_LRS_LINEAR 2
#define APTP_LRS_COSINE 3
#define APTP_LRS_COSINE_WITH_RESTARTS 4
#define APTP_LRS_POLYNOMIAL 5
#define APTP_LRS_KINDS 6
#define APTP_LRS_MAX_RATES 16
#define APTP_LRS_MAX_STEPS (1 << 24)   // k is an fp32 count: every integer below 2^24 is exact

// the host values of a schedule
struct AptpLrsCurve {
  int kind;
  double W, T;                         // integers
  double num_cycles, power, lr_end, lr_init;
};

// 0 when the curve is well formed, else a message (what aptp_lr_schedule refuses, and packed_train.LrSchedule with it)
inline const char* aptp_lrs_invalid(const AptpLrsCurve& c) {
  if (c.kind < 0 || c.kind >= APTP_LRS_KINDS) return "unknown kind";
  if (!(c.W >= 0.0) || !(c.T >= 0.0)) return "negative steps";
  if (!(c.W < (double)APTP_LRS_MAX_STEPS) || !(c.T < (double)APTP_LRS_MAX_STEPS)) return "steps must stay below 2^24";
  if (c.kind >= APTP_LRS_LINEAR && c.T < c.W) return "training_steps < warmup_steps";
  if ((c.kind == APTP_LRS_COSINE || c.kind == APTP_LRS_COSINE_WITH_RESTARTS) && !(c.num_cycles > 0.0)) return "num_cycles must be > 0";
  if (c.kind == APTP_LRS_POLYNOMIAL) {
    if (!(c.power > 0.0)) return "power must be > 0";
    if (!(c.lr_init > c.lr_end)) return "lr_init must be > lr_end";
    if (!(c.T > c.W)) return "polynomial needs training_steps > warmup_steps (the library divides by their difference)";
  }
  return 0;
}

APTP_LRS_HD double aptp_lrs_max(double a, double b) { return b > a ? b : a; }        // Python's max(a, b): a unless b is larger

// m(k) in fp64
APTP_LRS_HD double aptp_lrs_multiplier(const AptpLrsCurve& c, double k) {
  const double pi = 3.141592653589793;
  if (c.kind == APTP_LRS_CONSTANT) return 1.0;
  if (k < c.W) return k / aptp_lrs_max(1.0, c.W);
  if (c.kind == APTP_LRS_CONSTANT_WITH_WARMUP) return 1.0;
  if (c.kind == APTP_LRS_LINEAR) return aptp_lrs_max(0.0, (c.T - k) / aptp_lrs_max(1.0, c.T - c.W));
  if (c.kind == APTP_LRS_POLYNOMIAL) {
    if (k > c.T) return c.lr_end / c.lr_init;
    const double pct = 1.0 - (k - c.W) / (c.T - c.W);
    return ((c.lr_init - c.lr_end) * pow(pct, c.power) + c.lr_end) / c.lr_init;
  }
  const double prog = (k - c.W) / aptp_lrs_max(1.0, c.T - c.W);
  if (c.kind == APTP_LRS_COSINE) return aptp_lrs_max(0.0, 0.5 * (1.0 + cos(pi * c.num_cycles * 2.0 * prog)));
  if (prog >= 1.0) return 0.0;
  return aptp_lrs_max(0.0, 0.5 * (1.0 + cos(pi * fmod(c.num_cycles * prog, 1.0))));
}

// the fp32 rate stored for base rate lr after k applied steps (k as the fp32 count holds it)
APTP_LRS_HD float aptp_lrs_rate(const AptpLrsCurve& c, float lr, float k) {
  if (c.kind == APTP_LRS_CONSTANT) return lr;
  if (c.kind == APTP_LRS_CONSTANT_WITH_WARMUP) {       // packed_pass::warmup_lr, the same fp32 expression
    const float W = (float)c.W;
    return W > 0.0f ? lr * fminf(1.0f, k / W) : lr;
  }
  return (float)((double)lr * aptp_lrs_multiplier(c, (double)k));
}
