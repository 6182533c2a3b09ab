// The rate of the next optimizer step, computed on the device from the count of applied steps: one launch of one
// small block per optimizer step, in front of the AdamW launches that read what it stores -- aptp_adamw_many_lr and
// aptp_adamw8_many_lr through their lr_dev, aptp_group_adamw through the lr column of its groups_dev (out_stride = 3).  The count
// lives in device memory and advances under the device-side gate, so the host cannot know it without a wait per step, and the
// router's optimizer step sits inside a captured graph: the curve has to be evaluated here.  The formulas are lr_schedule.h's.
#include "aptp_common.h"
#include "lr_schedule.h"

static_assert(APTP_LR_CONSTANT == APTP_LRS_CONSTANT && APTP_LR_CONSTANT_WITH_WARMUP == APTP_LRS_CONSTANT_WITH_WARMUP &&
              APTP_LR_LINEAR == APTP_LRS_LINEAR && APTP_LR_COSINE == APTP_LRS_COSINE &&
              APTP_LR_COSINE_WITH_RESTARTS == APTP_LRS_COSINE_WITH_RESTARTS && APTP_LR_POLYNOMIAL == APTP_LRS_POLYNOMIAL,
              "lr_schedule.h numbers the kinds as the public header does");

namespace {

struct LrsK {
  AptpLrsCurve c;
  const float* count; const float* base; float* out; float* mult;
  int n, stride;
};

__global__ __launch_bounds__(APTP_WAVE) void lr_schedule_kernel(const LrsK k) {
  const int i = threadIdx.x;
  const float applied = k.count[0];             // uniform: one scalar load
  if (i < k.n) k.out[(int64_t)i * k.stride] = aptp_lrs_rate(k.c, k.base[i], applied);
  if (i == 0 && k.mult) k.mult[0] = (float)aptp_lrs_multiplier(k.c, (double)applied);
}

}  // namespace

extern "C" int aptp_lr_schedule(const AptpLrScheduleParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->count_dev && p->base_dev && p->out_dev, "lr_schedule: null pointer");
  APTP_CHECK((((uintptr_t)p->count_dev | (uintptr_t)p->base_dev | (uintptr_t)p->out_dev | (uintptr_t)p->mult_dev) & 3) == 0,
             "lr_schedule: misaligned pointer");
  APTP_CHECK(p->n >= 1 && p->n <= APTP_LRS_MAX_RATES, "lr_schedule: n = %d outside 1..%d", (int)p->n, APTP_LRS_MAX_RATES);
  APTP_CHECK(p->out_stride >= 1, "lr_schedule: out_stride must be >= 1");
  const AptpLrsCurve c{(int)p->kind, (double)p->warmup_steps, (double)p->training_steps, p->num_cycles, p->power, p->lr_end, p->lr_init};
  const char* why = aptp_lrs_invalid(c);
  APTP_CHECK(!why, "lr_schedule: %s", why);
  const LrsK k{c, p->count_dev, p->base_dev, p->out_dev, p->mult_dev, (int)p->n, (int)p->out_stride};
  hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(APTP_WAVE), 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
