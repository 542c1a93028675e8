// The learning-rate schedule on the device (the reference has none): the step counter, the factor s of the present step and
// the three networks' rates live in 32 device bytes, advanced by one launch at the top of the training step.  A captured graph bakes
// launch scalars in; the rates the Adam passes read (lgsch_clip_adam_*, loss_optim.hip) come from here, so a replayed step still walks
// warm-up and decay.  The definition is stated in include/littlegan_sched.h and restated on the host by config.lr_factor.
// Nothing here is on the critical path: one workgroup, one thread.
#include "lg_internal.h"
#include "../../include/littlegan_sched.h"

namespace {

#define LGSCH_PI 3.141592653589793

__global__ void sched_init_kernel(float* __restrict__ state, int k0) {
  if (threadIdx.x != 0) return;
  reinterpret_cast<f32x4*>(state)[0] = f32x4{__int_as_float(k0), 0.f, 0.f, 0.f};   // +0.f is the int32 0
  reinterpret_cast<f32x4*>(state)[1] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// fp64 throughout, then ONE conversion to fp32 and one fp32 multiply per network (-ffp-contract=off: no operation is fused)
__global__ void sched_step_kernel(float* __restrict__ state, int kind, int warmup, int decay_steps, float final_ratio, float lr_g,
                                  float lr_d, float lr_a) {
  if (threadIdx.x != 0) return;
  const int k = __float_as_int(state[0]);
  const double r = (double)final_ratio;
  const double up = k < warmup ? ((double)k + 1.0) / (double)warmup : 1.0;
  double d = 1.0;
  if (kind != LGSCH_KIND_CONSTANT) {
    const double t = k < warmup ? 0.0 : fmin(((double)k - (double)warmup) / (double)decay_steps, 1.0);
    d = kind == LGSCH_KIND_LINEAR ? 1.0 - (1.0 - r) * t : r + (1.0 - r) * 0.5 * (1.0 + cos(LGSCH_PI * t));
  }
  const float s = (float)(up * d);
  const int k1 = k < 0x7fffffff ? k + 1 : k;
  reinterpret_cast<f32x4*>(state)[0] = f32x4{__int_as_float(k1), s, lr_g * s, lr_d * s};
  reinterpret_cast<f32x4*>(state)[1] = f32x4{lr_a * s, 0.f, 0.f, 0.f};
}

bool rate_ok(float lr) { return lr > 0.f && lr <= 3.402823466e38f; }   // finite and positive; false for NaN

}  // namespace

extern "C" int lgsch_init(float* state, int k0, void* stream) {
  LG_CHECK_ARG(state, "lgsch_init: null pointer");
  LG_CHECK_ARG(((uintptr_t)state & 15) == 0, "lgsch_init: state must be 16-byte aligned");
  LG_CHECK_ARG(k0 >= 0, "lgsch_init: k0 %d below 0", k0);
  hipLaunchKernelGGL(sched_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, k0);
  LG_CHECK_LAUNCH("lgsch_init");
  lg_note_kernel("sched_init_kernel");
  return LG_OK;
}

extern "C" int lgsch_step(float* state, int kind, int warmup, int decay_steps, float final_ratio, float lr_g, float lr_d, float lr_a,
                          void* stream) {
  LG_CHECK_ARG(state, "lgsch_step: null pointer");
  LG_CHECK_ARG(((uintptr_t)state & 15) == 0, "lgsch_step: state must be 16-byte aligned");
  LG_CHECK_ARG(kind >= LGSCH_KIND_CONSTANT && kind <= LGSCH_KIND_COSINE, "lgsch_step: bad kind %d (0 constant, 1 linear, 2 cosine)", kind);
  LG_CHECK_ARG(warmup >= 0, "lgsch_step: warmup %d below 0", warmup);
  LG_CHECK_ARG(kind == LGSCH_KIND_CONSTANT || decay_steps >= 1, "lgsch_step: decay_steps %d below 1 for a decaying kind", decay_steps);
  LG_CHECK_ARG(final_ratio >= 0.f && final_ratio <= 1.f, "lgsch_step: final_ratio %g outside [0, 1]", (double)final_ratio);
  LG_CHECK_ARG(rate_ok(lr_g) && rate_ok(lr_d) && rate_ok(lr_a), "lgsch_step: every rate must be finite and > 0 (lr_g=%g lr_d=%g lr_a=%g)",
               (double)lr_g, (double)lr_d, (double)lr_a);
  hipLaunchKernelGGL(sched_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, kind, warmup, decay_steps, final_ratio, lr_g,
                     lr_d, lr_a);
  LG_CHECK_LAUNCH("lgsch_step");
  lg_note_kernel("sched_step_kernel");
  return LG_OK;
}
