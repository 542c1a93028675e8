// Adaptive augmentation probability on top of diff_augment (ADA; Karras et al. 2020, "Training GANs with limited data"; the
// reference has none).  Two parts, both on the device so that a captured step replays with the present p and the host never waits:
//   the gate        each named component of each row's record (diffaug_draw.h) is applied with probability p = state[0]: three independent
//                   Bernoulli(p) per row from a third Philox block of the row — the counter of its first block with the third counter word 1,
//                   which no record block has — compared as 24-bit integers with t = (unsigned)(p 2^24).  A gate that is off clears the
//                   component's policy bit, so "off" is the identity values lg_diffaug_draw writes for a component that is not named, and the
//                   passes T / T^T (diffaug.hip) know nothing of it: the identity record goes through them bit for bit.
//   the controller  state = {fp32 p, int32 sum of signs, int32 rows, int32 steps}.  Every step adds sign(real_pr - 0.5) over the B real rows
//                   of D's output (an integer sum: order-free); every `interval` steps p moves by rows * per_row towards making
//                   r = sum / rows meet the target, clamped to [0, 1], and the counters restart.
// Nothing here is on the critical path: one thread per row, one workgroup, one thread.
#include "lg_internal.h"
#include "../../include/littlegan_hip_ext.h"
#include "diffaug_draw.h"

namespace {

// params[i] = the record of row r0 + i of call slot `call` under the policy its own gates leave: bit j of `on` is w_j < t
__global__ __launch_bounds__(256) void diffaug_draw_gated_kernel(const unsigned long long* __restrict__ key, int call, int r0, int rows, int S,
                                                                 int policy, const float* __restrict__ state, float* __restrict__ params) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  const unsigned long long seed = key[0], ctr = diffaug_row_ctr(key[1], call, r0 + i);
  const u4 G = philox4x32_10(u4{(unsigned)ctr, (unsigned)(ctr >> 32), 1u, 0u}, (unsigned)seed, (unsigned)(seed >> 32));
  // exact: p is fp32 in [0, 1]; p = 1 gives 2^24, above every 24-bit word.  The clamp changes no p of that range and keeps the conversion
  // defined whatever the 4 bytes hold (fmaxf(NaN, 0) = 0): init, adjust and the checkpoint loader never write anything else
  const unsigned t = (unsigned)(fminf(fmaxf(state[0], 0.f), 1.f) * 16777216.0f);
  const int on = ((G.x >> 8) < t ? 1 : 0) | ((G.y >> 8) < t ? 2 : 0) | ((G.z >> 8) < t ? 4 : 0);
  f32x4 p0, p1;
  diffaug_record(seed, ctr, S, policy & on, p0, p1);
  reinterpret_cast<f32x4*>(params)[2 * i] = p0;
  reinterpret_cast<f32x4*>(params)[2 * i + 1] = p1;
}

__global__ void ada_init_kernel(float* __restrict__ state, float p0) {
  if (threadIdx.x == 0) *reinterpret_cast<f32x4*>(state) = f32x4{p0, 0.f, 0.f, 0.f};   // +0.f is the int32 0 of words 1..3
}

// One workgroup: thread t adds the signs of rows t, t + 256, ...; the 256 integer sums merge through the waves and 4 LDS words.
__global__ __launch_bounds__(256) void ada_accumulate_kernel(float* __restrict__ state, const float* __restrict__ heads, int ld, int B) {
  __shared__ int sred[4];
  int s = 0;
  for (int i = (int)threadIdx.x; i < B; i += 256) {
    const float v = heads[(long long)i * ld];
    s += (int)(v > 0.5f) - (int)(v < 0.5f);   // NaN: both comparisons false
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int* w = reinterpret_cast<int*>(state);
    w[1] += (sred[0] + sred[1]) + (sred[2] + sred[3]);
    w[2] += B;
    w[3] += 1;
  }
}

__global__ void ada_adjust_kernel(float* __restrict__ state, int interval, float target, float per_row) {
  if (threadIdx.x != 0) return;
  const f32x4 st = *reinterpret_cast<const f32x4*>(state);
  const int sum = __float_as_int(st[1]), rows = __float_as_int(st[2]), steps = __float_as_int(st[3]);
  if (steps < interval) return;
  const float r = (float)sum / (float)rows;
  const int dir = r > target ? 1 : r < target ? -1 : 0;
  const float p = fminf(fmaxf(st[0] + (float)dir * ((float)rows * per_row), 0.f), 1.f);
  *reinterpret_cast<f32x4*>(state) = f32x4{p, 0.f, 0.f, 0.f};
}

}  // namespace

extern "C" int lgx_diffaug_draw_gated(const long long* key, int call, int r0, int rows, int S, int policy_bits, const float* state,
                                      float* params, void* stream) {
  LG_CHECK_ARG(key && state && params, "lgx_diffaug_draw_gated: null pointer");
  LG_CHECK_ARG(((uintptr_t)key & 7) == 0 && (((uintptr_t)state | (uintptr_t)params) & 15) == 0,
               "lgx_diffaug_draw_gated: key must be 8-byte, state and params 16-byte aligned");
  LG_CHECK_ARG(call >= 0 && call <= 3, "lgx_diffaug_draw_gated: call slot %d outside 0..3", call);
  LG_CHECK_ARG(rows > 0 && r0 >= 0 && (long long)r0 + rows <= (1LL << 24), "lgx_diffaug_draw_gated: rows %d .. %d + %d outside a call slot's 2^24",
               r0, r0, rows);
  LG_CHECK_ARG(S >= 8 && S % 8 == 0 && S <= 1024, "lgx_diffaug_draw_gated: image side %d must be a multiple of 8, at least 8", S);
  LG_CHECK_ARG(policy_bits >= 0 && policy_bits <= 7, "lgx_diffaug_draw_gated: policy bits %d outside 0..7 (1 color, 2 translation, 4 cutout)",
               policy_bits);
  hipLaunchKernelGGL(diffaug_draw_gated_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long*>(key), call, r0, rows, S, policy_bits, state, params);
  LG_CHECK_LAUNCH("lgx_diffaug_draw_gated");
  return LG_OK;
}

extern "C" int lgx_ada_init(float* state, float p0, void* stream) {
  LG_CHECK_ARG(state, "lgx_ada_init: null pointer");
  LG_CHECK_ARG(((uintptr_t)state & 15) == 0, "lgx_ada_init: state must be 16-byte aligned");
  LG_CHECK_ARG(p0 >= 0.f && p0 <= 1.f, "lgx_ada_init: p0 %g outside [0, 1]", (double)p0);
  hipLaunchKernelGGL(ada_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, p0);
  LG_CHECK_LAUNCH("lgx_ada_init");
  return LG_OK;
}

extern "C" int lgx_ada_accumulate(float* state, const float* heads, int ld, int B, void* stream) {
  LG_CHECK_ARG(state && heads, "lgx_ada_accumulate: null pointer");
  LG_CHECK_ARG(((uintptr_t)state & 15) == 0 && ((uintptr_t)heads & 3) == 0,
               "lgx_ada_accumulate: state must be 16-byte, heads 4-byte aligned");
  LG_CHECK_ARG(ld >= 1, "lgx_ada_accumulate: leading dimension %d below 1", ld);
  LG_CHECK_ARG(B >= 1 && B <= (1 << 20), "lgx_ada_accumulate: bad row count %d", B);
  hipLaunchKernelGGL(ada_accumulate_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, state, heads, ld, B);
  LG_CHECK_LAUNCH("lgx_ada_accumulate");
  return LG_OK;
}

extern "C" int lgx_ada_adjust(float* state, int interval, float target, float per_row, void* stream) {
  LG_CHECK_ARG(state, "lgx_ada_adjust: null pointer");
  LG_CHECK_ARG(((uintptr_t)state & 15) == 0, "lgx_ada_adjust: state must be 16-byte aligned");
  LG_CHECK_ARG(interval >= 1, "lgx_ada_adjust: interval %d below 1", interval);
  LG_CHECK_ARG(target > 0.f && target < 1.f, "lgx_ada_adjust: target %g outside (0, 1)", (double)target);
  LG_CHECK_ARG(per_row > 0.f && per_row <= 3.402823466e38f, "lgx_ada_adjust: per_row %g must be positive and finite", (double)per_row);
  hipLaunchKernelGGL(ada_adjust_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, interval, target, per_row);
  LG_CHECK_LAUNCH("lgx_ada_adjust");
  return LG_OK;
}
