// Global-norm gradient clipping and the non-finite step guard (the reference has neither): one fp64 sum of squares over
// the gradient range a network trains this step, finished into a 32-byte record on the device that the Adam pass of that network reads
// (lgg_clip_adam_*, loss_optim.hip).  A captured graph bakes launch scalars in; the scale, the skip flag and the counters come from the
// record, so a replayed step clips by the norm of ITS gradient.  The definition, the order of the additions and the record are stated in
// include/littlegan_guard.h and restated on the host by config.grad_guard_restate.
#include "lg_internal.h"

namespace {

constexpr int GG_THREADS = 256;
constexpr int GG_GROUPS = GG_CHUNK / 4 / GG_THREADS;   // 4-element groups per thread and chunk: 16

// VEC: g is 16-byte aligned and a whole group is one 16-byte load; else four scalar loads of the same elements.  A group that crosses
// n is read element by element either way.  Nothing at or beyond g[n] is read.
template <bool VEC>
__global__ __launch_bounds__(GG_THREADS) void gg_sumsq_partial_kernel(const float* __restrict__ g, long long n, long long nchunks,
                                                                      double* __restrict__ partial) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (long long ck = blockIdx.x; ck < nchunks; ck += gridDim.x) {
    const long long base = ck * GG_CHUNK + 4ll * threadIdx.x;
#pragma unroll
    for (int k = 0; k < GG_GROUPS; ++k) {
      const long long i = base + 4ll * GG_THREADS * k;
      if (i + 3 < n) {
        f32x4 x;
        if (VEC) {
          x = *reinterpret_cast<const f32x4*>(g + i);
        } else {
          x = f32x4{g[i], g[i + 1], g[i + 2], g[i + 3]};
        }
        a0 += (double)x[0] * (double)x[0];
        a1 += (double)x[1] * (double)x[1];
        a2 += (double)x[2] * (double)x[2];
        a3 += (double)x[3] * (double)x[3];
      } else {
        if (i < n) a0 += (double)g[i] * (double)g[i];
        if (i + 1 < n) a1 += (double)g[i + 1] * (double)g[i + 1];
        if (i + 2 < n) a2 += (double)g[i + 2] * (double)g[i + 2];
      }
    }
  }
  __shared__ double sred[16];
  double red[1] = {(a0 + a1) + (a2 + a3)};
  lg_block_sum_d<1>(red, sred);   // xor butterflies inside a wave, the four waves in wave order: a fixed order
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ void gg_init_kernel(float* __restrict__ rec, int skipped0, int nonfinite0) {
  if (threadIdx.x != 0) return;
  reinterpret_cast<f32x4*>(rec)[0] = f32x4{0.f, 0.f, 0.f, __int_as_float(skipped0)};   // +0.f is the int32 0
  reinterpret_cast<f32x4*>(rec)[1] = f32x4{__int_as_float(nonfinite0), 0.f, 0.f, 0.f};
}

// The P partials go through LDS so that the one adding thread waits for no global load inside its chain of additions.
__global__ __launch_bounds__(GG_THREADS) void gg_finalise_kernel(const double* __restrict__ partial, int P, float* __restrict__ rec,
                                                                 float gscale, float clip_norm, int skip) {
  __shared__ double sp[GG_MAX_PARTIALS];
  for (int i = threadIdx.x; i < P; i += GG_THREADS) sp[i] = partial[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double S = 0.0;
  for (int i = 0; i < P; ++i) S += sp[i];
  const bool bad = !(fabs(S) <= 1.7976931348623157e308);   // NaN or +-Inf
  const float N = (float)(sqrt(S) * (double)gscale);
  float c = 1.f;
  if (clip_norm != 0.f && !bad) {
    const float q = clip_norm / (N + 1e-6f);
    c = q < 1.f ? q : 1.f;
  }
  const float eff = gscale * c;
  const int skip_now = (bad && skip) ? 1 : 0;
  int skipped = __float_as_int(rec[3]), nonfinite = __float_as_int(rec[4]);
  if (skip_now && skipped < 0x7fffffff) skipped += 1;
  if (bad && nonfinite < 0x7fffffff) nonfinite += 1;
  reinterpret_cast<f32x4*>(rec)[0] = f32x4{N, eff, __int_as_float(skip_now), __int_as_float(skipped)};
  reinterpret_cast<f32x4*>(rec)[1] = f32x4{__int_as_float(nonfinite), c, 0.f, 0.f};
}

long long chunks_of(long long n) { return (n + GG_CHUNK - 1) / GG_CHUNK; }

}  // namespace

extern "C" int lgg_partials_count(long long n) {
  if (n < 1) return 0;
  const long long ck = chunks_of(n);
  return ck < GG_MAX_PARTIALS ? (int)ck : GG_MAX_PARTIALS;
}

extern "C" size_t lgg_workspace_bytes(long long n) { return (size_t)lgg_partials_count(n) * sizeof(double); }

extern "C" int lgg_init(void* rec, int skipped0, int nonfinite0, void* stream) {
  LG_CHECK_ARG(rec, "lgg_init: null pointer");
  LG_CHECK_ARG(((uintptr_t)rec & 15) == 0, "lgg_init: rec must be 16-byte aligned");
  LG_CHECK_ARG(skipped0 >= 0 && nonfinite0 >= 0, "lgg_init: counter below 0 (skipped0=%d nonfinite0=%d)", skipped0, nonfinite0);
  hipLaunchKernelGGL(gg_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (float*)rec, skipped0, nonfinite0);
  LG_CHECK_LAUNCH("lgg_init");
  lg_note_kernel("gg_init_kernel");
  return LG_OK;
}

extern "C" int lgg_sumsq_partial(const float* g, long long n, void* partial, size_t partial_bytes, void* stream) {
  LG_CHECK_ARG(g && partial, "lgg_sumsq_partial: null pointer");
  LG_CHECK_ARG(n >= 1, "lgg_sumsq_partial: n=%lld below 1", n);
  LG_CHECK_ARG(((uintptr_t)g & 3) == 0 && ((uintptr_t)partial & 7) == 0,
               "lgg_sumsq_partial: g must be 4-byte, partial 8-byte aligned");
  LG_CHECK_ARG(partial_bytes >= lgg_workspace_bytes(n), "lgg_sumsq_partial: partial_bytes=%zu below lgg_workspace_bytes(%lld)=%zu",
               partial_bytes, n, lgg_workspace_bytes(n));
  const int P = lgg_partials_count(n);
  const bool vec = ((uintptr_t)g & 15) == 0;
  if (vec) {
    hipLaunchKernelGGL(gg_sumsq_partial_kernel<true>, dim3(P), dim3(GG_THREADS), 0, (hipStream_t)stream, g, n, chunks_of(n),
                       (double*)partial);
  } else {
    hipLaunchKernelGGL(gg_sumsq_partial_kernel<false>, dim3(P), dim3(GG_THREADS), 0, (hipStream_t)stream, g, n, chunks_of(n),
                       (double*)partial);
  }
  LG_CHECK_LAUNCH("lgg_sumsq_partial");
  lg_note_kernel(vec ? "gg_sumsq_partial_kernel<vec>" : "gg_sumsq_partial_kernel<scalar>");
  return LG_OK;
}

extern "C" int lgg_finalise(const void* partial, long long n, void* rec, float gscale, float clip_norm, int skip, void* stream) {
  LG_CHECK_ARG(partial && rec, "lgg_finalise: null pointer");
  LG_CHECK_ARG(n >= 1, "lgg_finalise: n=%lld below 1", n);
  LG_CHECK_ARG(((uintptr_t)partial & 7) == 0 && ((uintptr_t)rec & 15) == 0, "lgg_finalise: partial must be 8-byte, rec 16-byte aligned");
  LG_CHECK_ARG(gscale > 0.f && gscale <= 3.402823466e38f, "lgg_finalise: gscale=%g must be finite and > 0", (double)gscale);
  LG_CHECK_ARG(clip_norm >= 0.f && clip_norm <= 3.402823466e38f, "lgg_finalise: clip_norm=%g must be finite and >= 0 (0 = off)",
               (double)clip_norm);
  LG_CHECK_ARG(skip == 0 || skip == 1, "lgg_finalise: skip=%d must be 0 or 1", skip);
  hipLaunchKernelGGL(gg_finalise_kernel, dim3(1), dim3(GG_THREADS), 0, (hipStream_t)stream, (const double*)partial,
                     lgg_partials_count(n), (float*)rec, gscale, clip_norm, skip);
  LG_CHECK_LAUNCH("lgg_finalise");
  lg_note_kernel("gg_finalise_kernel");
  return LG_OK;
}
