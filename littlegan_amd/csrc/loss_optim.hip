// Losses and optimizer of the LittleGAN step.
//   bce_heads : tf.keras.losses.binary_crossentropy (TF-1.15 backend form) + reduce_mean, as combined
//               in /root/reference/eager_trainer.py:85-102, fused with the sigmoid backward of the heads:
//                 p^ = clip(p,1e-7,1-1e-7); l = -(t log(p^+1e-7) + (1-t) log(1-p^+1e-7))
//               loss (+)= w_pr * mean_b l(t_pr, p[b,0]) + w_c * mean_{b,j} l(t_c[b,j], p[b,1+j])
//               dz = dloss/dp * p(1-p)   (gradient w.r.t. the pre-sigmoid logits)
//   l1_tanh_bwd: loss (+)= lambda*mean|t - img| ; dpre = (g_in - lambda*sign(t-img)/n) * (1-img^2)
//               (eager_trainer.py:96,101 + the tanh of model.py:87)
//   clip_adam : tf.clip_by_value (eager_trainer.py:146-148) + tf.compat.v1.train.AdamOptimizer
//               (eager_trainer.py:28-30,164-168): lr_t = lr*sqrt(1-b2^t)/(1-b1^t), eps outside sqrt,
//               one beta-power pair per optimizer kept on the device so the step replays as a graph.
//               Its twins read the rate (lgsch_*) and the gradient scale and skip flag (gg_*, §30) from device memory.
#include "lg_internal.h"
#include "../../include/littlegan_sched.h"

#define LG_BCE_EPS 1e-7f

namespace {

__global__ __launch_bounds__(1024) void bce_heads_kernel(const float* __restrict__ p, const float* __restrict__ t_c,
                                                        float t_pr, float w_pr, float w_c, float* __restrict__ loss,
                                                        float* __restrict__ dz, int B, int c, int accumulate) {
  const int J = c + 1, n = B * J;
  const float s_pr = w_pr / (float)B, s_c = w_c / (float)(B * c);
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {  // one block (the loss is ONE scalar): 1024 threads, <= 21 trips at B=512
    const int b = i / J, j = i - b * J;
    const float sc = j == 0 ? s_pr : s_c;
    float g = 0.f;
    if (sc != 0.f) {
      const float t = j == 0 ? t_pr : t_c[b * c + j - 1];
      const float pv = p[i];
      const float pc = fminf(fmaxf(pv, LG_BCE_EPS), 1.f - LG_BCE_EPS);
      acc += -sc * (t * logf(pc + LG_BCE_EPS) + (1.f - t) * logf(1.f - pc + LG_BCE_EPS));
      const bool inside = pv >= LG_BCE_EPS && pv <= 1.f - LG_BCE_EPS;
      if (inside) g = -sc * (t / (pc + LG_BCE_EPS) - (1.f - t) / (1.f - pc + LG_BCE_EPS)) * pv * (1.f - pv);
    }
    dz[i] = g;
  }
  __shared__ float sred[16];
  float red[1] = {acc};
  lg_block_sum<1>(red, sred);
  if (threadIdx.x == 0) loss[0] = (accumulate ? loss[0] : 0.f) + red[0];
}

// partial[blk] = sum |t - img| ; dpre written
__global__ __launch_bounds__(256) void l1_tanh_bwd_kernel(const float* __restrict__ t, const float* __restrict__ img,
                                                          const float* __restrict__ g_in, float* __restrict__ dpre,
                                                          float* __restrict__ partial, long long n4, float gscale) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  float acc = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const f32x4 tv = *reinterpret_cast<const f32x4*>(t + i * 4);
    const f32x4 iv = *reinterpret_cast<const f32x4*>(img + i * 4);
    f32x4 gv = g_in ? *reinterpret_cast<const f32x4*>(g_in + i * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = tv[k] - iv[k];
      acc += fabsf(d);
      const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
      o[k] = (gv[k] - gscale * sg) * (1.f - iv[k] * iv[k]);
    }
    if (dpre) *reinterpret_cast<f32x4*>(dpre + i * 4) = o;
  }
  __shared__ float sred[16];
  float red[1] = {acc};
  lg_block_sum<1>(red, sred);
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void l1_final_kernel(const float* __restrict__ partial, int nb, float scale,
                                                       float* __restrict__ loss, int accumulate) {
  __shared__ double sd[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) s += (double)partial[i];
  sd[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sd[threadIdx.x] += sd[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (accumulate ? loss[0] : 0.f) + (float)(sd[0] * (double)scale);
}

// One element of clip + Adam, shared by the plain and the EMA-fused kernel so that both give the same bits (the library is built
// with -ffp-contract=off: the same expressions are the same IEEE operations).  Returns the new weight.
__device__ __forceinline__ float clip_adam_element(float w, float g, float& m, float& v, float lr_t, float b1, float b2, float eps,
                                                   float clip, float gscale) {
  float gv = g * gscale;
  if (clip > 0.f) gv = fminf(fmaxf(gv, -clip), clip);
  const float mv = b1 * m + (1.f - b1) * gv;
  const float vv = b2 * v + (1.f - b2) * gv * gv;
  m = mv; v = vv;
  return w - lr_t * mv / (sqrtf(vv) + eps);
}

// The grid-stride pass of clip + Adam over n elements at the bias-corrected rate lr_t: the body of clip_adam_kernel and of its twin that
// reads the rate from device memory (littlegan_sched.h), so that both are the same instructions after the one line that forms lr_t.
// (i0 and stride come from the kernel: with blockDim read in here the compiler fetches it another way than it did for clip_adam_kernel
// before the pass was taken out, and that kernel's instructions are to stay what they were.)
__device__ __forceinline__ void clip_adam_pass(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, long long n, long long i0, long long stride, float lr_t,
                                               float b1, float b2, float eps, float clip, float gscale) {
  for (long long i = i0; i < n; i += stride) {
    float mv = m[i], vv = v[i];
    w[i] = clip_adam_element(w[i], g[i], mv, vv, lr_t, b1, b2, eps, clip, gscale);
    m[i] = mv; v[i] = vv;
  }
}

// state = {beta1_power, beta2_power}
__global__ __launch_bounds__(256) void clip_adam_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, long long n,
                                                        const float* __restrict__ state, float lr, float b1, float b2,
                                                        float eps, float clip, float gscale) {
  const float lr_t = lr * sqrtf(1.f - state[1]) / (1.f - state[0]);
  const long long stride = (long long)gridDim.x * blockDim.x;
  clip_adam_pass(w, g, m, v, n, (long long)blockIdx.x * blockDim.x + threadIdx.x, stride, lr_t, b1, b2, eps, clip, gscale);
}

// ... with the rate of the present step read from the schedule's state: lr[0] where the launch scalar stands above
__global__ __launch_bounds__(256) void clip_adam_lrp_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v, long long n,
                                                            const float* __restrict__ state, const float* __restrict__ lr, float b1,
                                                            float b2, float eps, float clip, float gscale) {
  const float lr_t = lr[0] * sqrtf(1.f - state[1]) / (1.f - state[0]);
  const long long stride = (long long)gridDim.x * blockDim.x;
  clip_adam_pass(w, g, m, v, n, (long long)blockIdx.x * blockDim.x + threadIdx.x, stride, lr_t, b1, b2, eps, clip, gscale);
}

// 1 - d_t of the weight average below, from the device counter of averages taken
__device__ __forceinline__ float ema_one_minus_decay(const int* __restrict__ ema_state, float decay) {
  const float kf = (float)ema_state[0];
  return 1.f - fminf(decay, (1.f + kf) / (10.f + kf));
}

// clip + Adam on the 4-float groups [lo4, hi4) of one model's weights, and the weight average on ALL of its n4 groups:
//   ema -= (1 - d_t) * (ema - w),  d_t = min(decay, (1 + k) / (10 + k)),  k = ema_state[0] = averages taken so far
// (tf.train.ExponentialMovingAverage(decay, num_updates)).  d_t is computed here, from the device counter: a captured graph bakes
// launch scalars in, a replayed step still walks the ramp.  Outside [lo4, hi4) nothing but w and ema is touched: on a partition
// step the gradients there are stale and were not all-reduced.  16-byte accesses; the caller guarantees the alignment.
// (The pass of clip_adam_ema_kernel and of its twin that reads the rate from device memory; i0, stride as for clip_adam_pass.)
__device__ __forceinline__ void clip_adam_ema_pass(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, float* __restrict__ ema, long long n4, long long lo4,
                                                   long long hi4, long long i0, long long stride, float omd, float lr_t, float b1,
                                                   float b2, float eps, float clip, float gscale) {
  for (long long i = i0; i < n4; i += stride) {
    f32x4 wv = *reinterpret_cast<const f32x4*>(w + i * 4);
    if (i >= lo4 && i < hi4) {
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i * 4);
      f32x4 mv = *reinterpret_cast<const f32x4*>(m + i * 4);
      f32x4 vv = *reinterpret_cast<const f32x4*>(v + i * 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float mk = mv[k], vk = vv[k];
        wv[k] = clip_adam_element(wv[k], gv[k], mk, vk, lr_t, b1, b2, eps, clip, gscale);
        mv[k] = mk; vv[k] = vk;
      }
      *reinterpret_cast<f32x4*>(m + i * 4) = mv;
      *reinterpret_cast<f32x4*>(v + i * 4) = vv;
      *reinterpret_cast<f32x4*>(w + i * 4) = wv;
    }
    f32x4 ev = *reinterpret_cast<const f32x4*>(ema + i * 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) ev[k] -= omd * (ev[k] - wv[k]);
    *reinterpret_cast<f32x4*>(ema + i * 4) = ev;
  }
}

__global__ __launch_bounds__(256) void clip_adam_ema_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v,
                                                            float* __restrict__ ema, long long n4, long long lo4, long long hi4,
                                                            const float* __restrict__ state, const int* __restrict__ ema_state,
                                                            float lr, float b1, float b2, float eps, float clip, float gscale,
                                                            float decay) {
  const float lr_t = lr * sqrtf(1.f - state[1]) / (1.f - state[0]);
  const float omd = ema_one_minus_decay(ema_state, decay);
  const long long stride = (long long)gridDim.x * blockDim.x;
  clip_adam_ema_pass(w, g, m, v, ema, n4, lo4, hi4, (long long)blockIdx.x * blockDim.x + threadIdx.x, stride, omd, lr_t, b1, b2, eps,
                     clip, gscale);
}

// ... with the rate of the present step read from the schedule's state
__global__ __launch_bounds__(256) void clip_adam_ema_lrp_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                                float* __restrict__ m, float* __restrict__ v,
                                                                float* __restrict__ ema, long long n4, long long lo4, long long hi4,
                                                                const float* __restrict__ state, const int* __restrict__ ema_state,
                                                                const float* __restrict__ lr, float b1, float b2, float eps, float clip,
                                                                float gscale, float decay) {
  const float lr_t = lr[0] * sqrtf(1.f - state[1]) / (1.f - state[0]);
  const float omd = ema_one_minus_decay(ema_state, decay);
  const long long stride = (long long)gridDim.x * blockDim.x;
  clip_adam_ema_pass(w, g, m, v, ema, n4, lo4, hi4, (long long)blockIdx.x * blockDim.x + threadIdx.x, stride, omd, lr_t, b1, b2, eps,
                     clip, gscale);
}

// ... with the gradient scale and the skip flag read from the guard's record (include/littlegan_guard.h): rec[1] = eff where
// the launch scalar gscale stands above, the rate from device memory as in the _lrp twin; a skipped step returns before any access
__global__ __launch_bounds__(256) void clip_adam_gg_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, long long n, const float* __restrict__ state,
                                                           const float* __restrict__ lr, const float* __restrict__ rec, float b1,
                                                           float b2, float eps, float clip) {
  if (__float_as_int(rec[2]) != 0) return;
  const float rate = lr[0], eff = rec[1];
  const float lr_t = rate * sqrtf(1.f - state[1]) / (1.f - state[0]);
  const long long stride = (long long)gridDim.x * blockDim.x;
  clip_adam_pass(w, g, m, v, n, (long long)blockIdx.x * blockDim.x + threadIdx.x, stride, lr_t, b1, b2, eps, clip, eff);
}

// ... and the EMA-fused pass in the same way: a skipped step takes the average alone, as with lo4 == hi4
__global__ __launch_bounds__(256) void clip_adam_ema_gg_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                               float* __restrict__ m, float* __restrict__ v, float* __restrict__ ema,
                                                               long long n4, long long lo4, long long hi4,
                                                               const float* __restrict__ state, const int* __restrict__ ema_state,
                                                               const float* __restrict__ lr, const float* __restrict__ rec, float b1,
                                                               float b2, float eps, float clip, float decay) {
  const float rate = lr[0], eff = rec[1];
  const float lr_t = rate * sqrtf(1.f - state[1]) / (1.f - state[0]);
  const float omd = ema_one_minus_decay(ema_state, decay);
  const long long hi_now = __float_as_int(rec[2]) != 0 ? lo4 : hi4;
  const long long stride = (long long)gridDim.x * blockDim.x;
  clip_adam_ema_pass(w, g, m, v, ema, n4, lo4, hi_now, (long long)blockIdx.x * blockDim.x + threadIdx.x, stride, omd, lr_t, b1, b2, eps,
                     clip, eff);
}

__global__ void adam_advance_gg_kernel(float* state, const float* __restrict__ rec, float b1, float b2) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && __float_as_int(rec[2]) == 0) { state[0] *= b1; state[1] *= b2; }
}

__global__ void adam_advance_kernel(float* state, float b1, float b2) {
  if (threadIdx.x == 0 && blockIdx.x == 0) { state[0] *= b1; state[1] *= b2; }
}

// the count of averages taken: once per step, after the last launch that read it; saturates
__global__ void ema_advance_kernel(int* ema_state) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && ema_state[0] < 0x7fffffff) ema_state[0] += 1;
}

__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, long long n4) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const f32x4 av = *reinterpret_cast<const f32x4*>(a + i * 4);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(b + i * 4);
    *reinterpret_cast<f32x4*>(a + i * 4) = bv;
    *reinterpret_cast<f32x4*>(b + i * 4) = av;
  }
}

__global__ __launch_bounds__(256) void axpby_kernel(float* __restrict__ y, const float* __restrict__ x, float a, float b,
                                                    long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = a * x[i] + b * y[i];
}

}  // namespace

extern "C" int lg_bce_heads_loss_fwd_bwd(const float* p, const float* t_c, float t_pr, float w_pr, float w_c,
                                         float* loss, float* dz, int B, int c, int accumulate, void* stream) {
  LG_CHECK_ARG(p && loss && dz, "lg_bce_heads_loss_fwd_bwd: null pointer");
  LG_CHECK_ARG(B > 0 && c >= 1, "lg_bce_heads_loss_fwd_bwd: bad shape B=%d c=%d", B, c);
  LG_CHECK_ARG(t_c || w_c == 0.f, "lg_bce_heads_loss_fwd_bwd: t_c is null but w_c != 0");
  hipLaunchKernelGGL(bce_heads_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, p, t_c, t_pr, w_pr, w_c, loss, dz, B,
                     c, accumulate);
  LG_CHECK_LAUNCH("lg_bce_heads_loss_fwd_bwd");
  return LG_OK;
}

extern "C" size_t lg_l1_workspace_bytes(void) { return 1024 * sizeof(float); }

// loss (+)= lambda*mean|t-img| ; dpre = (g_in - lambda*sign(t-img)/n)*(1-img^2)  (dpre may be null: loss only)
extern "C" int lg_l1_tanh_loss_fwd_bwd(const float* t, const float* img, const float* g_in, float* dpre, float* loss,
                                       void* workspace, size_t ws_bytes, long long n, float lambda, int accumulate,
                                       void* stream) {
  LG_CHECK_ARG(t && img && loss && workspace, "lg_l1_tanh_loss_fwd_bwd: null pointer");
  LG_CHECK_ARG(n > 0 && n % 4 == 0, "lg_l1_tanh_loss_fwd_bwd: n=%lld must be a positive multiple of 4", n);
  LG_CHECK_ARG(ws_bytes >= lg_l1_workspace_bytes(), "lg_l1_tanh_loss_fwd_bwd: workspace too small");
  const long long n4 = n / 4;
  int nb = (int)((n4 + 255) / 256);
  if (nb > 1024) nb = 1024;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(l1_tanh_bwd_kernel, dim3(nb), dim3(256), 0, st, t, img, g_in, dpre, (float*)workspace, n4,
                     lambda / (float)n);
  LG_CHECK_LAUNCH("lg_l1_tanh_loss_fwd_bwd");
  hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, nb, lambda / (float)n, loss,
                     accumulate);
  LG_CHECK_LAUNCH("lg_l1_tanh_loss_fwd_bwd(final)");
  return LG_OK;
}

extern "C" int lg_clip_adam_update(float* w, const float* g, float* m, float* v, long long n, const float* state,
                                   float lr, float b1, float b2, float eps, float clip, float gscale, void* stream) {
  LG_CHECK_ARG(w && g && m && v && state, "lg_clip_adam_update: null pointer");
  LG_CHECK_ARG(n > 0, "lg_clip_adam_update: n=%lld", n);
  long long nb = (n + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(clip_adam_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, w, g, m, v, n, state, lr, b1, b2,
                     eps, clip, gscale);
  LG_CHECK_LAUNCH("lg_clip_adam_update");
  return LG_OK;
}

extern "C" int lg_adam_advance(float* state, float b1, float b2, void* stream) {
  LG_CHECK_ARG(state, "lg_adam_advance: null pointer");
  hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, b1, b2);
  LG_CHECK_LAUNCH("lg_adam_advance");
  return LG_OK;
}

// clip + Adam on [lo, hi) of one model's range [0, n) and the weight average over all of it (lo == hi: the average alone); no
// reference counterpart: tf.train.ExponentialMovingAverage(decay, num_updates) semantics, num_updates = ema_state[0] on the device
extern "C" int lg_clip_adam_ema_update(float* w, const float* g, float* m, float* v, float* ema, long long n, long long lo,
                                       long long hi, const float* adam_state, const int* ema_state, float lr, float b1, float b2,
                                       float eps, float clip, float gscale, float decay, void* stream) {
  LG_CHECK_ARG(w && g && m && v && ema && adam_state && ema_state, "lg_clip_adam_ema_update: null pointer");
  LG_CHECK_ARG(n > 0 && n % 4 == 0, "lg_clip_adam_ema_update: n=%lld must be a positive multiple of 4", n);
  LG_CHECK_ARG(lo >= 0 && lo <= hi && hi <= n && lo % 4 == 0 && hi % 4 == 0,
               "lg_clip_adam_ema_update: need 0 <= lo <= hi <= n, both multiples of 4 (lo=%lld hi=%lld n=%lld)", lo, hi, n);
  LG_CHECK_ARG(((uintptr_t)w | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) % 16 == 0,
               "lg_clip_adam_ema_update: w, g, m, v, ema must be 16-byte aligned");
  LG_CHECK_ARG(decay >= 0.f && decay < 1.f, "lg_clip_adam_ema_update: decay=%g outside [0, 1)", (double)decay);
  const long long n4 = n / 4;
  long long nb = (n4 + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(clip_adam_ema_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, w, g, m, v, ema, n4, lo / 4, hi / 4,
                     adam_state, ema_state, lr, b1, b2, eps, clip, gscale, decay);
  LG_CHECK_LAUNCH("lg_clip_adam_ema_update");
  return LG_OK;
}

// lg_clip_adam_update with the rate in device memory (include/littlegan_sched.h): the same grid, the same pass
extern "C" int lgsch_clip_adam_update(float* w, const float* g, float* m, float* v, long long n, const float* state, const float* lr,
                                      float b1, float b2, float eps, float clip, float gscale, void* stream) {
  LG_CHECK_ARG(w && g && m && v && state && lr, "lgsch_clip_adam_update: null pointer");
  LG_CHECK_ARG(((uintptr_t)lr & 3) == 0, "lgsch_clip_adam_update: lr must be 4-byte aligned");
  LG_CHECK_ARG(n > 0, "lgsch_clip_adam_update: n=%lld", n);
  long long nb = (n + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(clip_adam_lrp_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, w, g, m, v, n, state, lr, b1, b2, eps,
                     clip, gscale);
  LG_CHECK_LAUNCH("lgsch_clip_adam_update");
  lg_note_kernel("clip_adam_lrp_kernel");
  return LG_OK;
}

// lg_clip_adam_ema_update with the rate in device memory
extern "C" int lgsch_clip_adam_ema_update(float* w, const float* g, float* m, float* v, float* ema, long long n, long long lo,
                                          long long hi, const float* adam_state, const int* ema_state, const float* lr, float b1,
                                          float b2, float eps, float clip, float gscale, float decay, void* stream) {
  LG_CHECK_ARG(w && g && m && v && ema && adam_state && ema_state && lr, "lgsch_clip_adam_ema_update: null pointer");
  LG_CHECK_ARG(n > 0 && n % 4 == 0, "lgsch_clip_adam_ema_update: n=%lld must be a positive multiple of 4", n);
  LG_CHECK_ARG(lo >= 0 && lo <= hi && hi <= n && lo % 4 == 0 && hi % 4 == 0,
               "lgsch_clip_adam_ema_update: need 0 <= lo <= hi <= n, both multiples of 4 (lo=%lld hi=%lld n=%lld)", lo, hi, n);
  LG_CHECK_ARG(((uintptr_t)w | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) % 16 == 0 && ((uintptr_t)lr & 3) == 0,
               "lgsch_clip_adam_ema_update: w, g, m, v, ema must be 16-byte, lr 4-byte aligned");
  LG_CHECK_ARG(decay >= 0.f && decay < 1.f, "lgsch_clip_adam_ema_update: decay=%g outside [0, 1)", (double)decay);
  const long long n4 = n / 4;
  long long nb = (n4 + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(clip_adam_ema_lrp_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, w, g, m, v, ema, n4, lo / 4, hi / 4,
                     adam_state, ema_state, lr, b1, b2, eps, clip, gscale, decay);
  LG_CHECK_LAUNCH("lgsch_clip_adam_ema_update");
  lg_note_kernel("clip_adam_ema_lrp_kernel");
  return LG_OK;
}

// lgsch_clip_adam_update with the scale and the skip flag in device memory (include/littlegan_guard.h): the same grid, the same pass
extern "C" int lgg_clip_adam_update(float* w, const float* g, float* m, float* v, long long n, const float* adam_state, const float* lr,
                                   const void* rec, float b1, float b2, float eps, float clip, void* stream) {
  LG_CHECK_ARG(w && g && m && v && adam_state && lr && rec, "lgg_clip_adam_update: null pointer");
  LG_CHECK_ARG(((uintptr_t)lr & 3) == 0 && ((uintptr_t)rec & 15) == 0, "lgg_clip_adam_update: lr must be 4-byte, rec 16-byte aligned");
  LG_CHECK_ARG(n > 0, "lgg_clip_adam_update: n=%lld", n);
  long long nb = (n + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(clip_adam_gg_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, w, g, m, v, n, adam_state, lr,
                     (const float*)rec, b1, b2, eps, clip);
  LG_CHECK_LAUNCH("lgg_clip_adam_update");
  lg_note_kernel("clip_adam_gg_kernel");
  return LG_OK;
}

// lgsch_clip_adam_ema_update with the scale and the skip flag in device memory
extern "C" int lgg_clip_adam_ema_update(float* w, const float* g, float* m, float* v, float* ema, long long n, long long lo, long long hi,
                                       const float* adam_state, const int* ema_state, const float* lr, const void* rec, float b1,
                                       float b2, float eps, float clip, float decay, void* stream) {
  LG_CHECK_ARG(w && g && m && v && ema && adam_state && ema_state && lr && rec, "lgg_clip_adam_ema_update: null pointer");
  LG_CHECK_ARG(n > 0 && n % 4 == 0, "lgg_clip_adam_ema_update: n=%lld must be a positive multiple of 4", n);
  LG_CHECK_ARG(lo >= 0 && lo <= hi && hi <= n && lo % 4 == 0 && hi % 4 == 0,
               "lgg_clip_adam_ema_update: need 0 <= lo <= hi <= n, both multiples of 4 (lo=%lld hi=%lld n=%lld)", lo, hi, n);
  LG_CHECK_ARG(((uintptr_t)w | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema | (uintptr_t)rec) % 16 == 0 &&
                   ((uintptr_t)lr & 3) == 0,
               "lgg_clip_adam_ema_update: w, g, m, v, ema, rec must be 16-byte, lr 4-byte aligned");
  LG_CHECK_ARG(decay >= 0.f && decay < 1.f, "lgg_clip_adam_ema_update: decay=%g outside [0, 1)", (double)decay);
  const long long n4 = n / 4;
  long long nb = (n4 + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(clip_adam_ema_gg_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, w, g, m, v, ema, n4, lo / 4, hi / 4,
                     adam_state, ema_state, lr, (const float*)rec, b1, b2, eps, clip, decay);
  LG_CHECK_LAUNCH("lgg_clip_adam_ema_update");
  lg_note_kernel("clip_adam_ema_gg_kernel");
  return LG_OK;
}

// lg_adam_advance unless the record says that this step is skipped
extern "C" int lgg_adam_advance(float* adam_state, const void* rec, float b1, float b2, void* stream) {
  LG_CHECK_ARG(adam_state && rec, "lgg_adam_advance: null pointer");
  LG_CHECK_ARG(((uintptr_t)rec & 15) == 0, "lgg_adam_advance: rec must be 16-byte aligned");
  hipLaunchKernelGGL(adam_advance_gg_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, adam_state, (const float*)rec, b1, b2);
  LG_CHECK_LAUNCH("lgg_adam_advance");
  lg_note_kernel("adam_advance_gg_kernel");
  return LG_OK;
}

extern "C" int lg_ema_advance(int* ema_state, void* stream) {
  LG_CHECK_ARG(ema_state, "lg_ema_advance: null pointer");
  hipLaunchKernelGGL(ema_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ema_state);
  LG_CHECK_LAUNCH("lg_ema_advance");
  return LG_OK;
}

// a <-> b in place (raw weights <-> their average: no address a captured graph holds changes)
extern "C" int lg_swap_f32(float* a, float* b, long long n, void* stream) {
  LG_CHECK_ARG(a && b, "lg_swap_f32: null pointer");
  LG_CHECK_ARG(a != b, "lg_swap_f32: a and b are the same buffer");
  LG_CHECK_ARG(n > 0 && n % 4 == 0, "lg_swap_f32: n=%lld must be a positive multiple of 4", n);
  LG_CHECK_ARG(((uintptr_t)a | (uintptr_t)b) % 16 == 0, "lg_swap_f32: a, b must be 16-byte aligned");
  const long long n4 = n / 4;
  long long nb = (n4 + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(swap_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, a, b, n4);
  LG_CHECK_LAUNCH("lg_swap_f32");
  return LG_OK;
}

// y = a*x + b*y
extern "C" int lg_axpby(float* y, const float* x, float a, float b, long long n, void* stream) {
  LG_CHECK_ARG(x && y && n > 0, "lg_axpby: bad args");
  long long nb = (n + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(axpby_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, y, x, a, b, n);
  LG_CHECK_LAUNCH("lg_axpby");
  return LG_OK;
}
