// Input side of the training step, on the device (/root/reference/eager_trainer.py:125-131):
//   noise     = tf.random.normal([B, noise_dim])
//   new_image = random_flip_left_right -> random_brightness(0.02) -> random_contrast(0.75, 1.003)
//               -> random_hue(0.03) -> + 0.1 * tf.random.normal(shape, 0, 0.2)
// TensorFlow's random streams cannot be reproduced (and parity treats these tensors as step INPUTS), so
// the draws come from a counter-based generator — Philox4x32-10, the stateless generator of Random123 / cuRAND / torch —
// keyed by (seed, offset): any element of any step can be regenerated independently, on any rank, in any order.
// The deterministic part of the transform (given flip mask, brightness delta, contrast factor, hue delta) follows the
// TF-1.15 image ops: brightness adds the delta; contrast scales about the per-(image, channel) mean over H x W; hue is
// the fused AdjustHue op — a rotation of the hue angle that keeps each pixel's min and max channel values, defined for
// any value range (the images here live in [-1, 1]).
// The generator, the per-pixel transform and the kernels shared with the packed uint8 input path are in augment_core.h.
#include "lg_internal.h"
#include "augment_core.h"

namespace {

// out[i] = mean + std * N(0,1); element i uses normal (i & 3) of Philox block (offset + i / 4)
__global__ __launch_bounds__(256) void randn_kernel(float* __restrict__ out, long long n, float mean, float stdv,
                                                    unsigned long long seed, unsigned long long offset) {
  const long long nblk = (n + 3) / 4, stride = (long long)gridDim.x * blockDim.x;
  for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < nblk; b += stride) {
    float z[4];
    normal4(seed, offset + (unsigned long long)b, z);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (b * 4 + k < n) out[b * 4 + k] = mean + stdv * z[k];
  }
}

// raw generator output (known-answer tests): out[4 i .. 4 i + 3] = philox(counter = offset + i, key = seed)
__global__ void philox_kernel(unsigned* __restrict__ out, int nblk, unsigned long long seed, unsigned long long offset) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nblk) return;
  const unsigned long long c = offset + (unsigned long long)i;
  const u4 r = philox4x32_10(u4{(unsigned)c, (unsigned)(c >> 32), 0u, 0u}, (unsigned)seed, (unsigned)(seed >> 32));
  out[4 * i] = r.x; out[4 * i + 1] = r.y; out[4 * i + 2] = r.z; out[4 * i + 3] = r.w;
}

// eps[b] = u_b of the gradient penalty's interpolation (gp.hip): word (b & 3) of Philox block offset + b / 4, u = (bits >> 8) / 2^24
// in [0, 1) — the resolution and mapping of the augmentation's scalar draws (draws_kernel)
__global__ __launch_bounds__(256) void uniform_kernel(float* __restrict__ out, int n, unsigned long long seed,
                                                      unsigned long long offset) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long c = offset + (unsigned long long)(i >> 2);
  const u4 r = philox4x32_10(u4{(unsigned)c, (unsigned)(c >> 32), 0u, 0u}, (unsigned)seed, (unsigned)(seed >> 32));
  const unsigned w = (i & 3) == 0 ? r.x : (i & 3) == 1 ? r.y : (i & 3) == 2 ? r.z : r.w;
  out[i] = (float)(w >> 8) * (1.0f / 16777216.0f);
}

}  // namespace

extern "C" int lg_philox4x32(unsigned* out, int nblocks, unsigned long long seed, unsigned long long offset, void* stream) {
  LG_CHECK_ARG(out && nblocks > 0, "lg_philox4x32: bad arguments");
  hipLaunchKernelGGL(philox_kernel, dim3((nblocks + 255) / 256), dim3(256), 0, (hipStream_t)stream, out, nblocks, seed, offset);
  LG_CHECK_LAUNCH("lg_philox4x32");
  return LG_OK;
}

extern "C" int lg_randn(float* out, long long n, float mean, float stdv, unsigned long long seed,
                        unsigned long long offset, void* stream) {
  LG_CHECK_ARG(out && n > 0, "lg_randn: bad arguments");
  hipLaunchKernelGGL(randn_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, out, n, mean, stdv, seed,
                     offset);
  LG_CHECK_LAUNCH("lg_randn");
  return LG_OK;
}

extern "C" size_t lg_augment_workspace_bytes(int B) { return (size_t)B * 3 * sizeof(float); }

// out = [+ noise_scale * N(0,1)] hue(dh)( contrast(cf)( flip?(img) + db ) );  img, out [B,H,W,3] (out != img);
// flip [B] bytes (device) or null; the noise of pixel i is Philox block (offset + i) under `seed`
extern "C" int lg_augment(const float* img, float* out, int B, int H, int W, const unsigned char* flip, float db, float cf,
                          float dh, float noise_scale, unsigned long long seed, unsigned long long offset,
                          void* workspace, size_t ws_bytes, void* stream) {
  LG_CHECK_ARG(img && out && img != out && workspace, "lg_augment: null pointer (or in-place call)");
  LG_CHECK_ARG(B > 0 && H > 0 && W > 0, "lg_augment: bad shape B=%d H=%d W=%d", B, H, W);
  LG_CHECK_ARG(ws_bytes >= lg_augment_workspace_bytes(B), "lg_augment: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float* means = (float*)workspace;
  hipLaunchKernelGGL(chan_mean3_kernel, dim3(B), dim3(256), 0, st, img, means, H * W);
  LG_CHECK_LAUNCH("lg_augment(mean)");
  hipLaunchKernelGGL((augment_kernel<1, F32Rows>), dim3(grid_for((long long)B * H * W)), dim3(256), 0, st, F32Rows{img, H * W}, out,
                     (float*)nullptr, (const float*)means, flip, B, H, W, db, cf, dh, noise_scale, seed, offset, (const float*)nullptr);
  LG_CHECK_LAUNCH("lg_augment");
  return LG_OK;
}

extern "C" size_t lg_augment_drawn_workspace_bytes(int B) { return drawn_workspace_bytes(B); }

// lg_augment with the random draws of eager_trainer.py:127-130 made ON THE DEVICE from the Philox window at draw_offset
// (see draws_kernel): flip per image with probability 1/2, brightness delta U(-db_max, db_max), contrast factor
// U(c_lo, c_hi), hue delta U(-dh_max, dh_max); the pixel noise uses the window at noise_offset as in lg_augment.
// The whole input side of the step is then enqueued without a host synchronisation.
extern "C" int lg_augment_drawn(const float* img, float* out, int B, int H, int W, float db_max, float c_lo, float c_hi,
                                float dh_max, float noise_scale, unsigned long long seed, unsigned long long draw_offset,
                                unsigned long long noise_offset, void* workspace, size_t ws_bytes, void* stream) {
  LG_CHECK_ARG(img && out && img != out && workspace, "lg_augment_drawn: null pointer (or in-place call)");
  LG_CHECK_ARG(B > 0 && H > 0 && W > 0, "lg_augment_drawn: bad shape B=%d H=%d W=%d", B, H, W);
  LG_CHECK_ARG(ws_bytes >= lg_augment_drawn_workspace_bytes(B), "lg_augment_drawn: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float* means = (float*)workspace;
  float* params = (float*)((char*)workspace + ((size_t)B * 3 * sizeof(float) + 15) / 16 * 16);
  unsigned char* flip = (unsigned char*)(params + 4);
  hipLaunchKernelGGL(draws_kernel, dim3((B + 3 + 255) / 256), dim3(256), 0, st, params, flip, B, db_max, c_lo, c_hi, dh_max,
                     seed, draw_offset);
  LG_CHECK_LAUNCH("lg_augment_drawn(draws)");
  hipLaunchKernelGGL(chan_mean3_kernel, dim3(B), dim3(256), 0, st, img, means, H * W);
  LG_CHECK_LAUNCH("lg_augment_drawn(mean)");
  hipLaunchKernelGGL((augment_kernel<1, F32Rows>), dim3(grid_for((long long)B * H * W)), dim3(256), 0, st, F32Rows{img, H * W}, out,
                     (float*)nullptr, (const float*)means, (const unsigned char*)flip, B, H, W, 0.f, 1.f, 1.f, noise_scale, seed, noise_offset, (const float*)params);
  LG_CHECK_LAUNCH("lg_augment_drawn");
  return LG_OK;
}

extern "C" int lg_gp_draw_eps(float* eps, int B, unsigned long long seed, unsigned long long offset, void* stream) {
  LG_CHECK_ARG(eps && B > 0, "lg_gp_draw_eps: bad arguments");
  hipLaunchKernelGGL(uniform_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, eps, B, seed, offset);
  LG_CHECK_LAUNCH("lg_gp_draw_eps");
  return LG_OK;
}
