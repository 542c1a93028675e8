// Input side of the step from a PACKED data set: the images are rows of one uint8 array [N][H][W][3] that
// lives on the device (or a [B][H][W][3] slot that has just been streamed to it), a batch is a vector of B row indices.
//   lg_rescale_u8       out[b][e] = (float)src[idx[b]][e] / 127.5f - 1.0f            data_rescale, utils.py:51-52
//   lg_soft_labels      out[b][j] = 0.96f * attr[idx[b]][cols[j]] + 0.02f            soft, utils.py:47-48
//   lg_augment_drawn_u8 lg_augment_drawn with the rescale in front of it and the gather in its addressing: one read of
//                       the bytes gives both the augmented image and the plain rescaled one
// All three produce, bit for bit, what the float32 path produces from the rescaled copy of the same rows; the shared
// device code and the argument for the augmentation are in augment_core.h.  HBM-bound streaming work: no MFMA, no LDS
// beyond the mean pass's staging tile.
#include "lg_internal.h"
#include "augment_core.h"

namespace {

// 16 bytes -> 16 floats per thread: one 16-byte load, four 16-byte stores.  row_elems % 16 == 0, src and out 16-byte aligned.
__global__ __launch_bounds__(256) void rescale_u8_vec_kernel(const unsigned char* __restrict__ src,
                                                             const long long* __restrict__ idx, long long nchunk, int cpr,
                                                             float* __restrict__ out) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < nchunk; c += stride) {
    const long long b = c / cpr;
    const int e = (int)(c % cpr);
    const u32x4 v = reinterpret_cast<const u32x4*>(src + idx[b] * (long long)cpr * 16)[e];
    f32x4* o = reinterpret_cast<f32x4*>(out + c * 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned w = v[k];
      o[k] = f32x4{rescale_u8(w & 255u), rescale_u8((w >> 8) & 255u), rescale_u8((w >> 16) & 255u), rescale_u8(w >> 24)};
    }
  }
}

// any row length, any alignment: one element per thread
__global__ __launch_bounds__(256) void rescale_u8_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ idx,
                                                         long long n, long long row_elems, float* __restrict__ out) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const long long b = i / row_elems, e = i % row_elems;
    out[i] = rescale_u8(src[idx[b] * row_elems + e]);
  }
}

__global__ __launch_bounds__(256) void soft_labels_kernel(const float* __restrict__ attr, const long long* __restrict__ idx,
                                                          const int* __restrict__ cols, int B, int A_all, int c,
                                                          float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * c) return;
  const int b = i / c, j = i % c;
  const float t = 0.96f * attr[idx[b] * (long long)A_all + cols[j]];   // product rounded, then the sum (no contraction)
  out[i] = t + 0.02f;
}

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

}  // namespace

extern "C" int lg_rescale_u8(const unsigned char* src, const long long* idx, int B, long long row_elems, float* out,
                             void* stream) {
  LG_CHECK_ARG(src && idx && out, "lg_rescale_u8: null pointer");
  LG_CHECK_ARG(B > 0 && row_elems > 0, "lg_rescale_u8: bad shape B=%d row_elems=%lld", B, row_elems);
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)B * row_elems;
  if (row_elems % 16 == 0 && row_elems / 16 <= 0x7fffffffLL && aligned(src, 16) && aligned(out, 16)) {
    hipLaunchKernelGGL(rescale_u8_vec_kernel, dim3(grid_for(n / 16)), dim3(256), 0, st, src, idx, n / 16, (int)(row_elems / 16), out);
  } else {
    hipLaunchKernelGGL(rescale_u8_kernel, dim3(grid_for(n)), dim3(256), 0, st, src, idx, n, row_elems, out);
  }
  LG_CHECK_LAUNCH("lg_rescale_u8");
  return LG_OK;
}

extern "C" int lg_soft_labels(const float* attr, const long long* idx, const int* cols, int B, int A_all, int c, float* out,
                              void* stream) {
  LG_CHECK_ARG(attr && idx && cols && out, "lg_soft_labels: null pointer");
  LG_CHECK_ARG(B > 0 && A_all > 0 && c > 0 && (long long)B * c <= 0x7fffffffLL, "lg_soft_labels: bad shape B=%d A_all=%d c=%d", B, A_all, c);
  hipLaunchKernelGGL(soft_labels_kernel, dim3((B * c + 255) / 256), dim3(256), 0, (hipStream_t)stream, attr, idx, cols, B, A_all,
                     c, out);
  LG_CHECK_LAUNCH("lg_soft_labels");
  return LG_OK;
}

extern "C" size_t lg_augment_drawn_u8_workspace_bytes(int B) { return drawn_workspace_bytes(B); }

// out_aug = lg_augment_drawn(rescale(src[idx])), out_rescaled (may be null) = rescale(src[idx]); see include/littlegan_hip.h
extern "C" int lg_augment_drawn_u8(const unsigned char* src, const long long* idx, float* out_aug, float* out_rescaled, int B,
                                   int H, int W, float db_max, float c_lo, float c_hi, float dh_max, float noise_scale,
                                   unsigned long long seed, unsigned long long draw_offset, unsigned long long noise_offset,
                                   void* workspace, size_t ws_bytes, void* stream) {
  LG_CHECK_ARG(src && idx && out_aug && workspace, "lg_augment_drawn_u8: null pointer");
  LG_CHECK_ARG(out_aug != out_rescaled, "lg_augment_drawn_u8: out_aug and out_rescaled are the same buffer");
  LG_CHECK_ARG(B > 0 && H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL / 3, "lg_augment_drawn_u8: bad shape B=%d H=%d W=%d", B, H, W);
  LG_CHECK_ARG(ws_bytes >= lg_augment_drawn_u8_workspace_bytes(B), "lg_augment_drawn_u8: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float* means = (float*)workspace;
  float* params = (float*)((char*)workspace + ((size_t)B * 3 * sizeof(float) + 15) / 16 * 16);
  unsigned char* flip = (unsigned char*)(params + 4);
  const int HW = H * W;
  const U8Gather rows{src, idx, HW};
  hipLaunchKernelGGL(draws_kernel, dim3((B + 3 + 255) / 256), dim3(256), 0, st, params, flip, B, db_max, c_lo, c_hi, dh_max,
                     seed, draw_offset);
  LG_CHECK_LAUNCH("lg_augment_drawn_u8(draws)");
  const int vec_rows = aligned(src, 16) && ((long long)HW * 3) % 16 == 0;
  hipLaunchKernelGGL(chan_mean3_u8_kernel, dim3(B), dim3(256), 0, st, rows, means, HW, vec_rows);
  LG_CHECK_LAUNCH("lg_augment_drawn_u8(mean)");
  // 4 pixels per thread (12 bytes in, 2 x 48 bytes out as 16-byte stores) when the rows split into aligned groups of 4
  const bool g4 = W % 4 == 0 && aligned(src, 4) && aligned(out_aug, 16) && aligned(out_rescaled, 16);
  if (g4)
    hipLaunchKernelGGL((augment_kernel<4, U8Gather>), dim3(grid_for((long long)B * H * (W / 4))), dim3(256), 0, st, rows, out_aug,
                       out_rescaled, (const float*)means, (const unsigned char*)flip, B, H, W, 0.f, 1.f, 1.f, noise_scale, seed,
                       noise_offset, (const float*)params);
  else
    hipLaunchKernelGGL((augment_kernel<1, U8Gather>), dim3(grid_for((long long)B * H * W)), dim3(256), 0, st, rows, out_aug,
                       out_rescaled, (const float*)means, (const unsigned char*)flip, B, H, W, 0.f, 1.f, 1.f, noise_scale, seed,
                       noise_offset, (const float*)params);
  LG_CHECK_LAUNCH("lg_augment_drawn_u8");
  return LG_OK;
}
