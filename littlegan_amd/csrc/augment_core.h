// Device code shared by the two input-side translation units: augment.hip (float32 images that have already arrived) and
// input_u8.hip (rows of a packed uint8 data set, gathered by index and rescaled on load).  The generator, the draws, the
// per-pixel transform and the two kernels live here ONCE, parameterised on a source accessor, so that the uint8 entry
// point computes bit for bit what lg_augment_drawn computes on the rescaled float32 copy of the same rows: the same
// float32 values enter the same expressions in the same order (the library is built with -ffp-contract=off, so an
// expression means the same roundings in every instantiation).
#pragma once
#include "lg_common.h"
#include "philox.h"

namespace {

// 32 random bits -> (0, 1]  (never 0: safe for the log of Box-Muller), 24-bit resolution like cuRAND's uniform
__device__ __forceinline__ float u01(unsigned b) { return ((float)(b >> 8) + 1.0f) * (1.0f / 16777216.0f); }

// 4 standard normals from one Philox block (two Box-Muller pairs)
__device__ __forceinline__ void normal4(unsigned long long seed, unsigned long long ctr, float (&z)[4]) {
  const u4 r = philox4x32_10(u4{(unsigned)ctr, (unsigned)(ctr >> 32), 0u, 0u}, (unsigned)seed, (unsigned)(seed >> 32));
  const float r0 = sqrtf(-2.0f * logf(u01(r.x))), r1 = sqrtf(-2.0f * logf(u01(r.z)));
  float s0, c0, s1, c1;
  sincosf(6.28318530717958647692f * u01(r.y), &s0, &c0);
  sincosf(6.28318530717958647692f * u01(r.w), &s1, &c1);
  z[0] = r0 * c0; z[1] = r0 * s0; z[2] = r1 * c1; z[3] = r1 * s1;
}

// data_rescale of one byte (utils.py:51-52): a correctly rounded IEEE division, then the subtraction.  Multiplying by a
// rounded 1 / 127.5 instead gives another float32 for 111 of the 256 byte values.
__device__ __forceinline__ float rescale_u8(unsigned b) { return (float)b / 127.5f - 1.0f; }

// ---- source accessors: pixel `pix` (0 .. H*W-1) of image n, 3 channels -----------------------------------------------
struct F32Rows {   // float32 [B][H*W][3]
  const float* img;
  int HW;
  template <int G>
  __device__ __forceinline__ void load(int n, int pix, float (&p)[G][3]) const {
    const float* q = img + ((long long)n * HW + pix) * 3;
#pragma unroll
    for (int j = 0; j < G; ++j) { p[j][0] = q[j * 3]; p[j][1] = q[j * 3 + 1]; p[j][2] = q[j * 3 + 2]; }
  }
};

struct U8Gather {  // uint8 [N][H*W][3], image n is row idx[n]; rescaled to [-1, 1] on load
  const unsigned char* src;
  const long long* idx;
  int HW;
  __device__ __forceinline__ const unsigned char* row(int n) const { return src + idx[n] * (long long)HW * 3; }
  // G == 4: the 12 bytes of 4 pixels as three aligned 4-byte loads (the caller guarantees src % 4 == 0, H*W % 4 == 0 and
  // pix % 4 == 0), a wave reads 768 contiguous bytes; G == 1: three byte loads
  template <int G>
  __device__ __forceinline__ void load(int n, int pix, float (&p)[G][3]) const {
    const unsigned char* q = row(n) + (long long)pix * 3;
    if constexpr (G == 4) {
      const unsigned* w = reinterpret_cast<const unsigned*>(q);
      const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
      const unsigned by[12] = {w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u, w0 >> 24, w1 & 255u, (w1 >> 8) & 255u,
                               (w1 >> 16) & 255u, w1 >> 24, w2 & 255u, (w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24};
#pragma unroll
      for (int j = 0; j < 4; ++j) { p[j][0] = rescale_u8(by[j * 3]); p[j][1] = rescale_u8(by[j * 3 + 1]); p[j][2] = rescale_u8(by[j * 3 + 2]); }
    } else {
#pragma unroll
      for (int j = 0; j < G; ++j) { p[j][0] = rescale_u8(q[j * 3]); p[j][1] = rescale_u8(q[j * 3 + 1]); p[j][2] = rescale_u8(q[j * 3 + 2]); }
    }
  }
};

// ---- per-(image, channel) means ------------------------------------------------------------------------------------
// One block of 256 threads per image.  Thread t adds pixels t, t + 256, t + 512, ... in that order into three float32
// sums; the 256 partial sums are merged in fp64 (lg_block_sum_d) and divided by H*W in fp64.  Both mean kernels below
// finish through this function and feed it the same float32 values in the same order, hence the same means.
__device__ __forceinline__ void chan_mean3_finish(const float (&s)[3], float* __restrict__ means, int HW) {
  __shared__ double sred[48];
  double d[3] = {(double)s[0], (double)s[1], (double)s[2]};
  lg_block_sum_d<3>(d, sred);
  if (threadIdx.x == 0)
    for (int c = 0; c < 3; ++c) means[blockIdx.x * 3 + c] = (float)(d[c] / (double)HW);
}

// means[b][c] = mean over H x W of img[b][..][c]   (3 channels; one block per image, fp64 merge)
__global__ __launch_bounds__(256) void chan_mean3_kernel(const float* __restrict__ img, float* __restrict__ means,
                                                         int HW) {
  const float* p = img + (long long)blockIdx.x * HW * 3;
  float s[3] = {0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < HW; i += 256) { s[0] += p[i * 3]; s[1] += p[i * 3 + 1]; s[2] += p[i * 3 + 2]; }
  chan_mean3_finish(s, means, HW);
}

// The same from the bytes of row idx[b].  The image is staged through LDS in tiles of MEAN_TILE_PIX pixels (48 KiB; all of
// a 128 x 128 image) with 16-byte loads when the row is 16-byte aligned (`vec`), so that the strided pixel order of the
// float32 kernel costs LDS reads, not 3-byte global reads; the rescale is a 256-entry table in LDS that the block fills
// with one division per thread.  MEAN_TILE_PIX is a multiple of 256: a thread meets its pixels in ascending order across tiles.
constexpr int MEAN_TILE_PIX = 16384;
__global__ __launch_bounds__(256) void chan_mean3_u8_kernel(U8Gather src, float* __restrict__ means, int HW, int vec) {
  __shared__ __attribute__((aligned(16))) unsigned char tile[MEAN_TILE_PIX * 3];
  __shared__ float lut[256];
  lut[threadIdx.x] = rescale_u8(threadIdx.x);
  const unsigned char* p = src.row(blockIdx.x);
  float s[3] = {0.f, 0.f, 0.f};
  for (int t0 = 0; t0 < HW; t0 += MEAN_TILE_PIX) {
    const int npix = HW - t0 < MEAN_TILE_PIX ? HW - t0 : MEAN_TILE_PIX, nb = npix * 3;
    const unsigned char* q = p + (long long)t0 * 3;
    const int nvec = vec ? nb / 16 : 0;   // t0 * 3 is a multiple of 16, so an aligned row has aligned tiles
    for (int i = threadIdx.x; i < nvec; i += 256)
      reinterpret_cast<u32x4*>(tile)[i] = reinterpret_cast<const u32x4*>(q)[i];
    for (int i = nvec * 16 + threadIdx.x; i < nb; i += 256) tile[i] = q[i];
    __syncthreads();   // the tile (and, the first time round, the table) is complete
    for (int i = threadIdx.x; i < npix; i += 256) {
      s[0] += lut[tile[i * 3]]; s[1] += lut[tile[i * 3 + 1]]; s[2] += lut[tile[i * 3 + 2]];
    }
    __syncthreads();   // every thread is done with the tile before it is overwritten
  }
  chan_mean3_finish(s, means, HW);
}

// hue rotation by dh (fraction of a turn) that keeps the pixel's min and max channel values
__device__ __forceinline__ void hue_rotate(float& r, float& g, float& b, float dh) {
  const float vmax = fmaxf(r, fmaxf(g, b)), vmin = fminf(r, fminf(g, b)), range = vmax - vmin;
  if (!(range > 0.f)) return;  // grey: hue undefined, unchanged
  float h;  // hue in sixths of a turn, [0, 6)
  if (r == vmax) h = (g - b) / range;
  else if (g == vmax) h = 2.f + (b - r) / range;
  else h = 4.f + (r - g) / range;
  h += 6.f * dh;
  h -= 6.f * floorf(h * (1.f / 6.f));
  if (h >= 6.f) h = 0.f;
  const int sect = (int)h;
  const float f = h - (float)sect;
  const float up = vmin + range * f, dn = vmax - range * f;  // rising / falling edge inside the sector
  switch (sect) {
    case 0: r = vmax; g = up; b = vmin; break;
    case 1: r = dn; g = vmax; b = vmin; break;
    case 2: r = vmin; g = vmax; b = up; break;
    case 3: r = vmin; g = dn; b = vmax; break;
    case 4: r = up; g = vmin; b = vmax; break;
    default: r = vmax; g = vmin; b = dn; break;
  }
}

// ---- the transform ---------------------------------------------------------------------------------------------------
// A thread owns G consecutive SOURCE pixels sx0 .. sx0 + G - 1 of one image row (W % G == 0) and writes them where the
// flip sends them: output pixel x = W - 1 - sx of the same row when the image is flipped, x = sx otherwise; a flip is its
// own inverse, so every output pixel is written once.  The noise of a pixel is keyed by its OUTPUT index (offset + i),
// whichever thread produces it.  With G == 4 the group's 12 floats leave as three 16-byte stores (a flipped group is a
// contiguous group again, in reverse pixel order): the caller guarantees 16-byte aligned outputs.
// out_plain (may be null): the untransformed source pixels as float32, at their source position — for a uint8 source
// that is the rescaled image, produced from the one read of the bytes.
template <int G, class Src>
__global__ __launch_bounds__(256) void augment_kernel(Src src, float* __restrict__ out, float* __restrict__ out_plain,
                                                      const float* __restrict__ means, const unsigned char* __restrict__ flip,
                                                      int B, int H, int W, float db, float cf, float dh, float nscale,
                                                      unsigned long long seed, unsigned long long offset,
                                                      const float* __restrict__ dparams) {
  if (dparams) { db = dparams[0]; cf = dparams[1]; dh = dparams[2]; }  // draws made on the device (draws_kernel)
  const int WG = W / G;
  const long long ngrp = (long long)B * H * WG, stride = (long long)gridDim.x * blockDim.x;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < ngrp; g += stride) {
    const int sx0 = (int)(g % WG) * G;
    const long long row = g / WG;
    const int n = (int)(row / H), y = (int)(row % H);
    const bool fl = flip && flip[n];
    float p[G][3], c[G][3];
    src.template load<G>(n, y * W + sx0, p);
    float m[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) m[k] = means[n * 3 + k] + db;  // the mean is taken after the brightness shift (flips do not move it)
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int sx = sx0 + j, x = fl ? W - 1 - sx : sx;
      const long long i = row * W + x;   // output pixel
#pragma unroll
      for (int k = 0; k < 3; ++k) c[j][k] = ((p[j][k] + db) - m[k]) * cf + m[k];
      if (dh != 0.f) hue_rotate(c[j][0], c[j][1], c[j][2], dh);
      if (nscale != 0.f) {
        float z[4];
        normal4(seed, offset + (unsigned long long)i, z);
        c[j][0] += nscale * z[0]; c[j][1] += nscale * z[1]; c[j][2] += nscale * z[2];
      }
    }
    if constexpr (G == 4) {
      const int x0 = fl ? W - 4 - sx0 : sx0;
      float q[12];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        q[j * 3] = fl ? c[3 - j][0] : c[j][0]; q[j * 3 + 1] = fl ? c[3 - j][1] : c[j][1]; q[j * 3 + 2] = fl ? c[3 - j][2] : c[j][2];
      }
      f32x4* o = reinterpret_cast<f32x4*>(out + (row * W + x0) * 3);
      o[0] = f32x4{q[0], q[1], q[2], q[3]}; o[1] = f32x4{q[4], q[5], q[6], q[7]}; o[2] = f32x4{q[8], q[9], q[10], q[11]};
      if (out_plain) {
        f32x4* r = reinterpret_cast<f32x4*>(out_plain + (row * W + sx0) * 3);
        r[0] = f32x4{p[0][0], p[0][1], p[0][2], p[1][0]}; r[1] = f32x4{p[1][1], p[1][2], p[2][0], p[2][1]};
        r[2] = f32x4{p[2][2], p[3][0], p[3][1], p[3][2]};
      }
    } else {
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int sx = sx0 + j, x = fl ? W - 1 - sx : sx;
        float* o = out + (row * W + x) * 3;
        o[0] = c[j][0]; o[1] = c[j][1]; o[2] = c[j][2];
        if (out_plain) {
          float* r = out_plain + (row * W + sx) * 3;
          r[0] = p[j][0]; r[1] = p[j][1]; r[2] = p[j][2];
        }
      }
    }
  }
}

// The scalar draws of the TF ops (eager_trainer.py:127-130: one brightness delta, one contrast factor, one hue delta per
// batch; one coin per image for the flip) from the Philox window at `offset`: word w of the window is 24-bit uniform
// u_w = (bits >> 8) / 2^24;  u_0 -> brightness, u_1 -> contrast, u_2 -> hue, u_{3+n} -> flip of image n.
// params[0..2] = {db, cf, dh}; flip[n] = u_{3+n} < 0.5.  No host round trip: the step has no sync on its input side.
__global__ __launch_bounds__(256) void draws_kernel(float* __restrict__ params, unsigned char* __restrict__ flip, int B,
                                                    float db_max, float c_lo, float c_hi, float dh_max,
                                                    unsigned long long seed, unsigned long long offset) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;  // word index of the window
  if (w >= B + 3) return;
  const unsigned long long c = offset + (unsigned long long)(w >> 2);
  const u4 r = philox4x32_10(u4{(unsigned)c, (unsigned)(c >> 32), 0u, 0u}, (unsigned)seed, (unsigned)(seed >> 32));
  const unsigned bits = (w & 3) == 0 ? r.x : (w & 3) == 1 ? r.y : (w & 3) == 2 ? r.z : r.w;
  const float u = (float)(bits >> 8) * (1.0f / 16777216.0f);
  if (w == 0) params[0] = (2.0f * u - 1.0f) * db_max;
  else if (w == 1) params[1] = c_lo + u * (c_hi - c_lo);
  else if (w == 2) params[2] = (2.0f * u - 1.0f) * dh_max;
  else flip[w - 3] = u < 0.5f ? 1 : 0;
}

inline int grid_for(long long n) {
  long long b = (n + 255) / 256;
  return (int)(b < 4096 ? (b > 0 ? b : 1) : 4096);
}

// workspace of the drawn variants: means [B][3] f32 | params {db, cf, dh, -} f32 | flip [B] bytes, each 16-byte aligned
inline size_t drawn_workspace_bytes(int B) {
  return ((size_t)B * 3 * sizeof(float) + 15) / 16 * 16 + 16 + ((size_t)B + 15) / 16 * 16;
}

}  // namespace
