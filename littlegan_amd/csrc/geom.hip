// Geometric augmentation of the Discriminator's inputs (geom_augment; Karras et al. 2020, "Training GANs with limited
// data": the pixel-blitting and geometric group; the reference has none).  Every image D reads in the training step is resampled under a
// per-sample affine map, and the generator-side tapes are differentiated through it.  Per sample, x[S][S][3] fp32 NHWC and a record of
// 4 fp32 words {a, b, c, d}: the matrix M of the map from a DESTINATION pixel to its SOURCE position about the image centre.  With
// h = (S - 1) / 2, u = y - h, v = x - h:
//   sy = (a u + b v) + h      sx = (c u + d v) + h      y0 = floor(sy), x0 = floor(sx)
//   out_k(y, x) = sum over (i, j) in {y0, y0+1} x {x0, x0+1}, in that order, of  tent(sy - i) tent(sx - j) x_k(i, j)
//   tent(t) = 1 - |t| for |t| < 1, else 0;  a tap outside the image, or of weight exactly 0, contributes nothing and is not read
// in fp32, in exactly this order of operations (-ffp-contract=off).  S is even, so h is a half-integer: with entries in {0, +-1} every
// coordinate is an exact integer, one tap has weight 1 and the output is a permutation of the input bit for bit.
// The adjoint is a GATHER (no float atomics: eager and replayed steps agree bit for bit): the thread of a source pixel inverts M in fp32,
// walks the box of the destinations that can touch it in ascending (y, x) and recomputes (sy, sx) and the weight of its own pixel by the
// expressions of the forward — tent(sy - i) in both, never 1 - f in one and f in the other — so the weights agree bit for bit.  The box is
// only a superset: its slack covers the rounding of the inverse, and where that cannot be bounded it is the whole image.
// A record with a non-finite entry, or whose fp32 determinant is not finite or below 2^-20 in magnitude, gives zeros.  Coordinates are
// compared as floats before any conversion to an integer, so no record bits lead an access out of the images.
// The draws (lgeo_draw) are per row, on the device, from the step's diff_augment key: the Philox block of the row with third counter word
// 2 (gates: 3), M = R(theta) Q^k F / s in fp64, rounded once.  One launch per pass, no workspace, no LDS; the element-wise passes walk
// the batch in whole rounds of the CU budget, as diffaug.hip's.
#include "lg_internal.h"
#include "../../include/littlegan_geom.h"
#include "diffaug_draw.h"

namespace {

struct Geo { float a, b, c, d; bool ok, ident; };

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN

__device__ __forceinline__ Geo load_geo(const float* __restrict__ geo, int n) {
  const f32x4 m = reinterpret_cast<const f32x4*>(geo)[n];
  const float det = m[0] * m[3] - m[1] * m[2];
  const bool ok = finite_f(m[0]) && finite_f(m[1]) && finite_f(m[2]) && finite_f(m[3]) && finite_f(det) && fabsf(det) >= 0x1p-20f;
  return Geo{m[0], m[1], m[2], m[3], ok, m[0] == 1.f && m[1] == 0.f && m[2] == 0.f && m[3] == 1.f};
}

__device__ __forceinline__ float tent(float t) { return fabsf(t) < 1.f ? 1.f - fabsf(t) : 0.f; }

// source position of the destination pixel (y, x): the one expression both passes use
__device__ __forceinline__ void src_pos(const Geo& r, float h, int y, int x, float& sy, float& sx) {
  const float u = (float)y - h, v = (float)x - h;
  sy = (r.a * u + r.b * v) + h;
  sx = (r.c * u + r.d * v) + h;
}

// geo[i] = the record of row r0 + i of call slot `call`; state == null: ungated
__global__ __launch_bounds__(256) void geom_draw_kernel(const unsigned long long* __restrict__ key, int call, int r0, int rows, int policy,
                                                        const float* __restrict__ state, float* __restrict__ geo) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  const unsigned long long seed = key[0], ctr = diffaug_row_ctr(key[1], call, r0 + i);
  const u4 V = philox4x32_10(u4{(unsigned)ctr, (unsigned)(ctr >> 32), 2u, 0u}, (unsigned)seed, (unsigned)(seed >> 32));
  int on = policy;
  if (state) {   // the rule of lgx_diffaug_draw_gated (ada.hip), on a block of its own
    const u4 G = philox4x32_10(u4{(unsigned)ctr, (unsigned)(ctr >> 32), 3u, 0u}, (unsigned)seed, (unsigned)(seed >> 32));
    const unsigned t = (unsigned)(fminf(fmaxf(state[0], 0.f), 1.f) * 16777216.0f);
    on &= ((G.x >> 8) < t ? 1 : 0) | ((G.y >> 8) < t ? 2 : 0) | ((G.z >> 8) < t ? 4 : 0) | ((G.w >> 8) < t ? 8 : 0);
  }
  const bool flip = (on & 1) && (V.x >> 8) < (1u << 23);
  const int k = (on & 2) ? (int)((V.y >> 8) >> 22) : 0;
  const double k24 = 1.0 / 16777216.0;
  // an identity is selected, not computed: the record of a row without scale / rotate holds exact 0 / +-1
  const double s = (on & 4) ? exp2((double)(V.z >> 8) * k24 - 0.5) : 1.0;
  double cs = 1.0, sn = 0.0;
  if (on & 8) {
    const double th = 6.283185307179586476925 * ((double)(V.w >> 8) * k24 - 0.5);
    cs = cos(th); sn = sin(th);
  }
  // P = Q^k F, entries 0 / +-1: Q^k = [[qc, -qs], [qs, qc]], F negates the second column
  const double qc = (k == 0) ? 1.0 : (k == 2) ? -1.0 : 0.0, qs = (k == 1) ? 1.0 : (k == 3) ? -1.0 : 0.0, f = flip ? -1.0 : 1.0;
  const double p00 = qc, p01 = -qs * f, p10 = qs, p11 = qc * f;
  // M = R P / s; + 0.f: no record holds a negative zero
  f32x4 m;
  m[0] = (float)((cs * p00 + -sn * p10) / s) + 0.f;
  m[1] = (float)((cs * p01 + -sn * p11) / s) + 0.f;
  m[2] = (float)((sn * p00 + cs * p10) / s) + 0.f;
  m[3] = (float)((sn * p01 + cs * p11) / s) + 0.f;
  reinterpret_cast<f32x4*>(geo)[i] = m;
}

// A thread owns the destination pixels x0 .. x0+3 of one image row: up to 4 taps per pixel as 12-byte loads, three aligned 16-byte stores.
__global__ __launch_bounds__(256) void geom_fwd_kernel(const float* __restrict__ xin, const float* __restrict__ geo, float* __restrict__ out,
                                                       int rows, int S) {
  const int WG = S / 4, per = S * WG;
  const long long ngrp = (long long)rows * per, stride = (long long)gridDim.x * blockDim.x;
  const float h = (float)(S - 1) * 0.5f, fS = (float)S;
  for (long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x; gi < ngrp; gi += stride) {
    const int n = (int)(gi / per), rem = (int)(gi % per), y = rem / WG, x0 = (rem % WG) * 4;
    const Geo r = load_geo(geo, n);
    const float* src = xin + (long long)n * S * S * 3;
    f32x4* dst = reinterpret_cast<f32x4*>(out + (((long long)n * S + y) * S + x0) * 3);
    if (r.ident) {   // the copy path: the general one gives the same bits
      const f32x4* s4 = reinterpret_cast<const f32x4*>(src + ((long long)y * S + x0) * 3);
      const f32x4 q0 = s4[0], q1 = s4[1], q2 = s4[2];
      dst[0] = q0; dst[1] = q1; dst[2] = q2;
      continue;
    }
    float o[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float e0 = 0.f, e1 = 0.f, e2 = 0.f, sy, sx;
      src_pos(r, h, y, x0 + j, sy, sx);
      // compared as floats (NaN fails): only then is floor(s) in [-1, S-1] and the conversion defined
      if (r.ok && sy > -1.f && sy < fS && sx > -1.f && sx < fS) {
        const float fy = floorf(sy), fx = floorf(sx);
        const int iy = (int)fy, ix = (int)fx;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int ti = iy + (t >> 1), tj = ix + (t & 1);
          const float w = tent(sy - (float)ti) * tent(sx - (float)tj);
          if (w != 0.f && (unsigned)ti < (unsigned)S && (unsigned)tj < (unsigned)S) {
            const float* p = src + ((long long)ti * S + tj) * 3;
            e0 += w * p[0]; e1 += w * p[1]; e2 += w * p[2];
          }
        }
      }
      o[3 * j] = e0; o[3 * j + 1] = e1; o[3 * j + 2] = e2;
    }
    dst[0] = f32x4{o[0], o[1], o[2], o[3]}; dst[1] = f32x4{o[4], o[5], o[6], o[7]}; dst[2] = f32x4{o[8], o[9], o[10], o[11]};
  }
}

// lower / upper end of a clipped integer range from float bounds; a NaN bound gives the whole range
__device__ __forceinline__ int box_lo(float lo, int S) { return lo >= 0.f ? (lo <= (float)S ? (int)ceilf(lo) : S) : 0; }
__device__ __forceinline__ int box_hi(float hi, int S) { return hi <= (float)(S - 1) ? (hi >= -1.f ? (int)floorf(hi) : -1) : S - 1; }

// A thread owns the SOURCE pixels j0 .. j0+3 of image row i and gathers, over the union of their boxes in ascending (y, x), w g(y, x).
__global__ __launch_bounds__(256) void geom_bwd_kernel(const float* __restrict__ gin, const float* __restrict__ geo, float* __restrict__ gx,
                                                       int rows, int S) {
  const int WG = S / 4, per = S * WG;
  const long long ngrp = (long long)rows * per, stride = (long long)gridDim.x * blockDim.x;
  const float h = (float)(S - 1) * 0.5f, fS = (float)S;
  for (long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x; gi < ngrp; gi += stride) {
    const int n = (int)(gi / per), rem = (int)(gi % per), i = rem / WG, j0 = (rem % WG) * 4;
    const Geo r = load_geo(geo, n);
    const float* src = gin + (long long)n * S * S * 3;
    f32x4* dst = reinterpret_cast<f32x4*>(gx + (((long long)n * S + i) * S + j0) * 3);
    if (r.ident) {
      const f32x4* s4 = reinterpret_cast<const f32x4*>(src + ((long long)i * S + j0) * 3);
      const f32x4 q0 = s4[0], q1 = s4[1], q2 = s4[2];
      dst[0] = q0; dst[1] = q1; dst[2] = q2;
      continue;
    }
    float o[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) o[q] = 0.f;
    if (r.ok) {
      // M^-1 = adj(M) / det.  e bounds the relative error of det (cancellation of a d against b c) and through it of the inverse; the
      // centres carry at most (e + 2^-21) rowsum S of it, which the half sides take on beside the slack 0.01.  Beyond e = 1/8 (or NaN
      // anywhere): the whole image.  The box only has to contain the destinations that touch the pixels; the weights decide.
      const float ad = r.a * r.d, bc = r.b * r.c, det = ad - bc;
      const float e = 0x1p-22f * ((fabsf(ad) + fabsf(bc)) / fabsf(det));
      const float ia = r.d / det, ib = -r.b / det, ic = -r.c / det, id = r.a / det;
      const float ui = (float)i - h, v0 = (float)j0 - h, v1 = (float)(j0 + 3) - h;
      const float ry = fabsf(ia) + fabsf(ib), rx = fabsf(ic) + fabsf(id);
      const float hy = ry + ((e + 0x1p-21f) * ry * fS + 0.01f), hx = rx + ((e + 0x1p-21f) * rx * fS + 0.01f);
      const float cy0 = (ia * ui + ib * v0) + h, cy1 = (ia * ui + ib * v1) + h;
      const float cx0 = (ic * ui + id * v0) + h, cx1 = (ic * ui + id * v1) + h;
      int ylo = box_lo(fminf(cy0, cy1) - hy, S), yhi = box_hi(fmaxf(cy0, cy1) + hy, S);
      int xlo = box_lo(fminf(cx0, cx1) - hx, S), xhi = box_hi(fmaxf(cx0, cx1) + hx, S);
      if (!(e <= 0.125f) || !finite_f(hy) || !finite_f(hx) || !finite_f(cy0) || !finite_f(cy1) || !finite_f(cx0) || !finite_f(cx1)) {
        ylo = 0; yhi = S - 1; xlo = 0; xhi = S - 1;
      }
      for (int y = ylo; y <= yhi; ++y) {
        for (int x = xlo; x <= xhi; ++x) {
          float sy, sx;
          src_pos(r, h, y, x, sy, sx);
          const float wy = tent(sy - (float)i);
          if (!(wy != 0.f)) continue;   // (a NaN weight cannot arise from a usable record's finite coordinates; an infinite one fails tent)
          float w[4];
          bool any = false;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            w[q] = wy * tent(sx - (float)(j0 + q));
            any = any || w[q] != 0.f;
          }
          if (!any) continue;
          const float* p = src + ((long long)y * S + x) * 3;
          const float g0 = p[0], g1 = p[1], g2 = p[2];
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (w[q] != 0.f) { o[3 * q] += w[q] * g0; o[3 * q + 1] += w[q] * g1; o[3 * q + 2] += w[q] * g2; }
        }
      }
    }
    dst[0] = f32x4{o[0], o[1], o[2], o[3]}; dst[1] = f32x4{o[4], o[5], o[6], o[7]}; dst[2] = f32x4{o[8], o[9], o[10], o[11]};
  }
}

// blocks of an element-wise pass: one 4-pixel group per thread up to what the CU budget holds at once, beyond that whole rounds of it
// (the kernel's own residency: occupancy query, once per kernel, as diffaug.hip sizes its pass)
template <bool BWD>
inline int geom_blocks(long long ngrp) {
  static int per_cu = 0;
  if (!per_cu && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, BWD ? geom_bwd_kernel : geom_fwd_kernel, 256, 0) != hipSuccess ||
                  per_cu < 1))
    per_cu = 8;
  const long long resident = (long long)per_cu * lg_grid_cus();
  long long nb = (ngrp + 255) / 256;
  if (nb > resident) nb = nb / resident * resident;
  if (nb > 4 * resident) nb = 4 * resident;
  return (int)(nb < 1 ? 1 : nb);
}

int check_map(const char* who, const float* v, const float* geo, float* out, int rows, int S) {
  LG_CHECK_ARG(v && geo && out, "%s: null pointer", who);
  LG_CHECK_ARG(v != out, "%s: in-place call", who);
  LG_CHECK_ARG(rows > 0 && rows <= (1 << 20), "%s: bad row count %d", who, rows);
  LG_CHECK_ARG(S >= 8 && S % 8 == 0 && S <= 1024, "%s: image side %d must be a multiple of 8, at least 8", who, S);
  LG_CHECK_ARG((((uintptr_t)v | (uintptr_t)geo | (uintptr_t)out) & 15) == 0, "%s: images and records must be 16-byte aligned", who);
  return LG_OK;
}

}  // namespace

extern "C" int lgeo_draw(const long long* key, int call, int r0, int rows, int S, int policy_bits, const float* state, float* geo,
                         void* stream) {
  LG_CHECK_ARG(key && geo, "lgeo_draw: null pointer");
  LG_CHECK_ARG(((uintptr_t)key & 7) == 0 && (((uintptr_t)state | (uintptr_t)geo) & 15) == 0,
               "lgeo_draw: key must be 8-byte, state and geo 16-byte aligned");
  LG_CHECK_ARG(call >= 0 && call <= 3, "lgeo_draw: call slot %d outside 0..3", call);
  LG_CHECK_ARG(rows > 0 && rows <= (1 << 20) && r0 >= 0 && (long long)r0 + rows <= (1LL << 24),
               "lgeo_draw: rows %d .. %d + %d outside a call slot's 2^24 (at most 2^20 a call)", r0, r0, rows);
  LG_CHECK_ARG(S >= 8 && S % 8 == 0 && S <= 1024, "lgeo_draw: image side %d must be a multiple of 8, at least 8", S);
  LG_CHECK_ARG(policy_bits >= 0 && policy_bits <= 15, "lgeo_draw: policy bits %d outside 0..15 (1 xflip, 2 rot90, 4 scale, 8 rotate)",
               policy_bits);
  hipLaunchKernelGGL(geom_draw_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long*>(key), call, r0, rows, policy_bits, state, geo);
  LG_CHECK_LAUNCH("lgeo_draw");
  return LG_OK;
}

extern "C" int lgeo_fwd(const float* x, const float* geo, float* out, int rows, int S, void* stream) {
  if (int rc = check_map("lgeo_fwd", x, geo, out, rows, S)) return rc;
  const long long ngrp = (long long)rows * S * (S / 4);
  hipLaunchKernelGGL(geom_fwd_kernel, dim3(geom_blocks<false>(ngrp)), dim3(256), 0, (hipStream_t)stream, x, geo, out, rows, S);
  LG_CHECK_LAUNCH("lgeo_fwd");
  return LG_OK;
}

extern "C" int lgeo_bwd(const float* g, const float* geo, float* gx, int rows, int S, void* stream) {
  if (int rc = check_map("lgeo_bwd", g, geo, gx, rows, S)) return rc;
  const long long ngrp = (long long)rows * S * (S / 4);
  hipLaunchKernelGGL(geom_bwd_kernel, dim3(geom_blocks<true>(ngrp)), dim3(256), 0, (hipStream_t)stream, g, geo, gx, rows, S);
  LG_CHECK_LAUNCH("lgeo_bwd");
  return LG_OK;
}
