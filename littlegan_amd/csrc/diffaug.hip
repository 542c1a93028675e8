// Differentiable augmentation of the Discriminator's inputs (diff_augment; Zhao et al. 2020, "DiffAugment"; the reference has
// only the non-differentiable augmentation of the first real batch, augment.hip).  Every image D sees in the training step goes through a
// random map T, and the generator-side tapes are differentiated through it.  Per sample, x[S][S][3] fp32 NHWC and a record of 8 fp32 words
// {b, s, c, ty, tx, cy, cx, cut} (the last five small integers, stored exactly):
//   1 brightness  u = x + b                                  2 saturation  v = (u - mean_k u) s + mean_k u     (mean over the pixel's 3 channels)
//   3 contrast    w = (v - mean v) c + mean v (whole sample)  4 translation t(y,x) = w(y+ty, x+tx) inside the image, else 0
//   5 cutout      out = 0 on the cut x cut square at rows cy - cut/2 .., columns cx - cut/2 .. (clipped to the image), else t
// All five are affine in x, so T has the closed form the kernels evaluate.  With xv = x(y+ty, x+tx), m = mean of x over the sample,
// K = keep(y,x) inside(y+ty, x+tx):
//   out_k = K ( c s xv_k + c (1-s) mean_k(xv) + (1-c) m + b )
// and its exact adjoint, with h = K g moved back to the source position, h'(y',x') = h(y'-ty, x'-tx) (0 outside):
//   gx_k(y',x') = c s h'_k + c (1-s) mean_k(h') + (1-c) / (3 S^2) sum_sample h
// The identity record {0, 1, 1, 0, 0, 0, 0, 0} returns x and g bit for bit: every cross term is an exact zero (the library is built with
// -ffp-contract=off) and K is a selection, not a product.
// Each of T and its adjoint is two launches: per-sample sums (of x; of K g) as fp32 per-thread sums merged in fp64, one record per
// (sample, chunk of SUM_PIX pixels), in a fixed order — no float atomics, so eager and replayed steps agree bit for bit and a row range of a
// batch gives the bits of the whole; then one element-wise pass whose thread owns 4 consecutive DESTINATION pixels (three aligned 16-byte
// stores; a horizontal shift breaks the alignment of the source only) and walks the batch in a grid of whole rounds of the CU budget, not
// one workgroup per sample: 2 rows or 512, the pass fills the chip.
// The draws (lg_diffaug_draw) are per row of a call's batch, on the device: row r of call slot q reads Philox blocks
// key_offset + ((q << 24) + r) 2 + {0, 1} under the step's key {seed, key_offset} (device memory, like the dropout key); the policy acts
// there alone — a component that is not named gets its identity values, and the passes below know no policy.
#include "lg_internal.h"
#include "diffaug_draw.h"

namespace {

constexpr int SUM_PIX = 4096;   // pixels per sum record: S = 128 gives 4 records per sample, S <= 64 one

struct Rec { float b, s, c; int ty, tx, y0, x0, cut; };   // y0, x0: first row / column of the cutout square (may be negative)

__device__ __forceinline__ Rec load_rec(const float* __restrict__ params, int n) {
  const f32x4 p0 = reinterpret_cast<const f32x4*>(params)[2 * n], p1 = reinterpret_cast<const f32x4*>(params)[2 * n + 1];
  const int cut = (int)p1[3];
  return Rec{p0[0], p0[1], p0[2], (int)p0[3], (int)p1[0], (int)p1[1] - cut / 2, (int)p1[2] - cut / 2, cut};
}
__device__ __forceinline__ bool kept(const Rec& r, int y, int x) {
  return !(y >= r.y0 && y < r.y0 + r.cut && x >= r.x0 && x < r.x0 + r.cut);
}
__device__ __forceinline__ bool inside(int y, int x, int S) { return (unsigned)y < (unsigned)S && (unsigned)x < (unsigned)S; }

// params[i] = the record of row r0 + i of call slot `call` (diffaug_record, diffaug_draw.h)
__global__ __launch_bounds__(256) void diffaug_draw_kernel(const unsigned long long* __restrict__ key, int call, int r0, int rows, int S,
                                                           int policy, float* __restrict__ params) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  f32x4 p0, p1;
  diffaug_record(key[0], diffaug_row_ctr(key[1], call, r0 + i), S, policy, p0, p1);
  reinterpret_cast<f32x4*>(params)[2 * i] = p0;
  reinterpret_cast<f32x4*>(params)[2 * i + 1] = p1;
}

// part[n][p] = sum over the pixels [p SUM_PIX, (p+1) SUM_PIX) of sample n of all 3 channels of v (MASKED: of K v, K = keep(y,x) inside(y+ty, x+tx)).
// Block n * nparts + p; thread t adds the 4-pixel groups t, t + 256, ... of the chunk in that order into one fp32 sum, the 256 sums merge in fp64.
template <bool MASKED>
__global__ __launch_bounds__(256) void diffaug_sum_kernel(const float* __restrict__ v, const float* __restrict__ params,
                                                          double* __restrict__ part, int nparts, int S) {
  __shared__ double sred[16];
  const int n = blockIdx.x / nparts, p = blockIdx.x % nparts, HW = S * S;
  const int g0 = p * (SUM_PIX / 4), g1 = (HW / 4 < g0 + SUM_PIX / 4) ? HW / 4 : g0 + SUM_PIX / 4;
  const f32x4* q = reinterpret_cast<const f32x4*>(v + (long long)n * HW * 3);
  Rec r{};
  if (MASKED) r = load_rec(params, n);
  float s = 0.f;
  for (int g = g0 + (int)threadIdx.x; g < g1; g += 256) {
    const f32x4 a = q[3 * g], b = q[3 * g + 1], c = q[3 * g + 2];
    const float e[12] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], c[0], c[1], c[2], c[3]};
    const int y = (g * 4) / S, x0 = (g * 4) % S;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool K = !MASKED || (kept(r, y, x0 + j) && inside(y + r.ty, x0 + j + r.tx, S));
      s += K ? (e[3 * j] + e[3 * j + 1]) + e[3 * j + 2] : 0.f;
    }
  }
  double d[1] = {(double)s};
  lg_block_sum_d<1>(d, sred);
  if (threadIdx.x == 0) part[blockIdx.x] = d[0];
}

// The element-wise pass of T (BWD = false) and of its adjoint (BWD = true).  A thread owns the destination pixels x0 .. x0+3 of one image row
// and gathers each from (y + dy, x + dx), (dy, dx) = (ty, tx) forward, (-ty, -tx) backward; the cutout is looked up at the destination
// (forward: out = K ...) or at the gathered position (backward: h = K g lives where g does).  t = (float)(sum of the sample / (3 S^2)):
//   forward   out_k = K (((c s) xv_k + (c (1-s)) mean_k(xv)) + (1-c) t) + b)        backward  gx_k = ((c s) h'_k + (c (1-s)) mean_k(h')) + (1-c) t
template <bool BWD>
__global__ __launch_bounds__(256) void diffaug_apply_kernel(const float* __restrict__ v, const float* __restrict__ params,
                                                            const double* __restrict__ part, int nparts, float* __restrict__ out,
                                                            int rows, int S) {
  const int WG = S / 4, per = S * WG;
  const long long ngrp = (long long)rows * per, stride = (long long)gridDim.x * blockDim.x;
  const double inv_n = 1.0 / (3.0 * (double)S * (double)S);
  for (long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x; gi < ngrp; gi += stride) {
    const int n = (int)(gi / per), rem = (int)(gi % per), y = rem / WG, x0 = (rem % WG) * 4;
    const Rec r = load_rec(params, n);
    double tot = 0.0;
    for (int p = 0; p < nparts; ++p) tot += part[(long long)n * nparts + p];
    const float t = (float)(tot * inv_n);
    const float a1 = r.c * r.s, a2 = r.c * (1.0f - r.s), a3 = (1.0f - r.c) * t;
    const int sy = BWD ? y - r.ty : y + r.ty, dx = BWD ? -r.tx : r.tx;
    const float* src = v + ((long long)n * S + sy) * S * 3;
    float o[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x0 + j, sx = x + dx;
      const bool K = inside(sy, sx, S) && (BWD ? kept(r, sy, sx) : kept(r, y, x));
      float e0 = 0.f, e1 = 0.f, e2 = 0.f;
      if (K) { e0 = src[sx * 3]; e1 = src[sx * 3 + 1]; e2 = src[sx * 3 + 2]; }
      const float mk = a2 * (((e0 + e1) + e2) * (1.0f / 3.0f));
      if (BWD) {
        o[3 * j] = (a1 * e0 + mk) + a3; o[3 * j + 1] = (a1 * e1 + mk) + a3; o[3 * j + 2] = (a1 * e2 + mk) + a3;
      } else {
        o[3 * j] = K ? ((a1 * e0 + mk) + a3) + r.b : 0.f;
        o[3 * j + 1] = K ? ((a1 * e1 + mk) + a3) + r.b : 0.f;
        o[3 * j + 2] = K ? ((a1 * e2 + mk) + a3) + r.b : 0.f;
      }
    }
    f32x4* dst = reinterpret_cast<f32x4*>(out + (((long long)n * S + y) * S + x0) * 3);
    dst[0] = f32x4{o[0], o[1], o[2], o[3]}; dst[1] = f32x4{o[4], o[5], o[6], o[7]}; dst[2] = f32x4{o[8], o[9], o[10], o[11]};
  }
}

inline int sum_parts(int S) { return (S * S + SUM_PIX - 1) / SUM_PIX; }

// blocks of the element-wise pass: one 4-pixel group per thread up to what the CU budget holds at once, beyond that whole rounds of it
// (the kernel's own residency: occupancy query, once per kernel, as norm.hip sizes its element-wise grids)
template <bool BWD>
inline int apply_blocks(long long ngrp) {
  static int per_cu = 0;
  if (!per_cu && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, diffaug_apply_kernel<BWD>, 256, 0) != hipSuccess || per_cu < 1))
    per_cu = 8;
  const long long resident = (long long)per_cu * lg_grid_cus();
  long long nb = (ngrp + 255) / 256;
  if (nb > resident) nb = nb / resident * resident;
  if (nb > 4 * resident) nb = 4 * resident;
  return (int)(nb < 1 ? 1 : nb);
}

int check_map(const char* who, const float* v, const float* params, float* out, int rows, int S, void* workspace, size_t ws_bytes) {
  LG_CHECK_ARG(v && params && out && workspace, "%s: null pointer", who);
  LG_CHECK_ARG(v != out, "%s: in-place call", who);
  LG_CHECK_ARG(rows > 0 && rows <= (1 << 20), "%s: bad row count %d", who, rows);
  LG_CHECK_ARG(S >= 8 && S % 8 == 0 && S <= 1024, "%s: image side %d must be a multiple of 8, at least 8", who, S);
  LG_CHECK_ARG((((uintptr_t)v | (uintptr_t)params | (uintptr_t)out) & 15) == 0 && ((uintptr_t)workspace & 7) == 0,
               "%s: images and records must be 16-byte aligned, the workspace 8-byte aligned", who);
  LG_CHECK_ARG(ws_bytes >= lg_diffaug_workspace_bytes(rows, S), "%s: workspace too small", who);
  return LG_OK;
}

template <bool BWD>
int run_map(const char* who, const float* v, const float* params, float* out, int rows, int S, void* workspace, hipStream_t st) {
  double* part = (double*)workspace;
  const int np = sum_parts(S);
  hipLaunchKernelGGL(diffaug_sum_kernel<BWD>, dim3(np * rows), dim3(256), 0, st, v, params, part, np, S);
  LG_CHECK_LAUNCH(who);
  const long long ngrp = (long long)rows * S * (S / 4);
  hipLaunchKernelGGL(diffaug_apply_kernel<BWD>, dim3(apply_blocks<BWD>(ngrp)), dim3(256), 0, st, v, params,
                     (const double*)part, np, out, rows, S);
  LG_CHECK_LAUNCH(who);
  return LG_OK;
}

}  // namespace

extern "C" size_t lg_diffaug_workspace_bytes(int rows, int S) {
  if (rows <= 0 || S <= 0) return 0;
  return (size_t)rows * sum_parts(S) * sizeof(double);
}

extern "C" int lg_diffaug_draw(const long long* key, int call, int r0, int rows, int S, int policy_bits, float* params, void* stream) {
  LG_CHECK_ARG(key && params, "lg_diffaug_draw: null pointer");
  LG_CHECK_ARG(((uintptr_t)key & 7) == 0 && ((uintptr_t)params & 15) == 0, "lg_diffaug_draw: key must be 8-byte, params 16-byte aligned");
  LG_CHECK_ARG(call >= 0 && call <= 3, "lg_diffaug_draw: call slot %d outside 0..3", call);
  LG_CHECK_ARG(rows > 0 && r0 >= 0 && (long long)r0 + rows <= (1LL << 24), "lg_diffaug_draw: rows %d .. %d + %d outside a call slot's 2^24", r0,
               r0, rows);
  LG_CHECK_ARG(S >= 8 && S % 8 == 0 && S <= 1024, "lg_diffaug_draw: image side %d must be a multiple of 8, at least 8", S);
  LG_CHECK_ARG(policy_bits >= 0 && policy_bits <= 7, "lg_diffaug_draw: policy bits %d outside 0..7 (1 color, 2 translation, 4 cutout)",
               policy_bits);
  hipLaunchKernelGGL(diffaug_draw_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long*>(key), call, r0, rows, S, policy_bits, params);
  LG_CHECK_LAUNCH("lg_diffaug_draw");
  return LG_OK;
}

extern "C" int lg_diffaug_fwd(const float* x, const float* params, float* out, int rows, int S, void* workspace, size_t ws_bytes,
                              void* stream) {
  if (int rc = check_map("lg_diffaug_fwd", x, params, out, rows, S, workspace, ws_bytes)) return rc;
  return run_map<false>("lg_diffaug_fwd", x, params, out, rows, S, workspace, (hipStream_t)stream);
}

extern "C" int lg_diffaug_bwd(const float* g, const float* params, float* gx, int rows, int S, void* workspace, size_t ws_bytes,
                              void* stream) {
  if (int rc = check_map("lg_diffaug_bwd", g, params, gx, rows, S, workspace, ws_bytes)) return rc;
  return run_map<true>("lg_diffaug_bwd", g, params, gx, rows, S, workspace, (hipStream_t)stream);
}
