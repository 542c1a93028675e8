// InstanceNorm + LeakyReLU apply passes whose SKIP operand is RAW: the skip is the bf16 conv output z_s of an encoder
// level together with that level's finished statistics records, not the normalised map — the encoder pass that produced it fed its
// next conv through the normalising forward (conv_down3's NORM form) and never wrote the map.  Per element
//     s = bf16(leaky(a_s ((z_s - mu_s) - mul_s) + b_s))          exactly apply16_kernel<0>'s stored value (lg_norm8's arithmetic)
//     y = leaky?(a ((z - mu) - mul) + b) + (float)s              exactly apply16p_kernel<2> / apply16_kernel<2> on that map
// so the result is bit-identical to normalise-then-apply (tests/test_adj_fused_gpu.py); -ffp-contract=off keeps every line one IEEE
// operation.  The passes are HBM-bound (8 bytes moved per element, as the bf16-skip forms): the second normalisation is free.
// Two forms, as norm.hip has them: with the statistics of z finished (lgadj_instnorm_apply_rs) and with their finalize folded into the
// launch (lgadj_instnorm_apply_p_rs: apply16p_kernel's merge, order and grid).  A file of its own: the kernels of norm.hip are held
// one by one to the exact-arithmetic cases of tests/test_norm_exact_gpu.py, these two to the bit-equality tests named above.
#include "lg_internal.h"
#include "../../include/littlegan_adj.h"

namespace {

typedef __bf16 bf16x8v __attribute__((ext_vector_type(8)));
struct f32x8 { f32x4 lo, hi; };

template <bool NT>
__device__ __forceinline__ f32x8 load8(const __bf16* p, long long i8) {  // elements [8*i8, 8*i8 + 8)
  const bf16x8v* q = reinterpret_cast<const bf16x8v*>(p + i8 * 8);
  const bf16x8v w = NT ? __builtin_nontemporal_load(q) : *q;
  f32x8 r;
  r.lo = f32x4{(float)w[0], (float)w[1], (float)w[2], (float)w[3]};
  r.hi = f32x4{(float)w[4], (float)w[5], (float)w[6], (float)w[7]};
  return r;
}
__device__ __forceinline__ void store8_bf16(__bf16* p, long long i8, const f32x8& v) {
  bf16x8v w;
  w[0] = (__bf16)v.lo[0]; w[1] = (__bf16)v.lo[1]; w[2] = (__bf16)v.lo[2]; w[3] = (__bf16)v.lo[3];
  w[4] = (__bf16)v.hi[0]; w[5] = (__bf16)v.hi[1]; w[6] = (__bf16)v.hi[2]; w[7] = (__bf16)v.hi[3];
  *reinterpret_cast<bf16x8v*>(p + i8 * 8) = w;
}
__device__ __forceinline__ void store8_f32(float* p, long long i8, const f32x8& v) {
  *reinterpret_cast<f32x4*>(p + i8 * 8) = v.lo;
  *reinterpret_cast<f32x4*>(p + i8 * 8 + 4) = v.hi;
}

constexpr int UNR = 2;                  // 16-B accesses in flight per thread and stream (norm.hip: EW8_UNR)
constexpr long long MAX_BLOCKS = 8192;  // norm.hip: EW_MAX_BLOCKS

struct Rec { float mu, a, b, mul; };    // the fields of a statistics record {mu_hi, sigma, a, beta, mu_lo, ...} the apply reads

// 8 elements of one sample: v = z (in) / y (out), s = the raw skip
__device__ __forceinline__ void apply8(f32x8& v, const f32x8& s, const Rec r, const Rec q, int post_leaky, float alpha) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float t = k < 4 ? v.lo[k & 3] : v.hi[k & 3];
    float h = k < 4 ? s.lo[k & 3] : s.hi[k & 3];
    t = r.a * ((t - r.mu) - r.mul) + r.b;
    if (post_leaky) t = lg_leaky(t, alpha);
    h = q.a * ((h - q.mu) - q.mul) + q.b;
    h = lg_leaky(h, alpha);
    h = (float)(__bf16)h;   // the skip map as the encoder's apply pass stores it: bf16, round to nearest even
    t += h;
    if (k < 4) v.lo[k & 3] = t; else v.hi[k & 3] = t;
  }
}

// statistics of z finished: a grid-stride pass over all samples (apply16_kernel<2>'s walk)
__global__ __launch_bounds__(256) void apply16_rs_kernel(const __bf16* __restrict__ x, const float* __restrict__ stats,
                                                         const __bf16* __restrict__ skip, const float* __restrict__ skip_stats,
                                                         float* __restrict__ y, __bf16* __restrict__ y16, long long L8, long long total8,
                                                         int post_leaky, float alpha) {
  const unsigned stride = gridDim.x * blockDim.x * UNR, tot = (unsigned)total8, l8 = (unsigned)L8;
  for (unsigned i0 = blockIdx.x * blockDim.x * UNR + threadIdx.x; i0 < tot; i0 += stride) {
    f32x8 v[UNR], sk[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const unsigned i = i0 + u * 256;
      if (i < tot) { v[u] = load8<false>(x, i); sk[u] = load8<false>(skip, i); }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const unsigned i = i0 + u * 256;
      if (i >= tot) break;
      const float* sp = stats + (long long)(i / l8) * LG_NSTAT;
      const float* sq = skip_stats + (long long)(i / l8) * LG_NSTAT;
      apply8(v[u], sk[u], Rec{sp[0], sp[2], sp[3], sp[4]}, Rec{sq[0], sq[2], sq[3], sq[4]}, post_leaky, alpha);
      if (y) store8_f32(y, i, v[u]);
      if (y16) store8_bf16(y16, i, v[u]);
    }
  }
}

// statistics of z FINALISED IN THE SAME LAUNCH — apply16p_kernel (norm.hip) line by line: grid (blocks per sample, B), samples and
// chunks walked from the END, the first wave of every block merges the sample's moment partials {count, mean, M2} as stats_final_kernel
// does (same order, same fp64 arithmetic), block 0 of a sample writes the record.
__global__ __launch_bounds__(256) void apply16p_rs_kernel(const __bf16* __restrict__ x, const double* __restrict__ partial, int nchunk,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float* __restrict__ stats, const __bf16* __restrict__ skip,
                                                          const float* __restrict__ skip_stats, float* __restrict__ y,
                                                          __bf16* __restrict__ y16, unsigned L8, int post_leaky, float alpha) {
  __shared__ float sst[8];
  const int n = (int)(gridDim.y - 1 - blockIdx.y);
  const unsigned bx = gridDim.x - 1 - blockIdx.x;
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const double* p = partial + (long long)n * nchunk * 3;
    double cnt = 0.0, sum = 0.0;
    for (int i = lane; i < nchunk; i += 64) { cnt += p[i * 3]; sum += p[i * 3] * p[i * 3 + 1]; }
    cnt = lg_wave_sum_d(cnt); sum = lg_wave_sum_d(sum);
    const double mean = sum / cnt;
    double m2 = 0.0;
    for (int i = lane; i < nchunk; i += 64) {
      const double d = p[i * 3 + 1] - mean;
      m2 += p[i * 3 + 2] + p[i * 3] * d * d;
    }
    m2 = lg_wave_sum_d(m2);
    if (lane == 0) {
      const double sigma = sqrt(m2 / cnt);
      const double a = (double)gamma[0] / (sigma + (double)LG_IN_EPS);
      const float mu_hi = (float)mean;
      sst[0] = mu_hi; sst[1] = (float)sigma; sst[2] = (float)a; sst[3] = beta[0]; sst[4] = (float)(mean - (double)mu_hi);
      if (bx == 0) {
        float* o = stats + (long long)n * LG_NSTAT;
        o[0] = mu_hi; o[1] = (float)sigma; o[2] = (float)a; o[3] = beta[0];
        o[4] = (float)(mean - (double)mu_hi); o[5] = 0.f; o[6] = 0.f; o[7] = 0.f;
      }
    }
  }
  __syncthreads();
  const Rec r{sst[0], sst[2], sst[3], sst[4]};
  const float* sq = skip_stats + (long long)n * LG_NSTAT;
  const Rec q{sq[0], sq[2], sq[3], sq[4]};
  const long long base = (long long)n * L8;
  const unsigned stride = gridDim.x * blockDim.x * UNR;
  const int ntrip = (int)((L8 + stride - 1) / stride);
  for (int tr = 0; tr < ntrip; ++tr) {
    const unsigned i0 = (unsigned)(ntrip - 1 - tr) * stride + bx * blockDim.x * UNR + threadIdx.x;
    if (i0 >= L8) continue;
    f32x8 v[UNR], sk[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const unsigned i = i0 + u * 256;
      if (i < L8) { v[u] = load8<true>(x, base + i); sk[u] = load8<true>(skip, base + i); }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const unsigned i = i0 + u * 256;
      if (i >= L8) break;
      apply8(v[u], sk[u], r, q, post_leaky, alpha);
      if (y) store8_f32(y, base + i, v[u]);
      if (y16) store8_bf16(y16, base + i, v[u]);
    }
  }
}

}  // namespace

extern "C" int lgadj_instnorm_apply_rs(const void* z16, const float* stats, const void* skip_z16, const float* skip_stats, float* y,
                                       void* y16, int B, long long L, int post_leaky, float alpha, void* stream) {
  LG_CHECK_ARG(z16 && stats && skip_z16 && skip_stats && (y || y16), "lgadj_instnorm_apply_rs: null pointer");
  LG_CHECK_ARG(B > 0 && L > 0 && L % 8 == 0 && (long long)B * L / 8 < (1LL << 31), "lgadj_instnorm_apply_rs: bad shape B=%d L=%lld", B, L);
  const long long total8 = (long long)B * L / 8;
  long long nb = (total8 + 256 * UNR - 1) / (256 * UNR);
  if (nb > MAX_BLOCKS) nb = MAX_BLOCKS;
  hipLaunchKernelGGL(apply16_rs_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const __bf16*)z16, stats,
                     (const __bf16*)skip_z16, skip_stats, y, (__bf16*)y16, L / 8, total8, post_leaky, alpha);
  LG_CHECK_LAUNCH("lgadj_instnorm_apply_rs");
  lg_note_kernel("apply16_rs_kernel");
  return LG_OK;
}

extern "C" int lgadj_instnorm_apply_p_rs(const void* z16, const void* partials, int nparts, const float* gamma, const float* beta,
                                         float* stats, const void* skip_z16, const float* skip_stats, float* y, void* y16, int B,
                                         long long L, int post_leaky, float alpha, void* stream) {
  LG_CHECK_ARG(z16 && partials && gamma && beta && stats && skip_z16 && skip_stats && (y || y16), "lgadj_instnorm_apply_p_rs: null pointer");
  LG_CHECK_ARG(nparts > 0 && B > 0 && B <= 65535 && L > 0 && L % 8 == 0 && L / 8 < (1LL << 31),
               "lgadj_instnorm_apply_p_rs: bad shape B=%d L=%lld nparts=%d", B, L, nparts);
  const long long L8 = L / 8;
  long long bps = (L8 + 256 * UNR * 4 - 1) / (256 * UNR * 4);   // apply16p_kernel's grid: ~4 trips per block
  if (bps * B > MAX_BLOCKS) bps = MAX_BLOCKS / B;
  if (bps < 1) bps = 1;
  hipLaunchKernelGGL(apply16p_rs_kernel, dim3((unsigned)bps, (unsigned)B), dim3(256), 0, (hipStream_t)stream, (const __bf16*)z16,
                     (const double*)partials, nparts, gamma, beta, stats, (const __bf16*)skip_z16, skip_stats, y, (__bf16*)y16,
                     (unsigned)L8, post_leaky, alpha);
  LG_CHECK_LAUNCH("lgadj_instnorm_apply_p_rs");
  lg_note_kernel("apply16p_rs_kernel");
  return LG_OK;
}
