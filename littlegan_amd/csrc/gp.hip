// Gradient penalty of the discriminator (use_gp / gp_weight, /root/reference/sample.config.json:35-36).  The reference declares the
// switch and raises where it would be used (/root/reference/eager_trainer.py:141-143); this project defines the penalty itself as
// the WGAN-GP form (Gulrajani et al., 2017) on D's first output — a choice of this project, not of the reference:
//   x^_b = eps_b new_image_b + (1 - eps_b) fake_b,   p_b = output_pr(x^_b) (the sigmoid),   g_b = dp_b / dx^_b,   r_b = |g_b|_2,
//   gp = mean_b (r_b - 1)^2,   disc_loss += gp_weight gp.
// Its weight gradient is reverse over reverse: the first backward to the image, the seed u0 = dgp/dg, an upward
// adjoint sweep through the encoder, and a second backward seeded by the heads' second-order term.  The kernels here are the parts
// the library did not have: the interpolation, the seed, the InstanceNormalization backward with an injected adjoint, its double
// backward and the heads' second-order terms.  Convolutions and weight gradients are the library's own.
// InstanceNormalization per sample (axis=None): c = z - mu, sigma = sqrt(mean c^2), s = sigma + 1e-3, n = gamma c / s + beta,
// x = leaky(n), m = leaky'(n), gn = m g.  Statistics records [B][8] = {mu_hi, sigma, a, beta, mu_lo, ...} (norm.hip).
// Every reduction has a fixed order (per-block fp64 partials, merged in index order): bit-deterministic, no atomics.
#include "lg_internal.h"

namespace {

constexpr int CHUNK = 4096;  // elements per partial record at most (256 threads x 4 float4)
constexpr int NS = 5;        // doubles per norm partial record

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 ld4(const __bf16* p) {
  const uint2 w = *reinterpret_cast<const uint2*>(p);
  return f32x4{__builtin_bit_cast(float, w.x << 16), __builtin_bit_cast(float, w.x & 0xffff0000u),
               __builtin_bit_cast(float, w.y << 16), __builtin_bit_cast(float, w.y & 0xffff0000u)};
}
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void st4_16(__bf16* p, f32x4 v) {
  typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
  const unsigned lo = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{v[0], v[1]}, bf2));
  const unsigned hi = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{v[2], v[3]}, bf2));
  *reinterpret_cast<uint2*>(p) = uint2{lo, hi};
}

// fixed-order sum over the 256 threads of a block (tree in shared memory); result valid in thread 0
__device__ __forceinline__ double block_tree_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  return sh[0];
}

// out = eps_b a + (1 - eps_b) b
__global__ __launch_bounds__(256) void gp_interp_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        const float* __restrict__ eps, float* __restrict__ out, unsigned L4,
                                                        unsigned total4) {
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total4; i += gridDim.x * 256) {
    const float e = eps[i / L4], f = 1.0f - e;
    const f32x4 av = ld4(a + 4ull * i), bv = ld4(b + 4ull * i);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = e * av[k] + f * bv[k];
    st4(out + 4ull * i, o);
  }
}

// part[n][j] = sum of g^2 over the elements of sample n that block j covers
__global__ __launch_bounds__(256) void gp_sumsq_kernel(const float* __restrict__ g, double* __restrict__ part, long long L,
                                                       int nparts) {
  const int n = blockIdx.y;
  __shared__ double sred[16];
  double s = 0.0;
  const float* gs = g + (long long)n * L;
  for (long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; e < L; e += (long long)gridDim.x * 1024) {
    const f32x4 v = ld4(gs + e);
    s += (double)(v[0] * v[0] + v[1] * v[1]) + (double)(v[2] * v[2] + v[3] * v[3]);
  }
  double red[1] = {s};
  lg_block_sum_d<1>(red, sred);
  if (threadIdx.x == 0) part[(long long)n * nparts + blockIdx.x] = red[0];
}

// r_b, coef_b = (2 w / B)(r_b - 1) / max(r_b, 1e-12); loss (+)= w gp, gp_loss = w gp
__global__ __launch_bounds__(256) void gp_seed_final_kernel(const double* __restrict__ part, int nparts, int B, float w,
                                                            float* __restrict__ r, float* __restrict__ coef,
                                                            float* __restrict__ loss, float* __restrict__ gp_loss) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (int n = threadIdx.x; n < B; n += 256) {
    double s = 0.0;
    for (int j = 0; j < nparts; ++j) s += part[(long long)n * nparts + j];
    const double rr = sqrt(s);
    r[n] = (float)rr;
    coef[n] = (float)(2.0 * (double)w / (double)B * (rr - 1.0) / fmax(rr, 1e-12));
    acc += (rr - 1.0) * (rr - 1.0);
  }
  const double tot = block_tree_sum(acc, sh);
  if (threadIdx.x == 0) {
    const float term = (float)((double)w * tot / (double)B);
    if (loss) loss[0] = loss[0] + term;
    if (gp_loss) gp_loss[0] = term;
  }
}

// u0 = coef_b g
__global__ __launch_bounds__(256) void gp_scale_kernel(const float* __restrict__ g, const float* __restrict__ coef,
                                                       float* __restrict__ u0, unsigned L4, unsigned total4) {
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total4; i += gridDim.x * 256) {
    const float k = coef[i / L4];
    const f32x4 v = ld4(g + 4ull * i);
    st4(u0 + 4ull * i, f32x4{k * v[0], k * v[1], k * v[2], k * v[3]});
  }
}

// per (sample, block) sums {sum gn, sum gn c [, sum u, sum u c, sum u gn]} (DD: the three u sums too)
template <typename TZ, bool DD>
__global__ __launch_bounds__(256) void gp_norm_sums_kernel(const TZ* __restrict__ z, const float* __restrict__ stats,
                                                           const float* __restrict__ g, const float* __restrict__ u,
                                                           double* __restrict__ part, long long L, int nparts, float alpha) {
  const int n = blockIdx.y;
  const float* sp = stats + (long long)n * LG_NSTAT;
  const float mu = sp[0], a = sp[2], b = sp[3], mul = sp[4];
  __shared__ double sred[NS * 16];
  double s[NS] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const long long base = (long long)n * L;
  for (long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; e < L; e += (long long)gridDim.x * 1024) {
    const f32x4 zv = ld4(z + base + e), gv = ld4(g + base + e);
    f32x4 uv = {0.f, 0.f, 0.f, 0.f};
    if (DD) uv = ld4(u + base + e);
    float q[NS] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float c = (zv[k] - mu) - mul;
      const float gn = (a * c + b > 0.f) ? gv[k] : alpha * gv[k];
      q[0] += gn;
      q[1] += gn * c;
      if (DD) {
        q[2] += uv[k];
        q[3] += uv[k] * c;
        q[4] += uv[k] * gn;
      }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] += (double)q[i];
  }
  lg_block_sum_d<NS>(s, sred);
  if (threadIdx.x == 0) {
    double* o = part + ((long long)n * nparts + blockIdx.x) * NS;
#pragma unroll
    for (int i = 0; i < NS; ++i) o[i] = s[i];
  }
}

// per-sample coefficients of the apply pass and the gamma / beta contributions (summed over samples in index order).
//   first order (dd = 0): dz = k1 gn + k0 + kc c [+ add],  k1 = gamma/s, k0 = -gamma A/s, kc = -gamma M/(s^2 sigma);
//                         dgamma += sum_b N M/s, dbeta += sum_b N A.
//   double backward (dd = 1): u_h = m (k1 u + k0 + kc c) with k0 = -gamma U/(N s), kc = -gamma P/(N s^2 sigma);
//                         u_z2 = ec c + eg gn + eu u + e0;  dgamma += sum_b (T1 - M P/(s sigma))/s.
// A = mean gn, M = mean gn c, U = sum u, P = sum u c, T1 = sum u gn - A U.
__global__ __launch_bounds__(256) void gp_norm_coef_kernel(const double* __restrict__ part, int nparts,
                                                           const float* __restrict__ stats, const float* __restrict__ gamma,
                                                           float* __restrict__ coef, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, int B, long long L, int dd) {
  __shared__ double sh[256];
  double ag = 0.0, ab = 0.0;
  const double gm = (double)gamma[0], N = (double)L;
  for (int n = threadIdx.x; n < B; n += 256) {
    double S[NS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < nparts; ++j)
      for (int i = 0; i < NS; ++i) S[i] += part[((long long)n * nparts + j) * NS + i];
    const double sigma = (double)stats[(long long)n * LG_NSTAT + 1], s = sigma + (double)LG_IN_EPS;
    const double A = S[0] / N, M = S[1] / N;
    float* o = coef + (long long)n * 8;
    if (!dd) {
      o[0] = (float)(gm / s); o[1] = (float)(-gm * A / s); o[2] = (float)(-gm * M / (s * s * sigma));
      o[3] = o[4] = o[5] = o[6] = o[7] = 0.f;
      ag += S[1] / s;
      ab += S[0];
    } else {
      const double U = S[2], P = S[3], T1 = S[4] - A * U, q = gm / (s * s * sigma);
      o[0] = (float)(gm / s); o[1] = (float)(-gm * U / (N * s)); o[2] = (float)(-q * P / N);
      o[3] = (float)(-q * T1 / N + q * M * P * (2.0 / s + 1.0 / sigma) / (N * sigma));
      o[4] = (float)(-q * P / N); o[5] = (float)(-q * M); o[6] = (float)(q * (P * A + M * U) / N); o[7] = 0.f;
      ag += (T1 - M * P / (s * sigma)) / s;
    }
  }
  const double tg = block_tree_sum(ag, sh);
  __syncthreads();
  const double tb = block_tree_sum(ab, sh);
  if (threadIdx.x == 0) {
    if (dgamma) dgamma[0] = dgamma[0] + (float)tg;
    if (dbeta && !dd) dbeta[0] = dbeta[0] + (float)tb;
  }
}

// first order: o1 = k1 gn + k0 + kc c [+ u]  (u = the injected adjoint, may be null), o16 (may be null) its bf16 mirror.
// double backward: o1 = u_h, o2 (may be null) = u_z2.
template <typename TZ, bool DD>
__global__ __launch_bounds__(256) void gp_norm_apply_kernel(const TZ* __restrict__ z, const float* __restrict__ stats,
                                                            const float* __restrict__ g, const float* __restrict__ u,
                                                            const float* __restrict__ coef, float* __restrict__ o1,
                                                            __bf16* __restrict__ o16, float* __restrict__ o2, unsigned L4,
                                                            unsigned total4, float alpha) {
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total4; i += gridDim.x * 256) {
    const unsigned n = i / L4;
    const float* sp = stats + (unsigned long long)n * LG_NSTAT;
    const float* cf = coef + (unsigned long long)n * 8;
    const float mu = sp[0], a = sp[2], b = sp[3], mul = sp[4];
    const unsigned long long e = 4ull * i;
    const f32x4 zv = ld4(z + e), gv = ld4(g + e);
    f32x4 uv = {0.f, 0.f, 0.f, 0.f};
    if (u) uv = ld4(u + e);
    f32x4 r1, r2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float c = (zv[k] - mu) - mul;
      const bool pos = a * c + b > 0.f;
      const float gn = pos ? gv[k] : alpha * gv[k];
      if (!DD) {
        r1[k] = (cf[0] * gn + cf[1]) + cf[2] * c + uv[k];
      } else {
        const float t = (cf[0] * uv[k] + cf[1]) + cf[2] * c;
        r1[k] = pos ? t : alpha * t;
        r2[k] = ((cf[3] * c + cf[4] * gn) + cf[5] * uv[k]) + cf[6];
      }
    }
    if (o1) st4(o1 + e, r1);
    if (o16) st4_16(o16 + e, r1);
    if (DD && o2) st4(o2 + e, r2);
  }
}

// g[b][k] = sigma'(s_b) wpr[k], sigma' = p (1 - p): dp_b / d(heads input)
__global__ __launch_bounds__(256) void gp_heads_seed_kernel(const float* __restrict__ p, int J, const float* __restrict__ wpr,
                                                            float* __restrict__ g, int B, int K) {
  const long long tot = (long long)B * K;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < tot; i += (long long)gridDim.x * 256) {
    const int n = (int)(i / K), k = (int)(i - (long long)n * K);
    const float pr = p[(long long)n * J];
    g[i] = (pr * (1.0f - pr)) * wpr[k];
  }
}

// t_b = sigma''(s_b) <wpr, u_b>, sigma'' = p (1 - p)(1 - 2p); one block per sample
__global__ __launch_bounds__(256) void gp_heads_t_kernel(const float* __restrict__ p, int J, const float* __restrict__ wpr,
                                                         const float* __restrict__ u, float* __restrict__ t, int K) {
  const int n = blockIdx.x;
  __shared__ double sred[16];
  double s = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) s += (double)(wpr[k] * u[(long long)n * K + k]);
  double red[1] = {s};
  lg_block_sum_d<1>(red, sred);
  if (threadIdx.x == 0) {
    const double pr = (double)p[(long long)n * J];
    t[n] = (float)(pr * (1.0 - pr) * (1.0 - 2.0 * pr) * red[0]);
  }
}

// g2[b][k] = t_b wpr[k] (the second backward's gradient on the heads input); dwpr[k] += sum_b (sigma'_b u[b][k] + t_b x[b][k]),
// dbpr += sum_b t_b (both may be null).  One thread per column, rows in index order.
__global__ __launch_bounds__(256) void gp_heads_col_kernel(const float* __restrict__ p, int J, const float* __restrict__ wpr,
                                                           const float* __restrict__ x, const float* __restrict__ u,
                                                           const float* __restrict__ t, float* __restrict__ g2,
                                                           float* __restrict__ dwpr, float* __restrict__ dbpr, int B, int K) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < K) {
    const float w = wpr[k];
    double acc = 0.0;
    for (int n = 0; n < B; ++n) {
      const long long i = (long long)n * K + k;
      const float tn = t[n], pr = p[(long long)n * J];
      g2[i] = tn * w;
      if (dwpr) acc += (double)((pr * (1.0f - pr)) * u[i]) + (double)(tn * x[i]);
    }
    if (dwpr) dwpr[k] = dwpr[k] + (float)acc;
  }
  if (dbpr && blockIdx.x == 0 && threadIdx.x == 0) {
    double s = 0.0;
    for (int n = 0; n < B; ++n) s += (double)t[n];
    dbpr[0] = dbpr[0] + (float)s;
  }
}

// resident blocks of a 256-thread kernel (occupancy query once per kernel) over the CUs the persistent kernels may fill
#define GP_RESIDENT(kern)                                                                                              \
  ([]() -> long long {                                                                                                 \
    static int per_cu = 0;                                                                                             \
    if (!per_cu && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, 0) != hipSuccess || per_cu < 1)) \
      per_cu = 4;                                                                                                      \
    return (long long)per_cu * lg_grid_cus();                                                                          \
  }())

// element-wise grids: the blocks the work needs, at most one round of residency (threads then stride)
inline int ew_grid(long long total4, long long resident) {
  long long nb = (total4 + 255) / 256;
  if (nb > resident) nb = resident;
  return (int)(nb < 1 ? 1 : nb);
}
inline int nchunks(long long L) { return (int)((L + CHUNK - 1) / CHUNK); }
// blocks per sample of the reduction passes: B * nparts within one round of residency, at most one chunk per block
inline int parts_of(int B, long long L, long long resident) {
  long long np = resident / B;
  if (np > nchunks(L)) np = nchunks(L);
  return (int)(np < 1 ? 1 : np);
}
inline size_t al(size_t n) { return (n + 255) / 256 * 256; }
inline size_t part_bytes(int B, long long L) { return al((size_t)B * nchunks(L) * NS * sizeof(double)); }

bool shape_ok(int B, long long L) { return B > 0 && B <= 65535 && L > 0 && L % 4 == 0 && (long long)B * L / 4 < (1LL << 31); }

template <typename TZ>
int norm_run(const TZ* z, const float* stats, const float* gamma, const float* g, const float* u, float* o1, void* o16, float* o2,
             float* dgamma, float* dbeta, void* workspace, int B, long long L, float alpha, bool dd, hipStream_t st) {
  double* part = (double*)workspace;
  float* coef = (float*)((char*)workspace + part_bytes(B, L));
  const unsigned total4 = (unsigned)((long long)B * L / 4), L4 = (unsigned)(L / 4);
  if (dd) {
    const int np = parts_of(B, L, GP_RESIDENT((gp_norm_sums_kernel<TZ, true>)));
    hipLaunchKernelGGL((gp_norm_sums_kernel<TZ, true>), dim3(np, B), dim3(256), 0, st, z, stats, g, u, part, L, np, alpha);
    LG_CHECK_LAUNCH("lg_gp_norm_dd(sums)");
    hipLaunchKernelGGL(gp_norm_coef_kernel, dim3(1), dim3(256), 0, st, (const double*)part, np, stats, gamma, coef, dgamma,
                       (float*)nullptr, B, L, 1);
    LG_CHECK_LAUNCH("lg_gp_norm_dd(coef)");
    hipLaunchKernelGGL((gp_norm_apply_kernel<TZ, true>), dim3(ew_grid(total4, GP_RESIDENT((gp_norm_apply_kernel<TZ, true>)))),
                       dim3(256), 0, st, z, stats, g, u, (const float*)coef, o1, (__bf16*)nullptr, o2, L4, total4, alpha);
    LG_CHECK_LAUNCH("lg_gp_norm_dd(apply)");
  } else {
    const int np = parts_of(B, L, GP_RESIDENT((gp_norm_sums_kernel<TZ, false>)));
    hipLaunchKernelGGL((gp_norm_sums_kernel<TZ, false>), dim3(np, B), dim3(256), 0, st, z, stats, g, (const float*)nullptr, part,
                       L, np, alpha);
    LG_CHECK_LAUNCH("lg_gp_norm_bwd(sums)");
    hipLaunchKernelGGL(gp_norm_coef_kernel, dim3(1), dim3(256), 0, st, (const double*)part, np, stats, gamma, coef, dgamma, dbeta,
                       B, L, 0);
    LG_CHECK_LAUNCH("lg_gp_norm_bwd(coef)");
    hipLaunchKernelGGL((gp_norm_apply_kernel<TZ, false>), dim3(ew_grid(total4, GP_RESIDENT((gp_norm_apply_kernel<TZ, false>)))),
                       dim3(256), 0, st, z, stats, g, u, (const float*)coef, o1, (__bf16*)o16, (float*)nullptr, L4, total4, alpha);
    LG_CHECK_LAUNCH("lg_gp_norm_bwd(apply)");
  }
  return LG_OK;
}

}  // namespace

extern "C" size_t lg_gp_workspace_bytes(int B, long long L) {
  if (B <= 0 || L <= 0) return 0;
  return part_bytes(B, L) + al((size_t)B * 8 * sizeof(float));
}

extern "C" int lg_gp_interp(const float* real, const float* fake, const float* eps, float* out, int B, long long L, void* stream) {
  LG_CHECK_ARG(real && fake && eps && out, "lg_gp_interp: null pointer");
  LG_CHECK_ARG(shape_ok(B, L), "lg_gp_interp: bad shape B=%d L=%lld", B, L);
  const unsigned total4 = (unsigned)((long long)B * L / 4);
  lg_note_kernel("gp_interp_kernel");
  hipLaunchKernelGGL(gp_interp_kernel, dim3(ew_grid(total4, GP_RESIDENT(gp_interp_kernel))), dim3(256), 0, (hipStream_t)stream,
                     real, fake, eps, out, (unsigned)(L / 4), total4);
  LG_CHECK_LAUNCH("lg_gp_interp");
  return LG_OK;
}

extern "C" int lg_gp_seed(const float* g, float* u0, float* r, float* loss, float* gp_loss, float gp_weight, void* workspace,
                          size_t ws_bytes, int B, long long L, void* stream) {
  LG_CHECK_ARG(g && u0 && r && workspace, "lg_gp_seed: null pointer");
  LG_CHECK_ARG(shape_ok(B, L), "lg_gp_seed: bad shape B=%d L=%lld", B, L);
  LG_CHECK_ARG(ws_bytes >= lg_gp_workspace_bytes(B, L), "lg_gp_seed: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  float* coef = (float*)((char*)workspace + part_bytes(B, L));
  const int np = parts_of(B, L, GP_RESIDENT(gp_sumsq_kernel));
  lg_note_kernel("gp_seed");
  hipLaunchKernelGGL(gp_sumsq_kernel, dim3(np, B), dim3(256), 0, st, g, part, L, np);
  LG_CHECK_LAUNCH("lg_gp_seed(sumsq)");
  hipLaunchKernelGGL(gp_seed_final_kernel, dim3(1), dim3(256), 0, st, (const double*)part, np, B, gp_weight, r, coef, loss, gp_loss);
  LG_CHECK_LAUNCH("lg_gp_seed(final)");
  const unsigned total4 = (unsigned)((long long)B * L / 4);
  hipLaunchKernelGGL(gp_scale_kernel, dim3(ew_grid(total4, GP_RESIDENT(gp_scale_kernel))), dim3(256), 0, st, g, (const float*)coef,
                     u0, (unsigned)(L / 4), total4);
  LG_CHECK_LAUNCH("lg_gp_seed(scale)");
  return LG_OK;
}

extern "C" int lg_gp_norm_bwd(const float* z, const void* z16, const float* stats, const float* gamma, const float* g,
                              const float* add, float* dz, void* dz16, float* dgamma, float* dbeta, void* workspace,
                              size_t ws_bytes, int B, long long L, float alpha, void* stream) {
  LG_CHECK_ARG((z != nullptr) != (z16 != nullptr), "lg_gp_norm_bwd: give exactly one of z, z16");
  LG_CHECK_ARG(stats && gamma && g && (dz || dz16) && workspace, "lg_gp_norm_bwd: null pointer");
  LG_CHECK_ARG(shape_ok(B, L), "lg_gp_norm_bwd: bad shape B=%d L=%lld", B, L);
  LG_CHECK_ARG(ws_bytes >= lg_gp_workspace_bytes(B, L), "lg_gp_norm_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (z16) {
    lg_note_kernel("gp_norm_apply_kernel<bf16,bwd>");
    return norm_run((const __bf16*)z16, stats, gamma, g, add, dz, dz16, nullptr, dgamma, dbeta, workspace, B, L, alpha, false, st);
  }
  lg_note_kernel("gp_norm_apply_kernel<f32,bwd>");
  return norm_run(z, stats, gamma, g, add, dz, dz16, nullptr, dgamma, dbeta, workspace, B, L, alpha, false, st);
}

extern "C" int lg_gp_norm_dd(const float* z, const void* z16, const float* stats, const float* gamma, const float* g,
                             const float* u, float* uh, float* uz2, float* dgamma, void* workspace, size_t ws_bytes, int B,
                             long long L, float alpha, void* stream) {
  LG_CHECK_ARG((z != nullptr) != (z16 != nullptr), "lg_gp_norm_dd: give exactly one of z, z16");
  LG_CHECK_ARG(stats && gamma && g && u && uh && workspace, "lg_gp_norm_dd: null pointer");
  LG_CHECK_ARG(shape_ok(B, L), "lg_gp_norm_dd: bad shape B=%d L=%lld", B, L);
  LG_CHECK_ARG(ws_bytes >= lg_gp_workspace_bytes(B, L), "lg_gp_norm_dd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (z16) {
    lg_note_kernel("gp_norm_apply_kernel<bf16,dd>");
    return norm_run((const __bf16*)z16, stats, gamma, g, u, uh, nullptr, uz2, dgamma, nullptr, workspace, B, L, alpha, true, st);
  }
  lg_note_kernel("gp_norm_apply_kernel<f32,dd>");
  return norm_run(z, stats, gamma, g, u, uh, nullptr, uz2, dgamma, nullptr, workspace, B, L, alpha, true, st);
}

extern "C" int lg_gp_heads_seed(const float* p, const float* wpr, float* g, int B, int K, int c, void* stream) {
  LG_CHECK_ARG(p && wpr && g, "lg_gp_heads_seed: null pointer");
  LG_CHECK_ARG(B > 0 && K > 0 && c >= 0 && (long long)B * K < (1LL << 31), "lg_gp_heads_seed: bad shape B=%d K=%d c=%d", B, K, c);
  lg_note_kernel("gp_heads_seed_kernel");
  hipLaunchKernelGGL(gp_heads_seed_kernel, dim3(ew_grid((long long)B * K, GP_RESIDENT(gp_heads_seed_kernel))), dim3(256), 0,
                     (hipStream_t)stream, p, 1 + c, wpr, g, B, K);
  LG_CHECK_LAUNCH("lg_gp_heads_seed");
  return LG_OK;
}

extern "C" int lg_gp_heads_2nd(const float* p, const float* wpr, const float* x, const float* u, float* t, float* g2, float* dwpr,
                               float* dbpr, int B, int K, int c, void* stream) {
  LG_CHECK_ARG(p && wpr && u && t && g2, "lg_gp_heads_2nd: null pointer");
  LG_CHECK_ARG(!dwpr || x, "lg_gp_heads_2nd: dwpr needs the heads input x");
  LG_CHECK_ARG(B > 0 && K > 0 && c >= 0 && (long long)B * K < (1LL << 31), "lg_gp_heads_2nd: bad shape B=%d K=%d c=%d", B, K, c);
  hipStream_t st = (hipStream_t)stream;
  lg_note_kernel("gp_heads_2nd");
  hipLaunchKernelGGL(gp_heads_t_kernel, dim3(B), dim3(256), 0, st, p, 1 + c, wpr, u, t, K);
  LG_CHECK_LAUNCH("lg_gp_heads_2nd(t)");
  hipLaunchKernelGGL(gp_heads_col_kernel, dim3((K + 255) / 256), dim3(256), 0, st, p, 1 + c, wpr, x, u, (const float*)t, g2, dwpr,
                     dbpr, B, K);
  LG_CHECK_LAUNCH("lg_gp_heads_2nd(columns)");
  return LG_OK;
}
