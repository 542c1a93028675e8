// tr sqrt(S1 S2) and the Fréchet distance of the FID pass on the device, in fp64 (replaces the host scipy.linalg.sqrtm
// of the reference, fid.py:144-163).  Coupled Newton-Schulz iteration on A = S1 S2 (eigenvalues real and >= 0: A is similar to a PSD
// matrix):  c = |A|_F, Y0 = A / c, Z0 = I;  T = (3 I - Z Y) / 2, Y <- Y T, Z <- T Z;  t_k = sqrt(c) tr(Y_k) -> tr sqrt(A).
// Only the trace is needed.  The work is a general fp64 D x D x D GEMM on v_mfma_f64_16x16x4_f64 (64 x 64 output tiles, 4 waves of
// 32 x 32, epilogue C = alpha A B + beta I so that T is one launch; Y T and T Z share a launch) plus fixed-order trace / norm kernels:
// no atomics anywhere, the result is bit-reproducible.
#include "lg_internal.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int TILE = 64, KS = 32;
constexpr int LDB = TILE + 2;  // B tile [k][col]: pitch in doubles, as fid_cov_kernel (the k-strided fragment reads spread over banks)
constexpr int LDA = KS + 2;    // A tile [row][k] (row-major operand kept as it is read): 2 * 34 * row + 2 * k covers all 32 bank pairs

struct GemmProblem { const double* a; const double* b; double* c; };
struct GemmBatch { GemmProblem p[2]; };

// C = alpha A B + beta I, all D x D row-major fp64; blockIdx.x = output tile, blockIdx.y = problem.  Ragged D: rows / columns / k
// past D are read as 0 inside the tile and never written.
__global__ __launch_bounds__(256) void fid_gemm_kernel(GemmBatch batch, int D, int ntile, double alpha, double beta) {
  const GemmProblem pr = batch.p[blockIdx.y];
  const double* __restrict__ A = pr.a;
  const double* __restrict__ B = pr.b;
  double* __restrict__ Cm = pr.c;
  const int ti = blockIdx.x / ntile, tj = blockIdx.x - ti * ntile;
  const int i0 = ti * TILE, j0 = tj * TILE;
  __shared__ double sA[TILE * LDA], sB[KS * LDB];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int l15 = lane & 15, lk = lane >> 4;
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
  // staging: A tile 64 rows x 32 k, thread -> (row tid / 4, 8 consecutive k); B tile 32 k x 64 cols, thread -> (k tid / 8, 8 consecutive cols)
  const int ar = tid >> 2, ak = (tid & 3) * 8;
  const int bk = tid >> 3, bc = (tid & 7) * 8;
  // every row 16-byte aligned: the interior of a tile is read as double2
  const bool even = (D & 1) == 0 && (((uintptr_t)A | (uintptr_t)B) & 15) == 0;
  double ra[8], rb[8];
  auto fetch = [&](int k0) {
    const long long arow = (long long)(i0 + ar) * D, brow = (long long)(k0 + bk) * D;
    if (even && i0 + ar < D && k0 + ak + 8 <= D) {
#pragma unroll
      for (int q = 0; q < 8; q += 2) {
        const double2 v = *reinterpret_cast<const double2*>(A + arow + k0 + ak + q);
        ra[q] = v.x; ra[q + 1] = v.y;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) ra[q] = (i0 + ar < D && k0 + ak + q < D) ? A[arow + k0 + ak + q] : 0.0;
    }
    if (even && k0 + bk < D && j0 + bc + 8 <= D) {
#pragma unroll
      for (int q = 0; q < 8; q += 2) {
        const double2 v = *reinterpret_cast<const double2*>(B + brow + j0 + bc + q);
        rb[q] = v.x; rb[q + 1] = v.y;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) rb[q] = (k0 + bk < D && j0 + bc + q < D) ? B[brow + j0 + bc + q] : 0.0;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < D; k0 += KS) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      sA[ar * LDA + ak + q] = ra[q];
      sB[bk * LDB + bc + q] = rb[q];
    }
    __syncthreads();
    if (k0 + KS < D) fetch(k0 + KS);  // next slab's global loads fly under this slab's MFMAs
#pragma unroll
    for (int k4 = 0; k4 < KS; k4 += 4) {
      double af[2], bf[2];  // A[row = l15][k = lk], B[k = lk][col = l15]
#pragma unroll
      for (int a = 0; a < 2; ++a) af[a] = sA[(wr * 32 + a * 16 + l15) * LDA + k4 + lk];
#pragma unroll
      for (int b = 0; b < 2; ++b) bf[b] = sB[(k4 + lk) * LDB + wc * 32 + b * 16 + l15];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[a], bf[b], acc[a][b], 0, 0, 0);
    }
  }
  // C/D layout of the f64 instruction: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + wr * 32 + a * 16 + lk + 4 * e, j = j0 + wc * 32 + b * 16 + l15;
        if (i < D && j < D) Cm[(long long)i * D + j] = alpha * acc[a][b][e] + (i == j ? beta : 0.0);
      }
}

// fixed-order reductions: every thread sums a fixed strided subset, the block sum is a fixed tree + a serial pass (lg_block_sum_d)
constexpr int NORM_BLOCKS = 256;
__global__ __launch_bounds__(256) void fid_sumsq_partial_kernel(const double* __restrict__ x, long long n, double* __restrict__ part) {
  __shared__ double sm[16];
  double v[1] = {0.0};
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)NORM_BLOCKS * 256) v[0] += x[i] * x[i];
  lg_block_sum_d<1>(v, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = v[0];
}
// scal[0] = c = sqrt(sum of the partials)
__global__ __launch_bounds__(256) void fid_norm_final_kernel(const double* __restrict__ part, double* __restrict__ scal) {
  __shared__ double sm[16];
  double v[1] = {threadIdx.x < NORM_BLOCKS ? part[threadIdx.x] : 0.0};
  lg_block_sum_d<1>(v, sm);
  if (threadIdx.x == 0) scal[0] = sqrt(v[0]);
}
// Y = Y / c (c = scal[0], a device value), Z = I
__global__ __launch_bounds__(256) void fid_ns_init_kernel(double* __restrict__ Y, double* __restrict__ Z, const double* __restrict__ scal,
                                                          int D) {
  const double c = scal[0];
  const long long n = (long long)D * D;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    Y[i] = Y[i] / c;
    Z[i] = (i / D == i % D) ? 1.0 : 0.0;
  }
}
// out[0] = tr(Y)
__global__ __launch_bounds__(256) void fid_trace_kernel(const double* __restrict__ Y, int D, double* __restrict__ out) {
  __shared__ double sm[16];
  double v[1] = {0.0};
  for (int i = threadIdx.x; i < D; i += 256) v[0] += Y[(long long)i * D + i];
  lg_block_sum_d<1>(v, sm);
  if (threadIdx.x == 0) out[0] = v[0];
}
// out[0] = |mu1 - mu2|^2, out[1] = tr S1, out[2] = tr S2
__global__ __launch_bounds__(256) void fid_terms_kernel(const double* __restrict__ mu1, const double* __restrict__ s1,
                                                        const double* __restrict__ mu2, const double* __restrict__ s2, int D,
                                                        double* __restrict__ out) {
  __shared__ double sm[48];
  double v[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < D; i += 256) {
    const double d = mu1[i] - mu2[i];
    v[0] += d * d;
    v[1] += s1[(long long)i * D + i];
    v[2] += s2[(long long)i * D + i];
  }
  lg_block_sum_d<3>(v, sm);
  if (threadIdx.x == 0) { out[0] = v[0]; out[1] = v[1]; out[2] = v[2]; }
}

int launch_gemm(hipStream_t st, int D, int nprob, const GemmBatch& batch, double alpha, double beta) {
  const int ntile = (D + TILE - 1) / TILE;
  hipLaunchKernelGGL(fid_gemm_kernel, dim3(ntile * ntile, nprob), dim3(256), 0, st, batch, D, ntile, alpha, beta);
  LG_CHECK_LAUNCH("fid_gemm_kernel");
  return LG_OK;
}

constexpr size_t SCAL_BYTES = 4096;  // scalars [c, t, dmu2, tr1, tr2] + NORM_BLOCKS partials, in front of the matrices
inline bool finite_d(double x) { return x - x == 0.0; }

}  // namespace

// c = alpha_beta[0] a b + alpha_beta[1] I  (a, b, c: D x D row-major fp64 on the device, c distinct from a and b; alpha_beta: 2 HOST doubles)
extern "C" int lg_fid_gemm(const double* a, const double* b, double* c, int D, const double* alpha_beta, void* stream) {
  LG_CHECK_ARG(a && b && c && alpha_beta, "lg_fid_gemm: null pointer");
  LG_CHECK_ARG(D > 0 && D <= (1 << 14), "lg_fid_gemm: bad shape D=%d", D);
  LG_CHECK_ARG(c != a && c != b, "lg_fid_gemm: the output aliases an operand");
  GemmBatch batch;
  batch.p[0] = GemmProblem{a, b, c};
  batch.p[1] = batch.p[0];
  return launch_gemm((hipStream_t)stream, D, 1, batch, alpha_beta[0], alpha_beta[1]);
}

extern "C" size_t lg_fid_distance_workspace_bytes(int D) {
  return D > 0 ? SCAL_BYTES + 5 * (size_t)D * (size_t)D * sizeof(double) : 0;
}

extern "C" int lg_fid_distance(const double* mu1, const double* sigma1, const double* mu2, const double* sigma2, int D, int max_iter,
                               double* result_host, void* workspace, size_t ws_bytes, void* stream) {
  LG_CHECK_ARG(mu1 && sigma1 && mu2 && sigma2 && result_host && workspace, "lg_fid_distance: null pointer");
  LG_CHECK_ARG(D > 0 && D <= (1 << 14) && max_iter >= 1, "lg_fid_distance: bad shape D=%d max_iter=%d", D, max_iter);
  LG_CHECK_ARG(ws_bytes >= lg_fid_distance_workspace_bytes(D), "lg_fid_distance: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  double* scal = (double*)workspace;  // [0] c, [1] tr(Y), [2..4] |dmu|^2, tr S1, tr S2, [8..8+NORM_BLOCKS) partials
  double* part = scal + 8;
  const size_t dd = (size_t)D * (size_t)D;
  double* Y = (double*)((char*)workspace + SCAL_BYTES);
  double *Y2 = Y + dd, *Z = Y + 2 * dd, *Z2 = Y + 3 * dd, *T = Y + 4 * dd;
  double host[5];
  auto fetch = [&](double* dst, const double* src, int n) -> int {
    hipError_t e = hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
      lg_set_error("lg_fid_distance: copy back failed: %s", hipGetErrorString(e));
      return LG_ERR_LAUNCH;
    }
    return LG_OK;
  };
  int rc;
  GemmBatch batch;
  batch.p[0] = GemmProblem{sigma1, sigma2, Y};
  batch.p[1] = batch.p[0];
  if ((rc = launch_gemm(st, D, 1, batch, 1.0, 0.0)) != LG_OK) return rc;  // A = S1 S2
  hipLaunchKernelGGL(fid_sumsq_partial_kernel, dim3(NORM_BLOCKS), dim3(256), 0, st, (const double*)Y, (long long)dd, part);
  LG_CHECK_LAUNCH("lg_fid_distance(norm)");
  hipLaunchKernelGGL(fid_norm_final_kernel, dim3(1), dim3(256), 0, st, (const double*)part, scal);
  LG_CHECK_LAUNCH("lg_fid_distance(norm final)");
  hipLaunchKernelGGL(fid_terms_kernel, dim3(1), dim3(256), 0, st, mu1, sigma1, mu2, sigma2, D, scal + 2);
  LG_CHECK_LAUNCH("lg_fid_distance(terms)");
  if ((rc = fetch(host, scal, 5)) != LG_OK) return rc;
  const double c = host[0], base = host[2] + host[3] + host[4];
  double t_final = 0.0;
  int iters = 0, status = 0;
  if (!finite_d(c)) {
    status = 1;
    t_final = c;
  } else if (c > 0.0) {
    const int nb = (int)((dd + 255) / 256 < 2048 ? (dd + 255) / 256 : 2048);
    hipLaunchKernelGGL(fid_ns_init_kernel, dim3(nb), dim3(256), 0, st, Y, Z, (const double*)scal, D);
    LG_CHECK_LAUNCH("lg_fid_distance(init)");
    hipLaunchKernelGGL(fid_trace_kernel, dim3(1), dim3(256), 0, st, (const double*)Y, D, scal + 1);
    LG_CHECK_LAUNCH("lg_fid_distance(trace)");
    if ((rc = fetch(host, scal + 1, 1)) != LG_OK) return rc;
    const double sc = sqrt(c);
    double t_prev = sc * host[0], d_prev = HUGE_VAL;
    status = 1;
    t_final = t_prev;
    for (int k = 1; k <= max_iter; ++k) {
      iters = k;
      batch.p[0] = GemmProblem{Z, Y, T};
      batch.p[1] = batch.p[0];
      if ((rc = launch_gemm(st, D, 1, batch, -0.5, 1.5)) != LG_OK) return rc;  // T = (3 I - Z Y) / 2
      batch.p[0] = GemmProblem{Y, T, Y2};
      batch.p[1] = GemmProblem{T, Z, Z2};
      if ((rc = launch_gemm(st, D, 2, batch, 1.0, 0.0)) != LG_OK) return rc;   // Y T and T Z in one launch
      hipLaunchKernelGGL(fid_trace_kernel, dim3(1), dim3(256), 0, st, (const double*)Y2, D, scal + 1);
      LG_CHECK_LAUNCH("lg_fid_distance(trace)");
      if ((rc = fetch(host, scal + 1, 1)) != LG_OK) return rc;
      const double t = sc * host[0];
      if (!finite_d(t)) break;  // status 1, t_{k-1}
      const double d = fabs(t - t_prev);
      if (d <= 1e-12 * fabs(t)) { t_final = t; status = 0; break; }
      if (d >= d_prev && d <= 1e-5 * fabs(t)) { status = 0; break; }  // rounding floor: t_{k-1}
      t_prev = t; d_prev = d; t_final = t;
      double* s_ = Y; Y = Y2; Y2 = s_;
      s_ = Z; Z = Z2; Z2 = s_;
    }
  }
  result_host[0] = base - 2.0 * t_final;
  result_host[1] = t_final;
  result_host[2] = (double)iters;
  result_host[3] = (double)status;
  return LG_OK;
}
