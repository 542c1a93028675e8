// Pairwise passes over two activation sets X [n][D] against Y [m][D] (fp32, device) for the sample-based metrics of metrics.py
// (DESIGN.md 19): KID (Binkowski et al. 2018) and precision / recall / density / coverage (Kynkaanniemi et al. 2019, Naeem et al.
// 2020).  The reference has no counterpart.  One tile loop, three epilogues: a block computes a 64 x 64 tile of dot(x_i, y_j) in fp64
// on v_mfma_f64_16x16x4_f64 (4 waves of 32 x 32, as fid_cov_kernel / fid_gemm_kernel), both operands [rows][D], i.e. k-contiguous as
// read (fid_gemm_kernel's A-side LDS layout on both sides), fp32 converted to fp64 on the way into LDS, ragged n / m / D read as 0.
//   poly_sum   : k_ij = (gamma dot + coef0)^degree, tile sums (and diagonal sums) into the workspace, reduced in fixed order
//   knn        : d2_ij = max(0, |x_i|^2 + |y_j|^2 - 2 dot); every row keeps the ascending list of its kk smallest d2
//   ball_count : count[i] += #{ j : d2_ij <= radius2[j] }
// The n x m matrix never exists: the workspace holds the squared norms, the tile partials and the partial lists, O(n + m + tiles).
// No floating-point atomics: the same call twice gives the same bits.  The int32 counters are added with integer atomics (any order
// gives the same sum).
#include "lg_internal.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int TILE = 64, KS = 32;
constexpr int LDA = KS + 2;             // [row][k] pitch in doubles, as fid_gemm_kernel's A tile
constexpr int SMEM_D = 2 * TILE * LDA;  // X tile + Y tile
constexpr int LDT = TILE + 1;           // pitch of the d2 tile that reuses the operand tiles after the k loop (64 * 65 <= SMEM_D)
constexpr int KMAX = 16;                // longest neighbour list
constexpr int GROUP = 16;               // tile rows per group of the block order (below)
constexpr int KNN_TARGET_BLOCKS = 512, KNN_MIN_TILES = 4;
static_assert(TILE * LDT <= SMEM_D, "the d2 tile must fit in the operand tiles");

// Block order of the tile grids: groups of GROUP tile rows, column-major inside a group, so the blocks in flight together share
// GROUP row slabs of X and about as many of Y instead of one slab of X and every slab of Y.
__device__ __forceinline__ void tile_of_block(long long bid, long long tn, long long tm, long long& ti, long long& tj) {
  const long long per = (long long)GROUP * tm, g = bid / per, first = g * GROUP;
  const long long gs = tn - first < GROUP ? tn - first : GROUP, rem = bid - g * per;
  ti = first + rem % gs;
  tj = rem / gs;
}

// acc = X[i0 .. i0 + 63][:] . Y[j0 .. j0 + 63][:]^T; wave (wr, wc) holds rows wr * 32 + a * 16 + (lane >> 4) + 4 * e, columns
// wc * 32 + b * 16 + (lane & 15) in acc[a][b][e].  Ends with every wave past its last LDS read only after the caller's next barrier.
__device__ __forceinline__ void pairs_tile_dot(const float* __restrict__ X, long long n, long long i0, const float* __restrict__ Y,
                                               long long m, long long j0, int D, double* sA, double* sB, f64x4 (&acc)[2][2]) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int l15 = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
  // staging: 64 rows x 32 k per operand, thread -> (row tid / 4, 8 consecutive k)
  const int ar = tid >> 2, ak = (tid & 3) * 8;
  const bool xin = i0 + ar < n, yin = j0 + ar < m;
  const float* xr = X + (xin ? (i0 + ar) * (long long)D : 0);
  const float* yr = Y + (yin ? (j0 + ar) * (long long)D : 0);
  const bool vec = (D & 3) == 0 && (((uintptr_t)X | (uintptr_t)Y) & 15) == 0;  // every row 16-byte aligned
  float ra[8], rb[8];
  auto fetch = [&](int k0) {
    const int k = k0 + ak;
    if (vec && k + 8 <= D) {
      float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, b0 = a0, b1 = a0;
      if (xin) {
        a0 = *reinterpret_cast<const float4*>(xr + k);
        a1 = *reinterpret_cast<const float4*>(xr + k + 4);
      }
      if (yin) {
        b0 = *reinterpret_cast<const float4*>(yr + k);
        b1 = *reinterpret_cast<const float4*>(yr + k + 4);
      }
      ra[0] = a0.x; ra[1] = a0.y; ra[2] = a0.z; ra[3] = a0.w; ra[4] = a1.x; ra[5] = a1.y; ra[6] = a1.z; ra[7] = a1.w;
      rb[0] = b0.x; rb[1] = b0.y; rb[2] = b0.z; rb[3] = b0.w; rb[4] = b1.x; rb[5] = b1.y; rb[6] = b1.z; rb[7] = b1.w;
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        ra[q] = (xin && k + q < D) ? xr[k + q] : 0.f;
        rb[q] = (yin && k + q < D) ? yr[k + q] : 0.f;
      }
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < D; k0 += KS) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      sA[ar * LDA + ak + q] = (double)ra[q];
      sB[ar * LDA + ak + q] = (double)rb[q];
    }
    __syncthreads();
    if (k0 + KS < D) fetch(k0 + KS);  // next slab's global loads fly under this slab's MFMAs
#pragma unroll
    for (int k4 = 0; k4 < KS; k4 += 4) {
      double af[2], bf[2];  // A[row = l15][k = lk] = x[i][k], B[k = lk][col = l15] = y[j][k]
#pragma unroll
      for (int a = 0; a < 2; ++a) af[a] = sA[(wr * 32 + a * 16 + l15) * LDA + k4 + lk];
#pragma unroll
      for (int b = 0; b < 2; ++b) bf[b] = sB[(wc * 32 + b * 16 + l15) * LDA + k4 + lk];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[a], bf[b], acc[a][b], 0, 0, 0);
    }
  }
}

// out[i] = |x_i|^2 in fp64: one wave per row, a fixed strided order and a fixed tree (depends on the row and D alone)
__global__ __launch_bounds__(256) void pairs_norm_kernel(const float* __restrict__ X, long long n, int D, double* __restrict__ out) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;  // uniform over the wave
  double s = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double v = (double)X[row * D + d];
    s += v * v;
  }
  s = lg_wave_sum_d(s);
  if (lane == 0) out[row] = s;
}

// ---- poly_sum ---------------------------------------------------------------------------------------------------------------
// part[2 * block] = sum of k_ij over the block's tile, part[2 * block + 1] = sum of its k_ii (diag; only tiles on the diagonal)
__global__ __launch_bounds__(256) void pairs_poly_kernel(const float* __restrict__ X, long long n, const float* __restrict__ Y,
                                                         long long m, int D, int degree, double gamma, double coef0, int diag,
                                                         long long tn, long long tm, double* __restrict__ part) {
  __shared__ double smem[SMEM_D];
  __shared__ double sred[32];
  long long ti, tj;
  tile_of_block(blockIdx.x, tn, tm, ti, tj);
  const long long i0 = ti * TILE, j0 = tj * TILE;
  f64x4 acc[2][2];
  pairs_tile_dot(X, n, i0, Y, m, j0, D, smem, smem + TILE * LDA, acc);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wr = wid >> 1, wc = wid & 1, l15 = lane & 15, lk = lane >> 4;
  double v[2] = {0.0, 0.0};
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long long i = i0 + wr * 32 + a * 16 + lk + 4 * e, j = j0 + wc * 32 + b * 16 + l15;
        if (i < n && j < m) {
          const double t = gamma * acc[a][b][e] + coef0;
          double k = t;
          for (int d = 1; d < degree; ++d) k *= t;
          v[0] += k;
          if (diag && i == j) v[1] += k;
        }
      }
  lg_block_sum_d<2>(v, sred);
  if (threadIdx.x == 0) {
    part[2 * (long long)blockIdx.x] = v[0];
    part[2 * (long long)blockIdx.x + 1] = v[1];
  }
}

// sums[0] += sum of the tile sums, sums[1] += sum of the diagonal sums: every thread a fixed strided subset, then a fixed tree
__global__ __launch_bounds__(256) void pairs_poly_reduce_kernel(const double* __restrict__ part, long long ntile, double* __restrict__ sums) {
  __shared__ double sred[32];
  double v[2] = {0.0, 0.0};
  for (long long t = threadIdx.x; t < ntile; t += 256) {
    v[0] += part[2 * t];
    v[1] += part[2 * t + 1];
  }
  lg_block_sum_d<2>(v, sred);
  if (threadIdx.x == 0) {
    sums[0] += v[0];
    sums[1] += v[1];
  }
}

// ---- knn --------------------------------------------------------------------------------------------------------------------
// A list is KMAX registers, ascending, its kk entries at the END: lst[KMAX - kk .. KMAX), in front of them -inf sentinels.  The
// threshold is then always lst[KMAX - 1] and an insertion moves down until it meets a smaller entry or a sentinel: every index is a
// compile-time constant whatever kk is, so the list stays in registers (an index that depends on kk sends it to scratch memory).
__device__ __forceinline__ void knn_insert(double (&lst)[KMAX], double v) {
  lst[KMAX - 1] = v;
#pragma unroll
  for (int p = KMAX - 1; p >= 1; --p)
    if (lst[p] < lst[p - 1]) {
      const double t = lst[p];
      lst[p] = lst[p - 1];
      lst[p - 1] = t;
    }
}

// Block (rb, s) owns rows rb * 64 .. and walks column tiles s * tps .. (s + 1) * tps of the ct tiles of Y; its lists (from +inf) go to
// part[block][row in block][KMAX], the kk entries at the end as in the registers.  A list is the multiset of the smallest values: it
// does not depend on the order of insertion, hence not on the split.
__global__ __launch_bounds__(256) void pairs_knn_kernel(const float* __restrict__ X, long long n, const float* __restrict__ Y,
                                                        long long m, int D, int kk, const double* __restrict__ xn,
                                                        const double* __restrict__ yn, int S, long long tps, long long ct,
                                                        double* __restrict__ part) {
  __shared__ double smem[SMEM_D];
  __shared__ double slist[KMAX * TILE];
  __shared__ unsigned long long cand[TILE];
  const long long rb = blockIdx.x / S;
  const int s = blockIdx.x - (int)(rb * S);
  const long long i0 = rb * TILE;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1, l15 = lane & 15, lk = lane >> 4;
  // the lists wait in LDS ([entry][row]: conflict-free) between tiles, so no register is held for them under the MFMA loop
  if (tid < TILE) {
#pragma unroll
    for (int p = 0; p < KMAX; ++p) slist[p * TILE + tid] = p < KMAX - kk ? -HUGE_VAL : HUGE_VAL;
    cand[tid] = 0ull;
  }
  const long long t1 = (s + 1) * tps < ct ? (s + 1) * tps : ct;
  for (long long t = s * tps; t < t1; ++t) {
    const long long j0 = t * TILE;
    f64x4 acc[2][2];
    pairs_tile_dot(X, n, i0, Y, m, j0, D, smem, smem + TILE * LDA, acc);
    __syncthreads();  // the operand tiles are read out: reuse them for the d2 tile
    // every lane writes its d2 values and marks, in the row's 64-bit mask, the columns that lie below the row's present kk-th value:
    // after the first tiles few do, and the row's lane visits only those
    double nx[2][4], thr_r[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = wr * 32 + a * 16 + lk + 4 * e;
        nx[a][e] = i0 + r < n ? xn[i0 + r] : 0.0;
        thr_r[a][e] = slist[(KMAX - 1) * TILE + r];
      }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int c = wc * 32 + b * 16 + l15;
      const bool cin = j0 + c < m;
      const double ny = cin ? yn[j0 + c] : 0.0;
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = wr * 32 + a * 16 + lk + 4 * e;
          double d2 = (nx[a][e] + ny) - 2.0 * acc[a][b][e];
          d2 = d2 > 0.0 ? d2 : 0.0;
          smem[r * LDT + c] = d2;
          if (cin && d2 < thr_r[a][e]) atomicOr(&cand[r], 1ull << c);
        }
    }
    __syncthreads();
    if (tid < TILE) {  // one lane per row
      unsigned long long todo = cand[tid];
      cand[tid] = 0ull;
      if (todo && i0 + tid < n) {
        double lst[KMAX];
#pragma unroll
        for (int p = 0; p < KMAX; ++p) lst[p] = slist[p * TILE + tid];
        while (todo) {
          const int j = __ffsll(todo) - 1;
          todo &= todo - 1;
          const double v = smem[tid * LDT + j];
          if (v < lst[KMAX - 1]) knn_insert(lst, v);
        }
#pragma unroll
        for (int p = 0; p < KMAX; ++p) slist[p * TILE + tid] = lst[p];
      }
    }
    // the next tile's barriers (before its first LDS store, and again before this point) order these reads and the cleared masks
  }
  if (tid < TILE) {  // a row's list is written and read by its own lane alone
    double* o = part + ((long long)blockIdx.x * TILE + tid) * KMAX;
#pragma unroll
    for (int p = 0; p < KMAX; ++p) o[p] = slist[p * TILE + tid];
  }
}

// best[i][0 .. kk) (ascending) <- the kk smallest of itself and the S partial lists of row i
__global__ __launch_bounds__(256) void pairs_knn_merge_kernel(const double* __restrict__ part, long long n, int kk, int S,
                                                              double* __restrict__ best) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int off = KMAX - kk;
  double lst[KMAX];
#pragma unroll
  for (int p = 0; p < KMAX; ++p) lst[p] = p >= off ? best[i * kk + (p - off)] : -HUGE_VAL;
  const long long rb = i / TILE;
  const int r = (int)(i - rb * TILE);
  for (int s = 0; s < S; ++s) {
    const double* src = part + ((rb * S + s) * TILE + r) * KMAX + off;
    for (int p = 0; p < kk; ++p) {
      const double v = src[p];
      if (!(v < lst[KMAX - 1])) break;  // ascending: nothing further in this list enters
      knn_insert(lst, v);
    }
  }
#pragma unroll
  for (int p = 0; p < KMAX; ++p)
    if (p >= off) best[i * kk + (p - off)] = lst[p];
}

// ---- ball_count -------------------------------------------------------------------------------------------------------------
// count[i] += #{ j in the block's tile : d2(q_i, ref_j) <= radius2[j] }: per-row counts of the tile gathered in LDS, one integer
// atomic per row and tile
__global__ __launch_bounds__(256) void pairs_ball_kernel(const float* __restrict__ Q, long long n, const float* __restrict__ R,
                                                         long long m, int D, const double* __restrict__ qn,
                                                         const double* __restrict__ rn, const double* __restrict__ radius2,
                                                         long long tn, long long tm, int* __restrict__ count) {
  __shared__ double smem[SMEM_D];
  __shared__ int cnt[TILE];
  long long ti, tj;
  tile_of_block(blockIdx.x, tn, tm, ti, tj);
  const long long i0 = ti * TILE, j0 = tj * TILE;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1, l15 = lane & 15, lk = lane >> 4;
  if (tid < TILE) cnt[tid] = 0;
  f64x4 acc[2][2];
  pairs_tile_dot(Q, n, i0, R, m, j0, D, smem, smem + TILE * LDA, acc);  // its barriers order the zeroing before the adds below
  double ny[2], r2[2];
  bool jin[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const long long j = j0 + wc * 32 + b * 16 + l15;
    jin[b] = j < m;
    ny[b] = jin[b] ? rn[j] : 0.0;
    r2[b] = jin[b] ? radius2[j] : 0.0;
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = wr * 32 + a * 16 + lk + 4 * e;
      const long long i = i0 + r;
      const double nx = i < n ? qn[i] : 0.0;
      int c = 0;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        double d2 = (nx + ny[b]) - 2.0 * acc[a][b][e];
        d2 = d2 > 0.0 ? d2 : 0.0;
        c += (i < n && jin[b] && d2 <= r2[b]) ? 1 : 0;
      }
      // the 16 lanes of a row (same lane >> 4) are neighbours
      c += __shfl_xor(c, 1);
      c += __shfl_xor(c, 2);
      c += __shfl_xor(c, 4);
      c += __shfl_xor(c, 8);
      if (l15 == 0 && c) atomicAdd(&cnt[r], c);
    }
  __syncthreads();
  if (tid < TILE && i0 + tid < n && cnt[tid]) atomicAdd(&count[i0 + tid], cnt[tid]);
}

inline long long tiles_of(long long r) { return (r + TILE - 1) / TILE; }

// column split of the knn pass: enough blocks to fill the device when there are few row blocks, at least KNN_MIN_TILES tiles each
inline int knn_split(long long n, long long m) {
  const long long rb = tiles_of(n), ct = tiles_of(m);
  long long s = KNN_TARGET_BLOCKS / rb, cap = (ct + KNN_MIN_TILES - 1) / KNN_MIN_TILES;
  if (s > cap) s = cap;
  return (int)(s < 1 ? 1 : s);
}

constexpr long long MAX_BLOCKS = 1LL << 30;

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

int launch_norms(hipStream_t st, const float* x, long long n, int D, double* out, const char* what) {
  hipLaunchKernelGGL(pairs_norm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, x, n, D, out);
  LG_CHECK_LAUNCH(what);
  return LG_OK;
}

}  // namespace

// norms of both sets, then the larger of the tile partials (poly_sum) and the partial lists (knn)
extern "C" size_t lg_pairs_workspace_bytes(long long n, long long m, int D) {
  if (n < 1 || m < 1 || D < 1) return 0;
  const size_t poly = 2 * (size_t)tiles_of(n) * (size_t)tiles_of(m) * sizeof(double);
  const size_t knn = (size_t)tiles_of(n) * (size_t)knn_split(n, m) * TILE * KMAX * sizeof(double);
  return align256((size_t)n * sizeof(double)) + align256((size_t)m * sizeof(double)) + (poly > knn ? poly : knn);
}

#define PAIRS_CHECK_SHAPE(name, n, m, D)                                                                              \
  LG_CHECK_ARG((n) >= 1 && (m) >= 1 && (D) >= 1 && (D) <= (1 << 16), name ": bad shape n=%lld m=%lld D=%d", n, m, D); \
  LG_CHECK_ARG(tiles_of(n) * tiles_of(m) <= MAX_BLOCKS && (n) <= 4 * MAX_BLOCKS && (m) <= 4 * MAX_BLOCKS,            \
               name ": bad shape n=%lld m=%lld: too many tiles for one call, feed the sets in row blocks", n, m)

extern "C" int lg_pairs_poly_sum(const float* x, long long n, const float* y, long long m, int D, int degree,
                                 const double* gamma_coef0, int diag, double* sums, void* workspace, size_t ws_bytes, void* stream) {
  LG_CHECK_ARG(x && y && gamma_coef0 && sums && workspace, "lg_pairs_poly_sum: null pointer");
  PAIRS_CHECK_SHAPE("lg_pairs_poly_sum", n, m, D);
  LG_CHECK_ARG(degree >= 1 && degree <= 8, "lg_pairs_poly_sum: bad degree %d (1..8)", degree);
  LG_CHECK_ARG(!diag || n == m, "lg_pairs_poly_sum: diag needs n == m, got n=%lld m=%lld", n, m);
  LG_CHECK_ARG(ws_bytes >= lg_pairs_workspace_bytes(n, m, D), "lg_pairs_poly_sum: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const long long tn = tiles_of(n), tm = tiles_of(m);
  double* part = (double*)((char*)workspace + align256((size_t)n * sizeof(double)) + align256((size_t)m * sizeof(double)));
  hipLaunchKernelGGL(pairs_poly_kernel, dim3((unsigned)(tn * tm)), dim3(256), 0, st, x, n, y, m, D, degree, gamma_coef0[0],
                     gamma_coef0[1], diag ? 1 : 0, tn, tm, part);
  LG_CHECK_LAUNCH("lg_pairs_poly_sum(tiles)");
  hipLaunchKernelGGL(pairs_poly_reduce_kernel, dim3(1), dim3(256), 0, st, (const double*)part, tn * tm, sums);
  LG_CHECK_LAUNCH("lg_pairs_poly_sum(reduce)");
  return LG_OK;
}

extern "C" int lg_pairs_knn(const float* x, long long n, const float* y, long long m, int D, int kk, double* best, void* workspace,
                            size_t ws_bytes, void* stream) {
  LG_CHECK_ARG(x && y && best && workspace, "lg_pairs_knn: null pointer");
  PAIRS_CHECK_SHAPE("lg_pairs_knn", n, m, D);
  LG_CHECK_ARG(kk >= 1 && kk <= KMAX, "lg_pairs_knn: bad kk %d (1..%d)", kk, KMAX);
  LG_CHECK_ARG(ws_bytes >= lg_pairs_workspace_bytes(n, m, D), "lg_pairs_knn: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  double* xn = (double*)workspace;
  double* yn = (double*)((char*)workspace + align256((size_t)n * sizeof(double)));
  double* part = (double*)((char*)yn + align256((size_t)m * sizeof(double)));
  int rc;
  if ((rc = launch_norms(st, x, n, D, xn, "lg_pairs_knn(norms x)")) != LG_OK) return rc;
  if ((rc = launch_norms(st, y, m, D, yn, "lg_pairs_knn(norms y)")) != LG_OK) return rc;
  const long long rb = tiles_of(n), ct = tiles_of(m);
  const int S = knn_split(n, m);
  const long long tps = (ct + S - 1) / S;
  hipLaunchKernelGGL(pairs_knn_kernel, dim3((unsigned)(rb * S)), dim3(256), 0, st, x, n, y, m, D, kk, (const double*)xn,
                     (const double*)yn, S, tps, ct, part);
  LG_CHECK_LAUNCH("lg_pairs_knn(tiles)");
  hipLaunchKernelGGL(pairs_knn_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double*)part, n, kk, S, best);
  LG_CHECK_LAUNCH("lg_pairs_knn(merge)");
  return LG_OK;
}

extern "C" int lg_pairs_ball_count(const float* q, long long n, const float* ref, long long m, const double* radius2, int D,
                                   int* count, void* workspace, size_t ws_bytes, void* stream) {
  LG_CHECK_ARG(q && ref && radius2 && count && workspace, "lg_pairs_ball_count: null pointer");
  PAIRS_CHECK_SHAPE("lg_pairs_ball_count", n, m, D);
  LG_CHECK_ARG(ws_bytes >= lg_pairs_workspace_bytes(n, m, D), "lg_pairs_ball_count: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  double* qn = (double*)workspace;
  double* rn = (double*)((char*)workspace + align256((size_t)n * sizeof(double)));
  int rc;
  if ((rc = launch_norms(st, q, n, D, qn, "lg_pairs_ball_count(norms q)")) != LG_OK) return rc;
  if ((rc = launch_norms(st, ref, m, D, rn, "lg_pairs_ball_count(norms ref)")) != LG_OK) return rc;
  const long long tn = tiles_of(n), tm = tiles_of(m);
  hipLaunchKernelGGL(pairs_ball_kernel, dim3((unsigned)(tn * tm)), dim3(256), 0, st, q, n, ref, m, D, (const double*)qn,
                     (const double*)rn, radius2, tn, tm, count);
  LG_CHECK_LAUNCH("lg_pairs_ball_count(tiles)");
  return LG_OK;
}
