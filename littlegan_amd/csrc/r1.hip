// R1 gradient penalty of the discriminator (r1_gamma / r1_interval; Mescheder et al. 2018, applied lazily as in Karras et al. 2020; the
// reference has none — this project's definition):
//   x_b = row b of what D reads as its real batch,   l_b = <w_pr, h4(x_b)> + b_pr (the PRE-sigmoid value of output_pr),
//   g_b = dl_b / dx_b,   r2_b = |g_b|_2^2,   r1 = (w / 2) mean_b r2_b with w = r1_gamma r1_interval,   disc_loss += r1 on penalty steps.
// Its weight gradient is the reverse-over-reverse pass of the gradient penalty (gp.hip) with the sigmoid taken out; the
// norm backward with an injected adjoint, its double backward, the convolutions and the weight gradients are that pass's.  Here are the
// three parts that differ: the top seed (every row is w_pr: no p (1 - p) factor), the seed on the image gradient (u0 = (w / B) g does not
// depend on the sums, so ONE pass over g writes u0 and the partials) and the heads' weight gradient (l is bilinear in (w_pr, h4): the
// second-order scalar is zero, dw_pr is a column sum and b_pr gets nothing).
// Every reduction has ONE order that the shape alone decides: fp64 partials over chunks / slabs whose boundaries depend on (B, L) or
// (B, K), merged in index order.  The grids come from the CU budget (lg_grid_cus), the partial layout does not: blocks walk the items
// with a stride, and an item's partial is the same whichever block computes it.  No atomics.
// lgrel_r12_seed (R1 + R2 in one pass over a 2B-row batch, DESIGN.md §27, include/littlegan_rel.h) is the seed with a weight per half:
// the same pass kernel with the scale selected per row, the same final sums once per half.
#include "lg_internal.h"
#include "../../include/littlegan_hip_reg.h"
#include "../../include/littlegan_rel.h"

namespace {

constexpr int CHUNK = 4096;  // elements of a row per partial: 256 threads x 4 float4
constexpr int SLAB = 32;     // rows per partial of the column sum

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

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

// g[b][k] = wpr[k], as 32-bit words: a NaN or a -0.0 of wpr arrives with its bits
template <bool V4>
__global__ __launch_bounds__(256) void r1_heads_seed_kernel(const unsigned* __restrict__ wpr, unsigned* __restrict__ g, unsigned K,
                                                            unsigned total) {
  // V4: K and total count 16-byte words
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const unsigned k = i % K;
    if (V4) reinterpret_cast<u32x4*>(g)[i] = reinterpret_cast<const u32x4*>(wpr)[k];
    else g[i] = wpr[k];
  }
}

// item = (row b, chunk j): u0 = scale g over the chunk, part[b][j] = sum of g^2 over it (products and sum in fp64: exact products).
// Rows from `split` on take scale_hi (lgrel_r12_seed: the fake half of a 2B-row batch); lgr_r1_seed passes split = its row count.
__global__ __launch_bounds__(256) void r1_seed_kernel(const float* __restrict__ g, float* __restrict__ u0, double* __restrict__ part,
                                                      float scale_lo, float scale_hi, long long split, long long L, int nch,
                                                      long long items) {
  __shared__ double sred[16];
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const long long b = it / nch;
    const float scale = b < split ? scale_lo : scale_hi;
    const long long c0 = (it - b * nch) * CHUNK;
    const float* gs = g + b * L;
    float* us = u0 + b * L;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < CHUNK / 1024; ++k) {
      const long long e = c0 + (long long)(k * 256 + (int)threadIdx.x) * 4;
      if (e < L) {
        const f32x4 v = ld4(gs + e);
        st4(us + e, f32x4{scale * v[0], scale * v[1], scale * v[2], scale * v[3]});
        s += ((double)v[0] * (double)v[0] + (double)v[1] * (double)v[1]) + ((double)v[2] * (double)v[2] + (double)v[3] * (double)v[3]);
      }
    }
    double red[1] = {s};
    lg_block_sum_d<1>(red, sred);
    if (threadIdx.x == 0) part[it] = red[0];
  }
}

// r2[b] = the row's partials in chunk order over B rows; returns term = (w / 2) mean_b r2, valid in thread 0
__device__ __forceinline__ float seed_final_term(const double* __restrict__ part, int nch, int B, float w, float* __restrict__ r2,
                                                 double* sh) {
  double acc = 0.0;
  for (int n = threadIdx.x; n < B; n += 256) {
    double s = 0.0;
    for (int j = 0; j < nch; ++j) s += part[(long long)n * nch + j];
    r2[n] = (float)s;
    acc += s;
  }
  const double tot = block_tree_sum(acc, sh);
  return (float)(0.5 * (double)w * tot / (double)B);
}

// loss (+)= term, r1_loss = term
__global__ __launch_bounds__(256) void r1_seed_final_kernel(const double* __restrict__ part, int nch, int B, float w,
                                                            float* __restrict__ r2, float* __restrict__ loss,
                                                            float* __restrict__ r1_loss) {
  __shared__ double sh[256];
  const float term = seed_final_term(part, nch, B, w, r2, sh);
  if (threadIdx.x == 0) {
    if (loss) loss[0] = loss[0] + term;
    if (r1_loss) r1_loss[0] = term;
  }
}

// the two halves of a 2B-row batch, each as r1_seed_final_kernel takes its B rows: loss = (loss + term_real) + term_fake
__global__ __launch_bounds__(256) void r12_seed_final_kernel(const double* __restrict__ part, int nch, int B, float w_real, float w_fake,
                                                             float* __restrict__ r2, float* __restrict__ loss,
                                                             float* __restrict__ r1_loss, float* __restrict__ r2_loss) {
  __shared__ double sh[256];
  const float t_real = seed_final_term(part, nch, B, w_real, r2, sh);
  __syncthreads();   // thread 0 has read sh[0] before the second tree writes it
  const float t_fake = seed_final_term(part + (long long)B * nch, nch, B, w_fake, r2 + B, sh);
  if (threadIdx.x == 0) {
    if (loss) loss[0] = (loss[0] + t_real) + t_fake;
    if (r1_loss) r1_loss[0] = t_real;
    if (r2_loss) r2_loss[0] = t_fake;
  }
}

// item = (slab s, block of 256 columns): part[s][k] = sum of u[b][k] over the slab's rows, in row order
__global__ __launch_bounds__(256) void r1_colsum_part_kernel(const float* __restrict__ u, double* __restrict__ part, int B, int K, int ncb,
                                                             int items) {
  for (int it = blockIdx.x; it < items; it += gridDim.x) {
    const int sl = it / ncb;
    const int k = (it - sl * ncb) * 256 + (int)threadIdx.x;
    if (k >= K) continue;
    const int n0 = sl * SLAB, n1 = (n0 + SLAB < B) ? n0 + SLAB : B;
    double acc = 0.0;
#pragma unroll 8
    for (int n = n0; n < n1; ++n) acc += (double)u[(long long)n * K + k];
    part[(long long)sl * K + k] = acc;
  }
}

// dwpr[k] += the column's partials in slab order, rounded to fp32 once
__global__ __launch_bounds__(256) void r1_colsum_final_kernel(const double* __restrict__ part, float* __restrict__ dwpr, int nslab, int K) {
  for (int k = blockIdx.x * 256 + (int)threadIdx.x; k < K; k += gridDim.x * 256) {
    double acc = 0.0;
    for (int s = 0; s < nslab; ++s) acc += part[(long long)s * K + k];
    dwpr[k] = dwpr[k] + (float)acc;
  }
}

// resident blocks of a 256-thread kernel (occupancy query once per kernel) over the CUs the persistent kernels may fill
#define R1_RESIDENT(kern)                                                                                              \
  ([]() -> long long {                                                                                                 \
    static int per_cu = 0;                                                                                             \
    if (!per_cu && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, 0) != hipSuccess || per_cu < 1)) \
      per_cu = 4;                                                                                                      \
    return (long long)per_cu * lg_grid_cus();                                                                          \
  }())

// the blocks the work needs, at most one round of residency (blocks then stride over the items)
inline int grid_of(long long items, long long resident) {
  const long long nb = items < resident ? items : resident;
  return (int)(nb < 1 ? 1 : nb);
}
inline long long nchunks(long long L) { return (L + CHUNK - 1) / CHUNK; }
inline int nslabs(int B) { return (B + SLAB - 1) / SLAB; }
inline size_t al(size_t n) { return (n + 255) / 256 * 256; }
inline bool aligned16(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }
inline bool heads_shape_ok(int B, int K) { return B > 0 && K > 0 && (long long)B * K < (1LL << 31); }

}  // namespace

extern "C" size_t lgr_r1_workspace_bytes(int B, long long L) {
  if (B <= 0 || L <= 0) return 0;
  return al((size_t)B * (size_t)nchunks(L) * sizeof(double));
}

extern "C" size_t lgr_r1_colsum_workspace_bytes(int B, int K) {
  if (B <= 0 || K <= 0) return 0;
  return al((size_t)nslabs(B) * (size_t)K * sizeof(double));
}

extern "C" int lgr_r1_heads_seed(const float* wpr, float* g, int B, int K, void* stream) {
  LG_CHECK_ARG(wpr && g, "lgr_r1_heads_seed: null pointer");
  LG_CHECK_ARG((((uintptr_t)wpr | (uintptr_t)g) & 3) == 0, "lgr_r1_heads_seed: wpr and g must be 4-byte aligned");
  LG_CHECK_ARG(heads_shape_ok(B, K), "lgr_r1_heads_seed: bad shape B=%d K=%d", B, K);
  const long long tot = (long long)B * K;
  if (K % 4 == 0 && aligned16(wpr, g)) {
    lg_note_kernel("r1_heads_seed_kernel<v4>");
    hipLaunchKernelGGL(r1_heads_seed_kernel<true>, dim3(grid_of((tot / 4 + 255) / 256, R1_RESIDENT(r1_heads_seed_kernel<true>))),
                       dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const unsigned*>(wpr), reinterpret_cast<unsigned*>(g),
                       (unsigned)(K / 4), (unsigned)(tot / 4));
  } else {
    lg_note_kernel("r1_heads_seed_kernel<v1>");
    hipLaunchKernelGGL(r1_heads_seed_kernel<false>, dim3(grid_of((tot + 255) / 256, R1_RESIDENT(r1_heads_seed_kernel<false>))),
                       dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const unsigned*>(wpr), reinterpret_cast<unsigned*>(g),
                       (unsigned)K, (unsigned)tot);
  }
  LG_CHECK_LAUNCH("lgr_r1_heads_seed");
  return LG_OK;
}

extern "C" int lgr_r1_seed(const float* g, float* u0, float* r2, float* loss, float* r1_loss, float weight, void* workspace,
                           size_t ws_bytes, int B, long long L, void* stream) {
  LG_CHECK_ARG(g && u0 && r2 && workspace, "lgr_r1_seed: null pointer");
  LG_CHECK_ARG(aligned16(g, u0) && ((uintptr_t)workspace & 7) == 0, "lgr_r1_seed: g and u0 must be 16-byte, workspace 8-byte aligned");
  LG_CHECK_ARG(B > 0 && L > 0 && L % 4 == 0 && L / 4 < (1LL << 31) && (long long)B * (L / 4) < (1LL << 31),
               "lgr_r1_seed: bad shape B=%d L=%lld (L %% 4 == 0, B * L / 4 < 2^31)", B, L);
  LG_CHECK_ARG(weight >= 0.f && weight <= 3.402823466e38f, "lgr_r1_seed: weight %g must be finite and >= 0", (double)weight);
  LG_CHECK_ARG(ws_bytes >= lgr_r1_workspace_bytes(B, L), "lgr_r1_seed: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  const int nch = (int)nchunks(L);
  const long long items = (long long)B * nch;
  lg_note_kernel("r1_seed_kernel");
  hipLaunchKernelGGL(r1_seed_kernel, dim3(grid_of(items, R1_RESIDENT(r1_seed_kernel))), dim3(256), 0, st, g, u0, part,
                     weight / (float)B, 0.f, (long long)B, L, nch, items);
  LG_CHECK_LAUNCH("lgr_r1_seed(pass)");
  hipLaunchKernelGGL(r1_seed_final_kernel, dim3(1), dim3(256), 0, st, (const double*)part, nch, B, weight, r2, loss, r1_loss);
  LG_CHECK_LAUNCH("lgr_r1_seed(final)");
  return LG_OK;
}

extern "C" size_t lgrel_r12_workspace_bytes(int B, long long L) {
  if (B <= 0 || L <= 0) return 0;
  return al(2 * (size_t)B * (size_t)nchunks(L) * sizeof(double));
}

// lgr_r1_seed over g[2B][L] with a weight per half: the same pass kernel (the scale selected per row) and the same per-half final sums,
// so the bits are those of two lgr_r1_seed calls on the halves
extern "C" int lgrel_r12_seed(const float* g, float* u0, float* r2, float* loss, float* r1_loss, float* r2_loss, float w_real, float w_fake,
                              void* workspace, size_t ws_bytes, int B, long long L, void* stream) {
  LG_CHECK_ARG(g && u0 && r2 && workspace, "lgrel_r12_seed: null pointer");
  LG_CHECK_ARG(aligned16(g, u0) && ((uintptr_t)workspace & 7) == 0, "lgrel_r12_seed: g and u0 must be 16-byte, workspace 8-byte aligned");
  LG_CHECK_ARG((((uintptr_t)r2 | (uintptr_t)loss | (uintptr_t)r1_loss | (uintptr_t)r2_loss) & 3) == 0,
               "lgrel_r12_seed: r2, loss, r1_loss and r2_loss must be 4-byte aligned");
  LG_CHECK_ARG(B > 0 && L > 0 && L % 4 == 0 && L / 4 < (1LL << 31) && 2 * (long long)B * (L / 4) < (1LL << 31),
               "lgrel_r12_seed: bad shape B=%d L=%lld (g is [2B][L]; L %% 4 == 0, 2 B * L / 4 < 2^31)", B, L);
  LG_CHECK_ARG(w_real >= 0.f && w_real <= 3.402823466e38f && w_fake >= 0.f && w_fake <= 3.402823466e38f,
               "lgrel_r12_seed: weights w_real=%g w_fake=%g must be finite and >= 0", (double)w_real, (double)w_fake);
  LG_CHECK_ARG(ws_bytes >= lgrel_r12_workspace_bytes(B, L), "lgrel_r12_seed: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  const int nch = (int)nchunks(L);
  const long long items = 2 * (long long)B * nch;
  lg_note_kernel("r1_seed_kernel");
  hipLaunchKernelGGL(r1_seed_kernel, dim3(grid_of(items, R1_RESIDENT(r1_seed_kernel))), dim3(256), 0, st, g, u0, part,
                     w_real / (float)B, w_fake / (float)B, (long long)B, L, nch, items);
  LG_CHECK_LAUNCH("lgrel_r12_seed(pass)");
  lg_note_kernel("r12_seed_final_kernel");
  hipLaunchKernelGGL(r12_seed_final_kernel, dim3(1), dim3(256), 0, st, (const double*)part, nch, B, w_real, w_fake, r2, loss, r1_loss,
                     r2_loss);
  LG_CHECK_LAUNCH("lgrel_r12_seed(final)");
  return LG_OK;
}

extern "C" int lgr_r1_heads_colsum(const float* u, float* dwpr, void* workspace, size_t ws_bytes, int B, int K, void* stream) {
  LG_CHECK_ARG(u && dwpr && workspace, "lgr_r1_heads_colsum: null pointer");
  LG_CHECK_ARG((((uintptr_t)u | (uintptr_t)dwpr) & 3) == 0 && ((uintptr_t)workspace & 7) == 0,
               "lgr_r1_heads_colsum: u and dwpr must be 4-byte, workspace 8-byte aligned");
  LG_CHECK_ARG(heads_shape_ok(B, K), "lgr_r1_heads_colsum: bad shape B=%d K=%d", B, K);
  LG_CHECK_ARG(ws_bytes >= lgr_r1_colsum_workspace_bytes(B, K), "lgr_r1_heads_colsum: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  const int ncb = (K + 255) / 256, nslab = nslabs(B);
  const long long items = (long long)nslab * ncb;   // <= (B / 32 + 1)(K / 256 + 1) < 2^31 with B * K < 2^31
  lg_note_kernel("r1_colsum_kernel");
  hipLaunchKernelGGL(r1_colsum_part_kernel, dim3(grid_of(items, R1_RESIDENT(r1_colsum_part_kernel))), dim3(256), 0, st, u, part, B, K, ncb,
                     (int)items);
  LG_CHECK_LAUNCH("lgr_r1_heads_colsum(slabs)");
  hipLaunchKernelGGL(r1_colsum_final_kernel, dim3(grid_of(ncb, R1_RESIDENT(r1_colsum_final_kernel))), dim3(256), 0, st,
                     (const double*)part, dwpr, nslab, K);
  LG_CHECK_LAUNCH("lgr_r1_heads_colsum(merge)");
  return LG_OK;
}
