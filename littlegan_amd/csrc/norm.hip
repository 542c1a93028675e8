// InstanceNormalization(axis=None, eps=1e-3) of /root/reference/instance.py:105-128 as used at
// model.py:16,41,84,121: per-SAMPLE moments over all of (H,W,C), scalar gamma/beta, eps added to the
// std.  Because gamma/beta are scalars the whole op is a per-sample affine y = a_n*(x - mu_n) + beta with
// a_n = gamma/(sigma_n+eps); LeakyReLU(0.3) (model.py:24,50,100,130) and the decoder's skip add
// (model.py:46-47) are fused into the same elementwise pass.
//   stats : two-level reduction, block-local mean / M2 merged with Chan's formula, everything accumulated
//           in fp64 in a fixed order -> deterministic, no atomics.
//           stats[n][8] = {mu_hi, sigma, a, beta, mu_lo, 0, 0, 0}   (mu = mu_hi + mu_lo, float-float)
//   apply : y = [leaky]( a*(([leaky](x) - mu_hi) - mu_lo) + beta ) [+ skip]
//   bwd   : dx = a*(dz - m1 - c*m2'), c = x-mu, m1 = mean(dz), m2' = mean(dz*c)/((sigma+eps)*sigma);
//           dgamma = sum dz*c/(sigma+eps), dbeta = sum dz.
// Why fp64 sums and float-float means: mu, m1 and m2' are subtracted from EVERY element of a sample, so their
// rounding error is coherent; the later reductions of the step (bias / weight gradients = sums over up to
// 10^6 pixels of quantities whose mean was removed here) amplify a coherent 1e-7 error to 1e-3.
// All kernels are HBM-bound: 16-B vector loads, one pass over x for the moments (values kept in registers).
// The encoder's live dropout (dropout_train) rides on the same passes: dropped twins of apply / bwd regenerate the mask from a
// Philox counter in registers (DropK below); the mask-free kernels are the DROP = false instances of the shared bodies.
#include <stdio.h>
#include "lg_internal.h"
#include "philox.h"

namespace {

constexpr int CHUNK = 4096;  // elements per block in the reduction passes (256 threads x 4 float4)
constexpr int EW_UNR = 4;    // float4 per thread per trip of the elementwise passes

// partial[n][chunk] = {count, mean, M2} (doubles)
__global__ __launch_bounds__(256) void stats_partial_kernel(const float* __restrict__ x, double* __restrict__ partial,
                                                            long long L, int nchunk, int pre_leaky, float alpha,
                                                            __bf16* __restrict__ x16out) {
  const int n = blockIdx.y, ch = blockIdx.x;
  const long long base = (long long)n * L + (long long)ch * CHUNK;
  const long long lim = L - (long long)ch * CHUNK;  // valid elements in this chunk
  __shared__ double sred[32];
  f32x4 v[4];
  double s = 0.0;
  int cnt = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = (q * 256 + threadIdx.x) * 4;
    v[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (e < lim) {
      v[q] = *reinterpret_cast<const f32x4*>(x + base + e);
      if (x16out) {  // bf16 activation path: the bf16 copy of the raw conv output is made in this same pass
        bf16x4 w;
        w[0] = (__bf16)v[q][0]; w[1] = (__bf16)v[q][1]; w[2] = (__bf16)v[q][2]; w[3] = (__bf16)v[q][3];
        *reinterpret_cast<bf16x4*>(x16out + base + e) = w;
      }
      if (pre_leaky) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[q][k] = lg_leaky(v[q][k], alpha);
      }
      s += ((double)v[q][0] + (double)v[q][1]) + ((double)v[q][2] + (double)v[q][3]);
      cnt += 4;
    }
  }
  double red[2] = {s, (double)cnt};
  lg_block_sum_d<2>(red, sred);
  __shared__ double s_mean;
  if (threadIdx.x == 0) s_mean = red[0] / red[1];
  __syncthreads();
  const double mean = s_mean;
  double m2 = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = (q * 256 + threadIdx.x) * 4;
    if (e < lim) {
#pragma unroll
      for (int k = 0; k < 4; ++k) { const double d = (double)v[q][k] - mean; m2 += d * d; }
    }
  }
  double red2[1] = {m2};
  lg_block_sum_d<1>(red2, sred);
  if (threadIdx.x == 0) {
    double* o = partial + ((long long)n * nchunk + ch) * 3;
    o[0] = red[1]; o[1] = mean; o[2] = red2[0];
  }
}

// one wave per sample: Chan merge of the chunk partials in fp64
__global__ __launch_bounds__(64) void stats_final_kernel(const double* __restrict__ partial, float* __restrict__ stats,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         int nchunk) {
  const int n = blockIdx.x, lane = threadIdx.x;
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
    float* o = stats + (long long)n * LG_NSTAT;
    const float mu_hi = (float)mean;
    o[0] = mu_hi; o[1] = (float)sigma; o[2] = (float)a; o[3] = beta[0];
    o[4] = (float)(mean - (double)mu_hi); o[5] = 0.f; o[6] = 0.f; o[7] = 0.f;
  }
}

// Non-temporal LOADS in the element-wise passes (apply and backward apply), bf16 and fp32 path alike; their stores are plain.
// z, g and the skip map are dead behind these passes (z is read again only a whole tape later): loaded non-temporally they stop evicting
// what the neighbouring conv kernels live on (their sources and weights in L2 / the Infinity Cache).  Round 4, whole step on one box,
// variant builds, two rounds: 11.15 / 11.17 ms (0) -> 11.06 / 11.07 (1) -> 10.98 / 10.97 (5) = -1.6 %; the stores (3, 7: 11.07 / 10.98) add
// nothing there — although the passes in isolation (scripts/bench_norm.py) show the opposite: stores -9 .. -13 %, loads nothing.
// The same treatment of the final layer's input rows, the final weight gradient's activation operand and up_p16's source (their
// last readers) moved the step by nothing (10.79 - 10.86 against 10.81 - 10.90 ms): removed.
// (variants there: 0 none, 1 backward-apply loads, 5 + apply loads, 3 / 7 + the stores)
constexpr bool NT_LOAD = true;
// The bf16 apply / backward-apply passes (apply16p, bwd_apply16; not their fp32 twins) walk their maps from the END.  Their producers (the conv
// kernels) write a map front to back and their consumers read it front to back: a pass in between that starts at the END meets what the
// producer wrote last — still in the Infinity Cache when the map is larger than it — and leaves the START of its own output for the
// consumer's first reads.  Round 4, whole step, one box, three rounds: 10.79 / 10.76 / 10.72 ms (0) against 10.75 / 10.66 / 10.64 (3),
// captured 10.70 against 10.66; results unchanged except the bias column sums of a multi-trip backward pass (trip order).
template <bool NT, typename V>
__device__ __forceinline__ V lg_ld(const V* q) { if constexpr (NT) return __builtin_nontemporal_load(q); else return *q; }

// ---- encoder dropout (dropout_train): h = LeakyReLU(InstanceNorm(z)) * keep * scale, the mask REGENERATED in registers
// by every pass that needs it (forward apply, both passes of the backward) from a counter — nothing is stored.  Element e of sample row r
// (absolute row of the encoder call's batch, L elements per sample, NHWC) takes 16 bits of Philox block
//   offset = key_offset + (call << 34) + ((level-1) << 32) + r*(L/8) + e/8,  ctr = (lo32(offset), hi32(offset), 0, 0), key = seed:
//   w = (P[(e%8) >> 1] >> (16*(e&1))) & 0xFFFF,  keep = (w >= T),  T = round(rate * 65536),  scale = 65536 / (65536 - T)
// One block = 8 consecutive elements = one 16-byte bf16 access.  A launch covers whole rows of one tensor, so r*(L/8) + e/8 is the
// launch's first-row term (in `base`) plus the 8-element unit index within the launch's tensor: the mask cannot depend on the grid, the
// unroll, the operand path or the batch slice.  {seed, key_offset} are read from DEVICE memory (a step input: a captured graph replays
// with the masks of the step it is given).  The DROP = false instance of every body below is the mask-free kernel, unchanged.
struct DropK {
  const unsigned long long* key;  // device: {seed, key_offset}
  unsigned long long base;        // (call << 34) + ((level-1) << 32) + r0*(L/8)
  unsigned T;
  float scale;
};
// launch geometry, read in the KERNEL and handed to its body: there the compiler folds blockDim with the launch bounds
struct Geo { unsigned bdx, gdx, gdy; };
struct DropCtx { unsigned k0, k1; unsigned long long c0; unsigned T; float scale; };
template <bool DROP>
__device__ __forceinline__ DropCtx drop_begin(const DropK& dk) {
  DropCtx c{0u, 0u, 0ull, 0u, 1.f};
  if constexpr (DROP) {
    const unsigned long long seed = dk.key[0];
    c.k0 = (unsigned)seed; c.k1 = (unsigned)(seed >> 32);
    c.c0 = dk.key[1] + dk.base; c.T = dk.T; c.scale = dk.scale;
  }
  return c;
}
__device__ __forceinline__ float drop_mul(const DropCtx& c, unsigned w16) { return w16 >= c.T ? c.scale : 0.f; }
// keep*scale of the 8 elements of unit u8 (8-element unit index within the launch's tensor)
__device__ __forceinline__ void drop_mult8(const DropCtx& c, unsigned long long u8, float (&m)[8]) {
  const unsigned long long o = c.c0 + u8;
  const u4 p = philox4x32_10(u4{(unsigned)o, (unsigned)(o >> 32), 0u, 0u}, c.k0, c.k1);
  m[0] = drop_mul(c, p.x & 0xFFFFu); m[1] = drop_mul(c, p.x >> 16); m[2] = drop_mul(c, p.y & 0xFFFFu); m[3] = drop_mul(c, p.y >> 16);
  m[4] = drop_mul(c, p.z & 0xFFFFu); m[5] = drop_mul(c, p.z >> 16); m[6] = drop_mul(c, p.w & 0xFFFFu); m[7] = drop_mul(c, p.w >> 16);
}
// the same for the 4 elements of unit u4i of the fp32 passes (half a block)
__device__ __forceinline__ void drop_mult4(const DropCtx& c, unsigned long long u4i, float (&m)[4]) {
  const unsigned long long o = c.c0 + (u4i >> 1);
  const u4 p = philox4x32_10(u4{(unsigned)o, (unsigned)(o >> 32), 0u, 0u}, c.k0, c.k1);
  const unsigned w0 = (u4i & 1) ? p.z : p.x, w1 = (u4i & 1) ? p.w : p.y;
  m[0] = drop_mul(c, w0 & 0xFFFFu); m[1] = drop_mul(c, w0 >> 16); m[2] = drop_mul(c, w1 & 0xFFFFu); m[3] = drop_mul(c, w1 >> 16);
}

template <bool DROP>
__device__ __forceinline__ void apply_body(const float* __restrict__ x, const float* __restrict__ stats,
                                                    const float* __restrict__ skip, float* __restrict__ y,
                                                    __bf16* __restrict__ y16, long long L4, long long total4,
                                                    int pre_leaky, int post_leaky, float alpha, const DropK& dk, const Geo ge) {
  const DropCtx dc = drop_begin<DROP>(dk);
  // EW_UNR independent 16-B loads per thread per trip: a single load in flight per thread leaves the pass latency-bound
  // (measured 2.5-3.9 TB/s against 5.5+ for a streaming copy)
  const unsigned stride = ge.gdx * ge.bdx * EW_UNR, tot = (unsigned)total4, l4 = (unsigned)L4;
  const unsigned rb = blockIdx.x;
  const int ntrip = (int)(((unsigned long long)tot + stride - 1) / stride);
  for (int tr = 0; tr < ntrip; ++tr) {  // block-contiguous 16-KB trips
    const unsigned long long i0l = (unsigned long long)tr * stride + rb * ge.bdx * EW_UNR + threadIdx.x;
    if (i0l >= tot) continue;
    const unsigned i0 = (unsigned)i0l;
    f32x4 v[EW_UNR], sk[EW_UNR];
#pragma unroll
    for (int u = 0; u < EW_UNR; ++u) {
      const unsigned i = i0 + u * 256;
      if (i < tot) {
        v[u] = lg_ld<NT_LOAD>(reinterpret_cast<const f32x4*>(x + (long long)i * 4));
        if (skip) sk[u] = lg_ld<NT_LOAD>(reinterpret_cast<const f32x4*>(skip + (long long)i * 4));
      }
    }
#pragma unroll
    for (int u = 0; u < EW_UNR; ++u) {
      const unsigned i = i0 + u * 256;
      if (i >= tot) break;
      const float* sp = stats + (long long)(i / l4) * LG_NSTAT;
      const float mu = sp[0], a = sp[2], b = sp[3], mul = sp[4];
      float dm[4];
      if constexpr (DROP) drop_mult4(dc, i, dm);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float t = v[u][k];
        if (pre_leaky) t = lg_leaky(t, alpha);
        t = a * ((t - mu) - mul) + b;  // (x-mu)/(sigma+eps)*gamma + beta, as instance.py:116-127 (no cancellation)
        if (post_leaky) t = lg_leaky(t, alpha);
        if constexpr (DROP) t = t * dm[k];
        v[u][k] = t;
      }
      if (skip) v[u] += sk[u];
      if (y) *reinterpret_cast<f32x4*>(y + (long long)i * 4) = v[u];
      if (y16) {  // bf16 mirror = exactly the MFMA operand the consumers would round to themselves
        bf16x4 w;
        w[0] = (__bf16)v[u][0]; w[1] = (__bf16)v[u][1]; w[2] = (__bf16)v[u][2]; w[3] = (__bf16)v[u][3];
        *reinterpret_cast<bf16x4*>(y16 + (long long)i * 4) = w;
      }
    }
  }
}

__global__ __launch_bounds__(256) void apply_kernel(const float* __restrict__ x, const float* __restrict__ stats,
                                                    const float* __restrict__ skip, float* __restrict__ y,
                                                    __bf16* __restrict__ y16, long long L4, long long total4,
                                                    int pre_leaky, int post_leaky, float alpha) {
  apply_body<false>(x, stats, skip, y, y16, L4, total4, pre_leaky, post_leaky, alpha, DropK{}, Geo{blockDim.x, gridDim.x, gridDim.y});
}
// the encoder's form (no skip operand, LeakyReLU behind the norm) with the dropout mask
__global__ __launch_bounds__(256) void apply_drop_kernel(const float* __restrict__ x, const float* __restrict__ stats,
                                                         float* __restrict__ y, __bf16* __restrict__ y16, long long L4,
                                                         long long total4, float alpha, DropK dk) {
  apply_body<true>(x, stats, nullptr, y, y16, L4, total4, 0, 1, alpha, dk, Geo{blockDim.x, gridDim.x, gridDim.y});
}

template <bool NT = false>
__device__ __forceinline__ f32x4 load_g4(const void* g, long long i4, int g16) {  // 4 gradient values, fp32 or bf16 storage
  if (g16) {
    const bf16x4 w = lg_ld<NT>(reinterpret_cast<const bf16x4*>(reinterpret_cast<const __bf16*>(g) + i4));
    return f32x4{(float)w[0], (float)w[1], (float)w[2], (float)w[3]};
  }
  return lg_ld<NT>(reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(g) + i4));
}

// partial[n][chunk] = {sum dz, sum dz*c} (doubles)
template <bool DROP>
__device__ __forceinline__ void bwd_partial_body(const float* __restrict__ x, const void* __restrict__ g, int g16,
                                                 const float* __restrict__ stats, double* __restrict__ partial,
                                                 long long L, int nchunk, int pre_leaky, int post_leaky,
                                                 float alpha, const DropK& dk, const Geo ge) {
  const DropCtx dc = drop_begin<DROP>(dk);
  // ge.gdx blocks per sample, each sweeping chunks blockIdx.x, blockIdx.x + ge.gdx, ... (few long-lived blocks
  // stream better than one short block per chunk), ONE block reduction at the end; nchunk = ge.gdx partial records
  const int n = blockIdx.y;
  const float* sp = stats + (long long)n * LG_NSTAT;
  const float mu = sp[0], a = sp[2], b = sp[3], mul = sp[4];
  __shared__ double sred[32];
  double s1 = 0.0, s2 = 0.0;
  for (long long c0 = (long long)blockIdx.x * CHUNK; c0 < L; c0 += (long long)ge.gdx * CHUNK) {
   const long long base = (long long)n * L + c0;
   const long long lim = L - c0;
#pragma unroll
   for (int q = 0; q < 4; ++q) {
    const int e = (q * 256 + threadIdx.x) * 4;
    if (e < lim) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + base + e);
      const f32x4 gv = load_g4(g, base + e, g16);
      // the 4 values of a quad are summed in fp32 (c = (x - mu_hi) - mu_lo is the float-float centred value the
      // forward pass uses, so no coherent error enters), the quads in fp64: the fp64 VALU rate, not HBM, bounded this pass
      float q1 = 0.f, q2 = 0.f;
      float dm[4];
      if constexpr (DROP) drop_mult4(dc, (unsigned long long)(base + e) >> 2, dm);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float xx = xv[k];
        if (pre_leaky) xx = lg_leaky(xx, alpha);
        const float c = (xx - mu) - mul;
        float dz = gv[k];
        if constexpr (DROP) dz = dz * dm[k];   // the gradient behind the mask: both passes of the backward see it
        if (post_leaky) dz = (a * c + b > 0.f) ? dz : alpha * dz;
        q1 += dz;
        q2 += dz * c;
      }
      s1 += (double)q1;
      s2 += (double)q2;
    }
   }
  }
  double red[2] = {s1, s2};
  lg_block_sum_d<2>(red, sred);
  if (threadIdx.x == 0) {
    double* o = partial + ((long long)n * nchunk + blockIdx.x) * 2;
    o[0] = red[0]; o[1] = red[1];
  }
}

__global__ __launch_bounds__(256) void bwd_partial_kernel(const float* __restrict__ x, const void* __restrict__ g, int g16,
                                                          const float* __restrict__ stats, double* __restrict__ partial,
                                                          long long L, int nchunk, int pre_leaky, int post_leaky,
                                                          float alpha) {
  bwd_partial_body<false>(x, g, g16, stats, partial, L, nchunk, pre_leaky, post_leaky, alpha, DropK{}, Geo{blockDim.x, gridDim.x, gridDim.y});
}
__global__ __launch_bounds__(256) void bwd_partial_drop_kernel(const float* __restrict__ x, const void* __restrict__ g, int g16,
                                                               const float* __restrict__ stats, double* __restrict__ partial,
                                                               long long L, int nchunk, float alpha, DropK dk) {
  bwd_partial_body<true>(x, g, g16, stats, partial, L, nchunk, 0, 1, alpha, dk, Geo{blockDim.x, gridDim.x, gridDim.y});
}

// bstats[n][4] = {m1_hi, m2'_hi, m1_lo, m2'_lo} ; gsum[n] = per-sample dgamma / dbeta contributions
__global__ __launch_bounds__(64) void bwd_final_kernel(const double* __restrict__ partial, const float* __restrict__ stats,
                                                       float* __restrict__ bstats, double* __restrict__ gsum,
                                                       long long L, int nchunk) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const double* p = partial + (long long)n * nchunk * 2;
  double s1 = 0.0, s2 = 0.0;
  for (int i = lane; i < nchunk; i += 64) { s1 += p[i * 2]; s2 += p[i * 2 + 1]; }
  s1 = lg_wave_sum_d(s1); s2 = lg_wave_sum_d(s2);
  if (lane == 0) {
    const double sigma = (double)stats[(long long)n * LG_NSTAT + 1], s = sigma + (double)LG_IN_EPS;
    const double m1 = s1 / (double)L, m2 = s2 / (double)L / (s * sigma);
    const float m1h = (float)m1, m2h = (float)m2;
    bstats[n * 4] = m1h; bstats[n * 4 + 1] = m2h;
    bstats[n * 4 + 2] = (float)(m1 - (double)m1h); bstats[n * 4 + 3] = (float)(m2 - (double)m2h);
    gsum[n * 2] = s2 / s;  // dgamma contribution
    gsum[n * 2 + 1] = s1;  // dbeta contribution
  }
}

// coef[n][8] = {mu_hi, mu_lo, a, beta, m1_hi, m2'_hi, m1_lo, m2'_lo}: everything a consumer needs to form the norm backward's dz
// of sample n from (z, g) on the fly (lg_bwdnorm8, lg_common.h) — the sums are merged exactly as bwd_final_kernel merges them
__global__ __launch_bounds__(64) void bwd_coef_kernel(const double* __restrict__ partial, const float* __restrict__ stats,
                                                      float* __restrict__ coef, long long L, int nchunk) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const double* p = partial + (long long)n * nchunk * 2;
  double s1 = 0.0, s2 = 0.0;
  for (int i = lane; i < nchunk; i += 64) { s1 += p[i * 2]; s2 += p[i * 2 + 1]; }
  s1 = lg_wave_sum_d(s1); s2 = lg_wave_sum_d(s2);
  if (lane == 0) {
    const float* sp = stats + (long long)n * LG_NSTAT;
    const double sigma = (double)sp[1], s = sigma + (double)LG_IN_EPS;
    const double m1 = s1 / (double)L, m2 = s2 / (double)L / (s * sigma);
    const float m1h = (float)m1, m2h = (float)m2;
    float* o = coef + (long long)n * 8;
    o[0] = sp[0]; o[1] = sp[4]; o[2] = sp[2]; o[3] = sp[3];
    o[4] = m1h; o[5] = m2h; o[6] = (float)(m1 - (double)m1h); o[7] = (float)(m2 - (double)m2h);
  }
}

__global__ __launch_bounds__(256) void bwd_affine_grad_kernel(const double* __restrict__ gsum, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, int B, int accumulate) {
  __shared__ double sg[256], sb[256];
  double g = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < B; i += 256) { g += gsum[i * 2]; b += gsum[i * 2 + 1]; }
  sg[threadIdx.x] = g; sb[threadIdx.x] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) { sg[threadIdx.x] += sg[threadIdx.x + o]; sb[threadIdx.x] += sb[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    dgamma[0] = (accumulate ? dgamma[0] : 0.f) + (float)sg[0];
    dbeta[0] = (accumulate ? dbeta[0] : 0.f) + (float)sb[0];
  }
}

// DB: also the column sums of dx over (sample, position) = the bias gradient of the conv that produced x ([.., C]
// channels innermost).  The launch makes gridDim.x*256 a multiple of C/4, so a thread meets the same 4 channels in
// every trip; threads of a block are merged in thread order into colpart[block][C] (deterministic), blocks by
// colsum_final (below).
template <bool DB, bool DROP>
__device__ __forceinline__ void bwd_apply_body(const float* __restrict__ x, const void* __restrict__ g, int g16,
                                               const float* __restrict__ stats, const float* __restrict__ bstats,
                                               float* __restrict__ dx, __bf16* __restrict__ dx16, long long L4,
                                               long long total4, int pre_leaky, int post_leaky, float alpha,
                                               float* __restrict__ colpart, int C4, const DropK& dk, const Geo ge) {
  const DropCtx dc = drop_begin<DROP>(dk);
  constexpr int UNR = DB ? 1 : EW_UNR;  // DB: a thread must stay on one channel quad -> plain grid stride
  const unsigned stride = ge.gdx * ge.bdx * UNR, tot = (unsigned)total4, l4 = (unsigned)L4;
  f32x4 csum = {0.f, 0.f, 0.f, 0.f};
  const unsigned rb = blockIdx.x;
  const int ntrip = (int)(((unsigned long long)tot + stride - 1) / stride);
  for (int tr = 0; tr < ntrip; ++tr) {
   const unsigned long long i0l = (unsigned long long)tr * stride + rb * ge.bdx * UNR + threadIdx.x;
   if (i0l >= tot) continue;
   const unsigned i0 = (unsigned)i0l;
   f32x4 xs[UNR], gs[UNR];
#pragma unroll
   for (int u = 0; u < UNR; ++u) {
     const unsigned i = i0 + u * 256;
     if (i < tot) {
       xs[u] = lg_ld<NT_LOAD>(reinterpret_cast<const f32x4*>(x + (long long)i * 4));   // last reader of z and g
       gs[u] = load_g4<NT_LOAD>(g, (long long)i * 4, g16);
     }
   }
#pragma unroll
   for (int u = 0; u < UNR; ++u) {
    const unsigned i = i0 + u * 256;
    if (i >= tot) break;
    const int n = (int)(i / l4);
    const float* sp = stats + (long long)n * LG_NSTAT;
    const float mu = sp[0], a = sp[2], b = sp[3], mul = sp[4];
    const float m1 = bstats[n * 4], m2 = bstats[n * 4 + 1], m1l = bstats[n * 4 + 2], m2l = bstats[n * 4 + 3];
    const f32x4 xv = xs[u], gv = gs[u];
    f32x4 o;
    float dm[4];
    if constexpr (DROP) drop_mult4(dc, i, dm);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float xx = xv[k];
      if (pre_leaky) xx = lg_leaky(xx, alpha);
      const float c = (xx - mu) - mul;
      float dz = gv[k];
      if constexpr (DROP) dz = dz * dm[k];
      if (post_leaky) dz = (a * c + b > 0.f) ? dz : alpha * dz;
      float d = a * ((((dz - m1) - m1l) - c * m2) - c * m2l);
      if (pre_leaky) d = (xv[k] > 0.f) ? d : alpha * d;
      o[k] = d;
    }
    if (dx) *reinterpret_cast<f32x4*>(dx + (long long)i * 4) = o;
    if (dx16) {
      bf16x4 w;
      w[0] = (__bf16)o[0]; w[1] = (__bf16)o[1]; w[2] = (__bf16)o[2]; w[3] = (__bf16)o[3];
      *reinterpret_cast<bf16x4*>(dx16 + (long long)i * 4) = w;
    }
    if constexpr (DB) csum += o;
   }
  }
  if constexpr (DB) {
    __shared__ f32x4 sacc[256];
    sacc[threadIdx.x] = csum;
    __syncthreads();
    const int q = threadIdx.x;  // channel quad
    if (q < C4) {
      const int base = (int)(((long long)rb * 256) % C4);
      f32x4 t = {0.f, 0.f, 0.f, 0.f};
      for (int k = (q - base + C4) % C4; k < 256; k += C4) t += sacc[k];
      *reinterpret_cast<f32x4*>(colpart + ((long long)rb * C4 + q) * 4) = t;
    }
  }
}
template <bool DB>
__global__ __launch_bounds__(256) void bwd_apply_kernel(const float* __restrict__ x, const void* __restrict__ g, int g16,
                                                        const float* __restrict__ stats, const float* __restrict__ bstats,
                                                        float* __restrict__ dx, __bf16* __restrict__ dx16, long long L4,
                                                        long long total4, int pre_leaky, int post_leaky, float alpha,
                                                        float* __restrict__ colpart, int C4) {
  bwd_apply_body<DB, false>(x, g, g16, stats, bstats, dx, dx16, L4, total4, pre_leaky, post_leaky, alpha, colpart, C4, DropK{}, Geo{blockDim.x, gridDim.x, gridDim.y});
}
template <bool DB>
__global__ __launch_bounds__(256) void bwd_apply_drop_kernel(const float* __restrict__ x, const void* __restrict__ g, int g16,
                                                             const float* __restrict__ stats, const float* __restrict__ bstats,
                                                             float* __restrict__ dx, __bf16* __restrict__ dx16, long long L4,
                                                             long long total4, float alpha, float* __restrict__ colpart, int C4,
                                                             DropK dk) {
  bwd_apply_body<DB, true>(x, g, g16, stats, bstats, dx, dx16, L4, total4, 0, 1, alpha, colpart, C4, dk, Geo{blockDim.x, gridDim.x, gridDim.y});
}


// ---------------------------------------------------------------------------------------------------------------------
// bf16 activation path ("z16"): in the bf16 MFMA configuration the raw conv output z lives in HBM as bf16 only (the
// moments come from the fp32 accumulators of the conv epilogue, so they are unaffected), the skip tensors are the bf16
// mirrors the encoder wrote anyway, and the gradients arrive as bf16.  These kernels move 8 elements (16 B of bf16) per
// thread per access; fp32 operands, where one is mixed in, are two 16-B accesses.  L % 8 == 0.
typedef __bf16 bf16x8v __attribute__((ext_vector_type(8)));
struct f32x8 { f32x4 lo, hi; };

template <bool IS16, bool NT = false>
__device__ __forceinline__ f32x8 load8(const void* p, long long i8) {  // elements [8*i8, 8*i8 + 8)
  f32x8 r;
  if constexpr (IS16) {
    const bf16x8v* q = reinterpret_cast<const bf16x8v*>(reinterpret_cast<const __bf16*>(p) + i8 * 8);
    const bf16x8v w = NT ? __builtin_nontemporal_load(q) : *q;
    r.lo = f32x4{(float)w[0], (float)w[1], (float)w[2], (float)w[3]};
    r.hi = f32x4{(float)w[4], (float)w[5], (float)w[6], (float)w[7]};
  } else {
    const float* f = reinterpret_cast<const float*>(p) + i8 * 8;
    r.lo = *reinterpret_cast<const f32x4*>(f);
    r.hi = *reinterpret_cast<const f32x4*>(f + 4);
  }
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

// 16-B accesses in flight per thread and stream.  r3 sweep (same box, B=256 maps): 2 beats 4 and 8 by 3 - 8 % on apply, apply + skip and the
// backward apply (more waves resident)
constexpr int EW8_UNR = 2, DB_UNR = 2;

// y = leaky(a*((z - mu_hi) - mu_lo) + beta) [+ skip]  from the bf16 z;  SK: 0 none, 1 fp32 skip, 2 bf16 skip
template <int SK, bool DROP>
__device__ __forceinline__ void apply16_body(const __bf16* __restrict__ x, const float* __restrict__ stats,
                                             const void* __restrict__ skip, float* __restrict__ y,
                                             __bf16* __restrict__ y16, long long L8, long long total8,
                                             int pre_leaky, int post_leaky, float alpha, const DropK& dk, const Geo ge) {
  const DropCtx dc = drop_begin<DROP>(dk);
  const unsigned stride = ge.gdx * ge.bdx * EW8_UNR, tot = (unsigned)total8, l8 = (unsigned)L8;
  for (unsigned i0 = blockIdx.x * ge.bdx * EW8_UNR + threadIdx.x; i0 < tot; i0 += stride) {
    f32x8 v[EW8_UNR], sk[EW8_UNR];
#pragma unroll
    for (int u = 0; u < EW8_UNR; ++u) {
      const unsigned i = i0 + u * 256;
      if (i < tot) {
        v[u] = load8<true>(x, i);
        if constexpr (SK == 1) sk[u] = load8<false>(skip, i);
        if constexpr (SK == 2) sk[u] = load8<true>(skip, i);
      }
    }
#pragma unroll
    for (int u = 0; u < EW8_UNR; ++u) {
      const unsigned i = i0 + u * 256;
      if (i >= tot) break;
      const float* sp = stats + (long long)(i / l8) * LG_NSTAT;
      const float mu = sp[0], a = sp[2], b = sp[3], mul = sp[4];
      float dm[8];
      if constexpr (DROP) drop_mult8(dc, i, dm);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float t = k < 4 ? v[u].lo[k & 3] : v[u].hi[k & 3];
        if (pre_leaky) t = lg_leaky(t, alpha);
        t = a * ((t - mu) - mul) + b;
        if (post_leaky) t = lg_leaky(t, alpha);
        if constexpr (DROP) t = t * dm[k];
        if constexpr (SK != 0) t += k < 4 ? sk[u].lo[k & 3] : sk[u].hi[k & 3];
        if (k < 4) v[u].lo[k & 3] = t; else v[u].hi[k & 3] = t;
      }
      if (y) store8_f32(y, i, v[u]);
      if (y16) store8_bf16(y16, i, v[u]);
    }
  }
}

template <int SK>
__global__ __launch_bounds__(256) void apply16_kernel(const __bf16* __restrict__ x, const float* __restrict__ stats,
                                                      const void* __restrict__ skip, float* __restrict__ y,
                                                      __bf16* __restrict__ y16, long long L8, long long total8,
                                                      int pre_leaky, int post_leaky, float alpha) {
  apply16_body<SK, false>(x, stats, skip, y, y16, L8, total8, pre_leaky, post_leaky, alpha, DropK{}, Geo{blockDim.x, gridDim.x, gridDim.y});
}
__global__ __launch_bounds__(256) void apply16_drop_kernel(const __bf16* __restrict__ x, const float* __restrict__ stats,
                                                           float* __restrict__ y, __bf16* __restrict__ y16, long long L8,
                                                           long long total8, float alpha, DropK dk) {
  apply16_body<0, true>(x, stats, nullptr, y, y16, L8, total8, 0, 1, alpha, dk, Geo{blockDim.x, gridDim.x, gridDim.y});
}

// apply16 with the statistics FINALISED IN THE SAME LAUNCH: grid (blocks per sample, B); the first wave of every block merges the
// sample's moment partials {count, mean, M2} exactly as stats_final_kernel does (same order, same fp64 arithmetic: the record is
// bit-identical), block 0 of a sample writes the record for the later consumers (backward, fused conv epilogues).  One launch and
// one kernel boundary less per normalised map (22 per C3 step); post-LeakyReLU form only (pre_leaky = 0).
template <int SK, bool DROP>
__device__ __forceinline__ void apply16p_body(const __bf16* __restrict__ x, const double* __restrict__ partial, int nchunk,
                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                              float* __restrict__ stats, const void* __restrict__ skip,
                                              float* __restrict__ y, __bf16* __restrict__ y16, unsigned L8,
                                              int post_leaky, float alpha, const DropK& dk, const Geo ge) {
  const DropCtx dc = drop_begin<DROP>(dk);
  __shared__ float sst[8];
  // samples and chunks from the END — the producer wrote the end of the map last, the consumer reads its start first
  const int n = (int)(ge.gdy - 1 - blockIdx.y);
  const unsigned bx = ge.gdx - 1 - blockIdx.x;
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
  const float mu = sst[0], a = sst[2], b = sst[3], mul = sst[4];
  const long long base = (long long)n * L8;
  const unsigned stride = ge.gdx * ge.bdx * EW8_UNR;
  const int ntrip = (int)((L8 + stride - 1) / stride);
  for (int tr = 0; tr < ntrip; ++tr) {
    const unsigned i0 = (unsigned)(ntrip - 1 - tr) * stride + bx * ge.bdx * EW8_UNR + threadIdx.x;
    if (i0 >= L8) continue;
    f32x8 v[EW8_UNR], sk[EW8_UNR];
#pragma unroll
    for (int u = 0; u < EW8_UNR; ++u) {
      const unsigned i = i0 + u * 256;
      if (i < L8) {
        v[u] = load8<true, NT_LOAD>(x, base + i);
        if constexpr (SK == 1) sk[u] = load8<false, NT_LOAD>(skip, base + i);
        if constexpr (SK == 2) sk[u] = load8<true, NT_LOAD>(skip, base + i);
      }
    }
#pragma unroll
    for (int u = 0; u < EW8_UNR; ++u) {
      const unsigned i = i0 + u * 256;
      if (i >= L8) break;
      float dm[8];
      if constexpr (DROP) drop_mult8(dc, (unsigned long long)(base + i), dm);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float t = k < 4 ? v[u].lo[k & 3] : v[u].hi[k & 3];
        t = a * ((t - mu) - mul) + b;
        if (post_leaky) t = lg_leaky(t, alpha);
        if constexpr (DROP) t = t * dm[k];
        if constexpr (SK != 0) t += k < 4 ? sk[u].lo[k & 3] : sk[u].hi[k & 3];
        if (k < 4) v[u].lo[k & 3] = t; else v[u].hi[k & 3] = t;
      }
      if (y) store8_f32(y, base + i, v[u]);
      if (y16) store8_bf16(y16, base + i, v[u]);
    }
  }
}

template <int SK>
__global__ __launch_bounds__(256) void apply16p_kernel(const __bf16* __restrict__ x, const double* __restrict__ partial, int nchunk,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float* __restrict__ stats, const void* __restrict__ skip,
                                                       float* __restrict__ y, __bf16* __restrict__ y16, unsigned L8,
                                                       int post_leaky, float alpha) {
  apply16p_body<SK, false>(x, partial, nchunk, gamma, beta, stats, skip, y, y16, L8, post_leaky, alpha, DropK{}, Geo{blockDim.x, gridDim.x, gridDim.y});
}
__global__ __launch_bounds__(256) void apply16p_drop_kernel(const __bf16* __restrict__ x, const double* __restrict__ partial, int nchunk,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            float* __restrict__ stats, float* __restrict__ y,
                                                            __bf16* __restrict__ y16, unsigned L8, float alpha, DropK dk) {
  apply16p_body<0, true>(x, partial, nchunk, gamma, beta, stats, nullptr, y, y16, L8, 1, alpha, dk, Geo{blockDim.x, gridDim.x, gridDim.y});
}

// partial[n][blk] = {sum dz, sum dz*c} from the bf16 z; G16: gradient stored as bf16
template <bool G16, bool DROP>
__device__ __forceinline__ void bwd_partial16_body(const __bf16* __restrict__ x, const void* __restrict__ g,
                                                   const float* __restrict__ stats, double* __restrict__ partial,
                                                   long long L, int nchunk, int pre_leaky, int post_leaky,
                                                   float alpha, const DropK& dk, const Geo ge) {
  const DropCtx dc = drop_begin<DROP>(dk);
  const int n = blockIdx.y;
  const float* sp = stats + (long long)n * LG_NSTAT;
  const float mu = sp[0], a = sp[2], b = sp[3], mul = sp[4];
  __shared__ double sred[32];
  double s1 = 0.0, s2 = 0.0;
  constexpr int CH8 = 2 * CHUNK;  // elements per block trip (256 threads x 4 x 8)
  for (long long c0 = (long long)blockIdx.x * CH8; c0 < L; c0 += (long long)ge.gdx * CH8) {
    const long long base8 = ((long long)n * L + c0) / 8;
    const long long lim = L - c0;
    f32x8 xv[4], gv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = (q * 256 + threadIdx.x) * 8;
      if (e < lim) { xv[q] = load8<true>(x, base8 + e / 8); gv[q] = load8<G16>(g, base8 + e / 8); }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = (q * 256 + threadIdx.x) * 8;
      if (e < lim) {
        float q1 = 0.f, q2 = 0.f;
        float dm[8];
        if constexpr (DROP) drop_mult8(dc, (unsigned long long)(base8 + e / 8), dm);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float xx = k < 4 ? xv[q].lo[k & 3] : xv[q].hi[k & 3];
          if (pre_leaky) xx = lg_leaky(xx, alpha);
          const float c = (xx - mu) - mul;
          float dz = k < 4 ? gv[q].lo[k & 3] : gv[q].hi[k & 3];
          if constexpr (DROP) dz = dz * dm[k];
          if (post_leaky) dz = (a * c + b > 0.f) ? dz : alpha * dz;
          q1 += dz;
          q2 += dz * c;
        }
        s1 += (double)q1;
        s2 += (double)q2;
      }
    }
  }
  double red[2] = {s1, s2};
  lg_block_sum_d<2>(red, sred);
  if (threadIdx.x == 0) {
    double* o = partial + ((long long)n * nchunk + blockIdx.x) * 2;
    o[0] = red[0]; o[1] = red[1];
  }
}

template <bool G16>
__global__ __launch_bounds__(256) void bwd_partial16_kernel(const __bf16* __restrict__ x, const void* __restrict__ g,
                                                            const float* __restrict__ stats, double* __restrict__ partial,
                                                            long long L, int nchunk, int pre_leaky, int post_leaky,
                                                            float alpha) {
  bwd_partial16_body<G16, false>(x, g, stats, partial, L, nchunk, pre_leaky, post_leaky, alpha, DropK{}, Geo{blockDim.x, gridDim.x, gridDim.y});
}
template <bool G16>
__global__ __launch_bounds__(256) void bwd_partial16_drop_kernel(const __bf16* __restrict__ x, const void* __restrict__ g,
                                                                 const float* __restrict__ stats, double* __restrict__ partial,
                                                                 long long L, int nchunk, float alpha, DropK dk) {
  bwd_partial16_body<G16, true>(x, g, stats, partial, L, nchunk, 0, 1, alpha, dk, Geo{blockDim.x, gridDim.x, gridDim.y});
}

// dz = a*(dy' - m1 - c*m2') from the bf16 z; DB: + column sums (bias gradient); the launch makes gridDim.x*256 a multiple
// of C/8, so a thread meets the same 8 channels in every trip
template <bool DB, bool G16, bool DROP>
__device__ __forceinline__ void bwd_apply16_body(const __bf16* __restrict__ x, const void* __restrict__ g,
                                                 const float* __restrict__ stats, const float* __restrict__ bstats,
                                                 float* __restrict__ dx, __bf16* __restrict__ dx16, long long L8,
                                                 long long total8, int pre_leaky, int post_leaky, float alpha,
                                                 float* __restrict__ colpart, int C8, const DropK& dk, const Geo ge) {
  const DropCtx dc = drop_begin<DROP>(dk);
  constexpr int UNR = DB ? DB_UNR : EW8_UNR;  // DB: the extra loads of a trip sit ge.gdx*256 units apart (same channel octet)
  const unsigned tot = (unsigned)total8, l8 = (unsigned)L8;
  const unsigned ustep = DB ? ge.gdx * ge.bdx : 256u;                  // distance between a thread's units of one trip
  const unsigned stride = DB ? ge.gdx * ge.bdx * UNR : ge.gdx * ge.bdx * UNR;
  const unsigned rb = ge.gdx - 1 - blockIdx.x;   // from the END of the map (the block's data AND its column-sum row: results unchanged)
  const unsigned first = DB ? rb * ge.bdx + threadIdx.x : rb * ge.bdx * UNR + threadIdx.x;
  f32x8 csum;
  csum.lo = f32x4{0.f, 0.f, 0.f, 0.f}; csum.hi = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ntrip = (int)(((unsigned long long)tot + stride - 1) / stride);
  for (int tr = 0; tr < ntrip; ++tr) {
    const unsigned long long i0l = (unsigned long long)(ntrip - 1 - tr) * stride + first;
    if (i0l >= tot) continue;
    const unsigned i0 = (unsigned)i0l;
    f32x8 xs[UNR], gs[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const unsigned i = i0 + u * ustep;
      if (i < tot) { xs[u] = load8<true, NT_LOAD>(x, i); gs[u] = load8<G16, NT_LOAD>(g, i); }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const unsigned i = i0 + u * ustep;
      if (i >= tot) break;
      const int n = (int)(i / l8);
      const float* sp = stats + (long long)n * LG_NSTAT;
      const float mu = sp[0], a = sp[2], b = sp[3], mul = sp[4];
      const float m1 = bstats[n * 4], m2 = bstats[n * 4 + 1], m1l = bstats[n * 4 + 2], m2l = bstats[n * 4 + 3];
      f32x8 o;
      float dm[8];
      if constexpr (DROP) drop_mult8(dc, i, dm);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float x0 = k < 4 ? xs[u].lo[k & 3] : xs[u].hi[k & 3];
        float xx = x0;
        if (pre_leaky) xx = lg_leaky(xx, alpha);
        const float c = (xx - mu) - mul;
        float dz = k < 4 ? gs[u].lo[k & 3] : gs[u].hi[k & 3];
        if constexpr (DROP) dz = dz * dm[k];
        if (post_leaky) dz = (a * c + b > 0.f) ? dz : alpha * dz;
        float d = a * ((((dz - m1) - m1l) - c * m2) - c * m2l);
        if (pre_leaky) d = (x0 > 0.f) ? d : alpha * d;
        if (k < 4) o.lo[k & 3] = d; else o.hi[k & 3] = d;
      }
      if (dx) store8_f32(dx, i, o);
      if (dx16) store8_bf16(dx16, i, o);
      if constexpr (DB) { csum.lo += o.lo; csum.hi += o.hi; }
    }
  }
  if constexpr (DB) {
    __shared__ f32x4 sacc[512];
    sacc[2 * threadIdx.x] = csum.lo; sacc[2 * threadIdx.x + 1] = csum.hi;
    __syncthreads();
    const int q = threadIdx.x;  // channel octet
    if (q < C8) {
      const int base = (int)(((long long)rb * 256) % C8);
      f32x4 tl = {0.f, 0.f, 0.f, 0.f}, th = {0.f, 0.f, 0.f, 0.f};
      for (int k = (q - base + C8) % C8; k < 256; k += C8) { tl += sacc[2 * k]; th += sacc[2 * k + 1]; }
      *reinterpret_cast<f32x4*>(colpart + ((long long)rb * C8 + q) * 8) = tl;
      *reinterpret_cast<f32x4*>(colpart + ((long long)rb * C8 + q) * 8 + 4) = th;
    }
  }
}

template <bool DB, bool G16>
__global__ __launch_bounds__(256) void bwd_apply16_kernel(const __bf16* __restrict__ x, const void* __restrict__ g,
                                                          const float* __restrict__ stats, const float* __restrict__ bstats,
                                                          float* __restrict__ dx, __bf16* __restrict__ dx16, long long L8,
                                                          long long total8, int pre_leaky, int post_leaky, float alpha,
                                                          float* __restrict__ colpart, int C8) {
  bwd_apply16_body<DB, G16, false>(x, g, stats, bstats, dx, dx16, L8, total8, pre_leaky, post_leaky, alpha, colpart, C8, DropK{}, Geo{blockDim.x, gridDim.x, gridDim.y});
}
template <bool DB, bool G16>
__global__ __launch_bounds__(256) void bwd_apply16_drop_kernel(const __bf16* __restrict__ x, const void* __restrict__ g,
                                                               const float* __restrict__ stats, const float* __restrict__ bstats,
                                                               float* __restrict__ dx, __bf16* __restrict__ dx16, long long L8,
                                                               long long total8, float alpha, float* __restrict__ colpart, int C8,
                                                               DropK dk) {
  bwd_apply16_body<DB, G16, true>(x, g, stats, bstats, dx, dx16, L8, total8, 0, 1, alpha, colpart, C8, dk, Geo{blockDim.x, gridDim.x, gridDim.y});
}

// keep[r][e] (bytes, 1 = kept) of the rows r0 .. r0+B-1 of one (call, level) slot: the definition above made testable
__global__ __launch_bounds__(256) void dropout_mask_kernel(unsigned char* __restrict__ keep, long long total8, DropK dk) {
  const DropCtx dc = drop_begin<true>(dk);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total8; i += (long long)gridDim.x * 256) {
    float dm[8];
    drop_mult8(dc, (unsigned long long)i, dm);
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { lo |= (dm[k] != 0.f ? 1u : 0u) << (8 * k); hi |= (dm[4 + k] != 0.f ? 1u : 0u) << (8 * k); }
    *reinterpret_cast<unsigned long long*>(keep + i * 8) = (unsigned long long)lo | ((unsigned long long)hi << 32);
  }
}

// db[c] (+)= sum_k part[k][c]: 16 columns x 64 row groups per block (1024 threads: with 16 groups a thread walked 128 rows of
// the <= 2046, 12.7 us per launch, seven launches per step), merged in group order (deterministic)
__global__ __launch_bounds__(1024) void colsum_final_kernel(const float* __restrict__ partial, float* __restrict__ db, int nb,
                                                            int C, int accumulate) {
  __shared__ float sr[64][17];
  const int cl = threadIdx.x & 15, gq = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  float s = 0.f;
  if (c < C) {
    int k = gq;
    for (; k + 192 < nb; k += 256) {
      const float a = partial[(long long)k * C + c], b = partial[(long long)(k + 64) * C + c];
      const float e = partial[(long long)(k + 128) * C + c], f = partial[(long long)(k + 192) * C + c];
      s += (a + b) + (e + f);
    }
    for (; k < nb; k += 64) s += partial[(long long)k * C + c];
  }
  sr[gq][cl] = s;
  __syncthreads();
  if (gq == 0 && c < C) {
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < 64; q += 4) t += (sr[q][cl] + sr[q + 1][cl]) + (sr[q + 2][cl] + sr[q + 3][cl]);
    db[c] = (accumulate ? db[c] : 0.f) + t;
  }
}

// Grid cap of the element-wise passes (blocks of 256 threads walking the map in trips); the bias-sum forms are capped by DB_MAX_BLOCKS.
// (Fewer, longer-lived blocks against many short ones: swept in round 5, the whole-rounds rule below is what came of it.)
constexpr long long EW_MAX_BLOCKS = 8192;
// WHOLE ROUNDS (round 5).  These grids are larger than what the chip holds at once (blocks of 256 threads, 4 .. 8 per CU by their
// VGPRs), so they run in rounds — and a last partial round costs a whole trip time for a fraction of the work: the bias-sum form of
// the backward apply (71 VGPRs: 7 blocks per CU = 1792 resident) was launched as 2046 blocks = one round + 254 blocks, 14 % of a
// round at the price of one (1533 = six per CU beat both 2046 and 1023; C3 step -0.9 %).  A grid
// beyond one round is cut to a whole number of rounds of the kernel's own residency (occupancy query, once per kernel).
#define LG_RESIDENT_BLOCKS(kern)                                                                                       \
  ([]() -> long long {                                                                                                 \
    static long long r = 0;                                                                                            \
    if (!r) {                                                                                                          \
      int per_cu = 0;                                                                                                  \
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, 0) != hipSuccess || per_cu < 1) per_cu = 8; \
      r = (long long)per_cu * lg_device_cus();                                                                         \
    }                                                                                                                  \
    return r;                                                                                                          \
  }())
inline long long fit_rounds(long long nb, long long resident, long long hard, int unit) {
  if (nb > hard) nb = hard;
  if (nb > resident) nb = nb / resident * resident;
  nb = nb / unit * unit;
  return nb < unit ? unit : nb;
}
inline int nchunks(long long L) { return (int)((L + CHUNK - 1) / CHUNK); }
inline int ew_blocks(long long total4) {
  long long b = (total4 + 256 * EW_UNR - 1) / (256 * EW_UNR);
  return (int)(b < EW_MAX_BLOCKS ? (b > 0 ? b : 1) : EW_MAX_BLOCKS);
}
inline size_t part_bytes(int B, long long L) { return ((size_t)B * nchunks(L) * 3 * sizeof(double) + 255) / 256 * 256; }
inline size_t bst_bytes(int B) { return ((size_t)B * 4 * sizeof(float) + 255) / 256 * 256; }

// What the current entry point launched (lg_instnorm_last_launches): every launch of this file goes through NORM_LAUNCH, which
// records the kernel as it is spelled at the launch site (a string literal: nothing is formatted here) and its grid.  Reset on
// entry of every function below that can launch, BEFORE its argument checks: a refused call reports no launch.
struct LaunchNote { const char* name; unsigned gx, gy; };
constexpr int NL_MAX = 8;  // the longest chain is 5: partial, final, affine, apply + bias, colsum
thread_local LaunchNote g_nl[NL_MAX];
thread_local int g_nl_n = 0;
inline void nl_reset() { g_nl_n = 0; }
inline void nl_note(const char* name, const dim3& g) {
  if (g_nl_n < NL_MAX) g_nl[g_nl_n] = LaunchNote{name, g.x, g.y};
  ++g_nl_n;
}
#define NORM_LAUNCH(kern, grid, block, shmem, st, ...)                  \
  do {                                                                  \
    const dim3 nl_grid_ = (grid);                                       \
    nl_note(#kern, nl_grid_);                                           \
    hipLaunchKernelGGL(kern, nl_grid_, block, shmem, st, __VA_ARGS__);  \
  } while (0)

// host-side checks of a dropout launch + its kernel argument (see DropK)
int drop_args(const char* who, const long long* key, int call, int level, int r0, int B, long long L, float rate, DropK* dk) {
  nl_reset();
  LG_CHECK_ARG(key, "%s: null pointer (dropout key)", who);
  LG_CHECK_ARG(L > 0 && L % 8 == 0, "%s: dropout needs L %% 8 == 0 (one Philox block per 8 elements), got L=%lld", who, L);
  LG_CHECK_ARG(rate >= 0.f && rate < 1.f, "%s: dropout rate %g outside [0, 1)", who, (double)rate);
  LG_CHECK_ARG(call >= 0 && call <= 3, "%s: dropout call slot %d outside 0..3", who, call);
  LG_CHECK_ARG(level >= 1 && level <= 4, "%s: dropout level %d outside 1..4", who, level);
  // rows r0 .. r0+B-1 must stay inside the level's window of 2^32 blocks: the next level's (and call's) masks start there
  LG_CHECK_ARG(r0 >= 0 && B > 0 && ((unsigned long long)r0 + (unsigned long long)B) * (unsigned long long)(L / 8) <= (1ull << 32),
               "%s: first row %d + %d rows of %lld elements leave the level's counter window", who, r0, B, L);
  const long long T = llrint((double)rate * 65536.0);
  LG_CHECK_ARG(T < 65536, "%s: dropout rate %g rounds to 1", who, (double)rate);
  dk->key = reinterpret_cast<const unsigned long long*>(key);
  dk->base = ((unsigned long long)call << 34) + ((unsigned long long)(level - 1) << 32) + (unsigned long long)r0 * (unsigned long long)(L / 8);
  dk->T = (unsigned)T;
  dk->scale = 65536.f / (float)(65536 - T);
  return LG_OK;
}

__global__ void dropout_key_kernel(unsigned long long* __restrict__ key, unsigned long long seed, unsigned long long key_offset) {
  if (threadIdx.x == 0) { key[0] = seed; key[1] = key_offset; }
}

}  // namespace

extern "C" const char* lg_instnorm_last_launches(void) {
  static thread_local char buf[NL_MAX * 96];
  size_t o = 0;
  buf[0] = 0;
  for (int i = 0; i < g_nl_n && i < NL_MAX; ++i) {
    if (i) buf[o++] = ';';
    for (const char* p = g_nl[i].name; *p && o + 32 < sizeof(buf); ++p)   // "(kernel<a, b>)" at the launch site -> "kernel<a,b>"
      if (*p != '(' && *p != ')' && *p != ' ') buf[o++] = *p;
    o += (size_t)snprintf(buf + o, sizeof(buf) - o, "[%u,%u]", g_nl[i].gx, g_nl[i].gy);
  }
  if (g_nl_n > NL_MAX) snprintf(buf + o, sizeof(buf) - o, ";...");
  return buf;
}

extern "C" int lg_instnorm_stats_stride(void) { return LG_NSTAT; }

extern "C" size_t lg_instnorm_workspace_bytes(int B, long long L) {
  const size_t gs = ((size_t)B * 2 * sizeof(double) + 255) / 256 * 256;
  return part_bytes(B, L) + bst_bytes(B) + gs;
}

// stats[B][8] = {mu_hi, sigma, a, beta, mu_lo, 0,0,0} of (pre_leaky ? leaky(x) : x), x = [B][L]
extern "C" int lg_instnorm_leaky_stats(const float* x, float* stats, const float* gamma, const float* beta,
                                       void* workspace, size_t ws_bytes, int B, long long L, int pre_leaky,
                                       float alpha, void* stream) {
  return lg_instnorm_leaky_stats_z16(x, stats, gamma, beta, workspace, ws_bytes, B, L, pre_leaky, alpha, nullptr, stream);
}
// x16_out (may be null): also writes bf16(x) there — the bf16 activation path's copy of a conv output whose kernel had no
// fused-moments epilogue (the fp32 x can then be dropped)
extern "C" int lg_instnorm_leaky_stats_z16(const float* x, float* stats, const float* gamma, const float* beta,
                                           void* workspace, size_t ws_bytes, int B, long long L, int pre_leaky,
                                           float alpha, void* x16_out, void* stream) {
  nl_reset();
  LG_CHECK_ARG(x && stats && gamma && beta && workspace, "lg_instnorm_leaky_stats: null pointer");
  LG_CHECK_ARG(B > 0 && B <= 65535 && L > 0 && L % 4 == 0, "lg_instnorm_leaky_stats: bad shape B=%d L=%lld", B, L);
  LG_CHECK_ARG(ws_bytes >= lg_instnorm_workspace_bytes(B, L), "lg_instnorm_leaky_stats: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int nc = nchunks(L);
  NORM_LAUNCH(stats_partial_kernel, dim3(nc, B), dim3(256), 0, st, x, (double*)workspace, L, nc, pre_leaky, alpha,
                     (__bf16*)x16_out);
  LG_CHECK_LAUNCH("lg_instnorm_leaky_stats(partial)");
  NORM_LAUNCH(stats_final_kernel, dim3(B), dim3(64), 0, st, (const double*)workspace, stats, gamma, beta, nc);
  LG_CHECK_LAUNCH("lg_instnorm_leaky_stats(final)");
  return LG_OK;
}

// stats from moment partials [B][nparts][3] doubles {count, mean, M2} produced by a conv epilogue (conv_halo.hip)
extern "C" int lg_instnorm_stats_finalize(const void* partials, int nparts, float* stats, const float* gamma,
                                          const float* beta, int B, void* stream) {
  nl_reset();
  LG_CHECK_ARG(partials && stats && gamma && beta && nparts > 0 && B > 0, "lg_instnorm_stats_finalize: bad arguments");
  NORM_LAUNCH(stats_final_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const double*)partials, stats, gamma,
                     beta, nparts);
  LG_CHECK_LAUNCH("lg_instnorm_stats_finalize");
  return LG_OK;
}

// y = [post_leaky] (a_n * ([pre_leaky](x) - mu_n) + beta) [+ skip]
static int apply_impl(const float* x, const float* stats, const float* skip, float* y, void* y16, int B, long long L, int pre_leaky,
                      int post_leaky, float alpha, const DropK* dk, void* stream) {
  nl_reset();
  LG_CHECK_ARG(x && stats && (y || y16), "lg_instnorm_leaky_apply: null pointer");
  LG_CHECK_ARG(B > 0 && L > 0 && L % 4 == 0 && (long long)B * L / 4 < (1LL << 31), "lg_instnorm_leaky_apply: bad shape B=%d L=%lld", B, L);
  const long long total4 = (long long)B * L / 4;
  if (dk) {
    NORM_LAUNCH(apply_drop_kernel, dim3((int)fit_rounds(ew_blocks(total4), LG_RESIDENT_BLOCKS(apply_drop_kernel), EW_MAX_BLOCKS, 1)), dim3(256), 0,
                       (hipStream_t)stream, x, stats, y, (__bf16*)y16, L / 4, total4, alpha, *dk);
    LG_CHECK_LAUNCH("lg_instnorm_leaky_apply_drop");
    return LG_OK;
  }
  NORM_LAUNCH(apply_kernel, dim3((int)fit_rounds(ew_blocks(total4), LG_RESIDENT_BLOCKS(apply_kernel), EW_MAX_BLOCKS, 1)), dim3(256), 0, (hipStream_t)stream, x, stats, skip, y,
                     (__bf16*)y16, L / 4, total4, pre_leaky, post_leaky, alpha);
  LG_CHECK_LAUNCH("lg_instnorm_leaky_apply");
  return LG_OK;
}
extern "C" int lg_instnorm_leaky_apply(const float* x, const float* stats, const float* skip, float* y, void* y16, int B,
                                       long long L, int pre_leaky, int post_leaky, float alpha, void* stream) {
  return apply_impl(x, stats, skip, y, y16, B, L, pre_leaky, post_leaky, alpha, nullptr, stream);
}
// y = LeakyReLU(a_n (x - mu_n) + beta) * keep * scale: the encoder's form with the dropout mask of (call, level), first row r0
extern "C" int lg_instnorm_leaky_apply_drop(const float* x, const float* stats, float* y, void* y16, int B, long long L, float alpha,
                                            const long long* key, int call, int level, int r0, float rate, void* stream) {
  DropK dk;
  if (int rc = drop_args("lg_instnorm_leaky_apply_drop", key, call, level, r0, B, L, rate, &dk)) return rc;
  return apply_impl(x, stats, nullptr, y, y16, B, L, 0, 1, alpha, &dk, stream);
}

// g = dL/d(apply output before skip); writes dx = dL/dx, (accumulates) dgamma, dbeta
// g: dL/dy as fp32, or as bf16 when g_is_bf16; dx and dx16: fp32 result and/or its bf16 mirror (at least one)
constexpr int DB_MAX_BLOCKS = 2046;  // multiple of 3: gridDim*256 must be a multiple of C/4 (C/4 = 96 for 384 channels)

extern "C" size_t lg_instnorm_bwd_db_workspace_bytes(int B, long long L, int C) {
  return lg_instnorm_workspace_bytes(B, L) + (size_t)DB_MAX_BLOCKS * (size_t)C * sizeof(float);
}

extern "C" int lg_instnorm_leaky_bwd(const float* x, const float* stats, const void* g, int g_is_bf16, float* dx, void* dx16,
                                     float* dgamma, float* dbeta, void* workspace, size_t ws_bytes, int B, long long L, int pre_leaky,
                                     int post_leaky, float alpha, int accumulate, void* stream) {
  return lg_instnorm_leaky_bwd_db(x, stats, g, g_is_bf16, dx, dx16, dgamma, dbeta, nullptr, 0, workspace, ws_bytes, B, L,
                                  pre_leaky, post_leaky, alpha, accumulate, stream);
}

// as lg_instnorm_leaky_bwd; db (may be null): db[C] (+)= column sums of dx viewed as [B*L/C][C] — the bias gradient of the
// conv layer whose output x is (C = its channel count, innermost), taken in the same pass that writes dx
static int bwd_impl(const float* x, const float* stats, const void* g, int g_is_bf16, float* dx, void* dx16,
                    float* dgamma, float* dbeta, float* db, int C, void* workspace, size_t ws_bytes, int B,
                    long long L, int pre_leaky, int post_leaky, float alpha, int accumulate, const DropK* dk, void* stream) {
  nl_reset();
  LG_CHECK_ARG(x && stats && g && (dx || dx16) && workspace, "lg_instnorm_leaky_bwd: null pointer");
  LG_CHECK_ARG(B > 0 && B <= 65535 && L > 0 && L % 4 == 0 && (long long)B * L / 4 < (1LL << 31),
               "lg_instnorm_leaky_bwd: bad shape B=%d L=%lld", B, L);
  LG_CHECK_ARG(ws_bytes >= lg_instnorm_workspace_bytes(B, L), "lg_instnorm_leaky_bwd: workspace too small");
  if (db) {
    LG_CHECK_ARG(C > 0 && C % 4 == 0 && C / 4 <= 256 && L % C == 0 && (256 % (C / 4) == 0 || 768 % (C / 4) == 0),
                 "lg_instnorm_leaky_bwd_db: unsupported channel count C=%d (L=%lld)", C, L);
    LG_CHECK_ARG(ws_bytes >= lg_instnorm_bwd_db_workspace_bytes(B, L, C), "lg_instnorm_leaky_bwd_db: workspace too small");
  }
  hipStream_t st = (hipStream_t)stream;
  int nc = 4096 / B;  // bwd_partial blocks per sample: ~4096 long-lived blocks in all (the buffer is sized for nchunks(L))
  if (nc < 1) nc = 1;
  if (nc > nchunks(L)) nc = nchunks(L);
  char* ws = (char*)workspace;
  double* partial = (double*)ws;
  float* bstats = (float*)(ws + part_bytes(B, L));
  double* gsum = (double*)(ws + part_bytes(B, L) + bst_bytes(B));
  if (dk)
    NORM_LAUNCH(bwd_partial_drop_kernel, dim3(nc, B), dim3(256), 0, st, x, g, g_is_bf16, stats, partial, L, nc, alpha, *dk);
  else
    NORM_LAUNCH(bwd_partial_kernel, dim3(nc, B), dim3(256), 0, st, x, g, g_is_bf16, stats, partial, L, nc, pre_leaky,
                       post_leaky, alpha);
  LG_CHECK_LAUNCH("lg_instnorm_leaky_bwd(partial)");
  NORM_LAUNCH(bwd_final_kernel, dim3(B), dim3(64), 0, st, (const double*)partial, stats, bstats, gsum, L, nc);
  LG_CHECK_LAUNCH("lg_instnorm_leaky_bwd(final)");
  if (dgamma && dbeta) {
    NORM_LAUNCH(bwd_affine_grad_kernel, dim3(1), dim3(256), 0, st, (const double*)gsum, dgamma, dbeta, B,
                       accumulate);
    LG_CHECK_LAUNCH("lg_instnorm_leaky_bwd(affine)");
  }
  const long long total4 = (long long)B * L / 4;
  if (!db) {
    if (dk)
      NORM_LAUNCH(bwd_apply_drop_kernel<false>, dim3((int)fit_rounds(ew_blocks(total4), LG_RESIDENT_BLOCKS(bwd_apply_drop_kernel<false>), EW_MAX_BLOCKS, 1)), dim3(256), 0, st, x, g,
                         g_is_bf16, stats, (const float*)bstats, dx, (__bf16*)dx16, L / 4, total4, alpha, (float*)nullptr, 0, *dk);
    else
      NORM_LAUNCH(bwd_apply_kernel<false>, dim3((int)fit_rounds(ew_blocks(total4), LG_RESIDENT_BLOCKS(bwd_apply_kernel<false>), EW_MAX_BLOCKS, 1)), dim3(256), 0, st, x, g, g_is_bf16, stats,
                         (const float*)bstats, dx, (__bf16*)dx16, L / 4, total4, pre_leaky, post_leaky, alpha, nullptr, 0);
    LG_CHECK_LAUNCH("lg_instnorm_leaky_bwd(apply)");
    return LG_OK;
  }
  const int C4 = C / 4, unit = 256 % C4 == 0 ? 1 : 3;  // blocks per period of the thread -> channel map
  // (the dropped twin takes its plain twin's grid: the column sums then merge in the same order)
  long long nb = fit_rounds((total4 + 255) / 256, LG_RESIDENT_BLOCKS(bwd_apply_kernel<true>), DB_MAX_BLOCKS, unit);
  float* colpart = (float*)(ws + lg_instnorm_workspace_bytes(B, L));
  if (dk)
    NORM_LAUNCH(bwd_apply_drop_kernel<true>, dim3((int)nb), dim3(256), 0, st, x, g, g_is_bf16, stats, (const float*)bstats, dx,
                       (__bf16*)dx16, L / 4, total4, alpha, colpart, C4, *dk);
  else
    NORM_LAUNCH(bwd_apply_kernel<true>, dim3((int)nb), dim3(256), 0, st, x, g, g_is_bf16, stats, (const float*)bstats, dx,
                       (__bf16*)dx16, L / 4, total4, pre_leaky, post_leaky, alpha, colpart, C4);
  LG_CHECK_LAUNCH("lg_instnorm_leaky_bwd_db(apply)");
  NORM_LAUNCH(colsum_final_kernel, dim3((C + 15) / 16), dim3(1024), 0, st, (const float*)colpart, db, (int)nb, C,
                     accumulate);
  LG_CHECK_LAUNCH("lg_instnorm_leaky_bwd_db(bias)");
  return LG_OK;
}
extern "C" int lg_instnorm_leaky_bwd_db(const float* x, const float* stats, const void* g, int g_is_bf16, float* dx, void* dx16,
                                        float* dgamma, float* dbeta, float* db, int C, void* workspace, size_t ws_bytes, int B,
                                        long long L, int pre_leaky, int post_leaky, float alpha, int accumulate, void* stream) {
  return bwd_impl(x, stats, g, g_is_bf16, dx, dx16, dgamma, dbeta, db, C, workspace, ws_bytes, B, L, pre_leaky, post_leaky, alpha,
                  accumulate, nullptr, stream);
}
// lg_instnorm_leaky_bwd_db of the encoder's form with g multiplied by the mask of (call, level), first row r0, in both passes
extern "C" int lg_instnorm_leaky_bwd_drop(const float* x, const float* stats, const void* g, int g_is_bf16, float* dx, void* dx16,
                                          float* dgamma, float* dbeta, float* db, int C, void* workspace, size_t ws_bytes, int B,
                                          long long L, float alpha, int accumulate, const long long* key, int call, int level, int r0,
                                          float rate, void* stream) {
  DropK dk;
  if (int rc = drop_args("lg_instnorm_leaky_bwd_drop", key, call, level, r0, B, L, rate, &dk)) return rc;
  return bwd_impl(x, stats, g, g_is_bf16, dx, dx16, dgamma, dbeta, db, C, workspace, ws_bytes, B, L, 0, 1, alpha, accumulate, &dk, stream);
}

// ---- bf16 activation path: the same ops reading the conv output z as bf16 (see the kernels above) -------------------
// skip (may be null): fp32, or bf16 when skip_is_bf16
static int apply16_impl(const void* z16, const float* stats, const void* skip, int skip_is_bf16, float* y, void* y16, int B, long long L,
                        int pre_leaky, int post_leaky, float alpha, const DropK* dk, void* stream) {
  nl_reset();
  LG_CHECK_ARG(z16 && stats && (y || y16), "lg_instnorm_leaky_apply_z16: null pointer");
  LG_CHECK_ARG(B > 0 && L > 0 && L % 8 == 0 && (long long)B * L / 8 < (1LL << 31),
               "lg_instnorm_leaky_apply_z16: bad shape B=%d L=%lld", B, L);
  const long long total8 = (long long)B * L / 8;
  long long nb = (total8 + 256 * EW8_UNR - 1) / (256 * EW8_UNR);
  nb = fit_rounds(nb, !skip ? LG_RESIDENT_BLOCKS(apply16_kernel<0>) : !skip_is_bf16 ? LG_RESIDENT_BLOCKS(apply16_kernel<1>) : LG_RESIDENT_BLOCKS(apply16_kernel<2>), EW_MAX_BLOCKS, 1);
  hipStream_t st = (hipStream_t)stream;
  const __bf16* x = (const __bf16*)z16;
  if (dk) {
    nb = fit_rounds((total8 + 256 * EW8_UNR - 1) / (256 * EW8_UNR), LG_RESIDENT_BLOCKS(apply16_drop_kernel), EW_MAX_BLOCKS, 1);
    NORM_LAUNCH(apply16_drop_kernel, dim3((int)nb), dim3(256), 0, st, x, stats, y, (__bf16*)y16, L / 8, total8, alpha, *dk);
    LG_CHECK_LAUNCH("lg_instnorm_leaky_apply_z16_drop");
    return LG_OK;
  }
  if (!skip)
    NORM_LAUNCH(apply16_kernel<0>, dim3((int)nb), dim3(256), 0, st, x, stats, skip, y, (__bf16*)y16, L / 8, total8,
                       pre_leaky, post_leaky, alpha);
  else if (!skip_is_bf16)
    NORM_LAUNCH(apply16_kernel<1>, dim3((int)nb), dim3(256), 0, st, x, stats, skip, y, (__bf16*)y16, L / 8, total8,
                       pre_leaky, post_leaky, alpha);
  else
    NORM_LAUNCH(apply16_kernel<2>, dim3((int)nb), dim3(256), 0, st, x, stats, skip, y, (__bf16*)y16, L / 8, total8,
                       pre_leaky, post_leaky, alpha);
  LG_CHECK_LAUNCH("lg_instnorm_leaky_apply_z16");
  return LG_OK;
}
extern "C" int lg_instnorm_leaky_apply_z16(const void* z16, const float* stats, const void* skip, int skip_is_bf16, float* y,
                                           void* y16, int B, long long L, int pre_leaky, int post_leaky, float alpha,
                                           void* stream) {
  return apply16_impl(z16, stats, skip, skip_is_bf16, y, y16, B, L, pre_leaky, post_leaky, alpha, nullptr, stream);
}
// lg_instnorm_leaky_apply_drop reading the conv output as bf16
extern "C" int lg_instnorm_leaky_apply_z16_drop(const void* z16, const float* stats, float* y, void* y16, int B, long long L, float alpha,
                                                const long long* key, int call, int level, int r0, float rate, void* stream) {
  DropK dk;
  if (int rc = drop_args("lg_instnorm_leaky_apply_z16_drop", key, call, level, r0, B, L, rate, &dk)) return rc;
  return apply16_impl(z16, stats, nullptr, 0, y, y16, B, L, 0, 1, alpha, &dk, stream);
}

// lg_instnorm_stats_finalize + lg_instnorm_leaky_apply_z16 in ONE launch (see apply16p_kernel): `partials` = the [B][nparts][3]
// moment records a *_fwd_stats conv left behind; `stats` [B][8] receives the finished records (bit-identical to the two-call form)
static int apply16p_impl(const void* z16, const void* partials, int nparts, const float* gamma, const float* beta, float* stats,
                         const void* skip, int skip_is_bf16, float* y, void* y16, int B, long long L, int post_leaky, float alpha,
                         const DropK* dk, void* stream) {
  nl_reset();
  LG_CHECK_ARG(z16 && partials && gamma && beta && stats && (y || y16), "lg_instnorm_leaky_apply_z16_p: null pointer");
  LG_CHECK_ARG(nparts > 0 && B > 0 && B <= 65535 && L > 0 && L % 8 == 0 && L / 8 < (1LL << 31),
               "lg_instnorm_leaky_apply_z16_p: bad shape B=%d L=%lld nparts=%d", B, L, nparts);
  const long long L8 = L / 8;
  long long bps = (L8 + 256 * EW8_UNR * 4 - 1) / (256 * EW8_UNR * 4);   // ~4 trips per block: the merge is paid once per 32 KB of z
  if (bps * B > EW_MAX_BLOCKS) bps = EW_MAX_BLOCKS / B;
  if (bps < 1) bps = 1;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)bps, (unsigned)B);
  const __bf16* x = (const __bf16*)z16;
  const double* pr = (const double*)partials;
  if (dk)
    NORM_LAUNCH(apply16p_drop_kernel, grid, dim3(256), 0, st, x, pr, nparts, gamma, beta, stats, y, (__bf16*)y16, (unsigned)L8, alpha, *dk);
  else if (!skip)
    NORM_LAUNCH(apply16p_kernel<0>, grid, dim3(256), 0, st, x, pr, nparts, gamma, beta, stats, skip, y, (__bf16*)y16, (unsigned)L8, post_leaky, alpha);
  else if (!skip_is_bf16)
    NORM_LAUNCH(apply16p_kernel<1>, grid, dim3(256), 0, st, x, pr, nparts, gamma, beta, stats, skip, y, (__bf16*)y16, (unsigned)L8, post_leaky, alpha);
  else
    NORM_LAUNCH(apply16p_kernel<2>, grid, dim3(256), 0, st, x, pr, nparts, gamma, beta, stats, skip, y, (__bf16*)y16, (unsigned)L8, post_leaky, alpha);
  LG_CHECK_LAUNCH("lg_instnorm_leaky_apply_z16_p");
  return LG_OK;
}
extern "C" int lg_instnorm_leaky_apply_z16_p(const void* z16, const void* partials, int nparts, const float* gamma, const float* beta,
                                             float* stats, const void* skip, int skip_is_bf16, float* y, void* y16, int B,
                                             long long L, int post_leaky, float alpha, void* stream) {
  return apply16p_impl(z16, partials, nparts, gamma, beta, stats, skip, skip_is_bf16, y, y16, B, L, post_leaky, alpha, nullptr, stream);
}
// lg_instnorm_leaky_apply_z16_p (statistics finalised in the same launch) with the dropout mask
extern "C" int lg_instnorm_leaky_apply_z16_p_drop(const void* z16, const void* partials, int nparts, const float* gamma, const float* beta,
                                                  float* stats, float* y, void* y16, int B, long long L, float alpha,
                                                  const long long* key, int call, int level, int r0, float rate, void* stream) {
  DropK dk;
  if (int rc = drop_args("lg_instnorm_leaky_apply_z16_p_drop", key, call, level, r0, B, L, rate, &dk)) return rc;
  return apply16p_impl(z16, partials, nparts, gamma, beta, stats, nullptr, 0, y, y16, B, L, 1, alpha, &dk, stream);
}

// as lg_instnorm_leaky_bwd_db with x given as bf16 (workspace: lg_instnorm_bwd_db_workspace_bytes)
extern "C" int lg_instnorm_leaky_bwd_z16(const void* z16, const float* stats, const void* g, int g_is_bf16, float* dx,
                                         void* dx16, float* dgamma, float* dbeta, float* db, int C, void* workspace,
                                         size_t ws_bytes, int B, long long L, int pre_leaky, int post_leaky, float alpha,
                                         int accumulate, void* stream) {
  return lg_instnorm_leaky_bwd_z16_p(z16, stats, g, g_is_bf16, dx, dx16, dgamma, dbeta, db, C, nullptr, 0, workspace, ws_bytes, B, L,
                                     pre_leaky, post_leaky, alpha, accumulate, stream);
}
// partials / nparts_in (optional): the per-sample sums {sum g', sum g' c} as [B][nparts_in][2] doubles, already produced by
// the epilogue of the conv that wrote g (lg_conv2d_s2_dgrad_nf, ...): the first (partial-sums) pass over z and g is skipped
static int bwd16_impl(const void* z16, const float* stats, const void* g, int g_is_bf16, float* dx, void* dx16, float* dgamma, float* dbeta,
                      float* db, int C, const void* partials, int nparts_in, void* workspace, size_t ws_bytes, int B, long long L,
                      int pre_leaky, int post_leaky, float alpha, int accumulate, const DropK* dk, void* stream) {
  nl_reset();
  LG_CHECK_ARG(z16 && stats && g && (dx || dx16) && workspace, "lg_instnorm_leaky_bwd_z16: null pointer");
  // producer-fused sums are those of the UNMASKED gradient: with a mask they are right only when it keeps everything (T = 0)
  LG_CHECK_ARG(!(dk && partials && nparts_in > 0 && dk->T != 0), "lg_instnorm_leaky_bwd_z16_drop: fused partial sums know no dropout mask");
  LG_CHECK_ARG(B > 0 && B <= 65535 && L > 0 && L % 8 == 0 && (long long)B * L / 8 < (1LL << 31),
               "lg_instnorm_leaky_bwd_z16: bad shape B=%d L=%lld", B, L);
  LG_CHECK_ARG(ws_bytes >= lg_instnorm_workspace_bytes(B, L), "lg_instnorm_leaky_bwd_z16: workspace too small");
  // producer-fused sums (lg_nf_accum, lg_common.h) are those of the post-LeakyReLU form only; the caller must pass the alpha
  // the producer used (the record carries none)
  LG_CHECK_ARG(!(partials && nparts_in > 0) || (pre_leaky == 0 && post_leaky == 1),
               "lg_instnorm_leaky_bwd_z16_p: fused partial sums exist for pre_leaky=0, post_leaky=1 only (got %d, %d)", pre_leaky, post_leaky);
  if (db) {
    LG_CHECK_ARG(C > 0 && C % 8 == 0 && C / 8 <= 256 && L % C == 0 && (256 % (C / 8) == 0 || 768 % (C / 8) == 0),
                 "lg_instnorm_leaky_bwd_z16: unsupported channel count C=%d (L=%lld)", C, L);
    LG_CHECK_ARG(ws_bytes >= lg_instnorm_bwd_db_workspace_bytes(B, L, C), "lg_instnorm_leaky_bwd_z16: workspace too small");
  }
  hipStream_t st = (hipStream_t)stream;
  const __bf16* x = (const __bf16*)z16;
  int nc = 4096 / B;
  if (nc < 1) nc = 1;
  const int nch8 = (int)((L + 2 * CHUNK - 1) / (2 * CHUNK));
  if (nc > nch8) nc = nch8;   // nch8 <= nchunks(L): the partial buffer is large enough
  char* ws = (char*)workspace;
  double* partial = (double*)ws;
  float* bstats = (float*)(ws + part_bytes(B, L));
  double* gsum = (double*)(ws + part_bytes(B, L) + bst_bytes(B));
  if (partials && nparts_in > 0) {  // sums fused into the producer of g
    partial = (double*)partials;
    nc = nparts_in;
  } else {
    if (dk && g_is_bf16)
      NORM_LAUNCH(bwd_partial16_drop_kernel<true>, dim3(nc, B), dim3(256), 0, st, x, g, stats, partial, L, nc, alpha, *dk);
    else if (dk)
      NORM_LAUNCH(bwd_partial16_drop_kernel<false>, dim3(nc, B), dim3(256), 0, st, x, g, stats, partial, L, nc, alpha, *dk);
    else if (g_is_bf16)
      NORM_LAUNCH(bwd_partial16_kernel<true>, dim3(nc, B), dim3(256), 0, st, x, g, stats, partial, L, nc, pre_leaky,
                         post_leaky, alpha);
    else
      NORM_LAUNCH(bwd_partial16_kernel<false>, dim3(nc, B), dim3(256), 0, st, x, g, stats, partial, L, nc, pre_leaky,
                         post_leaky, alpha);
    LG_CHECK_LAUNCH("lg_instnorm_leaky_bwd_z16(partial)");
  }
  NORM_LAUNCH(bwd_final_kernel, dim3(B), dim3(64), 0, st, (const double*)partial, stats, bstats, gsum, L, nc);
  LG_CHECK_LAUNCH("lg_instnorm_leaky_bwd_z16(final)");
  if (dgamma && dbeta) {
    NORM_LAUNCH(bwd_affine_grad_kernel, dim3(1), dim3(256), 0, st, (const double*)gsum, dgamma, dbeta, B, accumulate);
    LG_CHECK_LAUNCH("lg_instnorm_leaky_bwd_z16(affine)");
  }
  const long long total8 = (long long)B * L / 8;
  if (!db) {
    long long nb = (total8 + 256 * EW8_UNR - 1) / (256 * EW8_UNR);
    if (dk)
      nb = fit_rounds(nb, g_is_bf16 ? LG_RESIDENT_BLOCKS((bwd_apply16_drop_kernel<false, true>)) : LG_RESIDENT_BLOCKS((bwd_apply16_drop_kernel<false, false>)), EW_MAX_BLOCKS, 1);
    else
      nb = fit_rounds(nb, g_is_bf16 ? LG_RESIDENT_BLOCKS((bwd_apply16_kernel<false, true>)) : LG_RESIDENT_BLOCKS((bwd_apply16_kernel<false, false>)), EW_MAX_BLOCKS, 1);
    if (dk && g_is_bf16)
      NORM_LAUNCH((bwd_apply16_drop_kernel<false, true>), dim3((int)nb), dim3(256), 0, st, x, g, stats, (const float*)bstats, dx,
                         (__bf16*)dx16, L / 8, total8, alpha, (float*)nullptr, 0, *dk);
    else if (dk)
      NORM_LAUNCH((bwd_apply16_drop_kernel<false, false>), dim3((int)nb), dim3(256), 0, st, x, g, stats, (const float*)bstats, dx,
                         (__bf16*)dx16, L / 8, total8, alpha, (float*)nullptr, 0, *dk);
    else if (g_is_bf16)
      NORM_LAUNCH((bwd_apply16_kernel<false, true>), dim3((int)nb), dim3(256), 0, st, x, g, stats, (const float*)bstats, dx,
                         (__bf16*)dx16, L / 8, total8, pre_leaky, post_leaky, alpha, (float*)nullptr, 0);
    else
      NORM_LAUNCH((bwd_apply16_kernel<false, false>), dim3((int)nb), dim3(256), 0, st, x, g, stats, (const float*)bstats, dx,
                         (__bf16*)dx16, L / 8, total8, pre_leaky, post_leaky, alpha, (float*)nullptr, 0);
    LG_CHECK_LAUNCH("lg_instnorm_leaky_bwd_z16(apply)");
    return LG_OK;
  }
  const int C8 = C / 8, unit = 256 % C8 == 0 ? 1 : 3;
  long long nb = (total8 + 511) / 512;   // two units per thread per trip
  nb = fit_rounds(nb, g_is_bf16 ? LG_RESIDENT_BLOCKS((bwd_apply16_kernel<true, true>)) : LG_RESIDENT_BLOCKS((bwd_apply16_kernel<true, false>)), DB_MAX_BLOCKS, unit);
  float* colpart = (float*)(ws + lg_instnorm_workspace_bytes(B, L));   // [nb][C] floats, nb <= DB_MAX_BLOCKS (+2)
  // (the dropped twins take their plain twins' grid: the column sums then merge in the same order)
  if (dk && g_is_bf16)
    NORM_LAUNCH((bwd_apply16_drop_kernel<true, true>), dim3((int)nb), dim3(256), 0, st, x, g, stats, (const float*)bstats, dx,
                       (__bf16*)dx16, L / 8, total8, alpha, colpart, C8, *dk);
  else if (dk)
    NORM_LAUNCH((bwd_apply16_drop_kernel<true, false>), dim3((int)nb), dim3(256), 0, st, x, g, stats, (const float*)bstats, dx,
                       (__bf16*)dx16, L / 8, total8, alpha, colpart, C8, *dk);
  else if (g_is_bf16)
    NORM_LAUNCH((bwd_apply16_kernel<true, true>), dim3((int)nb), dim3(256), 0, st, x, g, stats, (const float*)bstats, dx,
                       (__bf16*)dx16, L / 8, total8, pre_leaky, post_leaky, alpha, colpart, C8);
  else
    NORM_LAUNCH((bwd_apply16_kernel<true, false>), dim3((int)nb), dim3(256), 0, st, x, g, stats, (const float*)bstats, dx,
                       (__bf16*)dx16, L / 8, total8, pre_leaky, post_leaky, alpha, colpart, C8);
  LG_CHECK_LAUNCH("lg_instnorm_leaky_bwd_z16(apply+bias)");
  NORM_LAUNCH(colsum_final_kernel, dim3((C + 15) / 16), dim3(1024), 0, st, (const float*)colpart, db, (int)nb, C,
                     accumulate);
  LG_CHECK_LAUNCH("lg_instnorm_leaky_bwd_z16(bias)");
  return LG_OK;
}
extern "C" int lg_instnorm_leaky_bwd_z16_p(const void* z16, const float* stats, const void* g, int g_is_bf16, float* dx,
                                           void* dx16, float* dgamma, float* dbeta, float* db, int C, const void* partials,
                                           int nparts_in, void* workspace, size_t ws_bytes, int B, long long L, int pre_leaky,
                                           int post_leaky, float alpha, int accumulate, void* stream) {
  return bwd16_impl(z16, stats, g, g_is_bf16, dx, dx16, dgamma, dbeta, db, C, partials, nparts_in, workspace, ws_bytes, B, L, pre_leaky,
                    post_leaky, alpha, accumulate, nullptr, stream);
}
// lg_instnorm_leaky_bwd_drop reading the conv output as bf16.  partials / nparts_in as lg_instnorm_leaky_bwd_z16_p: accepted only
// where the mask keeps everything (rate rounds to T = 0) — producer-fused sums are those of the unmasked gradient
extern "C" int lg_instnorm_leaky_bwd_z16_drop(const void* z16, const float* stats, const void* g, int g_is_bf16, float* dx, void* dx16,
                                              float* dgamma, float* dbeta, float* db, int C, const void* partials, int nparts_in,
                                              void* workspace, size_t ws_bytes, int B, long long L, float alpha, int accumulate,
                                              const long long* key, int call, int level, int r0, float rate, void* stream) {
  DropK dk;
  if (int rc = drop_args("lg_instnorm_leaky_bwd_z16_drop", key, call, level, r0, B, L, rate, &dk)) return rc;
  return bwd16_impl(z16, stats, g, g_is_bf16, dx, dx16, dgamma, dbeta, db, C, partials, nparts_in, workspace, ws_bytes, B, L, 0, 1, alpha,
                    accumulate, &dk, stream);
}

// key[2] = {seed, key_offset} written on the device from launch scalars: the step's key without a host-to-device copy (no sync)
extern "C" int lg_dropout_key(long long* key, unsigned long long seed, unsigned long long key_offset, void* stream) {
  nl_reset();
  LG_CHECK_ARG(key && ((uintptr_t)key & 7) == 0, "lg_dropout_key: null or misaligned pointer");
  NORM_LAUNCH(dropout_key_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<unsigned long long*>(key), seed, key_offset);
  LG_CHECK_LAUNCH("lg_dropout_key");
  return LG_OK;
}

// keep[B][L] bytes (1 = kept) of the rows r0 .. r0+B-1 of the (call, level) slot under `key` = device {seed, key_offset}
extern "C" int lg_dropout_mask(const long long* key, int call, int level, int r0, int B, long long L, float rate, unsigned char* keep,
                               void* stream) {
  nl_reset();
  LG_CHECK_ARG(keep, "lg_dropout_mask: null pointer");
  LG_CHECK_ARG(((uintptr_t)keep & 7) == 0, "lg_dropout_mask: keep must be 8-byte aligned (8 decisions per store)");
  LG_CHECK_ARG(B > 0 && L > 0 && (long long)B * L / 8 < (1LL << 31), "lg_dropout_mask: bad shape B=%d L=%lld", B, L);
  DropK dk;
  if (int rc = drop_args("lg_dropout_mask", key, call, level, r0, B, L, rate, &dk)) return rc;
  const long long total8 = (long long)B * L / 8;
  long long nb = (total8 + 255) / 256;
  if (nb > EW_MAX_BLOCKS) nb = EW_MAX_BLOCKS;
  NORM_LAUNCH(dropout_mask_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, keep, total8, dk);
  LG_CHECK_LAUNCH("lg_dropout_mask");
  return LG_OK;
}

// The norm backward WITHOUT its apply pass: coef[B][8] (see bwd_coef_kernel) from the statistics records and the sums
// {sum g', sum g' c} the producer of g left as [B][nparts][2] doubles (lg_*_dgrad_nf).  The consumer of dz — the next data-gradient
// conv (lg_convT_s2_dgrad_bn) — forms dz = a (g' - m1 - c m2') while it stages its operand: dz is never written.  For tapes that
// ask the level for no weight gradient (dz then has ONE reader).  instance.py:105-128 differentiated; eager_trainer.py:158-163.
extern "C" int lg_instnorm_bwd_coef(const float* stats, const void* partials, int nparts, float* coef, int B, long long L,
                                    void* stream) {
  nl_reset();
  LG_CHECK_ARG(stats && partials && coef && nparts > 0 && B > 0 && B <= 65535 && L > 0, "lg_instnorm_bwd_coef: bad arguments");
  NORM_LAUNCH(bwd_coef_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const double*)partials, stats, coef, L, nparts);
  LG_CHECK_LAUNCH("lg_instnorm_bwd_coef");
  return LG_OK;
}
