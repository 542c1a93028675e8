// A faded Gaussian blur of every image the Discriminator reads (the reference has none): a separable FIR of up to 61 taps
// on [rows, S, S, 3] fp32, its sigma read from 16 bytes of device state that one launch at the top of the step advances.  A captured
// graph bakes launch scalars in; sigma, and with it the radius and the taps, come from the state, so a replayed step blurs by ITS sigma.
// The operator is its own adjoint, so lgblur_apply serves the forward and the backward.  The definition is stated in include/littlegan_blur.h and
// restated on the host by config.blur_restate.
//
// lgblur_apply: a workgroup of 256 threads owns a strip of the image TW = 32 pixels wide and walks down it in chunks of CH = 32 rows; per
// chunk three phases through LDS:
//   stage   the chunk's rows of the input, TW + 2R columns widened to whole 4-pixel groups, 16-byte loads, zeros where the row ends
//   H       LDS -> LDS: a thread owns 4 consecutive pixels of one channel of one row and slides over the 2R + 4 sources they share: one
//           data read per 4 multiply-adds, every output's taps in ascending order.  The filtered rows go into a ring of three chunks
//   V       of the tile one chunk back (its rows above and below are in the ring by now: R <= CH), LDS -> registers -> global: a thread
//           owns a 16-byte column group of 4 consecutive tile rows, one 16-byte LDS read per 16 multiply-adds, 16-byte stores
// so every image row is filtered horizontally once.  The chunks before the first and after the last row are zeros.  A zero-filled
// source adds +0 to a sum that started from +0, which changes no bit: the strip and chunk geometry is not visible in the result.
#include "lg_internal.h"

namespace {

constexpr int DB_THREADS = 256;
constexpr int DB_TW = 32;                                    // strip width, pixels; S % 8 == 0 keeps a clipped strip a multiple of 8
constexpr int DB_CH = 32;                                    // rows of a chunk and of an output tile
constexpr int DB_R = DBLUR_MAX_RADIUS;                       // 30 <= DB_CH: a tile's taps reach into the chunk above and the one below
constexpr int DB_RING = 3 * DB_CH;                           // filtered rows kept: image row y lives in ring row (y + DB_RING) % DB_RING
constexpr int DB_WPX = DB_TW + 2 * ((DB_R + 3) / 4 * 4);     // 96 window pixels: x0 - R floored, x0 + TW + R raised to 4-pixel groups
constexpr int DB_IN_STRIDE = DB_WPX * 3 + 4;                 // 292 floats: 16-byte rows, 4 banks apart
constexpr int DB_HS_STRIDE = DB_TW * 3 + 4;                  // 100 floats
constexpr int DB_WX = 64;                                    // wx[u] = w_|u - R|, u = 0..2R
constexpr int DB_LDS_FLOATS = DB_WX + DB_CH * DB_IN_STRIDE + DB_RING * DB_HS_STRIDE;
constexpr size_t DB_LDS_BYTES = (size_t)DB_LDS_FLOATS * sizeof(float) + (DB_R + 1) * sizeof(double);   // 76,280: two workgroups a CU
static_assert(DB_R <= DB_CH, "a tile's taps must stay within the neighbouring chunks");

// R of the definition, for any bits: a sigma that is NaN, +-Inf, zero or negative gives 0; the product is compared as a float before the
// conversion, so the conversion is always defined
__device__ __forceinline__ int blur_radius(float sigma) {
  if (!(sigma > 0.f && sigma <= 3.402823466e38f)) return 0;
  const float t = 3.0f * sigma;
  return t >= (float)DB_R ? DB_R : (int)floorf(t);
}

__global__ void dblur_init_kernel(float* __restrict__ state, int k0) {
  if (threadIdx.x != 0) return;
  reinterpret_cast<f32x4*>(state)[0] = f32x4{__int_as_float(k0), 0.f, 0.f, 0.f};   // +0.f is the int32 0
}

// fp64 throughout, basic operations only, then ONE conversion to fp32
__global__ void dblur_step_kernel(float* __restrict__ state, float sigma0, long long n, long long F) {
  if (threadIdx.x != 0) return;
  const int k = __float_as_int(state[0]);
  const long long kk = k > 0 ? k : 0;
  const double left = 1.0 - (double)(kk * n) / (double)F;
  const float sigma = (float)((double)sigma0 * (left > 0.0 ? left : 0.0));
  const int k1 = k < 0x7fffffff ? k + 1 : k;
  reinterpret_cast<f32x4*>(state)[0] = f32x4{__int_as_float(k1), sigma, 0.f, 0.f};
}

__global__ __launch_bounds__(DB_THREADS) void dblur_apply_kernel(const float* __restrict__ xin, const float* __restrict__ state,
                                                                 float* __restrict__ out, int rows, int S) {
  extern __shared__ __attribute__((aligned(16))) float db_lds[];
  const int tid = threadIdx.x;
  const float sigma = state[1];
  const int R = __builtin_amdgcn_readfirstlane(blur_radius(sigma));   // device data, the same in every lane: one scalar

  if (R == 0) {   // the copy: x bit for bit
    const long long n4 = (long long)rows * S * S * 3 / 4, stride = (long long)gridDim.x * DB_THREADS;
    const f32x4* s4 = reinterpret_cast<const f32x4*>(xin);
    f32x4* d4 = reinterpret_cast<f32x4*>(out);
    for (long long i = (long long)blockIdx.x * DB_THREADS + tid; i < n4; i += stride) d4[i] = s4[i];
    return;
  }

  float* wx = db_lds;                                // [2R + 1] of DB_WX
  float* in = db_lds + DB_WX;                        // [DB_CH][DB_IN_STRIDE]
  float* hs = in + DB_CH * DB_IN_STRIDE;             // [DB_RING][DB_HS_STRIDE]
  double* tt = reinterpret_cast<double*>(hs + DB_RING * DB_HS_STRIDE);   // [R + 1]; the float regions before it are a multiple of 8 bytes

  // taps, once per workgroup: t_i by thread i, then Z summed in ascending i by each of them (the same additions, the same Z)
  if (tid <= R) {
    const double q = (double)tid / (double)sigma;
    tt[tid] = exp2(-(q * q));
  }
  __syncthreads();
  if (tid <= R) {
    double rest = 0.0;
    for (int i = 1; i <= R; ++i) rest += tt[i];
    const float w = (float)(tt[tid] / (tt[0] + 2.0 * rest));
    wx[R + tid] = w;
    wx[R - tid] = w;
  }
  // (the first barrier of the strip loop orders these stores before the first read of wx)

  const int tilesX = (S + DB_TW - 1) / DB_TW, T = (S + DB_CH - 1) / DB_CH;
  const long long total = (long long)rows * tilesX;
  const int rowF = S * 3;   // floats of an image row: a multiple of 24
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long long strip = blockIdx.x; strip < total; strip += gridDim.x) {
    const int n = (int)(strip / tilesX), x0 = (int)(strip % tilesX) * DB_TW;
    const int tw = min(DB_TW, S - x0);                                   // a multiple of 8
    const int xs = (x0 - R) & ~3, xe = (x0 + tw + R + 3) & ~3;           // window columns [xs, xe): whole 4-pixel groups, xs may be < 0
    const int nF4 = (xe - xs) * 3 / 4, ncg = tw * 3 / 4, nq = tw / 4;    // <= 72 16-byte groups a window row, <= 24 a strip row
    const int base_px = x0 - xs - R;                                     // >= 0: window pixel of the first source of pixel x0
    const float* img = xin + (long long)n * S * rowF;
    __syncthreads();   // the previous strip's last V has read the ring
    // the chunk above the image (rows -CH .. -1, ring rows 2 CH ..): zeros
    for (int idx = tid; idx < DB_CH * ncg; idx += DB_THREADS)
      *reinterpret_cast<f32x4*>(hs + (2 * DB_CH + idx / ncg) * DB_HS_STRIDE + 4 * (idx % ncg)) = zero4;

    for (int c = 0; c <= T; ++c) {   // chunk c = image rows c CH .. c CH + cr - 1; chunk T lies below the image
      const int cr = c < T ? min(DB_CH, S - c * DB_CH) : 0, ring0 = (c % 3) * DB_CH;
      // ---- stage: a 16-byte group lies wholly inside the image row or wholly outside it (xs * 3 and rowF are multiples of 4)
      for (int idx = tid; idx < cr * nF4; idx += DB_THREADS) {
        const int ry = idx / nF4, m = idx - ry * nF4, fc = xs * 3 + 4 * m;
        f32x4 v = zero4;
        if ((unsigned)fc < (unsigned)rowF) v = *reinterpret_cast<const f32x4*>(img + (long long)(c * DB_CH + ry) * rowF + fc);
        *reinterpret_cast<f32x4*>(in + ry * DB_IN_STRIDE + 4 * m) = v;
      }
      __syncthreads();   // the stage is visible; the V of the last round has read the ring rows that this round overwrites

      // ---- H: item = (channel ch, chunk row ry, 4-pixel group q), ch fastest, then ry.  Source u = s + R of the group's first pixel
      // runs over 0 .. 2R + 3; output j takes it with tap index u - j of wx when that lies in 0 .. 2R: all four do for 3 <= u <= 2R,
      // j <= u before, j >= u - 2R after.
      for (int idx = tid; idx < 3 * cr * nq; idx += DB_THREADS) {
        const int ch = idx % 3, t2 = idx / 3, ry = t2 % cr, q = t2 / cr;
        const float* p = in + ry * DB_IN_STRIDE + (base_px + 4 * q) * 3 + ch;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          const float v = p[3 * u];
          a0 += wx[u] * v;
          if (u >= 1) a1 += wx[u - 1] * v;
          if (u >= 2) a2 += wx[u - 2] * v;
        }
        float w1 = wx[2], w2 = wx[1], w3 = wx[0];
#pragma unroll 4
        for (int u = 3; u <= 2 * R; ++u) {
          const float v = p[3 * u], w0 = wx[u];
          a0 += w0 * v; a1 += w1 * v; a2 += w2 * v; a3 += w3 * v;
          w3 = w2; w2 = w1; w1 = w0;
        }
#pragma unroll
        for (int e = 1; e <= 3; ++e) {
          const int u = 2 * R + e;
          const float v = p[3 * u];
          if (e <= 1) a1 += wx[u - 1] * v;
          if (e <= 2) a2 += wx[u - 2] * v;
          a3 += wx[u - 3] * v;
        }
        float* h = hs + (ring0 + ry) * DB_HS_STRIDE + 12 * q + ch;
        h[0] = a0; h[3] = a1; h[6] = a2; h[9] = a3;
      }
      // the chunk's rows below the image: zeros
      for (int idx = tid; idx < (DB_CH - cr) * ncg; idx += DB_THREADS)
        *reinterpret_cast<f32x4*>(hs + (ring0 + cr + idx / ncg) * DB_HS_STRIDE + 4 * (idx % ncg)) = zero4;
      __syncthreads();
      if (c == 0) continue;

      // ---- V of the tile one chunk back: item = (16-byte column group cg, block of 4 tile rows rb), cg fastest.  Filtered row u of
      // the block's first output row, image row y0 + 4 rb - R + u, runs over 0 .. 2R + 3, as above.
      const int y0 = (c - 1) * DB_CH, th = min(DB_CH, S - y0);
      float* dst0 = out + ((long long)n * S + y0) * rowF + x0 * 3;
      for (int idx = tid; idx < ncg * (th / 4); idx += DB_THREADS) {
        const int cg = idx % ncg, rb = idx / ncg;
        const int r0 = (y0 + 4 * rb - R + DB_RING) % DB_RING;   // y0 - R >= -CH
        const float* p = hs + 4 * cg;
        auto row = [&](int u) {
          const int r = r0 + u;   // < 2 DB_RING
          return *reinterpret_cast<const f32x4*>(p + (r >= DB_RING ? r - DB_RING : r) * DB_HS_STRIDE);
        };
        f32x4 a0 = zero4, a1 = zero4, a2 = zero4, a3 = zero4;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          const f32x4 v = row(u);
          a0 += wx[u] * v;
          if (u >= 1) a1 += wx[u - 1] * v;
          if (u >= 2) a2 += wx[u - 2] * v;
        }
        float w1 = wx[2], w2 = wx[1], w3 = wx[0];
#pragma unroll 4
        for (int u = 3; u <= 2 * R; ++u) {
          const f32x4 v = row(u);
          const float w0 = wx[u];
          a0 += w0 * v; a1 += w1 * v; a2 += w2 * v; a3 += w3 * v;
          w3 = w2; w2 = w1; w1 = w0;
        }
#pragma unroll
        for (int e = 1; e <= 3; ++e) {
          const int u = 2 * R + e;
          const f32x4 v = row(u);
          if (e <= 1) a1 += wx[u - 1] * v;
          if (e <= 2) a2 += wx[u - 2] * v;
          a3 += wx[u - 3] * v;
        }
        float* d = dst0 + (long long)(4 * rb) * rowF + 4 * cg;
        *reinterpret_cast<f32x4*>(d) = a0;
        *reinterpret_cast<f32x4*>(d + rowF) = a1;
        *reinterpret_cast<f32x4*>(d + 2 * rowF) = a2;
        *reinterpret_cast<f32x4*>(d + 3 * rowF) = a3;
      }
      // (no barrier here: the next round's stage writes `in`, which V does not read, and its H waits behind the barrier after the stage)
    }
  }
}

}  // namespace

extern "C" int lgblur_init(float* state, long long k0, void* stream) {
  LG_CHECK_ARG(state, "lgblur_init: null pointer");
  LG_CHECK_ARG(((uintptr_t)state & 15) == 0, "lgblur_init: state must be 16-byte aligned");
  LG_CHECK_ARG(k0 >= 0 && k0 < (1LL << 31), "lgblur_init: k0=%lld outside 0 .. 2^31 - 1", k0);
  hipLaunchKernelGGL(dblur_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, (int)k0);
  LG_CHECK_LAUNCH("lgblur_init");
  lg_note_kernel("dblur_init_kernel");
  return LG_OK;
}

extern "C" int lgblur_step(float* state, float sigma0, long long images_per_step, long long fade_images, void* stream) {
  LG_CHECK_ARG(state, "lgblur_step: null pointer");
  LG_CHECK_ARG(((uintptr_t)state & 15) == 0, "lgblur_step: state must be 16-byte aligned");
  LG_CHECK_ARG(sigma0 >= 0.f && sigma0 <= 3.402823466e38f, "lgblur_step: sigma0=%g must be finite and >= 0", (double)sigma0);
  LG_CHECK_ARG(images_per_step >= 1 && images_per_step <= (1LL << 31), "lgblur_step: images_per_step=%lld outside 1 .. 2^31",
               images_per_step);
  LG_CHECK_ARG(fade_images >= 1 && fade_images <= (1LL << 40), "lgblur_step: fade_images=%lld outside 1 .. 2^40", fade_images);
  hipLaunchKernelGGL(dblur_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, sigma0, images_per_step, fade_images);
  LG_CHECK_LAUNCH("lgblur_step");
  lg_note_kernel("dblur_step_kernel");
  return LG_OK;
}

extern "C" int lgblur_apply(const float* x, const float* state, float* out, int rows, int S, void* stream) {
  LG_CHECK_ARG(x && state && out, "lgblur_apply: null pointer");
  LG_CHECK_ARG(x != out, "lgblur_apply: in-place call");
  LG_CHECK_ARG(rows > 0 && rows <= (1 << 20), "lgblur_apply: bad row count %d", rows);
  LG_CHECK_ARG(S >= 8 && S % 8 == 0 && S <= 1024, "lgblur_apply: image side %d must be a multiple of 8, at least 8, at most 1024", S);
  LG_CHECK_ARG((((uintptr_t)x | (uintptr_t)state | (uintptr_t)out) & 15) == 0, "lgblur_apply: images and state must be 16-byte aligned");
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(dblur_apply_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)DB_LDS_BYTES);
    attr = true;
  }
  const long long total = (long long)rows * ((S + DB_TW - 1) / DB_TW);   // strips
  const int blocks = (int)(total < 65536 ? total : 65536);
  hipLaunchKernelGGL(dblur_apply_kernel, dim3(blocks), dim3(DB_THREADS), DB_LDS_BYTES, (hipStream_t)stream, x, state, out, rows, S);
  LG_CHECK_LAUNCH("lgblur_apply");
  lg_note_kernel("dblur_apply_kernel");
  return LG_OK;
}
