// Logit-side GAN objectives (gan_loss: logistic | hinge | lsgan | wgan; the reference has none — this project's definition, DESIGN.md §25,
// include/littlegan_hip_obj.h).  The reference's real / fake term sits behind a sigmoid and a clip (loss_optim.hip, bce_heads_kernel);
// these take it on z, the pre-sigmoid value of output_pr:
//   heads_final_logit_kernel : heads_final_kernel (heads.hip) that also stores z of column 0 — the GEMM partials are lg_heads_fwd's
//   gan_heads_kernel         : bce_heads_kernel with column 0 replaced by f(z) / f'(z); the attribute columns keep its expressions and
//                              its thread mapping, so with w_pr == 0 the two kernels write the same bits
//   pair_heads_kernel        : gan_heads_kernel with column 0 taken on the difference of two logits (relativistic pairing, DESIGN.md §27,
//                              include/littlegan_rel.h): the same gan_term at role 0, the same attribute columns
#include "lg_internal.h"
#include "../../include/littlegan_hip_obj.h"
#include "../../include/littlegan_rel.h"

#define LG_BCE_EPS 1e-7f   // = loss_optim.hip's

namespace {

constexpr int HC_MAX = 40;  // = heads.hip's: max cond_dim, 1 + c <= 64 lanes

// = heads_final_kernel, expression for expression (p is bit-identical), + z of column 0
__global__ __launch_bounds__(256) void heads_final_logit_kernel(const float* __restrict__ part, const float* __restrict__ bpr,
                                                                const float* __restrict__ bc, float* __restrict__ p,
                                                                float* __restrict__ zpr, int B, int c, int nkc) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n = B * (c + 1);
  if (i >= n) return;
  const int j = i % (c + 1);
  float z = 0.f;
  for (int q = 0; q < nkc; ++q) z += part[(long long)q * n + i];
  z += j == 0 ? bpr[0] : bc[j - 1];
  p[i] = 1.f / (1.f + expf(-z));
  if (j == 0) zpr[i / (c + 1)] = z;
}

// f(z) and f'(z) of (kind, role), both scaled by s.  A NaN z gives NaN in both.
__device__ __forceinline__ void gan_term(int kind, int role, float z, float s, float& f, float& g) {
  const bool fake = role == LGO_ROLE_D_FAKE;
  if (kind == LGO_KIND_LOGISTIC) {
    // softplus(x) with x = z on fake rows, -z otherwise: max(x, 0) + log1p(e), e = exp(-|x|) in (0, 1]; sigmoid(x) from the same e
    const float x = fake ? z : -z;
    const float e = expf(-fabsf(x));
    f = s * (fmaxf(x, 0.f) + log1pf(e));
    const float sg = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    g = fake ? s * sg : -s * sg;
  } else if (kind == LGO_KIND_HINGE) {
    if (role == LGO_ROLE_G) {
      f = -s * z;
      g = z != z ? z : -s;
    } else {
      const float t = fake ? 1.f + z : 1.f - z;   // max(0, t); subgradient 0 at the kink t == 0
      const bool nan = t != t;
      f = (t > 0.f || nan) ? s * t : 0.f;
      g = nan ? t : (t > 0.f ? (fake ? s : -s) : 0.f);
    }
  } else if (kind == LGO_KIND_LSGAN) {
    const float d = fake ? z : z - 1.f;
    f = s * (0.5f * (d * d));
    g = s * d;
  } else {  // LGO_KIND_WGAN
    f = fake ? s * z : -s * z;
    g = z != z ? z : (fake ? s : -s);
  }
}

// an attribute column (the expressions of bce_heads_kernel): returns its summand of the loss, g = its gradient (0 outside the clip)
__device__ __forceinline__ float attr_term(float t, float pv, float sc, float& g) {
  const float pc = fminf(fmaxf(pv, LG_BCE_EPS), 1.f - LG_BCE_EPS);
  const float f = -sc * (t * logf(pc + LG_BCE_EPS) + (1.f - t) * logf(1.f - pc + LG_BCE_EPS));
  const bool inside = pv >= LG_BCE_EPS && pv <= 1.f - LG_BCE_EPS;
  if (inside) g = -sc * (t / (pc + LG_BCE_EPS) - (1.f - t) / (1.f - pc + LG_BCE_EPS)) * pv * (1.f - pv);
  return f;
}

__global__ __launch_bounds__(1024) void gan_heads_kernel(const float* __restrict__ p, const float* __restrict__ zpr,
                                                        const float* __restrict__ t_c, int kind, int role, float w_pr, float w_c,
                                                        float* __restrict__ loss, float* __restrict__ dz, int B, int c, int accumulate) {
  const int J = c + 1, n = B * J;
  const float s_pr = w_pr / (float)B, s_c = w_c / (float)(B * c);
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {  // the loop of bce_heads_kernel: one block, the loss is ONE scalar
    const int b = i / J, j = i - b * J;
    const float sc = j == 0 ? s_pr : s_c;
    float g = 0.f;
    if (sc != 0.f) {
      if (j == 0) {
        float f;
        gan_term(kind, role, zpr[b], sc, f, g);
        acc += f;
      } else {
        acc += attr_term(t_c[b * c + j - 1], p[i], sc, g);
      }
    }
    dz[i] = g;
  }
  __shared__ float sred[16];
  float red[1] = {acc};
  lg_block_sum<1>(red, sred);
  if (threadIdx.x == 0) loss[0] = (accumulate ? loss[0] : 0.f) + red[0];
}

// gan_heads_kernel with column 0 taken on a PAIR of logits (relativistic pairing): f0 = gan_term's role-0 function of the
// kind, t = z[b] - z_ref[b mod m] (SELF: the loss and its gradient with respect to z) or z_ref[b mod m] - z[b] (OTHER: the gradient
// with respect to z of the pair's term, which the SELF call of the other half has added to the loss).  The attribute columns, the loop
// and the block sum are gan_heads_kernel's.
__global__ __launch_bounds__(1024) void pair_heads_kernel(const float* __restrict__ p, const float* __restrict__ z,
                                                         const float* __restrict__ z_ref, const float* __restrict__ t_c, int kind, int side,
                                                         float w_pr, float w_c, float* __restrict__ loss, float* __restrict__ dz, int n,
                                                         int m, int c, int accumulate) {
  const int J = c + 1, tot = n * J;
  const float s_pr = w_pr / (float)n, s_c = w_c / (float)(n * c);
  float acc = 0.f;
  for (int i = threadIdx.x; i < tot; i += blockDim.x) {
    const int b = i / J, j = i - b * J;
    const float sc = j == 0 ? s_pr : s_c;
    float g = 0.f;
    if (sc != 0.f) {
      if (j == 0) {
        const float zr = z_ref[b % m];
        float f;
        if (side == LGREL_SIDE_SELF) {
          gan_term(kind, LGO_ROLE_D_REAL, z[b] - zr, sc, f, g);
          acc += f;
        } else {
          gan_term(kind, LGO_ROLE_D_REAL, zr - z[b], sc, f, g);
          g = -g;
        }
      } else {
        acc += attr_term(t_c[b * c + j - 1], p[i], sc, g);
      }
    }
    dz[i] = g;
  }
  __shared__ float sred[16];
  float red[1] = {acc};
  lg_block_sum<1>(red, sred);
  if (threadIdx.x == 0) loss[0] = (accumulate ? loss[0] : 0.f) + red[0];
}

inline bool finite_f(float v) { return v >= -3.402823466e38f && v <= 3.402823466e38f; }

}  // namespace

extern "C" int lgo_heads_fwd(const float* x, const float* wpr, const float* bpr, const float* wc, const float* bc, float* p, float* z_pr,
                             void* workspace, size_t ws_bytes, int B, int K, int c, void* stream) {
  LG_CHECK_ARG(x && wpr && bpr && wc && bc && p && z_pr && workspace, "lgo_heads_fwd: null pointer");
  LG_CHECK_ARG(B > 0 && K > 0 && K % 4 == 0 && c >= 1 && c <= HC_MAX, "lgo_heads_fwd: bad shape B=%d K=%d c=%d", B, K, c);
  LG_CHECK_ARG(ws_bytes >= lg_heads_fwd_workspace_bytes(B, K, c), "lgo_heads_fwd: workspace too small (%zu bytes)", ws_bytes);
  int nkc = 0;
  float* part = (float*)workspace;
  const int rc = lg_heads_fwd_partials(x, wpr, wc, part, B, K, c, &nkc, stream);   // notes the GEMM kernel's name
  if (rc != LG_OK) return rc;
  hipLaunchKernelGGL(heads_final_logit_kernel, dim3(lg_cdiv(B * (c + 1), 256)), dim3(256), 0, (hipStream_t)stream, part, bpr, bc, p,
                     z_pr, B, c, nkc);
  LG_CHECK_LAUNCH("lgo_heads_fwd(final)");
  return LG_OK;
}

extern "C" int lgo_gan_heads_loss_fwd_bwd(const float* p, const float* z_pr, const float* t_c, int kind, int role, float w_pr, float w_c,
                                          float* loss, float* dz, int B, int c, int accumulate, void* stream) {
  LG_CHECK_ARG(p && z_pr && loss && dz, "lgo_gan_heads_loss_fwd_bwd: null pointer");
  LG_CHECK_ARG(kind >= LGO_KIND_LOGISTIC && kind <= LGO_KIND_WGAN, "lgo_gan_heads_loss_fwd_bwd: bad kind %d (1 logistic, 2 hinge, 3 lsgan, 4 wgan)",
               kind);
  LG_CHECK_ARG(role >= LGO_ROLE_D_REAL && role <= LGO_ROLE_G, "lgo_gan_heads_loss_fwd_bwd: bad role %d (0 D real, 1 D fake, 2 G)", role);
  LG_CHECK_ARG(B > 0 && c >= 1 && (long long)B * (c + 1) < (1LL << 31), "lgo_gan_heads_loss_fwd_bwd: bad shape B=%d c=%d", B, c);
  LG_CHECK_ARG(finite_f(w_pr) && finite_f(w_c), "lgo_gan_heads_loss_fwd_bwd: weights w_pr=%g w_c=%g must be finite", (double)w_pr,
               (double)w_c);
  LG_CHECK_ARG(t_c || w_c == 0.f, "lgo_gan_heads_loss_fwd_bwd: t_c is null but w_c != 0");
  hipLaunchKernelGGL(gan_heads_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, p, z_pr, t_c, kind, role, w_pr, w_c, loss, dz, B, c,
                     accumulate);
  LG_CHECK_LAUNCH("lgo_gan_heads_loss_fwd_bwd");
  lg_note_kernel("gan_heads_kernel");
  return LG_OK;
}

extern "C" int lgrel_pair_heads_loss_fwd_bwd(const float* p, const float* z, const float* z_ref, const float* t_c, int kind, int side,
                                             float w_pr, float w_c, float* loss, float* dz, int n, int m, int c, int accumulate,
                                             void* stream) {
  LG_CHECK_ARG(p && z && z_ref && loss && dz, "lgrel_pair_heads_loss_fwd_bwd: null pointer");
  LG_CHECK_ARG((((uintptr_t)p | (uintptr_t)z | (uintptr_t)z_ref | (uintptr_t)t_c | (uintptr_t)loss | (uintptr_t)dz) & 3) == 0,
               "lgrel_pair_heads_loss_fwd_bwd: every pointer must be 4-byte aligned");
  LG_CHECK_ARG(kind >= LGO_KIND_LOGISTIC && kind <= LGO_KIND_LSGAN,
               "lgrel_pair_heads_loss_fwd_bwd: bad kind %d (1 logistic, 2 hinge, 3 lsgan; wgan of a difference is wgan itself)", kind);
  LG_CHECK_ARG(side == LGREL_SIDE_SELF || side == LGREL_SIDE_OTHER, "lgrel_pair_heads_loss_fwd_bwd: bad side %d (0 self, 1 other)", side);
  LG_CHECK_ARG(n > 0 && c >= 1 && (long long)n * (c + 1) < (1LL << 31), "lgrel_pair_heads_loss_fwd_bwd: bad shape n=%d c=%d", n, c);
  LG_CHECK_ARG(m > 0 && n % m == 0, "lgrel_pair_heads_loss_fwd_bwd: n=%d must be a multiple of m=%d > 0", n, m);
  LG_CHECK_ARG(finite_f(w_pr) && finite_f(w_c), "lgrel_pair_heads_loss_fwd_bwd: weights w_pr=%g w_c=%g must be finite", (double)w_pr,
               (double)w_c);
  LG_CHECK_ARG(t_c || w_c == 0.f, "lgrel_pair_heads_loss_fwd_bwd: t_c is null but w_c != 0");
  hipLaunchKernelGGL(pair_heads_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, p, z, z_ref, t_c, kind, side, w_pr, w_c, loss, dz, n,
                     m, c, accumulate);
  LG_CHECK_LAUNCH("lgrel_pair_heads_loss_fwd_bwd");
  lg_note_kernel("pair_heads_kernel");
  return LG_OK;
}
