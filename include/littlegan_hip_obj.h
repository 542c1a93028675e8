/* littlegan_hip_obj.h — logit-side GAN objectives of liblittlegan_hip.so, no counterpart in the reference.
 *
 * Entry points with the `lgo_` prefix, exported by the same library as include/littlegan_hip.h under the same conventions — plain C,
 * device pointers, fp32, `stream` a hipStream_t passed as void* (NULL = default stream), return LG_OK (0) or LG_ERR_* with the text in
 * lg_last_error(), no allocation, no synchronisation, no atomics, every argument checked on the host before any launch, every launch
 * noted for lg_last_kernel().  lg_abi_version() covers this header too and stays 1: nothing declared in littlegan_hip.h changes.
 *
 * ---- gan_loss ---------------------------------------------------------------------------------------------------- *
 * THIS PROJECT's definition.  The reference trains output_pr through sigmoid + clipped binary cross entropy against the smoothed targets
 * 0.98 / 0.02 (lg_bce_heads_loss_fwd_bwd).  Here the real / fake term of a loss is taken on z, the PRE-sigmoid value of output_pr, with
 * no label smoothing and no clipping; the attribute terms stay the cross entropy of littlegan_hip.h, expression for expression.
 *
 *   kind            role 0: D on real rows   role 1: D on fake rows   role 2: G / Adjuster (D's output for their images)
 *   1 logistic      softplus(-z)             softplus(z)              softplus(-z)
 *   2 hinge         max(0, 1 - z)            max(0, 1 + z)            -z
 *   3 lsgan         (z - 1)^2 / 2            z^2 / 2                  (z - 1)^2 / 2
 *   4 wgan          -z                       z                        -z
 *
 * The subgradient at the hinge kink (z = +-1 exactly) is 0.  A NaN logit gives a NaN loss and a NaN gradient.  softplus(x) =
 * max(x, 0) + log1p(exp(-|x|)) and its derivative from the same exponential: finite at any finite z. */
#ifndef LITTLEGAN_HIP_OBJ_H
#define LITTLEGAN_HIP_OBJ_H
#include "littlegan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LGO_KIND_LOGISTIC 1
#define LGO_KIND_HINGE 2
#define LGO_KIND_LSGAN 3
#define LGO_KIND_WGAN 4
#define LGO_ROLE_D_REAL 0
#define LGO_ROLE_D_FAKE 1
#define LGO_ROLE_G 2

/* lg_heads_fwd that also keeps the logit of column 0: p[B][1 + c] is bit for bit lg_heads_fwd's on both GEMM routes (same partials,
 * same finalising expression), z_pr[b] is exactly the z whose sigmoid went into p[b][0].  Shapes and workspace as lg_heads_fwd
 * (lg_heads_fwd_workspace_bytes).  The name noted for lg_last_kernel() is that of the GEMM kernel. */
int lgo_heads_fwd(const float* x, const float* wpr, const float* bpr, const float* wc, const float* bc, float* p, float* z_pr,
                  void* workspace, size_t ws_bytes, int B, int K, int c, void* stream);
/* The logit-side counterpart of lg_bce_heads_loss_fwd_bwd.  p[B][1 + c], z_pr[B], t_c[B][c] (may be null when w_c == 0):
 *   loss[0] (+)= w_pr mean_b f(z_pr[b]) + w_c mean_{b,j} BCE(t_c[b][j], p[b][1 + j])       f by (kind, role), table above
 *   dz[b][0] = (w_pr / B) f'(z_pr[b]),   dz[b][1 + j] = the attribute gradient of lg_bce_heads_loss_fwd_bwd
 * With w_pr == 0 the call equals lg_bce_heads_loss_fwd_bwd(..., w_pr = 0, ...) bit for bit.  One 1024-thread block.  kind 1..4, role
 * 0..2, B > 0, c >= 1, w_pr and w_c finite. */
int lgo_gan_heads_loss_fwd_bwd(const float* p, const float* z_pr, const float* t_c, int kind, int role, float w_pr, float w_c,
                               float* loss, float* dz, int B, int c, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif
