/* littlegan_rel.h — relativistic pairing objective and the R2 penalty (relativistic / r2_gamma), no counterpart in the
 * reference.
 *
 * Entry points with the `lgrel_` prefix, exported by liblittlegan_hip.so under the conventions of littlegan_hip_ext.h — plain C, device
 * pointers, fp32, `stream` a hipStream_t passed as void* (NULL = default stream), return LG_OK (0) or LG_ERR_* with the message in
 * lg_last_error(), no allocation, no synchronisation, no atomics, every argument checked on the host before any launch.
 * lg_abi_version() stays 1: nothing declared in littlegan_hip*.h changes.  (Part of the C ABI like every include/littlegan_*.h:
 * bound by _lib.SIGNATURES, held to it by tests/test_abi.py.)
 *
 * ---- the definition (THIS PROJECT's; Jolicoeur-Martineau 2018, relativistic pairing; Huang et al. 2024, R1 + R2) ------------------- *
 * f0 = the ROLE-0 (D real) function of a logit-side kind of littlegan_hip_obj.h, evaluated by the device function that
 * lgo_gan_heads_loss_fwd_bwd uses:   logistic softplus(-t)      hinge max(0, 1 - t)      lsgan (t - 1)^2 / 2
 * With z_r / z_f the logits of the real / fake half of D's 2B-row batch, row b of one half paired with row b of the other:
 *     disc:  mean_b f0(z_r[b] - z_f[b])           differentiated with respect to z_r and z_f
 *     gen:   mean_b f0(z_f[b] - z_r[b])           with respect to z_f alone
 *     adj:   mean_i f0(z_a[i] - z_r[i mod B])     over the Adjuster's 2B rows, with respect to z_a alone
 * No smoothing, no clipping, subgradient 0 at hinge's kink t == 1; a NaN in either logit of a pair gives a NaN loss and NaN gradients
 * in that pair's rows.  "wgan" has no pairing of its own: f0(z_r - z_f) = -z_r + z_f is the wgan objective.
 * R2 is R1 (littlegan_hip_reg.h) on the fake rows D read; with both on, one pass over the 2B-row batch seeds both. */
#ifndef LITTLEGAN_REL_H
#define LITTLEGAN_REL_H
#include "littlegan_hip_obj.h"
#include "littlegan_hip_reg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LGREL_SIDE_SELF 0
#define LGREL_SIDE_OTHER 1

/* lgo_gan_heads_loss_fwd_bwd with column 0 taken on a pair of logits.  p[n][1+c] (the sigmoid outputs, read by the attribute columns),
 * z[n] the logits of these rows, z_ref[m] the logits they are paired with, n % m == 0: row i pairs with z_ref[i mod m].
 *   side 0 (SELF):  t_i = z[i] - z_ref[i mod m],  loss (+)= w_pr mean_i f0(t_i),  dz[i][0] =  (w_pr / n) f0'(t_i)
 *   side 1 (OTHER): t_i = z_ref[i mod m] - z[i],  column 0 adds NOTHING to the loss,  dz[i][0] = -(w_pr / n) f0'(t_i)
 * (OTHER is the gradient, with respect to the second logit, of the term a SELF call on the other half adds: both form the difference
 * from the same operands in the same order, so the two rows of a pair see the same t bit for bit.)
 * Columns 1..c, their loss w_c mean BCE(t_c, p) and `accumulate` are lgo_gan_heads_loss_fwd_bwd's, expression for expression; t_c may
 * be NULL when w_c == 0.  kind 1..3 (LGO_KIND_LOGISTIC, _HINGE, _LSGAN); n > 0, m > 0, c >= 1, n (1 + c) < 2^31; weights finite;
 * every pointer 4-byte aligned.  One launch of one 1024-thread block, no workspace. */
int lgrel_pair_heads_loss_fwd_bwd(const float* p, const float* z, const float* z_ref, const float* t_c, int kind, int side, float w_pr,
                                  float w_c, float* loss, float* dz, int n, int m, int c, int accumulate, void* stream);

/* workspace of lgrel_r12_seed for g[2B][L]: the fp64 partials of its 2B rows (0 for B <= 0 or L <= 0) */
size_t lgrel_r12_workspace_bytes(int B, long long L);
/* lgr_r1_seed over g[2B][L] with a weight per half: rows [0, B) take w_real, rows [B, 2B) w_fake.
 *   r2[b] = |g_b|^2 (2B values),  u0_b = (w_half / B) g_b,  term_h = (w_h / 2) mean over the half's B rows of r2_b,
 *   r1_loss[0] = term_real,  r2_loss[0] = term_fake,  loss[0] = (loss[0] + term_real) + term_fake  (fp32, in that order).
 * loss, r1_loss, r2_loss may each be NULL.  The sums are lgr_r1_seed's, per row and per half — fp64 partials over 4096-element chunks
 * merged in index order, the layout fixed by (B, L) alone — so the call gives the bits of two lgr_r1_seed calls on the halves.
 * g, u0 16-byte, workspace 8-byte, the others 4-byte aligned; B > 0, L > 0, L % 4 == 0, 2 B L / 4 < 2^31; weights finite and >= 0;
 * ws_bytes >= lgrel_r12_workspace_bytes(B, L).  Two launches. */
int lgrel_r12_seed(const float* g, float* u0, float* r2, float* loss, float* r1_loss, float* r2_loss, float w_real, float w_fake,
                   void* workspace, size_t ws_bytes, int B, long long L, void* stream);

#ifdef __cplusplus
}
#endif
#endif
