/* littlegan_hip_reg.h — regularisers of liblittlegan_hip.so beyond the reference's recipe, no counterpart in the reference.
 *
 * Entry points with the `lgr_` prefix, exported by the same library as include/littlegan_hip.h under the same conventions — plain C,
 * device pointers, fp32, `stream` a hipStream_t passed as void* (NULL = default stream), return LG_OK (0) or LG_ERR_* with the text in
 * lg_last_error(), no allocation, no synchronisation, every argument checked on the host before any launch, every launch noted for
 * lg_last_kernel().  lg_abi_version() covers this header too and stays 1: nothing declared in littlegan_hip.h changes.
 *
 * ---- R1 gradient penalty (Mescheder et al. 2018; lazily applied as in Karras et al. 2020) ------------------------ *
 * THIS PROJECT's definition.  x_b = row b of what D reads as its real batch, l_b = <w_pr, h4(x_b)> + b_pr the PRE-sigmoid value of
 * output_pr, g_b = dl_b / dx_b, r2_b = |g_b|^2, r1 = (weight / 2) mean_b r2_b with weight = r1_gamma * r1_interval, added to the disc
 * loss on every r1_interval-th step.  Its weight gradient is reverse over reverse, the pass of the gradient penalty
 * with the sigmoid taken out:
 *   1  forward of D on x, context kept                           (the library's own kernels)
 *   2  top seed g_h4[b] = w_pr                                    lgr_r1_heads_seed
 *   3  recorded backward down to the image -> g                   (lg_gp_norm_bwd + the data-gradient convs)
 *   4  r2, the term, u0 = (weight / B) g                          lgr_r1_seed
 *   5  adjoint sweep upward -> u4 and the injected adjoints       (lg_gp_norm_dd + convs + weight gradients)
 *   6  heads: dw_pr += sum_b u4[b]                                lgr_r1_heads_colsum     (l is bilinear in (w_pr, h4): no second-
 *   7  second backward from a ZERO top gradient                   (lg_gp_norm_bwd with `add`)   order scalar, nothing for b_pr)
 *
 * Every reduction has ONE order, fixed by the shape alone: fp64 partials over chunks / slabs whose boundaries depend on (B, L) or
 * (B, K) only, merged in index order.  The grids are sized from lg_grid_cus(), the partial layout is not: a process that reserves CUs
 * (lg_set_reserved_cus) computes the same bits as one that does not.  No atomics. */
#ifndef LITTLEGAN_HIP_REG_H
#define LITTLEGAN_HIP_REG_H
#include "littlegan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of lgr_r1_seed's workspace (one double per 4096-element chunk of every row); 0 for an empty shape */
size_t lgr_r1_workspace_bytes(int B, long long L);
/* step 2.  g[B][K] = wpr[K] for every row, copied bit for bit.  B, K > 0, B * K < 2^31 */
int lgr_r1_heads_seed(const float* wpr, float* g, int B, int K, void* stream);
/* step 4.  g[B][L] (L % 4 == 0, B * L / 4 < 2^31; g and u0 16-byte aligned): r2[b] = sum g_b^2; term = (weight / 2) mean_b r2;
 * loss[0] += term, r1_loss[0] = term (each may be null); u0 = (weight / B) g with the quotient rounded to fp32 once.  One pass over g
 * writes u0 and the per-chunk partials, a one-block finaliser merges them.  weight finite and >= 0. */
int lgr_r1_seed(const float* g, float* u0, float* r2, float* loss, float* r1_loss, float weight, void* workspace, size_t ws_bytes, int B,
                long long L, void* stream);
/* bytes of lgr_r1_heads_colsum's workspace (one double per column and 32-row slab); 0 for an empty shape */
size_t lgr_r1_colsum_workspace_bytes(int B, int K);
/* step 6.  dwpr[k] += sum_b u[b][k]: rows in slabs of 32, each summed in row order in fp64, the slabs merged in slab order, rounded to
 * fp32 once and added to dwpr.  B, K > 0, B * K < 2^31 */
int lgr_r1_heads_colsum(const float* u, float* dwpr, void* workspace, size_t ws_bytes, int B, int K, void* stream);

#ifdef __cplusplus
}
#endif
#endif
