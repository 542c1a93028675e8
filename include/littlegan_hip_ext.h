/* littlegan_hip_ext.h — training-control extensions of liblittlegan_hip.so, no counterpart in the reference.
 *
 * The functions of include/littlegan_hip.h are the drop-in boundary: kernels the training and evaluation passes are made of.  This
 * header holds what steers a run from the device instead: entry points with the `lgx_` prefix, exported by the same library, under
 * the same conventions — plain C, device pointers, fp32 unless stated, `stream` a hipStream_t passed as void* (NULL = default stream),
 * return LG_OK (0) or LG_ERR_* with lgx/lg sharing lg_last_error(), no allocation, no synchronisation, every argument checked on the
 * host before any launch.  lg_abi_version() covers both headers and stays 1: nothing declared in littlegan_hip.h changes.
 *
 * ---- adaptive augmentation probability (ADA; Karras et al. 2020, "Training GANs with limited data") -------------- *
 * THIS PROJECT's definition.  diff_augment (littlegan_hip.h) applies every named component to every row.  Here each
 * component of each row is applied with probability p, and p is driven from the Discriminator's own overfitting statistic
 * r = E[sign(D_logit(real))] towards a target.  Both live on the device: p is read from device memory by the draw, so a replayed graph
 * sees the current p, and the controller is two one-workgroup launches that need no host synchronisation.
 *
 * state: 16 bytes of DEVICE memory, 16-byte aligned, declared float* and holding
 *   state[0] fp32  p, 0 <= p <= 1
 *   state[1] int32 sum of signs this interval
 *   state[2] int32 rows this interval
 *   state[3] int32 steps this interval */
#ifndef LITTLEGAN_HIP_EXT_H
#define LITTLEGAN_HIP_EXT_H
#include "littlegan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* params[rows][8] = the records lg_diffaug_draw writes for rows r0 .. r0+rows-1 of call slot `call`, with each named component of each
 * row gated by an independent Bernoulli(p), p = state[0]: one gate for color (b, s, c together), one for translation, one for cutout.
 * A component that is gated off gets its identity values, exactly as one that policy_bits does not name.  The gate words are the
 * THIRD Philox block of the row: the counter of its first block, ctr = key_offset + (((call << 24) + r) << 1), with the third counter
 * word 1 instead of 0, philox4x32_10({lo(ctr), hi(ctr), 1, 0}, seed) — no block of any record has a non-zero third word.  With
 * w_j = word_j >> 8 (j = 0 color, 1 translation, 2 cutout; word 3 unused) and t = (unsigned)(p * 16777216.0f) (exact: p is fp32 in
 * [0, 1]), component j is on iff w_j < t.  p = 1 gates nothing off (the output is lg_diffaug_draw's, bit for bit), p = 0 everything.
 * key 8-byte, state and params 16-byte aligned; call 0..3, r0 + rows <= 2^24, S % 8 == 0 with 8 <= S <= 1024, policy_bits 0..7. */
int lgx_diffaug_draw_gated(const long long* key, int call, int r0, int rows, int S, int policy_bits, const float* state, float* params,
                           void* stream);
/* state = {p0, 0, 0, 0}, written by a one-block kernel from a launch scalar (no host-to-device copy, as lg_dropout_key).  0 <= p0 <= 1 */
int lgx_ada_init(float* state, float p0, void* stream);
/* One step's statistic.  heads[B][ld]: the first B rows (the real ones) of D's packed sigmoid output, column 0 = real_pr.  Per row
 * s_i = (v > 0.5f) - (v < 0.5f) (NaN gives 0; the sigmoid is above 0.5 exactly where the logit is positive), then
 *   state[1] += sum_i s_i;  state[2] += B;  state[3] += 1.
 * An integer sum: order-free and the same bits in every run.  One 256-thread workgroup.  ld >= 1, 1 <= B <= 2^20; heads 4-byte aligned. */
int lgx_ada_accumulate(float* state, const float* heads, int ld, int B, void* stream);
/* The controller.  If state[3] >= interval:
 *   r = (float)state[1] / (float)state[2];  dir = r > target ? 1 : r < target ? -1 : 0;
 *   p = min(max(state[0] + (float)dir * ((float)state[2] * per_row), 0.f), 1.f);  state = {p, 0, 0, 0}
 * in this order of operations (the library is built with -ffp-contract=off); otherwise nothing is written.  per_row is the change of
 * p per real row seen: float32(1 / (ada_kimg * 1000)).  interval >= 1, 0 < target < 1, per_row > 0 and finite. */
int lgx_ada_adjust(float* state, int interval, float target, float per_row, void* stream);

#ifdef __cplusplus
}
#endif
#endif
