/* littlegan_geom.h — geometric augmentation of the Discriminator's inputs (geom_augment), no counterpart in the reference.
 *
 * Entry points with the `lgeo_` prefix, exported by liblittlegan_hip.so under the conventions of littlegan_hip_ext.h — plain C, device
 * pointers, fp32, `stream` a hipStream_t passed as void* (NULL = default stream), return LG_OK (0) or LG_ERR_* with the message in
 * lg_last_error(), no allocation, no synchronisation, every argument checked on the host before any launch.  lg_abi_version() stays 1:
 * nothing declared in littlegan_hip*.h changes.  (Part of the C ABI like every include/littlegan_*.h: bound by _lib.SIGNATURES, held
 * to it by tests/test_abi.py.)
 *
 * ---- the definition (THIS PROJECT's; Karras et al. 2020, "Training GANs with limited data", pixel blitting + geometric group) ------ *
 * diff_augment (littlegan_hip.h) has colour, integer translation and cutout.  This is the other group: x-flip, quarter turns, isotropic
 * scaling and arbitrary rotation, as one per-sample affine resampling of every image D reads.
 *
 * Record: per row 4 fp32 words {a, b, c, d}, 16 bytes, 16-byte aligned: the matrix M, row-major, of the map from a DESTINATION pixel to
 * its SOURCE position about the image centre.  With h = (S - 1) / 2, u = y - h, v = x - h:
 *     sy = (a u + b v) + h        sx = (c u + d v) + h
 * Sampling: x[S][S][3] fp32 NHWC, S % 8 == 0, 8 <= S <= 1024.
 *     out_k(y, x) = sum over the taps (i, j) in {y0, y0+1} x {x0, x0+1}, in that order, of  w x_k(i, j),
 *     y0 = floor(sy), x0 = floor(sx),  w = tent(sy - i) tent(sx - j),  tent(t) = 1 - |t| for |t| < 1, else 0.
 * A tap outside the image contributes nothing (zero fill, as diff_augment's translation; the paper reflects).  A tap whose weight is
 * exactly 0 contributes nothing and is not read: a selection, not a product.
 * Arithmetic: fp32, in exactly the order written, one rounding per operation (the library is built with -ffp-contract=off).  The forward
 * and the adjoint evaluate tent(sy - i) by the same expression, so their weights agree bit for bit and <Geo x, g>, <x, Geo^T g> differ
 * by summation rounding only.
 * Adjoint: a gather, no float atomics.  The thread of a source pixel (i, j) inverts M in fp32, walks the integer box of the destinations
 * that can touch it — around M^-1 ((i, j) - h) + h, half sides the absolute row sums of M^-1 plus a slack that covers the rounding of
 * the inverse (the whole image when the inverse is ill-conditioned) — clipped to the image, in ascending (y, x), recomputes (sy, sx) by
 * the forward's expression for each and adds w g(y, x).  The loop bounds depend on the record.
 * Unusable records: one with a non-finite entry, or whose fp32 determinant a d - b c is not finite or below 2^-20 in magnitude, gives a
 * zero image and a zero gradient.  For ANY record bits no access leaves the images: the records are device data.
 * Exactness: S is even, so h is a half-integer; with entries in {0, +-1} every coordinate is an exact integer, exactly one tap has weight
 * 1, and the output is a permutation of the input bit for bit.  The identity record {1, 0, 0, 1} returns x (adjoint: g) bit for bit. */
#ifndef LITTLEGAN_GEOM_H
#define LITTLEGAN_GEOM_H
#include "littlegan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* geo[rows][4] = the records of rows r0 .. r0+rows-1 of call slot `call` under the step's diff_augment key {seed, key_offset} (device
 * memory).  Row r of slot q has ctr = key_offset + (((q << 24) + r) << 1), as lg_diffaug_draw; the geometry reads
 * philox4x32_10({lo(ctr), hi(ctr), 2, 0}, seed) and its gates the block with third counter word 3 (diff_augment's records use 0, its
 * gates 1: no block is shared).  With v_j = word_j >> 8:
 *   xflip  (bit 1): flip iff v0 < 2^23            rot90  (bit 2): k = v1 >> 22
 *   scale  (bit 4): s = exp2(v2 2^-24 - 0.5)      rotate (bit 8): theta = 2 pi (v3 2^-24 - 0.5)
 *   M = R(theta) Q^k F / s,  R = [[cos, -sin], [sin, cos]],  Q = [[0, -1], [1, 0]],  F = diag(1, -1) (the identity when not flipped),
 * evaluated in fp64 on the device and rounded to fp32 once.  A component that policy_bits does not name, or that is gated off, is
 * SELECTED as its identity (theta = 0, s = 1, k = 0, no flip), not computed: such records hold exact 0 / +-1.
 * state: NULL = every named component on every row; else the 16 bytes of littlegan_hip_ext.h, and component j (0 xflip, 1 rot90,
 * 2 scale, 3 rotate) is on iff (gate_word_j >> 8) < (unsigned)(p 2^24), p = state[0] clamped to [0, 1]: the rule of
 * lgx_diffaug_draw_gated, reading the same p.
 * key 8-byte, state and geo 16-byte aligned; call 0..3, 1 <= rows <= 2^20, r0 >= 0, r0 + rows <= 2^24, S % 8 == 0 with 8 <= S <= 1024,
 * policy_bits 0..15.  One thread per row. */
int lgeo_draw(const long long* key, int call, int r0, int rows, int S, int policy_bits, const float* state, float* geo, void* stream);
/* out[rows][S][S][3] = Geo(x) under geo[rows][4] (lgeo_draw, or hand-built records).  x, geo, out 16-byte aligned, x != out,
 * 1 <= rows <= 2^20.  One launch, no workspace; a row range of a batch gives the bits it has in the whole batch. */
int lgeo_fwd(const float* x, const float* geo, float* out, int rows, int S, void* stream);
/* gx = Geo^T(g): the gradient with respect to x of <Geo(x), g>, by the gather above.  Same arguments and checks as lgeo_fwd. */
int lgeo_bwd(const float* g, const float* geo, float* gx, int rows, int S, void* stream);

#ifdef __cplusplus
}
#endif
#endif
