/* littlegan_guard.h — global-norm gradient clipping and the non-finite step guard (clip_norm, skip_nonfinite), no counterpart in
 * the reference.
 *
 * Entry points with the `lgg_` prefix, exported by liblittlegan_hip.so under the conventions of the lgx_ / lgsch_ groups — plain C, device
 * pointers, fp32 gradients, `stream` a hipStream_t passed as void* (NULL = default stream), return LG_OK (0) or LG_ERR_* with the message
 * in lg_last_error(), no allocation, no synchronisation, no atomics, every argument checked on the host before any launch, every launch
 * noted for lg_last_kernel(), records and partials written with plain vector stores by one thread each.  lg_abi_version() stays 1:
 * nothing declared in littlegan_hip*.h changes.  (Part of the C ABI like every include/littlegan_*.h: bound by _lib.SIGNATURES, held
 * to it by tests/test_abi.py.)
 *
 * ---- the definition (THIS PROJECT's) ---------------------------------------------------------------------------------------------- *
 * Per network, on a step where it trains, over the n gradient elements g_i the step trains (after the all-reduce), gscale = 1 / world:
 *     S        = sum_i (double)g_i * (double)g_i      fp64; every product is exact, the additions run in an order that n alone decides
 *     bad      = !isfinite(S)                         exactly "some g_i is NaN or +-Inf": a sum of squares of finite fp32 stays far
 *                                                     below the fp64 range, so no separate scan is needed
 *     N        = (float)(sqrt(S) * (double)gscale)    the norm of the averaged gradient
 *     c        = 1                                    if clip_norm == 0 or bad
 *                q = clip_norm / (N + 1e-6f);  q < 1 ? q : 1        (fp32)
 *     eff      = gscale * c                           one fp32 multiply
 *     skip_now = bad && skip
 * The Adam passes below use eff where lg_clip_adam_update takes gscale and read nothing else differently; with skip_now they leave
 * w, m, v and the beta powers exactly as they were.  bad without skip is the step as it is without the guard (c = 1).
 * littlegan_amd/config.py::grad_guard_restate restates it on the host in numpy.
 *
 * The order of the additions (CH = GG_CHUNK = 16384 elements, P = lgg_partials_count(n) = min(1024, ceil(n / CH))): chunk k holds the
 * elements [k CH, (k + 1) CH); workgroup b of P (256 threads) owns the chunks b, b + P, b + 2P, ...; inside a chunk thread t owns the
 * 4-element groups j = t, t + 256, ..., t + 15 * 256 (elements k CH + 4 j + e, e = 0..3) and keeps one fp64 accumulator per e, adding
 * chunk after chunk, group after group; its sum is (a0 + a1) + (a2 + a3); the 64 lanes of a wave are summed by xor butterflies of
 * 32, 16, 8, 4, 2, 1, the four waves in wave order; lgg_finalise adds the P partials in index order.  Nothing in it depends on the number
 * of compute units, on reserved ones, or on the address of g: the map from element to thread goes by index, so a view of the same data
 * that is not 16-byte aligned (read with scalar loads instead of 16-byte ones) gives the same bits.
 *
 * ---- the record: 32 bytes of device memory, 16-byte aligned ------------------------------------------------------------------------ *
 *     word 0      fp32   N
 *     word 1      fp32   eff
 *     word 2      int32  skip_now
 *     word 3      int32  steps skipped so far, saturating at 2^31 - 1
 *     word 4      int32  steps with bad so far, skipped or not, saturating
 *     word 5      fp32   c
 *     words 6, 7  zero */
#ifndef GRADGUARD_H
#define GRADGUARD_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GG_CHUNK 16384
#define GG_MAX_PARTIALS 1024

/* P(n): the number of fp64 partials of n elements, min(1024, ceil(n / GG_CHUNK)); a pure function of n.  0 for n < 1. */
int lgg_partials_count(long long n);
/* 8 * P(n): the bytes lgg_sumsq_partial writes and lgg_finalise reads. */
size_t lgg_workspace_bytes(long long n);

/* rec = {0, 0, 0, skipped0, nonfinite0, 0, 0, 0}, written by one thread from the launch scalars: no host-to-device copy.  Both >= 0. */
int lgg_init(void* rec, int skipped0, int nonfinite0, void* stream);

/* partial[b] = the sum of squares of workgroup b's chunks, b < P(n), in the order stated above.  n >= 1; g 4-byte aligned (16-byte
 * loads are used when it is 16-byte aligned, scalar loads with the same map when not); partial 8-byte aligned, partial_bytes >=
 * lgg_workspace_bytes(n).  One launch of P(n) workgroups of 256 threads. */
int lgg_sumsq_partial(const float* g, long long n, void* partial, size_t partial_bytes, void* stream);

/* S = partial[0] + ... + partial[P(n) - 1] in index order, then the record by the definition above; the two counters are read from rec
 * and advance by skip_now and by bad.  gscale finite and > 0; clip_norm finite and >= 0 (0 = no clipping); skip 0 or 1.  One launch of
 * one workgroup of 256 threads; one thread adds and writes. */
int lgg_finalise(const void* partial, long long n, void* rec, float gscale, float clip_norm, int skip, void* stream);

/* lgsch_clip_adam_update with the scale read from the record: rec word 1 (eff) takes the place of gscale, in the same expressions on the
 * same grid (256 threads, at most 4096 blocks) — given eff == gscale it gives the bits of lg_clip_adam_update at the rate lr[0].  With
 * rec word 2 (skip_now) set the launch writes nothing.  lr, rec are read, never written; lr 4-byte, rec 16-byte aligned.  n > 0. */
int lgg_clip_adam_update(float* w, const float* g, float* m, float* v, long long n, const float* adam_state, const float* lr,
                        const void* rec, float b1, float b2, float eps, float clip, void* stream);

/* lgsch_clip_adam_ema_update with the scale read from the record, in the same way.  With skip_now set it takes the weight average alone,
 * as with lo == hi.  n > 0, n % 4 == 0; 0 <= lo <= hi <= n, both multiples of 4; w, g, m, v, ema, rec 16-byte aligned, lr 4-byte
 * aligned; 0 <= decay < 1. */
int lgg_clip_adam_ema_update(float* w, const float* g, float* m, float* v, float* ema, long long n, long long lo, long long hi,
                            const float* adam_state, const int* ema_state, const float* lr, const void* rec, float b1, float b2,
                            float eps, float clip, float decay, void* stream);

/* lg_adam_advance unless skip_now is set in rec: the beta powers of a skipped step stay. */
int lgg_adam_advance(float* adam_state, const void* rec, float b1, float b2, void* stream);

#ifdef __cplusplus
}
#endif
#endif
