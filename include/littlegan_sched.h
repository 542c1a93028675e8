/* littlegan_sched.h — the learning-rate schedule on the device and the Adam passes that read their rate from it (lr_g / lr_d / lr_adj,
 * lr_schedule, lr_warmup_steps, lr_decay_steps, lr_final_ratio), no counterpart in the reference.
 *
 * Entry points with the `lgsch_` prefix, exported by liblittlegan_hip.so under the conventions of littlegan_hip_ext.h — plain C, device
 * pointers, fp32, `stream` a hipStream_t passed as void* (NULL = default stream), return LG_OK (0) or LG_ERR_* with the message in
 * lg_last_error(), no allocation, no synchronisation, no atomics, every argument checked on the host before any launch, every launch
 * noted for lg_last_kernel().  lg_abi_version() stays 1: nothing declared in littlegan_hip*.h changes.  (Part of the C ABI like every
 * include/littlegan_*.h: bound by _lib.SIGNATURES, held to it by tests/test_abi.py.)
 *
 * ---- the definition (THIS PROJECT's) ---------------------------------------------------------------------------------------------- *
 * k = the number of training steps taken so far, over the whole run and across epochs; W = warmup, N = decay_steps, r = the fp32 value
 * of final_ratio.  Computed in fp64 (the library is built with -ffp-contract=off: every operation below is one IEEE operation):
 *     up = k < W ? (k + 1) / W : 1
 *     t  = k < W ? 0 : min((k - W) / N, 1)
 *     d  = 1                                       constant
 *          1 - (1 - r) * t                         linear
 *          r + (1 - r) * 0.5 * (1 + cos(pi * t))   cosine      (pi = the fp64 constant 3.141592653589793)
 *     s    = (float)(up * d)
 *     lr_m = (float)base_m * s                     one fp32 multiply per network
 * littlegan_amd/config.py::lr_factor restates it on the host in numpy fp64; constant and linear agree with it bit for bit (+, -, *, / and
 * conversions only), cosine to 1 fp32 ulp of s strictly inside the decay (the two fp64 cosines may differ in their last place) and bit
 * for bit at t == 0 and t >= 1.
 *
 * ---- the state: 32 bytes of device memory, 16-byte aligned ------------------------------------------------------------------------- *
 *     word 0      int32  k
 *     word 1      fp32   s                    of the step lgsch_step last ran for
 *     words 2..4  fp32   rate of G, D, A      of that step
 *     words 5..7  zero                        (reserved) */
#ifndef LITTLEGAN_SCHED_H
#define LITTLEGAN_SCHED_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LGSCH_KIND_CONSTANT 0
#define LGSCH_KIND_LINEAR 1
#define LGSCH_KIND_COSINE 2

/* state = {k0, 0, 0, 0, 0, 0, 0, 0}, written by one thread from the launch scalar: no host-to-device copy.  k0 >= 0. */
int lgsch_init(float* state, int k0, void* stream);

/* One step of the schedule: reads k, writes s and the three rates of step k by the definition above, then k = k + 1, saturating at
 * 2^31 - 1; words 5..7 are written as zero.  kind 0..2 (LGSCH_KIND_*); warmup >= 0; decay_steps >= 1 for linear and cosine (not read for
 * constant); 0 <= final_ratio <= 1; every rate finite and > 0.  One launch of one 64-thread workgroup (one thread works). */
int lgsch_step(float* state, int kind, int warmup, int decay_steps, float final_ratio, float lr_g, float lr_d, float lr_a, void* stream);

/* lg_clip_adam_update with the rate read from device memory: lr[0] takes the place of the scalar, in the same expressions on the same
 * grid (256 threads, at most 4096 blocks) — given the scalar's bits in lr[0] it gives the bits of lg_clip_adam_update.  lr is read, never
 * written; 4-byte aligned.  n > 0. */
int lgsch_clip_adam_update(float* w, const float* g, float* m, float* v, long long n, const float* state, const float* lr, float b1,
                           float b2, float eps, float clip, float gscale, void* stream);

/* lg_clip_adam_ema_update with the rate read from device memory, in the same way.  n > 0, n % 4 == 0; 0 <= lo <= hi <= n, both multiples
 * of 4; w, g, m, v, ema 16-byte aligned, lr 4-byte aligned; 0 <= decay < 1. */
int lgsch_clip_adam_ema_update(float* w, const float* g, float* m, float* v, float* ema, long long n, long long lo, long long hi,
                               const float* adam_state, const int* ema_state, const float* lr, float b1, float b2, float eps, float clip,
                               float gscale, float decay, void* stream);

#ifdef __cplusplus
}
#endif
#endif
