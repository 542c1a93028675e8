/* littlegan_adj.h — the Adjuster's forward with its single-reader normalised maps left out.
 *
 * The Adjuster's tape differentiates its own dense + norm only, so no weight gradient is ever asked of its encoder pass or of its
 * decoder pass: a normalised map of those passes has one reader (the next conv) or two (an encoder map is also a decoder skip).  The
 * entry points here let those readers take the RAW bf16 conv output z of a level plus that level's finished statistics records
 * [B][8] = {mu_hi, sigma, a, beta, mu_lo, 0, 0, 0} (lg_instnorm_stats_finalize) in place of the map, and normalise on the way in:
 *     h = bf16(leaky_alpha(a ((z - mu_hi) - mu_lo) + beta))            the value lg_instnorm_leaky_apply_z16 stores (post_leaky = 1)
 * Every result is bit-identical to the route through the stored maps (the library is built with -ffp-contract=off).
 *
 * Entry points with the `lgadj_` prefix, exported by liblittlegan_hip.so under the conventions of littlegan_hip_ext.h — plain C, device
 * pointers, `stream` a hipStream_t passed as void* (NULL = default stream), return LG_OK (0) or LG_ERR_* with the message in
 * lg_last_error(), no allocation, no synchronisation, no atomics, every argument checked on the host before any launch, every launch
 * noted for lg_last_kernel().  lg_abi_version() stays 1: nothing declared in littlegan_hip*.h changes.  (Part of the C ABI like every
 * include/littlegan_*.h: bound by _lib.SIGNATURES, held to it by tests/test_abi.py; tests/test_memory_contract_gpu.py runs every entry
 * point between guard bands.) */
#ifndef LITTLEGAN_ADJ_H
#define LITTLEGAN_ADJ_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* lg_instnorm_leaky_apply_z16 (pre_leaky = 0) with a RAW skip: y = leaky?(norm(z16)) + (float)h(skip_z16, skip_stats), h as above with
 * the same alpha.  z16, skip_z16: bf16 [B][L]; stats, skip_stats: [B][8]; y (fp32) and / or y16 (bf16) [B][L], either may be null.
 * L % 8 == 0, B * L / 8 < 2^31.  Bit-identical to lg_instnorm_leaky_apply_z16 with the bf16 map h as its skip. */
int lgadj_instnorm_apply_rs(const void* z16, const float* stats, const void* skip_z16, const float* skip_stats, float* y, void* y16,
                            int B, long long L, int post_leaky, float alpha, void* stream);

/* lg_instnorm_leaky_apply_z16_p (the finalize of z16's moment partials folded into the launch; `stats` receives the finished
 * records) with a RAW skip, in the same way.  partials [B][nparts][3] doubles; B <= 65535. */
int lgadj_instnorm_apply_p_rs(const void* z16, const void* partials, int nparts, const float* gamma, const float* beta, float* stats,
                              const void* skip_z16, const float* skip_stats, float* y, void* y16, int B, long long L, int post_leaky,
                              float alpha, void* stream);

/* 1 where lgadj_convT_s2_fwd_stats_ns runs: the shapes of conv_up3.hip's two forward tilings (Hs % 8 == 0, Ws % 16 == 0,
 * cs -> cb = 128 -> 64 or 64 -> 32, dtype bf16) with its kill switches off.  Hs x Ws: the SOURCE map, as lg_convT_s2_fwd_stats. */
int lgadj_convT_s2_fwd_ns_supported(int B, int Hs, int Ws, int cb, int cs, int dtype);

/* lg_convT_s2_fwd_stats (bf16 result y16 [B][2Hs][2Ws][cb], moment partials in spart, *nparts records per sample) of the input
 *     x = bf16(leaky_alpha(norm(z16; zstats)) + skip)        lg_instnorm_leaky_apply_z16_p's value with a bf16 skip (one rounding)
 * formed while the kernel stages its operand: x is never written.  z16: raw bf16 [B][Hs][Ws][cs] with its finished records zstats.
 * The skip comes as two row ranges: samples [0, b1) from skip0, samples [b1, B) from skip1 (0 <= b1 <= B; the pointer of an empty
 * range is not read).  A range whose *_stats pointer is null is a bf16 map [rows][Hs][Ws][cs]; otherwise it is a raw bf16 z of that
 * shape with its records [rows][8], normalised to h (above) before the add.  Pixels outside the image are zeros of x (SAME padding).
 * spart: lg_conv_stats_workspace_bytes(1, B, Hs, Ws, cb) bytes.  LG_ERR_UNSUPPORTED unless ..._ns_supported. */
int lgadj_convT_s2_fwd_stats_ns(const void* z16, const float* zstats, float alpha, const void* skip0, const float* skip0_stats,
                                const void* skip1, const float* skip1_stats, int b1, const void* pack, const float* bias, void* y16,
                                int B, int Hs, int Ws, int cb, int cs, int dtype, void* spart, size_t spart_bytes, int* nparts,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif
