// The library's internal interface: the ONE prototype of every function that is defined in one .hip file, used from another and not
// part of the public C ABI (include/littlegan_hip.h, which lg_common.h includes); the run-time services every kernel file uses
// (lg_set_error, lg_note_kernel, lg_env_flag, ...) stay declared in lg_common.h.  Every .hip file includes this header, so the compiler
// sees the declaration beside both the definition and each call; the build's -Werror=missing-prototypes refuses a non-static function
// that is declared nowhere.  The names keep C linkage (the exported symbol set is part of what tests/test_abi.py pins down).
// Convention of the *_try functions: LG_OK = launched, LG_ERR_UNSUPPORTED = the shape is not this kernel's, the caller takes the next one.
#pragma once
#include "lg_common.h"
#include "../../include/littlegan_guard.h"   // the lgg_ group: public; defined in gradguard.hip and loss_optim.hip
#include "../../include/littlegan_blur.h"    // the lgblur_ group: public; defined in dblur.hip

// Contraction forms of the implicit-GEMM convs (conv_igemm.hip, conv_halo.hip; chosen by capi.hip):
//   DOWN : src [B,2Hm,2Wm,Cs] -> out [B,Hm,Wm,N]
//   UP   : src [B,Hm,Wm,Cs]   -> out [B,2Hm,2Wm,N]
//   S1T  : src [B,Hm,Wm,Cs]   -> out [B,Hm,Wm,N]   (+ optional tanh)
//   PATCH: src [B,Hs,Ws,3], stride s, pad p -> out [B,Hm,Wm,N]; wp = [5][Npad][16]   (conv_igemm.hip only)
enum { MODE_DOWN = 0, MODE_UP = 1, MODE_S1T = 2, MODE_PATCH = 3 };

// ---- conv_igemm.hip ----
extern "C" int lg_npad(int n);   // columns of a weight pack: n where n % 64 == 0, else n rounded up to 32
extern "C" int lg_conv_igemm(int mode, int dtype, const float* src, const void* wpack, const float* bias, float* out,
                             int B, int Hm, int Wm, int Cs, int N, int act, int pstride, int ppad, void* stream);
// same, with an optional bf16 mirror src16 of the source, an optional bf16 destination out16 (instead of out) and optional fused
// InstanceNorm moment partials (*nparts_out == 0: the chosen kernel did not produce them)
extern "C" int lg_conv_igemm_ex(int mode, int dtype, const float* src, const void* src16, const void* wpack,
                                const float* bias, float* out, void* out16, int B, int Hm, int Wm, int Cs, int N, int act,
                                int pstride, int ppad, void* spart, size_t spart_bytes, int* nparts_out, void* stream);

// ---- conv_halo.hip ----
// spart / nparts_out (optional): with ONE sample per block the kernel also writes per-block InstanceNorm moments,
// *nparts_out = partial records per sample (0 = not produced).  out == out16 == null: dry run, the answer alone.
extern "C" int lg_conv_halo_try(int mode, int dtype, const float* src, const void* src16, const void* wpack,
                                const float* bias, float* out, void* out16, int B, int Hm, int Wm, int Cs, int N, int act, void* spart,
                                size_t spart_bytes, int* nparts_out, void* stream);

// ---- conv_down3.hip ----
extern "C" int lg_conv_down3_supported(int B, int Hm, int Wm, int Cs, int N);
extern "C" int lg_conv_down3_zn_supported(int B, int Hm, int Wm, int Cs, int N);   // NORM form
extern "C" int lg_conv_down3_bn_supported(int B, int Hm, int Wm, int Cs, int N);   // BWDNORM form
extern "C" int lg_conv_down3_try(const void* src16, const void* wpack, const float* bias, void* out16, int B, int Hm, int Wm,
                                 int Cs, int N, void* spart, size_t spart_bytes, int* nparts_out, void* stream);
// nf (optional; data-gradient use): also the norm-backward sums of the produced gradient ([B][*nparts_out][2] doubles in nf->part)
extern "C" int lg_conv_down3_nf_try(const void* src16, const void* wpack, const float* bias, void* out16, int B, int Hm, int Wm,
                                    int Cs, int N, void* spart, size_t spart_bytes, int* nparts_out, const LgNormFuse* nf,
                                    size_t nf_bytes, void* stream);
// fed with the RAW bf16 output z16 of the layer below and its statistics records; the moments of the produced map are always fused
extern "C" int lg_conv_down3_zn_try(const void* z16, const float* zstats, float alpha, const void* wpack, const float* bias, void* out16,
                                    int B, int Hm, int Wm, int Cs, int N, void* spart, size_t spart_bytes, int* nparts_out, void* stream);
// data gradient of a transposed conv fed with (z16, g16, coef) of its level instead of dz16; the sums of the next level (nf) always fused
extern "C" int lg_conv_down3_bn_try(const void* z16, const void* g16, const float* bcoef, float alpha, const void* wpack, void* out16,
                                    int B, int Hm, int Wm, int Cs, int N, int* nparts_out, const LgNormFuse* nf, size_t nf_bytes,
                                    void* stream);

// ---- conv_up3.hip / conv_up4.hip ----  Hm, Wm: the SOURCE (small) map; *nparts_out = records per sample; nf as above
extern "C" int lg_conv_up3_supported(int B, int Hm, int Wm, int Cs, int N);
extern "C" int lg_conv_up3_try(const void* src16, const void* wpack_up, const float* bias, void* out16, int B, int Hm, int Wm,
                               int Cs, int N, void* spart, size_t spart_bytes, int* nparts_out, void* stream);
extern "C" int lg_conv_up3_nf_try(const void* src16, const void* wpack_up, const float* bias, void* out16, int B, int Hm, int Wm,
                                  int Cs, int N, void* spart, size_t spart_bytes, int* nparts_out, const LgNormFuse* nf,
                                  size_t nf_bytes, void* stream);
extern "C" int lg_conv_up4_supported(int B, int Hm, int Wm, int Cs, int N);
extern "C" int lg_conv_up4_try(const void* src16, const void* wpack_up, const float* bias, void* out16, int B, int Hm, int Wm,
                               int Cs, int N, void* spart, size_t spart_bytes, int* nparts_out, void* stream);
extern "C" int lg_conv_up4_nf_try(const void* src16, const void* wpack_up, const float* bias, void* out16, int B, int Hm, int Wm,
                                  int Cs, int N, void* spart, size_t spart_bytes, int* nparts_out, const LgNormFuse* nf,
                                  size_t nf_bytes, void* stream);

// ---- n3_kernels.hip ----  the 3-channel layers on the VALU; w = the verbatim fp32 kernel (lg_conv_pack_raw_offset)
extern "C" int lg_n3_s1t_fwd_try(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int C,
                                 void* stream);
extern "C" int lg_n3_up_try(const float* src, const float* w, float* out, int B, int H, int W, int C, void* stream);
extern "C" size_t lg_n3_wgrad_workspace_bytes(int B, int H, int W, int Cs);
extern "C" int lg_n3_wgrad_try(const float* big3, const float* small, const void* small16, float* dw, void* workspace,
                               size_t ws_bytes, int B, int H, int W, int Cs, int s, int pad, int accumulate, void* stream);

// ---- n3_pgemm.hip ----  the same layers as tap-product GEMMs from the bf16 mirrors
extern "C" int lg_n3_p16_supported(int H, int W, int C);
extern "C" int lg_n3_s1t_fwd_p16_try(const void* x16, const float* w, const float* bias, float* y, int B, int H, int W,
                                     int C, void* stream);
extern "C" int lg_n3_up_p16_try(const void* src16, const float* w, float* out, int B, int H, int W, int C, void* stream);
extern "C" int lg_n3_conv1_p16_supported(int H, int W, int N);
// conv1 forward from the fp32 image, with the per-block InstanceNorm moments; *nparts = records per sample
extern "C" int lg_n3_conv1_fwd_p16_try(const float* img, const float* w, const float* bias, float* z, void* z16, int B, int H,
                                       int W, int N, void* spart, size_t spart_bytes, int* nparts, void* stream);
// data gradient of the final stride-1 layer: dpre [B,H,W,3] fp32 -> dx [B,H,W,32] as bf16 (dx16) or fp32 (dx);
// nf (optional, bf16 output): also the norm-backward sums of the produced gradient, [B][*nparts_out][2] doubles
extern "C" int lg_n3_s1_dgrad_p16_try(const float* dpre, const float* w, float* dx, void* dx16, int B, int H, int W, int N,
                                      void* stream);
extern "C" int lg_n3_s1_dgrad_p16_nf_try(const float* dpre, const float* w, float* dx, void* dx16, int B, int H, int W, int N,
                                         const LgNormFuse* nf, size_t nf_bytes, int* nparts_out, void* stream);

// ---- n3_rows.hip ----
extern "C" int lg_n3_rows_supported(int H, int W, int C);
// x16: the bf16 input h [B,H,W,C]; or, with stats != null, the raw bf16 conv output z of the level below, normalised +
// LeakyReLU(alpha)'d on the fly from its statistics records [B][8]
extern "C" int lg_n3_s1t_fwd_rows_try(const void* x16, const float* stats, float alpha, const float* w, const float* bias, float* y,
                                      int B, int H, int W, int C, void* stream);

// ---- pack.hip ----  byte offsets inside a layer pack (the down pack is at 0), both 256-B aligned
extern "C" size_t lg_conv_pack_up_offset(int cb, int cs, int dtype);
extern "C" size_t lg_conv_pack_raw_offset(int cb, int cs, int dtype);   // cb == 3: the verbatim fp32 kernel [5][5][3][cs]

// ---- heads.hip ----  the partials stage of the heads forward (route, split of K, GEMM launch): part[*nkc_out][B][1 + c]; arguments checked
// by the caller (lg_heads_fwd, lgo_heads_fwd)
extern "C" int lg_heads_fwd_partials(const float* x, const float* wpr, const float* wc, float* part, int B, int K, int c, int* nkc_out,
                                     void* stream);

// ---- skinny_mfma.hip ----  the dense / head GEMMs on the exact-f32 MFMA
extern "C" int lg_heads_fwd_mfma_try(const float* x, const float* wpr, const float* wc, float* part, int B, int K, int c,
                                     int* nkc_out, void* stream);
extern "C" int lg_heads_wgrad_mfma_try(const float* x, const float* dz, float* dwpr, float* dbpr, float* dwc, float* dbc, int B,
                                       int K, int c, int accumulate, void* stream);
extern "C" int lg_heads_dgrad_mfma_try(const float* dz, const float* wpr, const float* wc, float* dx, int B, int K, int c,
                                       void* stream);
extern "C" int lg_dense_fwd_mfma_try(const float* x, const float* w, const float* bias, float* y, int B, int K, int N,
                                     void* stream);
extern "C" int lg_dense_wgrad_mfma_try(const float* x, const float* dy, float* dw, float* db, int B, int K, int N, int accumulate,
                                       void* stream);

// ---- wgrad_at.hip / wgrad_at32.hip ----  write slab[nsplit][25][cb][cs] into `workspace` and *nsplit_out; lg_conv_wgrad_m16 reduces
extern "C" size_t lg_wgrad_at_workspace_bytes(int B, int Hm, int Wm, int cb, int cs);
extern "C" int lg_wgrad_at_try(const void* big16, const void* small16, void* workspace, size_t ws_bytes, int B, int Hm, int Wm,
                               int cb, int cs, int* nsplit_out, void* stream);
extern "C" size_t lg_wgrad_at32_workspace_bytes(int B, int Hm, int Wm, int cb, int cs);
extern "C" int lg_wgrad_at32_try(const float* big, const float* small, void* workspace, size_t ws_bytes, int B, int Hm, int Wm,
                                 int cb, int cs, int* nsplit_out, void* stream);

// ---- wgrad_igemm.hip ----
// dW[5][5][cb][cs] (+)= big (x) small ; big [B,s*Hm,s*Wm,cb], small [B,Hm,Wm,cs].  cb == 3 selects the patch form with source
// stride `pstride` and pad-before `ppad` (conv1: 2,1 ; stride-1 final layer: 1,2); otherwise stride 2 / pad 1.
extern "C" int lg_conv_wgrad(const float* big, const float* small, float* dw, void* workspace, size_t ws_bytes, int B,
                             int Hm, int Wm, int cb, int cs, int pstride, int ppad, int accumulate, int dtype,
                             void* stream);
extern "C" int lg_conv_wgrad_m16(const float* big, const void* big16, const float* small, const void* small16, float* dw,
                                 void* workspace, size_t ws_bytes, int B, int Hm, int Wm, int cb, int cs, int pstride,
                                 int ppad, int accumulate, int dtype, void* stream);
