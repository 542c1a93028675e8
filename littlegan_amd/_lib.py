"""ctypes binding of liblittlegan_hip.so.  The C ABI is every function declared in include/littlegan_*.h; SIGNATURES below is its one
table (tests/test_abi.py holds it to the headers and to the symbols the library exports).  A new group is a new
include/littlegan_<group>.h with `lg<group>_` names: its entries go in SIGNATURES, its rows in tests/test_memory_contract_gpu.py.

The product path has NO fallback: if the shared library is missing this module raises at
import of the symbol table, and every op raises `LittleGanHipError` on a non-zero return.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblittlegan_hip.so")

DT_F32, DT_BF16 = 0, 1

P, I, L, F, Z = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_size_t

# name -> (restype, [argtypes])
SIGNATURES = {
    "lg_abi_version": (I, []),
    "lg_last_error": (C.c_char_p, []),
    "lg_conv_pack_bytes": (Z, [I, I, I]),
    "lg_conv_pack": (I, [P, P, I, I, I, P]),
    "lg_conv2d_s2_fwd": (I, [P, P, P, P, I, I, I, I, I, I, P]),
    "lg_conv_stats_workspace_bytes": (Z, [I, I, I, I, I]),
    "lg_conv_fwd_stats_fused": (I, [I, I, I, I, I, I, I]),
    "lg_conv2d_s2_fwd_stats": (I, [P, P, P, P, P, P, I, I, I, I, I, I, P, Z, P, P]),
    "lg_conv2d_s2_dgrad_m16": (I, [P, P, P, P, P, I, I, I, I, I, I, P]),
    "lg_conv2d_s2_wgrad_m16": (I, [P, P, P, P, P, P, Z, I, I, I, I, I, I, I, P]),
    "lg_conv2d_s2_dgrad": (I, [P, P, P, I, I, I, I, I, I, P]),
    "lg_conv2d_s2_wgrad": (I, [P, P, P, P, Z, I, I, I, I, I, I, I, P]),
    "lg_convT_s2_fwd": (I, [P, P, P, P, I, I, I, I, I, I, P]),
    "lg_convT_s2_fwd_stats": (I, [P, P, P, P, P, P, I, I, I, I, I, I, P, Z, P, P]),
    "lg_convT_s2_dgrad_m16": (I, [P, P, P, P, P, I, I, I, I, I, I, P]),
    "lg_convT_s2_wgrad_m16": (I, [P, P, P, P, P, P, Z, I, I, I, I, I, I, I, P]),
    "lg_convT_s2_dgrad": (I, [P, P, P, I, I, I, I, I, I, P]),
    "lg_convT_s2_wgrad": (I, [P, P, P, P, Z, I, I, I, I, I, I, I, P]),
    "lg_wgrad_workspace_bytes": (Z, [I, I, I, I, I, I]),
    "lg_convT_s1_tanh_fwd": (I, [P, P, P, P, I, I, I, I, I, I, P]),
    "lg_convT_s1_tanh_bwd": (I, [P, P, P, P, P, P, P, Z, I, I, I, I, I, I, I, P]),
    "lg_convT_s1_bwd_workspace_bytes": (Z, [I, I, I, I, I, I]),
    "lg_n3_m16_supported": (I, [I, I, I, I, I]),
    "lg_convT_s1_tanh_fwd_m16": (I, [P, P, P, P, P, I, I, I, I, I, I, P]),
    "lg_conv2d_s2_fwd_stats_zn_supported": (I, [I, I, I, I, I, I]),
    "lg_conv2d_s2_fwd_stats_zn": (I, [P, P, F, P, P, P, I, I, I, I, I, I, P, Z, P, P]),
    "lg_convT_s1_tanh_fwd_z16_supported": (I, [I, I, I, I, I]),
    "lg_convT_s1_tanh_fwd_z16": (I, [P, P, F, P, P, P, I, I, I, I, I, I, P]),
    "lg_convT_s1_tanh_bwd_m16": (I, [P, P, P, P, P, P, P, P, P, Z, I, I, I, I, I, I, I, P]),
    "lg_bias_grad_workspace_bytes": (Z, [L, I]),
    "lg_bias_grad": (I, [P, P, P, Z, L, I, I, P]),
    "lg_bias_grad_m16": (I, [P, P, P, P, Z, L, I, I, P]),
    "lg_conv_halo_supported": (I, [I, I, I, I, I, I, I]),
    "lg_instnorm_workspace_bytes": (Z, [I, L]),
    "lg_instnorm_stats_stride": (I, []),
    "lg_instnorm_leaky_stats": (I, [P, P, P, P, P, Z, I, L, I, F, P]),
    "lg_instnorm_leaky_stats_z16": (I, [P, P, P, P, P, Z, I, L, I, F, P, P]),
    "lg_instnorm_stats_finalize": (I, [P, I, P, P, P, I, P]),
    "lg_instnorm_leaky_apply": (I, [P, P, P, P, P, I, L, I, I, F, P]),
    "lg_instnorm_leaky_bwd": (I, [P, P, P, I, P, P, P, P, P, Z, I, L, I, I, F, I, P]),
    "lg_instnorm_bwd_db_workspace_bytes": (Z, [I, L, I]),
    "lg_instnorm_leaky_bwd_db": (I, [P, P, P, I, P, P, P, P, P, I, P, Z, I, L, I, I, F, I, P]),
    "lg_last_kernel": (C.c_char_p, []),
    "lg_clear_kernel": (I, []),
    "lg_instnorm_last_launches": (C.c_char_p, []),
    "lg_instnorm_leaky_apply_z16": (I, [P, P, P, I, P, P, I, L, I, I, F, P]),
    "lg_instnorm_leaky_apply_z16_p": (I, [P, P, I, P, P, P, P, I, P, P, I, L, I, F, P]),
    "lg_instnorm_leaky_bwd_z16": (I, [P, P, P, I, P, P, P, P, P, I, P, Z, I, L, I, I, F, I, P]),
    "lg_instnorm_leaky_bwd_z16_p": (I, [P, P, P, I, P, P, P, P, P, I, P, I, P, Z, I, L, I, I, F, I, P]),
    "lg_conv2d_s2_dgrad_nf": (I, [P, P, P, I, I, I, I, I, P, P, F, P, Z, P, P]),
    "lg_convT_s2_dgrad_nf": (I, [P, P, P, I, I, I, I, I, P, P, F, P, Z, P, P]),
    "lg_convT_s2_dgrad_bn_supported": (I, [I, I, I, I, I]),
    "lg_convT_s2_dgrad_bn": (I, [P, P, P, F, P, P, I, I, I, I, I, P, P, F, P, Z, P, P]),
    "lg_instnorm_bwd_coef": (I, [P, P, I, P, I, L, P]),
    # encoder dropout (dropout_train): the mask made testable + the dropped twins of the encoder's norm passes (norm.hip)
    "lg_dropout_key": (I, [P, L, L, P]),   # seed / key_offset: unsigned long long in C, passed as their 64-bit pattern
    "lg_dropout_mask": (I, [P, I, I, I, I, L, F, P, P]),
    "lg_instnorm_leaky_apply_drop": (I, [P, P, P, P, I, L, F, P, I, I, I, F, P]),
    "lg_instnorm_leaky_apply_z16_drop": (I, [P, P, P, P, I, L, F, P, I, I, I, F, P]),
    "lg_instnorm_leaky_apply_z16_p_drop": (I, [P, P, I, P, P, P, P, P, I, L, F, P, I, I, I, F, P]),
    "lg_instnorm_leaky_bwd_drop": (I, [P, P, P, I, P, P, P, P, P, I, P, Z, I, L, F, I, P, I, I, I, F, P]),
    "lg_instnorm_leaky_bwd_z16_drop": (I, [P, P, P, I, P, P, P, P, P, I, P, I, P, Z, I, L, F, I, P, I, I, I, F, P]),
    "lg_convT_s1_tanh_bwd_nf": (I, [P, P, P, P, P, P, P, P, Z, I, I, I, I, I, I, I, P, P, F, P, Z, P, P]),
    "lg_dense_fwd": (I, [P, P, P, P, I, I, I, P]),
    "lg_dense_wgrad": (I, [P, P, P, P, I, I, I, I, P]),
    "lg_dense_dgrad": (I, [P, P, P, I, I, I, P]),
    "lg_concat_cols": (I, [P, I, P, I, P, I, P]),
    "lg_adj_conditions": (I, [P, P, P, P, I, I, P]),
    "lg_heads_fwd_workspace_bytes": (Z, [I, I, I]),
    "lg_heads_fwd": (I, [P, P, P, P, P, P, P, Z, I, I, I, P]),
    "lg_heads_dgrad": (I, [P, P, P, P, I, I, I, P]),
    "lg_heads_wgrad": (I, [P, P, P, P, P, P, I, I, I, I, P]),
    "lg_bce_heads_loss_fwd_bwd": (I, [P, P, F, F, F, P, P, I, I, I, P]),
    "lg_l1_workspace_bytes": (Z, []),
    "lg_l1_tanh_loss_fwd_bwd": (I, [P, P, P, P, P, P, Z, L, F, I, P]),
    "lg_clip_adam_update": (I, [P, P, P, P, L, P, F, F, F, F, F, F, P]),
    "lg_adam_advance": (I, [P, F, F, P]),
    "lg_axpby": (I, [P, P, F, F, L, P]),
    # weight average for sampling (loss_optim.hip): fused into the Adam pass; the counter's advance; raw <-> averaged swap
    "lg_clip_adam_ema_update": (I, [P, P, P, P, P, L, L, L, P, P, F, F, F, F, F, F, F, P]),
    "lg_ema_advance": (I, [P, P]),
    "lg_swap_f32": (I, [P, P, L, P]),
    "lg_philox4x32": (I, [P, I, L, L, P]),   # seed / offset: unsigned long long in C, passed as their 64-bit pattern
    "lg_randn": (I, [P, L, F, F, L, L, P]),
    "lg_augment_workspace_bytes": (Z, [I]),
    "lg_augment": (I, [P, P, I, I, I, P, F, F, F, F, L, L, P, Z, P]),
    "lg_fid_stats_workspace_bytes": (Z, [L, I]),
    "lg_fid_stats": (I, [P, L, I, P, P, P, Z, P]),
    # streaming statistics + the Frechet distance on the device (fid.hip, fid_sqrt.hip); replace fid.py:185-188 / :144-163
    "lg_fid_accum": (I, [P, L, I, P, P, P, P]),
    "lg_fid_finalize": (I, [P, P, P, L, I, P, P, P]),
    "lg_fid_gemm": (I, [P, P, P, I, P, P]),
    "lg_fid_distance_workspace_bytes": (Z, [I]),
    "lg_fid_distance": (I, [P, P, P, P, I, I, P, P, Z, P]),
    # pairwise passes of KID / precision / recall / density / coverage (pairs.hip); no counterpart in the reference
    "lg_pairs_workspace_bytes": (Z, [L, L, I]),
    "lg_pairs_poly_sum": (I, [P, L, P, L, I, I, P, I, P, P, Z, P]),
    "lg_pairs_knn": (I, [P, L, P, L, I, I, P, P, Z, P]),
    "lg_pairs_ball_count": (I, [P, L, P, L, P, I, P, P, Z, P]),
    "lg_augment_drawn_workspace_bytes": (Z, [I]),
    "lg_device_cus": (I, []),
    "lg_set_reserved_cus": (I, [I]),
    "lg_grid_cus": (I, []),
    "lg_contention_probe": (I, [P, P, L, I, I, I, P]),
    "lg_set_clock_census": (I, [P]),
    "lg_clock_sample": (I, [P, I, P]),
    "lg_augment_drawn": (I, [P, P, I, I, I, F, F, F, F, F, L, L, L, P, Z, P]),
    # discriminator gradient penalty (gp.hip; eps draw in augment.hip)
    "lg_gp_draw_eps": (I, [P, I, L, L, P]),
    "lg_gp_interp": (I, [P, P, P, P, I, L, P]),
    "lg_gp_workspace_bytes": (Z, [I, L]),
    "lg_gp_seed": (I, [P, P, P, P, P, F, P, Z, I, L, P]),
    "lg_gp_norm_bwd": (I, [P, P, P, P, P, P, P, P, P, P, P, Z, I, L, F, P]),
    "lg_gp_norm_dd": (I, [P, P, P, P, P, P, P, P, P, P, Z, I, L, F, P]),
    "lg_gp_heads_seed": (I, [P, P, P, I, I, I, P]),
    "lg_gp_heads_2nd": (I, [P, P, P, P, P, P, P, P, I, I, I, P]),
    # differentiable augmentation of D's inputs (diffaug.hip): per-row draws, T and its adjoint
    "lg_diffaug_draw": (I, [P, I, I, I, I, I, P, P]),
    "lg_diffaug_workspace_bytes": (Z, [I, I]),
    "lg_diffaug_fwd": (I, [P, P, P, I, I, P, Z, P]),
    "lg_diffaug_bwd": (I, [P, P, P, I, I, P, Z, P]),
    # packed uint8 data set: gather + rescale, labels, fused augmentation (input_u8.hip)
    "lg_rescale_u8": (I, [P, P, I, L, P, P]),
    "lg_soft_labels": (I, [P, P, P, I, I, I, P, P]),
    "lg_augment_drawn_u8_workspace_bytes": (Z, [I]),
    "lg_augment_drawn_u8": (I, [P, P, P, P, I, I, I, F, F, F, F, F, L, L, L, P, Z, P]),
    # training-control extensions (include/littlegan_hip_ext.h)
    # adaptive augmentation probability (ada.hip): the gated draw and the controller of p; state = 16 device bytes
    "lgx_diffaug_draw_gated": (I, [P, I, I, I, I, I, P, P, P]),
    "lgx_ada_init": (I, [P, F, P]),
    "lgx_ada_accumulate": (I, [P, P, I, I, P]),
    "lgx_ada_adjust": (I, [P, I, F, F, P]),
    # regularisers beyond the reference's recipe (include/littlegan_hip_reg.h)
    # R1 gradient penalty (r1.hip): the top seed, the seed on the image gradient, the heads' column sum
    "lgr_r1_workspace_bytes": (Z, [I, L]),
    "lgr_r1_heads_seed": (I, [P, P, I, I, P]),
    "lgr_r1_seed": (I, [P, P, P, P, P, F, P, Z, I, L, P]),
    "lgr_r1_colsum_workspace_bytes": (Z, [I, I]),
    "lgr_r1_heads_colsum": (I, [P, P, P, Z, I, I, P]),
    # logit-side GAN objectives (include/littlegan_hip_obj.h)
    # gan_loss (objective.hip): the heads forward that keeps the logit of output_pr, and the loss on it
    "lgo_heads_fwd": (I, [P, P, P, P, P, P, P, P, Z, I, I, I, P]),
    "lgo_gan_heads_loss_fwd_bwd": (I, [P, P, P, I, I, F, F, P, P, I, I, I, P]),
    # geometric augmentation of D's inputs (include/littlegan_geom.h; geom.hip): the per-row draw, Geo and its adjoint
    "lgeo_draw": (I, [P, I, I, I, I, I, P, P, P]),
    "lgeo_fwd": (I, [P, P, P, I, I, P]),
    "lgeo_bwd": (I, [P, P, P, I, I, P]),
    # the relativistic pairing objective and the R1 + R2 seed (include/littlegan_rel.h; objective.hip, r1.hip)
    "lgrel_pair_heads_loss_fwd_bwd": (I, [P, P, P, P, I, I, F, F, P, P, I, I, I, I, P]),
    "lgrel_r12_workspace_bytes": (Z, [I, L]),
    "lgrel_r12_seed": (I, [P, P, P, P, P, P, F, F, P, Z, I, L, P]),
    # the learning-rate schedule on the device and the Adam passes that read their rate from its state (include/littlegan_sched.h;
    # sched.hip, loss_optim.hip)
    "lgsch_init": (I, [P, I, P]),
    "lgsch_step": (I, [P, I, I, I, F, F, F, F, P]),
    "lgsch_clip_adam_update": (I, [P, P, P, P, L, P, P, F, F, F, F, F, P]),
    "lgsch_clip_adam_ema_update": (I, [P, P, P, P, P, L, L, L, P, P, P, F, F, F, F, F, F, P]),
    # the Adjuster's forward without its single-reader normalised maps (include/littlegan_adj.h; norm_rs.hip, conv_up3.hip)
    "lgadj_instnorm_apply_rs": (I, [P, P, P, P, P, P, I, L, I, F, P]),
    "lgadj_instnorm_apply_p_rs": (I, [P, P, I, P, P, P, P, P, P, P, I, L, I, F, P]),
    "lgadj_convT_s2_fwd_ns_supported": (I, [I, I, I, I, I, I]),
    "lgadj_convT_s2_fwd_stats_ns": (I, [P, P, F, P, P, P, P, I, P, P, P, I, I, I, I, I, I, P, Z, P, P]),
    # global-norm gradient clipping and the non-finite step guard (include/littlegan_guard.h; gradguard.hip, loss_optim.hip):
    # the fp64 sum of squares, the record, and the Adam passes that read their scale and skip flag from it
    "lgg_partials_count": (I, [L]),
    "lgg_workspace_bytes": (Z, [L]),
    "lgg_init": (I, [P, I, I, P]),
    "lgg_sumsq_partial": (I, [P, L, P, Z, P]),
    "lgg_finalise": (I, [P, L, P, F, F, I, P]),
    "lgg_clip_adam_update": (I, [P, P, P, P, L, P, P, P, F, F, F, F, P]),
    "lgg_clip_adam_ema_update": (I, [P, P, P, P, P, L, L, L, P, P, P, P, F, F, F, F, F, P]),
    "lgg_adam_advance": (I, [P, P, F, F, P]),
    # the faded blur of D's inputs (include/littlegan_blur.h; dblur.hip): the state, its step, Blur (its own adjoint)
    "lgblur_init": (I, [P, L, P]),
    "lgblur_step": (I, [P, F, L, L, P]),
    "lgblur_apply": (I, [P, P, P, I, I, P]),
}


class LittleGanHipError(RuntimeError):
    pass


_lib = None


def load():
    """Loads the HIP library (once).  Raises if it has not been built: there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LittleGanHipError(
            f"{LIB_PATH} not found: build it with `python -m littlegan_amd.csrc.build` "
            "(the LittleGAN hot path has no CPU fallback)")
    # Probe / ablation variants (scripts/probe/*: LG_EXTRA_FLAGS macros, "results wrong, timing only") live in their own
    # liblittlegan_hip_<variant>.so and are loaded ONLY when LG_LIB_VARIANT names one; the product library must have been
    # linked with the default flags.
    from .csrc import build as _build
    variant = os.environ.get("LG_LIB_VARIANT") or None
    path = _build.variant_paths(variant)[1]
    if variant is None:
        fl = _build.built_flags()
        if fl is not None and fl != " ".join(_build.FLAGS):
            raise LittleGanHipError(f"{LIB_PATH} was built with non-default flags ({fl!r}); rebuild with `python -m littlegan_amd.csrc.build`")
    elif not os.path.exists(path):
        raise LittleGanHipError(f"{path} not found: build it with LG_EXTRA_FLAGS=... python -m littlegan_amd.csrc.build --variant {variant}")
    # torch first: it ships its own libamdhip64 and must be the HIP runtime of the process.  If this library were loaded
    # before torch, the system runtime it links against would come in as a SECOND runtime and its kernels would see no device.
    import torch  # noqa: F401
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.lg_abi_version() != 1:
        raise LittleGanHipError("liblittlegan_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().lg_last_error().decode("utf-8", "replace")
        raise LittleGanHipError(f"{what} failed (rc={rc}): {msg}")
