"""Mirror of /root/reference/config.py:6-42: sample.config.json < <env>.config.json < CLI, every key an
attribute, derived cond_dim / result_dir / gpu / prefetch.  Extra keys of this build: mfma_dtype ("f32" |
"bf16"), synthetic (bool: use the synthetic CelebA-shaped dataset), seed, packed_path / data_resident / fuse_input
(the packed uint8 data set, dataset.py), fid_chunk_rows / fid_device_sqrt (streamed FID statistics, device square root, fid.py), dropout_train (bool: make the encoder's
dropout(dropout_rate) live in the training step — the reference's, and the default here, is the identity),
ema_decay / sample_ema (exponential moving average of the weights, used for sampling and kept in checkpoints),
diff_augment (comma list out of color,translation,cutout: differentiable augmentation of every image the Discriminator sees in the
training step, the generator-side tapes differentiated through it; "" = off, the reference's step),
diff_augment_p / ada_target / ada_interval / ada_kimg (adaptive augmentation probability: each diff_augment component is applied per
row with probability p, fixed or driven on the device towards ada_target; null / null = every component always),
geom_augment (comma list out of xflip,rot90,scale,rotate: geometric augmentation of the same images — a per-sample affine resampling,
bilinear with zero fill, applied before diff_augment's map and differentiated through on the gen / adj tapes; gated by the same p;
"" = off),
evaluate_metrics (list out of fid, kid, prdc: what `evaluate` computes; ["fid"] = the reference's run) / evaluate_real_activations (the
real images' saved activations that kid and prdc need) / kid_subsets / kid_subset_size / prdc_k (metrics.py),
r1_gamma / r1_interval (R1 gradient penalty on the Discriminator's real-image logit, (r1_gamma r1_interval / 2) mean |dlogit/dx|^2 added
to the disc loss on every r1_interval-th step; 0 = off; excludes use_gp and dropout_train, allowed with diff_augment),
gan_loss ("bce" | "logistic" | "hinge" | "lsgan" | "wgan": the real / fake terms of the three losses; "bce" = the reference's sigmoid +
clipped cross entropy against 0.98 / 0.02, the others are taken on the pre-sigmoid value of output_pr without smoothing; "wgan" needs
use_gp, which then penalises the logit),
relativistic (bool: the real / fake terms become f0(D(real) - D(fake)) per pair of rows, f0 the D-real function of gan_loss, which must be
logistic, hinge or lsgan) / r2_gamma (the R1 penalty's twin on the fake rows D read, on R1's schedule: r1_interval, weight
r2_gamma r1_interval; 0 = off; excludes use_gp and dropout_train; with r1_gamma also on, one pass over the 2B-row batch carries both;
DESIGN.md §27),
lr_g / lr_d / lr_adj (base learning rate of the Generator's, the Discriminator's and the Adjuster's optimizer; null = lr) / lr_schedule
("constant" | "linear" | "cosine") / lr_warmup_steps / lr_decay_steps / lr_final_ratio (a factor s(k) on all three rates, k the number of
training steps taken over the whole run: (k + 1) / lr_warmup_steps during warm-up, then a linear or cosine decay over lr_decay_steps from 1
to lr_final_ratio, where it stays; it is computed on the device from a counter on the device, so replayed graphs follow it, and the
counter is part of the checkpoint; constant without warm-up = the step as it was),
clip_norm (null = off, or a number > 0: each optimizer's gradient is scaled so that its global L2 norm, taken in fp64 on the device after
the all-reduce, is at most clip_norm; the element-wise clip_range of D acts after it) / skip_nonfinite (bool: a network whose gradient
holds a NaN or an Inf this step keeps its weights, Adam slots and beta powers, and the event is counted; the norms and the counters live
on the device, so replayed graphs clip and skip by their own gradients, and the counters are part of the checkpoint; both off = the step
as it was),
blur_init_sigma / blur_fade_kimg (a Gaussian blur of every image the Discriminator reads in the training step, before geom_augment and
diff_augment, differentiated through on the gen / adj tapes: sigma falls linearly from blur_init_sigma to 0 while D sees its first
blur_fade_kimg thousand real images, computed on the device from a counter on the device, so replayed graphs follow it, and the counter
is part of the checkpoint; after the fade the step is the one without the key, launch for launch; 0 = off; excludes use_gp and
dropout_train)."""
import json
import os
from argparse import ArgumentParser

# hyper-parameter defaults of the reference (sample.config.json:1-54), kept in code so that the JSON files of this
# build only carry overrides
DEFAULTS = {
    'batch_size': 32,
    'image_channel': 3,
    'image_path': '/path/to/image',
    'attr_path': '/path/to/attr/list.txt',
    'image_ext': 'jpg',
    'image_dim': 128,
    'attr': [8, 15, 20, 22, 26, 36, 39],
    'noise_dim': 93,
    'init_dim': 8,
    'norm': 'instance',
    'conv_filter': [384, 256, 128, 64, 32],
    'kernel_size': 5,
    'leaky_alpha': 0.3,
    'dropout_rate': 0.5,
    'l1_lambda': 0.02,
    'lr': 5e-05,
    'beta_1': 0.5,
    'beta_2': 0.9,
    'epoch': 100,
    'use_gp': False,
    'gp_weight': 5.0,
    'use_clip': True,
    'clip_range': 0.5,
    'use_partition': True,
    'partition_interval': 4,
    'freq_gen': 100,
    'freq_test': 2000,
    'all_result_dir': '/path/to/LittleGAN-result',
    'test_data_dir': '/path/to/LittleGAN-test',
    'evaluate_pre_calculated': 'fid_stats_celeba_128_all.npz',
    'random_sample_batch': 4,
    'condition_sample_batch': 100,
    'evaluate_sample_size': 30000,
    'restore': True,
    'reuse': False,
    'train_adj': True,
    'prefetch_batch': 3,
    'threads': 8,
    # keys added by this build
    'mfma_dtype': 'f32', 'synthetic': False, 'seed': 0,
    # packed uint8 data set: directory written by `main.py pack`; where its bytes live ("auto" | true | false);
    # whether the step reads the bytes through the fused u8 input kernels
    'packed_path': None, 'data_resident': 'auto', 'fuse_input': True,
    # FID pass: rows per streamed block of activations (null: the whole matrix at once, the present path); whether
    # tr sqrt(S1 S2) is taken on the device by the fp64 Newton-Schulz iteration instead of scipy's sqrtm
    'fid_chunk_rows': None, 'fid_device_sqrt': False,
    # live encoder dropout: the reference declares dropout_rate and never applies it (model.py:25); with this key the
    # training step's encoder passes apply it (0 < dropout_rate < 1), masks regenerated inside the norm kernels.  Excludes use_gp.
    'dropout_train': False,
    # weight average for sampling: an exponential moving average of every weight, taken inside the Adam pass with the
    # semantics of tf.train.ExponentialMovingAverage(ema_decay, num_updates); 0 = off.  sample_ema: predict and the sampling modes read
    # the average instead of the raw last-step weights (only when ema_decay > 0).
    'ema_decay': 0.0, 'sample_ema': True,
    # differentiable augmentation of D's inputs (Zhao et al. 2020): a comma list out of color, translation, cutout.  The
    # real batch, the Generator's fakes and the Adjuster's outputs are transformed per sample before D reads them, and the gen / adj
    # tapes are differentiated through the transform.  "" = off.  Excludes use_gp and dropout_train.
    'diff_augment': '',
    # adaptive augmentation probability on top of diff_augment (Karras et al. 2020): each named component is applied to
    # each row with probability p.  diff_augment_p: the fixed (or, with ada_target, the initial) p; null = 1.0, today's path, or 0.0
    # when ada_target is set.  ada_target: null = p stays fixed; else p is driven on the device so that E[sign(D_logit(real))] meets it
    # (the paper uses 0.6), adjusted every ada_interval steps at a rate that takes p from 0 to 1 while D sees ada_kimg thousand real
    # images.  Both need diff_augment to name a component.
    'diff_augment_p': None, 'ada_target': None, 'ada_interval': 4, 'ada_kimg': 500,
    # geometric augmentation of D's inputs (the blitting / geometric group of Karras et al. 2020): a comma list out of
    # xflip, rot90, scale, rotate.  Every image D reads is resampled under a per-sample map M = R(theta) Q^k F / s (bilinear, zero fill)
    # before diff_augment's T, and the gen / adj tapes are differentiated through it; diff_augment_p / ada_target gate its components
    # with the same p.  "" = off.  Excludes use_gp and dropout_train.
    'geom_augment': '',
    # sample-based metrics beside FID: which metrics `evaluate` runs (a list out of fid, kid, prdc); the saved
    # activations of the real images that kid / prdc compare against (the stats file holds only mu and sigma; a path, relative ones
    # under test_data_dir); subsets and rows per subset of KID (0 subsets = one estimate over the full sets); k of the k-NN manifolds
    'evaluate_metrics': ['fid'], 'evaluate_real_activations': None, 'kid_subsets': 100, 'kid_subset_size': 1000, 'prdc_k': 3,
    # R1 gradient penalty (Mescheder et al. 2018, lazily as in Karras et al. 2020): on every r1_interval-th step
    # (batch_no % r1_interval == 0) disc_loss += (r1_gamma r1_interval / 2) mean_b |d logit(x_b) / d x_b|^2 over the real rows D read (under
    # diff_augment: the augmented rows, differentiated with respect to them).  r1_gamma 0 = off.  Excludes use_gp and dropout_train.
    'r1_gamma': 0.0, 'r1_interval': 16,
    # objective of the real / fake terms: "bce" = the reference's (sigmoid + clipped cross entropy against the smoothed
    # targets); "logistic" (non-saturating), "hinge", "lsgan", "wgan" are taken on the logit of output_pr, without label smoothing.  The
    # attribute and L1 terms are the same under every value.  "wgan" needs use_gp; under a logit-side objective use_gp penalises the logit.
    'gan_loss': 'bce',
    # relativistic pairing (Jolicoeur-Martineau 2018): with gan_loss logistic | hinge | lsgan, the real / fake terms of the
    # three losses become f0(z_r[b] - z_f[b]) (disc), f0(z_f[b] - z_r[b]) (gen) and f0(z_a[i] - z_r[i mod B]) (adj), f0 the kind's D-real
    # function, row b of the real half paired with row b of the fake half.  false = the terms of §25.
    'relativistic': False,
    # R2 gradient penalty (Huang et al. 2024): R1's term on the FAKE rows D read, on R1's schedule — on every
    # r1_interval-th step disc_loss += (r2_gamma r1_interval / 2) mean_b |d logit(x_b) / d x_b|^2.  0 = off.  With r1_gamma also on, both
    # penalties are one reverse-over-reverse pass over the 2B-row batch.  Excludes use_gp and dropout_train.
    'r2_gamma': 0.0,
    # learning rates per network and their schedule (the reference has one constant lr).  lr_g / lr_d / lr_adj: the base
    # rate of that optimizer, null = lr.  lr_schedule: "constant", "linear" or "cosine"; with k the number of training steps taken so far
    # (over the whole run, kept in the checkpoint) every rate is its base times s(k) = up(k) d(k): up = (k + 1) / lr_warmup_steps while
    # k < lr_warmup_steps, else 1; d falls from 1 to lr_final_ratio over the lr_decay_steps steps after warm-up (a straight line, or half
    # a cosine) and stays there.  lr_decay_steps is required by linear / cosine and refused with constant.  s is computed on the device.
    'lr_g': None, 'lr_d': None, 'lr_adj': None, 'lr_schedule': 'constant', 'lr_warmup_steps': 0, 'lr_decay_steps': None,
    'lr_final_ratio': 0.0,
    # global-norm gradient clipping and the non-finite step guard (the reference clips D element-wise and nothing else).
    # clip_norm: null = off, else each of the three optimizers scales its gradient by min(1, clip_norm / (N + 1e-6)), N the L2 norm of
    # the (all-reduced, averaged) gradient range it trains this step; clip_range still acts on D, after the scaling.  skip_nonfinite: a
    # network whose gradient holds a NaN or an Inf is left exactly as it was for this step (weights, Adam slots, beta powers) and the
    # skip is counted.  Allowed with every other key.
    'clip_norm': None, 'skip_nonfinite': False,
    # blur of D's inputs (the discriminator-input blur of Karras et al. 2021): every image D reads in the training step is
    # filtered with a normalised Gaussian of radius floor(3 sigma) (zero fill), before geom_augment and diff_augment, and the gen / adj
    # tapes are differentiated through it.  sigma = blur_init_sigma * max(1 - images D has seen / (1000 blur_fade_kimg), 0), computed
    # on the device; once the radius is 0 the step is the one without the key.  blur_init_sigma 0 = off (at most 10); blur_fade_kimg 200
    # is StyleGAN3's.  Not gated by diff_augment_p.  Excludes use_gp and dropout_train.
    'blur_init_sigma': 0.0, 'blur_fade_kimg': 200,
}

GAN_LOSS_KINDS = {"bce": 0, "logistic": 1, "hinge": 2, "lsgan": 3, "wgan": 4}   # the `kind` of lgo_gan_heads_loss_fwd_bwd; 0 = not its


def gan_loss_kind(name, use_gp=None) -> int:
    """The gan_loss key as the `kind` of lgo_gan_heads_loss_fwd_bwd (0 for "bce": the reference's objective, none of that code runs).
    Raises ValueError for anything but one of the five names as a string and, when use_gp is given (not None), for "wgan" without
    use_gp: the Wasserstein objective has no bound of its own and needs the penalty on the logit."""
    if not isinstance(name, str) or name not in GAN_LOSS_KINDS:
        raise ValueError(f"gan_loss must be one of {', '.join(GAN_LOSS_KINDS)} (a string), got {name!r}")
    if name == "wgan" and use_gp is not None and not use_gp:
        raise ValueError("gan_loss 'wgan' needs use_gp: the Wasserstein objective is unbounded without the gradient penalty on the logit "
                         "(DESIGN.md §25)")
    return GAN_LOSS_KINDS[name]

DIFF_AUGMENT_BITS = {"color": 1, "translation": 2, "cutout": 4}


def diff_augment_bits(policy) -> int:
    """The diff_augment key as the policy bits of lg_diffaug_draw (1 color, 2 translation, 4 cutout); "" or None = 0 (off).
    Raises ValueError for anything but a comma list of the three names."""
    if policy is None:
        return 0
    if not isinstance(policy, str):
        raise ValueError(f"diff_augment must be a string (a comma list out of {', '.join(DIFF_AUGMENT_BITS)}), got {policy!r}")
    bits = 0
    for name in (n.strip() for n in policy.split(",")) if policy.strip() else ():
        if name not in DIFF_AUGMENT_BITS:
            raise ValueError(f"diff_augment: unknown component {name!r} in {policy!r} (a comma list out of {', '.join(DIFF_AUGMENT_BITS)})")
        bits |= DIFF_AUGMENT_BITS[name]
    return bits


GEOM_AUGMENT_BITS = {"xflip": 1, "rot90": 2, "scale": 4, "rotate": 8}


def geom_augment_bits(policy) -> int:
    """The geom_augment key as the policy bits of lgeo_draw (1 xflip, 2 rot90, 4 scale, 8 rotate); "" or None = 0 (off).
    Raises ValueError for anything but a comma list of the four names."""
    if policy is None:
        return 0
    if not isinstance(policy, str):
        raise ValueError(f"geom_augment must be a string (a comma list out of {', '.join(GEOM_AUGMENT_BITS)}), got {policy!r}")
    bits = 0
    for name in (n.strip() for n in policy.split(",")) if policy.strip() else ():
        if name not in GEOM_AUGMENT_BITS:
            raise ValueError(f"geom_augment: unknown component {name!r} in {policy!r} (a comma list out of {', '.join(GEOM_AUGMENT_BITS)})")
        bits |= GEOM_AUGMENT_BITS[name]
    return bits


def ada_settings(diff_augment, diff_augment_p=None, ada_target=None, ada_interval=4, ada_kimg=500.0, geom_augment=""):
    """The four keys of the adaptive augmentation probability, validated: None when the step is the plain augmenting
    one (diff_augment_p null or 1.0 and ada_target null: every component applied to every row), else a dict {p0, target (None = a fixed
    p), interval, per_row} of the gated path.  Raises ValueError for a value out of range, and for diff_augment_p or ada_target set
    while neither diff_augment nor geom_augment (gated by the same p) names a component."""
    def number(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
            raise ValueError(f"{name} must be a number, got {v!r}")
        return float(v)
    if diff_augment_p is not None and not 0.0 <= number("diff_augment_p", diff_augment_p) <= 1.0:
        raise ValueError(f"diff_augment_p must be null or satisfy 0 <= diff_augment_p <= 1, got {diff_augment_p!r}")
    if ada_target is not None and not 0.0 < number("ada_target", ada_target) < 1.0:
        raise ValueError(f"ada_target must be null or satisfy 0 < ada_target < 1, got {ada_target!r}")
    if isinstance(ada_interval, bool) or not isinstance(ada_interval, int) or ada_interval < 1:
        raise ValueError(f"ada_interval must be an integer >= 1, got {ada_interval!r}")
    if not 0.0 < number("ada_kimg", ada_kimg) < float("inf"):
        raise ValueError(f"ada_kimg must be a positive number, got {ada_kimg!r}")
    import numpy as np
    with np.errstate(over="ignore"):
        per_row = float(np.float32(1.0 / (float(ada_kimg) * 1000.0)))
    if not 0.0 < per_row < float("inf"):
        raise ValueError(f"ada_kimg {ada_kimg!r}: 1 / (ada_kimg * 1000) must be a positive finite fp32 number")
    if (diff_augment_p is not None or ada_target is not None) and not diff_augment_bits(diff_augment) \
            and not geom_augment_bits(geom_augment):
        raise ValueError("diff_augment_p / ada_target need diff_augment to name a component (or geom_augment): there is nothing to gate "
                         f"(diff_augment = {diff_augment!r}, geom_augment = {geom_augment!r})")
    if ada_target is None and (diff_augment_p is None or float(diff_augment_p) == 1.0):
        return None
    return {"p0": float(np.float32(0.0 if diff_augment_p is None else diff_augment_p)),
            "target": None if ada_target is None else float(np.float32(ada_target)), "interval": int(ada_interval), "per_row": per_row}


def r1_settings(r1_gamma=0.0, r1_interval=16):
    """The two keys of the R1 penalty, validated: None when it is off (r1_gamma == 0), else a dict {gamma, interval,
    weight} with weight = gamma * interval, the factor a penalty step applies so that the lazily applied term averages to gamma.
    Raises ValueError for an r1_gamma that is no finite number >= 0 and for an r1_interval that is no integer >= 1 (bools refused),
    whether or not the penalty is on."""
    import math
    if isinstance(r1_gamma, bool) or not isinstance(r1_gamma, (int, float)) or not math.isfinite(r1_gamma) or r1_gamma < 0:
        raise ValueError(f"r1_gamma must be a finite number >= 0 (0 = off), got {r1_gamma!r}")
    if isinstance(r1_interval, bool) or not isinstance(r1_interval, int) or r1_interval < 1:
        raise ValueError(f"r1_interval must be an integer >= 1, got {r1_interval!r}")
    weight = float(r1_gamma) * r1_interval
    if not weight <= 3.0e38:
        raise ValueError(f"r1_gamma * r1_interval = {weight!r} does not fit fp32 (r1_gamma {r1_gamma!r}, r1_interval {r1_interval!r})")
    if r1_gamma == 0:
        return None
    return {"gamma": float(r1_gamma), "interval": int(r1_interval), "weight": weight}


def r2_settings(r2_gamma=0.0, r1_interval=16):
    """The R2 penalty's key on R1's schedule, validated as r1_settings validates its own: None when it is off
    (r2_gamma == 0), else {gamma, interval, weight} with weight = r2_gamma * r1_interval.  Raises ValueError for an r2_gamma that is no
    finite number >= 0 (bools and strings refused) and for a bad r1_interval."""
    import math
    if isinstance(r2_gamma, bool) or not isinstance(r2_gamma, (int, float)) or not math.isfinite(r2_gamma) or r2_gamma < 0:
        raise ValueError(f"r2_gamma must be a finite number >= 0 (0 = off), got {r2_gamma!r}")
    if isinstance(r1_interval, bool) or not isinstance(r1_interval, int) or r1_interval < 1:
        raise ValueError(f"r1_interval must be an integer >= 1, got {r1_interval!r}")
    weight = float(r2_gamma) * r1_interval
    if not weight <= 3.0e38:
        raise ValueError(f"r2_gamma * r1_interval = {weight!r} does not fit fp32 (r2_gamma {r2_gamma!r}, r1_interval {r1_interval!r})")
    if r2_gamma == 0:
        return None
    return {"gamma": float(r2_gamma), "interval": int(r1_interval), "weight": weight}


def relativistic_setting(relativistic=False, gan_loss="bce"):
    """The relativistic key, validated against gan_loss: a bool; True needs gan_loss logistic, hinge or lsgan — "bce" has
    no logit to pair, and the pairing of "wgan" is wgan itself.  Returns the bool."""
    if not isinstance(relativistic, bool):
        raise ValueError(f"relativistic must be true or false, got {relativistic!r}")
    if relativistic and gan_loss == "bce":
        raise ValueError("relativistic needs a logit-side gan_loss (logistic, hinge or lsgan): 'bce' is taken behind the sigmoid and has "
                         "no logit to pair (DESIGN.md §27)")
    if relativistic and gan_loss == "wgan":
        raise ValueError("relativistic excludes gan_loss 'wgan': f0(z_r - z_f) = -z_r + z_f is the wgan objective itself (DESIGN.md §27)")
    if relativistic and gan_loss not in ("logistic", "hinge", "lsgan"):
        raise ValueError(f"relativistic needs gan_loss logistic, hinge or lsgan, got {gan_loss!r}")
    return relativistic


LR_SCHEDULE_KINDS = {"constant": 0, "linear": 1, "cosine": 2}   # the `kind` of lgsch_step


def lr_schedule_settings(lr, lr_g=None, lr_d=None, lr_adj=None, lr_schedule="constant", lr_warmup_steps=0, lr_decay_steps=None,
                         lr_final_ratio=0.0):
    """The keys of the learning rates and their schedule, validated: a dict {lr_g, lr_d, lr_adj (the base rates as the
    fp32 values they are used at; a null key takes lr), schedule, kind (of lgsch_step), warmup, decay (None under constant), final_ratio
    (its fp32 value), device}.  device: the rates are computed on the device from its step counter — true exactly when lr_schedule is not
    "constant" or lr_warmup_steps > 0; false = the rates are the launch scalars they always were.  Raises ValueError for a rate that is no
    finite number > 0 fitting fp32 (bools and strings refused; lr itself may be 0, which freezes the weights, as long as nothing is
    scheduled), a schedule that is not one of the three names, lr_warmup_steps no integer >= 0, lr_decay_steps no integer >= 1, missing
    under linear / cosine or given under constant, and lr_final_ratio outside [0, 1]."""
    import math
    import numpy as np

    def number(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
        return float(v)

    def rate(name, v):
        with np.errstate(over="ignore"):
            r = float(np.float32(number(name, v)))
        if not 0.0 < r < float("inf"):
            raise ValueError(f"{name} must be a finite number > 0 that fits fp32, got {v!r}")
        return r

    if not isinstance(lr_schedule, str) or lr_schedule not in LR_SCHEDULE_KINDS:
        raise ValueError(f"lr_schedule must be one of {', '.join(LR_SCHEDULE_KINDS)} (a string), got {lr_schedule!r}")
    if isinstance(lr_warmup_steps, bool) or not isinstance(lr_warmup_steps, int) or not 0 <= lr_warmup_steps < 2 ** 31:
        raise ValueError(f"lr_warmup_steps must be an integer >= 0 (below 2^31), got {lr_warmup_steps!r}")
    if lr_decay_steps is not None and (isinstance(lr_decay_steps, bool) or not isinstance(lr_decay_steps, int)
                                       or not 1 <= lr_decay_steps < 2 ** 31):
        raise ValueError(f"lr_decay_steps must be null or an integer >= 1 (below 2^31), got {lr_decay_steps!r}")
    if lr_schedule == "constant" and lr_decay_steps is not None:
        raise ValueError(f"lr_decay_steps = {lr_decay_steps!r} needs lr_schedule linear or cosine: a constant schedule decays nothing")
    if lr_schedule != "constant" and lr_decay_steps is None:
        raise ValueError(f"lr_schedule {lr_schedule!r} needs lr_decay_steps (an integer >= 1)")
    if not 0.0 <= number("lr_final_ratio", lr_final_ratio) <= 1.0:
        raise ValueError(f"lr_final_ratio must satisfy 0 <= lr_final_ratio <= 1, got {lr_final_ratio!r}")
    device = lr_schedule != "constant" or lr_warmup_steps > 0
    base = number("lr", lr)
    with np.errstate(over="ignore"):
        base = float(np.float32(base))
    if not 0.0 <= base < float("inf"):
        raise ValueError(f"lr must be a finite number >= 0 that fits fp32, got {lr!r}")
    rates = {}
    for name, v in (("lr_g", lr_g), ("lr_d", lr_d), ("lr_adj", lr_adj)):
        rates[name] = base if v is None else rate(name, v)
        if device and not rates[name] > 0.0:
            raise ValueError(f"lr must be > 0 under a schedule or warm-up ({name} is null and takes lr = {lr!r})")
    return dict(rates, schedule=lr_schedule, kind=LR_SCHEDULE_KINDS[lr_schedule], warmup=int(lr_warmup_steps),
                decay=None if lr_decay_steps is None else int(lr_decay_steps), final_ratio=float(np.float32(lr_final_ratio)), device=device)


def lr_factor(k, settings):
    """s(k) of DESIGN.md §28 as the device computes it (lgsch_step), restated in numpy: fp64 throughout, one conversion to fp32.
    k: training steps taken so far; settings: what lr_schedule_settings returned.  -> numpy.float32.  For the log and the tests."""
    import numpy as np
    f64 = np.float64
    k, W, N = int(k), settings["warmup"], settings["decay"]
    r = f64(np.float32(settings["final_ratio"]))
    up = f64(k + 1) / f64(W) if k < W else f64(1.0)
    d = f64(1.0)
    if settings["schedule"] != "constant":
        t = f64(0.0) if k < W else min(f64(k - W) / f64(N), f64(1.0))
        if settings["schedule"] == "linear":
            d = f64(1.0) - (f64(1.0) - r) * t
        else:
            d = r + (f64(1.0) - r) * f64(0.5) * (f64(1.0) + np.cos(f64(np.pi) * t))
    return np.float32(up * d)


def lr_rates(k, settings):
    """The three rates (G, D, A) of step k: float32(base) * s(k), one fp32 multiply each, as numpy.float32."""
    import numpy as np
    s = lr_factor(k, settings)
    return tuple(np.float32(settings[m]) * s for m in ("lr_g", "lr_d", "lr_adj"))


def grad_guard_settings(clip_norm=None, skip_nonfinite=False):
    """The two keys of the gradient guard, validated: None when both are off (no state exists and no gg_* function is
    fetched), else {clip_norm: the fp32 value it is used at, 0.0 = no clipping; skip: bool}.  Raises ValueError for a clip_norm that is
    neither null nor a finite number > 0 that fits fp32 (bools and strings refused) and for a skip_nonfinite that is no bool."""
    import math
    import numpy as np
    if not isinstance(skip_nonfinite, bool):
        raise ValueError(f"skip_nonfinite must be true or false, got {skip_nonfinite!r}")
    c = 0.0
    if clip_norm is not None:
        if isinstance(clip_norm, bool) or not isinstance(clip_norm, (int, float)) or not math.isfinite(clip_norm):
            raise ValueError(f"clip_norm must be null (off) or a finite number > 0, got {clip_norm!r}")
        with np.errstate(over="ignore"):
            c = float(np.float32(clip_norm))
        if not 0.0 < c < float("inf"):
            raise ValueError(f"clip_norm must be null (off) or a finite number > 0 that fits fp32, got {clip_norm!r}")
    if clip_norm is None and not skip_nonfinite:
        return None
    return {"clip_norm": c, "skip": skip_nonfinite}


def grad_guard_restate(g, gscale, clip_norm, skip, sumsq=None):
    """The record of DESIGN.md §30 as the device computes it (lgg_finalise), restated in numpy: S = the fp64 sum of the squares of g (or
    `sumsq` when given: the device's own S, ops.grad_sumsq — g is then not read), then the fp32 steps of the definition.  clip_norm 0 = no
    clipping.  -> {S (float64), bad, N, c, eff (float32), skip_now (bool)}.  The order of numpy's additions is not the device's: N agrees
    to 1 fp32 ulp, and c, eff follow bit for bit from a given N.  For the log and the tests."""
    import numpy as np
    f32, f64 = np.float32, np.float64
    with np.errstate(over="ignore", invalid="ignore"):
        if sumsq is None:
            g64 = np.asarray(g, dtype=f32).astype(f64).reshape(-1)
            S = f64(np.sum(g64 * g64))
        else:
            S = f64(sumsq)
        bad = not bool(np.isfinite(S))
        gs = f32(gscale)
        N = f32(np.sqrt(S) * f64(gs))
        c = f32(1.0)
        if f32(clip_norm) != 0 and not bad:
            q = f32(clip_norm) / (N + f32(1e-6))
            c = q if q < f32(1.0) else f32(1.0)
        eff = gs * c
    return {"S": S, "bad": bad, "N": N, "c": f32(c), "eff": f32(eff), "skip_now": bool(bad and skip)}


BLUR_MAX_SIGMA, BLUR_MAX_RADIUS, BLUR_MAX_FADE_IMAGES = 10.0, 30, 1 << 40


def blur_settings(blur_init_sigma=0.0, blur_fade_kimg=200):
    """The two keys of the Discriminator-input blur, validated: None when blur_init_sigma is 0 (no state exists and no
    dblur_* function is fetched), else {sigma0: the fp32 value it is used at, fade_images: F = round(blur_fade_kimg * 1000)}.  Raises
    ValueError for a blur_init_sigma that is not a finite number in [0, 10] (bools and strings refused) and for a blur_fade_kimg whose
    image count is not an integer in [1, 2^40]."""
    import math
    import numpy as np
    s0 = blur_init_sigma
    if isinstance(s0, bool) or not isinstance(s0, (int, float)) or not math.isfinite(s0) or not 0.0 <= s0 <= BLUR_MAX_SIGMA:
        raise ValueError(f"blur_init_sigma must be a finite number in [0, {BLUR_MAX_SIGMA:g}] (0 = off), got {s0!r}")
    kimg = blur_fade_kimg
    if isinstance(kimg, bool) or not isinstance(kimg, (int, float)) or not math.isfinite(kimg):
        raise ValueError(f"blur_fade_kimg must be a number of thousand images, got {kimg!r}")
    F = int(round(kimg * 1000))
    if not 1 <= F <= BLUR_MAX_FADE_IMAGES:
        raise ValueError(f"blur_fade_kimg: {kimg!r} thousand images is {F} images, outside [1, 2^40]")
    s0 = float(np.float32(s0))
    if s0 == 0.0:
        return None
    return {"sigma0": s0, "fade_images": F}


def blur_radius(sigma):
    """R of DESIGN.md §31 as lgblur_apply derives it from the fp32 sigma: min((int)floorf(3.0f * sigma), 30), 0 for a sigma that is not
    finite or not > 0."""
    import numpy as np
    sigma = np.float32(sigma)
    if not (np.isfinite(sigma) and sigma > 0):
        return 0
    with np.errstate(over="ignore"):
        t = np.float32(3.0) * sigma
    return BLUR_MAX_RADIUS if t >= np.float32(BLUR_MAX_RADIUS) else int(np.floor(t))


def blur_taps(sigma):
    """(R, w fp32 [R + 1]) of DESIGN.md §31 for an fp32 sigma: t_i = exp2(-(i / sigma)^2) in fp64, Z = t_0 + 2 sum t_i in ascending i,
    w_i = fp32(t_i / Z).  R == 0 gives the one tap 1."""
    import numpy as np
    R = blur_radius(sigma)
    if R == 0:
        return 0, np.ones(1, np.float32)
    t = np.exp2(-(np.arange(R + 1, dtype=np.float64) / np.float64(np.float32(sigma))) ** 2)
    rest = np.float64(0.0)
    for v in t[1:]:
        rest = rest + v
    return R, (t / (t[0] + np.float64(2.0) * rest)).astype(np.float32)


def blur_restate(k, n, settings):
    """(sigma fp32, R, taps fp32 [R + 1]) of step k as the device computes them (lgblur_step, lgblur_apply), restated in numpy: k training
    steps taken before this one, n real images D reads per step over all ranks, settings what blur_settings returned.  sigma is fp64
    basic operations and one conversion, so it agrees bit for bit.  For the host mirror, the log and the tests."""
    import numpy as np
    f64 = np.float64
    left = f64(1.0) - f64(max(int(k), 0) * int(n)) / f64(settings["fade_images"])
    sigma = np.float32(f64(np.float32(settings["sigma0"])) * (left if left > 0 else f64(0.0)))
    R, w = blur_taps(sigma)
    return sigma, R, w


METRIC_NAMES = ("fid", "kid", "prdc")


def metric_list(metrics):
    """The evaluate_metrics key (a list of names, or a comma list in one string, as the CLI gives it) as a list without repeats.
    Raises ValueError for an empty selection or a name outside fid, kid, prdc."""
    if isinstance(metrics, str):
        metrics = [n.strip() for n in metrics.split(",") if n.strip()]
    if not isinstance(metrics, (list, tuple)) or not metrics:
        raise ValueError(f"evaluate_metrics must be a non-empty list out of {', '.join(METRIC_NAMES)}, got {metrics!r}")
    for name in metrics:
        if name not in METRIC_NAMES:
            raise ValueError(f"evaluate_metrics: unknown metric {name!r} in {metrics!r} (a list out of {', '.join(METRIC_NAMES)})")
    return list(dict.fromkeys(metrics))


MODES = ["train", "pack", "plot", "visual", "random-sample", "evaluate", "condition-sample", "evaluate-sample", "export-model"]


class Arg:
    def __init__(self, argv=None, config_dir="."):
        print(" - Initializing Application...")
        parser = ArgumentParser(prog="LittleGAN", description="The code for paper: LittleGAN")
        parser.add_argument("mode", type=str, help="run mode", default="train", choices=MODES)
        parser.add_argument("exp_name", type=str, help="experience name")
        parser.add_argument("-e", "--env", type=str, help="config environment", default="sample")
        parser.add_argument("-g", "--gpu", type=str, required=False, help="gpu ids, eg: 0,1,2,3", default="-1")
        parser.add_argument("--debug", help="use debug mode, ignore git repo is dirty", action="store_true")
        args = parser.parse_args(argv)
        for k, v in DEFAULTS.items():
            setattr(self, k, v)
        self.env_file = args.env + ".config.json"
        for name in dict.fromkeys(["sample.config.json", self.env_file]):  # defaults < sample < env (config.py:19-29)
            fp = os.path.join(config_dir, name)
            if os.path.exists(fp):
                with open(fp) as f:
                    for k, v in json.load(f).items():
                        setattr(self, k, v)
            elif name != "sample.config.json":
                raise FileNotFoundError(fp)
        for k, v in vars(args).items():
            setattr(self, k, v)
        diff_augment_bits(self.diff_augment)   # a misspelt component fails here, not at the first training step
        geom_augment_bits(self.geom_augment)
        ada_settings(self.diff_augment, self.diff_augment_p, self.ada_target, self.ada_interval, self.ada_kimg, self.geom_augment)
        r1_settings(self.r1_gamma, self.r1_interval)
        gan_loss_kind(self.gan_loss, bool(self.use_gp))   # a misspelt objective fails here, and so does wgan without its penalty
        relativistic_setting(self.relativistic, self.gan_loss)
        r2_settings(self.r2_gamma, self.r1_interval)
        lr_schedule_settings(self.lr, self.lr_g, self.lr_d, self.lr_adj, self.lr_schedule, self.lr_warmup_steps, self.lr_decay_steps,
                             self.lr_final_ratio)   # a misspelt schedule fails here, not at the first step
        grad_guard_settings(self.clip_norm, self.skip_nonfinite)
        blur_settings(self.blur_init_sigma, self.blur_fade_kimg)
        self.evaluate_metrics = metric_list(self.evaluate_metrics)   # a misspelt metric fails here, not after the sampling run
        if int(self.kid_subsets) < 0 or int(self.kid_subset_size) < 2 or not 1 <= int(self.prdc_k) <= 15:
            raise ValueError("need kid_subsets >= 0, kid_subset_size >= 2 and 1 <= prdc_k <= 15")
        self.cond_dim = len(self.attr)
        self.result_dir = os.path.join(self.all_result_dir, args.exp_name)
        # the reference sets CUDA_VISIBLE_DEVICES (config.py:35); with one process per GPU the launcher
        # (torchrun) owns device selection, so only the parsed list is kept.
        self.gpu = [int(item) for item in self.gpu.split(",") if item.isnumeric() and int(item) >= 0]
        self.prefetch = self.prefetch_batch * self.batch_size

    def __str__(self):
        return self.__dict__.__str__()
