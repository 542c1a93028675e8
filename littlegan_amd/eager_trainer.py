"""EagerTrainer — host-side mirror of /root/reference/eager_trainer.py on the HIP kernels.

The hot path is `train_step_from_inputs` = the arithmetic of eager_trainer.py:133-168 (the two
GradientTapes replaced by a static backward plan), called by `_train_step` (eager_trainer.py:115-169)
after it has drawn the two batches, the noise and the augmented image.  Data parallelism (new,
BASELINE.json north star): one process per GPU, the three gradient sets are contiguous ranges of one
flat buffer and are all-reduced (RCCL) on a side stream while the next tape's backward runs.
"""
from __future__ import annotations

import contextlib
import json
import os
import time
from typing import Dict, Optional

import torch

from . import ops
from .config import (ada_settings, blur_restate, blur_settings, diff_augment_bits, gan_loss_kind, geom_augment_bits, grad_guard_settings, lr_schedule_settings,
                     r1_settings, r2_settings, relativistic_setting)
from .dist import GradSync
from .model import Adjuster, Discriminator, Generator, ParamStore
from .utils import save_image, soft

ADAM_EPS = 1e-8


def _dist_rank_world():
    d = torch.distributed
    if d.is_available() and d.is_initialized():
        return d.get_rank(), d.get_world_size()
    return 0, 1


def _barrier():
    d = torch.distributed
    if d.is_available() and d.is_initialized() and d.get_world_size() > 1:
        d.barrier()


def train_weight_range(args, model: str, batch_no: int):
    """eager_trainer.py:104-113 + part_groups :48-52 as (lo, hi) weight-index ranges."""
    groups = {"G": [(0, 4), (4, 8), (8, 22)], "D": [(0, 12), (12, 16), (16, 20)], "A": [(0, 4)]}[model]
    n_all = {"G": 22, "D": 20, "A": 4}[model]
    if args.use_partition and batch_no % (args.partition_interval + 1) == 0:
        return groups[(batch_no // (args.partition_interval + 1)) % len(groups)]
    return (0, n_all)


def validate_ema_decay(decay) -> float:
    """ema_decay of the configuration: 0 (off) or a decay in (0, 1)."""
    d = float(decay)
    if not 0.0 <= d < 1.0:
        raise ValueError(f"ema_decay must satisfy 0 <= ema_decay < 1 (0 = off), got {decay}")
    return d


class EagerTrainer:
    def __init__(self, args, generator: Generator, discriminator: Discriminator, adjuster: Adjuster, dataset):
        self.args = args
        print(" - Initializing Trainer(Executor)...")
        self.dataset = dataset
        self.adjuster = adjuster
        self.discriminator = discriminator
        self.generator = generator
        self.models = [self.discriminator, self.generator, self.adjuster]
        self.device = generator.device
        # gradient penalty on the disc tape (the reference raises here, eager_trainer.py:141-143; definition: DESIGN.md §12)
        self.use_gp = bool(getattr(args, "use_gp", False))
        # live encoder dropout (the reference's dropout is the identity, model.py:25): on when dropout_train is set
        # and 0 < dropout_rate < 1.  dropout_rate == 0 under dropout_train keeps the whole plumbing (key, call slots, the dropped
        # kernels) with masks that keep everything: bit-identical to the feature off (tests/test_dropout_gpu.py)
        self.dropout_rate = float(getattr(args, "dropout_rate", 0.0))
        self.dropout = bool(getattr(args, "dropout_train", False))
        if self.dropout and not 0.0 <= self.dropout_rate < 1.0:
            raise ValueError(f"dropout_train needs 0 <= dropout_rate < 1, got {self.dropout_rate}")
        if self.dropout and self.use_gp:
            raise ValueError("use_gp and dropout_train exclude each other: the penalty's double backward through a masked norm "
                             "is not built (DESIGN.md §15)")
        # differentiable augmentation of D's inputs (the reference has none): on when diff_augment names a component
        self.diffaug = diff_augment_bits(getattr(args, "diff_augment", ""))
        if self.diffaug and self.use_gp:
            raise ValueError("diff_augment and use_gp exclude each other: the penalty's double backward through the augmentation T "
                             "is not built (DESIGN.md §18)")
        if self.diffaug and self.dropout:
            raise ValueError("diff_augment and dropout_train exclude each other: under diff_augment the Adjuster encodes `fake` itself "
                             "and the masks of the rows D used to hand over are not built for that pass (DESIGN.md §18)")
        if self.diffaug and int(getattr(args, "image_channel", 3)) != 3:
            raise ValueError("diff_augment needs 3-channel images")
        # adaptive augmentation probability (the reference has none): None = every named component on every row, the
        # plain diff_augment step with no state and no launch of its own; else the gated draw, with the controller when a target is set
        # geometric augmentation of D's inputs (the reference has none): on when geom_augment names a component.  D then
        # reads T(Geo(image)); the step is "augmenting" (self.augmenting) when either key is on
        self.geom = geom_augment_bits(getattr(args, "geom_augment", ""))
        if self.geom and self.use_gp:
            raise ValueError("geom_augment and use_gp exclude each other: the penalty's double backward through the resampling "
                             "is not built (DESIGN.md §26)")
        if self.geom and self.dropout:
            raise ValueError("geom_augment and dropout_train exclude each other: under geom_augment the Adjuster encodes `fake` itself "
                             "and the masks of the rows D used to hand over are not built for that pass (DESIGN.md §26)")
        if self.geom and int(getattr(args, "image_channel", 3)) != 3:
            raise ValueError("geom_augment needs 3-channel images")
        self.augmenting = bool(self.diffaug or self.geom)
        self.ada = ada_settings(getattr(args, "diff_augment", ""), getattr(args, "diff_augment_p", None), getattr(args, "ada_target", None),
                                getattr(args, "ada_interval", 4), getattr(args, "ada_kimg", 500.0), getattr(args, "geom_augment", ""))
        # R1 penalty on D's real-image logit, applied every r1_interval-th step (the reference has none): None = off
        self.r1 = r1_settings(getattr(args, "r1_gamma", 0.0), getattr(args, "r1_interval", 16))
        if self.r1 is not None and self.use_gp:
            raise ValueError("r1_gamma and use_gp exclude each other: two gradient penalties on one disc tape (DESIGN.md §24)")
        if self.r1 is not None and self.dropout:
            raise ValueError("r1_gamma and dropout_train exclude each other: the penalty's double backward through a masked norm "
                             "is not built (DESIGN.md §24)")
        # objective of the real / fake terms (the reference's is "bce"): read once.  0 = "bce", the step as it always was,
        # none of the logit-side code runs; else the `kind` of ops.gan_heads_loss, and use_gp penalises the logit
        self.gan_loss = getattr(args, "gan_loss", "bce")
        self.gan_kind = gan_loss_kind(self.gan_loss, self.use_gp)
        # relativistic pairing of the real / fake terms (the reference has none): f0(z_r - z_f) per pair of rows, through
        # ops.pair_heads_loss where ops.gan_heads_loss stands otherwise; refused for "bce" (no logit) and "wgan" (its pairing is itself)
        self.relativistic = relativistic_setting(getattr(args, "relativistic", False), self.gan_loss)
        # R2 penalty: R1's term on the fake rows D read, on R1's schedule (the reference has none): None = off
        self.r2 = r2_settings(getattr(args, "r2_gamma", 0.0), getattr(args, "r1_interval", 16))
        # with both penalties on: one joint 2B-row pass (the product path), or two B-row passes.  No configuration key: an attribute
        # that scripts/bench_rel.py clears on one of its trainers to time the alternative
        self.r12_joint = True
        if self.r2 is not None and self.use_gp:
            raise ValueError("r2_gamma and use_gp exclude each other: two gradient penalties on one disc tape (DESIGN.md §27)")
        if self.r2 is not None and self.dropout:
            raise ValueError("r2_gamma and dropout_train exclude each other: the penalty's double backward through a masked norm "
                             "is not built (DESIGN.md §27)")
        # weight average for sampling (the reference has none): on when ema_decay > 0
        self.ema_decay = validate_ema_decay(getattr(args, "ema_decay", 0.0))
        self.sample_ema = bool(getattr(args, "sample_ema", True))
        self._ema_live = False   # inside ema_weights(): `flat` holds the average
        self.store = ParamStore(generator, discriminator, adjuster)
        if self.ema_decay > 0.0:
            self.store.enable_ema()
        # tf.compat.v1.train.AdamOptimizer x3 (eager_trainer.py:28-30): {beta1_power, beta2_power} per optimizer
        # learning rates per network and their schedule (the reference has one constant lr): the base rates go where lr
        # went; lr_sched["device"] false = they are the launch scalars of the Adam passes, nothing else changes
        self.lr_sched = lr_schedule_settings(args.lr, *(getattr(args, k, d) for k, d in (
            ("lr_g", None), ("lr_d", None), ("lr_adj", None), ("lr_schedule", "constant"), ("lr_warmup_steps", 0), ("lr_decay_steps", None),
            ("lr_final_ratio", 0.0))))
        self.opt_cfg = {"G": (self.lr_sched["lr_g"], args.beta_1, args.beta_2), "D": (self.lr_sched["lr_d"], args.beta_1, args.beta_2),
                        "A": (self.lr_sched["lr_adj"], 0.9, 0.999)}
        self.opt_state = {m: torch.tensor([b1, b2], dtype=torch.float32, device=self.device)
                          for m, (_, b1, b2) in self.opt_cfg.items()}
        self.losses = {k: torch.zeros(1, dtype=torch.float32, device=self.device)
                       for k in ("gen", "disc", "adj") + (("gp",) if self.use_gp else ()) + (("r1",) if self.r1 is not None else ())
                       + (("r2",) if self.r2 is not None else ())}
        self.sync = GradSync(self.device)
        self.adam_order = ("D", "G", "A")   # = the launch order of the all-reduces (see train_step_from_inputs)
        self.global_epoch = 1
        self._input_step = 0  # counter window of the device-side step inputs (draw_step_inputs); part of the checkpoint
        self.rank, self.world = _dist_rank_world()
        if self.ada is not None:
            # {p, sum of signs, rows, steps} on the device (lgx_ada_init: written from a launch scalar); _ada_steps mirrors its last
            # word on the host, which only needs it to place the data-parallel all-reduce of the counters (_ada_control)
            self.ada_state = ops.ada_init(self.ada["p0"], device=self.device)
            self._ada_steps, self._ada_due, self._ada_ticked = 0, False, False
        # {k, s, rate of G, D, A, 0, 0, 0} on the device (lgsch_init: written from a launch scalar), advanced by the first launch of every
        # step; None = the rates are constants.  No host mirror: nothing on the host depends on k
        self.lr_state = ops.sched_init(0, device=self.device) if self.lr_sched["device"] else None
        # global-norm clipping and the non-finite step guard (the reference has neither): None = off, no state and no
        # launch of its own; else three 32-byte records {N, eff, skip_now, skipped, nonfinite, c, 0, 0} on the device (G, D, A; lgg_init:
        # written from launch scalars), one partials workspace sized for the largest network, and, without a schedule, the three base
        # rates on the device (filled once, here: the guarded Adam passes always read their rate through a pointer)
        self.guard = grad_guard_settings(getattr(args, "clip_norm", None), getattr(args, "skip_nonfinite", False))
        if self.guard is not None:
            self.guard_state = torch.empty(24, dtype=torch.float32, device=self.device)
            self._guard_rec = {m: self.guard_state[8 * i:8 * i + 8] for i, m in enumerate("GDA")}
            for m in "GDA":
                ops.guard_init(0, 0, out=self._guard_rec[m])
            n_max = max(e - s for s, e in (self.store.model_range(m) for m in "GDA"))
            self._guard_ws = torch.empty(ops.guard_workspace_bytes(n_max), dtype=torch.uint8, device=self.device)
            self._guard_lr = None
            if self.lr_state is None:
                self._guard_lr = torch.tensor([self.opt_cfg[m][0] for m in "GDA"], dtype=torch.float32, device=self.device)
        # blur of D's inputs (the reference has none): None = off, no state and no launch of its own; else {k, sigma, 0, 0}
        # on the device (lgblur_init: written from a launch scalar), advanced by lgblur_step on every step whose restated radius is >= 1.
        # _blur_k mirrors k on the host (every rank walks the same counter: no collective): it decides, before anything is enqueued,
        # whether a step blurs at all.  sigma never rises, so once the radius is 0 the step is the one without the key
        self.blur = blur_settings(getattr(args, "blur_init_sigma", 0.0), getattr(args, "blur_fade_kimg", 200))
        if self.blur is not None:
            if self.use_gp:
                raise ValueError("blur_init_sigma and use_gp exclude each other: the penalty's double backward through the blur is not "
                                 "built (DESIGN.md §31)")
            if self.dropout:
                raise ValueError("blur_init_sigma and dropout_train exclude each other: under the blur the Adjuster encodes `fake` itself "
                                 "and the masks of the rows D used to hand over are not built for that pass (DESIGN.md §31)")
            if int(getattr(args, "image_channel", 3)) != 3:
                raise ValueError("blur_init_sigma needs 3-channel images")
            self.blur_state = ops.blur_init(0, device=self.device)
            self._blur_k, self._blur_k_step, self._blur_ticked = 0, 0, False
        self._init_dir()
        # eager_trainer.py:36-43: restore the newest checkpoint (weights, the three optimizers' slots and beta powers)
        # and the epoch from status.json when args.restore is set
        if getattr(args, "restore", False) and not getattr(args, "no_io", False) and getattr(args, "result_dir", None):
            latest = self.latest_checkpoint()
            if latest is not None:
                print("Loading Checkpoint...")
                self.load_checkpoint(latest)
                st = os.path.join(args.result_dir, "checkpoint", "status.json")
                if os.path.isfile(st):
                    with open(st) as f:
                        self.global_epoch = json.load(f)["epoch"]
        self._init_test_data()

    # ------------------------------------------------------------------ hot path
    def train_step_from_inputs(self, batch_no: int, inp: Dict[str, torch.Tensor]):
        """inp: real_image_1, real_cond_1, real_image_2, real_cond_2, noise, new_image (device fp32, NHWC); with use_gp also
        gp_eps [B] (the penalty's interpolation weights, U[0,1)); with dropout_train also dropout_key (int64 [2] = {seed, key_offset} of
        the step's mask stream, draw_dropout_key); with diff_augment or geom_augment also diffaug_key (the same kind of pair, draw_diffaug_key:
        both read it, on Philox blocks of their own; the blur of blur_init_sigma draws nothing and needs no key).
        Returns (fake_image, adj_image|None, gen_loss, disc_loss, adj_loss|None) — losses are 1-element device tensors
        (no host sync on the hot path)."""
        a = self.args
        if self._ema_live:
            raise RuntimeError("train_step_from_inputs inside ema_weights(): the store holds the averaged weights")
        G, D, A = self.generator, self.discriminator, self.adjuster
        img1, c1, img2, c2 = inp["real_image_1"], inp["real_cond_1"], inp["real_image_2"], inp["real_cond_2"]
        noise, new_image = inp["noise"], inp["new_image"]
        B = img1.shape[0]
        c = a.cond_dim
        gp_eps = inp.get("gp_eps") if self.use_gp else None
        if self.use_gp and gp_eps is None:
            raise ValueError("train_step_from_inputs: use_gp is on and inp has no 'gp_eps' ([B] fp32 device tensor, U[0,1))")
        # dropout call slots of the step's encoder passes: 0 = D on [new_image ; fake], 1 = the Adjuster's own pass on img1,
        # 2 = D on the Adjuster's output.  The key is a device tensor: a captured graph replays with the masks of its step.
        drop = [None, None, None]
        if self.dropout:
            if inp.get("dropout_key") is None:
                raise ValueError("train_step_from_inputs: dropout_train is on and inp has no 'dropout_key' (int64 [2] device tensor "
                                 "{seed, key_offset}: draw_dropout_key)")
            drop = [ops.Drop(inp["dropout_key"], call, rate=self.dropout_rate) for call in range(3)]

        # differentiable augmentation call slots: 0 = D on [new_image ; fake], 1 = D on the Adjuster's output.  D reads
        # T(image); `fake` itself (the L1 term, the Adjuster's input, the returned image) stays un-augmented.
        aug_key, S = None, img1.shape[1]
        # blur of D's inputs: D reads T(Geo(Blur(image))).  Live while the restated radius of this step is >= 1; a step
        # with live blur is an augmenting step (the Adjuster encodes `fake` itself), a faded one enqueues nothing of the blur's
        blur = None
        if self.blur is not None:
            if not self._blur_ticked:   # (graph_step has counted this step already, whichever way it runs it)
                self._blur_tick()
            if self.blur_live(self._blur_k_step):
                blur = self.blur_state
        augmenting = self.augmenting or blur is not None
        if self.augmenting:
            aug_key = inp.get("diffaug_key")
            if aug_key is None:
                raise ValueError(f"train_step_from_inputs: {'diff_augment' if self.diffaug else 'geom_augment'} is on and inp has no "
                                 "'diffaug_key' (int64 [2] device tensor {seed, key_offset}: draw_diffaug_key)")

        # ---- forward: fake = G(noise, c2); D on the [new_image ; fake] batch (eager_trainer.py:134-137)
        ctx_g: dict = {}
        # D's input batch [new_image ; fake].  A caller that owns the step inputs hands the 2B-image buffer over as
        # inp["disc_input"] with new_image ALREADY in its first half (`_train_step` lets the augmentation kernel write there,
        # bench.py generates its synthetic new_image there): G writes `fake` into the second half and nothing is copied.
        d_in = inp.get("disc_input")
        if d_in is None:
            d_in = torch.empty((2 * B,) + tuple(img1.shape[1:]), dtype=torch.float32, device=self.device)
            d_in[:B].copy_(new_image)
        elif not (tuple(d_in.shape) == (2 * B,) + tuple(img1.shape[1:]) and d_in.dtype == torch.float32 and d_in.is_contiguous()
                  and d_in.device == new_image.device and d_in.data_ptr() == new_image.data_ptr()
                  and tuple(new_image.shape) == tuple(img1.shape) and new_image.is_contiguous()):
            raise ValueError("train_step_from_inputs: inp['disc_input'] must be a contiguous fp32 [2B, H, W, C] buffer whose first B "
                             "images ARE inp['new_image'] (a view of it)")
        if self.lr_state is not None:   # the step's first launch: s(k) and the three rates of this step, then k += 1
            ls = self.lr_sched
            ops.sched_step(self.lr_state, ls["kind"], ls["warmup"], ls["decay"], ls["final_ratio"], *(self.opt_cfg[m][0] for m in "GDA"))
        if blur is not None:   # the first of the blur's launches: sigma(k) of this step, then k += 1
            ops.blur_step(blur, self.blur["sigma0"], self._blur_images_per_step(), self.blur["fade_images"])
        fake = G([noise, c2], ctx_g, out=d_in[B:])
        ctx_d: dict = {}
        run_adj = bool(a.train_adj and batch_no > 10)
        adaptive = self.ada is not None and self.ada["target"] is not None
        if adaptive and not self._ada_ticked:   # (graph_step has counted this step already, whichever way it runs it)
            self._ada_tick()
        # the Adjuster reuses D's encoder maps of `fake` as its skip inputs: keep the fp32 maps only then
        x_real = new_image   # what D reads as its real batch: the R1 penalty's input on a penalty step
        x_all = d_in         # ... and the whole batch D reads, [real ; fake]: the fake half is the R2 penalty's input
        kind = self.gan_kind
        lk = dict(logits=True) if kind else {}   # a logit-side objective: the heads keep z_pr (same launches, another finaliser)
        par0 = geo0 = par1 = geo1 = None
        if augmenting:
            if self.augmenting:
                par0, geo0 = self._augment_draw(aug_key, 0, 2 * B, S)
            d_aug = self._augment_fwd(d_in, par0, geo0, blur)   # T(Geo(Blur(d_in))), each present only when its key is on / live
            x_real, x_all = d_aug[:B], d_aug
            p = D.forward_packed(d_aug, ctx_d, keep_maps=False, **lk)   # the maps are those of T(fake): not handed over
            if adaptive and not run_adj:   # after the step's last draw: step n + 1 is the first to see a new p
                self._ada_control(p, B)
        else:
            p = D.forward_packed(d_in, ctx_d, keep_maps=run_adj, drop=drop[0], **lk)  # [2B, 1+c]: rows [0,B) real, [B,2B) fake

        # ---- disc tape (eager_trainer.py:139,145): 2*BCE(c1,real_c) + BCE(.98,real_pr) + BCE(.02,fake_pr)
        dz = torch.empty(2 * B, 1 + c, dtype=torch.float32, device=self.device)
        # (a logit-side gan_loss, DESIGN.md §25: the two BCE(., _pr) become f(z) of the D-real / D-fake rows, no smoothing; the same launches)
        rel = self.relativistic
        if rel:
            # (relativistic pairing, DESIGN.md §27: ONE term f0(z_r - z_f) per pair, written by the real rows' call; the fake rows' call
            # adds its gradient with respect to z_f alone.  The same launches, one for one)
            z = ctx_d["z_pr"]
            ops.pair_heads_loss(p[:B], z[:B], z[B:], c1, kind, ops.REL_SIDE_SELF, 1.0, 2.0, self.losses["disc"], dz[:B], False)
            ops.pair_heads_loss(p[B:], z[B:], z[:B], None, kind, ops.REL_SIDE_OTHER, 1.0, 0.0, self.losses["disc"], dz[B:], True)
        elif kind:
            z = ctx_d["z_pr"]
            ops.gan_heads_loss(p[:B], z[:B], c1, kind, ops.GAN_ROLE_D_REAL, 1.0, 2.0, self.losses["disc"], dz[:B], False)
            ops.gan_heads_loss(p[B:], z[B:], None, kind, ops.GAN_ROLE_D_FAKE, 1.0, 0.0, self.losses["disc"], dz[B:], True)
        else:
            ops.bce_heads_loss(p[:B], c1, soft(1.0), 1.0, 2.0, self.losses["disc"], dz[:B], False)
            ops.bce_heads_loss(p[B:], None, soft(0.0), 1.0, 0.0, self.losses["disc"], dz[B:], True)
        # a partition step differentiates one weight group only (eager_trainer.py:104-113,145): untrained groups get no
        # weight-gradient kernels, no all-reduce, and the backward chain stops where nothing below is asked for
        rng_d = train_weight_range(a, "D", batch_no)
        D.backward(ctx_d, dz, need_wgrad=True, need_input_grad=False, train_range=rng_d)
        if self.use_gp:
            # disc_loss += gp_weight * mean_b (|d output_pr(x^_b) / d x^_b| - 1)^2 on x^ = eps new_image + (1 - eps) fake; its weight
            # gradients are added to the disc tape's before the all-reduce
            # (under a logit-side gan_loss the penalised quantity is the logit: DESIGN.md §25)
            D.gradient_penalty(ops.gp_interp(new_image, fake, gp_eps), a.gp_weight, self.losses["disc"], self.losses["gp"],
                               train_range=rng_d, **(dict(logit=True) if kind else {}))
        if self.r1_step(batch_no):
            # disc_loss += (r1_gamma r1_interval / 2) mean_b |d logit(x_b) / d x_b|^2 over the real rows D read (under diff_augment the
            # augmented rows, kept from above: no new draw); its weight gradients are added to the disc tape's before the all-reduce
            if self.r2 is None:
                D.r1_penalty(x_real, self.r1["weight"], self.losses["disc"], self.losses["r1"], train_range=rng_d)
            elif self.r12_joint:   # R1 + R2: one pass over the 2B rows D read, a weight per half
                D.r12_penalty(x_all, self.r1["weight"], self.r2["weight"], self.losses["disc"], self.losses["r1"], self.losses["r2"],
                              train_range=rng_d)
            else:   # the same as two B-row passes: what scripts/bench_rel.py measures the joint pass against
                D.r1_penalty(x_real, self.r1["weight"], self.losses["disc"], self.losses["r1"], train_range=rng_d)
                D.r1_penalty(x_all[B:], self.r2["weight"], self.losses["disc"], self.losses["r2"], train_range=rng_d)
        elif self.r2_step(batch_no):
            # R2 alone: R1's pass on the fake rows D read, a constant on this tape
            D.r1_penalty(x_all[B:], self.r2["weight"], self.losses["disc"], self.losses["r2"], train_range=rng_d)
        self.sync.launch("D", self.store, *self.store.model_range("D", *rng_d))

        # ---- gen tape (eager_trainer.py:140,149): BCE(.98,fake_pr) + BCE(c2,fake_c) + l1*mean|img2-fake|
        dz_g = torch.empty(B, 1 + c, dtype=torch.float32, device=self.device)
        if rel:   # f0(z_f - z_r), differentiated with respect to z_f alone: z_r is a constant of this tape
            ops.pair_heads_loss(p[B:], ctx_d["z_pr"][B:], ctx_d["z_pr"][:B], c2, kind, ops.REL_SIDE_SELF, 1.0, 1.0, self.losses["gen"],
                                dz_g, False)
        elif kind:
            ops.gan_heads_loss(p[B:], ctx_d["z_pr"][B:], c2, kind, ops.GAN_ROLE_G, 1.0, 1.0, self.losses["gen"], dz_g, False)
        else:
            ops.bce_heads_loss(p[B:], c2, soft(1.0), 1.0, 1.0, self.losses["gen"], dz_g, False)
        g_img = D.backward(ctx_d, dz_g, need_wgrad=False, need_input_grad=True, rows=slice(B, 2 * B))
        if augmenting:   # the gen tape is differentiated through the augmentation, Blur(Geo^T(T^T g)): rows B..2B of slot 0
            g_img = self._augment_bwd(g_img, None if par0 is None else par0[B:], None if geo0 is None else geo0[B:], blur)
        dpre = torch.empty_like(g_img)
        ops.l1_tanh_loss(img2, fake, g_img, dpre, self.losses["gen"], a.l1_lambda, True)
        rng_g = train_weight_range(a, "G", batch_no)
        G.backward(ctx_g, dpre, train_range=rng_g)
        self.sync.launch("G", self.store, *self.store.model_range("G", *rng_g))

        # ---- adjuster branch (eager_trainer.py:152-164)
        adj_image = None
        if run_adj:
            adj_t_cond, adj_in_cond = ops.adj_conditions(c2, c1)   # concat([c2, c1], 0) and (that + 1) * 0.5, one launch
            ctx_a: dict = {}
            # encoder(fake) was computed by D above with the same weights: hand its 4 maps to the Adjuster.  Under diff_augment D
            # encoded T(fake), so `fake` is encoded here, by one more B-row pass whose maps take the same place
            if augmenting:
                tails = A.encoder(fake)
            else:
                tails = [m[B:] for m in ctx_d["enc_maps"]]  # fp32 maps (f32 path) / bf16 mirrors + the fp32 top map (bf16 path)
            # Adjuster input = [img1 ; fake]: with the encoder maps of `fake` handed over, only img1 is encoded here (dropout: the
            # handed-over maps keep the masks call 0 drew for them — no tape differentiates through the skips)
            adj_image = A([img1, adj_in_cond], ctx_a, enc_tails=tails, drop=drop[1])
            ctx_d2: dict = {}
            if augmenting:
                if self.augmenting:
                    par1, geo1 = self._augment_draw(aug_key, 1, 2 * B, S)
                if adaptive:   # both draws of the step have read p: the real rows of slot 0 feed the controller
                    self._ada_control(p, B)
                p_a = D.forward_packed(self._augment_fwd(adj_image, par1, geo1, blur), ctx_d2, keep_maps=False, top_only=True, **lk)
            else:
                p_a = D.forward_packed(adj_image, ctx_d2, keep_maps=False, top_only=True, drop=drop[2], **lk)
            dz_a = torch.empty(2 * B, 1 + c, dtype=torch.float32, device=self.device)
            if rel:   # f0(z_a[i] - z_r[i mod B]) over the Adjuster's 2B rows against the real logits of slot 0
                ops.pair_heads_loss(p_a, ctx_d2["z_pr"], ctx_d["z_pr"][:B], adj_t_cond, kind, ops.REL_SIDE_SELF, 1.0, 1.0,
                                    self.losses["adj"], dz_a, False)
            elif kind:
                ops.gan_heads_loss(p_a, ctx_d2["z_pr"], adj_t_cond, kind, ops.GAN_ROLE_G, 1.0, 1.0, self.losses["adj"], dz_a, False)
            else:
                ops.bce_heads_loss(p_a, adj_t_cond, soft(1.0), 1.0, 1.0, self.losses["adj"], dz_a, False)
            g_adj = D.backward(ctx_d2, dz_a, need_wgrad=False, need_input_grad=True)
            if augmenting:
                g_adj = self._augment_bwd(g_adj, par1, geo1, blur)
            dpre_a = torch.empty_like(g_adj)
            # target = [img2 ; img1]: one call per half instead of a 2B-image concatenation (lambda / 2 over half the elements is
            # the same scale, exactly: the element count is a multiple of a power of two)
            ops.l1_tanh_loss(img2, adj_image[:B], g_adj[:B], dpre_a[:B], self.losses["adj"], 0.5 * a.l1_lambda, True)
            ops.l1_tanh_loss(img1, adj_image[B:], g_adj[B:], dpre_a[B:], self.losses["adj"], 0.5 * a.l1_lambda, True)
            A.backward_own(ctx_a, dpre_a)
            self.sync.launch("A", self.store, *self.store.model_range("A"))

        # ---- optimizer applies.  The reference applies A, D, G (eager_trainer.py:164-168); the three weight ranges, Adam
        # slots and beta-power pairs are disjoint, so any order gives the same bits (tests/test_step_gpu.py::
        # test_adam_order_is_immaterial, tests/test_dp_cpu.py).  Here: the order the all-reduces were launched in, each set
        # waited for on its own right before its Adam — D and G are applied while A's all-reduce (launched last) is on the
        # wire.  D-grads are clipped after the all-reduce, inside the Adam kernel.
        self._apply_optimizers(batch_no, run_adj)
        self.sync.wait_all()
        self.store.bump()
        return (fake, adj_image, self.losses["gen"], self.losses["disc"], self.losses["adj"] if run_adj else None)

    # ------------------------------------------------------------------ adaptive augmentation probability
    def _diffaug_draw(self, key, call, rows, S):
        """The records of a call slot: every named component on every row, or (gated path) each with the probability in ada_state"""
        if self.ada is None:
            return ops.diffaug_draw(key, call, 0, rows, S, self.diffaug)
        return ops.diffaug_draw_gated(key, call, 0, rows, S, self.diffaug, self.ada_state)

    def _augment_draw(self, key, call, rows, S):
        """The records of call slot `call`: (diff_augment's | None, the geometric ones | None), each under the present p on the gated path"""
        par = self._diffaug_draw(key, call, rows, S) if self.diffaug else None
        geo = ops.geom_draw(key, call, 0, rows, S, self.geom, None if self.ada is None else self.ada_state) if self.geom else None
        return par, geo

    def _augment_fwd(self, images, par, geo, blur=None):
        """What D reads of `images`: T(Geo(Blur(images))), Geo alone when diff_augment is off, T alone when
        geom_augment is — then exactly the launches of the diff_augment step; Blur (blur: its state) only while the blur is live"""
        if blur is not None:
            images = ops.blur_apply(images, blur)
        if geo is not None:
            images = ops.geom_fwd(images, geo)
        if par is not None:
            images = ops.diffaug_fwd(images, par)
        return images

    def _augment_bwd(self, g, par, geo, blur=None):
        """The adjoint of _augment_fwd on an image gradient: Blur(Geo^T(T^T g)) — the blur is its own adjoint"""
        if par is not None:
            g = ops.diffaug_bwd(g, par)
        if geo is not None:
            g = ops.geom_bwd(g, geo)
        if blur is not None:
            g = ops.blur_apply(g, blur)
        return g

    # ------------------------------------------------------------------ faded blur of D's inputs
    def _blur_images_per_step(self):
        """n of the schedule: the real images D reads per step over all ranks"""
        return int(self.args.batch_size) * int(self.world)

    def _blur_tick(self):
        """Advances the host mirror of the blur's step counter, once per training step: at the top of train_step_from_inputs, or at the top
        of graph_step for a step that goes through it (eager, captured or replayed).  _blur_k_step: the k of the step now running."""
        self._blur_k_step = self._blur_k
        self._blur_k += 1

    def blur_live(self, k=None):
        """Whether the step after k training steps blurs: the restated radius is >= 1.  k None = the step now running (inside one), else
        the next one.  False for good once it has been false: sigma never rises."""
        if self.blur is None:
            return False
        if k is None:
            k = self._blur_k_step if self._blur_ticked else self._blur_k
        return blur_restate(k, self._blur_images_per_step(), self.blur)[1] >= 1

    def blur_sigma_now(self):
        """The sigma of the most recent step that blurred: the 1-element device view of the state's second word (no synchronisation;
        float() of it waits like float() of a loss), None when the key is off.  After the fade no launch writes it any more: it keeps the
        last live value, and blur_live() says that the step no longer blurs."""
        return None if self.blur is None else self.blur_state[1:2]

    def _ada_tick(self):
        """Advances the host mirror of the state's step counter, once per training step: at the top of train_step_from_inputs, or at
        the top of graph_step for a step that goes through it (eager, captured or replayed).  _ada_due: this step completes an interval."""
        self._ada_steps += 1
        self._ada_due = self._ada_steps >= self.ada["interval"]
        if self._ada_due:
            self._ada_steps = 0

    def _ada_control(self, heads, B):
        """One step of the controller on the compute stream: accumulate sign(real_pr - 0.5) over the B real rows of D's output, then
        adjust (a no-op on the device until the interval is full).  Data parallel: on the step that completes the interval the two
        counters {sum, rows} are all-reduced in between (8 bytes), so every rank computes the same p from the global statistic."""
        ops.ada_accumulate(self.ada_state, heads, B)
        if self._ada_due and self.sync.enabled:
            self.sync.all_reduce_now(self.ada_state.view(torch.int32)[1:3])
        ops.ada_adjust(self.ada_state, self.ada["interval"], self.ada["target"], self.ada["per_row"])

    def ada_p(self):
        """The present augmentation probability: the 1-element device view of the state's first word on the gated path (no
        synchronisation; float() of it waits like float() of a loss), None when every component is always applied."""
        return None if self.ada is None else self.ada_state[:1]

    def lr_now(self):
        """The rates of G, D, A of the most recent step under a schedule or warm-up: the 3-element device view of the state's words 2..4
        (no synchronisation; float() of an element waits like float() of a loss), None when the rates are constants (opt_cfg)."""
        return None if self.lr_state is None else self.lr_state[2:5]

    def grad_norm_now(self):
        """The gradient norms N of G, D, A of the most recent step each trained in, under clip_norm or skip_nonfinite: the 3-element
        device view of the records' first words (no synchronisation; float() of an element waits like float() of a loss), None when
        the guard is off."""
        return None if self.guard is None else self.guard_state.view(3, 8)[:, 0]

    def guard_counts(self):
        """{"G" | "D" | "A": (steps skipped, steps with a non-finite gradient)} so far, read from the device (synchronises: for the
        log and checkpoints), None when the guard is off."""
        if self.guard is None:
            return None
        words = self.guard_state.detach().cpu().view(torch.int32).view(3, 8)
        return {m: (int(words[i, 3]), int(words[i, 4])) for i, m in enumerate("GDA")}

    def _apply_optimizers(self, batch_no: int, run_adj: bool):
        a, st = self.args, self.store
        gscale = 1.0 / self.sync.world_size
        # under a schedule the Adam passes read their rate from the state the step's first launch wrote (1-element views of it)
        lr_view = None if self.lr_state is None else {m: self.lr_state[i:i + 1] for m, i in (("G", 2), ("D", 3), ("A", 4))}
        gd = self.guard
        g_lr = lr_view
        if gd is not None and lr_view is None:   # the guarded passes read their rate from device memory whether it is scheduled or not
            g_lr = {m: self._guard_lr[i:i + 1] for i, m in enumerate("GDA")}
        for m in self.adam_order:
            trained = m != "A" or run_adj
            if not trained and st.ema is None:
                continue
            lr, b1, b2 = self.opt_cfg[m]
            clip = a.clip_range if (m == "D" and a.use_clip) else 0.0
            lo, hi = train_weight_range(a, m, batch_no)
            s, e = st.model_range(m, lo, hi)
            if trained:
                self.sync.wait(m)
            if gd is not None and trained:
                # the norm of the (all-reduced) range this step trains, finished into the network's record, which the Adam pass and the
                # advance of the beta powers read: two more launches, nothing on the host
                rec = self._guard_rec[m]
                ops.guard_sumsq_partial(st.grad[s:e], self._guard_ws)
                ops.guard_finalise(self._guard_ws, e - s, rec, gscale, gd["clip_norm"], gd["skip"])
                if st.ema is None:
                    ops.guard_clip_adam_update(st.flat[s:e], st.grad[s:e], st.m[s:e], st.v[s:e], self.opt_state[m], g_lr[m], rec, b1, b2,
                                               ADAM_EPS, clip)
                else:
                    s0, e0 = st.model_range(m)
                    ops.guard_clip_adam_ema_update(st.flat[s0:e0], st.grad[s0:e0], st.m[s0:e0], st.v[s0:e0], st.ema[s0:e0], s - s0, e - s0,
                                                   self.opt_state[m], st.ema_updates, g_lr[m], rec, b1, b2, ADAM_EPS, clip,
                                                   self.ema_decay)
                ops.guard_adam_advance(self.opt_state[m], rec, b1, b2)
                continue
            # (under the guard only an Adjuster that does not train this step gets here: today's call, the average alone)
            if st.ema is None and lr_view is not None:
                ops.sched_clip_adam_update(st.flat[s:e], st.grad[s:e], st.m[s:e], st.v[s:e], self.opt_state[m], lr_view[m], b1, b2,
                                           ADAM_EPS, clip, gscale)
            elif st.ema is None:
                ops.clip_adam_update(st.flat[s:e], st.grad[s:e], st.m[s:e], st.v[s:e], self.opt_state[m], lr, b1, b2,
                                     ADAM_EPS, clip, gscale)
            else:
                # the same Adam on [s, e) fused with the weight average over the model's WHOLE range: outside the
                # trained group only w and ema are read; an Adjuster that does not train this step gets the average alone (lo == hi)
                s0, e0 = st.model_range(m)
                t_lo, t_hi = (s - s0, e - s0) if trained else (0, 0)
                if lr_view is not None:
                    ops.sched_clip_adam_ema_update(st.flat[s0:e0], st.grad[s0:e0], st.m[s0:e0], st.v[s0:e0], st.ema[s0:e0], t_lo, t_hi,
                                                   self.opt_state[m], st.ema_updates, lr_view[m], b1, b2, ADAM_EPS, clip, gscale,
                                                   self.ema_decay)
                else:
                    ops.clip_adam_ema_update(st.flat[s0:e0], st.grad[s0:e0], st.m[s0:e0], st.v[s0:e0], st.ema[s0:e0], t_lo, t_hi,
                                             self.opt_state[m], st.ema_updates, lr, b1, b2, ADAM_EPS, clip, gscale, self.ema_decay)
            if trained:
                ops.adam_advance(self.opt_state[m], b1, b2)
        if st.ema is not None:
            ops.ema_advance(st.ema_updates)   # after the last launch that read the counter: one average per step

    # ------------------------------------------------------------------ the weight average
    def reset_ema(self):
        """The average restarts from the present weights (count 0): after weights were loaded from outside a training step."""
        if self.store.ema is not None:
            self.store.ema.copy_(self.store.flat)
            self.store.ema_updates.zero_()

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block every model computes with the AVERAGED weights: `flat` and `ema` are exchanged in place (lg_swap_f32: no
        address changes, captured graphs stay valid) and exchanged back on exit.  A no-op when ema_decay == 0.  Nested use is a
        no-op too: the inner block finds the average already in place and leaves the way back to the outer one.  Training inside
        the block is refused."""
        st = self.store
        if st.ema is None or self._ema_live:
            yield
            return
        ops.swap_f32(st.flat, st.ema)
        st.bump()
        self._ema_live = True
        try:
            yield
        finally:
            ops.swap_f32(st.flat, st.ema)
            st.bump()
            self._ema_live = False

    def sampling_weights(self):
        """ema_weights() when the configuration samples from the average (ema_decay > 0 and sample_ema), else the raw weights."""
        return self.ema_weights() if (self.ema_decay > 0.0 and self.sample_ema) else contextlib.nullcontext()

    # ------------------------------------------------------------------ the same step as a replayed HIP graph
    def r1_step(self, batch_no: int) -> bool:
        """Whether this step carries the R1 penalty: stateless and resumable, like the partition steps."""
        return self.r1 is not None and batch_no % self.r1["interval"] == 0

    def r2_step(self, batch_no: int) -> bool:
        """Whether this step carries the R2 penalty: R1's schedule."""
        return self.r2 is not None and batch_no % self.r2["interval"] == 0

    def step_kind(self, batch_no: int):
        """Steps with the same kind enqueue the same kernels on the same shapes: (partition group or -1, Adjuster on, a penalty step
        — R1, R2 or both, which share a schedule; the last is constant with r1_gamma == 0 and r2_gamma == 0)."""
        a = self.args
        part = (batch_no // (a.partition_interval + 1)) % 3 if (a.use_partition and batch_no % (a.partition_interval + 1) == 0) else -1
        kind = part, bool(a.train_adj and batch_no > 10), self.r1_step(batch_no) or self.r2_step(batch_no)
        if self.blur is not None:   # with blur_init_sigma also: whether this step blurs — a faded step holds no blur launch
            kind += (self.blur_live(),)
        return kind

    def graph_step(self, batch_no: int, inp: Dict[str, torch.Tensor]):
        """train_step_from_inputs through a captured HIP graph, one graph per step kind (full step, the three partition
        groups, with / without the Adjuster branch).  The C ABI allocates nothing and never synchronises, so the whole
        step (~330 launches) is capturable; the first step of a kind runs eagerly (it is a real training step and sizes
        every workspace), the graph is captured right after it and every later step of that kind is one replay.
        Results are bit-identical to the eager path (tests/test_step_gpu.py::test_graph_replay_is_bit_exact).
        Single-GPU only: with data parallelism the all-reduces stay on the eager path."""
        if self.sync.enabled:
            if not getattr(self, "_graph_dp_warned", False):   # (round 5: said once instead of silently)
                import warnings
                warnings.warn("graph_step: data parallelism is on — the step runs on the eager path (all-reduces are not captured)",
                              RuntimeWarning, stacklevel=2)
                self._graph_dp_warned = True
            return self.train_step_from_inputs(batch_no, inp)
        if self.ada is not None and self.ada["target"] is not None:
            self._ada_tick()   # one training step, whether it runs eagerly, is captured and replayed, or is a replay alone
            self._ada_ticked = True
        if self.blur is not None:
            self._blur_tick()   # in the same way
            self._blur_ticked = True
        try:
            return self._graph_step(batch_no, inp)
        finally:
            self._ada_ticked = False
            if self.blur is not None:
                self._blur_ticked = False

    def _graph_step(self, batch_no: int, inp: Dict[str, torch.Tensor]):
        kind = self.step_kind(batch_no)
        if not hasattr(self, "_graphs"):
            self._graphs, self._graph_pool, self._graph_seen = {}, None, set()
            self._graph_in = {k: torch.empty_like(v) for k, v in inp.items()}
            if "disc_input" in inp:   # new_image must stay the first half of the static 2B-image buffer
                self._graph_in["new_image"] = self._graph_in["disc_input"][:inp["new_image"].shape[0]]
        for k, v in inp.items():
            if k != "disc_input":     # (its first half arrives as new_image, its second half is written by the step)
                self._graph_in[k].copy_(v)
        if kind not in self._graphs:
            if kind not in self._graph_seen:  # first step of this kind: eager (sizes workspaces, builds every lazy static)
                self._graph_seen.add(kind)
                return self.train_step_from_inputs(batch_no, self._graph_in)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            if self._graph_pool is None:
                self._graph_pool = torch.cuda.graph_pool_handle()
            # the graph records the raw addresses of ops.workspace() buffers: from here on an outgrown buffer is retired, not freed
            ops.pin_workspaces()
            prof_was, ops.Profile.enabled = ops.Profile.enabled, False   # HIP events cannot sit inside a captured graph
            try:
                with torch.cuda.graph(g, pool=self._graph_pool):   # records the launches, executes nothing
                    out = self.train_step_from_inputs(batch_no, self._graph_in)
            finally:
                ops.Profile.enabled = prof_was
            self._graphs[kind] = (g, out)
        g, out = self._graphs[kind]
        g.replay()
        return out

    # ------------------------------------------------------------------ eager_trainer.py:115-169
    def _train_step(self, batch_no, iterator):
        if hasattr(iterator, "get_next_raw") and getattr(self.args, "fuse_input", True):
            return self._train_step_packed(batch_no, iterator)
        try:
            real_image_1, real_cond_1 = iterator.get_next()
            real_image_2, real_cond_2 = iterator.get_next()
        except StopIteration:  # tf.errors.OutOfRangeError
            return None,
        if not real_cond_1.shape[0] == real_cond_2.shape[0] == self.args.batch_size:
            return False,
        # the augmented batch is written straight into the first half of D's [new_image ; fake] input
        d_in = torch.empty((2 * real_image_1.shape[0],) + tuple(real_image_1.shape[1:]), dtype=torch.float32, device=self.device)
        noise, new_image = self.draw_step_inputs(real_image_1, out=d_in[:real_image_1.shape[0]])
        inp = dict(real_image_1=real_image_1, real_cond_1=real_cond_1, real_image_2=real_image_2,
                   real_cond_2=real_cond_2, noise=noise, new_image=new_image, disc_input=d_in)
        if self.use_gp:
            inp["gp_eps"] = self.draw_gp_eps(real_image_1.shape[0])
        if self.dropout:
            inp["dropout_key"] = self.draw_dropout_key()
        if self.augmenting:
            inp["diffaug_key"] = self.draw_diffaug_key()
        fake, adj, lg, ld, la = self.train_step_from_inputs(batch_no, inp)
        return True, fake, adj, lg, ld, la

    def _train_step_packed(self, batch_no, iterator):
        """_train_step on a packed uint8 data set: the batches arrive as row indices into bytes on the device
        and the fused input kernels produce, bit for bit, the dict the float32 path builds."""
        if not iterator.has_next():
            return None,
        raw = iterator.get_next_raw()
        if not iterator.has_next():   # an odd batch at the end of the epoch: the float32 path draws nothing for it either
            raw.release()
            iterator.close()
            return None,
        B = raw.idx.shape[0]
        d_in = torch.empty((2 * B,) + tuple(raw.src.shape[1:]), dtype=torch.float32, device=self.device)
        noise, new_image, real_image_1 = self.draw_step_inputs_u8(raw.src, raw.idx, out=d_in[:B])
        raw.release()   # batch 1's bytes are consumed: its slot may be refilled (streamed mode; at least 1 slot in the ring)
        real_cond_1 = raw.cond
        raw = iterator.get_next_raw()
        real_image_2, real_cond_2 = ops.rescale_u8(raw.src, raw.idx), raw.cond
        raw.release()
        inp = dict(real_image_1=real_image_1, real_cond_1=real_cond_1, real_image_2=real_image_2,
                   real_cond_2=real_cond_2, noise=noise, new_image=new_image, disc_input=d_in)
        if self.use_gp:
            inp["gp_eps"] = self.draw_gp_eps(B)
        if self.dropout:
            inp["dropout_key"] = self.draw_dropout_key()
        if self.augmenting:
            inp["diffaug_key"] = self.draw_diffaug_key()
        fake, adj, lg, ld, la = self.train_step_from_inputs(batch_no, inp)
        return True, fake, adj, lg, ld, la

    def draw_step_inputs_u8(self, src, idx, out=None):
        """draw_step_inputs for a batch that is still bytes: the same step counter, seed and Philox windows; returns
        (noise, new_image, real_image_1), the last being the plain rescaled batch the same pass writes."""
        a = self.args
        self._input_step += 1
        seed = (int(getattr(a, "seed", 0)) << 20) ^ self.rank
        base = self._input_step << 40
        noise = ops.randn((a.batch_size, a.noise_dim), seed, base, device=self.device)
        new_image, real_image_1 = ops.augment_drawn_u8(src, idx, 0.02, 0.75, 1.003, 0.03, 0.1 * 0.2, seed, base + (1 << 39),
                                                       base + (1 << 38), out=out)
        return noise, new_image, real_image_1

    def draw_step_inputs(self, real_image_1, out=None):
        """eager_trainer.py:125-131 on the device: noise ~ N(0,1) and the augmented copy of the first real batch.  All
        draws are counter-based (Philox4x32-10 keyed by args.seed and the rank; one 2^40-block counter window per step),
        so a step's inputs can be regenerated from (seed, rank, step) alone."""
        a = self.args
        self._input_step += 1
        step = self._input_step
        seed = (int(getattr(a, "seed", 0)) << 20) ^ self.rank
        base = step << 40
        noise = ops.randn((a.batch_size, a.noise_dim), seed, base, device=self.device)
        # the scalar draws of the TF ops (one per batch) and the per-image flips come from the block window at 2^39 and are
        # made ON THE DEVICE (lg_augment_drawn): random_brightness(0.02), random_contrast(0.75, 1.003), random_hue(0.03),
        # random_flip_left_right, + 0.1 * N(0, 0.2) from the window at 2^38 — no host synchronisation in the step
        new_image = ops.augment_drawn(real_image_1.contiguous(), 0.02, 0.75, 1.003, 0.03, 0.1 * 0.2, seed,
                                      base + (1 << 39), base + (1 << 38), out=out)
        return noise, new_image

    def draw_gp_eps(self, B):
        """The gradient penalty's interpolation weights of the step draw_step_inputs last drew for: eps [B] ~ U[0,1) from the
        block window at 2^37 of that step's counter window (no other draw of a step uses it), on the device."""
        seed = (int(getattr(self.args, "seed", 0)) << 20) ^ self.rank
        return ops.gp_draw_eps(B, seed, (self._input_step << 40) + (1 << 37), device=self.device)

    def dropout_key_words(self):
        """(seed, key_offset) of the dropout masks of the step draw_step_inputs last drew for: the block window at 2^36 of that step's
        counter window (0, 2^39, 2^38 and 2^37 are the other draws').  input_step is part of the checkpoint, so a resumed run
        continues the mask stream."""
        seed = (int(getattr(self.args, "seed", 0)) << 20) ^ self.rank
        return seed, (self._input_step << 40) + (1 << 36)

    def draw_dropout_key(self):
        """dropout_key_words as the int64 [2] device tensor the norm kernels read, written on the device from launch scalars
        (lg_dropout_key): like the other draws of the step, no host-to-device copy and no host synchronisation."""
        return ops.dropout_key(*self.dropout_key_words(), device=self.device)

    def diffaug_key_words(self):
        """(seed, key_offset) of the augmentation draws of the step draw_step_inputs last drew for: the block window at 2^35 of that
        step's counter window (0, 2^39, 2^38, 2^37 and 2^36 are the other draws').  input_step is part of the checkpoint, so a resumed
        run continues the stream."""
        seed = (int(getattr(self.args, "seed", 0)) << 20) ^ self.rank
        return seed, (self._input_step << 40) + (1 << 35)

    def draw_diffaug_key(self):
        """diffaug_key_words as the int64 [2] device tensor lg_diffaug_draw reads, written on the device from launch scalars (the
        kernel of the dropout key): no host-to-device copy and no host synchronisation."""
        return ops.dropout_key(*self.diffaug_key_words(), device=self.device)

    # ------------------------------------------------------------------ eager_trainer.py:180-229
    def _interrupted(self, signum, f_name):
        """eager_trainer.py:171-178: SIGINT saves an "interrupt" checkpoint + status.json and exits 1."""
        self.save_checkpoint("interrupt")
        with open(os.path.join(self.args.result_dir, "checkpoint", "status.json"), "w") as f:
            json.dump({"epoch": self.global_epoch}, f)
        print("\n Checkpoint has been saved")
        print(signum, f_name)
        import sys
        sys.exit(1)

    def train(self):
        a = self.args
        # data parallel (one process per GPU): every file of the run is written by rank 0 alone — two ranks writing the
        # same checkpoint / image / JSON paths race (and a rank that dies there leaves the others in an all-reduce)
        io = not getattr(a, "no_io", False) and getattr(a, "result_dir", None) and self.rank == 0
        if io:
            import signal
            signal.signal(signal.SIGINT, self._interrupted)
        for e in range(self.global_epoch, a.epoch + 1):
            print("Experiment:", a.exp_name, "Epoch:", e, "Starting...")
            self.global_epoch = e
            iterator = self.dataset.get_new_iterator()
            start_time = time.time()
            seen = 0
            for b in range(1, self.dataset.batches + 1):
                result = self._train_step(b, iterator)
                if result[0] is None:
                    break
                elif not result[0]:
                    continue
                seen += a.batch_size * 2
                if b % a.freq_gen == 0 and self.rank == 0:
                    if io:
                        save_image(result[1], os.path.join(a.result_dir, "train", "gen", "%d-%d.jpg" % (e, b)))
                        if result[2] is not None:
                            save_image(result[2], os.path.join(a.result_dir, "train", "adj", "%d-%d.jpg" % (e, b)))
                    lg, ld = float(result[3]), float(result[4])
                    la = float(result[5]) if result[5] is not None else float("nan")
                    aug_p = "" if self.ada is None else f" AugP {float(self.ada_p()):.4f}"   # read where the losses are: no sync of its own
                    r1 = "" if self.r1 is None else f" R1 {float(self.losses['r1']):.4f}"   # the term of the most recent penalty step
                    if self.r2 is not None:
                        r1 += f" R2 {float(self.losses['r2']):.4f}"
                    lrs = "" if self.lr_state is None else " LR g/d/a " + "/".join(f"{x:.3e}" for x in self.lr_now().tolist())
                    gn = ""
                    if self.guard is not None:   # the norms of the most recent step and the skips so far, read where the losses are
                        cnt = self.guard_counts()
                        gn = " GN g/d/a " + "/".join(f"{x:.3e}" for x in self.grad_norm_now().tolist()) \
                             + " Skip g/d/a " + "/".join(str(cnt[m][0]) for m in "GDA")
                    bl = ""
                    if self.blur is not None and self.blur_live(self._blur_k_step):   # the sigma of the step the losses are of
                        bl = f" Blur {float(self.blur_sigma_now()):.4f}"
                    print(f"  [{seen}] LossG {lg:.4f} LossD {ld:.4f} LossA {la:.4f}{r1}{aug_p}{lrs}{gn}{bl}")
                if b % a.freq_test == 0 and io and self.test_cond is not None:
                    self.predict(self.test_noise, self.test_cond, self.test_image,
                                 os.path.join(a.result_dir, "test", "gen", "%d-%d.jpg" % (e, b)),
                                 os.path.join(a.result_dir, "test", "disc", "%d-%d.json" % (e, b)),
                                 os.path.join(a.result_dir, "test", "adj", "%d-%d.jpg" % (e, b)))
            torch.cuda.synchronize()
            print("Time usage:", time.time() - start_time, "s")
            if io:  # eager_trainer.py:229
                self.save_checkpoint(str(e))
            _barrier()  # the other ranks do not run ahead into the next epoch while rank 0 writes

    # ------------------------------------------------------------------ eager_trainer.py:265-298
    def predict(self, noise, cond, image, gen_image_save_path=None, json_save_path=None, adj_image_save_path=None, ema=None):
        """ema: compute with the averaged weights.  None = the configuration's choice (ema_decay > 0 and sample_ema);
        True without an average (ema_decay == 0) is the raw weights."""
        with (self.sampling_weights() if ema is None else self.ema_weights() if ema else contextlib.nullcontext()):
            return self._predict(noise, cond, image, gen_image_save_path, json_save_path, adj_image_save_path)

    def _predict(self, noise, cond, image, gen_image_save_path, json_save_path, adj_image_save_path):
        start_time = time.time()
        gen_image = self.generator([noise, cond])
        torch.cuda.synchronize()
        print("Generate Time", time.time() - start_time, "s")
        if gen_image_save_path is not None:
            save_image(gen_image, gen_image_save_path)
        save = dict()
        save["real_cond"] = cond
        save["real_pr"], save["real_c"] = self.discriminator(image)
        save["fake_pr"], save["fake_c"] = self.discriminator(gen_image)
        mse = lambda t, p: float(((t - p) ** 2).mean(dim=-1).mean(dim=0))
        save["real_pr_mse"] = mse(soft(1.0), save["real_pr"])
        save["real_c_mse"] = mse(cond, save["real_c"])
        save["fake_pr_mse"] = mse(soft(0.0), save["fake_pr"])
        save["fake_c_mse"] = mse(cond, save["fake_c"])
        for x in ["real_cond", "real_pr", "real_c", "fake_c", "fake_pr"]:
            save[x] = torch.round(save[x] * 100).to(torch.int64).cpu().tolist()
        if json_save_path is not None:
            with open(json_save_path, "w") as f:
                json.dump(save, f)
        adj_fake_image, adj_real_image = None, None
        if self.args.train_adj:
            adj_real_image = self.adjuster([image, cond])
            adj_fake_image = self.adjuster([gen_image, cond])
            if adj_image_save_path is not None:
                save_image(torch.cat([adj_real_image, adj_fake_image], 0), adj_image_save_path)
        return gen_image, save, adj_real_image, adj_fake_image

    # ------------------------------------------------------------------ shell (own format; TF checkpoints are out of scope)
    def _init_dir(self):
        rd = getattr(self.args, "result_dir", None)
        if not rd or getattr(self.args, "no_io", False):
            return
        for item in [".", "train/gen", "train/adj", "test/adj", "test/gen", "test/disc", "checkpoint", "log", "sample",
                     "evaluate/gen", "evaluate/adj", "evaluate/disc", "model"]:
            os.makedirs(os.path.join(rd, item), exist_ok=True)

    def _init_test_data(self):
        """eager_trainer.py:65-83: the FIXED evaluation batch {n: noise, c: cond, i: image} of `predict`.  Loaded from
        <test_data_dir>/test_data_<env>.npz when that file exists and args.reuse is set; otherwise drawn once (first
        batch of a fresh iterator + N(0,1) noise) and written there, so every later run evaluates the same batch."""
        import numpy as np
        self.test_noise = self.test_cond = self.test_image = None
        a = self.args
        tdir = getattr(a, "test_data_dir", None)
        npz = os.path.join(tdir, "test_data_" + str(getattr(a, "env", "default")) + ".npz") if tdir else None

        def usable(path):
            """a complete file whose shapes the models accept (the reference loads whatever batch count the file holds and regenerates
            only when G / D / A reject its shapes, :69-83): noise_dim, cond_dim, H, W, C must fit; n, c, i share one leading
            dimension, which need NOT be args.batch_size (a file written under another batch size, or from a short first batch)."""
            try:
                with np.load(path) as d:
                    n, c, i = d["n"], d["c"], d["i"]
            except Exception as e:
                print(f"test data {path}: unreadable ({e}); regenerating")
                return False
            H = a.init_dim * 16
            why = None
            if n.ndim != 2 or n.shape[1] != a.noise_dim:
                why = f"noise {n.shape} does not fit noise_dim {a.noise_dim}"
            elif c.ndim != 2 or c.shape[1] != a.cond_dim:
                why = f"cond {c.shape} does not fit cond_dim {a.cond_dim}"
            elif i.ndim != 4 or tuple(i.shape[1:]) != (H, H, a.image_channel):
                why = f"image {i.shape} does not fit {H}x{H}x{a.image_channel}"
            elif not (n.shape[0] == c.shape[0] == i.shape[0] and n.shape[0] > 0):
                why = f"n, c, i hold {n.shape[0]}, {c.shape[0]}, {i.shape[0]} samples"
            if why:
                print(f"test data {path}: {why}; regenerating")
            return why is None

        # data parallel: ONE decision for all ranks (rank 0 looks, the others are told) — a rank that finds rank 0's half-
        # written file, or loads while others generate, would leave the dataset generators of the ranks one draw apart
        load = bool(npz and getattr(a, "reuse", False) and os.path.isfile(npz) and usable(npz)) if self.rank == 0 else False
        if self.world > 1:
            flag = [load]
            torch.distributed.broadcast_object_list(flag, src=0)
            load = flag[0]
        if load:
            data = np.load(npz)
            to = lambda v: torch.tensor(np.asarray(v, np.float32), device=self.device)
            self.test_noise, self.test_cond, self.test_image = to(data["n"]), to(data["c"]), to(data["i"])
            if self.dataset is not None and self.world > 1:
                # data parallel only: the generating path draws one epoch order — keep every rank's (and every path's) dataset
                # generator in step.  A single process does not draw (the reference does not on reuse, :69-76).
                self.dataset.get_new_iterator()
            return
        if self.dataset is None:
            if getattr(a, "reuse", False) and npz:   # dataset-less modes (condition-sample, export-model): say so, they do not evaluate
                print(f"No fixed evaluation batch: {npz} is missing or does not fit this configuration and there is no dataset to draw "
                      "one from (test_noise / test_cond / test_image stay None)")
            return
        print("No reuse test data, generating...")
        it = self.dataset.get_new_iterator()
        self.test_image, self.test_cond = it.get_next()
        # tf.random.normal([B, noise_dim]) (:82) from the counter-based generator: window 0 is never used by a step
        seed = (int(getattr(a, "seed", 0)) << 20) ^ 0xFFFFF
        self.test_noise = ops.randn((self.test_cond.shape[0], a.noise_dim), seed, 0, device=self.device)
        if npz and self.rank == 0 and not getattr(a, "no_io", False):
            os.makedirs(tdir, exist_ok=True)
            tmp = npz + ".tmp.npz"   # written whole, then renamed: no reader ever sees a partial file
            np.savez_compressed(tmp, n=self.test_noise.cpu().numpy(), c=self.test_cond.cpu().numpy(),
                                i=self.test_image.cpu().numpy())
            os.replace(tmp, npz)
        _barrier()

    # ---- checkpoints (own format: the TF checkpoint format is out of scope, the CONTENT is the reference's:
    # tf.train.Checkpoint(discriminator, generator, adjuster, three optimizers) eager_trainer.py:31-35)
    def checkpoint_state(self) -> dict:
        st = self.store
        ck = {"format": "littlegan_amd-ckpt-1",
              "names": {m: st.names(m) for m in "GDA"},
              "flat": st.flat.detach().cpu(), "adam_m": st.m.detach().cpu(), "adam_v": st.v.detach().cpu(),
              "beta_powers": {m: t.detach().cpu() for m, t in self.opt_state.items()},
              "epoch": self.global_epoch, "input_step": int(self._input_step)}
        if st.ema is not None:   # the weight average and the count of averages taken (absent with ema_decay == 0; same format)
            ck["ema"], ck["ema_updates"] = st.ema.detach().cpu(), int(st.ema_updates.item())
        if self.ada is not None:   # {p, sum, rows, steps} as its four 32-bit words (absent on the plain diff_augment path)
            ck["ada_state"] = self.ada_state.detach().cpu().view(torch.int32)
        if self.lr_state is not None:   # the schedule's step counter (absent when the rates are constants)
            ck["lr_sched_state"] = ops.sched_read(self.lr_state)[0]
        if self.guard is not None:   # the six counters {skipped, non-finite} of G, D, A (absent when the guard is off)
            cnt = self.guard_counts()
            ck["grad_guard_state"] = [int(x) for m in "GDA" for x in cnt[m]]
        if self.blur is not None:   # the blur's step counter, from the host mirror (absent when the key is off)
            ck["blur_state"] = int(self._blur_k)
        return ck

    def save_checkpoint(self, tag: str) -> str:
        """Rank 0 writes (weights are identical on every rank after the all-reduced step); other ranks return the path."""
        d = os.path.join(self.args.result_dir, "checkpoint")
        if self.rank != 0:
            return os.path.join(d, f"ckpt-{tag}.pt")
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, f"ckpt-{tag}.pt")
        tmp = path + ".tmp"
        torch.save(self.checkpoint_state(), tmp)
        os.replace(tmp, path)  # a killed save never leaves a truncated "latest"
        with open(os.path.join(d, "checkpoint"), "w") as f:  # same role as TF's "checkpoint" index file
            json.dump({"latest": os.path.basename(path)}, f)
        return path

    def latest_checkpoint(self) -> Optional[str]:
        d = os.path.join(self.args.result_dir, "checkpoint")
        idx = os.path.join(d, "checkpoint")
        if not os.path.isfile(idx):
            return None
        with open(idx) as f:
            p = os.path.join(d, json.load(f)["latest"])
        return p if os.path.isfile(p) else None

    def load_checkpoint(self, path: str):
        ck = torch.load(path, map_location="cpu", weights_only=True)
        st = self.store
        if ck.get("format") != "littlegan_amd-ckpt-1":
            raise ValueError(f"{path}: not a littlegan_amd checkpoint")
        for m in "GDA":
            if ck["names"][m] != st.names(m):
                raise ValueError(f"{path}: weight list of {m} does not match this model configuration")
        if ck["flat"].numel() != st.flat.numel():
            raise ValueError(f"{path}: {ck['flat'].numel()} parameters, this configuration has {st.flat.numel()}")
        ada_words = None
        if self.ada is not None and "ada_state" in ck:   # checked before anything is loaded: the draw turns p into an integer threshold
            ada_words = ck["ada_state"].to(torch.int32).reshape(-1)
            p = float(ada_words[:1].view(torch.float32)) if ada_words.numel() == 4 else float("nan")
            if not (0.0 <= p <= 1.0 and int(ada_words[2]) >= 0 and int(ada_words[3]) >= 0):
                raise ValueError(f"{path}: ada_state {ada_words.tolist()} is not a controller state (four words with 0 <= p <= 1, "
                                 f"rows >= 0, steps >= 0; p read as {p})")
        lr_k = None
        if self.lr_state is not None and "lr_sched_state" in ck:   # checked before anything is loaded, like the words above
            lr_k = ck["lr_sched_state"]
            if isinstance(lr_k, bool) or not isinstance(lr_k, int) or not 0 <= lr_k < 2 ** 31:
                raise ValueError(f"{path}: lr_sched_state {lr_k!r} is not a step counter (one integer, 0 <= k < 2^31)")
        guard_cnt = None
        if self.guard is not None and "grad_guard_state" in ck:   # checked before anything is loaded, like the words above
            guard_cnt = ck["grad_guard_state"]
            if not (isinstance(guard_cnt, (list, tuple)) and len(guard_cnt) == 6
                    and all(isinstance(x, int) and not isinstance(x, bool) and 0 <= x < 2 ** 31 for x in guard_cnt)
                    and all(guard_cnt[i] <= guard_cnt[i + 1] for i in (0, 2, 4))):
                raise ValueError(f"{path}: grad_guard_state {guard_cnt!r} is not the guard's counters (six integers {{skipped, non-finite}} "
                                 "of G, D, A, 0 <= skipped <= non-finite < 2^31)")
        blur_k = None
        if self.blur is not None and "blur_state" in ck:   # checked before anything is loaded, like the words above
            blur_k = ck["blur_state"]
            if isinstance(blur_k, bool) or not isinstance(blur_k, int) or not 0 <= blur_k < 2 ** 31:
                raise ValueError(f"{path}: blur_state {blur_k!r} is not a step counter (one integer, 0 <= k < 2^31)")
        st.flat.copy_(ck["flat"])
        st.m.copy_(ck["adam_m"])
        st.v.copy_(ck["adam_v"])
        for m, t in ck["beta_powers"].items():
            self.opt_state[m].copy_(t)
        self._input_step = int(ck.get("input_step", 0))  # a resumed run continues the Philox input stream
        if st.ema is not None:   # (a checkpoint's average is ignored when this run keeps none)
            if "ema" in ck and "ema_updates" in ck:
                st.ema.copy_(ck["ema"])
                st.ema_updates.fill_(int(ck["ema_updates"]))
            else:
                print(f"{path}: no weight average in this checkpoint; it restarts from the loaded weights (0 updates)")
                self.reset_ema()
        if self.ada is not None:   # (a checkpoint's p is ignored when this run gates nothing; without one p starts as configured)
            if "ada_state" in ck:
                self.ada_state.view(torch.int32).copy_(ada_words)
                self._ada_steps = int(ada_words[3])
            else:
                print(f"{path}: no augmentation probability in this checkpoint; it starts from the configured {self.ada['p0']}")
        if self.lr_state is not None:   # (a checkpoint's counter is ignored when this run schedules nothing)
            if lr_k is None:
                print(f"{path}: no learning-rate step counter in this checkpoint; the schedule starts at k = 0")
            ops.sched_init(lr_k or 0, out=self.lr_state)
        if self.guard is not None:   # (a checkpoint's counters are ignored when this run guards nothing; without them they start at zero)
            if guard_cnt is None:
                print(f"{path}: no gradient-guard counters in this checkpoint; they start at zero")
            for i, m in enumerate("GDA"):
                ops.guard_init(*(guard_cnt[2 * i:2 * i + 2] if guard_cnt is not None else (0, 0)), out=self._guard_rec[m])
        if self.blur is not None:
            if blur_k is None:
                print(f"{path}: no blur step counter in this checkpoint; the fade starts at k = 0")
            self._blur_k = self._blur_k_step = blur_k or 0
            ops.blur_init(self._blur_k, out=self.blur_state)
        elif "blur_state" in ck:
            print(f"{path}: this run does not blur (blur_init_sigma = 0); the checkpoint's blur step counter is ignored")
        st.bump()

    def export_model_checkpoint(self):
        path = os.path.join(self.args.result_dir, "model", "model.pt")
        out = {"names": {m: self.store.names(m) for m in "GDA"}, "flat": self.store.flat.cpu()}
        if self.store.ema is not None:
            out["ema_flat"] = self.store.ema.cpu()
        torch.save(out, path)
        return path

    def plot(self):
        raise NotImplementedError("plot (keras plot_model / pydot) is UI tooling outside the hot path (SURVEY.md §2 row 5)")
