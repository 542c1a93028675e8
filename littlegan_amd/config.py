"""Mirror of /root/reference/config.py:6-42: sample.config.json < <env>.config.json < CLI, every key an
attribute, derived cond_dim / result_dir / gpu / prefetch.  Extra keys of this build: mfma_dtype ("f32" |
"bf16"), synthetic (bool: use the synthetic CelebA-shaped dataset), seed, packed_path / data_resident / fuse_input
(the packed uint8 data set, dataset.py), fid_chunk_rows / fid_device_sqrt (streamed FID statistics, device square root, fid.py), dropout_train (bool: make the encoder's
dropout(dropout_rate) live in the training step — the reference's, and the default here, is the identity),
ema_decay / sample_ema (exponential moving average of the weights, used for sampling and kept in checkpoints),
diff_augment (comma list out of color,translation,cutout: differentiable augmentation of every image the Discriminator sees in the
training step, the generator-side tapes differentiated through it; "" = off, the reference's step),
evaluate_metrics (list out of fid, kid, prdc: what `evaluate` computes; ["fid"] = the reference's run) / evaluate_real_activations (the
real images' saved activations that kid and prdc need) / kid_subsets / kid_subset_size / prdc_k (metrics.py)."""
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
    # sample-based metrics beside FID: which metrics `evaluate` runs (a list out of fid, kid, prdc); the saved
    # activations of the real images that kid / prdc compare against (the stats file holds only mu and sigma; a path, relative ones
    # under test_data_dir); subsets and rows per subset of KID (0 subsets = one estimate over the full sets); k of the k-NN manifolds
    'evaluate_metrics': ['fid'], 'evaluate_real_activations': None, 'kid_subsets': 100, 'kid_subset_size': 1000, 'prdc_k': 3,
}

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
