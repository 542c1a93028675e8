"""Input side of the C3 step (128x128, B=256, bf16, Adjuster on) measured end to end:

    python scripts/bench_input.py [--steps K] [--warmup W] [--images N] [--out FILE]

A loop of EagerTrainer._train_step calls (two real batches per step) on
  (a) a synthetic data set whose batches are already float32 on the device (no input work: the ceiling),
  (b) the JPEG folder loader (decode, rescale and upload in the training thread),
  (c) the uint8 pack, streamed through the ring of pinned buffers,
  (d) the uint8 pack, resident on the device,
and the three input kernels alone, timed with HIP events at B=256, with their achieved GB/s.  The JPEG folder is written
here, seeded, into a temporary directory, packed with pack_dataset, and removed at the end.  One process, one JSON line."""
import argparse
import contextlib
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIM, B, N_ATTR = 128, 256, 40


def write_folder(root, n, workers):
    """n seeded 128x128 JPEGs (smooth gradients + noise: a photo-like decode cost) and a 40-column attribute file"""
    from PIL import Image
    os.makedirs(os.path.join(root, "img"))
    yy, xx = np.mgrid[0:DIM, 0:DIM].astype(np.float32) / DIM

    def one(i):
        rng = np.random.default_rng(i)
        base = np.stack([np.sin(6.28 * (xx * rng.uniform(0.5, 3) + rng.uniform())), np.cos(6.28 * (yy * rng.uniform(0.5, 3))),
                         xx * yy * 2 - 1], -1)
        a = np.clip(127.5 * (base + 1) + rng.normal(0, 12, (DIM, DIM, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(a, "RGB").save(os.path.join(root, "img", f"{i:06d}.jpg"), quality=90)

    with ThreadPoolExecutor(workers) as ex:
        list(ex.map(one, range(n)))
    rng = np.random.default_rng(1)
    with open(os.path.join(root, "attr.txt"), "w") as f:
        for i in range(n):
            f.write(f"{i:06d}.jpg " + " ".join(str(v) for v in rng.choice([-1, 1], N_ATTR)) + "\n")


class ResidentSynthetic:
    """(a): the synthetic stand-in's batches generated once and kept on the device; get_next() only hands them out."""

    def __init__(self, ds, n):
        self.batches = [ds._batch(b) for b in range(n)]
        self.i = 0

    def get_next(self):
        self.i += 1
        return self.batches[self.i % len(self.batches)]


class Epochs:
    """get_next()/get_next_raw()/has_next() over a data set, opening a new iterator when an epoch ends (the timed loop
    spans several epochs of the small benchmark folder; a step always finds two batches)."""

    def __init__(self, ds):
        self.ds, self.it = ds, ds.get_new_iterator()
        if hasattr(self.it, "get_next_raw"):
            self.get_next_raw, self.has_next = self._raw, (lambda: True)

    def _fresh(self):
        if hasattr(self.it, "close"):
            self.it.close()
        self.it = self.ds.get_new_iterator()

    def _raw(self):
        if not self.it.has_next():
            self._fresh()
        return self.it.get_next_raw()

    def get_next(self):
        try:
            return self.it.get_next()
        except StopIteration:
            self._fresh()
            return self.it.get_next()


def time_loop(tr, it, warmup, steps):
    for b in range(1, warmup + 1):
        assert tr._train_step(b, it)[0] is True
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ok = [tr._train_step(b, it)[0] for b in range(warmup + 1, warmup + steps + 1)]
    torch.cuda.synchronize()
    assert all(r is True for r in ok)   # every timed call ran a whole step
    return (time.perf_counter() - t0) / steps * 1e3


def time_kernel(fn, variants, iters=20):
    """mean ms of fn(variant) over `iters` launches between two HIP events, cycling through different row sets"""
    for v in variants[:3]:
        fn(v)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(variants[i % len(variants)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=12)   # >= 11: the Adjuster branch runs from step 11
    ap.add_argument("--folder-steps", type=int, default=8, help="timed steps of the (slow) folder loader")
    ap.add_argument("--images", type=int, default=32 * B)
    ap.add_argument("--repeats", type=int, default=3, help="repeats of (a), (c), (d): the run-to-run spread")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.warmup < 11:
        ap.error("--warmup must be at least 11 (the Adjuster branch)")
    import bench
    from littlegan_amd import ops
    from littlegan_amd.dataset import CelebA, pack_dataset
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    workers = min(16, os.cpu_count() or 1)
    torch.cuda.set_device(0)
    tmp = tempfile.mkdtemp(prefix="littlegan_input_bench_")
    res = {"workload": "C3: 128x128x3, B=256, bf16, Adjuster on; 2 real batches per step", "steps": a.steps, "warmup": a.warmup,
           "images": a.images, "device": torch.cuda.get_device_name(0)}
    try:
        t0 = time.perf_counter()
        write_folder(tmp, a.images, workers)
        res["write_jpeg_s"] = round(time.perf_counter() - t0, 2)
        args = bench.make_args("c3", "cuda:0")
        for k, v in dict(image_path=os.path.join(tmp, "img"), attr_path=os.path.join(tmp, "attr.txt"), image_ext="jpg", image_dim=DIM,
                         attr=list(range(N_ATTR)), threads=workers, prefetch_batch=3, packed_path=None, data_resident="auto",
                         fuse_input=True, synthetic=False).items():
            setattr(args, k, v)
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(sys.stderr):
            pack_dataset(args, os.path.join(tmp, "pack"))
        res["pack_s"] = round(time.perf_counter() - t0, 2)
        with contextlib.redirect_stdout(sys.stderr):
            def trainer(fuse=True):
                # a new trainer per loop: every loop starts from the initial weights, as bench.py does (the step's time drifts
                # by several per cent over a few hundred steps of training in one process, whatever feeds it)
                torch.manual_seed(0)
                targs = argparse.Namespace(**dict(vars(args), fuse_input=fuse))
                decoder, encoder = Decoder(targs), Encoder(targs)
                gen = Generator(targs, decoder)
                disc = Discriminator(targs, encoder)
                return EagerTrainer(targs, gen, disc, Adjuster(targs, disc, gen), None)

            def dataset(**kw):
                d = dict(vars(args))
                d.update(kw)
                return CelebA(argparse.Namespace(**d))

            pack = os.path.join(tmp, "pack")
            loops = {"a_synthetic_resident": [], "d_pack_resident": [], "d_pack_resident_unfused": [], "c_pack_streamed": []}
            syn = ResidentSynthetic(dataset(synthetic=True, synthetic_images=8 * B), 8)
            ds_res, ds_str = dataset(packed_path=pack, data_resident=True), dataset(packed_path=pack, data_resident=False)
            for _ in range(a.repeats):   # the modes interleaved, so that a drift of the clock shows in all of them alike
                loops["a_synthetic_resident"].append(time_loop(trainer(), syn, a.warmup, a.steps))
                loops["d_pack_resident"].append(time_loop(trainer(), Epochs(ds_res), a.warmup, a.steps))
                # the same pack through get_next(): lg_rescale_u8 x 2, then the float32 augmentation
                loops["d_pack_resident_unfused"].append(time_loop(trainer(fuse=False), Epochs(ds_res), a.warmup, a.steps))
                loops["c_pack_streamed"].append(time_loop(trainer(), Epochs(ds_str), a.warmup, a.steps))
            loops["b_jpeg_folder"] = [time_loop(trainer(), Epochs(dataset()), a.warmup, a.folder_steps)]
        # what one streamed batch costs its worker: rows of the memory map into a pinned buffer, then the upload
        pinned = torch.empty((B, DIM, DIM, 3), dtype=torch.uint8).pin_memory()
        slot = torch.empty((B, DIM, DIM, 3), dtype=torch.uint8, device="cuda")
        t0 = time.perf_counter()
        for b in range(16):
            np.copyto(pinned.numpy(), ds_str._images[b * B:(b + 1) * B])
        memcpy_ms = (time.perf_counter() - t0) / 16 * 1e3
        h2d_ms = time_kernel(lambda _: slot.copy_(pinned, non_blocking=True), [None])
        res["stream_worker_per_batch"] = {"memmap_to_pinned_ms": round(memcpy_ms, 3), "h2d_ms": round(h2d_ms, 3),
                                          "bytes": pinned.numel()}
        res["ms_per_step"] = {k: [round(x, 3) for x in v] for k, v in loops.items()}
        res["images_per_s"] = {k: round(2 * B / (min(v) * 1e-3)) for k, v in loops.items()}
        # the kernels alone: B=256 rows drawn from the resident pack, a different row set per launch
        src, attr = ds_res._images_dev, ds_res._attr
        g = torch.Generator().manual_seed(0)
        rows = [torch.randperm(a.images, generator=g)[:B].cuda() for _ in range(8)]
        cols = torch.arange(N_ATTR, dtype=torch.int32, device="cuda")
        out_a, out_r = torch.empty(B, DIM, DIM, 3, device="cuda"), torch.empty(B, DIM, DIM, 3, device="cuda")
        out_c = torch.empty(B, N_ATTR, device="cuda")
        u8, f32 = B * DIM * DIM * 3, B * DIM * DIM * 3 * 4
        kern = {}
        for name, fn, nbytes in (
                ("lg_rescale_u8", lambda r: ops.rescale_u8(src, r, out=out_r), u8 + f32),
                ("lg_augment_drawn_u8", lambda r: ops.augment_drawn_u8(src, r, 0.02, 0.75, 1.003, 0.03, 0.02, 1, 1 << 39, 1 << 38,
                                                                       out=out_a, out_rescaled=out_r), 2 * u8 + 2 * f32),
                ("lg_augment_drawn_u8(noise_scale=0)", lambda r: ops.augment_drawn_u8(src, r, 0.02, 0.75, 1.003, 0.03, 0.0, 1, 1 << 39, 1 << 38,
                                                                                      out=out_a, out_rescaled=out_r), 2 * u8 + 2 * f32),
                ("lg_augment_drawn(f32, for comparison)", lambda r: ops.augment_drawn(out_r, 0.02, 0.75, 1.003, 0.03, 0.02, 1, 1 << 39,
                                                                                      1 << 38, out=out_a), 3 * f32),
                ("lg_soft_labels", lambda r: ops.soft_labels(attr, r, cols, out=out_c), 2 * B * N_ATTR * 4 + B * 8)):
            ms = time_kernel(fn, rows)
            kern[name] = {"ms": round(ms, 4), "bytes": nbytes, "GB_per_s": round(nbytes / ms / 1e6, 1)}
        res["kernels_B256"] = kern
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
