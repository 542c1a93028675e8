"""Times the training step with the discriminator gradient penalty off and on and prints one JSON line per
configuration.  `python scripts/bench_gp.py [--workload c3|c2] [--steps K] [--warmup W]`: C3 = bf16, B = 256, G + D + Adjuster;
C2 = exact f32, B = 64, G + D.  Steps are replayed graphs of the full-step kind (EagerTrainer.graph_step), timed with HIP events."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_step(workload, use_gp, steps, warmup):
    import bench
    from littlegan_amd import ops
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    args = bench.make_args(workload, "cuda")
    args.use_gp, args.gp_weight = use_gp, 5.0
    args.use_partition = False   # every step the full-step kind: one graph
    dec, enc = Decoder(args), Encoder(args)
    g = Generator(args, dec)
    d = Discriminator(args, enc)
    tr = EagerTrainer(args, g, d, Adjuster(args, d, g), None)
    inp = bench.synthetic_inputs(args, "cuda", 0)
    if use_gp:
        inp["gp_eps"] = ops.gp_draw_eps(args.batch_size, 7, 0)
    b0 = 12 if args.train_adj else 1   # the Adjuster branch runs from step 11
    for i in range(warmup):
        tr.graph_step(b0 + i, inp)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        tr.graph_step(b0 + warmup + i, inp)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    out = {"workload": workload, "dtype": args.mfma_dtype, "batch": args.batch_size, "use_gp": use_gp, "ms_per_step": round(ms, 3),
           "images_per_sec": round(2 * args.batch_size / ms * 1e3, 1), "steps": steps, "warmup": warmup}
    if use_gp:
        out["gp"] = float(tr.losses["gp"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["c3", "c2"], default=None, help="default: both")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    for wl in ([a.workload] if a.workload else ["c3", "c2"]):
        for gp in (False, True):
            print(json.dumps(time_step(wl, gp, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
