"""Times the training step with the differentiable augmentation of D's inputs off and on (diff_augment) and records the
result in profiles/diffaug_bench.json.  `python scripts/bench_diffaug.py [--workload c3|c2] [--pairs P] [--block K] [--out FILE]`:
C3 = bf16, B = 256, G + D + Adjuster; C2 = exact f32, B = 64, G + D; synthetic data (bench.synthetic_inputs).

Both trainers live in ONE process and start from the same weights.  Steps are replayed graphs (EagerTrainer.graph_step) with the
partition schedule of the benchmark, so a block holds every step kind in its schedule's proportion (K a multiple of 15: three full
cycles of the partition groups per 45 steps); the warm-up runs 45 steps per trainer, which takes every kind through its eager
step, its capture and a replay.  Then P pairs of blocks alternate off / on, each block timed with HIP events; the on trainer gets
a fresh key every step, as in training.  Reported: every block's ms per step, the mean difference on - off, and the spread
(max - min) of the off blocks — the yardstick a difference has to exceed to mean anything.  "on" is the full policy
(color,translation,cutout): the passes cost the same whatever the policy names, which acts in the draw kernel alone.
The times of the three new kernels (draw, per-sample sums, the element-wise pass; forward and adjoint) come from a separate
`rocprofv3 --kernel-trace --stats` run of this script with --trace-run (eager steps, no timing), kept under "kernels" of the same
file, with the bytes each moves (kernel_bytes below) over its time, by whoever ran it."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP = 45


POLICY = "color,translation,cutout"


def make_trainer(workload, on):
    import bench
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    args = bench.make_args(workload, "cuda")
    args.diff_augment = POLICY if on else ""
    dec, enc = Decoder(args), Encoder(args)
    g = Generator(args, dec)
    d = Discriminator(args, enc)
    return EagerTrainer(args, g, d, Adjuster(args, d, g), None), args


class Side:
    def __init__(self, workload, on, nsteps):
        import bench
        self.tr, self.args = make_trainer(workload, on)
        self.inp = bench.synthetic_inputs(self.args, "cuda", 0)
        self.b = 12 if self.args.train_adj else 1   # the Adjuster branch runs from step 11
        self.on = on
        self.n = 0

    def step(self, graph=True):
        from littlegan_amd import ops
        if self.on:   # drawn as EagerTrainer.draw_diffaug_key draws it: one tiny launch per step, (seed, key_offset) of input step n
            self.n += 1
            self.inp["diffaug_key"] = ops.dropout_key(0, (self.n << 40) + (1 << 35))
        out = (self.tr.graph_step if graph else self.tr.train_step_from_inputs)(self.b, self.inp)
        self.b += 1
        return out

    def block(self, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            self.step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k


def time_workload(workload, pairs, block):
    total = WARMUP + pairs * block
    off, on = Side(workload, False, total), Side(workload, True, total)
    on.tr.store.flat.copy_(off.tr.store.flat)   # (same seed: the same weights anyway)
    on.tr.store.bump()
    for s in (off, on):
        for _ in range(WARMUP):
            s.step()
    torch.cuda.synchronize()
    t_off, t_on = [], []
    for _ in range(pairs):
        t_off.append(off.block(block))
        t_on.append(on.block(block))
    a = off.args
    d = sum(t_on) / pairs - sum(t_off) / pairs
    return {"workload": workload, "dtype": a.mfma_dtype, "batch": a.batch_size, "policy": POLICY, "pairs": pairs,
            "steps_per_block": block, "warmup_steps": WARMUP, "off_ms_per_step": [round(t, 4) for t in t_off],
            "on_ms_per_step": [round(t, 4) for t in t_on], "on_minus_off_ms": round(d, 4),
            "on_minus_off_percent": round(100.0 * d * pairs / sum(t_off), 2), "off_spread_ms": round(max(t_off) - min(t_off), 4),
            "on_spread_ms": round(max(t_on) - min(t_on), 4), "gen_loss_on": float(on.tr.losses["gen"]), "disc_loss_on": float(on.tr.losses["disc"])}


def kernel_bytes(workload):
    """Bytes each new kernel moves per launch at the workload's shapes: the sums read the 2B-row (gen tape: B-row) image batch once,
    the element-wise pass reads and writes it once; the records and partial sums are noise beside that."""
    import bench
    a = bench.make_args(workload, "cuda")
    img = a.batch_size * (16 * a.init_dim) ** 2 * 3 * 4   # one B-row fp32 image batch
    return {"image_batch_bytes_B_rows": img, "sum_2B_rows": 2 * img, "sum_B_rows": img, "apply_2B_rows": 4 * img, "apply_B_rows": 2 * img}


def trace_run(workload, on, steps):
    """eager steps of every kind for a kernel trace (rocprofv3 --kernel-trace --stats -- python scripts/bench_diffaug.py --trace-run ...)"""
    s = Side(workload, on, steps)
    for _ in range(steps):
        s.step(graph=False)
    torch.cuda.synchronize()
    print(json.dumps({"trace_run": workload, "diff_augment": on, "steps": steps, "bytes": kernel_bytes(workload)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["c3", "c2"], default=None, help="default: both")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--block", type=int, default=30, help="steps per timed block (a multiple of 15 holds every step kind in proportion)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffaug_bench.json"))
    ap.add_argument("--trace-run", choices=["off", "on"], default=None, help="no timing: run --steps eager steps for a kernel trace")
    ap.add_argument("--steps", type=int, default=15)
    a = ap.parse_args()
    if a.pairs < 3:
        ap.error("--pairs: at least 3 (the spread of the off blocks is the yardstick)")
    wls = [a.workload] if a.workload else ["c3", "c2"]
    if a.trace_run:
        for wl in wls:
            trace_run(wl, a.trace_run == "on", a.steps)
        return
    res = []
    for wl in wls:
        r = time_workload(wl, a.pairs, a.block)
        print(json.dumps(r), flush=True)
        res.append(r)
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc.setdefault("on_vs_off", {}).update({r["workload"]: r for r in res})
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
