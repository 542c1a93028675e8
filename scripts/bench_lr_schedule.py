"""Times the training step with the learning-rate schedule on the device (lr_schedule / lr_warmup_steps; DESIGN.md §28: one more launch
per step, lgsch_step, and the Adam passes reading their rate from device memory) against the constant rate, in ONE process, and writes
profiles/lr_schedule_bench.json.
`python scripts/bench_lr_schedule.py [--workload c3|c2] [--pairs P] [--block K] [--out FILE] [--defaults LABEL=FILE ...]`: C3 = bf16,
B = 256, G + D + Adjuster; C2 = exact f32, B = 64, G + D; synthetic data (bench.synthetic_inputs).

In the mould of scripts/bench_ada.py: both trainers live in one process and start from the same weights; steps are replayed graphs
(EagerTrainer.graph_step) with the partition schedule of the benchmark; 45 warm-up steps per trainer take every step kind through its
eager step, its capture and a replay; then P pairs of K-step blocks alternate constant / scheduled, each timed with HIP events.
Reported: every block's ms per step, the mean difference scheduled - constant, and the spread (max - min) of the constant blocks — the
yardstick a difference has to exceed to mean anything.  The figures are reported, not gated.  The scheduled side is cosine with warm-up,
long enough that the rates move during every timed block.  --defaults takes JSON result lines of bench.py (label=file: the parent
commit's and this tree's, with every new key at its default) and records them beside the blocks.  Not measured: per-kernel times, world
sizes above 1, the eager (un-captured) step."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_r1 import read_defaults  # noqa: E402

WARMUP = 45
SCHEDULE = dict(lr_schedule="cosine", lr_warmup_steps=100, lr_decay_steps=100000, lr_final_ratio=0.1, lr_d=1e-4)


class Side:
    """one trainer with its own inputs and step counter; every step goes through graph_step"""

    def __init__(self, workload, kw):
        import bench
        from littlegan_amd.eager_trainer import EagerTrainer
        from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
        self.args = bench.make_args(workload, "cuda")
        for k, v in kw.items():
            setattr(self.args, k, v)
        dec, enc = Decoder(self.args), Encoder(self.args)
        g = Generator(self.args, dec)
        d = Discriminator(self.args, enc)
        self.tr = EagerTrainer(self.args, g, d, Adjuster(self.args, d, g), None)
        self.inp = bench.synthetic_inputs(self.args, "cuda", 0)
        self.b = 12 if self.args.train_adj else 1   # the Adjuster branch runs from step 11

    def run(self, n):
        for _ in range(n):
            self.tr.graph_step(self.b, self.inp)
            self.b += 1

    def block(self, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.run(k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k


def time_workload(workload, pairs, block):
    from littlegan_amd import ops
    const, sched = Side(workload, {}), Side(workload, SCHEDULE)
    sched.tr.store.flat.copy_(const.tr.store.flat)   # (same seed: the same weights anyway)
    sched.tr.store.bump()
    assert const.tr.lr_state is None and sched.tr.lr_state is not None
    for s in (const, sched):
        s.run(WARMUP)
    torch.cuda.synchronize()
    t_c, t_s = [], []
    for _ in range(pairs):
        t_c.append(const.block(block))
        t_s.append(sched.block(block))
    a = const.args
    d = sum(t_s) / pairs - sum(t_c) / pairs
    k, s, lr_g, lr_d, lr_a = ops.sched_read(sched.tr.lr_state)
    assert k == WARMUP + pairs * block   # every step, replayed ones included, advanced the counter
    return {"workload": workload, "dtype": a.mfma_dtype, "batch": a.batch_size, "schedule": SCHEDULE, "pairs": pairs, "steps_per_block": block,
            "warmup_steps": WARMUP, "constant_ms_per_step": [round(t, 4) for t in t_c], "scheduled_ms_per_step": [round(t, 4) for t in t_s],
            "scheduled_minus_constant_ms": round(d, 4), "scheduled_minus_constant_percent": round(100.0 * d * pairs / sum(t_c), 2),
            "constant_spread_ms": round(max(t_c) - min(t_c), 4), "scheduled_spread_ms": round(max(t_s) - min(t_s), 4),
            "graphs": [len(const.tr._graphs), len(sched.tr._graphs)], "state_after": {"k": k, "s": s, "lr_g": lr_g, "lr_d": lr_d, "lr_a": lr_a}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["c3", "c2"], default=None, help="default: both")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--block", type=int, default=30, help="steps per timed block (a multiple of 15 holds every step kind in proportion)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lr_schedule_bench.json"))
    ap.add_argument("--defaults", nargs="*", default=[], metavar="LABEL=FILE", help="bench.py result lines to record (parent / this tree)")
    a = ap.parse_args()
    if a.pairs < 3:
        ap.error("--pairs: at least 3 (the spread of the constant blocks is the yardstick)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_lr_schedule.py measures on the GPU: none found")
    out = {"device": torch.cuda.get_device_name(0), "workloads": []}
    for wl in ([a.workload] if a.workload else ["c3", "c2"]):
        r = time_workload(wl, a.pairs, a.block)
        print(json.dumps(r), flush=True)
        out["workloads"].append(r)
    if a.defaults:
        out["defaults_bench_py"] = read_defaults(a.defaults)
    out["not_measured"] = ["per-kernel times", "world sizes above 1", "the eager (un-captured) step"]
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
