"""Times the training step under diff_augment with every component always applied (p = 1: lg_diffaug_draw, no state) against the
adaptive augmentation probability (ada_target = 0.6: the gated draw and the controller's two launches per step) and
records the result in profiles/ada_bench.json.  `python scripts/bench_ada.py [--workload c3|c2] [--pairs P] [--block K] [--out FILE]`:
C3 = bf16, B = 256, G + D + Adjuster; C2 = exact f32, B = 64, G + D; synthetic data (bench.synthetic_inputs).

In the mould of scripts/bench_diffaug.py: both trainers live in ONE process and start from the same weights; steps are replayed graphs
(EagerTrainer.graph_step) with the partition schedule of the benchmark; 45 warm-up steps per trainer take every step kind through its
eager step, its capture and a replay; then P pairs of K-step blocks alternate fixed / adaptive, each timed with HIP events, a fresh key
every step on both sides.  Reported: every block's ms per step, the mean difference adaptive - fixed, and the spread (max - min) of
the fixed blocks — the yardstick a difference has to exceed to mean anything.  The adaptive side is not the same computation as the
fixed one: its p starts at 0 and moves, so fewer rows are transformed — the passes T / T^T run on every row whatever its record holds,
so the launches and the bytes are the same, which is what is timed.  The p the controller has reached is recorded with the times."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP = 45
POLICY = "color,translation,cutout"
ADA = dict(ada_target=0.6, ada_interval=4, ada_kimg=500)   # the paper's target, the defaults of the other two keys


def make_trainer(workload, adaptive):
    import bench
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    args = bench.make_args(workload, "cuda")
    args.diff_augment = POLICY
    if adaptive:
        for k, v in ADA.items():
            setattr(args, k, v)
    dec, enc = Decoder(args), Encoder(args)
    g = Generator(args, dec)
    d = Discriminator(args, enc)
    return EagerTrainer(args, g, d, Adjuster(args, d, g), None), args


class Side:
    def __init__(self, workload, adaptive):
        import bench
        self.tr, self.args = make_trainer(workload, adaptive)
        self.inp = bench.synthetic_inputs(self.args, "cuda", 0)
        self.b = 12 if self.args.train_adj else 1   # the Adjuster branch runs from step 11
        self.n = 0

    def step(self):
        from littlegan_amd import ops
        self.n += 1   # drawn as EagerTrainer.draw_diffaug_key draws it: one tiny launch per step, (seed, key_offset) of input step n
        self.inp["diffaug_key"] = ops.dropout_key(0, (self.n << 40) + (1 << 35))
        out = self.tr.graph_step(self.b, self.inp)
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
    from littlegan_amd import ops
    fixed, ada = Side(workload, False), Side(workload, True)
    ada.tr.store.flat.copy_(fixed.tr.store.flat)   # (same seed: the same weights anyway)
    ada.tr.store.bump()
    assert fixed.tr.ada is None and ada.tr.ada["target"] is not None
    for s in (fixed, ada):
        for _ in range(WARMUP):
            s.step()
    torch.cuda.synchronize()
    t_fix, t_ada = [], []
    for _ in range(pairs):
        t_fix.append(fixed.block(block))
        t_ada.append(ada.block(block))
    a = fixed.args
    d = sum(t_ada) / pairs - sum(t_fix) / pairs
    p, s, n, k = ops.ada_read(ada.tr.ada_state)
    return {"workload": workload, "dtype": a.mfma_dtype, "batch": a.batch_size, "policy": POLICY, "ada": ADA, "pairs": pairs,
            "steps_per_block": block, "warmup_steps": WARMUP, "fixed_ms_per_step": [round(t, 4) for t in t_fix],
            "adaptive_ms_per_step": [round(t, 4) for t in t_ada], "adaptive_minus_fixed_ms": round(d, 4),
            "adaptive_minus_fixed_percent": round(100.0 * d * pairs / sum(t_fix), 2), "fixed_spread_ms": round(max(t_fix) - min(t_fix), 4),
            "adaptive_spread_ms": round(max(t_ada) - min(t_ada), 4), "p_after": p, "state_after": [s, n, k], "steps_adaptive": ada.n,
            "host_mirror_steps": ada.tr._ada_steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["c3", "c2"], default=None, help="default: both")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--block", type=int, default=30, help="steps per timed block (a multiple of 15 holds every step kind in proportion)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ada_bench.json"))
    a = ap.parse_args()
    if a.pairs < 3:
        ap.error("--pairs: at least 3 (the spread of the fixed blocks is the yardstick)")
    res = []
    for wl in ([a.workload] if a.workload else ["c3", "c2"]):
        r = time_workload(wl, a.pairs, a.block)
        print(json.dumps(r), flush=True)
        res.append(r)
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc.setdefault("adaptive_vs_fixed", {}).update({r["workload"]: r for r in res})
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
