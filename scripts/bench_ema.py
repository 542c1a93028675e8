"""Times the training step with the weight average off, fused into the Adam pass (ema_decay = 0.999) and UNFUSED, and
records the result in profiles/ema_bench.json.  `python scripts/bench_ema.py [--workload c3|c2] [--pairs P] [--block K] [--out FILE]`:
C3 = bf16, B = 256, G + D + Adjuster; synthetic data (bench.synthetic_inputs).

  off     : ema_decay = 0 — the launches of the step as it was before the feature
  fused   : lg_clip_adam_ema_update per model (Adam on the trained range, the average over the model's whole range) + lg_ema_advance
  unfused : the alternative the fusion is measured against — today's lg_clip_adam_update per model, then ONE separate sweep of the
            average over the whole store (the same kernel with lo == hi: reads w and ema, writes ema) + lg_ema_advance.  It exists in
            this script only.

All three trainers live in ONE process and start from the same weights.  Steps are replayed graphs (EagerTrainer.graph_step) with the
partition schedule of the benchmark (K a multiple of 15 holds every step kind in its proportion); the warm-up runs 45 steps per
trainer, which takes every kind through its eager step, its capture and a replay.  Then P rounds of blocks alternate off / fused /
unfused (the order rotates from round to round), each block timed with HIP events.  Reported: every block's ms per step, the mean differences, and the spread (max - min) of
the off blocks — the yardstick a difference has to exceed to mean anything.  The optimizer launches of one full step (Adjuster on)
are counted on an eager step; at the end the three trainers' weights must be bit-identical and the two averages too."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP = 45
DECAY = 0.999


def make_trainer(workload, mode):
    import bench
    from littlegan_amd import ops
    from littlegan_amd.eager_trainer import ADAM_EPS, EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator

    class Unfused(EagerTrainer):
        def _apply_optimizers(self, batch_no, run_adj):
            st = self.store
            ema, st.ema = st.ema, None          # today's Adam launches ...
            try:
                super()._apply_optimizers(batch_no, run_adj)
            finally:
                st.ema = ema
            lr, b1, b2 = self.opt_cfg["G"]      # ... then the average alone over the whole store (lo == hi: no Adam argument is used)
            ops.clip_adam_ema_update(st.flat, st.grad, st.m, st.v, st.ema, 0, 0, self.opt_state["G"], st.ema_updates, lr, b1, b2,
                                     ADAM_EPS, 0.0, 1.0, self.ema_decay)
            ops.ema_advance(st.ema_updates)

    args = bench.make_args(workload, "cuda")
    args.ema_decay = 0.0 if mode == "off" else DECAY
    dec, enc = Decoder(args), Encoder(args)
    g = Generator(args, dec)
    d = Discriminator(args, enc)
    return (Unfused if mode == "unfused" else EagerTrainer)(args, g, d, Adjuster(args, d, g), None), args


class Side:
    def __init__(self, workload, mode):
        import bench
        self.mode = mode
        self.tr, self.args = make_trainer(workload, mode)
        self.inp = bench.synthetic_inputs(self.args, "cuda", 0)
        self.b = 12 if self.args.train_adj else 1   # the Adjuster branch runs from step 11

    def step(self, graph=True):
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


def optimizer_launches(side):
    """Launches of the optimizer phase of one eager full step (no partition; Adjuster on where the workload has one)."""
    from littlegan_amd import ops
    names = ("clip_adam_update", "clip_adam_ema_update", "adam_advance", "ema_advance")
    real = {n: getattr(ops, n) for n in names}
    count = dict.fromkeys(names, 0)

    def wrap(n):
        def f(*a, **k):
            count[n] += 1
            return real[n](*a, **k)
        return f
    for n in names:
        setattr(ops, n, wrap(n))
    try:
        while side.tr.step_kind(side.b)[0] != -1:
            side.step()
        side.step(graph=False)
    finally:
        for n in names:
            setattr(ops, n, real[n])
    return dict(count, total=sum(count.values()))


def time_workload(workload, pairs, block):
    modes = ("off", "fused", "unfused")
    sides = {m: Side(workload, m) for m in modes}
    for m in modes[1:]:
        sides[m].tr.store.flat.copy_(sides["off"].tr.store.flat)   # (same seed: the same weights anyway)
        sides[m].tr.store.bump()
        sides[m].tr.reset_ema()
    for s in sides.values():
        for _ in range(WARMUP):
            s.step()
    torch.cuda.synchronize()
    t = {m: [] for m in modes}
    for r in range(pairs):
        for m in modes[r % 3:] + modes[:r % 3]:   # the order rotates: no mode always runs first (or last) in its round
            t[m].append(sides[m].block(block))
    launches = {m: optimizer_launches(sides[m]) for m in modes}
    torch.cuda.synchronize()
    st = {m: sides[m].tr.store for m in modes}
    mean = {m: sum(t[m]) / pairs for m in modes}
    a = sides["off"].args
    n = st["off"].flat.numel()
    return {"workload": workload, "dtype": a.mfma_dtype, "batch": a.batch_size, "ema_decay": DECAY, "store_floats": n, "pairs": pairs,
            "steps_per_block": block, "warmup_steps": WARMUP,
            "ms_per_step": {m: [round(x, 4) for x in t[m]] for m in modes},
            "mean_ms_per_step": {m: round(mean[m], 4) for m in modes},
            "fused_minus_off_ms": round(mean["fused"] - mean["off"], 4),
            "fused_minus_off_percent": round(100.0 * (mean["fused"] - mean["off"]) / mean["off"], 3),
            "unfused_minus_off_ms": round(mean["unfused"] - mean["off"], 4),
            "unfused_minus_fused_ms": round(mean["unfused"] - mean["fused"], 4),
            "spread_ms": {m: round(max(t[m]) - min(t[m]), 4) for m in modes},
            "optimizer_launches_full_step": launches,
            "weights_bit_identical": bool(torch.equal(st["off"].flat, st["fused"].flat) and torch.equal(st["off"].flat, st["unfused"].flat)),
            "averages_bit_identical": bool(torch.equal(st["fused"].ema, st["unfused"].ema)),
            "ema_updates": int(st["fused"].ema_updates)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["c3", "c2"], default="c3")
    ap.add_argument("--pairs", type=int, default=6, help="rounds of one block per mode (a multiple of 3 gives every mode every position)")
    ap.add_argument("--block", type=int, default=30, help="steps per timed block (a multiple of 15 holds every step kind in proportion)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.json"))
    a = ap.parse_args()
    if a.pairs < 3:
        ap.error("--pairs: at least 3 (the spread of the off blocks is the yardstick)")
    r = time_workload(a.workload, a.pairs, a.block)
    print(json.dumps(r), flush=True)
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc.setdefault("off_fused_unfused", {})[r["workload"]] = r
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
