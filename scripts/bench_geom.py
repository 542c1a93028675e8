"""Times the training step with the geometric augmentation of D's inputs off and on (geom_augment) and records the
result in profiles/geom_bench.json.  `python scripts/bench_geom.py [--workload c3|c2] [--pairs P] [--block K] [--out FILE]`:
C3 = bf16, B = 256, G + D + Adjuster; C2 = exact f32, B = 64, G + D; synthetic data (bench.synthetic_inputs).

In the mould of scripts/bench_diffaug.py: the trainers live in ONE process and start from the same weights; steps are replayed graphs
(EagerTrainer.graph_step) with the partition schedule of the benchmark (K a multiple of 15 holds every step kind in proportion); the
warm-up runs 45 steps per trainer, which takes every kind through its eager step, its capture and a replay.  Three comparisons, each P
pairs of alternating off / on blocks timed with HIP events, the on trainer under a fresh key every step:
  alone     off = the default step;  on = geom_augment xflip,rot90,scale,rotate (every component on every row)
  on_top    off = diff_augment color,translation,cutout with ada_target 0.6;  on = the same plus geom_augment (the gated draw, p
            driven by the controller: rows whose gates are off take the copy path of the passes)
  on_top_p1 the same without ada_target: every component of both keys on every row (on_top measures the passes at the p the
            controller reaches on the synthetic inputs, which may be 0: then every row takes the copy path)
Reported, not gated: every block's ms per step, the mean difference on - off, and the spread (max - min) of the off blocks — the
yardstick a difference has to exceed to mean anything.  The cost depends on the records: a zoomed-in row (s > 1) has more candidate
destinations per source pixel in the adjoint's gather than a zoomed-out one.
--parent FILE merges the figures of bench.py runs of the parent commit and of this tree taken in the same visit (a JSON file
{"c3": {"parent_ms": [a, b], "this_ms": [c, d]}, "c2": ...}) under "default_keys_vs_parent": with the default keys the step enqueues
the parent's launches, and "this" has to lie within what the parent's own two runs differ by.
No per-kernel trace is taken here; --trace-run runs eager steps for one (rocprofv3 --kernel-trace --stats -- python
scripts/bench_geom.py --trace-run on), kept under "kernels" of the same file by whoever ran it (a timing run keeps what is there)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP = 45
GEOM = "xflip,rot90,scale,rotate"
DIFF = "color,translation,cutout"
MODES = {   # name -> (keys of the off side, keys of the on side)
    "alone": ({}, {"geom_augment": GEOM}),
    "on_top": ({"diff_augment": DIFF, "ada_target": 0.6}, {"diff_augment": DIFF, "ada_target": 0.6, "geom_augment": GEOM}),
    "on_top_p1": ({"diff_augment": DIFF}, {"diff_augment": DIFF, "geom_augment": GEOM}),
}


def make_trainer(workload, keys):
    import bench
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    args = bench.make_args(workload, "cuda")
    for k, v in keys.items():
        setattr(args, k, v)
    dec, enc = Decoder(args), Encoder(args)
    g = Generator(args, dec)
    d = Discriminator(args, enc)
    return EagerTrainer(args, g, d, Adjuster(args, d, g), None), args


class Side:
    def __init__(self, workload, keys):
        import bench
        self.tr, self.args = make_trainer(workload, keys)
        self.inp = bench.synthetic_inputs(self.args, "cuda", 0)
        self.b = 12 if self.args.train_adj else 1   # the Adjuster branch runs from step 11
        self.n = 0

    def step(self, graph=True):
        from littlegan_amd import ops
        if self.tr.augmenting:   # drawn as EagerTrainer.draw_diffaug_key draws it: one tiny launch per step
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


def time_mode(workload, mode, pairs, block):
    off, on = (Side(workload, keys) for keys in MODES[mode])
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
    p = on.tr.ada_p()
    return {"workload": workload, "mode": mode, "dtype": a.mfma_dtype, "batch": a.batch_size, "off_keys": MODES[mode][0],
            "on_keys": MODES[mode][1], "pairs": pairs, "steps_per_block": block, "warmup_steps": WARMUP,
            "off_ms_per_step": [round(t, 4) for t in t_off], "on_ms_per_step": [round(t, 4) for t in t_on],
            "on_minus_off_ms": round(d, 4), "on_minus_off_percent": round(100.0 * d * pairs / sum(t_off), 2),
            "off_spread_ms": round(max(t_off) - min(t_off), 4), "on_spread_ms": round(max(t_on) - min(t_on), 4),
            "p_at_end_on": None if p is None else float(p), "gen_loss_on": float(on.tr.losses["gen"]),
            "disc_loss_on": float(on.tr.losses["disc"])}


def pass_bytes(workload):
    """Bytes one pass moves at the workload's shapes, from bytes alone: it reads and writes the image batch once (the gathers of
    neighbouring threads overlap in cache); the records are noise beside that.  A step with the Adjuster branch makes four passes: Geo on
    2B rows twice (slots 0 and 1), Geo^T on B and on 2B rows; without it two; R1 adds none (the penalty reads the kept rows)."""
    import bench
    a = bench.make_args(workload, "cuda")
    img = a.batch_size * (16 * a.init_dim) ** 2 * 3 * 4   # one B-row fp32 image batch
    return {"image_batch_bytes_B_rows": img, "pass_2B_rows": 4 * img, "pass_B_rows": 2 * img}


def trace_run(workload, on, steps):
    s = Side(workload, MODES["alone"][1 if on else 0])
    for _ in range(steps):
        s.step(graph=False)
    torch.cuda.synchronize()
    print(json.dumps({"trace_run": workload, "geom_augment": on, "steps": steps, "bytes": pass_bytes(workload)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["c3", "c2"], default=None, help="default: both")
    ap.add_argument("--mode", choices=list(MODES), default=None, help="default: all three")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--block", type=int, default=30, help="steps per timed block (a multiple of 15 holds every step kind in proportion)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geom_bench.json"))
    ap.add_argument("--parent", default=None, help="JSON file with bench.py figures of the parent commit and of this tree (see the module docstring)")
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
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    if a.parent:
        with open(a.parent) as f:
            doc["default_keys_vs_parent"] = json.load(f)
    else:
        for wl in wls:
            for mode in ([a.mode] if a.mode else list(MODES)):
                r = time_mode(wl, mode, a.pairs, a.block)
                print(json.dumps(r), flush=True)
                doc.setdefault("on_vs_off", {}).setdefault(wl, {})[mode] = r
            doc.setdefault("bytes", {})[wl] = pass_bytes(wl)
        doc["kernels"] = doc.get("kernels", "no per-kernel trace taken")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
