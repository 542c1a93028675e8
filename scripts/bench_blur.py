"""Times the training step with the blur of D's inputs off and live (blur_init_sigma), and lgblur_apply alone, and records
the result in profiles/blur_bench.json.  `python scripts/bench_blur.py [--workload c3|c2] [--pairs P] [--block K] [--out FILE]`:
C3 = bf16, B = 256, G + D + Adjuster; C2 = exact f32, B = 64, G + D; synthetic data (bench.synthetic_inputs).

In the mould of scripts/bench_geom.py: the trainers live in ONE process and start from the same weights; steps are replayed graphs
(EagerTrainer.graph_step) with the partition schedule of the benchmark (K a multiple of 15 holds every step kind in proportion); the
warm-up runs 45 steps per trainer, which takes every kind through its eager step, its capture and a replay.  Two comparisons per
workload, each P pairs of alternating off / on blocks timed with HIP events:
  r3     off = the default step;  on = blur_init_sigma 1 (R = 3, 7 taps a pass)
  r30    off = the default step;  on = blur_init_sigma 10 (R = 30, 61 taps a pass: the largest filter there is)
A fade moves sigma every step, and with it R; to time ONE radius the on side puts its counter back to 0 before every step (the host
mirror, and the device state by one lgblur_init launch: a tiny launch per step, as the key draw of bench_geom.py is), so every step runs
at sigma = blur_init_sigma.
Reported, not gated: every block's ms per step, the mean difference on - off, and the spread (max - min) of the off blocks — the
yardstick a difference has to exceed to mean anything.
--apply times lgblur_apply alone at 2B = 512 rows, S = 128 under sigma 0.2 / 1 / 4 / 10 (R = 0, 3, 12, 30) and, in the same process,
lgeo_fwd on identity records — a plain copy of the same bytes — as the yardstick for how far each case is from a copy: HIP events around
REPS back-to-back launches after a warm-up, ms per launch and achieved GB/s (the bytes the operator needs: the batch read once and
written once).
--parent FILE merges the figures of bench.py runs of the parent commit and of this tree taken in the same visit (a JSON file
{"c3": {"parent_ms": [a, b], "this_ms": [c, d]}, "c2": ...}) under "default_keys_vs_parent": with the keys at their defaults the step
enqueues the parent's launches, and "this" has to lie within what the parent's own two runs differ by.
No per-kernel counters are taken and no world size above 1 is measured."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP = 45
REPS = 50
MODES = {"r3": 1.0, "r30": 10.0}   # name -> blur_init_sigma of the on side
APPLY_SIGMAS = (0.2, 1.0, 4.0, 10.0)


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

    def step(self):
        from littlegan_amd import ops
        if self.tr.blur is not None:   # every step at k = 0: sigma = blur_init_sigma, one radius for the whole run
            self.tr._blur_k = 0
            ops.blur_init(0, out=self.tr.blur_state)
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


def time_mode(workload, mode, pairs, block):
    from littlegan_amd import config, ops
    on_keys = {"blur_init_sigma": MODES[mode]}
    off, on = Side(workload, {}), Side(workload, on_keys)
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
    sigma = ops.blur_read(on.tr.blur_state)[1]
    return {"workload": workload, "mode": mode, "dtype": a.mfma_dtype, "batch": a.batch_size, "on_keys": on_keys, "pairs": pairs,
            "steps_per_block": block, "warmup_steps": WARMUP, "sigma_on": sigma, "radius_on": config.blur_radius(sigma),
            "off_ms_per_step": [round(t, 4) for t in t_off], "on_ms_per_step": [round(t, 4) for t in t_on],
            "on_minus_off_ms": round(d, 4), "on_minus_off_percent": round(100.0 * d * pairs / sum(t_off), 2),
            "off_spread_ms": round(max(t_off) - min(t_off), 4), "on_spread_ms": round(max(t_on) - min(t_on), 4),
            "gen_loss_on": float(on.tr.losses["gen"]), "disc_loss_on": float(on.tr.losses["disc"])}


def time_launches(fn, reps=REPS):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def time_apply(rows=512, S=128):
    """ms per launch and GB/s of lgblur_apply per radius, and of lgeo_fwd on identity records (a plain copy), three rounds alternating"""
    from littlegan_amd import config, ops
    x = torch.rand(rows, S, S, 3, device="cuda") * 2 - 1
    out = torch.empty_like(x)
    ident = torch.tensor([1.0, 0.0, 0.0, 1.0], device="cuda").repeat(rows, 1).contiguous()
    nbytes = 2 * x.numel() * 4
    states = {}
    for sigma in APPLY_SIGMAS:
        st = ops.blur_init(0)
        ops.blur_step(st, sigma, 1, 1 << 40)
        states[sigma] = st
    res = {"rows": rows, "S": S, "bytes_read_plus_written": nbytes, "launches_per_timing": REPS, "copy_lgeo_fwd_identity_ms": [],
           "dblur_apply": {f"R{config.blur_radius(s)}": {"sigma": s, "ms": []} for s in APPLY_SIGMAS}}
    for _ in range(3):
        res["copy_lgeo_fwd_identity_ms"].append(round(time_launches(lambda: ops.geom_fwd(x, ident, out=out)), 5))
        for sigma, st in states.items():
            res["dblur_apply"][f"R{config.blur_radius(sigma)}"]["ms"].append(round(time_launches(lambda: ops.blur_apply(x, st, out=out)), 5))
    gbs = lambda ms: round(nbytes / (min(ms) * 1e-3) / 1e9, 1)
    res["copy_lgeo_fwd_identity_gbs"] = gbs(res["copy_lgeo_fwd_identity_ms"])
    for v in res["dblur_apply"].values():
        v["gbs"] = gbs(v["ms"])
        v["times_the_copy"] = round(min(v["ms"]) / min(res["copy_lgeo_fwd_identity_ms"]), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["c3", "c2"], default=None, help="default: both")
    ap.add_argument("--mode", choices=list(MODES), default=None, help="default: both")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--block", type=int, default=30, help="steps per timed block (a multiple of 15 holds every step kind in proportion)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blur_bench.json"))
    ap.add_argument("--apply", action="store_true", help="time lgblur_apply alone against a copy instead of whole steps")
    ap.add_argument("--parent", default=None, help="JSON file with bench.py figures of the parent commit and of this tree (see the module docstring)")
    a = ap.parse_args()
    if a.pairs < 3:
        ap.error("--pairs: at least 3 (the spread of the off blocks is the yardstick)")
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    if a.parent:
        with open(a.parent) as f:
            doc["default_keys_vs_parent"] = json.load(f)
    elif a.apply:
        doc["apply"] = time_apply()
        print(json.dumps(doc["apply"]), flush=True)
    else:
        for wl in [a.workload] if a.workload else ["c3", "c2"]:
            for mode in ([a.mode] if a.mode else list(MODES)):
                r = time_mode(wl, mode, a.pairs, a.block)
                print(json.dumps(r), flush=True)
                doc.setdefault("on_vs_off", {}).setdefault(wl, {})[mode] = r
    doc["not_measured"] = "per-kernel counters; world sizes above 1"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
