"""Times the training step with the gradient guard on (clip_norm + skip_nonfinite; DESIGN.md §30: two more launches per trained network,
lgg_sumsq_partial and lgg_finalise, one more read of the trained gradient bytes, and the Adam passes reading their scale, skip flag and
rate from device memory) against the guard off, in ONE process, and writes profiles/grad_guard_bench.json.
`python scripts/bench_grad_guard.py [--workload c3|c2] [--pairs P] [--block K] [--out FILE] [--defaults LABEL=FILE ...]`: C3 = bf16,
B = 256, G + D + Adjuster; C2 = exact f32, B = 64, G + D; synthetic data (bench.synthetic_inputs).

In the mould of scripts/bench_lr_schedule.py, whose Side it uses: both trainers live in one process and start from the same weights;
steps are replayed graphs (EagerTrainer.graph_step) with the partition schedule of the benchmark; 45 warm-up steps per trainer take every
step kind through its eager step, its capture and a replay; then P pairs of K-step blocks alternate off / guarded, each timed with HIP
events.  Reported: every block's ms per step, the mean difference guarded - off, and the spread (max - min) of the off blocks — the
yardstick a difference has to exceed to mean anything.  The figures are reported, not gated.  The guarded side clips at a threshold the
gradient norms of the synthetic step stand on both sides of, so the scale it applies is live.  --defaults takes JSON result lines of
bench.py (label=file: the parent commit's and this tree's, with every new key at its default) and records them beside the blocks.  Not
measured: per-kernel times, world sizes above 1, the eager (un-captured) step."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_lr_schedule import WARMUP, Side  # noqa: E402
from bench_r1 import read_defaults  # noqa: E402

GUARD = dict(clip_norm=1.0, skip_nonfinite=True)


def time_workload(workload, pairs, block):
    off, on = Side(workload, {}), Side(workload, GUARD)
    on.tr.store.flat.copy_(off.tr.store.flat)   # (same seed: the same weights anyway)
    on.tr.store.bump()
    assert off.tr.guard is None and on.tr.guard is not None
    for s in (off, on):
        s.run(WARMUP)
    torch.cuda.synchronize()
    t_off, t_on = [], []
    for _ in range(pairs):
        t_off.append(off.block(block))
        t_on.append(on.block(block))
    a = off.args
    d = sum(t_on) / pairs - sum(t_off) / pairs
    norms = [float(x) for x in on.tr.grad_norm_now().tolist()]
    counts = on.tr.guard_counts()
    trained = {m: e - s for m, (s, e) in ((m, on.tr.store.model_range(m)) for m in "GDA")}
    return {"workload": workload, "dtype": a.mfma_dtype, "batch": a.batch_size, "guard": GUARD, "pairs": pairs, "steps_per_block": block,
            "warmup_steps": WARMUP, "off_ms_per_step": [round(t, 4) for t in t_off], "guarded_ms_per_step": [round(t, 4) for t in t_on],
            "guarded_minus_off_ms": round(d, 4), "guarded_minus_off_percent": round(100.0 * d * pairs / sum(t_off), 2),
            "off_spread_ms": round(max(t_off) - min(t_off), 4), "guarded_spread_ms": round(max(t_on) - min(t_on), 4),
            "graphs": [len(off.tr._graphs), len(on.tr._graphs)], "weights_per_network": trained,
            "after": {"grad_norm_g_d_a": norms, "skipped_nonfinite": {m: list(counts[m]) for m in "GDA"}}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["c3", "c2"], default=None, help="default: both")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--block", type=int, default=30, help="steps per timed block (a multiple of 15 holds every step kind in proportion)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_guard_bench.json"))
    ap.add_argument("--defaults", nargs="*", default=[], metavar="LABEL=FILE", help="bench.py result lines to record (parent / this tree)")
    a = ap.parse_args()
    if a.pairs < 3:
        ap.error("--pairs: at least 3 (the spread of the off blocks is the yardstick)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_guard.py measures on the GPU: none found")
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
