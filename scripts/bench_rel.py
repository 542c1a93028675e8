"""Times the training step under the relativistic pairing objective and the R2 penalty (relativistic / r2_gamma) in ONE
process and writes profiles/rel_bench.json.
`python scripts/bench_rel.py [--workload c3|c2] [--block 48] [--repeats 4] [--out FILE] [--defaults LABEL=FILE ...]`: C3 = bf16, B = 256,
G + D + Adjuster; C2 = exact f32, B = 64, G + D.  Steps are replayed graphs (EagerTrainer.graph_step) timed with HIP events.  The
configurations are timed in alternating blocks (logistic, logistic + relativistic, r1 alone, r1 + r2 joint, r1 + r2 as two passes, then
the lazy interval 16 of the three penalty configurations, logistic, ...), each block a whole multiple of 16 steps so that the lazy
interval is amortised exactly; the figure of a configuration is the mean of its blocks and its spread the difference between its slowest
and fastest block.  The pairing is launch-count neutral: its figure is reported against the spread of the baseline blocks, not gated.
--defaults takes JSON result lines of bench.py (label=file, e.g. the parent commit's and this tree's, two runs each) and records them
beside the blocks.  Not measured: per-kernel times, world sizes above 1."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_r1 import read_defaults  # noqa: E402

LOGISTIC = {"gan_loss": "logistic"}
REL = dict(LOGISTIC, relativistic=True)
# (name, keys, joint pass?) — the penalties ride on the published recipe's objective
CONFIGS = [("logistic", LOGISTIC, True), ("relativistic", REL, True)]
for _iv in (1, 16):
    CONFIGS += [(f"r1_interval_{_iv}", dict(REL, r1_gamma=10.0, r1_interval=_iv), True),
                (f"r1_r2_joint_interval_{_iv}", dict(REL, r1_gamma=10.0, r2_gamma=10.0, r1_interval=_iv), True),
                (f"r1_r2_two_passes_interval_{_iv}", dict(REL, r1_gamma=10.0, r2_gamma=10.0, r1_interval=_iv), False)]


class Side:
    """one trainer with its own inputs and step counter; every step goes through graph_step"""

    def __init__(self, workload, kw, joint):
        import bench
        from littlegan_amd.eager_trainer import EagerTrainer
        from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
        args = bench.make_args(workload, "cuda")
        args.use_partition = False   # two step kinds at most: with and without the penalties
        for k, v in kw.items():
            setattr(args, k, v)
        dec, enc = Decoder(args), Encoder(args)
        g = Generator(args, dec)
        d = Discriminator(args, enc)
        self.args = args
        self.tr = EagerTrainer(args, g, d, Adjuster(args, d, g), None)
        self.tr.r12_joint = joint
        self.inp = bench.synthetic_inputs(args, "cuda", 0)
        self.b = 16   # past step 10: the Adjuster branch runs where the workload has one; a multiple of 16: a penalty step first

    def run(self, n):
        for _ in range(n):
            self.tr.graph_step(self.b, self.inp)
            self.b += 1

    def timed(self, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.run(n)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n


def bench_workload(workload, block, repeats):
    sides = [(name, Side(workload, kw, joint)) for name, kw, joint in CONFIGS]
    for _, s in sides:
        s.run(48)   # three penalty steps at interval 16: eager, captured, replayed; every other kind long since replayed
        torch.cuda.synchronize()
        assert s.b % 16 == 0
    blocks = {name: [] for name, _ in sides}
    for _ in range(repeats):
        for name, s in sides:
            blocks[name].append(s.timed(block))
    res = {"workload": workload, "dtype": sides[0][1].args.mfma_dtype, "batch": sides[0][1].args.batch_size, "block_steps": block,
           "repeats": repeats, "configs": {}}
    for name, s in sides:
        ms = blocks[name]
        res["configs"][name] = {"ms_per_step": round(sum(ms) / len(ms), 4), "spread_ms": round(max(ms) - min(ms), 4),
                                "blocks_ms": [round(v, 4) for v in ms], "graphs": len(s.tr._graphs)}
        for k in ("r1", "r2"):
            if k in s.tr.losses:
                res["configs"][name][k] = float(s.tr.losses[k])
    c = res["configs"]
    base = c["logistic"]["ms_per_step"]
    res["baseline_spread_ms"] = c["logistic"]["spread_ms"]
    res["block_spread_ms"] = round(max(v["spread_ms"] for v in c.values()), 4)
    res["relativistic_minus_logistic_ms"] = round(c["relativistic"]["ms_per_step"] - base, 4)
    rel = c["relativistic"]["ms_per_step"]
    res["added_ms_over_relativistic"] = {k: round(v["ms_per_step"] - rel, 4) for k, v in c.items() if k.startswith("r1_")}
    for iv in (1, 16):
        j, t = c[f"r1_r2_joint_interval_{iv}"]["ms_per_step"], c[f"r1_r2_two_passes_interval_{iv}"]["ms_per_step"]
        res[f"joint_minus_two_passes_ms_interval_{iv}"] = round(j - t, 4)
    # the decision of DESIGN.md §27: the joint pass is the product path unless it is slower than two passes by more than the spread
    res["joint_is_slower_beyond_spread"] = bool(res["joint_minus_two_passes_ms_interval_1"] > res["block_spread_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["c3", "c2"], default=None, help="default: both")
    ap.add_argument("--block", type=int, default=48, help="steps per timed block (a multiple of 16)")
    ap.add_argument("--repeats", type=int, default=4, help="blocks per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rel_bench.json"))
    ap.add_argument("--defaults", nargs="*", default=[], metavar="LABEL=FILE", help="bench.py result lines to record (parent / this tree)")
    a = ap.parse_args()
    if a.block % 16 or a.block < 16 or a.repeats < 2:
        raise SystemExit("--block must be a positive multiple of 16 and --repeats at least 2 (a spread needs two blocks)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_rel.py measures on the GPU: none found")
    out = {"device": torch.cuda.get_device_name(0), "workloads": []}
    for wl in ([a.workload] if a.workload else ["c3", "c2"]):
        r = bench_workload(wl, a.block, a.repeats)
        print(json.dumps(r), flush=True)
        out["workloads"].append(r)
    if a.defaults:
        out["defaults_bench_py"] = read_defaults(a.defaults)
    out["not_measured"] = ["per-kernel times", "world sizes above 1"]
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
