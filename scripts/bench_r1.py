"""Times the training step with no gradient regulariser, with the gradient penalty (use_gp) and with the R1 penalty
(r1_gamma) on every step and on every 16th, in ONE process, and writes profiles/r1_bench.json.
`python scripts/bench_r1.py [--workload c3|c2] [--block 48] [--repeats 4] [--out FILE] [--defaults FILE ...]`: C3 = bf16, B = 256,
G + D + Adjuster; C2 = exact f32, B = 64, G + D.  Steps are replayed graphs (EagerTrainer.graph_step) timed with HIP events.  The four
configurations are timed in alternating blocks (off, use_gp, r1 every step, r1 every 16th, off, ...), each block a whole multiple of
16 steps so that the lazy interval is amortised exactly; the figure of a configuration is the mean of its blocks and its spread the
difference between its slowest and fastest block.  --defaults takes JSON result lines of bench.py (label=file, e.g. the parent
commit's and this tree's, two runs each) and records them beside the blocks."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("off", {}), ("use_gp", {"use_gp": True, "gp_weight": 5.0}), ("r1_interval_1", {"r1_gamma": 10.0, "r1_interval": 1}),
           ("r1_interval_16", {"r1_gamma": 10.0, "r1_interval": 16})]


class Side:
    """one trainer with its own inputs and step counter; every step goes through graph_step"""

    def __init__(self, workload, kw):
        import bench
        from littlegan_amd import ops
        from littlegan_amd.eager_trainer import EagerTrainer
        from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
        args = bench.make_args(workload, "cuda")
        args.use_partition = False   # two step kinds at most: with and without the R1 penalty
        for k, v in kw.items():
            setattr(args, k, v)
        dec, enc = Decoder(args), Encoder(args)
        g = Generator(args, dec)
        d = Discriminator(args, enc)
        self.args = args
        self.tr = EagerTrainer(args, g, d, Adjuster(args, d, g), None)
        self.inp = bench.synthetic_inputs(args, "cuda", 0)
        if kw.get("use_gp"):
            self.inp["gp_eps"] = ops.gp_draw_eps(args.batch_size, 7, 0)
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
    sides = [(name, Side(workload, kw)) for name, kw in CONFIGS]
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
        if "r1" in s.tr.losses:
            res["configs"][name]["r1"] = float(s.tr.losses["r1"])
    c = res["configs"]
    off = c["off"]["ms_per_step"]
    spread = max(v["spread_ms"] for v in c.values())
    add = {k: round(c[k]["ms_per_step"] - off, 4) for k in c if k != "off"}
    res["block_spread_ms"] = round(spread, 4)
    res["added_ms"] = add
    res["added_percent"] = {k: round(100.0 * v / off, 2) for k, v in add.items()}
    # the two expectations of the issue, as figures: R1 on every step adds no more than use_gp does (it runs a subset of its launches);
    # every 16th step costs a sixteenth of that, within the spread
    res["r1_minus_gp_ms"] = round(add["r1_interval_1"] - add["use_gp"], 4)
    res["r1_16_expected_ms"] = round(add["r1_interval_1"] / 16.0, 4)
    res["r1_16_minus_expected_ms"] = round(add["r1_interval_16"] - add["r1_interval_1"] / 16.0, 4)
    return res


def read_defaults(items):
    out = {}
    for it in items:
        label, _, path = it.partition("=")
        lines = []
        for ln in open(path):
            ln = ln.strip()
            if ln.startswith("{"):
                try:
                    r = json.loads(ln)
                except ValueError:
                    continue
                lines.append({k: r[k] for k in ("workload", "dtype", "batch", "ms_per_step", "images_per_sec", "steps", "warmup") if k in r})
        out[label] = lines
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["c3", "c2"], default=None, help="default: both")
    ap.add_argument("--block", type=int, default=48, help="steps per timed block (a multiple of 16)")
    ap.add_argument("--repeats", type=int, default=4, help="blocks per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1_bench.json"))
    ap.add_argument("--defaults", nargs="*", default=[], metavar="LABEL=FILE", help="bench.py result lines to record (parent / this tree)")
    a = ap.parse_args()
    if a.block % 16 or a.block < 16 or a.repeats < 2:
        raise SystemExit("--block must be a positive multiple of 16 and --repeats at least 2 (a spread needs two blocks)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_r1.py measures on the GPU: none found")
    out = {"device": torch.cuda.get_device_name(0), "workloads": []}
    for wl in ([a.workload] if a.workload else ["c3", "c2"]):
        r = bench_workload(wl, a.block, a.repeats)
        print(json.dumps(r), flush=True)
        out["workloads"].append(r)
    if a.defaults:
        out["defaults_bench_py"] = read_defaults(a.defaults)
    out["per_kernel_times"] = "not measured"
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
