"""Times the training step under each objective of the real / fake terms (gan_loss) in ONE process and writes
profiles/gan_loss_bench.json.
`python scripts/bench_gan_loss.py [--workload c3|c2] [--block 48] [--repeats 4] [--out FILE] [--defaults FILE ...]`: C3 = bf16, B = 256,
G + D + Adjuster; C2 = exact f32, B = 64, G + D.  Steps are replayed graphs (EagerTrainer.graph_step) timed with HIP events.  The
configurations are timed in alternating blocks (bce, logistic, hinge, lsgan, bce + use_gp, wgan + use_gp, bce, ...); the figure of a
configuration is the mean of its blocks and its spread the difference between its slowest and fastest block.  A logit-side objective
enqueues the launches of the bce step one for one (another finaliser of the heads, another loss kernel), so the expectation is a
difference inside the spread of the bce blocks; wgan needs use_gp and is compared with bce + use_gp (the penalty is then taken on the
logit: one seed kernel without the sigmoid factor, a column sum instead of the second-order kernel at the heads).  --defaults takes JSON
result lines of bench.py (label=file, e.g. the parent commit's and this tree's, two runs each) and records them beside the blocks."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GP = {"use_gp": True, "gp_weight": 5.0}
CONFIGS = [("bce", {}), ("logistic", {"gan_loss": "logistic"}), ("hinge", {"gan_loss": "hinge"}), ("lsgan", {"gan_loss": "lsgan"}),
           ("bce_use_gp", dict(GP)), ("wgan_use_gp", dict(GP, gan_loss="wgan"))]
BASE = {"logistic": "bce", "hinge": "bce", "lsgan": "bce", "wgan_use_gp": "bce_use_gp"}   # what each configuration is compared with


class Side:
    """one trainer with its own inputs and step counter; every step goes through graph_step"""

    def __init__(self, workload, kw):
        import bench
        from littlegan_amd import ops
        from littlegan_amd.eager_trainer import EagerTrainer
        from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
        args = bench.make_args(workload, "cuda")
        args.use_partition = False   # one step kind
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
        self.b = 16   # past step 10: the Adjuster branch runs where the workload has one

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
        s.run(16)   # eager, captured, then replayed
        torch.cuda.synchronize()
    blocks = {name: [] for name, _ in sides}
    for _ in range(repeats):
        for name, s in sides:
            blocks[name].append(s.timed(block))
    res = {"workload": workload, "dtype": sides[0][1].args.mfma_dtype, "batch": sides[0][1].args.batch_size, "block_steps": block,
           "repeats": repeats, "configs": {}}
    for name, s in sides:
        ms = blocks[name]
        res["configs"][name] = {"ms_per_step": round(sum(ms) / len(ms), 4), "spread_ms": round(max(ms) - min(ms), 4),
                                "blocks_ms": [round(v, 4) for v in ms], "graphs": len(s.tr._graphs),
                                "losses": {k: float(v) for k, v in s.tr.losses.items()}}
    c = res["configs"]
    res["bce_spread_ms"] = {b: c[b]["spread_ms"] for b in sorted(set(BASE.values()))}
    res["minus_base_ms"] = {k: round(c[k]["ms_per_step"] - c[b]["ms_per_step"], 4) for k, b in BASE.items()}
    res["minus_base_percent"] = {k: round(100.0 * (c[k]["ms_per_step"] - c[b]["ms_per_step"]) / c[b]["ms_per_step"], 3) for k, b in BASE.items()}
    res["inside_base_spread"] = {k: abs(res["minus_base_ms"][k]) <= c[b]["spread_ms"] for k, b in BASE.items()}
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
    ap.add_argument("--block", type=int, default=48, help="steps per timed block")
    ap.add_argument("--repeats", type=int, default=4, help="blocks per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gan_loss_bench.json"))
    ap.add_argument("--defaults", nargs="*", default=[], metavar="LABEL=FILE", help="bench.py result lines to record (parent / this tree)")
    a = ap.parse_args()
    if a.block < 1 or a.repeats < 2:
        raise SystemExit("--block must be positive and --repeats at least 2 (a spread needs two blocks)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_gan_loss.py measures on the GPU: none found")
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
