"""Per-level A/B of the Adjuster's fused forward on the C3 step's shapes, both routes in one process, interleaved:

  decoder level L (2B = 512 samples; skip = [own rows ; rows handed over by D], B each)
      two-pass : apply + skip, one launch per skip part (moments finished inside the launch), then the plain transposed conv
      fused    : the stand-alone finalize, then the conv that forms norm + LeakyReLU + skip while it stages its halo
                 (own part of the skip RAW, as the encoder hands it over; the other part a stored map)
  encoder level L (B = 256, the Adjuster's own pass)
      two-pass : apply (moments finished inside), then the plain conv
      fused    : the stand-alone finalize, then the normalising conv
  the apply pass with a stored and with a raw skip part (same bytes moved)

Each figure is the mean of N back-to-back launches of the whole route between two events; R interleaved repetitions per route; the JSON
line holds every repetition.  usage: python scripts/bench_adj_fused.py [out.json] [--batch 256] [--reps 9] [--n 20]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from littlegan_amd import ops  # noqa: E402

A, BF16 = 0.3, 1


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3   # us


def ab(routes, reps, n):
    for _ in range(2):   # two whole untimed rounds: the first timed round otherwise carries the clock ramp (seen: +20 % on every route)
        for fn in routes.values():
            timed(fn, n)
    runs = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            runs[k].append(round(timed(fn, n), 2))
    return runs


def rnd16(*shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, device="cuda") * scale + shift).to(torch.bfloat16)


def vec(*v):
    return torch.tensor(v, dtype=torch.float32, device="cuda")


def producer_moments(shape, gm, bt):
    """raw z of a level as its producing conv leaves it: bf16 map + moment partials (private copy of the workspace records)"""
    B, H, W, C = shape
    cs = 2 * C
    x16 = rnd16(B, H // 2, W // 2, cs)
    pack = ops.conv_pack(torch.randn(5, 5, C, cs, device="cuda") * 0.03, C, cs, BF16)
    z, mom = ops.convT_s2_fwd_stats(None, pack, torch.zeros(C, device="cuda"), C, BF16, gm, bt, x16=x16, z16=True, defer_stats=True)
    ws = mom.ws[:B * mom.nparts * 24].clone()
    return z, (lambda: ops.Moments(ws, mom.nparts, gm, bt, B))


def decoder_level(B, H, C, reps, n):
    """map [2B, H, H, C] -> transposed conv C -> C / 2"""
    gm, bt = vec(1.1), vec(0.05)
    z, moments = producer_moments((2 * B, H, H, C), gm, bt)
    raw_z = rnd16(B, H, H, C, shift=0.2)
    raw = ops.Raw(raw_z, ops.instnorm_stats(raw_z.float(), gm, bt, 0, A))
    own_map, tail_map = torch.empty_like(raw_z), rnd16(B, H, H, C)
    ops.instnorm_apply(raw.z, raw.stats, None, 0, 1, A, out16=own_map, want_f32=False)
    cb = C // 2
    pack = ops.conv_pack(torch.randn(5, 5, cb, C, device="cuda") * 0.03, cb, C, BF16)
    bias = torch.zeros(cb, device="cuda")
    h16 = torch.empty_like(z)

    def apply_parts(first):
        mom = moments()
        ops.instnorm_apply(z[:B], mom[:B], first, 0, 1, A, out16=h16[:B], want_f32=False)
        ops.instnorm_apply(z[B:], mom[B:], tail_map, 0, 1, A, out16=h16[B:], want_f32=False)

    def two_pass():
        apply_parts(own_map)
        return ops.convT_s2_fwd_stats(None, pack, bias, cb, BF16, gm, bt, x16=h16, z16=True, defer_stats=True)

    def fused():
        st = ops.stats_tensor(moments())
        return ops.convT_s2_fwd_stats_ns(z, st, A, (raw, tail_map), pack, bias, cb, BF16, gm, bt, defer_stats=True)

    assert ops.convT_s2_fwd_ns_supported(2 * B, H, H, cb, C, BF16)
    assert torch.equal(two_pass()[0], fused()[0])
    kernel = ops.last_kernel()
    out = ab({"two_pass": two_pass, "fused": fused, "apply_stored_skip": lambda: apply_parts(own_map), "apply_raw_skip": lambda: apply_parts(raw)},
             reps, n)
    out["conv_kernel"] = kernel
    return out


def encoder_level(B, H, C, reps, n):
    """map [B, H, H, C] -> conv C -> 2C"""
    gm, bt = vec(1.1), vec(0.05)
    z, moments = producer_moments((B, H, H, C), gm, bt)
    cs = 2 * C
    pack = ops.conv_pack(torch.randn(5, 5, C, cs, device="cuda") * 0.03, C, cs, BF16)
    bias = torch.zeros(cs, device="cuda")
    h16 = torch.empty_like(z)

    def two_pass():
        ops.instnorm_apply(z, moments(), None, 0, 1, A, out16=h16, want_f32=False)
        return ops.conv2d_s2_fwd_stats(None, pack, bias, cs, BF16, gm, bt, x16=h16, z16=True, alpha=A, defer_stats=True)

    def fused():
        return ops.conv2d_s2_fwd_stats_zn(z, ops.stats_tensor(moments()), A, pack, bias, cs, BF16, gm, bt)

    assert ops.conv2d_s2_fwd_stats_zn_supported(B, H, H, C, cs, BF16)
    assert torch.equal(two_pass()[0], fused()[0])
    return ab({"two_pass": two_pass, "fused": fused}, reps, n)


def summary(runs):
    out = {}
    for k, v in runs.items():
        if isinstance(v, list):
            out[k] = {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v), "runs_us": v}
        else:
            out[k] = v
    if "two_pass" in out and "fused" in out:
        spread = max(out[r]["max_us"] - out[r]["min_us"] for r in ("two_pass", "fused"))
        out["gain_us"] = round(out["two_pass"]["median_us"] - out["fused"]["median_us"], 2)
        out["spread_us"] = round(spread, 2)
        out["every_fused_run_faster"] = out["fused"]["max_us"] < out["two_pass"]["min_us"]
    return out


def main():
    B, reps, n = arg("--batch", 256), arg("--reps", 9), arg("--n", 20)
    torch.manual_seed(0)
    res = {"batch": B, "reps": reps, "launches_per_rep": n, "device": torch.cuda.get_device_name(0)}
    res["decoder_level2_32x32x128_convT3"] = summary(decoder_level(B, 32, 128, reps, n))
    res["decoder_level3_64x64x64_convT4"] = summary(decoder_level(B, 64, 64, reps, n))
    res["encoder_level1_64x64x64_conv2"] = summary(encoder_level(B, 64, 64, reps, n))
    res["encoder_level2_32x32x128_conv3"] = summary(encoder_level(B, 32, 128, reps, n))
    line = json.dumps(res)
    print(line)
    outs = [a for a in sys.argv[1:] if a.endswith(".json")]
    if outs:
        with open(outs[0], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
