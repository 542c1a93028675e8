"""Timing of the sample metrics of littlegan_amd/metrics.py on synthetic Inception-sized activations, N = M = 30000,
D = 2048: full-set KID, 100 x 1000 subset KID, precision / recall / density / coverage at k = 3 and each pair kernel alone, as the
median of repeated runs.  Two yardsticks are measured in the same process: lg_fid_gemm at D = 2048 (the existing kernel with the same
MFMA work per 64 x 64 tile) and the same metrics written with torch fp64 on the device (matmul and topk in row blocks: what a user
does without csrc/pairs.hip).  --json PATH writes the numbers (profiles/metrics_bench.json); --n N / --reps R shrink the run."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from littlegan_amd import metrics, ops


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


N = M = _arg("--n", 30000)
D = _arg("--d", 2048)
REPS = _arg("--reps", 3)
K = 3
BLOCK = 4096   # rows per block of the torch versions: a [4096, 30000] fp64 block is 0.98 GB


def timed(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


g = torch.Generator(device="cuda").manual_seed(0)
P = torch.randn(16, D, device="cuda", generator=g) / 2
real = (torch.randn(N, 16, device="cuda", generator=g) @ P + 0.05 * torch.randn(N, D, device="cuda", generator=g)).contiguous()
fake = ((0.7 * torch.randn(M, 16, device="cuda", generator=g) + 0.5) @ P + 0.05 * torch.randn(M, D, device="cuda", generator=g)).contiguous()
pass_flop = 2.0 * N * M * D
results = {"device": torch.cuda.get_device_name(0), "N": N, "M": M, "D": D, "k": K, "reps": REPS,
           "workspace_bytes": ops.pairs_workspace_bytes(N, M, D)}


# ---- yardstick 1: the fp64 GEMM of the FID pass, two runs of the same code to see how much such runs differ
x, y = torch.randn(2048, 2048, device="cuda", dtype=torch.float64), torch.randn(2048, 2048, device="cuda", dtype=torch.float64)
gemm = [2.0 * 2048 ** 3 / timed(lambda: ops.fid_gemm(x, y), reps=10) / 1e12 for _ in range(2)]
results["fid_gemm_tflops"] = gemm
print(f"lg_fid_gemm D=2048: {gemm[0]:.1f} / {gemm[1]:.1f} TFLOP/s (two runs)", flush=True)
del x, y

# ---- each kernel alone
sums = torch.zeros(2, dtype=torch.float64, device="cuda")
best = torch.full((N, K + 1), float("inf"), dtype=torch.float64, device="cuda")
count = torch.zeros(N, dtype=torch.int32, device="cuda")
radius2 = torch.full((M,), 1.0, dtype=torch.float64, device="cuda")
for name, fn in (("poly_sum", lambda: ops.pairs_poly_sum(real, fake, sums)),
                 ("knn", lambda: ops.pairs_knn(real, fake, best.fill_(float("inf")))),
                 ("ball_count", lambda: ops.pairs_ball_count(real, fake, radius2, count))):
    runs = [timed(fn) for _ in range(2)]
    results[name] = {"ms": [t * 1e3 for t in runs], "tflops": [pass_flop / t / 1e12 for t in runs],
                     "ratio_to_fid_gemm": pass_flop / min(runs) / 1e12 / max(gemm)}
    print(f"lg_pairs_{name} [{N} x {M} x {D}]: {runs[0]*1e3:.1f} / {runs[1]*1e3:.1f} ms, {pass_flop/runs[0]/1e12:.1f} / "
          f"{pass_flop/runs[1]/1e12:.1f} TFLOP/s, {results[name]['ratio_to_fid_gemm']:.2f} x lg_fid_gemm", flush=True)


# ---- yardstick 2: the same metrics with torch fp64 on the device
def torch_poly_sums(a, b, diag):
    a64 = a.double()
    s, tr = 0.0, 0.0
    for r in range(0, b.shape[0], BLOCK):
        k = (a64 @ b[r:r + BLOCK].double().t() / a.shape[1] + 1.0) ** 3
        s = s + k.sum()
        if diag:
            tr = tr + k[r:r + BLOCK].diagonal().sum()
    return s, tr


def torch_mmd2(a, b):
    n, m = a.shape[0], b.shape[0]
    sxx, txx = torch_poly_sums(a, a, True)
    syy, tyy = torch_poly_sums(b, b, True)
    sxy, _ = torch_poly_sums(a, b, False)
    return float((sxx - txx) / (n * (n - 1.0)) + (syy - tyy) / (m * (m - 1.0)) - 2.0 * sxy / (float(n) * m))


def torch_kid_subsets(a, b, subsets=100, size=1000, seed=0):
    vals = []
    for ir, jf in metrics.kid_subset_indices(a.shape[0], b.shape[0], subsets, size, seed):
        vals.append(torch_mmd2(a[torch.from_numpy(ir).cuda()], b[torch.from_numpy(jf).cuda()]))
    return float(np.mean(vals))


def torch_d2_blocks(a, b):
    """yields (row range, [rows, m] squared distances) in the GEMM form"""
    b64 = b.double()
    nb = (b64 * b64).sum(1)
    for r in range(0, a.shape[0], BLOCK):
        a64 = a[r:r + BLOCK].double()
        yield r, ((a64 * a64).sum(1)[:, None] + nb[None, :] - 2.0 * (a64 @ b64.t())).clamp_(min=0.0)


def torch_prdc(a, b, k=K):
    r_real = torch.cat([d.topk(k + 1, dim=1, largest=False).values[:, k] for _, d in torch_d2_blocks(a, a)])
    r_fake = torch.cat([d.topk(k + 1, dim=1, largest=False).values[:, k] for _, d in torch_d2_blocks(b, b)])
    count_fake = torch.zeros(b.shape[0], dtype=torch.int64, device="cuda")
    rec = cov = 0
    for r, d in torch_d2_blocks(a, b):               # [real block, fake]
        count_fake += (d <= r_real[r:r + d.shape[0], None]).sum(0)
        rec += int(((d <= r_fake[None, :]).sum(1) > 0).sum())
        cov += int((d.min(1).values <= r_real[r:r + d.shape[0]]).sum())
    return {"precision": float((count_fake > 0).sum()) / b.shape[0], "recall": rec / a.shape[0],
            "density": float(count_fake.sum()) / (k * b.shape[0]), "coverage": cov / a.shape[0]}


subset_size = min(1000, N)
for name, ours, theirs, flop in (
        ("kid_full", lambda: metrics.kid_from_activations(real, fake, subsets=0)["kid"], lambda: torch_mmd2(real, fake), 3 * pass_flop),
        ("kid_100x1000", lambda: metrics.kid_from_activations(real, fake, subsets=100, subset_size=subset_size)["kid"],
         lambda: torch_kid_subsets(real, fake, 100, subset_size), 100 * 3 * 2.0 * subset_size ** 2 * D),
        ("prdc_k3", lambda: metrics.prdc_from_activations(real, fake, k=K), lambda: torch_prdc(real, fake), 5 * pass_flop)):
    t_ours, t_torch = timed(ours), timed(theirs)
    v_ours, v_torch = ours(), theirs()
    results[name] = {"ms": t_ours * 1e3, "tflops": flop / t_ours / 1e12, "torch_fp64_ms": t_torch * 1e3, "speedup_over_torch": t_torch / t_ours,
                     "ratio_to_fid_gemm": flop / t_ours / 1e12 / max(gemm), "value": v_ours, "torch_value": v_torch}
    print(f"{name}: {t_ours*1e3:.1f} ms ({flop/t_ours/1e12:.1f} TFLOP/s, {results[name]['ratio_to_fid_gemm']:.2f} x lg_fid_gemm) | torch fp64 "
          f"{t_torch*1e3:.1f} ms = {t_torch/t_ours:.2f} x | {v_ours} against {v_torch}", flush=True)
results["torch_peak_bytes"] = torch.cuda.max_memory_allocated()

if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(results, f, indent=1)
