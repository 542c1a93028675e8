"""Timing of the FID activation statistics (fid.py:185-188) on synthetic Inception-sized activations [N, 2048]:
the in-tree fp64-MFMA kernel (lg_fid_stats) on the GPU, np.mean / np.cov on the host cores beside it, and the host
matrix square root of the Frechet distance (fid.py:144-163)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from littlegan_amd import ops
from littlegan_amd.fid import frechet_distance
for N in (10000, 50000):
    D = 2048
    a = torch.randn(N, D, device="cuda") * 0.5 + 0.3
    ops.fid_stats(a); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        mu, sg = ops.fid_stats(a)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 3
    fl = 2.0 * N * D * (D + 64) / 2 * 1.0  # upper-triangular tiles only
    an = a.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter(); ref = np.cov(an, rowvar=False); tc = time.perf_counter() - t0
    err = np.abs(sg.cpu().numpy() - ref).max()
    print(f"[N={N}, D={D}] lg_fid_stats {dt*1e3:.2f} ms ({fl/dt/1e12:.1f} TFLOP/s fp64, triangular) | numpy cov on {os.cpu_count()} host threads {tc*1e3:.0f} ms | max |sigma - np.cov| {err:.1e}", flush=True)
m1, s1 = mu.cpu().numpy(), sg.cpu().numpy()
t0 = time.perf_counter(); d = frechet_distance(m1, s1, m1 + 0.01, s1 * 1.01); ts = time.perf_counter() - t0
print(f"host sqrtm + trace (scipy) for D=2048: {ts:.1f} s, d^2 = {d:.4f}")

# ---- streamed statistics, the fp64 GEMM and the distance on the device; the lines below go into
# profiles/fid_device.json (--json PATH writes them)
import json
import warnings
from littlegan_amd.fid import frechet_distance_ns

results = {"device": torch.cuda.get_device_name(0)}


def _timed(fn, reps=3):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


D, N = 2048, 50000
a = torch.randn(N, D, device="cuda") * 0.5 + 0.3
t_whole = _timed(lambda: ops.fid_stats(a))
s = torch.zeros(D, dtype=torch.float64, device="cuda")
g = torch.zeros(ops.fid_gram_elems(D), dtype=torch.float64, device="cuda")
for rows in (4096, 256):
    def stream():
        s.zero_(); g.zero_()
        for r in range(0, N, rows):
            ops.fid_accum(a[r:r + rows], s, g)
        return ops.fid_finalize(s, g, N)
    t_acc = _timed(stream)
    err = (stream()[1] - ops.fid_stats(a)[1]).abs().max().item()
    rmw = 2 * g.numel() * 8 * ((N + rows - 1) // rows)
    print(f"[N={N}, D={D}] lg_fid_accum in batches of {rows}: {t_acc*1e3:.2f} ms against lg_fid_stats {t_whole*1e3:.2f} ms (ratio {t_acc/t_whole:.2f}; "
          f"read-modify-write of the Gram tiles {rmw/1e9:.2f} GB), max |sigma - lg_fid_stats| {err:.1e}", flush=True)
    results[f"accum_batch_{rows}"] = {"N": N, "D": D, "accum_ms": t_acc * 1e3, "fid_stats_ms": t_whole * 1e3, "ratio": t_acc / t_whole,
                                     "gram_rmw_gb": rmw / 1e9, "max_abs_diff_sigma": err}
del a

x, y = torch.randn(D, D, device="cuda", dtype=torch.float64), torch.randn(D, D, device="cuda", dtype=torch.float64)
t_gemm = _timed(lambda: ops.fid_gemm(x, y), reps=10)
print(f"fp64 GEMM D={D}: {t_gemm*1e3:.3f} ms, {2.0*D**3/t_gemm/1e12:.1f} TFLOP/s (one launch, 1024 tiles)", flush=True)
results["gemm"] = {"D": D, "ms": t_gemm * 1e3, "tflops": 2.0 * D ** 3 / t_gemm / 1e12}

# covariances of ReLU-ed correlated Gaussian features rounded to fp32 (the full-rank D = 2048 fixture of tests/test_fid_stream.py)
rng = np.random.default_rng(0)
W = rng.standard_normal((D, D)) * (np.arange(1, D + 1) ** -0.7)[None, :] * (4 / np.sqrt(D))
fa = np.maximum(rng.standard_normal((10000, D)) @ W.T + 0.3, 0).astype(np.float32).astype(np.float64)
fb = np.maximum(rng.standard_normal((10000, D)) @ (1.1 * W.T) + 0.35, 0).astype(np.float32).astype(np.float64)
mu1, S1, mu2, S2 = fa.mean(0), np.cov(fa, rowvar=False), fb.mean(0), np.cov(fb, rowvar=False)
dev = [torch.from_numpy(v).cuda() for v in (mu1, S1, mu2, S2)]
ops.fid_distance(*dev)
t0 = time.perf_counter(); d2, tr, iters, status = ops.fid_distance(*dev); t_dev = time.perf_counter() - t0
t0 = time.perf_counter(); d2p, info = frechet_distance_ns(mu1, S1, mu2, S2, device="cuda"); t_pub = time.perf_counter() - t0
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    t0 = time.perf_counter(); d_host = frechet_distance(mu1, S1, mu2, S2); t_host = time.perf_counter() - t0
print(f"lg_fid_distance D={D}: {t_dev*1e3:.1f} ms ({iters} iterations, status {status}, 3 launches + 1 copy back per iteration; "
      f"{3*2.0*D**3*iters/t_dev/1e12:.1f} TFLOP/s over the call; {t_pub*1e3:.1f} ms through frechet_distance_ns from host arrays) | "
      f"scipy sqrtm path on {os.cpu_count()} host threads, same statistics, same run: {t_host:.2f} s = {t_host/t_dev:.0f} x | "
      f"d^2 {d2:.9f} against {d_host:.9f}", flush=True)
results["distance"] = {"D": D, "device_ms": t_dev * 1e3, "public_entry_ms": t_pub * 1e3, "iterations": iters, "status": status,
                       "launches_per_iteration": 3, "scipy_s": t_host, "speedup": t_host / t_dev, "d2_device": d2, "d2_scipy": d_host}
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(results, f, indent=1)
