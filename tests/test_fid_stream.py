"""Streaming, mergeable FID statistics (ActivationAccumulator, iter_activation_chunks) and the Newton-Schulz Fréchet distance
(frechet_distance_ns) on the host path: torch / numpy float64 restatements of what lg_fid_accum, lg_fid_finalize and lg_fid_distance
compute on the device (tests/test_fid_stream_gpu.py).  The reference of tr sqrt(S1 S2) is sum sqrt(eigvalsh(R S2 R)), R = sqrt(S1) by
eigh: exact up to rounding for PSD input and independent of both scipy's sqrtm and the iteration under test."""
import os
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture(D, N, seed):
    """covariances of ReLU-ed correlated Gaussian features rounded to fp32 (N < D: rank-deficient)"""
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((D, D)) * (np.arange(1, D + 1) ** -0.7)[None, :] * (4 / np.sqrt(D))
    a = np.maximum(rng.standard_normal((N, D)) @ W.T + 0.3, 0).astype(np.float32)
    b = np.maximum(rng.standard_normal((N, D)) @ (1.1 * W.T) + 0.35, 0).astype(np.float32)
    S1, S2 = np.cov(a.astype(np.float64), rowvar=False), np.cov(b.astype(np.float64), rowvar=False)
    return a.astype(np.float64).mean(0), S1, b.astype(np.float64).mean(0), S2


def eigh_reference(mu1, S1, mu2, S2):
    """d2 with tr sqrt(S1 S2) = sum sqrt(eig(R S2 R)), R = sqrt(S1) (S1 S2 is similar to the PSD matrix R S2 R)"""
    w, v = np.linalg.eigh(S1)
    R = (v * np.sqrt(np.clip(w, 0, None))) @ v.T
    M = R @ S2 @ R
    tr = np.sqrt(np.clip(np.linalg.eigvalsh((M + M.T) / 2), 0, None)).sum()
    d = mu1 - mu2
    return float(d @ d + np.trace(S1) + np.trace(S2) - 2 * tr), float(tr)


def check_stats(mu, sigma, a64):
    """the tolerance of tests/test_fid.py::test_in_tree_covariance_kernel_matches_numpy"""
    ref = np.cov(a64, rowvar=False)
    e_mu, e_s = np.abs(mu - a64.mean(0)).max(), np.abs(sigma - ref).max()
    print(f"|mu - mean|max {e_mu:.2e}  |sigma - cov|max {e_s:.2e}  |cov|max {np.abs(ref).max():.2e}")
    assert e_mu < 1e-12
    assert e_s < 1e-10 * max(1.0, np.abs(ref).max())
    assert np.array_equal(sigma, sigma.T)


def _feed(acc, a, chunk):
    for r in range(0, a.shape[0], chunk):
        acc.update(torch.from_numpy(a[r:r + chunk]))
    return acc


@pytest.mark.parametrize("chunk", [1, 33, 1000])
@pytest.mark.parametrize("shifted", [False, True])
def test_accumulator_chunked_equals_whole(chunk, shifted):
    from littlegan_amd.fid import ActivationAccumulator
    rng = np.random.default_rng(11)
    a = (rng.standard_normal((257, 70)) * 3.0 + 1.5).astype(np.float32)   # D not a multiple of the 64-wide tile
    shift = rng.standard_normal(70) + 1.5 if shifted else None
    acc = _feed(ActivationAccumulator(70, "cpu", shift), a, chunk)
    assert acc.count == 257
    check_stats(*acc.finalize(), a.astype(np.float64))


def test_shift_rescues_a_mean_far_from_zero():
    """mean = 1e4 std: the uncentred form (shift 0) loses about log10(mean^2 / var) = 8 of 16 digits and may miss the tolerance;
    with shift = mean it holds.  Only the shifted case is asserted."""
    from littlegan_amd.fid import ActivationAccumulator
    rng = np.random.default_rng(12)
    a = (rng.standard_normal((500, 24)) * 1e-2 + 1e2).astype(np.float32)
    a64 = a.astype(np.float64)
    mu0, s0 = _feed(ActivationAccumulator(24, "cpu"), a, 64).finalize()
    print("shift 0: |sigma - cov|max", np.abs(s0 - np.cov(a64, rowvar=False)).max())
    check_stats(*_feed(ActivationAccumulator(24, "cpu", a64.mean(0)), a, 64).finalize(), a64)


def test_merge_of_two_halves_and_error_cases():
    from littlegan_amd.fid import ActivationAccumulator
    rng = np.random.default_rng(13)
    a = (rng.standard_normal((300, 130)) * 2.0 - 0.5).astype(np.float32)
    shift = np.full(130, -0.4)
    one = _feed(ActivationAccumulator(130, "cpu", shift), a, 50)
    h1 = _feed(ActivationAccumulator(130, "cpu", shift), a[:140], 50)
    h2 = _feed(ActivationAccumulator(130, "cpu", shift), a[140:], 33)
    h1.merge(h2)
    assert h1.count == 300
    mu, sigma = h1.finalize()
    check_stats(mu, sigma, a.astype(np.float64))
    mu1, sigma1 = one.finalize()
    assert np.abs(mu - mu1).max() < 1e-12 and np.abs(sigma - sigma1).max() < 1e-10 * max(1.0, np.abs(sigma1).max())
    with pytest.raises(ValueError):
        ActivationAccumulator(8, "cpu").finalize()                                    # no samples
    with pytest.raises(ValueError):
        ActivationAccumulator(8, "cpu").update(torch.zeros(1, 8)).finalize()          # one sample
    with pytest.raises(ValueError):
        ActivationAccumulator(8, "cpu").update(torch.zeros(4, 9))                     # D mismatch
    with pytest.raises(ValueError):
        ActivationAccumulator(8, "cpu").merge(ActivationAccumulator(9, "cpu"))        # D mismatch
    with pytest.raises(ValueError):
        ActivationAccumulator(8, "cpu", np.ones(8)).merge(ActivationAccumulator(8, "cpu"))             # shift against none
    with pytest.raises(ValueError):
        ActivationAccumulator(8, "cpu", np.ones(8)).merge(ActivationAccumulator(8, "cpu", np.zeros(8)))  # different shifts
    with pytest.raises(ValueError):
        ActivationAccumulator(8, "cpu", np.ones(7))


def _save_sources(tmp, a):
    np.save(os.path.join(tmp, "all.npy"), a)
    sh = os.path.join(tmp, "shards")
    os.makedirs(sh)
    for i, (s, e) in enumerate(((0, 40), (40, 41), (41, a.shape[0]))):
        np.save(os.path.join(sh, f"activations-{i:03d}.npy"), a[s:e])
    np.savez(os.path.join(tmp, "all.npz"), act=a)
    return [os.path.join(tmp, "all.npy"), sh, os.path.join(tmp, "all.npz")]


@pytest.mark.parametrize("world", [1, 2, 3])
def test_chunk_shares_cover_every_row_once(tmp_path, world):
    from littlegan_amd.fid import iter_activation_chunks
    a = np.arange(101 * 5, dtype=np.float32).reshape(101, 5)      # 101 rows: not divisible by 2 or 3
    for src in _save_sources(str(tmp_path), a):
        got = []
        for r in range(world):
            blocks = list(iter_activation_chunks(src, 16, r, world))
            assert all(b.dtype == np.float32 and b.ndim == 2 and 1 <= b.shape[0] <= 16 for b in blocks)
            got.append(np.concatenate(blocks))
        assert abs(max(len(g) for g in got) - min(len(g) for g in got)) <= 1
        assert np.array_equal(np.concatenate(got), a)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, src, D, shift, outdir, device="cpu"):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        from littlegan_amd.fid import ActivationAccumulator, iter_activation_chunks
        acc = ActivationAccumulator(D, device, shift)
        for blk in iter_activation_chunks(src, 16, rank, world):
            acc.update(torch.from_numpy(blk))
        own = acc.count
        acc.all_reduce()
        mu, sigma = acc.finalize()
        np.savez(os.path.join(outdir, f"rank_{rank}.npz"), own=own, count=acc.count, sum=acc.sum.cpu().numpy(),
                 gram=acc.gram.cpu().numpy(), mu=mu, sigma=sigma)
    finally:
        dist.destroy_process_group()


def run_ranks(target, args_of_rank, world, timeout):
    """spawn `world` rank processes, join them with a timeout and terminate exactly those on a failure"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=target, args=args_of_rank(r)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        for p in procs:
            p.join(timeout=timeout)
            assert p.exitcode == 0, f"rank process exit code {p.exitcode}"
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=20)
                if p.is_alive():
                    p.kill()


@pytest.mark.parametrize("kind", ["npy", "shards"])
def test_world2_gloo_sharded_statistics(tmp_path, kind):
    from littlegan_amd.fid import activation_statistics
    rng = np.random.default_rng(14)
    a = (rng.standard_normal((101, 70)) * 2.0 + 0.7).astype(np.float32)
    srcs = _save_sources(str(tmp_path), a)
    src = srcs[0] if kind == "npy" else srcs[1]
    shift = np.full(70, 0.5)
    port = _free_port()
    run_ranks(_rank_worker, lambda r: (r, 2, port, src, 70, shift, str(tmp_path)), 2, 240)
    r0, r1 = np.load(tmp_path / "rank_0.npz"), np.load(tmp_path / "rank_1.npz")
    assert int(r0["own"]) + int(r1["own"]) == 101 and int(r0["count"]) == int(r1["count"]) == 101
    for k in ("sum", "gram", "mu", "sigma"):
        assert np.array_equal(r0[k], r1[k]), k     # identical state on both ranks after the all-reduce
    mu, sigma = activation_statistics(torch.from_numpy(a))
    assert np.abs(r0["mu"] - mu).max() < 1e-12
    assert np.abs(r0["sigma"] - sigma).max() < 1e-10 * max(1.0, np.abs(sigma).max())
    check_stats(r0["mu"], r0["sigma"], a.astype(np.float64))


@pytest.mark.parametrize("D,N,seed", [(64, 512, 1), (256, 2048, 2)])
def test_newton_schulz_distance_full_rank(D, N, seed):
    from littlegan_amd.fid import frechet_distance_ns
    mu1, S1, mu2, S2 = fixture(D, N, seed)
    ref, _ = eigh_reference(mu1, S1, mu2, S2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        d2, info = frechet_distance_ns(mu1, S1, mu2, S2)
        same, info_same = frechet_distance_ns(mu1, S1, mu1, S1)
    scale = np.trace(S1) + np.trace(S2)
    print(f"D={D} N={N}: {info['iterations']} iterations, error {abs(d2 - ref) / scale:.2e}; identical: {abs(same) / np.trace(S1):.2e}")
    assert info["status"] == 0 and not info["fallback"] and info_same["status"] == 0
    assert abs(d2 - ref) <= 1e-9 * scale
    assert abs(same) <= 1e-9 * np.trace(S1)


def test_newton_schulz_diagonal_closed_form_and_shape_checks():
    from littlegan_amd.fid import frechet_distance_ns
    rng = np.random.default_rng(1)
    m1, m2 = rng.standard_normal(16), rng.standard_normal(16)
    v1, v2 = rng.uniform(0.1, 2.0, 16), rng.uniform(0.1, 2.0, 16)
    exp = ((m1 - m2) ** 2).sum() + ((np.sqrt(v1) - np.sqrt(v2)) ** 2).sum()
    d2, info = frechet_distance_ns(m1, np.diag(v1), m2, np.diag(v2))
    assert info["status"] == 0 and abs(d2 - exp) <= 1e-9 * (v1.sum() + v2.sum())
    with pytest.raises(ValueError):
        frechet_distance_ns(np.zeros(3), np.eye(3), np.zeros(4), np.eye(4))
    with pytest.raises(ValueError):
        frechet_distance_ns(np.zeros(3), np.eye(3), np.zeros(3), np.eye(4))
    d0, info0 = frechet_distance_ns(np.zeros(4), np.zeros((4, 4)), np.ones(4), np.zeros((4, 4)))   # zero product: root 0
    assert info0["status"] == 0 and abs(d0 - 4.0) < 1e-12


@pytest.mark.parametrize("D,N,seed", [(256, 100, 5), (384, 50, 6)])
def test_newton_schulz_distance_rank_deficient(D, N, seed):
    """N < D: the iteration sits on a rounding plateau and would then diverge; the second stopping condition ends it there.  No
    fallback may be taken: a fallback would hide a broken stopping rule."""
    from littlegan_amd.fid import frechet_distance_ns
    mu1, S1, mu2, S2 = fixture(D, N, seed)
    ref, _ = eigh_reference(mu1, S1, mu2, S2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        d2, info = frechet_distance_ns(mu1, S1, mu2, S2)
    scale = np.trace(S1) + np.trace(S2)
    print(f"D={D} N={N}: {info['iterations']} iterations, error {abs(d2 - ref) / scale:.2e}")
    assert np.isfinite(d2) and info["status"] == 0 and not info["fallback"]
    assert abs(d2 - ref) <= 1e-4 * scale


def test_forced_non_convergence_falls_back_to_the_host_root():
    from littlegan_amd.fid import frechet_distance, frechet_distance_ns
    mu1, S1, mu2, S2 = fixture(256, 100, 5)
    with pytest.warns(UserWarning, match="did not converge"):
        d2, info = frechet_distance_ns(mu1, S1, mu2, S2, max_iter=3)
    assert info["status"] == 1 and info["fallback"] and info["iterations"] == 3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert d2 == frechet_distance(mu1, S1, mu2, S2)


def _saved_fixture(tmp_path):
    """the fixtures of tests/test_fid.py::test_evaluate_calc_on_saved_activations"""
    rng = np.random.default_rng(5)
    real = rng.standard_normal((300, 16)).astype(np.float32)
    np.save(tmp_path / "real.npy", real)
    gen_dir = tmp_path / "gen"
    gen_dir.mkdir()
    shift = np.zeros(16, np.float32)
    shift[3] = 2.0
    np.save(gen_dir / "activations.npy", real + shift)
    return real, gen_dir


def test_calc_streamed_with_device_sqrt_on_saved_activations(tmp_path):
    from littlegan_amd import fid
    real, gen_dir = _saved_fixture(tmp_path)
    stats = str(tmp_path / "stats.npz")
    mu, sigma = fid.pre_calculate(str(tmp_path / "real.npy"), stats, chunk_rows=64)
    check_stats(mu, sigma, real.astype(np.float64))
    with np.load(stats) as f:
        assert np.array_equal(f["mu"], mu) and np.array_equal(f["sigma"], sigma)
    log = str(tmp_path / "fid.log")
    assert abs(fid.calc(str(tmp_path / "real.npy"), stats, log, chunk_rows=64, device_sqrt=True)) < 1e-6
    v = fid.calc(str(gen_dir), stats, log, chunk_rows=64, device_sqrt=True)
    assert abs(v - 4.0) < 1e-4
    lines = [ln for ln in open(log).read().split("\n") if ln.strip()]
    assert len(lines) == 2 and abs(float(lines[1].split()[-1]) - v) < 1e-9
    assert open(log).read().startswith("\n ") and open(log).read().endswith("\n ")


def test_evaluate_cli_with_chunk_rows_and_device_sqrt(tmp_path):
    real, gen_dir = _saved_fixture(tmp_path)
    stats, log = str(tmp_path / "stats.npz"), str(tmp_path / "fid.log")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, os.path.join(ROOT, "evaluate.py")]
    flags = ["--chunk-rows", "64", "--device-sqrt"]
    r = subprocess.run(base + ["pre-calculate", str(tmp_path / "real.npy"), stats, "unused"] + flags, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "finished" in r.stdout, r.stderr
    vals = []
    for src in (str(tmp_path / "real.npy"), str(gen_dir)):
        r = subprocess.run(base + ["calc", src, stats, "unused", log] + flags, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        vals.append(float([ln for ln in r.stdout.splitlines() if ln.startswith("FID: ")][-1].split()[1]))
    assert abs(vals[0]) < 1e-6 and abs(vals[1] - 4.0) < 1e-4
    lines = [ln for ln in open(log).read().split("\n") if ln.strip()]
    assert len(lines) == 2 and abs(float(lines[1].split()[-1]) - vals[1]) < 1e-9


def test_config_keys_default_to_the_present_path():
    from littlegan_amd.config import DEFAULTS
    assert DEFAULTS["fid_chunk_rows"] is None and DEFAULTS["fid_device_sqrt"] is False


def test_abi_rejects_bad_arguments_without_gpu():
    from littlegan_amd.csrc.build import build
    build(verbose=False)
    from littlegan_amd import _lib
    h = _lib.load()
    assert h.lg_fid_accum(None, 4, 8, None, None, None, None) == -1 and b"null pointer" in h.lg_last_error()
    assert h.lg_fid_accum(8, 0, 8, None, 8, 8, None) == -1 and b"bad shape" in h.lg_last_error()
    assert h.lg_fid_accum(8, 4, 0, None, 8, 8, None) == -1 and b"bad shape" in h.lg_last_error()
    assert h.lg_fid_finalize(None, None, None, 4, 8, None, None, None) == -1 and b"null pointer" in h.lg_last_error()
    assert h.lg_fid_finalize(8, 8, None, 1, 8, 8, 8, None) == -1 and b"bad shape" in h.lg_last_error()
    assert h.lg_fid_distance(None, None, None, None, 8, 100, None, None, 0, None) == -1 and b"null pointer" in h.lg_last_error()
    assert h.lg_fid_distance(8, 8, 8, 8, 0, 100, 8, 8, 0, None) == -1 and b"bad shape" in h.lg_last_error()
    assert h.lg_fid_distance(8, 8, 8, 8, 8, 0, 8, 8, 0, None) == -1 and b"bad shape" in h.lg_last_error()
    assert h.lg_fid_distance(8, 8, 8, 8, 8, 100, 8, 8, 0, None) == -1 and b"workspace" in h.lg_last_error()
    assert h.lg_fid_gemm(None, None, None, 8, None, None) == -1 and b"null pointer" in h.lg_last_error()
    assert h.lg_fid_distance_workspace_bytes(64) == 4096 + 5 * 64 * 64 * 8
    assert h.lg_abi_version() == 1
