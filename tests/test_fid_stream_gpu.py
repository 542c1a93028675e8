"""The device side of the streamed FID pass: lg_fid_accum / lg_fid_finalize (csrc/fid.hip) against numpy and lg_fid_stats,
lg_fid_distance and its fp64 GEMM (csrc/fid_sqrt.hip) against the eigh reference and torch.matmul, run-to-run bit identity, two gloo
ranks on the one GPU, and calc(..., chunk_rows, device_sqrt=True) against the default calc."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # the spawned ranks import the CPU test module by name too
from test_fid_stream import _free_port, _rank_worker, check_stats, eigh_reference, fixture, run_ranks  # noqa: E402

pytestmark = pytest.mark.gpu


def _data(N, D):
    g = torch.Generator(device="cuda").manual_seed(N)
    return torch.randn(N, D, device="cuda", generator=g) * 3.0 + 1.5


def _accumulate(a, chunk, shift):
    from littlegan_amd import ops
    N, D = a.shape
    s = torch.zeros(D, dtype=torch.float64, device="cuda")
    g = torch.zeros(ops.fid_gram_elems(D), dtype=torch.float64, device="cuda")
    for r in range(0, N, chunk):
        ops.fid_accum(a[r:r + chunk].contiguous(), s, g, shift)
    mu, sigma = ops.fid_finalize(s, g, N, shift)
    return s, g, mu, sigma


@pytest.mark.parametrize("N,D", [(1000, 2048), (777, 192), (33, 70)])
@pytest.mark.parametrize("shifted", [False, True])
def test_accum_finalize_match_numpy_and_fid_stats(N, D, shifted):
    from littlegan_amd import ops
    a = _data(N, D)
    an = a.double().cpu().numpy()
    shift = (torch.full((D,), 1.4, dtype=torch.float64, device="cuda") + torch.arange(D, device="cuda").double() * 1e-3) if shifted else None
    mu_w, sigma_w = ops.fid_stats(a)
    for chunk in (1, 33, 256, N):
        s, g, mu, sigma = _accumulate(a, chunk, shift)
        check_stats(mu.cpu().numpy(), sigma.cpu().numpy(), an)
        assert torch.equal(sigma, sigma.t())
        assert (mu - mu_w).abs().max().item() < 1e-12
        assert (sigma - sigma_w).abs().max().item() < 1e-10 * max(1.0, sigma_w.abs().max().item())


def test_same_chunk_sequence_is_bit_identical():
    a = _data(777, 192)
    shift = torch.full((192,), 1.5, dtype=torch.float64, device="cuda")
    r1 = _accumulate(a, 33, shift)
    r2 = _accumulate(a, 33, shift)
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)


def test_accumulator_on_the_device_and_argument_checks():
    from littlegan_amd import ops
    from littlegan_amd.fid import ActivationAccumulator
    a = _data(300, 70)
    acc = ActivationAccumulator(70, "cuda", np.full(70, 1.5))
    for r in range(0, 300, 64):
        acc.update(a[r:r + 64])
    other = ActivationAccumulator(70, "cuda", np.full(70, 1.5)).update(a[:10])
    acc.merge(other)
    check_stats(*acc.finalize(), torch.cat([a, a[:10]]).double().cpu().numpy())
    with pytest.raises(ValueError):
        ops.fid_accum(a, torch.zeros(70, dtype=torch.float64, device="cuda"), torch.zeros(5, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ops.fid_accum(a, torch.zeros(64, dtype=torch.float64, device="cuda"),
                      torch.zeros(ops.fid_gram_elems(70), dtype=torch.float64, device="cuda"))


def test_two_gloo_ranks_share_the_gpu(tmp_path):
    from littlegan_amd import ops
    a = (torch.randn(203, 130, generator=torch.Generator().manual_seed(3)) * 2.0 + 0.7).numpy()
    np.save(tmp_path / "all.npy", a)
    shift = np.full(130, 0.5)
    port = _free_port()
    run_ranks(_rank_worker, lambda r: (r, 2, port, str(tmp_path / "all.npy"), 130, shift, str(tmp_path), "cuda"), 2, 300)
    r0, r1 = np.load(tmp_path / "rank_0.npz"), np.load(tmp_path / "rank_1.npz")
    assert int(r0["own"]) + int(r1["own"]) == 203 and int(r0["count"]) == int(r1["count"]) == 203
    for k in ("sum", "gram", "mu", "sigma"):
        assert np.array_equal(r0[k], r1[k]), k
    mu, sigma = ops.fid_stats(torch.from_numpy(a).cuda())
    assert np.abs(r0["mu"] - mu.cpu().numpy()).max() < 1e-12
    assert np.abs(r0["sigma"] - sigma.cpu().numpy()).max() < 1e-10 * max(1.0, sigma.abs().max().item())
    check_stats(r0["mu"], r0["sigma"], a.astype(np.float64))


def _device(*xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


@pytest.mark.parametrize("D,N,seed", [(2048, 10000, 0), (192, 2000, 3), (70, 600, 4)])
def test_distance_full_rank_against_eigh(D, N, seed):
    from littlegan_amd import ops
    mu1, S1, mu2, S2 = fixture(D, N, seed)
    ref, ref_tr = eigh_reference(mu1, S1, mu2, S2)
    t = _device(mu1, S1, mu2, S2)
    d2, tr, iters, status = ops.fid_distance(*t)
    again = ops.fid_distance(*t)
    same = ops.fid_distance(t[0], t[1], t[0], t[1])
    scale = np.trace(S1) + np.trace(S2)
    print(f"D={D} N={N}: {iters} iterations, error {abs(d2 - ref) / scale:.2e}; identical: {abs(same[0]) / np.trace(S1):.2e}")
    assert status == 0 and same[3] == 0
    assert abs(d2 - ref) <= 1e-9 * scale
    assert abs(same[0]) <= 1e-9 * np.trace(S1)
    assert again == (d2, tr, iters, status)      # bit-identical: floats compared exactly


@pytest.mark.parametrize("D,N,seed", [(256, 100, 5), (384, 50, 6)])
def test_distance_rank_deficient_against_eigh(D, N, seed):
    from littlegan_amd import ops
    from littlegan_amd.fid import frechet_distance_ns
    mu1, S1, mu2, S2 = fixture(D, N, seed)
    ref, _ = eigh_reference(mu1, S1, mu2, S2)
    d2, tr, iters, status = ops.fid_distance(*_device(mu1, S1, mu2, S2))
    scale = np.trace(S1) + np.trace(S2)
    print(f"D={D} N={N}: {iters} iterations, status {status}, error {abs(d2 - ref) / scale:.2e}")
    assert np.isfinite(d2) and status == 0
    assert abs(d2 - ref) <= 1e-4 * scale
    with warnings.catch_warnings():
        warnings.simplefilter("error")           # no fallback through the public entry point either
        d2p, info = frechet_distance_ns(mu1, S1, mu2, S2, device="cuda")
    assert d2p == d2 and info["status"] == 0 and not info["fallback"]


def test_forced_non_convergence_on_the_device_falls_back():
    from littlegan_amd.fid import frechet_distance, frechet_distance_ns
    mu1, S1, mu2, S2 = fixture(256, 100, 5)
    with pytest.warns(UserWarning, match="did not converge"):
        d2, info = frechet_distance_ns(mu1, S1, mu2, S2, device="cuda", max_iter=3)
    assert info["status"] == 1 and info["fallback"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert d2 == frechet_distance(mu1, S1, mu2, S2)


@pytest.mark.parametrize("D", [70, 193, 256])
def test_fp64_gemm_matches_torch(D):
    """asymmetric operands (a swapped row / column in the C write or the A fragment would show), ragged D, alpha / beta epilogue"""
    from littlegan_amd import ops
    g = torch.Generator().manual_seed(D)
    a = torch.randn(D, D, generator=g, dtype=torch.float64) + torch.arange(D, dtype=torch.float64)[:, None] * 0.01
    b = torch.randn(D, D, generator=g, dtype=torch.float64) - torch.arange(D, dtype=torch.float64)[None, :] * 0.02
    tol = 1e-13 * D * a.abs().max().item() * b.abs().max().item()
    for alpha, beta in ((1.0, 0.0), (-0.5, 1.5)):
        c = ops.fid_gemm(a.cuda(), b.cuda(), alpha, beta).cpu()
        ref = alpha * torch.matmul(a, b) + beta * torch.eye(D, dtype=torch.float64)
        err = (c - ref).abs().max().item()
        print(f"D={D} alpha={alpha} beta={beta}: |c - ref|max {err:.2e} (bound {tol:.2e})")
        assert err <= tol
    assert torch.equal(ops.fid_gemm(a.cuda(), b.cuda()), ops.fid_gemm(a.cuda(), b.cuda()))


def test_calc_streamed_device_sqrt_agrees_with_default_calc(tmp_path):
    from littlegan_amd import fid
    rng = np.random.default_rng(9)
    W = rng.standard_normal((96, 96)) * 0.3
    real = np.maximum(rng.standard_normal((1500, 96)) @ W + 0.3, 0).astype(np.float32)
    gen = np.maximum(rng.standard_normal((1300, 96)) @ (1.1 * W) + 0.35, 0).astype(np.float32)
    np.save(tmp_path / "real.npy", real)
    np.save(tmp_path / "gen.npy", gen)
    stats = str(tmp_path / "stats.npz")
    mu, sigma = fid.pre_calculate(str(tmp_path / "real.npy"), stats)
    log_a, log_b = str(tmp_path / "a.log"), str(tmp_path / "b.log")
    base = fid.calc(str(tmp_path / "gen.npy"), stats, log_a)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        new = fid.calc(str(tmp_path / "gen.npy"), stats, log_b, chunk_rows=200, device_sqrt=True)
    sg = np.cov(gen.astype(np.float64), rowvar=False)
    scale = np.trace(sigma) + np.trace(sg)
    print(f"calc default {base!r}, streamed + device sqrt {new!r}, difference {abs(new - base) / scale:.2e} of the trace scale")
    assert abs(new - base) <= 1e-9 * scale
    assert len([ln for ln in open(log_b).read().split("\n") if ln.strip()]) == 1
