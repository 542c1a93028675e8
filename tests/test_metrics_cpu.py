"""KID and precision / recall / density / coverage (littlegan_amd/metrics.py) on the host path, against an oracle that
is independent of metrics.py: brute-force fp64 squared distances by differences with a sort, and explicit kernel matrices.

Tolerances are derived, not tuned.  The project bounds an fp64 dot of length D by eps = 1e-13 D max|a| max|b|
(tests/test_fid_stream_gpu.py).  A squared distance and a radius then carry at most 4 eps; a kernel sum at most
S_ij degree |t_ij|^(degree-1) gamma eps + 1e-13 S_ij |k_ij| with t = gamma dot + coef0 taken from the oracle's own matrices; a KID
value the same bounds divided by the estimator's normalisers.  Counts and flags must match exactly: the oracle asserts that no pair
of these inputs lies within 1e-9 (relative) of a ball boundary, five orders above the error of a squared distance."""
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # the spawned ranks import this module by name
from test_fid_stream import _free_port, run_ranks  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(0, 67, 129, 37), (1, 200, 131, 70), (2, 130, 70, 2048), (3, 64, 64, 4), (4, 65, 193, 33)]
KS = (1, 3, 5)
MARGIN = 1e-9


# ------------------------------------------------------------------ inputs and oracle (shared with tests/test_metrics_gpu.py)
@functools.lru_cache(maxsize=None)
def make_sets(seed, n, m, D):
    rng = np.random.default_rng(seed)
    L = 4
    P = rng.standard_normal((L, D)) / 2
    real = (rng.standard_normal((n, L)) @ P + 0.05 * rng.standard_normal((n, D))).astype(np.float32)
    fake = ((0.7 * rng.standard_normal((m, L)) + 0.5) @ P + 0.05 * rng.standard_normal((m, D))).astype(np.float32)
    return real, fake


def dot_eps(a, b):
    """the project's bound on an fp64 dot product of rows of a and b"""
    return 1e-13 * a.shape[1] * float(np.abs(a).max()) * float(np.abs(b).max())


def oracle_d2(a, b):
    """brute-force fp64 squared distances by differences"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    out = np.empty((a.shape[0], b.shape[0]))
    step = max(1, (1 << 22) // (b.shape[0] * b.shape[1]))
    for r in range(0, a.shape[0], step):
        out[r:r + step] = ((a[r:r + step, None] - b[None]) ** 2).sum(-1)
    return out


def oracle_d2_gemm(a, b):
    """the fp64 GEMM form, for sets too large for the difference form"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.maximum(0.0, (a * a).sum(1)[:, None] + (b * b).sum(1)[None] - 2.0 * (a @ b.T))


def ball_margin(d2, r2_of_column):
    """smallest relative distance of any pair to its ball boundary"""
    return float((np.abs(d2 - r2_of_column[None, :]) / r2_of_column[None, :]).min())


def oracle_prdc_from_d2(d_rr, d_ff, d_rf, k):
    n, m = d_rf.shape
    r_real = np.sort(d_rr, axis=1)[:, k]      # entry k of the list that includes the row itself
    r_fake = np.sort(d_ff, axis=1)[:, k]
    inside_real = d_rf <= r_real[:, None]     # [i, j]: fake j inside real i's ball
    inside_fake = d_rf <= r_fake[None, :]     # [i, j]: real i inside fake j's ball
    count_fake = inside_real.sum(0)
    count_real = inside_fake.sum(1)
    nearest = d_rf.min(1)
    margin = min(ball_margin(d_rf.T, r_real), ball_margin(d_rf, r_fake), float((np.abs(nearest - r_real) / r_real).min()))
    return {"precision": float((count_fake > 0).sum()) / m, "recall": float((count_real > 0).sum()) / n,
            "density": float(count_fake.sum()) / (float(k) * m), "coverage": float((nearest <= r_real).sum()) / n, "k": k,
            "r_real": r_real, "r_fake": r_fake, "count_fake": count_fake, "count_real": count_real, "nearest": nearest,
            "margin": margin}


@functools.lru_cache(maxsize=None)
def case_d2(case):
    real, fake = make_sets(*case)
    return oracle_d2(real, real), oracle_d2(fake, fake), oracle_d2(real, fake)


@functools.lru_cache(maxsize=None)
def oracle_prdc(case, k):
    return oracle_prdc_from_d2(*case_d2(case), k)


def oracle_poly(a, b, degree=3, gamma=None, coef0=1.0):
    """explicit kernel matrix -> (sum, trace (square only), bound on the sum, bound on the trace)"""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    gamma = 1.0 / a.shape[1] if gamma is None else gamma
    t = gamma * (a64 @ b64.T) + coef0
    k = t ** degree
    eps = dot_eps(a64, b64)
    err = degree * np.abs(t) ** (degree - 1) * gamma * eps
    bound = float(err.sum() + 1e-13 * np.abs(k).sum())
    if a.shape[0] == b.shape[0]:
        return float(k.sum()), float(np.trace(k)), bound, float(np.trace(err) + 1e-13 * np.abs(np.diagonal(k)).sum())
    return float(k.sum()), 0.0, bound, 0.0


def oracle_mmd2(x, y, **kw):
    """-> (MMD²_u, bound)"""
    n, m = x.shape[0], y.shape[0]
    sxx, txx, bxx, btxx = oracle_poly(x, x, **kw)
    syy, tyy, byy, btyy = oracle_poly(y, y, **kw)
    sxy, _, bxy, _ = oracle_poly(x, y, **kw)
    v = (sxx - txx) / (n * (n - 1.0)) + (syy - tyy) / (m * (m - 1.0)) - 2.0 * sxy / (float(n) * m)
    return v, (bxx + btxx) / (n * (n - 1.0)) + (byy + btyy) / (m * (m - 1.0)) + 2.0 * bxy / (float(n) * m)


def oracle_kid_subsets(real, fake, subsets, subset_size, seed, **kw):
    """repeats the documented draw order: per subset first the real rows, then the fake rows, from one RandomState(seed)"""
    rng = np.random.RandomState(seed)
    vals, bounds = [], []
    for _ in range(subsets):
        ir = rng.choice(real.shape[0], subset_size, replace=False)
        jf = rng.choice(fake.shape[0], subset_size, replace=False)
        v, b = oracle_mmd2(real[ir], fake[jf], **kw)
        vals.append(v)
        bounds.append(b)
    return np.array(vals), max(bounds)


def check_prdc(got, ora):
    assert ora["margin"] >= MARGIN, ora["margin"]           # the oracle excludes no pair: exactness may be asked
    for key in ("precision", "recall", "density", "coverage"):
        assert 0.0 < ora[key] < 1.25, (key, ora[key])        # no degenerate all-in / all-out case hides an error
        assert got[key] == ora[key], (key, got[key], ora[key])
    assert got["k"] == ora["k"]


# ------------------------------------------------------------------ host path against the oracle
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", CASES)
def test_prdc_host_matches_the_oracle_exactly(case, k):
    from littlegan_amd.metrics import prdc_from_activations
    real, fake = make_sets(*case)
    check_prdc(prdc_from_activations(torch.from_numpy(real), torch.from_numpy(fake), k=k), oracle_prdc(case, k))


@pytest.mark.parametrize("case", CASES)
def test_kid_host_full_sets_and_subsets_match_the_oracle(case):
    from littlegan_amd.metrics import kid_from_activations, kid_subset_indices
    real, fake = make_sets(*case)
    tr, tf = torch.from_numpy(real), torch.from_numpy(fake)
    ref, bound = oracle_mmd2(real, fake)
    full = kid_from_activations(tr, tf, subsets=0)
    print(f"{case}: full-set KID {full['kid']:.6e}, oracle {ref:.6e}, |diff| {abs(full['kid'] - ref):.2e}, bound {bound:.2e}")
    assert full["kid_std"] is None and full["subsets"] == 0 and abs(full["kid"] - ref) <= bound
    vals, vbound = oracle_kid_subsets(real, fake, 6, 50, 11)
    sub = kid_from_activations(tr, tf, subsets=6, subset_size=50, seed=11)
    assert sub["subsets"] == 6 and sub["subset_size"] == 50
    assert abs(sub["kid"] - vals.mean()) <= vbound and abs(sub["kid_std"] - vals.std()) <= 2 * vbound
    # the documented draw order, reproduced without metrics.py
    rng = np.random.RandomState(11)
    for ir, jf in kid_subset_indices(real.shape[0], fake.shape[0], 3, 50, 11):
        assert np.array_equal(ir, rng.choice(real.shape[0], 50, replace=False))
        assert np.array_equal(jf, rng.choice(fake.shape[0], 50, replace=False))
    # other kernel parameters
    ref2, bound2 = oracle_mmd2(real, fake, degree=2, gamma=0.5, coef0=0.25)
    assert abs(kid_from_activations(tr, tf, subsets=0, degree=2, gamma=0.5, coef0=0.25)["kid"] - ref2) <= bound2


def test_kid_subset_size_is_clamped_with_a_warning_and_arguments_are_checked():
    from littlegan_amd.metrics import kid_from_activations, prdc_from_activations
    real, fake = make_sets(*CASES[3])
    tr, tf = torch.from_numpy(real), torch.from_numpy(fake)
    with pytest.warns(UserWarning, match="subset_size"):
        res = kid_from_activations(tr, tf, subsets=2, subset_size=1000, seed=1)
    vals, bound = oracle_kid_subsets(real, fake, 2, 64, 1)
    assert res["subset_size"] == 64 and abs(res["kid"] - vals.mean()) <= bound
    for bad in (dict(subsets=-1), dict(degree=0), dict(degree=9), dict(subset_size=1), dict(chunk_rows=0)):
        with pytest.raises(ValueError):
            kid_from_activations(tr, tf, **bad)
    with pytest.raises(ValueError):
        kid_from_activations(tr, tf[:, :3])
    with pytest.raises(ValueError):
        kid_from_activations(tr[:1], tf)
    for bad in (0, 16, 64):
        with pytest.raises(ValueError):
            prdc_from_activations(tr, tf, k=bad)


@pytest.mark.parametrize("chunk", [64, 50, 10 ** 6])   # one tile, ragged, larger than N
def test_chunk_rows_changes_nothing(chunk):
    from littlegan_amd import metrics
    case = CASES[1]
    real, fake = make_sets(*case)
    tr, tf = torch.from_numpy(real), torch.from_numpy(fake)
    x, y = metrics._prepare(tr, tf, "test")
    for k in KS:
        whole = metrics._radii(x, k, *metrics._row_blocks(x.shape[0], None, 0, 1), False)
        every, own = metrics._row_blocks(x.shape[0], chunk, 0, 1)
        assert sum(hi - lo for lo, hi in every) == x.shape[0] and all(hi - lo <= chunk for lo, hi in every)
        assert torch.equal(metrics._radii(x, k, every, own, False), whole)                    # radii: exactly
        assert np.abs(whole.numpy() - oracle_prdc(case, k)["r_real"]).max() <= 4 * dot_eps(real, real)
        check_prdc(metrics.prdc_from_activations(tr, tf, k=k, chunk_rows=chunk), oracle_prdc(case, k))   # counts: exactly
    ref, bound = oracle_mmd2(real, fake)
    assert abs(metrics.kid_from_activations(tr, tf, subsets=0, chunk_rows=chunk)["kid"] - ref) <= bound
    vals, vbound = oracle_kid_subsets(real, fake, 3, 100, 2)
    assert abs(metrics.kid_from_activations(tr, tf, subsets=3, subset_size=100, seed=2, chunk_rows=chunk)["kid"] - vals.mean()) <= vbound


def test_identical_sets():
    from littlegan_amd.metrics import kid_from_activations, prdc_from_activations
    real, _ = make_sets(*CASES[0])
    t = torch.from_numpy(real)
    res = prdc_from_activations(t, t.clone(), k=3)
    assert res["precision"] == 1.0 and res["recall"] == 1.0 and res["coverage"] == 1.0
    _, bound = oracle_mmd2(real, real)
    assert kid_from_activations(t, t.clone(), subsets=0)["kid"] <= bound


# ------------------------------------------------------------------ two ranks
def _metrics_rank_worker(rank, world, port, real_path, fake_path, outdir, device="cpu"):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        from littlegan_amd.metrics import kid_from_activations, prdc_from_activations
        real, fake = torch.from_numpy(np.load(real_path)).to(device), torch.from_numpy(np.load(fake_path)).to(device)
        full = kid_from_activations(real, fake, subsets=0, chunk_rows=48)
        sub = kid_from_activations(real, fake, subsets=5, subset_size=60, seed=3)
        pr = prdc_from_activations(real, fake, k=3, chunk_rows=48)
        np.savez(os.path.join(outdir, f"rank_{rank}.npz"), full=full["kid"], sub=sub["kid"], sub_std=sub["kid_std"],
                 prdc=np.array([pr[key] for key in ("precision", "recall", "density", "coverage")]))
    finally:
        dist.destroy_process_group()


def check_two_ranks(tmp_path, device, timeout):
    case = CASES[1]
    real, fake = make_sets(*case)
    np.save(tmp_path / "real.npy", real)
    np.save(tmp_path / "fake.npy", fake)
    port = _free_port()
    run_ranks(_metrics_rank_worker, lambda r: (r, 2, port, str(tmp_path / "real.npy"), str(tmp_path / "fake.npy"), str(tmp_path), device),
              2, timeout)
    r0, r1 = np.load(tmp_path / "rank_0.npz"), np.load(tmp_path / "rank_1.npz")
    for key in ("full", "sub", "sub_std", "prdc"):
        assert np.array_equal(r0[key], r1[key]), key       # every rank reports the same values
    ora = oracle_prdc(case, 3)
    assert ora["margin"] >= MARGIN
    assert list(r0["prdc"]) == [ora[key] for key in ("precision", "recall", "density", "coverage")]
    ref, bound = oracle_mmd2(real, fake)
    assert abs(float(r0["full"]) - ref) <= bound
    vals, vbound = oracle_kid_subsets(real, fake, 5, 60, 3)
    assert abs(float(r0["sub"]) - vals.mean()) <= vbound and abs(float(r0["sub_std"]) - vals.std()) <= 2 * vbound
    return r0


def test_world2_gloo_agrees_with_world1(tmp_path):
    from littlegan_amd.metrics import kid_from_activations, prdc_from_activations
    r0 = check_two_ranks(tmp_path, "cpu", 240)
    real, fake = (torch.from_numpy(a) for a in make_sets(*CASES[1]))
    pr = prdc_from_activations(real, fake, k=3)
    assert list(r0["prdc"]) == [pr[key] for key in ("precision", "recall", "density", "coverage")]
    _, bound = oracle_mmd2(*make_sets(*CASES[1]))
    assert abs(float(r0["full"]) - kid_from_activations(real, fake, subsets=0)["kid"]) <= 2 * bound


# ------------------------------------------------------------------ CLI, config, ABI
def test_evaluate_cli_writes_three_logs_and_keeps_the_fid_line(tmp_path):
    real, fake = make_sets(*CASES[0])
    np.save(tmp_path / "real.npy", real)
    np.save(tmp_path / "fake.npy", fake)
    stats = str(tmp_path / "stats.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, os.path.join(ROOT, "evaluate.py")]
    r = subprocess.run(base + ["pre-calculate", str(tmp_path / "real.npy"), stats, "unused"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "finished" in r.stdout, r.stderr
    plain_log, log = str(tmp_path / "plain.log"), str(tmp_path / "all.log")
    calc = base + ["calc", str(tmp_path / "fake.npy"), stats, "unused"]
    plain = subprocess.run(calc + [plain_log], env=env, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr
    assert not os.path.exists(plain_log + ".kid") and not os.path.exists(plain_log + ".prdc")   # the default selects FID alone
    full = subprocess.run(calc + [log, "--metrics", "fid,kid,prdc", "--real-activations", str(tmp_path / "real.npy"), "--kid-subsets", "4",
                                  "--kid-subset-size", "40", "--prdc-k", "3", "--seed", "5"], env=env, capture_output=True, text=True,
                          timeout=300)
    assert full.returncode == 0, full.stderr
    fid_line = [ln for ln in plain.stdout.splitlines() if ln.startswith("FID: ")]
    assert len(fid_line) == 1 and fid_line == [ln for ln in full.stdout.splitlines() if ln.startswith("FID: ")]
    assert plain.stdout.splitlines() == fid_line            # nothing new on stdout without the flags
    for path in (plain_log, log, log + ".kid", log + ".prdc"):
        text = open(path).read()
        assert text.startswith("\n ") and text.endswith("\n ") and len([ln for ln in text.split("\n") if ln.strip()]) == 1, path
    assert open(log).read().split()[1:] == open(plain_log).read().split()[1:] == [fid_line[0].split()[1]]
    vals, bound = oracle_kid_subsets(real, fake, 4, 40, 5)
    kid_line = [ln for ln in full.stdout.splitlines() if ln.startswith("KID: ")][0].split()
    assert kid_line[2] == "+-" and abs(float(kid_line[1]) - vals.mean()) <= bound and abs(float(kid_line[3]) - vals.std()) <= 2 * bound
    assert [float(v) for v in open(log + ".kid").read().split()[1:]] == [float(kid_line[1]), float(kid_line[3])]
    ora = oracle_prdc(CASES[0], 3)
    assert [float(v) for v in open(log + ".prdc").read().split()[1:]] == [ora[key] for key in ("precision", "recall", "density", "coverage")]
    assert any(ln.startswith("PRDC: ") for ln in full.stdout.splitlines())
    bad = subprocess.run(calc + [log, "--metrics", "fid,kidd"], env=env, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "kidd" in bad.stderr
    need = subprocess.run(calc + [log, "--metrics", "kid"], env=env, capture_output=True, text=True, timeout=300)
    assert need.returncode != 0 and "--real-activations" in need.stderr


def test_config_defaults_select_fid_alone(tmp_path):
    from littlegan_amd import config
    d = config.DEFAULTS
    assert d["evaluate_metrics"] == ["fid"] and d["evaluate_real_activations"] is None
    assert (d["kid_subsets"], d["kid_subset_size"], d["prdc_k"]) == (100, 1000, 3)
    for key in ("evaluate_metrics", "evaluate_real_activations", "kid_subsets", "kid_subset_size", "prdc_k"):
        assert key in config.__doc__
    assert config.Arg(["evaluate", "x"], config_dir=str(tmp_path)).evaluate_metrics == ["fid"]
    (tmp_path / "all.config.json").write_text('{"evaluate_metrics": ["fid", "kid", "prdc"], "kid_subsets": 0}')
    a = config.Arg(["evaluate", "x", "-e", "all"], config_dir=str(tmp_path))
    assert a.evaluate_metrics == ["fid", "kid", "prdc"] and a.kid_subsets == 0
    (tmp_path / "bad.config.json").write_text('{"evaluate_metrics": ["fid", "is"]}')
    with pytest.raises(ValueError, match="evaluate_metrics"):
        config.Arg(["evaluate", "x", "-e", "bad"], config_dir=str(tmp_path))
    for bad in ([], "", "fid;kid", 3):
        with pytest.raises(ValueError, match="evaluate_metrics"):
            config.metric_list(bad)
    assert config.metric_list("kid, prdc,kid") == ["kid", "prdc"]


def test_abi_rejects_bad_arguments_without_gpu():
    import ctypes
    from littlegan_amd.csrc.build import build
    build(verbose=False)
    from littlegan_amd import _lib
    h = _lib.load()
    gc = (ctypes.c_double * 2)(0.5, 1.0)
    g = ctypes.addressof(gc)
    big = 1 << 40
    # poly_sum(x, n, y, m, D, degree, gamma_coef0, diag, sums, ws, ws_bytes, stream)
    assert h.lg_pairs_poly_sum(None, 4, 8, 4, 8, 3, g, 0, 8, 8, big, None) == -1 and b"null pointer" in h.lg_last_error()
    assert h.lg_pairs_poly_sum(8, 4, 8, 4, 8, 3, None, 0, 8, 8, big, None) == -1 and b"null pointer" in h.lg_last_error()
    assert h.lg_pairs_poly_sum(8, 4, 8, 4, 8, 3, g, 0, None, 8, big, None) == -1 and b"null pointer" in h.lg_last_error()
    assert h.lg_pairs_poly_sum(8, 4, 8, 4, 8, 3, g, 0, 8, None, big, None) == -1 and b"null pointer" in h.lg_last_error()
    for n, m, D in ((0, 4, 8), (4, 0, 8), (4, 4, 0)):
        assert h.lg_pairs_poly_sum(8, n, 8, m, D, 3, g, 0, 8, 8, big, None) == -1 and b"bad shape" in h.lg_last_error()
        assert h.lg_pairs_knn(8, n, 8, m, D, 3, 8, 8, big, None) == -1 and b"bad shape" in h.lg_last_error()
        assert h.lg_pairs_ball_count(8, n, 8, m, 8, D, 8, 8, big, None) == -1 and b"bad shape" in h.lg_last_error()
        assert h.lg_pairs_workspace_bytes(n, m, D) == 0
    for degree in (0, 9):
        assert h.lg_pairs_poly_sum(8, 4, 8, 4, 8, degree, g, 0, 8, 8, big, None) == -1 and b"degree" in h.lg_last_error()
    assert h.lg_pairs_poly_sum(8, 4, 8, 5, 8, 3, g, 1, 8, 8, big, None) == -1 and b"diag" in h.lg_last_error()
    need = h.lg_pairs_workspace_bytes(4, 5, 8)
    assert need > 0
    assert h.lg_pairs_poly_sum(8, 4, 8, 5, 8, 3, g, 0, 8, 8, need - 1, None) == -1 and b"workspace" in h.lg_last_error()
    # knn(x, n, y, m, D, kk, best, ws, ws_bytes, stream)
    assert h.lg_pairs_knn(None, 4, 8, 5, 8, 3, 8, 8, big, None) == -1 and b"null pointer" in h.lg_last_error()
    assert h.lg_pairs_knn(8, 4, 8, 5, 8, 3, None, 8, big, None) == -1 and b"null pointer" in h.lg_last_error()
    for kk in (0, 17):
        assert h.lg_pairs_knn(8, 4, 8, 5, 8, kk, 8, 8, big, None) == -1 and b"kk" in h.lg_last_error()
    assert h.lg_pairs_knn(8, 4, 8, 5, 8, 3, 8, 8, need - 1, None) == -1 and b"workspace" in h.lg_last_error()
    # ball_count(q, n, ref, m, radius2, D, count, ws, ws_bytes, stream)
    assert h.lg_pairs_ball_count(8, 4, None, 5, 8, 8, 8, 8, big, None) == -1 and b"null pointer" in h.lg_last_error()
    assert h.lg_pairs_ball_count(8, 4, 8, 5, None, 8, 8, 8, big, None) == -1 and b"null pointer" in h.lg_last_error()
    assert h.lg_pairs_ball_count(8, 4, 8, 5, 8, 8, None, 8, big, None) == -1 and b"null pointer" in h.lg_last_error()
    assert h.lg_pairs_ball_count(8, 4, 8, 5, 8, 8, 8, 8, need - 1, None) == -1 and b"workspace" in h.lg_last_error()
    # the workspace never grows with n m: norms + tile partials + partial lists
    assert h.lg_pairs_workspace_bytes(30000, 30000, 2048) < 64 * 1000 * 1000
    assert h.lg_abi_version() == 1
