"""The pair kernels of csrc/pairs.hip (lg_pairs_poly_sum / lg_pairs_knn / lg_pairs_ball_count) through ops, and metrics.py on CUDA
tensors, against the oracle of tests/test_metrics_cpu.py (brute-force fp64, independent of metrics.py) with its derived bounds:
eps = 1e-13 D max|a| max|b| per dot, 4 eps per squared distance, the kernel-sum bound from the oracle's own matrices; counts exact
once the oracle has shown that no pair lies within 1e-9 of a ball boundary.  The knn column split changes at ceil(m / 64) > 4 and at
n > 16384 (pairs.hip, knn_split): the five cases and the extra shapes sit on both sides of each."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # the spawned ranks import the CPU test module by name too
from test_metrics_cpu import (CASES, MARGIN, ball_margin, check_prdc, check_two_ranks, dot_eps, make_sets, oracle_d2,  # noqa: E402
                              oracle_d2_gemm, oracle_kid_subsets, oracle_mmd2, oracle_poly, oracle_prdc)

pytestmark = pytest.mark.gpu

LARGE = (7, 1500, 1100, 256)            # many blocks, a split knn pass with several column tiles per block
ROUTE = [(8, 16384, 320, 8), (9, 16385, 320, 8)]   # the last n with a column split, the first without


def _cuda(*xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


@functools.lru_cache(maxsize=None)
def _d2(case):
    """oracle squared distances [n, m] of a case: by differences, the GEMM form for the large shapes"""
    real, fake = make_sets(*case)
    return oracle_d2(real, fake) if real.shape[0] * fake.shape[0] * real.shape[1] <= (1 << 25) else oracle_d2_gemm(real, fake)


def _knn(x, y, kk, cuts=None):
    from littlegan_amd import ops
    best = torch.full((x.shape[0], kk), float("inf"), dtype=torch.float64, device="cuda")
    cuts = [0, y.shape[0]] if cuts is None else cuts
    for c0, c1 in zip(cuts[:-1], cuts[1:]):
        ops.pairs_knn(x, y[c0:c1], best)
    return best


def _ball(q, ref, r2, cuts=None):
    from littlegan_amd import ops
    count = torch.zeros(q.shape[0], dtype=torch.int32, device="cuda")
    cuts = [0, ref.shape[0]] if cuts is None else cuts
    for c0, c1 in zip(cuts[:-1], cuts[1:]):
        ops.pairs_ball_count(q, ref[c0:c1], r2[c0:c1], count)
    return count


def _pieces(m):
    return [[0, m // 2, m], [0, m // 3, m // 3 + 1, m]] if m >= 4 else [[0, 1, m]]


@pytest.mark.parametrize("kk", [1, 4, 6])
@pytest.mark.parametrize("case", CASES + [LARGE])
def test_knn_lists_match_the_oracle_and_do_not_depend_on_the_column_pieces(case, kk):
    _check_knn(case, kk)


@pytest.mark.parametrize("case", ROUTE)
def test_knn_on_both_sides_of_the_row_count_that_ends_the_column_split(case):
    _check_knn(case, 4)


def _check_knn(case, kk):
    real, fake = make_sets(*case)
    x, y = _cuda(real, fake)
    ref = np.sort(_d2(case), axis=1)[:, :kk]
    best = _knn(x, y, kk)
    err = np.abs(best.cpu().numpy() - ref).max()
    print(f"{case} kk={kk}: max |d2 - oracle| {err:.2e}, bound {4 * dot_eps(real, fake):.2e}")
    assert err <= 4 * dot_eps(real, fake)
    assert torch.equal(best, best.sort(dim=1).values)
    for cuts in _pieces(fake.shape[0]):
        assert torch.equal(_knn(x, y, kk, cuts), best), cuts     # bit for bit
    assert torch.equal(_knn(x, y, kk), best)


def test_knn_list_as_long_as_the_set_and_self_distances():
    real, _ = make_sets(5, 16, 16, 8)
    (x,) = _cuda(real)
    best = _knn(x, x, 16)
    ref = np.sort(oracle_d2(real, real), axis=1)
    assert np.abs(best.cpu().numpy() - ref).max() <= 4 * dot_eps(real, real)
    assert torch.isfinite(best).all() and (best >= 0).all()


@pytest.mark.parametrize("case", CASES + [LARGE, (6, 1, 3, 5)])
def test_ball_counts_are_exact_and_do_not_depend_on_the_column_pieces(case):
    real, fake = make_sets(*case)
    n, m = real.shape[0], fake.shape[0]
    d2 = _d2(case)                                   # [real, fake]
    if n > 3:
        d_rr = oracle_d2(real, real) if n <= 256 else oracle_d2_gemm(real, real)
        r2 = np.sort(d_rr, axis=1)[:, 3]             # the radii of k = 3
        q, ref, dq = fake, real, d2.T                # fakes inside the real balls
    else:
        r2 = np.full(m, d2.mean())                   # one ragged tile: a radius that takes some pairs and leaves some
        q, ref, dq = real, fake, d2
    assert ball_margin(dq, r2) >= MARGIN             # the oracle excludes no pair: exactness may be asked
    want = (dq <= r2[None, :]).sum(1)
    assert 0 < want.sum() < dq.size
    tq, tref, tr2 = _cuda(q, ref, r2)
    got = _ball(tq, tref, tr2)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    for cuts in _pieces(ref.shape[0]):
        assert torch.equal(_ball(tq, tref, tr2, cuts), got), cuts
    from littlegan_amd import ops
    ops.pairs_ball_count(tq, tref, tr2, got)         # the counters are added to
    assert np.array_equal(got.cpu().numpy(), 2 * want)


@pytest.mark.parametrize("case", CASES + [LARGE, (6, 1, 3, 5)])
def test_poly_sums_match_the_oracle_and_repeat_bit_for_bit(case):
    from littlegan_amd import ops
    real, fake = make_sets(*case)
    x, y = _cuda(real, fake)
    for kw in (dict(), dict(degree=2, gamma=0.5, coef0=0.25), dict(degree=8, gamma=0.01, coef0=1.0), dict(degree=1, gamma=1.0, coef0=0.0)):
        s, _, bound, _ = oracle_poly(real, fake, **kw)
        sums = ops.pairs_poly_sum(x, y, torch.zeros(2, dtype=torch.float64, device="cuda"), **kw)
        again = ops.pairs_poly_sum(x, y, torch.zeros(2, dtype=torch.float64, device="cuda"), **kw)
        assert torch.equal(sums, again)              # bit for bit
        print(f"{case} {kw}: |sum - oracle| {abs(sums[0].item() - s):.2e}, bound {bound:.2e}")
        assert abs(sums[0].item() - s) <= bound and sums[1].item() == 0.0
        ops.pairs_poly_sum(x, y, sums, **kw)         # the sums are added to
        assert abs(sums[0].item() - 2 * s) <= 2 * bound
    # diag: the trace of Kxx
    s, tr, bound, tbound = oracle_poly(real, real)
    sums = ops.pairs_poly_sum(x, x, torch.zeros(2, dtype=torch.float64, device="cuda"), diag=True)
    assert abs(sums[0].item() - s) <= bound and abs(sums[1].item() - tr) <= tbound
    assert torch.equal(sums, ops.pairs_poly_sum(x, x, torch.zeros(2, dtype=torch.float64, device="cuda"), diag=True))


@pytest.mark.parametrize("case", CASES)
def test_metrics_on_the_device_equal_the_host_path(case):
    from littlegan_amd.metrics import kid_from_activations, prdc_from_activations
    real, fake = make_sets(*case)
    hr, hf = torch.from_numpy(real), torch.from_numpy(fake)
    dr, df = hr.cuda(), hf.cuda()
    ref, bound = oracle_mmd2(real, fake)
    host_prdc = {k: prdc_from_activations(hr, hf, k=k) for k in (1, 3, 5)}
    host_kid = kid_from_activations(hr, hf, subsets=0)["kid"]
    for chunk in (None, 64):
        for k in (1, 3, 5):
            got = prdc_from_activations(dr, df, k=k, chunk_rows=chunk)
            check_prdc(got, oracle_prdc(case, k))
            assert got == host_prdc[k]                                           # the four values: exactly
        dev = kid_from_activations(dr, df, subsets=0, chunk_rows=chunk)["kid"]
        assert abs(dev - ref) <= bound and abs(host_kid - ref) <= bound          # both within the bound of the oracle's value
    vals, vbound = oracle_kid_subsets(real, fake, 4, 40, 9)
    for a, b in ((hr, hf), (dr, df)):
        res = kid_from_activations(a, b, subsets=4, subset_size=40, seed=9)
        assert res["subset_size"] == 40 and abs(res["kid"] - vals.mean()) <= vbound and abs(res["kid_std"] - vals.std()) <= 2 * vbound


def test_workspace_stays_small_and_arguments_are_checked():
    from littlegan_amd import ops
    assert ops.pairs_workspace_bytes(30000, 30000, 2048) < 64 * 1000 * 1000
    x = torch.zeros(8, 4, device="cuda")
    s2 = torch.zeros(2, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        ops.pairs_poly_sum(x, torch.zeros(8, 5, device="cuda"), s2)
    with pytest.raises(ValueError):
        ops.pairs_poly_sum(x, x[:7], s2, diag=True)
    with pytest.raises(ValueError):
        ops.pairs_poly_sum(x, x, s2, degree=9)
    with pytest.raises(ValueError):
        ops.pairs_poly_sum(x, x, torch.zeros(2, device="cuda"))
    with pytest.raises(ValueError):
        ops.pairs_knn(x, x, torch.zeros(8, 17, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ops.pairs_knn(x, x, torch.zeros(7, 3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ops.pairs_ball_count(x, x, torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros(8, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ops.pairs_ball_count(x, x, torch.zeros(7, dtype=torch.float64, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda"))


def test_two_gloo_ranks_share_the_gpu(tmp_path):
    check_two_ranks(tmp_path, "cuda", 300)
