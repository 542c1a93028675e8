"""Sample-based companions of FID on saved activations: KID (Bińkowski et al. 2018: the unbiased MMD² with the cubic
polynomial kernel) and improved precision / recall (Kynkäänniemi et al. 2019: k-NN manifolds) with density / coverage (Naeem et al.
2020) from the same passes.  The reference evaluates FID alone; these are this project's additions.

Everything reduces to pairwise passes over two activation sets, X [n, D] against Y [m, D], that never materialise the n x m matrix.
CUDA tensors run the in-tree fp64-MFMA kernels (csrc/pairs.hip: lg_pairs_poly_sum / lg_pairs_knn / lg_pairs_ball_count); host tensors
(tests, tiny inputs) run the same formulas in torch float64, as fid.py does.  chunk_rows streams both sets in row blocks; under an
initialised process group every rank takes the contiguous row share iter_activation_chunks defines and the group all-reduces."""
import warnings

import numpy as np
import torch

from .config import METRIC_NAMES, metric_list  # noqa: F401  (re-exported: the CLI and main.py validate through these)
from .fid import _dist_rank_world

_HOST_D2_ELEMS = 1 << 22   # doubles in one [rows, m, D] difference block of the host path


def _prepare(real, fake, who):
    real, fake = torch.as_tensor(real), torch.as_tensor(fake)
    if real.dim() != 2 or fake.dim() != 2 or real.shape[1] != fake.shape[1] or real.shape[1] < 1:
        raise ValueError(f"{who}: need [N, D] and [M, D] activation matrices with the same D, got {tuple(real.shape)} and {tuple(fake.shape)}")
    if real.is_cuda != fake.is_cuda:
        raise ValueError(f"{who}: both activation sets must be on the host or both on the GPU")
    if real.is_cuda:
        return real.to(torch.float32).contiguous(), fake.to(device=real.device, dtype=torch.float32).contiguous()
    # the device reads the activations as float32; so does the host path, then computes in float64
    return real.to(torch.float32).to(torch.float64).contiguous(), fake.to(torch.float32).to(torch.float64).contiguous()


def _row_blocks(N, chunk_rows, rank, world):
    """-> (every block, this rank's blocks) as (lo, hi) row ranges: rank r owns rows N r / world ... N (r + 1) / world (the share of
    iter_activation_chunks), cut into pieces of chunk_rows rows.  Column blocks are EVERY rank's row blocks, so a rank's row block meets
    itself among the columns exactly once."""
    if chunk_rows is not None and int(chunk_rows) < 1:
        raise ValueError("chunk_rows must be positive")
    every, own = [], []
    for r in range(world):
        lo, hi = N * r // world, N * (r + 1) // world
        step = hi - lo if chunk_rows is None else int(chunk_rows)
        for s in range(lo, hi, max(step, 1)):
            blk = (s, min(s + step, hi))
            every.append(blk)
            if r == rank:
                own.append(blk)
    return every, own


def _all_reduce(t, grouped):
    if grouped:
        import torch.distributed as dist
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t


# ------------------------------------------------------------------ the three passes, device or host
def _poly_sum(x, y, sums, degree, gamma, coef0, diag):
    """sums [2] += (sum_ij k_ij, sum_i k_ii when diag), k_ij = (gamma x_i . y_j + coef0)^degree"""
    if x.is_cuda:
        from . import ops
        ops.pairs_poly_sum(x, y, sums, degree, gamma, coef0, diag)
        return
    t = gamma * (x @ y.t()) + coef0
    k = t.clone()
    for _ in range(1, degree):
        k *= t
    sums[0] += k.sum()
    if diag:
        sums[1] += k.diagonal().sum()


def _host_d2(x, y):
    """[n, m] squared distances by differences in float64: every entry depends on its own two rows alone, not on the blocking"""
    n, m, D = x.shape[0], y.shape[0], x.shape[1]
    out = torch.empty(n, m, dtype=torch.float64)
    rows = max(1, _HOST_D2_ELEMS // max(1, m * D))
    for r in range(0, n, rows):
        d = x[r:r + rows, None, :] - y[None, :, :]
        out[r:r + rows] = (d * d).sum(dim=-1)
    return out


def _knn(x, y, best):
    """best [n, kk] ascending <- the kk smallest of itself and the squared distances to the rows of y"""
    if x.is_cuda:
        from . import ops
        ops.pairs_knn(x, y, best)
        return
    both = torch.cat([best, _host_d2(x, y)], dim=1)
    best.copy_(both.sort(dim=1).values[:, :best.shape[1]])


def _ball_count(q, ref, radius2, count):
    """count [n] += #{ j : |q_i - ref_j|^2 <= radius2[j] }"""
    if q.is_cuda:
        from . import ops
        ops.pairs_ball_count(q, ref, radius2, count)
        return
    count += (_host_d2(q, ref) <= radius2[None, :]).sum(dim=1).to(count.dtype)


# ------------------------------------------------------------------ KID
def _kernel_sums(x, y, degree, gamma, coef0, chunk_rows, rank=0, world=1):
    """-> [3, 2] on x's device: (sum, trace) of Kxx, Kyy, Kxy.  The sums add over pairs of row blocks (this rank's row blocks against
    every column block); the trace is taken where a block meets itself."""
    n, m = x.shape[0], y.shape[0]
    sums = torch.zeros(3, 2, dtype=torch.float64, device=x.device)
    x_all, x_own = _row_blocks(n, chunk_rows, rank, world)
    y_all, y_own = _row_blocks(m, chunk_rows, rank, world)
    for lo, hi in x_own:
        for c0, c1 in x_all:
            _poly_sum(x[lo:hi], x[c0:c1], sums[0], degree, gamma, coef0, (lo, hi) == (c0, c1))
        for c0, c1 in y_all:
            _poly_sum(x[lo:hi], y[c0:c1], sums[2], degree, gamma, coef0, False)
    for lo, hi in y_own:
        for c0, c1 in y_all:
            _poly_sum(y[lo:hi], y[c0:c1], sums[1], degree, gamma, coef0, (lo, hi) == (c0, c1))
    return sums


def _mmd2(s, n, m):
    """MMD²_u = (S Kxx - tr Kxx) / (n (n - 1)) + (S Kyy - tr Kyy) / (m (m - 1)) - 2 S Kxy / (n m) from the host copy of the sums"""
    return float((s[0, 0] - s[0, 1]) / (n * (n - 1.0)) + (s[1, 0] - s[1, 1]) / (m * (m - 1.0)) - 2.0 * s[2, 0] / (float(n) * m))


def kid_subset_indices(n_real, n_fake, subsets, subset_size, seed):
    """The rows of every subset, in the order kid_from_activations draws them: rng = np.random.RandomState(seed); per subset FIRST
    rng.choice(n_real, subset_size, replace=False), THEN rng.choice(n_fake, subset_size, replace=False)."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(subsets):
        ir = rng.choice(n_real, subset_size, replace=False)
        out.append((ir, rng.choice(n_fake, subset_size, replace=False)))
    return out


def kid_from_activations(real, fake, subsets=100, subset_size=1000, seed=0, degree=3, gamma=None, coef0=1.0, chunk_rows=None):
    """Kernel Inception Distance between two activation sets -> {"kid", "kid_std", "subsets", "subset_size"}.
    One estimate is MMD²_u with k(x, y) = (gamma x.y + coef0)^degree (gamma None = 1 / D).  subsets > 0: mean and standard deviation
    (divisor = subsets) of the estimates over `subsets` draws of subset_size rows from each set, drawn as kid_subset_indices documents;
    a subset_size above the smaller set is clamped, with a warning.  subsets = 0: the estimate over the two full sets, one value,
    kid_std None.  chunk_rows streams the sets in row blocks.  Under an initialised process group the subsets (or, for the full sets,
    the row blocks) are divided over the ranks and the results all-reduced; every rank returns the same values."""
    x, y = _prepare(real, fake, "kid_from_activations")
    n, m, D = x.shape[0], y.shape[0], x.shape[1]
    subsets, subset_size, degree = int(subsets), int(subset_size), int(degree)
    if n < 2 or m < 2:
        raise ValueError("kid_from_activations: need at least 2 rows in each set")
    if subsets < 0 or not 1 <= degree <= 8 or (subsets > 0 and subset_size < 2):
        raise ValueError("kid_from_activations: need subsets >= 0, subset_size >= 2 and 1 <= degree <= 8")
    gamma = 1.0 / D if gamma is None else float(gamma)
    coef0 = float(coef0)
    rank, world, grouped = _dist_rank_world()
    if subsets == 0:
        s = _all_reduce(_kernel_sums(x, y, degree, gamma, coef0, chunk_rows, rank, world), grouped).cpu().numpy()
        return {"kid": _mmd2(s, n, m), "kid_std": None, "subsets": 0, "subset_size": None}
    if subset_size > min(n, m):
        warnings.warn(f"kid_from_activations: subset_size {subset_size} is above the smaller set; using {min(n, m)}")
        subset_size = min(n, m)
    sums = torch.zeros(subsets, 3, 2, dtype=torch.float64, device=x.device)   # one copy back for all subsets, not one each
    for t, (ir, jf) in enumerate(kid_subset_indices(n, m, subsets, subset_size, seed)):
        if t % world != rank:
            continue
        xs = x[torch.from_numpy(ir).to(x.device)]
        ys = y[torch.from_numpy(jf).to(y.device)]
        sums[t] = _kernel_sums(xs, ys, degree, gamma, coef0, chunk_rows)
    v = np.array([_mmd2(s, subset_size, subset_size) for s in _all_reduce(sums, grouped).cpu().numpy()])
    return {"kid": float(v.mean()), "kid_std": float(v.std()), "subsets": subsets, "subset_size": subset_size}


# ------------------------------------------------------------------ precision / recall / density / coverage
def _radii(x, k, every, own, grouped):
    """r[i] = squared distance of x_i to its k-th nearest OTHER row: entry k of the (k + 1)-list that includes the row itself"""
    r = torch.zeros(x.shape[0], dtype=torch.float64, device=x.device)
    for lo, hi in own:
        best = torch.full((hi - lo, k + 1), float("inf"), dtype=torch.float64, device=x.device)
        for c0, c1 in every:
            _knn(x[lo:hi], x[c0:c1], best)
        r[lo:hi] = best[:, k]
    return _all_reduce(r, grouped)   # every rank wrote its slice of a zero vector


def prdc_from_activations(real, fake, k=3, chunk_rows=None):
    """Improved precision / recall and density / coverage -> {"precision", "recall", "density", "coverage", "k"}.
    r_real[i] (r_fake[j]) = squared distance to the k-th nearest other row of the same set.  With count_j = #{ i : |fake_j - real_i|²
    <= r_real[i] }: precision = mean_j [count_j > 0], density = S_j count_j / (k M); recall is precision with the roles swapped;
    coverage = mean_i [min_j |real_i - fake_j|² <= r_real[i]].  chunk_rows streams the sets in row blocks; under an initialised process
    group every rank takes its row share, the radii, counts and hits are all-reduced and every rank returns the same values."""
    x, y = _prepare(real, fake, "prdc_from_activations")
    k = int(k)
    n, m = x.shape[0], y.shape[0]
    if not 1 <= k <= 15:
        raise ValueError("prdc_from_activations: k outside 1..15")
    if n <= k or m <= k:
        raise ValueError(f"prdc_from_activations: need more than k = {k} rows in each set, got {n} and {m}")
    rank, world, grouped = _dist_rank_world()
    x_all, x_own = _row_blocks(n, chunk_rows, rank, world)
    y_all, y_own = _row_blocks(m, chunk_rows, rank, world)
    r_real = _radii(x, k, x_all, x_own, grouped)
    r_fake = _radii(y, k, y_all, y_own, grouped)
    hits = torch.zeros(4, dtype=torch.int64, device=x.device)   # fakes inside a real ball, S count, reals inside a fake ball, covered reals
    for lo, hi in y_own:
        cnt = torch.zeros(hi - lo, dtype=torch.int32, device=x.device)
        for c0, c1 in x_all:
            _ball_count(y[lo:hi], x[c0:c1], r_real[c0:c1], cnt)
        hits[0] += (cnt > 0).sum()
        hits[1] += cnt.sum(dtype=torch.int64)
    for lo, hi in x_own:
        cnt = torch.zeros(hi - lo, dtype=torch.int32, device=x.device)
        nearest = torch.full((hi - lo, 1), float("inf"), dtype=torch.float64, device=x.device)
        for c0, c1 in y_all:
            _ball_count(x[lo:hi], y[c0:c1], r_fake[c0:c1], cnt)
            _knn(x[lo:hi], y[c0:c1], nearest)
        hits[2] += (cnt > 0).sum()
        hits[3] += (nearest[:, 0] <= r_real[lo:hi]).sum()
    h = _all_reduce(hits, grouped).cpu().numpy()
    return {"precision": float(h[0]) / m, "recall": float(h[2]) / n, "density": float(h[1]) / (float(k) * m),
            "coverage": float(h[3]) / n, "k": k}


# ------------------------------------------------------------------ evaluate.py calc on saved activations
def _log(output_file, *values):
    import datetime
    with open(output_file, "a") as f:   # the shape of the FID line: "\n <iso time> <values>\n "
        print("\n", datetime.datetime.now().isoformat(), *values, end="\n ", file=f)


def calc_kid(act_path, real_act_path, output_file, subsets=100, subset_size=1000, seed=0, chunk_rows=None):
    """KID of the activations at act_path against the real activations at real_act_path: "KID: <value> +- <std>" on stdout and one
    line "<iso time> <value> <std>" appended to output_file (rank 0 alone prints and logs)."""
    from .fid import load_activations
    res = kid_from_activations(load_activations(real_act_path), load_activations(act_path), subsets=subsets, subset_size=subset_size,
                               seed=seed, chunk_rows=chunk_rows)
    if _dist_rank_world()[0] == 0:
        print("KID: %s +- %s" % (res["kid"], res["kid_std"]))
        _log(output_file, res["kid"], res["kid_std"])
    return res


def calc_prdc(act_path, real_act_path, output_file, k=3, chunk_rows=None):
    """precision / recall / density / coverage of the activations at act_path against the real activations at real_act_path: one
    stdout line and one line "<iso time> <precision> <recall> <density> <coverage>" appended to output_file (rank 0 alone)."""
    from .fid import load_activations
    res = prdc_from_activations(load_activations(real_act_path), load_activations(act_path), k=k, chunk_rows=chunk_rows)
    if _dist_rank_world()[0] == 0:
        print("PRDC: precision %s recall %s density %s coverage %s" % (res["precision"], res["recall"], res["density"], res["coverage"]))
        _log(output_file, res["precision"], res["recall"], res["density"], res["coverage"])
    return res
