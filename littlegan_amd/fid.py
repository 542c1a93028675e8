"""Fréchet-distance arithmetic of the FID pass (/root/reference/fid.py:112-163 and :185-188).

Only the arithmetic: d^2 = |mu1 - mu2|^2 + tr(S1 + S2 - 2 (S1 S2)^(1/2)).  The Inception pool_3 activations it is
normally fed with need a frozen graph that the reference downloads (fid.py:276) and this pipeline cannot obtain, so
the entry points take activation matrices.  The O(N D^2) part (mean and covariance of [N, D] activations) runs on the
device in fp64 (in-tree kernel on the fp64 matrix instruction, csrc/fid.hip); the D x D matrix square root stays on the host (scipy), as in the reference,
unless asked for on the device (frechet_distance_ns: coupled Newton-Schulz iteration in fp64, csrc/fid_sqrt.hip).  ActivationAccumulator
streams the statistics batch by batch and merges them over ranks (lg_fid_accum / lg_fid_finalize)."""
import warnings

import numpy as np
import torch


def activation_statistics(act: torch.Tensor):
    """fid.py:185-188: mu = mean over samples, sigma = np.cov(act, rowvar=False) (divisor N - 1).  act [N, D].
    On the GPU this is the in-tree fp64-MFMA kernel (csrc/fid.hip, lg_fid_stats); a host tensor (tests, tiny inputs) is
    reduced with torch in float64."""
    if act.dim() != 2 or act.shape[0] < 2:
        raise ValueError("activation_statistics: need an [N >= 2, D] matrix")
    if act.is_cuda:
        from . import ops
        mu, sigma = ops.fid_stats(act.to(torch.float32).contiguous())
        return mu.cpu().numpy(), sigma.cpu().numpy()
    a = act.to(torch.float64)
    mu = a.mean(dim=0)
    c = a - mu
    sigma = (c.t() @ c) / (a.shape[0] - 1)
    return mu.cpu().numpy(), sigma.cpu().numpy()


def frechet_distance(mu1, sigma1, mu2, sigma2, eps: float = 1e-6) -> float:
    """fid.py:112-163.  Same guards as the reference: a non-finite square root of the product retries with eps on both
    diagonals (with a warning); a complex result is accepted only if its diagonal is real to 1e-3."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, np.float64)), np.atleast_1d(np.asarray(mu2, np.float64))
    s1, s2 = np.atleast_2d(np.asarray(sigma1, np.float64)), np.atleast_2d(np.asarray(sigma2, np.float64))
    if mu1.shape != mu2.shape:
        raise ValueError("frechet_distance: mean vectors have different lengths")
    if s1.shape != s2.shape:
        raise ValueError("frechet_distance: covariances have different dimensions")
    root = linalg.sqrtm(s1 @ s2)
    if isinstance(root, tuple):  # old scipy returns (sqrtm, error estimate) when disp=False; be liberal
        root = root[0]
    if not np.isfinite(root).all():
        warnings.warn(f"fid calculation produces singular product; adding {eps} to diagonal of cov estimates")
        ridge = np.eye(s1.shape[0]) * eps
        root = linalg.sqrtm((s1 + ridge) @ (s2 + ridge))
    if np.iscomplexobj(root):
        if not np.allclose(np.diagonal(root).imag, 0.0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(root.imag))}")
        root = root.real
    d = mu1 - mu2
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * np.trace(root))


def fid_from_activations(act_a: torch.Tensor, act_b: torch.Tensor) -> float:
    """FID between two activation sets (what evaluate.py computes once the Inception features exist)."""
    m1, s1 = activation_statistics(act_a)
    m2, s2 = activation_statistics(act_b)
    return frechet_distance(m1, s1, m2, s2)


# ------------------------------------------------------------------ streaming, mergeable statistics
def _tile_index(D):
    nt = (D + 63) // 64
    return nt, torch.triu_indices(nt, nt)   # row-major over (ti <= tj): the tile numbering of lg_fid_accum


def _pack_tiles(full):
    """[D, D] fp64 -> the packed upper-triangular 64 x 64 tile image of lg_fid_accum (entries past D are 0)"""
    D = full.shape[0]
    nt, iu = _tile_index(D)
    pad = torch.zeros(nt * 64, nt * 64, dtype=torch.float64)
    pad[:D, :D] = full
    return pad.view(nt, 64, nt, 64).permute(0, 2, 1, 3)[iu[0], iu[1]].reshape(-1).clone()


def _unpack_tiles(gram, D):
    """packed tiles -> [D, D] with the upper-triangular tiles filled (the strictly lower tiles are 0)"""
    nt, iu = _tile_index(D)
    t4 = torch.zeros(nt, nt, 64, 64, dtype=torch.float64)
    t4[iu[0], iu[1]] = gram.view(-1, 64, 64)
    return t4.permute(0, 2, 1, 3).reshape(nt * 64, nt * 64)[:D, :D]


class ActivationAccumulator:
    """fid.py:185-188 batch by batch and rank by rank.  State, all fp64 on `device`: count (host integer), shift c [D] (fixed at
    creation, default zeros), sum = S (x - c), gram = S (x - c)(x - c)^T as packed upper-triangular 64 x 64 tiles.  Every field but c
    is a plain sum over samples: accumulators with the same c merge by addition, a group of ranks with one all-reduce (SUM).
    finalize: mu = c + sum / N, sigma = (gram - sum sum^T / N) / (N - 1), exactly symmetric.

    The shift is there because the uncentred form cancels: with c = 0 about log10(mean^2 / var) of the 16 decimal digits of sigma are
    lost (mean = 1e4 std: 8 digits).  A shift near the mean (calc passes the pre-calculated mu of the real set) keeps them.
    CUDA state runs the in-tree kernels (lg_fid_accum / lg_fid_finalize); host state the same formulas in torch float64."""

    def __init__(self, D, device="cpu", shift=None):
        self.D = int(D)
        if self.D < 1:
            raise ValueError("ActivationAccumulator: D must be positive")
        self.device = torch.device(device)
        self.count = 0
        from .ops import fid_gram_elems
        if shift is None:
            self.shift = None
        else:
            self.shift = torch.as_tensor(shift).to(device=self.device, dtype=torch.float64).contiguous()
            if tuple(self.shift.shape) != (self.D,):
                raise ValueError(f"ActivationAccumulator: shift has shape {tuple(self.shift.shape)}, need ({self.D},)")
        self.sum = torch.zeros(self.D, dtype=torch.float64, device=self.device)
        self.gram = torch.zeros(fid_gram_elems(self.D), dtype=torch.float64, device=self.device)

    def update(self, act):
        """add the rows of act [n, D] (any float dtype; read as float32 on the device, as lg_fid_stats does)"""
        if act.dim() != 2 or act.shape[1] != self.D:
            raise ValueError(f"ActivationAccumulator.update: need an [n, {self.D}] matrix, got {tuple(act.shape)}")
        if act.shape[0] == 0:
            return self
        if self.device.type == "cuda":
            from . import ops
            ops.fid_accum(act.to(device=self.device, dtype=torch.float32).contiguous(), self.sum, self.gram, self.shift)
        else:
            x = act.to(device="cpu", dtype=torch.float64)
            if self.shift is not None:
                x = x - self.shift
            self.sum += x.sum(dim=0)
            self.gram += _pack_tiles(x.t() @ x)
        self.count += int(act.shape[0])
        return self

    def _same_shift(self, other):
        if (self.shift is None) != (other.shift is None):
            return False
        return self.shift is None or torch.equal(self.shift.cpu(), other.shift.cpu())

    def merge(self, other):
        """add another accumulator's samples (same D, same shift)"""
        if other.D != self.D:
            raise ValueError(f"ActivationAccumulator.merge: D {other.D} != {self.D}")
        if not self._same_shift(other):
            raise ValueError("ActivationAccumulator.merge: the accumulators were created with different shifts")
        self.sum += other.sum.to(self.device)
        self.gram += other.gram.to(self.device)
        self.count += other.count
        return self

    def all_reduce(self, group=None):
        """sum the state over the ranks of `group` (every rank must hold the same shift); gloo and RCCL both carry doubles"""
        import torch.distributed as dist
        n = torch.tensor([self.count], dtype=torch.int64, device=self.device)
        dist.all_reduce(n, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self.sum, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self.gram, op=dist.ReduceOp.SUM, group=group)
        self.count = int(n.item())
        return self

    def finalize(self):
        """-> (mu [D], sigma [D, D]) as numpy float64; sigma == sigma.T bit for bit"""
        if self.count < 2:
            raise ValueError("ActivationAccumulator.finalize: need at least 2 samples")
        if self.device.type == "cuda":
            from . import ops
            mu, sigma = ops.fid_finalize(self.sum, self.gram, self.count, self.shift)
            return mu.cpu().numpy(), sigma.cpu().numpy()
        n = float(self.count)
        mu = self.sum / n if self.shift is None else self.shift + self.sum / n
        up = torch.triu(_unpack_tiles(self.gram, self.D))
        g = up + torch.triu(up, 1).t()
        sigma = (g - torch.outer(self.sum, self.sum) / n) / (n - 1.0)
        return mu.numpy(), sigma.numpy()


def _activation_segments(path):
    """the [n_i, D] arrays (memory-mapped where the format allows) that `path` holds, in row order"""
    import glob
    import os
    if os.path.isdir(path):
        shards = sorted(glob.glob(os.path.join(path, "activations-*.npy")))
        files = shards if shards else [os.path.join(path, "activations.npy")]
    else:
        files = [path]
    segs = []
    for f in files:
        a = np.load(f, mmap_mode="r")
        if hasattr(a, "files"):
            a = a["act"] if "act" in a.files else a[a.files[0]]
        if a.ndim != 2:
            raise ValueError(f"{f}: need an [N, D] activation matrix, got {a.shape}")
        if segs and a.shape[1] != segs[0].shape[1]:
            raise ValueError(f"{f}: {a.shape[1]} features, the shards before it have {segs[0].shape[1]}")
        segs.append(a)
    return segs


def iter_activation_chunks(path, rows, rank=0, world=1):
    """Yields [<= rows, D] float32 blocks of rank `rank`'s contiguous share (rows N rank / world ... N (rank + 1) / world) of the
    activations at `path`: what load_activations accepts (.npy opened memory-mapped, .npz, a directory holding activations.npy) or a
    directory of activations-*.npy shards (sorted by name).  The shares of all ranks cover every row exactly once."""
    rows = int(rows)
    if rows < 1 or not 0 <= rank < world:
        raise ValueError("iter_activation_chunks: need rows >= 1 and 0 <= rank < world")
    segs = _activation_segments(path)
    total = sum(a.shape[0] for a in segs)
    lo, hi = total * rank // world, total * (rank + 1) // world
    base = 0
    for a in segs:
        s, e = max(lo, base) - base, min(hi, base + a.shape[0]) - base
        for r in range(s, e, rows):
            yield np.array(a[r:min(r + rows, e)], dtype=np.float32)   # a copy: the block outlives the memory map
        base += a.shape[0]


def _dist_rank_world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size(), True
    return 0, 1, False


def streamed_statistics(path, chunk_rows, shift=None):
    """activation_statistics of the activations at `path`, streamed in blocks of chunk_rows rows through an ActivationAccumulator
    (on the GPU when there is one).  With a process group initialised every rank streams its own share and the group all-reduces."""
    rank, world, grouped = _dist_rank_world()
    segs = _activation_segments(path)
    D = segs[0].shape[1]
    if sum(a.shape[0] for a in segs) < 2:
        raise ValueError(f"{path}: need an [N >= 2, D] activation matrix")
    acc = ActivationAccumulator(D, "cuda" if torch.cuda.is_available() else "cpu", shift)
    for blk in iter_activation_chunks(path, chunk_rows, rank, world):
        acc.update(torch.from_numpy(blk))
    if grouped:
        acc.all_reduce()
    return acc.finalize()


# ------------------------------------------------------------------ tr sqrt(S1 S2) without the host sqrtm
def newton_schulz_trace(s1, s2, max_iter=100):
    """numpy fp64 restatement of lg_fid_distance's iteration and stopping rule -> (tr sqrt(S1 S2), iterations, status).
    c = |A|_F, Y0 = A / c, Z0 = I; T = (3 I - Z Y) / 2, Y <- Y T, Z <- T Z; t_k = sqrt(c) tr Y_k.  Stops with t_k when
    |t_k - t_{k-1}| <= 1e-12 |t_k|, with t_{k-1} when the step has stopped shrinking while <= 1e-5 |t_k| (the rounding floor, reached
    early when S1 S2 is rank-deficient; past it Z grows in the null space and the iteration diverges).  status 1 = not converged."""
    a = s1 @ s2
    c = float(np.sqrt((a * a).sum()))
    if not np.isfinite(c):
        return c, 0, 1
    if c == 0.0:
        return 0.0, 0, 0
    n = a.shape[0]
    y, z, eye = a / c, np.eye(n), np.eye(n)
    sc = np.sqrt(c)
    t_prev, d_prev = sc * np.trace(y), np.inf
    t_out = t_prev
    with np.errstate(all="ignore"):
        for k in range(1, int(max_iter) + 1):
            t_mat = 1.5 * eye - 0.5 * (z @ y)
            y, z = y @ t_mat, t_mat @ z
            t = sc * np.trace(y)
            if not np.isfinite(t):
                return float(t_prev), k, 1
            d = abs(t - t_prev)
            if d <= 1e-12 * abs(t):
                return float(t), k, 0
            if d >= d_prev and d <= 1e-5 * abs(t):
                return float(t_prev), k, 0
            t_prev, d_prev, t_out = t, d, t
    return float(t_out), int(max_iter), 1


def frechet_distance_ns(mu1, sigma1, mu2, sigma2, device=None, max_iter=100):
    """frechet_distance with tr sqrt(S1 S2) by the coupled Newton-Schulz iteration in fp64: on the GPU (lg_fid_distance) when `device`
    is a CUDA device, else its numpy restatement.  -> (d2, info) with info = {tr_sqrt, iterations, status, fallback}.
    When the iteration does not converge (status 1) it warns and returns frechet_distance's value (scipy, the reference's guards)."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, np.float64)), np.atleast_1d(np.asarray(mu2, np.float64))
    s1, s2 = np.atleast_2d(np.asarray(sigma1, np.float64)), np.atleast_2d(np.asarray(sigma2, np.float64))
    if mu1.shape != mu2.shape:
        raise ValueError("frechet_distance_ns: mean vectors have different lengths")
    if s1.shape != s2.shape:
        raise ValueError("frechet_distance_ns: covariances have different dimensions")
    if mu1.ndim != 1 or s1.shape != (mu1.shape[0], mu1.shape[0]):
        raise ValueError("frechet_distance_ns: need [D] means and [D, D] covariances")
    if device is not None and torch.device(device).type == "cuda":
        from . import ops
        dev = torch.device(device)
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (mu1, s1, mu2, s2)]
        d2, tr, iters, status = ops.fid_distance(*t, max_iter=max_iter)
    else:
        tr, iters, status = newton_schulz_trace(s1, s2, max_iter)
        d = mu1 - mu2
        d2 = float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * tr)
    info = {"tr_sqrt": tr, "iterations": iters, "status": status, "fallback": False}
    if status != 0:
        warnings.warn(f"frechet_distance_ns: the iteration did not converge in {iters} iterations; using the host matrix square root")
        info["fallback"] = True
        d2 = frechet_distance(mu1, s1, mu2, s2)
    return d2, info


# ------------------------------------------------------------------ evaluate.py:29-59 on saved activations
def load_activations(path: str) -> torch.Tensor:
    """[N, D] float32 Inception pool_3 activations from `path`: an .npy / .npz file (key "act", else its first array), or a
    directory holding activations.npy.  The reference computes them from the JPEGs of `image_path` with a frozen Inception graph
    it downloads (evaluate.py:45-46,53-55, fid.py:36-106,276); that graph cannot be obtained in this pipeline, so the entry points
    below start from the activations a user has saved."""
    import os
    if os.path.isdir(path):
        path = os.path.join(path, "activations.npy")
    a = np.load(path)
    if hasattr(a, "files"):
        a = a["act"] if "act" in a.files else a[a.files[0]]
    a = np.asarray(a, np.float32)
    if a.ndim != 2 or a.shape[0] < 2:
        raise ValueError(f"{path}: need an [N >= 2, D] activation matrix, got {a.shape}")
    t = torch.from_numpy(a)
    return t.cuda() if torch.cuda.is_available() else t


def pre_calculate(act_path: str, stats_path: str, chunk_rows=None, device_sqrt=False):
    """evaluate.py `pre-calculate` (:29-42): statistics of the real images' activations -> stats npz {mu, sigma}.
    chunk_rows streams the activations in blocks of that many rows (shift = the mean of the first block, which every rank reads for
    itself; all-reduced over an initialised process group, rank 0 alone writes).  device_sqrt is accepted for symmetry with calc:
    this mode takes no square root."""
    if chunk_rows is None:
        mu, sigma = activation_statistics(load_activations(act_path))
        rank = 0
    else:
        first = next(iter_activation_chunks(act_path, chunk_rows))
        mu, sigma = streamed_statistics(act_path, chunk_rows, shift=first.astype(np.float64).mean(0))
        rank = _dist_rank_world()[0]
    if rank == 0:
        np.savez_compressed(stats_path, mu=mu, sigma=sigma)
        print("finished")
    return mu, sigma


def calc(act_path: str, stats_path: str, output_file: str, chunk_rows=None, device_sqrt=False) -> float:
    """evaluate.py `calc` (:43-59): statistics of the generated images' activations (on the device: lg_fid_stats), the Frechet
    distance to the pre-calculated statistics, "FID: <value>" on stdout and one line appended to the log in the reference's
    format ("\\n <iso time> <value>\\n ").
    chunk_rows streams the activations through an ActivationAccumulator shifted by the stored mu (each rank of an initialised process
    group its own share, all-reduced; rank 0 alone prints and logs); device_sqrt takes the square root by frechet_distance_ns."""
    import datetime
    with np.load(stats_path) as f:
        mu_real, sigma_real = f["mu"][:], f["sigma"][:]
    if chunk_rows is None:
        mu_gen, sigma_gen = activation_statistics(load_activations(act_path))
        rank = 0
    else:
        mu_gen, sigma_gen = streamed_statistics(act_path, chunk_rows, shift=mu_real)
        rank = _dist_rank_world()[0]
    if device_sqrt:
        fid_value, _ = frechet_distance_ns(mu_gen, sigma_gen, mu_real, sigma_real, device="cuda" if torch.cuda.is_available() else None)
    else:
        fid_value = frechet_distance(mu_gen, sigma_gen, mu_real, sigma_real)
    if rank == 0:
        print("FID: %s" % fid_value)
        with open(output_file, "a") as f:
            print("\n", datetime.datetime.now().isoformat(), fid_value, end="\n ", file=f)
    return fid_value
