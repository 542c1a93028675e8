"""The norm kernels (littlegan_amd/csrc/norm.hip) in exact arithmetic at every launch-geometry edge.

The library is built with -ffp-contract=off and the norm passes use no division or transcendental per element, so every element-wise
result can be restated in numpy float32, one operation per line, and compared BIT FOR BIT.  Two forms of operands:

  * exact apply form: z integers in [-8, 8], skip integers in [-4, 4], hand-made statistics records {mu_hi, sigma, a, beta, mu_lo}
    (a fixed cycle over the samples: mu_hi integer, mu_lo in {0, +-2^-5}, a in {0.5, 1, 2}, beta = k/64).  Then
    [leaky](a(([leaky](z) - mu_hi) - mu_lo) + beta) [+ skip], evaluated step by step in float32, IS the fp64 value
    (tests/test_norm_exact_cpu.py), a share of the values are exact bf16 ties in both directions, and the bf16 stores must equal the
    round-to-nearest-even of the exact value.
  * backward: the per-sample sums s1 = sum dz', s2 = sum dz' c are exact in any order (integers times a power of two below 2^24), the
    finaliser's fp64 lines are restated in numpy fp64, dx in numpy float32.  The BALANCED form (second half of a sample = the first
    with the channels rotated by C/2 and g negated) has s1 = s2 = 0, so dx = a dz' and the bias column sums db are exact too.

Every case asserts the kernels it launched and their grids (ops.last_norm_launches), recomputed here from B, L, C and the CU count;
where a grid was cut to whole residency rounds the residency is read back from the grid itself.  The case table below is plain data:
tests/test_norm_exact_cpu.py checks its conditions on the oracle alone and holds the ledger of launched kernel names.

Operands are drawn iid per element from default_rng(crc32(shape id)); the forms of one shape share them."""
import math
import os
import sys
import zlib
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

F32, F64 = np.float32, np.float64
ALPHA = 0.25
A32 = F32(ALPHA)
EPS = float(F32(1e-3))          # LG_IN_EPS as the kernels see it: the float constant, widened
GAMMA, BETA = 1.25, -0.375      # scalar affine of the moment cases (exact in fp32)
ROWS_PER_BLOCK = 1 << 22        # the restatements walk large maps in blocks of whole samples of about this many elements

# ---------------------------------------------------------------------------------------------------------------- operands
MU_HI = np.array([-2, -1, 0, 1, 2], F32)
MU_LO = np.array([0, 2.0 ** -5, -2.0 ** -5], F32)
A_CYC = np.array([1, 2, 0.5, 2, 1, 0.5, 2], F32)
BETA_K = np.array([1, -3, 16, 37, -64, 0, 21, -11, 64, -27, 5])
SIGMA = np.array([1.5, 2.25, 3.0, 4.75], F32)


def records(B):
    """[B, 8] hand-made statistics records {mu_hi, sigma, a, beta, mu_lo, 0, 0, 0}: a fixed cycle (periods 5, 4, 7, 11, 3), not drawn"""
    n = np.arange(B)
    rec = np.zeros((B, 8), F32)
    rec[:, 0], rec[:, 1], rec[:, 2] = MU_HI[n % 5], SIGMA[n % 4], A_CYC[n % 7]
    rec[:, 3], rec[:, 4] = (BETA_K[n % 11] / 64.0).astype(F32), MU_LO[n % 3]
    return rec


@lru_cache(maxsize=3)
def operands(B, L):
    """(z in [-8, 8], g in [-4, 4], skip in [-4, 4]) as int8 [B, L]"""
    rng = np.random.default_rng(zlib.crc32(f"norm-exact-{B}x{L}".encode()))
    return tuple(rng.integers(-k, k + 1, (B, L), dtype=np.int8) for k in (8, 4, 4))


@lru_cache(maxsize=2)
def balanced_operands(B, P, C, gdiv):
    """(z, g) [B, P*C] float32: rows [P/2, P) repeat rows [0, P/2) with the channel index rotated by C/2 and g negated;
    g = integers in [-4 gdiv, 4 gdiv] / gdiv.  The column sums of dx = a dz' (post-LeakyReLU form under records(B)) must all be non-zero,
    or a kernel that lost a column would go unnoticed: where a drawn column sums to zero, g of sample 0, position 0 in that column is
    moved by one unit (towards zero from the ends of its range), and the check is repeated."""
    rng = np.random.default_rng(zlib.crc32(f"norm-balanced-{B}x{P}x{C}/{gdiv}".encode()))
    zh = rng.integers(-8, 9, (B, P // 2, C)).astype(F32)
    gk = rng.integers(-4 * gdiv, 4 * gdiv + 1, (B, P // 2, C))
    rec = records(B)
    for _ in range(4 * C):
        gh = (gk / F64(gdiv)).astype(F32)
        z = np.concatenate([zh, np.roll(zh, C // 2, axis=2)], 1).reshape(B, -1)
        g = np.concatenate([gh, -np.roll(gh, C // 2, axis=2)], 1).reshape(B, -1) + F32(0)   # (no negative zeros)
        _, dz, _ = _c_dz(z, g, rec, 0, 1, None, 0, B)
        zero = np.flatnonzero((rec[:, 2:3] * dz).reshape(-1, C).sum(0, dtype=F64) == 0)
        if not zero.size:
            return z, g
        c = zero[0]
        gk[0, 0, c] += 1 if gk[0, 0, c] < 4 * gdiv else -1
    raise AssertionError("balanced operands: a zero column sum is left")


def bf16_bits(v):
    """uint16 bit patterns of the round-to-nearest-even bf16 of a float32 array"""
    u = np.ascontiguousarray(v, F32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


# ------------------------------------------------------------------------------------------------------------ restatements
def leaky32(x):
    return np.where(x > 0, x, A32 * x)


def _rows(B, L):
    step = max(1, ROWS_PER_BLOCK // L)
    return [(lo, min(B, lo + step)) for lo in range(0, B, step)]


def apply32(z, rec, pre, post, skip=None, mult=None):
    """the apply pass, one float32 operation per line, as apply_body / apply16_body / apply16p_body write it"""
    B, L = z.shape
    out = np.empty((B, L), F32)
    for lo, hi in _rows(B, L):
        mu, a, b, mul = (rec[lo:hi, i:i + 1] for i in (0, 2, 3, 4))
        t = z[lo:hi].astype(F32)
        if pre:
            t = leaky32(t)
        t = t - mu
        t = t - mul
        t = a * t
        t = t + b
        if post:
            t = leaky32(t)
        if mult is not None:
            t = t * mult[lo:hi]
        if skip is not None:
            t = t + skip[lo:hi].astype(F32)
        assert t.dtype == F32
        out[lo:hi] = t
    return out


def apply64(z, rec, pre, post, skip=None, mult=None):
    """the same map in fp64 with mu = mu_hi + mu_lo: the exact value"""
    r = rec.astype(F64)
    t = z.astype(F64)
    if pre:
        t = np.where(t > 0, t, ALPHA * t)
    t = r[:, 2:3] * (t - (r[:, 0:1] + r[:, 4:5])) + r[:, 3:4]
    if post:
        t = np.where(t > 0, t, ALPHA * t)
    if mult is not None:
        t = t * mult
    if skip is not None:
        t = t + skip
    return t


def bwd_sums(z, g, rec, pre, post, mult=None):
    """(s1, s2) [B] fp64 = sum dz', sum dz' c per sample; dz' c is formed in float32 as the kernels form it (exact for these operands)"""
    B, L = z.shape
    s1, s2 = np.empty(B, F64), np.empty(B, F64)
    for lo, hi in _rows(B, L):
        c, dz, _ = _c_dz(z, g, rec, pre, post, mult, lo, hi)
        s1[lo:hi] = dz.sum(1, dtype=F64)
        s2[lo:hi] = (dz * c).sum(1, dtype=F64)
    return s1, s2


def _c_dz(z, g, rec, pre, post, mult, lo, hi):
    mu, a, b, mul = (rec[lo:hi, i:i + 1] for i in (0, 2, 3, 4))
    x0 = z[lo:hi].astype(F32)
    xx = leaky32(x0) if pre else x0
    c = xx - mu
    c = c - mul
    dz = g[lo:hi].astype(F32)
    if mult is not None:
        dz = dz * mult[lo:hi]
    if post:
        y = a * c
        y = y + b
        dz = np.where(y > 0, dz, A32 * dz)
    return c, dz, x0


def bwd_coef(s1, s2, rec, L):
    """[B, 4] float32 {m1_hi, m2'_hi, m1_lo, m2'_lo} and the per-sample dgamma terms, in fp64 exactly as bwd_final_kernel writes them"""
    sigma = rec[:, 1].astype(F64)
    s = sigma + F64(EPS)
    with np.errstate(invalid="ignore", divide="ignore"):
        m1 = s1 / F64(L)
        m2 = s2 / F64(L) / (s * sigma)
        m1h, m2h = m1.astype(F32), m2.astype(F32)
        m = np.stack([m1h, m2h, (m1 - m1h.astype(F64)).astype(F32), (m2 - m2h.astype(F64)).astype(F32)], 1)
    return m, s2 / s


def bwd32(z, g, rec, pre, post, mult=None, sums=None):
    """the norm backward: dx [B, L] float32 one operation per line as bwd_apply_body / bwd_apply16_body write it, the coefficient
    records m [B, 4], and the exact fp64 (dgamma, dbeta)"""
    B, L = z.shape
    s1, s2 = bwd_sums(z, g, rec, pre, post, mult) if sums is None else sums
    m, dg = bwd_coef(s1, s2, rec, L)
    dx = np.empty((B, L), F32)
    for lo, hi in _rows(B, L):
        c, dz, x0 = _c_dz(z, g, rec, pre, post, mult, lo, hi)
        m1, m2, m1l, m2l = (m[lo:hi, i:i + 1] for i in range(4))
        t = dz - m1
        t = t - m1l
        t = t - c * m2
        t = t - c * m2l
        d = rec[lo:hi, 2:3] * t
        if pre:
            d = np.where(x0 > 0, d, A32 * d)
        assert d.dtype == F32
        dx[lo:hi] = d
    return dx, m, math.fsum(dg), math.fsum(s1), (s1, s2)


def colsums(dx, C):
    """(fp64 column sums, largest absolute column mass) of dx viewed as [.., C]"""
    d = dx.reshape(-1, C)
    return d.sum(0, dtype=F64), float(np.abs(d).sum(0, dtype=F64).max())


def exact_moments(k, unit_den, pre):
    """per-sample (mean, population sigma) of x = k / unit_den (k integers), after LeakyReLU(0.25) if pre, from exact integer sums:
    Fractions, rounded once to fp64 (the square root adds at most one more fp64 rounding)"""
    out = []
    for row in np.asarray(k, np.int64):
        v = np.where(row > 0, 4 * row, row) if pre else 4 * row        # units of 1 / (4 unit_den)
        n, s, q = int(v.size), int(v.sum()), int((v * v).sum())
        den = 4 * unit_den
        mean = Fraction(s, n * den)
        var = Fraction(n * q - s * s, n * n * den * den)
        out.append((float(mean), math.sqrt(float(var))))
    return np.array(out, F64)


P_OFFSET = 4096.0   # the apply16p cases sit at a mean near 4096: mu_lo (up to 2^-12 there) then moves every z - mu_hi by many ulps
P_STEP = 32.0       # ... and their z = 4096 + 32 k, k integers in [-8, 8], is exact in bf16


def handmade_partials(B, nparts):
    """[B, nparts, 3] fp64 {count, mean, M2} with unequal counts, and the exact merged (mean, sigma) [B, 2]"""
    n, i = np.arange(B)[:, None], np.arange(nparts)[None, :]
    cnt = 8 * (1 + (7 * i + n) % 5)
    k = (5 * i + 3 * n) % 17 - 8                       # mean = P_OFFSET + k / 8
    q = cnt * (1 + (i + n) % 3)                        # M2 = q / 4
    part = np.stack([cnt, P_OFFSET + k / 8.0, q / 4.0], 2).astype(F64)
    exact = []
    for b in range(B):
        N = int(cnt[b].sum())
        mean = Fraction(int((cnt[b] * k[b]).sum()), 8 * N)
        m2 = Fraction(int(q[b].sum()), 4) + sum(int(c) * (Fraction(int(kk), 8) - mean) ** 2 for c, kk in zip(cnt[b], k[b]))
        exact.append((float(mean + int(P_OFFSET)), math.sqrt(float(m2 / N))))
    return part, np.array(exact, F64)


# --------------------------------------------------------------------------------------------------------- launch geometry
def cdiv(a, b):
    return -(-a // b)


def fit_rounds(nb, resident, hard, unit=1):
    nb = min(nb, hard)
    if nb > resident:
        nb = nb // resident * resident
    return max(nb // unit * unit, unit)


def fit_candidates(raw, cus, hard, unit=1):
    """{grid: [per-CU residencies that give it]} of fit_rounds for residencies 1..16"""
    out = {}
    for per in range(1, 17):
        out.setdefault(fit_rounds(raw, per * cus, hard, unit), []).append(per)
    return out


EW_MAX, DB_MAX = 8192, 2046


def db_unit(C, per):
    return 1 if 256 % (C // per) == 0 else 3


def expected_launches(s):
    """[(kernel, ("fixed", gx) | ("fit", raw, hard, unit, elements per block trip, total units), gy)] of a spec, in launch order"""
    k, B, L = s["kind"], s["B"], s["L"]
    if k == "stats":
        return [("stats_partial_kernel", ("fixed", cdiv(L, 4096)), B), ("stats_final_kernel", ("fixed", B), 1)]
    if k == "finalize":
        return [("stats_final_kernel", ("fixed", B), 1)]
    if k == "coef":
        return [("bwd_coef_kernel", ("fixed", B), 1)]
    z16, drop = s["path"] != "f32", s.get("drop", False)
    per = 8 if z16 else 4
    tot = B * L // per
    if k == "apply":
        sk = {None: 0, "f32": 1, "bf16": 2}[s["skip"]]
        if s["path"] == "p":
            bps = cdiv(L // 8, 2048)
            if bps * B > EW_MAX:
                bps = EW_MAX // B
            return [("apply16p_drop_kernel" if drop else f"apply16p_kernel<{sk}>", ("fixed", max(bps, 1)), B)]
        name = ("apply16_drop_kernel" if drop else f"apply16_kernel<{sk}>") if z16 else ("apply_drop_kernel" if drop else "apply_kernel")
        unr = 512 if z16 else 1024
        return [(name, ("fit", max(cdiv(tot, unr), 1), EW_MAX, 1, unr, tot), 1)]
    assert k == "bwd"
    g16, C = "true" if s["g16"] else "false", s.get("C", 0)
    d = "_drop" if drop else ""
    out = []
    if not s.get("nparts"):
        nc = min(max(4096 // B, 1), cdiv(L, 8192 if z16 else 4096))
        out.append((f"bwd_partial16{d}_kernel<{g16}>" if z16 else f"bwd_partial{d}_kernel", ("fixed", nc), B))
    out += [("bwd_final_kernel", ("fixed", B), 1), ("bwd_affine_grad_kernel", ("fixed", 1), 1)]
    db = "true" if C else "false"
    name = f"bwd_apply16{d}_kernel<{db},{g16}>" if z16 else f"bwd_apply{d}_kernel<{db}>"
    if not C:
        unr = 512 if z16 else 1024
        out.append((name, ("fit", max(cdiv(tot, unr), 1), EW_MAX, 1, unr, tot), 1))
    else:
        unr = 512 if z16 else 256
        out += [(name, ("fit", cdiv(tot, unr), DB_MAX, db_unit(C, per), unr, tot), 1), ("colsum_final_kernel", ("fixed", cdiv(C, 16)), 1)]
    return out


def kernel_names(s):
    return [n for n, _, _ in expected_launches(s)]


# --------------------------------------------------------------------------------------------------------------- the table
def spec(kind, **kw):
    return dict(kind=kind, **kw)


F32_EDGE = [(1, 4), (1, 8), (5, 320), (3, 1364), (4, 1024), (5, 820), (3, 4 * 4 * 32), (2, 6 * 10 * 128), (2, 8 * 8 * 384)]   # total4 = 1023, 1024, 1025
Z16_EDGE = [(1, 8), (5, 320), (7, 584), (4, 1024), (3, 1368), (3, 4 * 4 * 32), (2, 6 * 10 * 128), (2, 8 * 8 * 384)]            # total8 = 511, 512, 513
BIG32, BIG16 = (5, 4098052), (5, 4098056)     # raw grid 5003 blocks: two trips, the second ragged, at every residency 1..8

# (pre_leaky, post_leaky, skip, outputs)
F32_APPLY_FORMS = [(0, 1, None, "both"), (0, 1, "f32", "y"), (1, 0, "f32", "y16"), (0, 0, None, "both")]
Z16_APPLY_FORMS = [(0, 1, None, "both"), (0, 1, "f32", "y16"), (0, 1, "bf16", "y"), (1, 0, "f32", "both"), (1, 0, "bf16", "y16"),
                   (1, 1, None, "y"), (0, 0, None, "y")]
# (pre_leaky, post_leaky, g is bf16, outputs, accumulate)
F32_BWD_FORMS = [(0, 1, False, "both", 0), (1, 0, True, "dx16", 1), (0, 0, False, "dx", 0), (0, 1, True, "both", 1)]
Z16_BWD_FORMS = [(0, 1, True, "dx16", 0), (0, 1, False, "both", 1), (1, 0, True, "both", 0), (0, 0, False, "dx", 1)]


def apply_groups():
    out = []
    for path, shapes, forms in (("f32", F32_EDGE, F32_APPLY_FORMS), ("z16", Z16_EDGE, Z16_APPLY_FORMS)):
        for B, L in shapes:
            out.append((f"apply-{path}-{B}x{L}", [spec("apply", path=path, B=B, L=L, pre=p, post=q, skip=sk, outs=o) for p, q, sk, o in forms]))
    out.append(("apply-f32-big", [spec("apply", path="f32", B=BIG32[0], L=BIG32[1], pre=0, post=1, skip=None, outs="both", trips=2)]))
    for sk in (None, "f32", "bf16"):
        out.append((f"apply-z16-big-skip-{sk}", [spec("apply", path="z16", B=BIG16[0], L=BIG16[1], pre=0, post=1, skip=sk,
                                                     outs="y16" if sk else "both", trips=2)]))
    out.append(("apply-f32-big-drop", [spec("apply", path="f32", B=BIG32[0], L=BIG16[1], pre=0, post=1, skip=None, outs="both", drop=True, trips=2)]))
    out.append(("apply-z16-big-drop", [spec("apply", path="z16", B=BIG16[0], L=BIG16[1], pre=0, post=1, skip=None, outs="y16", drop=True, trips=2)]))
    return out


# apply16p: (B, L, nparts, skip, post_leaky, drop); L8 = 1, 2048, 2049 (3 trips, the last ragged), 6*2048 + 5; bps clamped at B = 8193
P_CASES = [(3, 8, 1, None, 1, False), (3, 8 * 2048, 63, "f32", 1, False), (3, 8 * 2049, 64, "bf16", 0, False), (3, 8 * (6 * 2048 + 5), 65, None, 1, False),
           (4, 8 * 2049, 130, "f32", 1, False), (8193, 8, 1, "bf16", 1, False), (3, 8 * 2049, 65, None, 1, True)]


def p_groups():
    return [(f"apply-p-{B}x{L}-n{n}-skip-{sk}" + ("-drop" if d else ""),
             [spec("apply", path="p", B=B, L=L, pre=0, post=q, skip=sk, outs="both", nparts=n, drop=d)]) for B, L, n, sk, q, d in P_CASES]


def bwd_groups():
    out = []
    for path, shapes, forms in (("f32", F32_EDGE, F32_BWD_FORMS), ("z16", Z16_EDGE, Z16_BWD_FORMS)):
        for B, L in shapes:
            out.append((f"bwd-{path}-{B}x{L}", [spec("bwd", path=path, B=B, L=L, pre=p, post=q, g16=g, outs=o, acc=a) for p, q, g, o, a in forms]))
    # reductions: 65 partial records (second lane round of bwd_final), nc = 5 blocks sweeping 7 chunks with a ragged last one, more than 256 samples
    for B, L in [(2, 4092), (2, 4096), (2, 4100), (2, 64 * 4096 + 4), (257, 8), (4097, 8), (700, 24580)]:
        out.append((f"bwd-f32-red-{B}x{L}", [spec("bwd", path="f32", B=B, L=L, pre=0, post=1, g16=False, outs="dx", acc=0)]))
    for B, L in [(2, 4088), (2, 8192), (2, 8200), (2, 64 * 8192 + 8), (257, 8), (4097, 8), (700, 49160)]:
        out.append((f"bwd-z16-red-{B}x{L}", [spec("bwd", path="z16", B=B, L=L, pre=0, post=1, g16=True, outs="dx16", acc=0)]))
    out.append(("bwd-f32-big", [spec("bwd", path="f32", B=BIG32[0], L=BIG32[1], pre=0, post=1, g16=False, outs="both", acc=0, trips=2)]))
    out.append(("bwd-f32-big-drop", [spec("bwd", path="f32", B=BIG32[0], L=BIG16[1], pre=0, post=1, g16=True, outs="dx", acc=0, drop=True, trips=2)]))
    for g16 in (True, False):
        out.append((f"bwd-z16-big-g16-{g16}", [spec("bwd", path="z16", B=BIG16[0], L=BIG16[1], pre=0, post=1, g16=g16, outs="dx16", acc=0, trips=2)]))
        out.append((f"bwd-z16-big-drop-g16-{g16}", [spec("bwd", path="z16", B=BIG16[0], L=BIG16[1], pre=0, post=1, g16=g16, outs="dx16", acc=0,
                                                         drop=True, trips=2)]))
    return out


# bias-sum forms: per channel count a one-block shape (B = 2, two positions) and one of several blocks; nb = 1, 3, 65 for colsum_final
DB_SHAPES = [(2, 2, 32), (3, 22, 32), (5, 410, 32), (2, 2, 64), (3, 22, 64), (2, 2, 128), (3, 22, 128), (2, 2, 384), (3, 22, 384),
             (2, 2, 24), (3, 22, 24), (2, 2, 1024), (3, 22, 1024)]
DB_BIG32, DB_BIG16 = (3, 48 * 48, 384), (12, 48 * 48, 384)   # raw grid 2592 > DB_MAX_BLOCKS: two trips, colsum_final past its unrolled loop


def db_groups():
    out = []
    for B, P, C in DB_SHAPES:
        for path in ("f32", "z16"):
            sp = [spec("bwd", path=path, B=B, L=P * C, C=C, pre=0, post=1, g16=g, outs=o, acc=a, form=f)
                  for g, o, a, f in [(False, "both", 0, "general"), (True, "dx16", 1, "general"), (False, "both", 0, "balanced"), (True, "both", 1, "balanced")]]
            out.append((f"db-{path}-{B}x{P}x{C}", sp))
    B, P, C = DB_BIG32
    out.append(("db-f32-big", [spec("bwd", path="f32", B=B, L=P * C, C=C, pre=0, post=1, g16=False, outs="dx", acc=0, form="balanced", trips=2)]))
    out.append(("db-f32-big-drop", [spec("bwd", path="f32", B=B, L=P * C, C=C, pre=0, post=1, g16=True, outs="dx", acc=1, form="general",
                                         drop=True, trips=2)]))
    B, P, C = DB_BIG16
    for g16 in (True, False):
        out.append((f"db-z16-big-g16-{g16}", [spec("bwd", path="z16", B=B, L=P * C, C=C, pre=0, post=1, g16=g16, outs="dx16", acc=int(g16),
                                                   form="balanced", trips=2)]))
        out.append((f"db-z16-big-drop-g16-{g16}", [spec("bwd", path="z16", B=B, L=P * C, C=C, pre=0, post=1, g16=g16, outs="dx16", acc=0,
                                                        form="general", drop=True, trips=2)]))
    return out


# producer-style partial sums [B][nparts][2] into the backward (first pass skipped) and into lg_instnorm_bwd_coef
FUSED = [(3, 512, 1), (3, 512, 63), (2, 7680, 64), (3, 512, 65), (2, 7680, 130)]


def fused_groups():
    return [(f"bwd-z16-fused-{B}x{L}-n{n}", [spec("bwd", path="z16", B=B, L=L, pre=0, post=1, g16=True, outs="both", acc=0, nparts=n),
                                              spec("coef", B=B, L=L, nparts=n)]) for B, L, n in FUSED]


# moments: (B, L, pre_leaky, denominator of the unit, range of the integers, x16_out, offset in units)
STATS = [(2, 4092, 0, 1, 8, False, 0), (2, 4096, 1, 1, 8, False, 0), (2, 4100, 0, 64, 1024, True, 0), (2, 64 * 4096 + 4, 1, 1, 8, False, 0),
         (257, 8, 0, 64, 1024, True, 0), (4097, 8, 1, 1, 8, False, 0), (3, 512, 1, 64, 1024, True, 0), (3, 4100, 0, 8, 64, False, 4096 * 8)]


def stats_groups():
    return [(f"stats-{B}x{L}-pre{p}-u{den}" + ("-cancel" if off else ""), [spec("stats", B=B, L=L, pre=p, den=den, rng=r, x16=x16, off=off)])
            for B, L, p, den, r, x16, off in STATS]


def all_groups():
    return apply_groups() + p_groups() + bwd_groups() + db_groups() + fused_groups() + stats_groups()


# kernels of norm.hip that no case of this file launches, with the reason
NOT_REACHED = {}
AUX_NAMES = ["dropout_key_kernel", "dropout_mask_kernel"]   # asserted by every dropped case (Ctx.key_and_mask), outside expected_launches


def stats_input(s):
    """integers k [B, L] (x = k / den) of a moments case"""
    rng = np.random.default_rng(zlib.crc32(f"norm-stats-{s['B']}x{s['L']}/{s['den']}".encode()))
    return rng.integers(-s["rng"], s["rng"] + 1, (s["B"], s["L"])).astype(np.int64) + s["off"]


def balanced_gdiv(s):
    """g of the balanced form: a unit of 2^-7 with an fp32 g (bf16 ties in dx16) where every column's absolute sum stays below 2^24 units
    (unit 2^-7 * 2^-2 (leaky) * 2^-1 (a)), integers otherwise (bf16 g must be exact in bf16; the large maps would leave 2^24)"""
    rows = s["B"] * s["L"] // s["C"]
    return 128 if (not s["g16"] and rows * 8 * 1024 < 2 ** 24) else 1


# ------------------------------------------------------------------------------------------------------------- GPU harness
def _torch():
    import torch
    return torch


def dev32(a):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=F32)).cuda()


def dev16(a):
    t = _torch()
    return t.from_numpy(np.ascontiguousarray(a, dtype=F32)).cuda().to(t.bfloat16)   # exact: every bf16 operand of this file is representable


def bits_equal(got, want32, what):
    """got: a float32 or bf16 device tensor; want32: float32 numpy (rounded to bf16, nearest even, for a bf16 tensor)"""
    t = _torch()
    if got.dtype == t.bfloat16:
        g = got.contiguous().view(t.int16).cpu().numpy().view(np.uint16).ravel()
        w = bf16_bits(want32).ravel()
    else:
        g = got.contiguous().cpu().numpy().view(np.uint32).ravel()
        w = np.ascontiguousarray(want32, F32).view(np.uint32).ravel()
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        raise AssertionError(f"{what}: {bad.size} of {g.size} elements differ in bits, first at {bad[0]}: got {g[bad[0]]:#x}, want {w[bad[0]]:#x}")


class Ctx:
    def __init__(self):
        from littlegan_amd import _lib, ops
        self.ops, self.lib = ops, _lib.load()
        self.cus = self.lib.lg_device_cus()
        self.t = _torch()

    def check_launches(self, s, want=None):
        got = self.ops.last_norm_launches()
        want = expected_launches(s) if want is None else want
        assert [g[0] for g in got] == [w[0] for w in want], (got, want)
        for (name, gx, gy), (_, how, wy) in zip(got, want):
            assert gy == wy, (name, gx, gy, how, wy)
            if how[0] == "fixed":
                assert gx == how[1], (name, gx, how)
                continue
            _, raw, hard, unit, per_block, total = how
            cands = fit_candidates(raw, self.cus, hard, unit)
            assert gx in cands, f"{name}: grid {gx} is fit_rounds({raw}, per-CU residency x {self.cus} CUs, {hard}, {unit}) for no residency 1..16: {sorted(cands)}"
            trips = cdiv(total, gx * per_block)
            print(f"{name}: grid {gx} of raw {raw} (per-CU residency {cands[gx] if gx < min(raw, hard) else 'not binding'}), {trips} trips, "
                  f"last trip {'ragged' if total % (gx * per_block) else 'full'}")
            if s.get("C"):   # bias-sum forms: a thread must meet the same channels in every trip
                assert (gx * 256) % (s["C"] // (8 if s["path"] != "f32" else 4)) == 0, (name, gx, s["C"])
            if s.get("trips"):   # the multi-trip cases: the grid was cut (whole rounds of the CUs; the bias-sum forms also by their cap and unit)
                assert gx < raw and (s.get("C") or gx % self.cus == 0), f"{name}: grid {gx} of raw {raw} was not cut to whole rounds of {self.cus} CUs"
                assert (trips >= 2 if s.get("C") else trips == s["trips"]) and total % (gx * per_block) != 0, \
                    f"{name}: {trips} trips, want {s['trips']} with a ragged last one"

    def key_and_mask(self, B, L, level=2, call=1, r0=3):
        ops = self.ops
        key = ops.dropout_key(0x1234567 + B, (5 << 40) + L)
        assert ops.last_norm_launches() == [("dropout_key_kernel", 1, 1)]
        keep = ops.dropout_mask(key, call, level, r0, B, L, 0.5)
        assert ops.last_norm_launches() == [("dropout_mask_kernel", min(cdiv(B * L // 8, 256), EW_MAX), 1)]
        k = keep.cpu().numpy()
        assert 0.45 < k.mean() < 0.55 or k.size < 4096
        return ops.Drop(key, call, level, r0, 0.5), k.astype(F32) * F32(2)


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


def run_apply(cx, s):
    ops, t = cx.ops, cx.t
    B, L = s["B"], s["L"]
    z, _, sk = operands(B, L)
    skip = None if s["skip"] is None else sk
    z_d = dev32(z) if s["path"] == "f32" else dev16(z)
    skip_d = None if skip is None else (dev32(skip) if s["skip"] == "f32" else dev16(skip))
    drop, mult = cx.key_and_mask(B, L) if s.get("drop") else (None, None)
    y16 = t.empty((B, L), dtype=t.bfloat16, device="cuda") if s["outs"] != "y" else None
    want_f32 = s["outs"] != "y16"
    if s["path"] == "p":
        zp = F32(P_OFFSET) + F32(P_STEP) * z.astype(F32)
        return run_apply_p(cx, s, zp, dev16(zp), skip, skip_d, drop, mult, y16)
    rec = records(B)
    y = ops.instnorm_apply(z_d, dev32(rec), skip_d, s["pre"], s["post"], ALPHA, out16=y16, want_f32=want_f32, drop=drop)
    cx.check_launches(s)
    want = apply32(z, rec, s["pre"], s["post"], skip, mult)
    if B * L <= 1 << 16:   # the restatement IS the exact value (all shapes: tests/test_norm_exact_cpu.py)
        assert np.array_equal(want.astype(F64), apply64(z, rec, s["pre"], s["post"], skip, mult))
    if want_f32:
        bits_equal(y, want, f"y {s}")
    else:
        assert y is None
    if y16 is not None:
        bits_equal(y16, want, f"y16 {s}")


def check_record(st, exact, gamma, beta, what):
    """a statistics record [B, 8] against the exact (mean, sigma) [B, 2]"""
    st = st.astype(F64)
    mean, sigma = exact[:, 0], exact[:, 1]
    err = np.abs(st[:, 0] + st[:, 4] - mean) / np.maximum(np.abs(mean), sigma)
    print(f"{what}: |mu_hi + mu_lo - mean| <= {err.max():.3e} = 2^{np.log2(max(err.max(), 1e-300)):.1f} of max(|mean|, sigma)")
    assert err.max() <= 2.0 ** -44, (what, err.max())
    assert np.array_equal(st[:, 0].astype(F32), (st[:, 0] + st[:, 4]).astype(F32)), f"{what}: mu_hi is not float32(mu_hi + mu_lo)"
    for col, ex in ((1, sigma), (2, gamma / (sigma + EPS))):
        w = ex.astype(F32)
        assert (np.abs(st[:, col] - w.astype(F64)) <= np.spacing(w).astype(F64)).all(), (what, col, st[:, col], w)
    assert np.array_equal(st[:, 3], np.full(len(st), beta)) and not st[:, 5:].any(), what


def run_apply_p(cx, s, z, z_d, skip, skip_d, drop, mult, y16):
    """hand-made moment partials, finished inside the apply launch over two row ranges and by the stand-alone finaliser"""
    ops, t = cx.ops, cx.t
    B, L, n = s["B"], s["L"], s["nparts"]
    part, exact = handmade_partials(B, n)
    ws = t.from_numpy(part).cuda()
    gm, bt = dev32([GAMMA]), dev32([BETA])
    m = ops.Moments(ws, n, gm, bt, B)
    y = t.empty((B, L), dtype=t.float32, device="cuda")
    h = B // 2 + 1
    for lo, hi in ((0, h), (h, B)):
        d = None if drop is None else drop.at(r0=drop.r0 + lo)
        ops.instnorm_apply(z_d[lo:hi], m[lo:hi], None if skip_d is None else skip_d[lo:hi], 0, s["post"], ALPHA, out=y[lo:hi], out16=y16[lo:hi], drop=d)
        cx.check_launches(dict(s, B=hi - lo))
    assert m.covered == B
    rec = m.stats.cpu().numpy()
    assert n == 1 or (np.abs(rec[:, 4]) > 2.0 ** -20).any(), "mu_lo of these records is too small to move z - mu_hi"   # (one partial: the mean is k/8)
    check_record(rec, exact, GAMMA, BETA, f"apply16p {B}x{L} nparts={n}")
    st2 = ops.stats_tensor(ops.Moments(ws, n, gm, bt, B))
    cx.check_launches(spec("finalize", B=B, L=L))
    bits_equal(st2, rec, "stats_finalize against the record apply16p wrote")
    want = apply32(z, rec, 0, s["post"], skip, mult)
    bits_equal(y, want, f"y {s}")
    bits_equal(y16, want, f"y16 {s}")


def one_ulp(got, want64, what):
    w = F32(want64)
    assert abs(float(got) - float(w)) <= abs(float(np.spacing(w))), (what, float(got), float(w))


def run_bwd(cx, s):
    ops, t = cx.ops, cx.t
    B, L, C = s["B"], s["L"], s.get("C", 0)
    if s.get("form") == "balanced":
        z, g = balanced_operands(B, L // C, C, balanced_gdiv(s))
    else:
        z, g, _ = operands(B, L)
    rec = records(B)
    shape = (B, L // C, C) if C else (B, L)
    z_d = (dev32(z) if s["path"] == "f32" else dev16(z)).reshape(shape)
    g_d = (dev16(g) if s["g16"] else dev32(g)).reshape(shape)
    drop, mult = cx.key_and_mask(B, L) if s.get("drop") else (None, None)
    prior_g, prior_b = (3.5, -1.25) if s["acc"] else (float("nan"), float("nan"))
    dgm, dbt = dev32([prior_g]), dev32([prior_b])
    db = None
    if C:
        prior_db = (np.arange(C) % 7 - 3).astype(F32) if s["acc"] else np.full(C, np.nan, F32)   # accumulate covers dgamma, dbeta and db
        db = dev32(prior_db)
    dx16 = t.empty(shape, dtype=t.bfloat16, device="cuda") if s["outs"] != "dx" else None
    sums = partials = None
    if s.get("nparts"):   # the sums arrive from the producer of g: the exact ones, split into integer pieces
        n = s["nparts"]
        s1, s2 = bwd_sums(z, g, rec, s["pre"], s["post"])
        piece = np.zeros((B, n, 2), F64)
        piece[:, :, 0], piece[:, :, 1] = (np.arange(n) % 5 - 2)[None, :], (np.arange(n) % 3 - 1)[None, :] / 8.0
        piece[:, n - 1, 0] += s1 - piece[:, :, 0].sum(1)
        piece[:, n - 1, 1] += s2 - piece[:, :, 1].sum(1)
        assert np.array_equal(piece[:, :, 0].sum(1), s1) and np.array_equal(piece[:, :, 1].sum(1), s2)
        sums = (s1, s2)
        partials = ops.NormPartials(t.from_numpy(piece).cuda(), n, ALPHA, shape)
        s["_partials"], s["_rec"], s["_sums"] = partials, rec, sums
    dx = ops.instnorm_bwd(z_d, dev32(rec), g_d, dgm, dbt, s["pre"], s["post"], ALPHA, accumulate=bool(s["acc"]), out16=dx16,
                          want_f32=s["outs"] != "dx16", db=db, partials=partials, drop=drop)
    cx.check_launches(s)
    want, m, dg, dbeta, _ = bwd32(z, g, rec, s["pre"], s["post"], mult, sums)
    if s["outs"] != "dx16":
        bits_equal(dx, want, f"dx {s}")
    if dx16 is not None:
        bits_equal(dx16, want, f"dx16 {s}")
    # dbeta: the exact sum, rounded once; dgamma: within one fp32 ulp (the fp64 tree sum can differ from fsum by B 2^-53 relative)
    got_g, got_b = float(dgm.cpu()), float(dbt.cpu())
    if s["acc"]:
        assert got_b == float(F32(prior_b) + F32(dbeta)), (got_b, dbeta)
        cand = {float(F32(prior_g) + v) for v in (F32(dg), np.nextafter(F32(dg), F32(np.inf)), np.nextafter(F32(dg), F32(-np.inf)))}
        assert got_g in cand, (got_g, dg, cand)
    else:
        assert got_b == float(F32(dbeta)), (got_b, dbeta)
        one_ulp(got_g, dg, f"dgamma {s}")
    if C:
        cs, mass = colsums(want, C)
        got_db = db.cpu().numpy().astype(F64)
        prior = prior_db.astype(F64) if s["acc"] else 0.0
        if s["form"] == "balanced":
            assert not m.any(), "balanced form: s1 = s2 = 0"
            assert np.array_equal(got_db, prior + cs) and (cs != 0).all(), (s, np.abs(got_db - prior - cs).max())
        else:
            err = np.abs(got_db - prior - cs).max()
            print(f"db {s['path']} {B}x{L} C={C}: max error {err / mass:.3e} of the largest column's absolute mass")
            assert err <= 3e-6 * mass, (s, err, mass)


def run_coef(cx, s, prev):
    """lg_instnorm_bwd_coef on the partial sums the preceding backward spec was fed"""
    ops = cx.ops
    B, L = s["B"], s["L"]
    rec = prev["_rec"]
    z16 = cx.t.empty(prev["_partials"].shape, dtype=cx.t.bfloat16, device="cuda")   # shape only
    coef = ops.instnorm_bwd_coef(z16, dev32(rec), prev["_partials"])
    cx.check_launches(s)
    m, _ = bwd_coef(*prev["_sums"], rec, L)
    want = np.concatenate([rec[:, [0, 4, 2, 3]], m], 1)
    bits_equal(coef, want, f"coef {s}")


def run_stats(cx, s):
    ops, t = cx.ops, cx.t
    B, L = s["B"], s["L"]
    k = stats_input(s)
    x = (k / F64(s["den"])).astype(F32)
    assert np.array_equal(x.astype(F64) * s["den"], k)
    x16 = t.empty((B, L), dtype=t.bfloat16, device="cuda") if s["x16"] else None
    st = ops.instnorm_stats(dev32(x), dev32([GAMMA]), dev32([BETA]), s["pre"], ALPHA, x16_out=x16)
    cx.check_launches(s)
    check_record(st.cpu().numpy(), exact_moments(k, s["den"], s["pre"]), GAMMA, BETA, f"stats {s}")
    if x16 is not None:
        bits_equal(x16, x, f"x16_out {s}")


RUN = {"apply": run_apply, "bwd": run_bwd, "stats": run_stats}
GROUPS = all_groups()


@pytest.mark.gpu
@pytest.mark.parametrize("gid,specs", GROUPS, ids=[g[0] for g in GROUPS])
def test_norm_exact(ctx, gid, specs):
    prev = None
    for s in specs:
        s = dict(s)
        if s["kind"] == "coef":
            run_coef(ctx, s, prev)
        else:
            RUN[s["kind"]](ctx, s)
        prev = s


REFUSED = [("f32", 20, "unsupported channel count"), ("f32", 1028, "unsupported channel count"), ("z16", 40, "unsupported channel count"),
           ("f32", 32, "L % C"), ("z16", 32, "L % C")]


@pytest.mark.gpu
@pytest.mark.parametrize("path,C,why", REFUSED, ids=[f"{p}-C{c}-{'ragged' if 'L' in w else 'count'}" for p, c, w in REFUSED])
def test_bias_sum_forms_refuse_what_they_cannot_map(ctx, path, C, why):
    """channel counts whose thread-to-channel map has no period of 1 or 3 blocks, and maps that are no whole number of pixels: an error
    and no launch (db keeps its contents)"""
    from littlegan_amd import _lib
    t, ops = ctx.t, ctx.ops
    B, P = 2, 4
    L = P * C + (8 if "L" in why else 0)
    shape = (B, P, C) if "L" not in why else (B, L // 8, 8)
    z = t.zeros(shape, dtype=t.float32 if path == "f32" else t.bfloat16, device="cuda")
    g = t.zeros(shape, dtype=t.float32, device="cuda")
    db = t.full((C,), 7.0, device="cuda")
    ops.dropout_key(1, 2)
    assert ops.last_norm_launches()
    lib = ctx.lib
    ws = t.empty(1 << 22, dtype=t.uint8, device="cuda")
    p = lambda x: x.data_ptr()
    dx = t.empty(shape, dtype=t.float32, device="cuda")
    dgm, dbt, st = t.zeros(1, device="cuda"), t.zeros(1, device="cuda"), dev32(records(B))
    fn = lib.lg_instnorm_leaky_bwd_db if path == "f32" else lib.lg_instnorm_leaky_bwd_z16
    rc = fn(p(z), p(st), p(g), 0, p(dx), None, p(dgm), p(dbt), p(db), C, p(ws), ws.numel(), B, L, 0, 1, ALPHA, 0, None)
    assert rc == -1 and b"unsupported channel count" in lib.lg_last_error(), (rc, lib.lg_last_error())
    assert ops.last_norm_launches() == []
    t.cuda.synchronize()
    assert (db == 7.0).all()
    with pytest.raises(_lib.LittleGanHipError):
        _lib.check(rc, "x")


@pytest.mark.gpu
def test_constant_sample_backward_matches_the_oracle(ctx):
    """sigma == 0: bwd_final_kernel forms m2' = 0 / 0.  What the backward returns is recorded next to the fp64 oracle's result for the same
    input: the finite values agree at 2e-5 and the non-finite positions are the same (both give NaN in every element of the
    constant sample, as instance.py's formula does; dgamma and dbeta stay finite)."""
    from oracle import np_oracle as O
    ops, t = ctx.ops, ctx.t
    B, L = 3, 512
    z, g, _ = operands(B, L)
    x = z.astype(F32)
    x[1] = 3.0
    st = ops.instnorm_stats(dev32(x), dev32([GAMMA]), dev32([BETA]), 0, ALPHA)
    rec = st.cpu().numpy()
    assert rec[1, 1] == 0.0 and rec[1, 0] == 3.0 and rec[1, 4] == 0.0
    dgm, dbt = dev32([0]), dev32([0])
    dx = ops.instnorm_bwd(dev32(x), st, dev32(g), dgm, dbt, 0, 0, ALPHA).cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        _, cache = O.instnorm(x.astype(F64), GAMMA, BETA, eps=EPS)
        ref, rg, rb = O.instnorm_bwd(cache, GAMMA, g.astype(F64))
    fin = np.isfinite(ref)
    print(f"constant sample: kernel non-finite {int((~np.isfinite(dx)).sum())} (all NaN: {bool(np.isnan(dx[1]).all())}), oracle non-finite {int((~fin).sum())}; "
          f"dgamma {float(dgm.cpu())} / {rg}, dbeta {float(dbt.cpu())} / {rb}")
    assert np.array_equal(np.isfinite(dx), fin) and np.array_equal(np.isnan(dx), np.isnan(ref))
    assert not fin[1].any() and fin[0].all() and fin[2].all()
    assert np.abs(dx[fin] - ref[fin]).max() <= 2e-5 * np.abs(ref[fin]).max()
    assert abs(float(dgm.cpu()) - rg) <= 2e-5 * max(1.0, abs(rg)) and abs(float(dbt.cpu()) - rb) <= 2e-5 * max(1.0, abs(rb))
