"""The conditions of the exact forms of tests/test_norm_exact_gpu.py, checked on the oracle and the restatement alone.

These are conditions on the INPUTS and on the reference of the GPU cases, not measurements of a kernel; they are generated from the same
table.  For every case:

  * the float32 restatement of the apply form, one operation per line, equals the fp64 value (the large maps on a slice);
  * the products dz' c are exact in float32, a quad / octet of them sums below 2^24 units, a sample's sums stay below 2^53 units and
    every column sum of the balanced form below 2^24 units: the sums are exact in any order;
  * every bf16 result of the exact forms (y16 under the hand-made records, x16_out, dx16 of the balanced form with an fp32 g) has at
    least 1 % exact ties, rounding to even in BOTH directions.  Results of fewer than 200 elements are left out of this condition (1 % of
    them is less than the two elements that two directions need); their bit equality with the rounded exact value is asserted all the same;
  * the balanced form has s1 = s2 = 0 in every sample and no zero db column;
  * a raw grid of 5003 blocks is cut to two trips with a ragged second one at every per-CU residency 1..8;
  * the restatement of the backward agrees with the fp64 oracle (O.instnorm_bwd) at the 2e-5 tests/test_ops_gpu.py grants dx.

The ledger reads every kernel launched in norm.hip from the source, template arguments included: each must be launched (and asserted
through ops.last_norm_launches) by a case of the table or stand in NOT_REACHED with a reason."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import np_oracle as O  # noqa: E402
import test_norm_exact_gpu as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
GROUPS = T.all_groups()
SPECS = [(gid, s) for gid, specs in GROUPS for s in specs]
SLICE = 1 << 18     # columns of a large map the CPU conditions look at
TIE_MIN_ELEMENTS = 200


def _ops(s):
    """(z, g, skip) of a spec, the large maps cut to their first SLICE columns"""
    if s.get("form") == "balanced":
        z, g = T.balanced_operands(s["B"], s["L"] // s["C"], s["C"], T.balanced_gdiv(s))
        return z, g, None
    z, g, sk = T.operands(s["B"], s["L"])
    if s["B"] * s["L"] > 1 << 23:
        z, g, sk = z[:, :SLICE], g[:, :SLICE], sk[:, :SLICE]
    return z, g, sk


def _mult(s, shape):
    """a stand-in for the dropout multipliers (0 or 2 per element): the conditions hold for any mask"""
    if not s.get("drop"):
        return None
    return (np.random.default_rng(5).integers(0, 2, shape) * 2).astype(F32)


def tie_counts(v32):
    """(ties rounding down to even, ties rounding up to even, elements) of the bf16 rounding of a float32 array"""
    u = np.ascontiguousarray(v32, F32).view(np.uint32).ravel()
    tie = (u & np.uint32(0xFFFF)) == np.uint32(0x8000)
    up = tie & (((u >> np.uint32(16)) & np.uint32(1)) == 1)
    return int((tie & ~up).sum()), int(up.sum()), u.size


def assert_ties(v32, what):
    down, up, n = tie_counts(v32)
    print(f"{what}: {down} ties to even downwards, {up} upwards, of {n} ({100.0 * (down + up) / n:.1f} %)")
    if n >= TIE_MIN_ELEMENTS:
        assert down + up >= 0.01 * n and down > 0 and up > 0, f"{what}: {down} + {up} ties of {n}"


def test_bf16_rounding_helper_is_the_oracles():
    v = np.random.default_rng(1).standard_normal(4096).astype(F32)
    v[:8] = [0.0, -0.0, 1.00390625, 1.01171875, -1.00390625, 257.0, 259.0, 3.0]   # ties in both directions among them
    bits = T.bf16_bits(v)
    back = (bits.astype(np.uint32) << np.uint32(16)).view(F32).astype(F64)
    assert np.array_equal(back, O.bf16_round(v.astype(F64)))
    assert tie_counts(v[:8])[:2] == (3, 2)


APPLY = [(g, s) for g, s in SPECS if s["kind"] == "apply"]
# (apply16p runs under the record the kernel wrote, an arbitrary mean: restated in float32, no exact form; its conditions follow below)
APPLY_EXACT = [(g, s) for g, s in APPLY if s["path"] != "p"]


@pytest.mark.parametrize("gid,s", APPLY_EXACT, ids=[f"{g}-{i}" for i, (g, _) in enumerate(APPLY_EXACT)])
def test_apply_restatement_is_exact_and_meets_ties(gid, s):
    z, _, sk = _ops(s)
    rec = T.records(s["B"])
    skip = None if s["skip"] is None else sk
    mult = _mult(s, z.shape)
    y32 = T.apply32(z, rec, s["pre"], s["post"], skip, mult)
    assert np.array_equal(y32.astype(F64), T.apply64(z, rec, s["pre"], s["post"], skip, mult)), "the float32 restatement is not the fp64 value"
    if s["outs"] != "y" and mult is None:
        assert_ties(y32, f"{gid} y16 pre={s['pre']} post={s['post']} skip={s['skip']}")


def test_apply16p_cases_are_stated_in_float32_only():
    """every apply16p case carries hand-made partial records with unequal counts and a positive sigma"""
    for _, s in APPLY:
        if s["path"] == "p":
            part, exact = T.handmade_partials(min(s["B"], 5), s["nparts"])
            assert len({tuple(r) for r in part[0, :, 0:1]}) > 1 or s["nparts"] == 1, "counts are equal"
            assert np.isfinite(exact).all() and (exact[:, 1] > 0).all()


BWD = [(g, s) for g, s in SPECS if s["kind"] == "bwd"]


@pytest.mark.parametrize("gid,s", BWD, ids=[f"{g}-{i}" for i, (g, _) in enumerate(BWD)])
def test_backward_sums_are_exact_in_any_order(gid, s):
    z, g, _ = _ops(s)
    B, L = z.shape
    rec = T.records(B)
    mult = _mult(s, z.shape)
    c, dz, _ = T._c_dz(z, g, rec, s["pre"], s["post"], mult, 0, B)
    prod = dz * c
    assert prod.dtype == F32 and np.array_equal(prod.astype(F64), dz.astype(F64) * c.astype(F64)), "dz' c is not exact in float32"
    gdiv = T.balanced_gdiv(s) if s.get("form") == "balanced" else 1
    u_dz = 0.25 / gdiv                                  # LeakyReLU'(0.25) of integers / gdiv (the mask's scale of 2 is no finer)
    u_c = 2.0 ** -5 * (0.25 if s["pre"] else 1.0)
    for a, unit in ((dz, u_dz), (prod, u_dz * u_c)):
        k = a.astype(F64) / unit
        assert np.array_equal(k, np.rint(k)), "not a multiple of its unit"
        assert np.abs(k).max() * 8 < 2.0 ** 24, "an octet of them can leave the fp32 integers"
        full = s["B"] * s["L"] / (B * L)               # a slice stands for the whole map
        assert np.abs(k).sum(1).max() * full < 2.0 ** 53
    s1, s2 = T.bwd_sums(z, g, rec, s["pre"], s["post"], mult)
    assert np.array_equal(s1, dz.astype(F64).sum(1)) and np.array_equal(s2, (dz.astype(F64) * c.astype(F64)).sum(1))
    if s.get("form") == "balanced":
        C = s["C"]
        assert not s1.any() and not s2.any(), (s1, s2)
        dx, m, dg, dbeta, _ = T.bwd32(z, g, rec, s["pre"], s["post"])
        assert np.array_equal(dx, rec[:, 2:3] * dz) and dg == 0 and dbeta == 0
        cs, mass = T.colsums(dx, C)
        unit = 0.5 * u_dz
        assert mass / unit < 2.0 ** 24, f"a column's absolute sum reaches {mass / unit:.0f} units"
        assert (cs != 0).all(), f"{int((cs == 0).sum())} zero db columns of {C}"
        if s["outs"] != "dx" and not s["g16"] and gdiv > 1:
            assert_ties(dx, f"{gid} dx16 (balanced, g in units of 1/{gdiv})")


GENERAL = [(g, s) for g, s in BWD if s.get("form") != "balanced" and s["B"] * s["L"] <= 1 << 21 and not s.get("drop")]


@pytest.mark.parametrize("gid,s", GENERAL, ids=[f"{g}-{i}" for i, (g, _) in enumerate(GENERAL)])
def test_backward_restatement_against_the_oracle(gid, s):
    z, g, _ = _ops(s)
    rec = T.records(s["B"])
    dx, m, dg, dbeta, _ = T.bwd32(z, g, rec, s["pre"], s["post"])
    c, dz, x0 = T._c_dz(z, g, rec, s["pre"], s["post"], None, 0, s["B"])
    sg = rec[:, 1:2].astype(F64)
    sc = sg + 1e-3
    ref, rg, rb = O.instnorm_bwd((c.astype(F64), sg, sc), rec[:, 2:3].astype(F64) * sc, dz.astype(F64))
    if s["pre"]:
        ref = np.where(x0 > 0, ref, T.ALPHA * ref)
    err = np.abs(dx - ref).max() / np.abs(ref).max()
    print(f"{gid}: restatement against the oracle {err:.2e} of max |dx|; dgamma {dg:.6f} / {rg:.6f}, dbeta {dbeta} / {rb}")
    assert err <= 2e-5
    assert abs(dg - rg) <= 2e-5 * max(1.0, abs(rg)) and dbeta == rb


STATS = [(g, s) for g, s in SPECS if s["kind"] == "stats"]


@pytest.mark.parametrize("gid,s", STATS, ids=[g for g, _ in STATS])
def test_moment_cases(gid, s):
    k = T.stats_input(s)
    x = (k / F64(s["den"])).astype(F32)
    assert np.array_equal(x.astype(F64) * s["den"], k), "x is not exact in float32"
    ex = T.exact_moments(k, s["den"], s["pre"])
    xx = x.astype(F64)
    if s["pre"]:
        xx = np.where(xx > 0, xx, T.ALPHA * xx)
    assert np.allclose(ex[:, 0], xx.mean(1), rtol=1e-12, atol=1e-12) and np.allclose(ex[:, 1], xx.std(1), rtol=1e-9)
    if s["off"]:
        assert (np.abs(ex[:, 0]) > 500 * ex[:, 1]).all(), "no cancellation in the cancellation sample"
    if s["x16"]:
        assert_ties(x, f"{gid} x16_out")


def test_handmade_partials_merge_to_the_stated_moments():
    for n in (1, 63, 64, 65, 130):
        part, exact = T.handmade_partials(3, n)
        assert n == 1 or len(np.unique(part[:, :, 0])) > 1
        for b in range(3):
            # the records of a sample as explicit populations: count/2 values at mean +- sqrt(M2 / count)
            vals = np.concatenate([np.concatenate([np.full(int(c) // 2, m + np.sqrt(q / c)), np.full(int(c) // 2, m - np.sqrt(q / c))]) for c, m, q in part[b]])
            assert abs(vals.mean() - exact[b, 0]) < 1e-9 and abs(vals.std() - exact[b, 1]) < 1e-9   # (fp64 mean of < 4000 values near 4096)


def test_5003_blocks_are_two_trips_with_a_ragged_second_at_every_residency():
    for (B, L), per, unr in ((T.BIG32, 4, 1024), (T.BIG16, 8, 512)):
        total = B * L // per
        raw = T.cdiv(total, unr)
        assert raw == 5003
        for cus in (256, 304, 240):
            for res in range(1, 9):
                gx = T.fit_rounds(raw, res * cus, T.EW_MAX)
                if gx == raw:
                    continue   # the whole grid is resident at this CU count: one trip, and the GPU case says so (it asserts a cut)
                trips = T.cdiv(total, gx * unr)
                assert trips == 2 and total % (gx * unr) != 0, (cus, res, gx, trips)
        for res in range(1, 9):
            gx = T.fit_rounds(raw, res * 256, T.EW_MAX)
            assert 3584 <= gx <= 4864 and T.cdiv(total, gx * unr) == 2, (res, gx)


def launched_in_source():
    src = open(os.path.join(ROOT, "littlegan_amd", "csrc", "norm.hip")).read()
    src = re.sub(r"//[^\n]*", "", src)
    bare = re.findall(r"hipLaunchKernelGGL\(\s*([^,]+),", src)
    assert bare == ["kern"], f"launches outside NORM_LAUNCH (not recorded by lg_instnorm_last_launches): {bare}"
    names = set()
    for m in re.finditer(r"NORM_LAUNCH\(\s*(\((?:[^()]|\([^()]*\))*\)|[^,(]+)\s*,", src):
        n = re.sub(r"[()\s]", "", m.group(1))
        if n != "kern":
            names.add(n)
    return names


def test_every_launched_norm_kernel_has_an_exact_case():
    names = launched_in_source()
    assert len(names) >= 35 and "bwd_apply16_drop_kernel<true,false>" in names and "apply16p_kernel<1>" in names, sorted(names)
    asserted = {n for _, s in SPECS for n in T.kernel_names(s)} | set(T.AUX_NAMES)
    missing = sorted(n for n in names if n not in asserted and n not in T.NOT_REACHED)
    assert not missing, f"norm kernels that no case of tests/test_norm_exact_gpu.py launches, without a NOT_REACHED reason: {missing}"
    assert not sorted(n for n in T.NOT_REACHED if n in asserted or n not in names), "stale NOT_REACHED entries"
    unknown = sorted(n for n in asserted if n not in names)
    assert not unknown, f"kernels a case asserts that norm.hip does not launch: {unknown}"
    assert all(len(r) > 20 for r in T.NOT_REACHED.values())


def test_apply16p_cases_walk_the_trips_they_are_named_for():
    """apply16p's grid is fixed by (B, L) alone (the GPU cases assert it): L8 = 2048 is four full trips of one block, 2049 three trips of
    two blocks with a ragged last one, 6 * 2048 + 5 four trips of seven blocks with a ragged last one, and B = 8193 clamps bps to 1"""
    seen = {}
    for _, s in APPLY:
        if s["path"] != "p":
            continue
        (_, (_, bps), gy), = T.expected_launches(s)
        L8 = s["L"] // 8
        seen[(s["B"], L8)] = (bps, T.cdiv(L8, bps * 512), L8 % (bps * 512) != 0, gy)
    assert seen[(3, 1)] == (1, 1, True, 3) and seen[(3, 2048)] == (1, 4, False, 3) and seen[(3, 2049)] == (2, 3, True, 3)
    assert seen[(3, 6 * 2048 + 5)] == (7, 4, True, 3) and seen[(8193, 1)] == (1, 1, True, 8193) and seen[(4, 2049)] == (2, 3, True, 4)
