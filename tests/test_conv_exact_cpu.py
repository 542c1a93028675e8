"""The conditions of the exact integer form of tests/test_conv_exact_gpu.py, checked on the oracle alone.

These are conditions on the INPUTS of the GPU cases, not measurements of a kernel: the seeds, ranges and units of that file are
chosen so that the fp64 oracle meets every one of them.  For every case:

  * the oracle on the absolute operands stays below 2^24 units, so every partial sum in any order is exact in fp32;
  * the oracle result is an integer multiple of its unit;
  * a result that a kernel stores as bf16 has at least 1 % exact ties, and ties that round to even downwards AND upwards;
  * a tanh case has |pre-activation| <= 2, so saturation cannot hide an error.

The ledger reads the kernel names passed to lg_note_kernel in the conv sources: each one must be the asserted route of an exact case
or stand in NOT_EXACT with its reason, so a new conv kernel fails here until it has a case."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import np_oracle as O  # noqa: E402
from test_conv_exact_gpu import NOT_EXACT, BWDNORM_ROUTE, all_cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = all_cases()
LEDGER_FILES = ["conv_igemm.hip", "conv_halo.hip", "conv_down3.hip", "conv_up3.hip", "conv_up4.hip", "wgrad_igemm.hip", "wgrad_at.hip",
                "wgrad_at32.hip", "n3_kernels.hip", "n3_pgemm.hip", "n3_rows.hip"]

# bf16 results whose contraction is too shallow for integer sums to reach the range where bf16 rounds (|sum| >= 256 units), with the
# reason; the bit equality with bf16_round(exact) is asserted for them all the same
SHALLOW = {
    "dx16": "data gradient of the final layer: 75 products of at most 16 units per output and no bias, standard deviation 58 units, so "
            "|sum| >= 256 is a 4.4 sigma event; the same kernel template's bf16 store (patch_p16_kernel) meets ties in conv1's z16, "
            "whose bias unit of 64 moves the sums into [256, 512)",
}


def tie_counts(exact):
    """(ties rounding down to even, ties rounding up to even, elements) of the bf16 rounding of an exact fp64 array"""
    v = np.abs(np.asarray(exact, np.float64)).ravel()
    q = O.bf16_round(v)
    f32 = v.astype(np.float32).view(np.uint32)
    assert np.array_equal(f32.view(np.float32).astype(np.float64), v), "not exact in fp32"
    tie = (f32 & np.uint32(0xFFFF)) == np.uint32(0x8000)   # exactly half-way between two bf16 values
    return int((tie & (q < v)).sum()), int((tie & (q > v)).sum()), v.size


@pytest.mark.parametrize("cid,routes,make", CASES, ids=[c[0] for c in CASES])
def test_conditions_of_the_exact_form(cid, routes, make):
    e = make()
    assert e.want, "a case without results"
    for name, want in e.want.items():
        unit = e.unit[name]
        assert e.bound[name] < 2.0 ** 24 * unit, f"{name}: a partial sum can reach {e.bound[name] / unit:.0f} units, not below 2^24"
        k = want / unit
        assert np.array_equal(k, np.rint(k)), f"{name}: not an integer multiple of {unit}"
        assert np.abs(want).max() <= e.bound[name]
    for name in e.bf16:
        down, up, n = tie_counts(e.want[name])
        print(f"{cid} {name}: {down} ties to even downwards, {up} upwards, of {n} ({100.0 * (down + up) / n:.1f} %), max |value| {np.abs(e.want[name]).max():.0f}")
        if name in SHALLOW:
            continue
        assert down + up >= 0.01 * n and down > 0 and up > 0, f"{name}: {down} + {up} ties of {n}"
    if e.pre is not None:
        assert np.abs(e.pre).max() <= 2.0, f"tanh pre-activation reaches {np.abs(e.pre).max():.3f}"


def test_operands_are_iid_integers_in_range():
    """every operand of every case: integers times a power-of-two unit, |integer| <= 4 (the activated maps of the NORM forms: multiples
    of 1/8 below 32), and not symmetric under a swap of taps or of channels"""
    for cid, _, make in CASES:
        for name, a in make().op.items():
            if name == "rec":
                assert set(np.unique(a[:, 2])) <= {0.5, 1.0, 2.0} and not a[:, 4:].any(), cid
                assert np.array_equal(a[:, [0, 3]], np.rint(a[:, [0, 3]])), cid
                continue
            if name == "h":
                assert np.array_equal(a * 8, np.rint(a * 8)) and np.abs(a).max() < 32, cid
                continue
            unit = max(u for u in 2.0 ** np.arange(-12, 9) if np.array_equal(a / u, np.rint(a / u)))   # the largest unit that fits
            k = a / unit
            assert np.array_equal(k, np.rint(k)) and np.abs(k).max() <= 4, (cid, name)
            if a.ndim == 4 and a.shape[0] == 5 and a.shape[2] > 1:   # a 5 x 5 kernel
                assert not np.array_equal(a, a.transpose(1, 0, 2, 3)) and not np.array_equal(a, a[::-1, ::-1])


def noted_names():
    """the string literals passed to lg_note_kernel in the conv sources"""
    names = {}
    for f in LEDGER_FILES:
        src = open(os.path.join(ROOT, "littlegan_amd", "csrc", f)).read()
        for call in re.finditer(r"lg_note_kernel\((.*?)\);", src, re.S):
            for lit in re.findall(r'"([^"]*)"', call.group(1)):
                names.setdefault(lit, f)
    return names


def test_every_noted_conv_kernel_has_an_exact_case():
    names = noted_names()
    assert len(names) >= 30 and "conv_down3_kernel<PAIR>" in names and "wgrad_at32_kernel<8,8>" in names, sorted(names)
    asserted = {r for _, routes, _ in CASES for r in routes}
    missing = sorted(n for n in names if n not in asserted and n not in NOT_EXACT)
    assert not missing, f"kernels without an exact case (tests/test_conv_exact_gpu.py) and without a NOT_EXACT reason: {missing}"
    stale = sorted(n for n in NOT_EXACT if n in asserted or n not in names)
    assert not stale, f"NOT_EXACT entries that are asserted by a case, or that no source notes any more: {stale}"
    unknown = sorted(r for r in asserted if r and r not in names)
    assert not unknown, f"routes asserted by a case that no source notes: {unknown}"
    assert all(len(reason) > 20 for reason in NOT_EXACT.values())
    assert BWDNORM_ROUTE[0] in NOT_EXACT and BWDNORM_ROUTE[1] in asserted   # the bit-equality test pins the one to the other
