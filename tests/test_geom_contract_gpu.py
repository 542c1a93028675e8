"""The memory contract of the entry points of include/littlegan_geom.h (geom_augment), checked with guard bands
(tests/guards.py) the way tests/test_memory_contract_gpu.py checks the functions of include/littlegan_hip*.h: each row runs plain twice
and inside 0xFF, 0x00 and 0x3F red zones, and the test asserts that the plain runs agree bit for bit, that the guarded runs give the
plain bits, that every red zone and every input came back unchanged, that every output element was written, and the row's oracle
(the restatement of tests/test_geom_cpu.py at the bounds of tests/test_geom_gpu.py).  The entry points take no workspace.

The row `arbitrary-records` hands lgeo_fwd / lgeo_bwd records of arbitrary bits — NaN, infinities, huge and denormal entries, nearly
singular matrices.  The records are device data that the host cannot validate, so the kernels compare every coordinate as a float before
it becomes an index: the row checks that property (nothing read outside x, nothing written outside out).  It must not fault.

tests/test_geom_cpu.py checks that every pointer-taking function of the header is named by a row here."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_memory_contract_gpu import Alloc, Row, _diff, _stale  # noqa: E402
from test_geom_cpu import (FULL, extreme_records, geom_adjoint_np, geom_np, geom_records, key_of, usable)  # noqa: E402

pytestmark = pytest.mark.gpu

F32, I64 = torch.float32, torch.int64
CASES = []


class _Recorder:
    """the names with the header's prefix that a piece of code fetched from the library handle"""

    def __init__(self, handle, names):
        object.__setattr__(self, "_handle", handle)
        object.__setattr__(self, "_names", names)

    def __getattr__(self, name):
        if name.startswith("lgeo_"):
            self._names.append(name)
        return getattr(self._handle, name)


def _once(row_, ops, monkeypatch, mode, byte=0xFF):
    alloc, names = Alloc(mode, byte), []
    with monkeypatch.context() as mp:
        real = ops._lib.load
        mp.setattr(ops._lib, "load", lambda *a, **k: _Recorder(real(*a, **k), names))
        res = dict(row_.run(ops, alloc))
        torch.cuda.synchronize()
    return res, alloc, set(names)


@pytest.fixture(scope="module")
def ops():
    from littlegan_amd import ops as _ops
    return _ops


def f64(t):
    return t.detach().double().cpu().numpy()


def fwd_ok(out, x, recs):
    """lgeo_fwd against the restatement (the same fp32 weights): 8 2^-24 max|x| per row — one rounding per weight product, per term, per add"""
    err = np.abs(f64(out) - geom_np(x, recs)).reshape(len(recs), -1).max(1)
    bound = 8 * 2.0 ** -24 * np.abs(x).reshape(len(recs), -1).max(1)
    assert (err <= bound).all(), (err, bound)


def bwd_ok(gx, g, recs):
    """lgeo_bwd against the scatter restatement: (n + 3) 2^-24 sum |w g| per source pixel"""
    ref, cnt, mag = geom_adjoint_np(g, recs, stats=True)
    bound = (cnt[..., None] + 3) * 2.0 ** -24 * mag
    assert (np.abs(f64(gx) - ref) <= bound).all(), float((np.abs(f64(gx) - ref) - bound).max())


# ------------------------------------------------------------------------------------------------------------------ the rows
def _draw_row():
    rows, S, seed_arg, step = 300, 16, 3, 7        # two blocks of the one-thread-per-row launch, the second partly empty
    seed, koff = key_of(seed_arg, 1, step)

    def run(ops, alloc):
        key = alloc.inp("key", np.array([seed, koff], np.int64))
        state = alloc.inp("state", np.array([0.3, 0, 0, 0], np.float32))
        return {"plain": ops.geom_draw(key, 1, 5, rows, S, FULL, out=alloc.out("geo", (rows, 4))),
                "gated": ops.geom_draw(key, 0, 0, rows, S, FULL, state=state, out=alloc.out("geo_gated", (rows, 4)))}

    def check(res):
        for name, want in (("plain", geom_records(seed, koff, 1, 5, rows, S, FULL)),
                           ("gated", geom_records(seed, koff, 0, 0, rows, S, FULL, p=0.3))):
            got = res[name].cpu().numpy()
            assert (np.abs(got.astype(np.float64) - want) <= 2.0 ** -23 * np.maximum(1, np.abs(want))).all(), name
            exact = (np.abs(want) == 1) | (want == 0)        # what a selected identity leaves
            assert np.array_equal(got[exact], want[exact]), name
    CASES.append(Row("draw-300", ("lgeo_draw",), run, check))


def _map_row(id_, S, recs, seed):
    B = len(recs)
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (B, S, S, 3)).astype(np.float32)
    g = rng.uniform(-1, 1, (B, S, S, 3)).astype(np.float32)

    def run(ops, alloc):
        geo = alloc.inp("geo", recs)
        return {"out": ops.geom_fwd(alloc.inp("x", x), geo, out=alloc.out("out", x.shape)),
                "gx": ops.geom_bwd(alloc.inp("g", g), geo, out=alloc.out("gx", g.shape))}

    def check(res):
        assert torch.isfinite(res["out"]).all() and torch.isfinite(res["gx"]).all()
        fwd_ok(res["out"], x, recs)
        bwd_ok(res["gx"], g, recs)
        dead = [n for n, r in enumerate(recs) if not usable(r)]
        assert not res["out"][dead].any() and not res["gx"][dead].any()
    CASES.append(Row(id_, ("lgeo_fwd", "lgeo_bwd"), run, check))


def arbitrary_records():
    """Record bits a kernel has to survive: random 32-bit patterns (NaN, infinities, every exponent), entries with random mantissas near
    1, nearly singular matrices at both sides of the 2^-20 bound, huge entries with a finite determinant, denormals and negative zeros"""
    rng = np.random.default_rng(2026)
    recs = [rng.integers(0, 1 << 32, 4, dtype=np.uint64).astype(np.uint32).view(np.float32) for _ in range(8)]
    recs += [rng.uniform(-1.5, 1.5, 4).astype(np.float32) for _ in range(4)]
    recs += [np.array(r, np.float32) for r in (
        [1, 1, 1, 1 + 2.0 ** -19], [1, 1, 1, 1 + 2.0 ** -21], [2.0 ** -9, 0, 0, 2.0 ** -9], [1e30, 0, 0, 1e-30], [1e30, -1e30, 1, 0],
        [3e38, 3e38, -3e38, 3e38], [1e-40, 0, 0, 1e-40], [-0.0, 1, -1, -0.0], [np.nan] * 4, [np.inf, 0, 0, -np.inf], [0, 0, 0, 0],
        [1e19, 1, 1e-19, 1], [512, 0, 0, 2.0 ** -9])]
    return np.stack(recs).astype(np.float32)


_draw_row()
_map_row("extreme-records-16", 16, extreme_records(), 11)
_map_row("arbitrary-records-8", 8, arbitrary_records(), 12)
_map_row("workload-row-128", 128, extreme_records()[[0, 10]], 13)      # the workload's row length: many blocks, the row stride


@pytest.mark.parametrize("case", CASES, ids=lambda r: r.id)
def test_geom_memory_contract(case, ops, monkeypatch):
    plain, _, names = _once(case, ops, monkeypatch, "plain")
    missing = set(case.covers) - names
    assert not missing, f"the row claims entry points it never fetched: {sorted(missing)} (fetched {sorted(names)})"
    plain2, _, _ = _once(case, ops, monkeypatch, "plain")
    d = _diff("two plain runs differ (the op is not reproducible; nothing below can be read)", plain, plain2)
    assert not d, d
    for tag, byte in (("A (0xFF)", 0xFF), ("B (0x00)", 0x00), ("C (0x3F)", 0x3F)):
        got, alloc, _ = _once(case, ops, monkeypatch, "guard", byte)
        bad = alloc.problems()       # nothing outside written, every input unchanged
        assert not bad, f"run {tag}: " + " | ".join(bad)
        if byte == 0xFF:             # everything written
            stale = _stale(plain, got)
            assert not stale, f"run {tag}: " + " | ".join(stale)
        d = _diff(f"run {tag} differs from the plain run (foreign bytes or stale output contents show in the result)", plain, got)
        assert not d, d
    case.check(plain)
