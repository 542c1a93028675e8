"""Global-norm gradient clipping and the non-finite step guard (clip_norm, skip_nonfinite) without a GPU: the configuration
keys; the names of the header include/littlegan_guard.h; every host-side refusal of its eight entry points; lgg_partials_count; the host
restatement config.grad_guard_restate that tests/test_grad_guard_gpu.py holds the device to; and a trainer built without a device, whose
default path knows nothing of the guard.

The definition (this project's), per network over the n gradient elements it trains this step, gscale = 1 / world:
  S = sum (double)g_i (double)g_i     bad = !isfinite(S)     N = float32(sqrt(S) * gscale)
  c = 1 if clip_norm == 0 or bad, else q = clip_norm / (N + 1e-6f), q < 1 ? q : 1      eff = gscale * c      skip_now = bad && skip"""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guards import called  # noqa: E402
from test_abi import ROOT, _protos  # noqa: E402
from test_diffaug_cpu import _cpu_trainer  # noqa: E402

GUARD_HEADER = os.path.join(ROOT, "include", "littlegan_guard.h")
ENTRY_POINTS = ("lgg_partials_count", "lgg_workspace_bytes", "lgg_init", "lgg_sumsq_partial", "lgg_finalise", "lgg_clip_adam_update",
                "lgg_clip_adam_ema_update", "lgg_adam_advance")
CH, PMAX = 16384, 1024
F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    from littlegan_amd.csrc.build import build
    build(verbose=False)
    from littlegan_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------------------------
# the header include/littlegan_guard.h
def test_guard_header_declares_the_entry_points(lib):
    assert set(_protos(GUARD_HEADER)) == set(ENTRY_POINTS) == {n for n in lib.SIGNATURES if n.startswith("lgg_")}


def test_the_sources_include_the_header_and_are_built(lib):
    """the header reaches every source through lg_internal.h; the guarded Adam kernels call the one pass, which calls the one element"""
    assert lib.load().lg_abi_version() == 1
    from littlegan_amd.csrc import build as B
    assert "gradguard.hip" in B.SOURCES
    csrc = os.path.join(ROOT, "littlegan_amd", "csrc")
    assert "littlegan_guard.h" in open(os.path.join(csrc, "lg_internal.h")).read()
    assert re.search(r'^#include "lg_internal\.h"', open(os.path.join(csrc, "gradguard.hip")).read(), flags=re.M)
    lo = open(os.path.join(csrc, "loss_optim.hip")).read()
    assert len(re.findall(r"\bfloat clip_adam_element\(", lo)) == 1 and len(re.findall(r"sqrtf\(vv\) \+ eps", lo)) == 1
    assert "clip_adam_pass(w, g, m, v, n," in lo.split("clip_adam_gg_kernel")[1].split("__global__")[0]
    assert "clip_adam_ema_pass(w, g, m, v, ema," in lo.split("clip_adam_ema_gg_kernel")[1].split("__global__")[0]


# ---------------------------------------------------------------------------------------------------------------------
# host-side refusals: no launch, the pointers are never dereferenced (there is no device here)
def test_argument_validation_without_gpu(lib):
    h = lib.load()
    err = lambda: h.lg_last_error()
    nan, inf = float("nan"), float("inf")
    rec, part, g = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(16384)

    who = b"lgg_init"
    assert h.lgg_init(None, 0, 0, None) == -1 and b"null pointer" in err() and who in err()
    for p in (4097, 4100, 4104):
        assert h.lgg_init(C.c_void_p(p), 0, 0, None) == -1 and b"aligned" in err() and who in err(), p
    for a, b in ((-1, 0), (0, -1), (-(1 << 31), 0)):
        assert h.lgg_init(rec, a, b, None) == -1 and b"below 0" in err() and who in err(), (a, b)

    who = b"lgg_sumsq_partial"

    def partial(g=g, n=5, part=part, nbytes=None):
        return h.lgg_sumsq_partial(g, n, part, h.lgg_workspace_bytes(n) if nbytes is None else nbytes, None)

    for kw in (dict(g=None), dict(part=None)):
        assert partial(**kw) == -1 and b"null pointer" in err() and who in err(), kw
    for n in (0, -1, -(1 << 40)):
        assert partial(n=n, nbytes=8192) == -1 and b"below 1" in err() and who in err(), n
    for p in (16385, 16386, 16387):
        assert partial(g=C.c_void_p(p)) == -1 and b"aligned" in err() and who in err(), p
    for p in (8193, 8194, 8196):
        assert partial(part=C.c_void_p(p)) == -1 and b"aligned" in err() and who in err(), p
    for n in (1, CH, CH + 1, 5 * CH, 1024 * CH + 5):
        need = h.lgg_workspace_bytes(n)
        for nb in (0, need - 8, need - 1):
            assert partial(n=n, nbytes=nb) == -1 and b"partial_bytes" in err() and who in err(), (n, nb)

    who = b"lgg_finalise"

    def final(part=part, n=5, rec=rec, gscale=1.0, clip=1.0, skip=1):
        return h.lgg_finalise(part, n, rec, gscale, clip, skip, None)

    for kw in (dict(part=None), dict(rec=None)):
        assert final(**kw) == -1 and b"null pointer" in err() and who in err(), kw
    for n in (0, -1):
        assert final(n=n) == -1 and b"below 1" in err() and who in err(), n
    for p in (4097, 4100, 4104):
        assert final(rec=C.c_void_p(p)) == -1 and b"aligned" in err() and who in err(), p
    for p in (8193, 8196):
        assert final(part=C.c_void_p(p)) == -1 and b"aligned" in err() and who in err(), p
    for bad in (0.0, -0.5, nan, inf, -inf):
        assert final(gscale=bad) == -1 and b"gscale" in err() and who in err(), bad
    for bad in (-1e-6, -1.0, nan, inf, -inf):
        assert final(clip=bad) == -1 and b"clip_norm" in err() and who in err(), bad
    for bad in (-1, 2, 1 << 20):
        assert final(skip=bad) == -1 and b"skip" in err() and who in err(), bad

    who = b"lgg_clip_adam_update"
    w, gr, m, v, s, lr = (C.c_void_p(1024 * (i + 1)) for i in range(6))
    rc = C.c_void_p(7168)

    def plain(w=w, g=gr, m=m, v=v, s=s, lr=lr, rec=rc, n=8):
        return h.lgg_clip_adam_update(w, g, m, v, n, s, lr, rec, 0.5, 0.9, 1e-8, 0.5, None)

    for kw in (dict(w=None), dict(g=None), dict(m=None), dict(v=None), dict(s=None), dict(lr=None), dict(rec=None)):
        assert plain(**kw) == -1 and b"null pointer" in err() and who in err(), kw
    for p in (6145, 6146, 6147):
        assert plain(lr=C.c_void_p(p)) == -1 and b"aligned" in err() and who in err(), p
    for p in (7169, 7172, 7176):
        assert plain(rec=C.c_void_p(p)) == -1 and b"aligned" in err() and who in err(), p
    for n in (0, -1, -(1 << 40)):
        assert plain(n=n) == -1 and b"n=" in err() and who in err(), n

    who = b"lgg_clip_adam_ema_update"
    ema, es = C.c_void_p(9216), C.c_void_p(10240)

    def fused(w=w, g=gr, m=m, v=v, ema=ema, s=s, es=es, lr=lr, rec=rc, n=16, lo=4, hi=12, decay=0.99):
        return h.lgg_clip_adam_ema_update(w, g, m, v, ema, n, lo, hi, s, es, lr, rec, 0.5, 0.9, 1e-8, 0.5, decay, None)

    for kw in (dict(w=None), dict(g=None), dict(m=None), dict(v=None), dict(ema=None), dict(s=None), dict(es=None), dict(lr=None),
               dict(rec=None)):
        assert fused(**kw) == -1 and b"null pointer" in err() and who in err(), kw
    for n in (0, -4, 6, 17):
        assert fused(n=n, lo=0, hi=0) == -1 and b"multiple of 4" in err() and who in err(), n
    for lo, hi in ((-4, 8), (8, 4), (0, 20), (2, 8), (4, 10)):
        assert fused(lo=lo, hi=hi) == -1 and b"lo <= hi" in err() and who in err(), (lo, hi)
    for key in ("w", "g", "m", "v", "ema", "rec"):
        for off in (4, 8, 12):
            assert fused(**{key: C.c_void_p(32768 + off)}) == -1 and b"aligned" in err() and who in err(), (key, off)
    for p in (6145, 6146, 6147):
        assert fused(lr=C.c_void_p(p)) == -1 and b"aligned" in err() and who in err(), p
    for d in (-0.1, 1.0, 1.5, nan):
        assert fused(decay=d) == -1 and b"decay" in err() and who in err(), d

    who = b"lgg_adam_advance"
    assert h.lgg_adam_advance(None, rc, 0.5, 0.9, None) == -1 and b"null pointer" in err() and who in err()
    assert h.lgg_adam_advance(s, None, 0.5, 0.9, None) == -1 and b"null pointer" in err() and who in err()
    for p in (7169, 7172, 7176):
        assert h.lgg_adam_advance(s, C.c_void_p(p), 0.5, 0.9, None) == -1 and b"aligned" in err() and who in err(), p


def test_partials_count(lib):
    h = lib.load()
    ns = [1, 2, 255, CH - 1, CH, CH + 1, 2 * CH, 2 * CH + 7, 100 * CH, 1023 * CH, 1023 * CH + 1, 1024 * CH, 1024 * CH + 5, 5000 * CH,
          (1 << 40) + 3]
    got = [h.lgg_partials_count(n) for n in ns]
    assert got == [min(PMAX, -(-n // CH)) for n in ns]                       # a pure function of n
    assert got == sorted(got) and max(got) == PMAX and got[-3:] == [PMAX] * 3  # monotone, capped at 1024
    assert all(h.lgg_partials_count(n) == 1 for n in (1, 7, CH - 1, CH)) and h.lgg_partials_count(CH + 1) == 2
    assert [h.lgg_partials_count(n) for n in ns] == got                       # equal on repeated calls
    assert [h.lgg_workspace_bytes(n) for n in ns] == [8 * p for p in got]
    assert h.lgg_partials_count(0) == 0 and h.lgg_partials_count(-5) == 0 and h.lgg_workspace_bytes(0) == 0
    from littlegan_amd import ops
    assert (ops.GUARD_CHUNK, ops.GUARD_MAX_PARTIALS) == (CH, PMAX)
    hdr = open(GUARD_HEADER).read()
    assert f"#define GG_CHUNK {CH}" in hdr and f"#define GG_MAX_PARTIALS {PMAX}" in hdr


# ---------------------------------------------------------------------------------------------------------------------
# configuration
def test_config_keys_default_to_off(tmp_path):
    from littlegan_amd import config
    assert config.DEFAULTS["clip_norm"] is None and config.DEFAULTS["skip_nonfinite"] is False
    assert "clip_norm" in config.__doc__ and "skip_nonfinite" in config.__doc__
    a = config.Arg(["train", "x"], config_dir=str(tmp_path))
    assert a.clip_norm is None and a.skip_nonfinite is False
    assert config.grad_guard_settings() is None and config.grad_guard_settings(None, False) is None
    assert config.grad_guard_settings(2.5) == {"clip_norm": 2.5, "skip": False}
    assert config.grad_guard_settings(None, True) == {"clip_norm": 0.0, "skip": True}
    assert config.grad_guard_settings(0.1, True) == {"clip_norm": float(F32(0.1)), "skip": True}       # the fp32 value it is used at
    assert config.grad_guard_settings(3, True) == {"clip_norm": 3.0, "skip": True}
    (tmp_path / "g.config.json").write_text(json.dumps({"clip_norm": 10, "skip_nonfinite": True}))
    a = config.Arg(["train", "x", "-e", "g"], config_dir=str(tmp_path))
    assert config.grad_guard_settings(a.clip_norm, a.skip_nonfinite) == {"clip_norm": 10.0, "skip": True}


BAD = [("clip_norm", 0), ("clip_norm", 0.0), ("clip_norm", -1.0), ("clip_norm", float("nan")), ("clip_norm", float("inf")),
       ("clip_norm", 1e39), ("clip_norm", True), ("clip_norm", "1"), ("clip_norm", 1e-60), ("clip_norm", [1.0]),
       ("skip_nonfinite", 1), ("skip_nonfinite", "yes"), ("skip_nonfinite", None), ("skip_nonfinite", 0)]


@pytest.mark.parametrize("key,value", BAD, ids=lambda v: str(v))
def test_a_bad_value_raises(tmp_path, key, value):
    from littlegan_amd import config
    with pytest.raises(ValueError, match=key):
        config.grad_guard_settings(**{key: value})
    (tmp_path / "bad.config.json").write_text(json.dumps({key: value}))
    with pytest.raises(ValueError, match=key):
        config.Arg(["train", "x", "-e", "bad"], config_dir=str(tmp_path))
    with pytest.raises(ValueError, match=key):
        _cpu_trainer(**{key: value})


# ---------------------------------------------------------------------------------------------------------------------
# the host restatement
def test_host_restatement():
    from littlegan_amd import config
    R = config.grad_guard_restate
    rng = np.random.default_rng(5)
    g = rng.standard_normal(1000).astype(F32)
    S = float(np.sum(g.astype(np.float64) ** 2))
    for gscale in (1.0, 0.5, 0.125, 1.0 / 3.0):
        gs = F32(gscale)
        N = F32(np.sqrt(np.float64(S)) * np.float64(gs))
        # clip_norm around N + 1e-6: c == 1 exactly when N + 1e-6f <= clip_norm, and eff == gscale bit for bit then
        d = N + F32(1e-6)
        for clip in (np.nextafter(d, F32(0)), d, np.nextafter(d, F32(np.inf)), F32(0.5) * d, F32(2) * d, F32(1e30), F32(1e-30)):
            r = R(g, gscale, float(clip), True)
            assert r["S"] == S and r["N"] == N and not r["bad"] and not r["skip_now"]
            assert all(isinstance(r[k], np.float32) for k in ("N", "c", "eff")) and isinstance(r["S"], np.float64)
            assert (r["c"] == F32(1.0)) == bool(d <= clip), (gscale, clip)
            if d <= clip:
                assert r["eff"].view(np.int32) == gs.view(np.int32)
            else:
                assert r["c"] == clip / d and r["c"] < 1 and r["eff"] == gs * r["c"]
        r = R(g, gscale, 0.0, True)          # clip_norm 0: no clipping
        assert r["c"] == 1 and r["eff"] == gs and r["N"] == N
        assert R(None, gscale, 1.0, False, sumsq=S) == R(g, gscale, 1.0, False)      # from a given S: g is not read
    # bad: a NaN, a +Inf, a -Inf anywhere; c = 1 then, whatever clip_norm; skip_now only with skip
    for poison in (np.nan, np.inf, -np.inf):
        for at in (0, 500, 999):
            gb = g.copy()
            gb[at] = poison
            for skip in (False, True):
                r = R(gb, 0.5, 1e-3, skip)
                assert r["bad"] and r["skip_now"] == skip and r["c"] == 1 and r["eff"] == F32(0.5) and not np.isfinite(r["N"])
    # the largest finite fp32, a million times: S stays finite (no false alarm), N overflows fp32 and the scale goes to 0
    big = np.full(1 << 20, np.finfo(F32).max, F32)
    r = R(big, 1.0, 1.0, True)
    assert np.isfinite(r["S"]) and not r["bad"] and np.isinf(r["N"]) and r["c"] == 0 and r["eff"] == 0
    z = R(np.zeros(7, F32), 1.0, 1.0, True)
    assert z["S"] == 0 and z["N"] == 0 and z["c"] == 1 and not z["bad"]


# ---------------------------------------------------------------------------------------------------------------------
# a trainer without a device
def test_the_default_path_knows_nothing_of_the_guard(monkeypatch):
    from littlegan_amd import ops
    names = called(monkeypatch, ops)
    guard_names = lambda: [n for n in names if n.startswith("lgg_")]   # noqa: E731
    base, _ = _cpu_trainer()
    assert base.guard is None and base.grad_norm_now() is None and base.guard_counts() is None
    assert not hasattr(base, "guard_state") and not hasattr(base, "_guard_ws") and not hasattr(base, "_guard_lr")
    assert "grad_guard_state" not in base.checkpoint_state()
    off, _ = _cpu_trainer(clip_norm=None, skip_nonfinite=False)
    assert off.guard is None and not hasattr(off, "guard_state")
    assert [off.step_kind(b) for b in range(40)] == [base.step_kind(b) for b in range(40)]
    assert not guard_names(), names
    # the guarded path owns records on the device: without one its construction reaches the wrapper and goes no further
    for kw in (dict(clip_norm=1.0), dict(skip_nonfinite=True)):
        with pytest.raises(ValueError, match="guard's record"):
            _cpu_trainer(**kw)
    assert not guard_names()      # refused by the wrapper, before the library was asked
    h = ops._lib.load()
    h.lgg_partials_count(5)
    assert guard_names() == ["lgg_partials_count"]      # the recorder does record
