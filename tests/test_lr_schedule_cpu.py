"""Per-network learning rates and the device-side schedule (lr_g / lr_d / lr_adj, lr_schedule, lr_warmup_steps, lr_decay_steps,
lr_final_ratio) without a GPU: the names of the header include/littlegan_sched.h;
every host-side refusal of its four entry points; the configuration keys; the host restatement config.lr_factor that
tests/test_lr_schedule_gpu.py holds the device to; and a trainer built without a device, whose default path knows nothing of the schedule.

The definition (this project's), in fp64 with k the steps taken so far, W the warm-up, N the decay steps, r the fp32 final ratio:
  up = k < W ? (k + 1) / W : 1      t = k < W ? 0 : min((k - W) / N, 1)      d = 1 | 1 - (1 - r) t | r + (1 - r) 0.5 (1 + cos(pi t))
  s = float32(up d)                 lr_m = float32(base_m) * s"""
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

SCHED_HEADER = os.path.join(ROOT, "include", "littlegan_sched.h")
ENTRY_POINTS = ("lgsch_init", "lgsch_step", "lgsch_clip_adam_update", "lgsch_clip_adam_ema_update")
KINDS = ("constant", "linear", "cosine")          # kind 0..2 of lgsch_step, in this order
F32 = np.float32


def settings(schedule="constant", W=0, N=None, r=0.0, lr=5e-5, **rates):
    from littlegan_amd import config
    return config.lr_schedule_settings(lr, lr_schedule=schedule, lr_warmup_steps=W, lr_decay_steps=N, lr_final_ratio=r, **rates)


# ---------------------------------------------------------------------------------------------------------------------
# the header include/littlegan_sched.h
@pytest.fixture(scope="module")
def lib():
    from littlegan_amd.csrc.build import build
    build(verbose=False)
    from littlegan_amd import _lib
    return _lib


def test_sched_header_declares_the_entry_points(lib):
    assert set(_protos(SCHED_HEADER)) == set(ENTRY_POINTS) == {n for n in lib.SIGNATURES if n.startswith("lgsch_")}


def test_the_sources_include_the_header_and_are_built():
    from littlegan_amd.csrc import build as B
    for name in ("loss_optim.hip", "sched.hip"):
        assert "littlegan_sched.h" in open(os.path.join(ROOT, "littlegan_amd", "csrc", name)).read() and name in B.SOURCES


def test_the_adam_arithmetic_is_written_once():
    """the Adam variants sit beside clip_adam_element, which stays the one definition of the arithmetic"""
    lo = open(os.path.join(ROOT, "littlegan_amd", "csrc", "loss_optim.hip")).read()
    assert len(re.findall(r"\bfloat clip_adam_element\(", lo)) == 1
    assert len(re.findall(r"sqrtf\(vv\) \+ eps", lo)) == 1                                   # the update is written once
    assert len(re.findall(r"= lr \* sqrtf\(1\.f - state\[1\]\) / \(1\.f - state\[0\]\);", lo)) == 2
    assert len(re.findall(r"= lr\[0\] \* sqrtf\(1\.f - state\[1\]\) / \(1\.f - state\[0\]\);", lo)) == 2


def test_argument_validation_without_gpu(lib):
    """every refusal happens on the host, before any launch: the pointers are never dereferenced (there is no device here)"""
    h = lib.load()
    err = lambda: h.lg_last_error()
    st = C.c_void_p(4096)
    nan, inf = float("nan"), float("inf")

    who = b"lgsch_init"
    assert h.lgsch_init(None, 0, None) == -1 and b"null pointer" in err() and who in err()
    for p in (4097, 4100, 4104):
        assert h.lgsch_init(C.c_void_p(p), 0, None) == -1 and b"aligned" in err() and who in err(), p
    for k0 in (-1, -(1 << 31)):
        assert h.lgsch_init(st, k0, None) == -1 and b"below 0" in err() and who in err(), k0

    who = b"lgsch_step"

    def step(state=st, kind=1, warmup=2, decay=6, ratio=0.1, g=1e-4, d=2e-4, a=3e-4):
        return h.lgsch_step(state, kind, warmup, decay, ratio, g, d, a, None)

    assert step(state=None) == -1 and b"null pointer" in err() and who in err()
    for p in (4097, 4100, 4104):
        assert step(state=C.c_void_p(p)) == -1 and b"aligned" in err() and who in err(), p
    for kind in (-1, 3, 1 << 20):
        assert step(kind=kind) == -1 and b"bad kind" in err() and who in err(), kind
    for w in (-1, -(1 << 31)):
        assert step(warmup=w) == -1 and b"warmup" in err() and who in err(), w
    for kind in (1, 2):
        for n in (0, -1):
            assert step(kind=kind, decay=n) == -1 and b"decay_steps" in err() and who in err(), (kind, n)
    for r in (-1e-6, 1.0001, nan, inf, -inf):
        assert step(ratio=r) == -1 and b"final_ratio" in err() and who in err(), r
    for bad in (0.0, -1e-4, nan, inf, -inf):
        for key in "gda":
            assert step(**{key: bad}) == -1 and b"finite and > 0" in err() and who in err(), (key, bad)

    who = b"lgsch_clip_adam_update"
    w, g, m, v, s, lr = (C.c_void_p(1024 * (i + 1)) for i in range(6))

    def plain(w=w, g=g, m=m, v=v, s=s, lr=lr, n=8):
        return h.lgsch_clip_adam_update(w, g, m, v, n, s, lr, 0.5, 0.9, 1e-8, 0.5, 1.0, None)

    for kw in (dict(w=None), dict(g=None), dict(m=None), dict(v=None), dict(s=None), dict(lr=None)):
        assert plain(**kw) == -1 and b"null pointer" in err() and who in err(), kw
    for p in (6145, 6146, 6147):
        assert plain(lr=C.c_void_p(p)) == -1 and b"aligned" in err() and who in err(), p
    for n in (0, -1, -(1 << 40)):
        assert plain(n=n) == -1 and b"n=" in err() and who in err(), n

    who = b"lgsch_clip_adam_ema_update"
    ema, es = C.c_void_p(7168), C.c_void_p(8192)

    def fused(w=w, g=g, m=m, v=v, ema=ema, s=s, es=es, lr=lr, n=16, lo=4, hi=12, decay=0.99):
        return h.lgsch_clip_adam_ema_update(w, g, m, v, ema, n, lo, hi, s, es, lr, 0.5, 0.9, 1e-8, 0.5, 1.0, decay, None)

    for kw in (dict(w=None), dict(g=None), dict(m=None), dict(v=None), dict(ema=None), dict(s=None), dict(es=None), dict(lr=None)):
        assert fused(**kw) == -1 and b"null pointer" in err() and who in err(), kw
    for n in (0, -4, 6, 17):
        assert fused(n=n, lo=0, hi=0) == -1 and b"multiple of 4" in err() and who in err(), n
    for lo, hi in ((-4, 8), (8, 4), (0, 20), (2, 8), (4, 10)):
        assert fused(lo=lo, hi=hi) == -1 and b"lo <= hi" in err() and who in err(), (lo, hi)
    for key in ("w", "g", "m", "v", "ema"):
        for off in (4, 8, 12):
            assert fused(**{key: C.c_void_p(16384 + off)}) == -1 and b"aligned" in err() and who in err(), (key, off)
    for p in (6145, 6146, 6147):
        assert fused(lr=C.c_void_p(p)) == -1 and b"aligned" in err() and who in err(), p
    for d in (-0.1, 1.0, 1.5, nan):
        assert fused(decay=d) == -1 and b"decay" in err() and who in err(), d


# ---------------------------------------------------------------------------------------------------------------------
# configuration
def test_config_keys_default_to_off(tmp_path):
    from littlegan_amd import config
    d = config.DEFAULTS
    assert d["lr_g"] is None and d["lr_d"] is None and d["lr_adj"] is None and d["lr_schedule"] == "constant"
    assert d["lr_warmup_steps"] == 0 and d["lr_decay_steps"] is None and d["lr_final_ratio"] == 0.0
    for key in ("lr_g", "lr_d", "lr_adj", "lr_schedule", "lr_warmup_steps", "lr_decay_steps", "lr_final_ratio"):
        assert key in config.__doc__, key
    a = config.Arg(["train", "x"], config_dir=str(tmp_path))
    assert (a.lr_g, a.lr_d, a.lr_adj, a.lr_schedule, a.lr_warmup_steps, a.lr_decay_steps, a.lr_final_ratio) == (None, None, None, "constant", 0, None, 0.0)
    off = config.lr_schedule_settings(a.lr)
    lr32 = float(F32(a.lr))
    assert off == dict(lr_g=lr32, lr_d=lr32, lr_adj=lr32, schedule="constant", kind=0, warmup=0, decay=None, final_ratio=0.0, device=False)
    (tmp_path / "s.config.json").write_text(json.dumps({"lr_d": 2e-4, "lr_schedule": "cosine", "lr_warmup_steps": 100, "lr_decay_steps": 5000,
                                                        "lr_final_ratio": 0.1}))
    a = config.Arg(["train", "x", "-e", "s"], config_dir=str(tmp_path))
    s = config.lr_schedule_settings(a.lr, a.lr_g, a.lr_d, a.lr_adj, a.lr_schedule, a.lr_warmup_steps, a.lr_decay_steps, a.lr_final_ratio)
    assert s == dict(lr_g=lr32, lr_d=float(F32(2e-4)), lr_adj=lr32, schedule="cosine", kind=2, warmup=100, decay=5000,
                     final_ratio=float(F32(0.1)), device=True)
    # the device flag: true exactly when something depends on k
    assert settings(lr_g=1e-3, lr_d=2e-3, lr_adj=3e-3)["device"] is False
    assert settings(W=1)["device"] is True and settings("linear", N=1)["device"] is True and settings("cosine", N=9, r=1.0)["device"] is True
    assert config.LR_SCHEDULE_KINDS == {k: i for i, k in enumerate(KINDS)}
    assert settings(lr=0.0)["lr_g"] == 0.0        # lr = 0 freezes the weights (existing tests do); nothing can be scheduled on it


BAD = [("lr_g", 0.0), ("lr_g", -1e-4), ("lr_d", float("nan")), ("lr_d", float("inf")), ("lr_adj", True), ("lr_adj", "1e-4"), ("lr_g", 1e39),
       ("lr_d", 1e-60), ("lr_g", [1e-4]),
       ("lr_schedule", "cosin"), ("lr_schedule", 1), ("lr_schedule", None), ("lr_schedule", True),
       ("lr_warmup_steps", -1), ("lr_warmup_steps", 2.0), ("lr_warmup_steps", True), ("lr_warmup_steps", "3"), ("lr_warmup_steps", None),
       ("lr_decay_steps", 0), ("lr_decay_steps", -5), ("lr_decay_steps", 7.0), ("lr_decay_steps", True), ("lr_decay_steps", "7"),
       ("lr_final_ratio", -0.1), ("lr_final_ratio", 1.5), ("lr_final_ratio", float("nan")), ("lr_final_ratio", True), ("lr_final_ratio", "0.1"),
       ("lr_final_ratio", None)]


@pytest.mark.parametrize("key,value", BAD, ids=lambda v: str(v))
def test_a_bad_value_raises(tmp_path, key, value):
    from littlegan_amd import config
    good = {"lr_schedule": "linear", "lr_decay_steps": 6}
    with pytest.raises(ValueError, match=key):
        config.lr_schedule_settings(5e-5, **{**good, key: value})
    (tmp_path / "bad.config.json").write_text(json.dumps({**good, key: value}))
    with pytest.raises(ValueError, match=key):
        config.Arg(["train", "x", "-e", "bad"], config_dir=str(tmp_path))
    with pytest.raises(ValueError, match=key):
        _cpu_trainer(**{**good, key: value})


def test_decay_steps_and_the_schedule_need_each_other(tmp_path):
    from littlegan_amd import config
    for kind in ("linear", "cosine"):
        with pytest.raises(ValueError, match="needs lr_decay_steps"):
            config.lr_schedule_settings(5e-5, lr_schedule=kind)
        (tmp_path / "bad.config.json").write_text(json.dumps({"lr_schedule": kind}))
        with pytest.raises(ValueError, match="needs lr_decay_steps"):
            config.Arg(["train", "x", "-e", "bad"], config_dir=str(tmp_path))
    with pytest.raises(ValueError, match="decays nothing"):
        config.lr_schedule_settings(5e-5, lr_decay_steps=100)
    (tmp_path / "bad.config.json").write_text(json.dumps({"lr_decay_steps": 100}))
    with pytest.raises(ValueError, match="decays nothing"):
        config.Arg(["train", "x", "-e", "bad"], config_dir=str(tmp_path))
    with pytest.raises(ValueError, match="decays nothing"):
        _cpu_trainer(lr_decay_steps=100)
    for bad in ("5e-5", True, float("nan"), -1e-5, 1e39):
        with pytest.raises(ValueError, match="lr must be"):
            config.lr_schedule_settings(bad)
    with pytest.raises(ValueError, match="lr must be > 0 under a schedule"):
        config.lr_schedule_settings(0.0, lr_warmup_steps=3)


# ---------------------------------------------------------------------------------------------------------------------
# the host restatement
WS, NS, RS = (0, 1, 3), (1, 7), (0.0, 0.1, 1.0)      # the cases tests/test_lr_schedule_gpu.py runs on the device


def test_host_restatement():
    from littlegan_amd import config
    for W in WS + (10,):
        c = settings(W=W)
        assert c["device"] == (W > 0)
        assert all(config.lr_factor(k, c) == F32(1.0) for k in range(W, W + 20)) and config.lr_factor(2 ** 31 - 1, c) == F32(1.0)
        if W:
            assert config.lr_factor(0, c) == F32(1.0 / W) and config.lr_factor(W - 1, c) == F32(1.0)
            ups = [float(config.lr_factor(k, c)) for k in range(W)]
            assert ups == sorted(ups) and len(set(ups)) == W
        for kind in ("linear", "cosine"):
            for N in NS + (1000,):
                for r in RS:
                    c = settings(kind, W=W, N=N, r=r)
                    r32 = F32(r)
                    assert isinstance(config.lr_factor(0, c), np.float32)
                    if W:
                        assert config.lr_factor(0, c) == F32(1.0 / W) and config.lr_factor(W - 1, c) == F32(1.0)
                    assert config.lr_factor(W, c) == F32(1.0)                                  # t == 0: the decay starts at 1
                    for k in (W + N, W + N + 1, W + N + 5, 2 ** 31 - 2, 2 ** 31 - 1):
                        assert config.lr_factor(k, c) == r32, (kind, W, N, r, k)               # exactly r from the end of the decay on
                    after = [float(config.lr_factor(k, c)) for k in range(W, W + min(N, 64) + 3)]
                    assert all(a >= b for a, b in zip(after, after[1:])), (kind, W, N, r)       # never increases after warm-up
                    assert r == 1.0 or after[0] > after[-1] or N > 64
    # linear is the straight line, cosine half a cosine: against their closed forms
    c = settings("linear", W=2, N=8, r=0.25)
    assert [float(config.lr_factor(k, c)) for k in (0, 1, 2, 6, 10)] == [0.5, 1.0, 1.0, 0.625, 0.25]
    c = settings("cosine", W=0, N=4, r=0.0)
    assert abs(float(config.lr_factor(1, c)) - 0.5 * (1 + np.cos(np.pi / 4))) < 1e-7 and float(config.lr_factor(2, c)) == 0.5
    # the three rates: one fp32 multiply of the fp32 base
    c = settings("linear", W=3, N=7, r=0.1, lr_g=2e-4, lr_adj=1.25e-3)
    for k in (0, 2, 5, 11):
        s = config.lr_factor(k, c)
        assert config.lr_rates(k, c) == (F32(2e-4) * s, F32(5e-5) * s, F32(1.25e-3) * s)
        assert all(isinstance(x, np.float32) for x in config.lr_rates(k, c))


# ---------------------------------------------------------------------------------------------------------------------
# a trainer without a device
def test_the_default_path_knows_nothing_of_the_schedule(monkeypatch):
    from littlegan_amd import ops
    names = called(monkeypatch, ops)
    base, cfg = _cpu_trainer()
    assert base.lr_state is None and base.lr_now() is None and base.lr_sched["device"] is False
    assert [base.opt_cfg[m][0] for m in "GDA"] == [float(F32(cfg.lr))] * 3
    assert "lr_sched_state" not in base.checkpoint_state()
    # rates per network alone: three launch scalars, still no state
    tr, _ = _cpu_trainer(lr_g=1e-4, lr_d=4e-4, lr_adj=2e-3)
    assert tr.lr_state is None and [tr.opt_cfg[m][0] for m in "GDA"] == [float(F32(v)) for v in (1e-4, 4e-4, 2e-3)]
    assert [tr.opt_cfg[m][1:] for m in "GDA"] == [base.opt_cfg[m][1:] for m in "GDA"]
    assert [tr.step_kind(b) for b in range(40)] == [base.step_kind(b) for b in range(40)]
    assert "lr_sched_state" not in tr.checkpoint_state()
    assert not [n for n in names if n.startswith("lgsch_")], names
    # the device path owns a state on the device: without one its construction reaches the wrapper and goes no further
    with pytest.raises(ValueError, match="schedule's state"):
        _cpu_trainer(lr_warmup_steps=2)
