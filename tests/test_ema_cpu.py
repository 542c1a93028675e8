"""Weight average for sampling, the parts that need no GPU: the restatement of the kernel's arithmetic (also the
reference of tests/test_ema_gpu.py), the configuration keys, and the host-side argument checks of the new entry points.

Semantics = tf.train.ExponentialMovingAverage(decay, num_updates):
  d_t = min(decay, (1 + k) / (10 + k)),  ema <- ema - (1 - d_t) (ema - w),  k = averages taken before this one.
The kernel computes d_t in fp32 from the device counter: decay arrives rounded to fp32, the ratio is (1.f + (float)k) / (10.f + (float)k),
the minimum of the two is exact.  `ema_update` applies that d_t in float64."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_abi import _protos  # noqa: E402

EMA_ENTRY_POINTS = ("lg_clip_adam_ema_update", "lg_ema_advance", "lg_swap_f32")


def ema_decay_at(decay, k):
    """d_t as the kernel forms it: fp32-rounded decay, fp32 ratio; returned as a Python float (an fp32 value)."""
    kf = np.float32(k)
    ratio = (np.float32(1.0) + kf) / (np.float32(10.0) + kf)
    return float(min(np.float32(decay), ratio))


def ema_update(ema, w, decay, k):
    """One average in float64 on the arrays `ema` (previous average) and `w` (the weights after the step)."""
    d = ema_decay_at(decay, k)
    ema = np.asarray(ema, np.float64)
    return ema - (1.0 - d) * (ema - np.asarray(w, np.float64))


def test_ramp():
    assert ema_decay_at(0.999, 0) == float(np.float32(0.1))
    assert ema_decay_at(0.05, 0) == float(np.float32(0.05))          # a decay below the ramp's start is taken as it is
    ds = [ema_decay_at(0.999, k) for k in range(0, 20000)]
    assert all(b >= a for a, b in zip(ds, ds[1:]))                   # monotone
    assert ds[-1] == float(np.float32(0.999))                        # (1 + k) / (10 + k) > 0.999 from k = 8990
    assert ds[8000] < ds[-1]
    assert ema_decay_at(0.9, 10 ** 6) == float(np.float32(0.9))
    assert ema_decay_at(0.9, 2 ** 31 - 1) == float(np.float32(0.9))   # the saturated counter
    # k = 0: the first average moves 90 % of the way to the weights
    assert np.allclose(ema_update(np.zeros(3), np.ones(3), 0.999, 0), 1.0 - float(np.float32(0.1)))
    assert np.array_equal(ema_update(np.ones(3), np.ones(3), 0.999, 7), np.ones(3))   # a fixed point


def test_config_defaults():
    from littlegan_amd import config
    assert config.DEFAULTS["ema_decay"] == 0.0 and config.DEFAULTS["sample_ema"] is True
    assert "ema_decay" in config.__doc__ and "sample_ema" in config.__doc__


def test_ema_decay_validation():
    from littlegan_amd.eager_trainer import validate_ema_decay
    assert validate_ema_decay(0) == 0.0 and validate_ema_decay(0.999) == 0.999
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            validate_ema_decay(bad)


def test_trainer_construction_follows_the_key():
    from test_dropout_cpu import _cpu_trainer
    tr, _ = _cpu_trainer()
    assert tr.ema_decay == 0.0 and tr.store.ema is None and tr.store.ema_updates is None
    with tr.ema_weights():        # off: a no-op, no kernel
        pass
    assert tr.checkpoint_state().keys() == {"format", "names", "flat", "adam_m", "adam_v", "beta_powers", "epoch", "input_step"}
    tr, _ = _cpu_trainer(ema_decay=0.99)
    st = tr.store
    assert tr.ema_decay == 0.99 and tr.sample_ema is True
    assert st.ema.shape == st.flat.shape and st.ema.data_ptr() != st.flat.data_ptr() and bool((st.ema == st.flat).all())
    assert st.ema_updates.dtype.is_floating_point is False and int(st.ema_updates) == 0
    assert st.ema.numel() % 4 == 0 and all(s % 4 == 0 and e % 4 == 0 for m in "GDA" for s, e in st.ranges[m])   # 16-byte groups
    ck = tr.checkpoint_state()
    assert ck["format"] == "littlegan_amd-ckpt-1" and ck["ema_updates"] == 0 and ck["ema"].shape == st.flat.shape
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError, match="ema_decay"):
            _cpu_trainer(ema_decay=bad)


def test_header_documents_the_semantics():
    protos = _protos()
    for name in EMA_ENTRY_POINTS:
        assert name in protos, name
    names = [a.split()[-1].lstrip("*") for a in protos["lg_clip_adam_ema_update"][1]]
    assert names == ["w", "g", "m", "v", "ema", "n", "lo", "hi", "adam_state", "ema_state", "lr", "b1", "b2", "eps", "clip", "gscale",
                     "decay", "stream"]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "littlegan_hip.h")).read()
    assert "tf.train.ExponentialMovingAverage" in hdr


@pytest.fixture(scope="module")
def lib():
    from littlegan_amd.csrc.build import build
    build(verbose=False)
    from littlegan_amd import _lib
    return _lib.load()


def test_argument_validation_without_gpu(lib):
    """The host-side checks return before any launch (safe without a GPU).  Pointers are never dereferenced on the host."""
    A = [0x1000 * (i + 1) for i in range(7)]   # seven distinct 16-byte-aligned non-null addresses
    w, g, m, v, ema, st, est = A
    sc = (5e-5, 0.5, 0.9, 1e-8, 0.5, 1.0, 0.999)

    def call(w=w, g=g, m=m, v=v, ema=ema, n=8, lo=0, hi=8, st=st, est=est, sc=sc):
        return lib.lg_clip_adam_ema_update(w, g, m, v, ema, n, lo, hi, st, est, *sc, None)

    for kw in (dict(w=None), dict(g=None), dict(m=None), dict(v=None), dict(ema=None), dict(st=None), dict(est=None)):
        assert call(**kw) == -1, kw
        assert b"lg_clip_adam_ema_update: null pointer" in lib.lg_last_error()
    assert call(n=6, hi=4) == -1 and b"multiple of 4" in lib.lg_last_error()
    assert call(n=0, hi=0) == -1 and b"multiple of 4" in lib.lg_last_error()
    assert call(lo=8, hi=4) == -1 and b"lo <= hi" in lib.lg_last_error()
    assert call(lo=2, hi=8) == -1 and call(hi=6) == -1 and call(hi=12) == -1 and call(lo=-4) == -1
    assert call(ema=ema + 4) == -1 and b"16-byte aligned" in lib.lg_last_error()
    assert call(sc=sc[:6] + (1.0,)) == -1 and b"decay" in lib.lg_last_error()
    assert lib.lg_swap_f32(None, A[1], 8, None) == -1 and b"lg_swap_f32: null pointer" in lib.lg_last_error()
    assert lib.lg_swap_f32(A[0], None, 8, None) == -1 and b"lg_swap_f32: null pointer" in lib.lg_last_error()
    assert lib.lg_swap_f32(A[0], A[1], 6, None) == -1 and b"multiple of 4" in lib.lg_last_error()
    assert lib.lg_swap_f32(A[0], A[1] + 8, 8, None) == -1 and b"16-byte aligned" in lib.lg_last_error()
    assert lib.lg_swap_f32(A[0], A[0], 8, None) == -1
    assert lib.lg_ema_advance(None, None) == -1 and b"lg_ema_advance: null pointer" in lib.lg_last_error()
