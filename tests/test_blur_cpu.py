"""The faded blur of D's inputs (blur_init_sigma, blur_fade_kimg) without a GPU: the names of the header
include/littlegan_blur.h; every host-side refusal of its three entry points; the configuration keys; the host restatement config.blur_restate; the numpy restatement of
the operator (blur_np, which tests/test_blur_gpu.py holds the device to) and its symmetry; a trainer built without a device.

The definition (this project's): k steps taken before this one, n real images D reads per step, F = round(blur_fade_kimg * 1000):
  sigma = float32(sigma0 * max(1 - double(k n) / double(F), 0))      R = min(int(floorf(3.0f * sigma)), 30), 0 unless sigma is finite, > 0
  t_i = exp2(-(i / sigma)^2) (fp64), Z = t_0 + 2 sum_{i >= 1} t_i, w_i = float32(t_i / Z)
  h(y, x) = sum_{i = -R..R} w_|i| x(y, x + i),  out(y, x) = sum_{j = -R..R} w_|j| h(y + j, x),  zero outside the image"""
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

BLUR_HEADER = os.path.join(ROOT, "include", "littlegan_blur.h")
ENTRY_POINTS = ("lgblur_init", "lgblur_step", "lgblur_apply")
F32, F64 = np.float32, np.float64
SIGMAS = ((0.2, 0), (0.34, 1), (1.0, 3), (2.7, 8), (10.0, 30))   # (sigma, its R)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement of the operator
def blur_np(x, sigma):
    """Blur(x) by the definition, float64 sums of the fp32 taps; x [rows, S, S, 3], sigma the fp32 value the device reads"""
    from littlegan_amd.config import blur_taps
    x = np.asarray(x, F64)
    R, w = blur_taps(F32(sigma))
    if R == 0:
        return x.copy()
    w = w.astype(F64)
    S = x.shape[1]
    out = x
    for axis in (2, 1):   # H, then V
        pad = [(0, 0)] * 4
        pad[axis] = (R, R)
        xp = np.pad(out, pad)
        acc = np.zeros_like(out)
        for i in range(-R, R + 1):
            sl = [slice(None)] * 4
            sl[axis] = slice(R + i, R + i + S)
            acc = acc + w[abs(i)] * xp[tuple(sl)]
        out = acc
    return out


@pytest.fixture(scope="module")
def lib():
    from littlegan_amd.csrc.build import build
    build(verbose=False)
    from littlegan_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------------------------
# the header include/littlegan_blur.h
def test_blur_header_declares_the_entry_points(lib):
    assert set(_protos(BLUR_HEADER)) == set(ENTRY_POINTS) == {n for n in lib.SIGNATURES if n.startswith("lgblur_")}


def test_the_sources_include_the_header_and_are_built(lib):
    """the header reaches every source through lg_internal.h"""
    assert lib.load().lg_abi_version() == 1
    from littlegan_amd.csrc import build as B
    assert "dblur.hip" in B.SOURCES
    csrc = os.path.join(ROOT, "littlegan_amd", "csrc")
    assert "littlegan_blur.h" in open(os.path.join(csrc, "lg_internal.h")).read()
    assert re.search(r'^#include "lg_internal\.h"', open(os.path.join(csrc, "dblur.hip")).read(), flags=re.M)
    assert "#define DBLUR_MAX_RADIUS 30" in open(BLUR_HEADER).read()


# ---------------------------------------------------------------------------------------------------------------------
# host-side refusals: no launch, the pointers are never dereferenced (there is no device here)
def test_argument_validation_without_gpu(lib):
    h = lib.load()
    err = lambda: h.lg_last_error()
    nan, inf = float("nan"), float("inf")
    st, x, out = C.c_void_p(4096), C.c_void_p(1 << 20), C.c_void_p(2 << 20)

    who = b"lgblur_init"
    assert h.lgblur_init(None, 0, None) == -1 and b"null pointer" in err() and who in err()
    for p in (4097, 4100, 4104):
        assert h.lgblur_init(C.c_void_p(p), 0, None) == -1 and b"aligned" in err() and who in err(), p
    for k0 in (-1, -(1 << 40), 1 << 31, 1 << 40):
        assert h.lgblur_init(st, k0, None) == -1 and b"k0" in err() and who in err(), k0

    who = b"lgblur_step"
    assert h.lgblur_step(None, 1.0, 64, 1000, None) == -1 and b"null pointer" in err() and who in err()
    for p in (4097, 4100, 4104):
        assert h.lgblur_step(C.c_void_p(p), 1.0, 64, 1000, None) == -1 and b"aligned" in err() and who in err(), p
    for bad in (-1.0, -1e-30, nan, inf, -inf):
        assert h.lgblur_step(st, bad, 64, 1000, None) == -1 and b"sigma0" in err() and who in err(), bad
    for bad in (0, -1, (1 << 31) + 1):
        assert h.lgblur_step(st, 1.0, bad, 1000, None) == -1 and b"images_per_step" in err() and who in err(), bad
    for bad in (0, -5, (1 << 40) + 1):
        assert h.lgblur_step(st, 1.0, 64, bad, None) == -1 and b"fade_images" in err() and who in err(), bad

    who = b"lgblur_apply"

    def apply(x=x, st=st, out=out, rows=2, S=16):
        return h.lgblur_apply(x, st, out, rows, S, None)

    for kw in (dict(x=None), dict(st=None), dict(out=None)):
        assert apply(**kw) == -1 and b"null pointer" in err() and who in err(), kw
    assert apply(out=x) == -1 and b"in-place" in err() and who in err()
    for key in ("x", "st", "out"):
        for off in (1, 4, 8, 12):
            assert apply(**{key: C.c_void_p((3 << 20) + off)}) == -1 and b"aligned" in err() and who in err(), (key, off)
    for S in (0, -8, 4, 12, 20, 1028, 1032, 2048):
        assert apply(S=S) == -1 and b"image side" in err() and who in err(), S
    for rows in (0, -1, (1 << 20) + 1):
        assert apply(rows=rows) == -1 and b"row count" in err() and who in err(), rows


# ---------------------------------------------------------------------------------------------------------------------
# configuration
def test_config_keys_default_to_off(tmp_path):
    from littlegan_amd import config
    assert config.DEFAULTS["blur_init_sigma"] == 0.0 and config.DEFAULTS["blur_fade_kimg"] == 200
    assert "blur_init_sigma" in config.__doc__ and "blur_fade_kimg" in config.__doc__
    a = config.Arg(["train", "x"], config_dir=str(tmp_path))
    assert a.blur_init_sigma == 0.0 and a.blur_fade_kimg == 200
    assert config.blur_settings() is None and config.blur_settings(0.0, 200) is None and config.blur_settings(0, 1) is None
    assert config.blur_settings(10, 200) == {"sigma0": 10.0, "fade_images": 200000}
    assert config.blur_settings(0.1, 0.5) == {"sigma0": float(F32(0.1)), "fade_images": 500}       # the fp32 value it is used at
    assert config.blur_settings(2.5, 0.0064) == {"sigma0": 2.5, "fade_images": 6}
    assert config.blur_settings(1.0, (1 << 40) / 1000)["fade_images"] == 1 << 40
    (tmp_path / "b.config.json").write_text(json.dumps({"blur_init_sigma": 3, "blur_fade_kimg": 50}))
    a = config.Arg(["train", "x", "-e", "b"], config_dir=str(tmp_path))
    assert config.blur_settings(a.blur_init_sigma, a.blur_fade_kimg) == {"sigma0": 3.0, "fade_images": 50000}


BAD = [("blur_init_sigma", -0.5), ("blur_init_sigma", 10.5), ("blur_init_sigma", float("nan")), ("blur_init_sigma", float("inf")),
       ("blur_init_sigma", True), ("blur_init_sigma", "1"), ("blur_init_sigma", None), ("blur_init_sigma", [1.0]),
       ("blur_fade_kimg", 0), ("blur_fade_kimg", 0.0004), ("blur_fade_kimg", -1), ("blur_fade_kimg", 2e9), ("blur_fade_kimg", float("nan")),
       ("blur_fade_kimg", float("inf")), ("blur_fade_kimg", True), ("blur_fade_kimg", "200"), ("blur_fade_kimg", None)]


@pytest.mark.parametrize("key,value", BAD, ids=lambda v: str(v))
def test_a_bad_value_raises(tmp_path, key, value):
    from littlegan_amd import config
    kw = {"blur_init_sigma": 1.0, key: value}   # (a bad fade is refused whether the blur is on or not)
    with pytest.raises(ValueError, match=key):
        config.blur_settings(**kw)
    (tmp_path / "bad.config.json").write_text(json.dumps(kw))
    with pytest.raises(ValueError, match=key):
        config.Arg(["train", "x", "-e", "bad"], config_dir=str(tmp_path))
    with pytest.raises(ValueError, match=key):
        _cpu_trainer(**kw)


# ---------------------------------------------------------------------------------------------------------------------
# the host restatement of the schedule and the taps
def test_host_restatement():
    from littlegan_amd import config
    for sigma, R in SIGMAS + ((0.0, 0), (-1.0, 0), (float("nan"), 0), (float("inf"), 0), (1e30, 30), (1.0 / 3.0, 1), (0.3333, 0)):
        assert config.blur_radius(sigma) == R, sigma
    for sigma0, n, kimg in ((10.0, 64, 200), (2.7, 2, 0.01), (1.0, 6, 0.05), (0.34, 32, 1.0)):
        st = config.blur_settings(sigma0, kimg)
        F = st["fade_images"]
        s0, R0, w0 = config.blur_restate(0, n, st)
        assert isinstance(s0, np.float32) and s0 == F32(sigma0) and R0 == config.blur_radius(sigma0)      # sigma(0) == sigma0
        last = -(-F // n)   # the first k with k n >= F
        rs = []
        for k in list(range(0, min(last, 40))) + [last - 1, last, last + 1, 10 * last, (1 << 31) - 1]:
            s, R, w = config.blur_restate(k, n, st)
            assert (s == 0 and R == 0) if k * n >= F else (0 < s <= s0), (k, s)                            # exactly 0 from k n >= F on
            want = F32(F64(F32(sigma0)) * max(F64(1.0) - F64(k * n) / F64(F), F64(0.0)))
            assert s.view(np.int32) == want.view(np.int32), k
            assert w.dtype == np.float32 and w.shape == (R + 1,) and R == config.blur_radius(s)
            full = np.concatenate([w[:0:-1], w]).astype(F64)                                               # symmetric by construction
            assert abs(full.sum() - 1.0) <= 1e-6 and np.all(w > 0) and np.all(np.diff(w) <= 0), (k, full.sum())
            if k <= last:
                rs.append(R)
        assert rs == sorted(rs, reverse=True) and rs[-1] == 0                                              # R never rises
    # the taps of StyleGAN3's filter at sigma = 1: exp2(-i^2), normalised
    R, w = config.blur_taps(1.0)
    t = np.exp2(-np.arange(4.0) ** 2)
    assert R == 3 and np.array_equal(w, (t / (t[0] + 2 * t[1:].sum())).astype(F32))
    R, w = config.blur_taps(1e30)
    assert R == 30 and np.array_equal(w, np.full(31, F32(1.0 / 61.0)))                                     # the 61-tap box


def test_the_restated_operator_is_symmetric():
    """H and V are symmetric under zero fill: the impulse-response matrix of Blur equals its transpose, so Blur is its own adjoint"""
    S = 8
    eye = np.zeros((S * S, S, S, 3))
    for p in range(S * S):
        eye[p, p // S, p % S, :] = 1.0
    for sigma, R in SIGMAS:
        M = blur_np(eye, sigma)[..., 0].reshape(S * S, S * S)       # row p: the response to a one-hot pixel p, read at every q
        assert np.array_equal(M, M.T), sigma
        assert np.array_equal(M, np.eye(S * S)) == (R == 0)
    rng = np.random.default_rng(3)
    for S, (sigma, R) in zip((8, 16, 24, 40, 16), SIGMAS):
        x, g = rng.uniform(-1, 1, (2, S, S, 3)), rng.uniform(-1, 1, (2, S, S, 3))
        a, b = np.sum(blur_np(x, sigma) * g), np.sum(x * blur_np(g, sigma))
        assert abs(a - b) <= 1e-12 * max(abs(a), abs(b)), (S, sigma, a, b)
    x = rng.uniform(-1, 1, (1, 8, 8, 3))
    assert np.array_equal(blur_np(x, 0.2), x)
    # a constant image keeps its value where every tap lies inside: the taps sum to 1
    c = blur_np(np.ones((1, 24, 24, 3)), 1.0)
    from littlegan_amd.config import blur_taps
    half = 0.5 * (1.0 + float(blur_taps(1.0)[1][0]))   # a corner keeps w_0 + ... + w_R of each pass: no renormalisation
    assert np.abs(c[0, 3:-3, 3:-3] - 1.0).max() < 1e-6 and abs(c[0, 0, 0, 0] - half * half) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# a trainer without a device
def test_the_default_path_knows_nothing_of_the_blur(monkeypatch):
    from littlegan_amd import ops
    names = called(monkeypatch, ops)
    blur_names = lambda: [n for n in names if n.startswith("lgblur_")]   # noqa: E731
    base, _ = _cpu_trainer()
    assert base.blur is None and base.blur_sigma_now() is None and not base.blur_live() and not base.blur_live(0)
    assert not hasattr(base, "blur_state") and not hasattr(base, "_blur_k")
    assert "blur_state" not in base.checkpoint_state()
    off, _ = _cpu_trainer(blur_init_sigma=0.0, blur_fade_kimg=200)
    assert off.blur is None and not hasattr(off, "blur_state") and "blur_state" not in off.checkpoint_state()
    assert [off.step_kind(b) for b in range(40)] == [base.step_kind(b) for b in range(40)]
    assert base.step_kind(11) == (-1, True, False)
    assert not blur_names(), names
    for kw, what in ((dict(use_gp=True), "use_gp"), (dict(dropout_train=True), "dropout_train"), (dict(image_channel=1), "3-channel")):
        with pytest.raises(ValueError, match=what):
            _cpu_trainer(blur_init_sigma=2.0, **kw)
    # the blurring path owns a state on the device: without one its construction reaches the wrapper and goes no further
    with pytest.raises(ValueError, match="blur's state"):
        _cpu_trainer(blur_init_sigma=2.0)
    assert not blur_names()      # refused before the library was asked
    ops._lib.load().lgblur_init(None, 0, None)
    assert blur_names() == ["lgblur_init"]      # the recorder does record
