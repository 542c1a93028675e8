"""Geometric augmentation of D's inputs (geom_augment) without a GPU: the restatement of the definition, of its adjoint
and of the per-row draws (the oracle of tests/test_geom_gpu.py and of the geom rows of tests/test_memory_contract_gpu.py), the three entry points of
include/littlegan_geom.h (their names, and that they validate before any launch) and the configuration / trainer behaviour.

The definition (include/littlegan_geom.h), per sample x[S][S][3] with the record {a, b, c, d}, h = (S - 1) / 2, u = y - h, v = x - h:
  sy = (a u + b v) + h,  sx = (c u + d v) + h,  y0 = floor(sy),  x0 = floor(sx)
  out_k(y, x) = sum over (i, j) in {y0, y0+1} x {x0, x0+1} of tent(sy - i) tent(sx - j) x_k(i, j),  tent(t) = 1 - |t| for |t| < 1 else 0
a tap outside the image or of weight exactly 0 contributing nothing; coordinates and weights in fp32, one rounding per operation.  A
record with a non-finite entry, or whose fp32 determinant is not finite or below 2^-20 in magnitude, gives zeros.
`geom_taps` restates coordinates and weights in np.float32 in that order; `geom_np` and `geom_adjoint_np` sum over those taps in float64
(the adjoint as a SCATTER: not the device's gather); `geom_def64` takes the coordinates in float64.
Draws: row r of call slot q has ctr = key_offset + (((q << 24) + r) << 1); the geometry reads philox4x32_10({lo, hi, 2, 0}, seed), its
gates the block with third word 3; v_j = word_j >> 8: flip iff v0 < 2^23, k = v1 >> 22, s = exp2(v2 2^-24 - 0.5),
theta = 2 pi (v3 2^-24 - 0.5); M = R(theta) Q^k F / s in float64, rounded to fp32 once."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import input_oracle as IO  # noqa: E402
from test_abi import _protos  # noqa: E402
from test_diffaug_cpu import _cpu_trainer, key_of  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM_HEADER = os.path.join(ROOT, "include", "littlegan_geom.h")
ENTRY_POINTS = ("lgeo_draw", "lgeo_fwd", "lgeo_bwd")
BITS = {"xflip": 1, "rot90": 2, "scale": 4, "rotate": 8}
FULL = "xflip,rot90,scale,rotate"
IDENTITY = np.array([1, 0, 0, 1], np.float32)
F32 = np.float32
M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
def policy_bits(policy):
    return sum(BITS[n] for n in policy.split(",") if n) if isinstance(policy, str) else int(policy)


def _block(seed, ctr, third):
    return [int(v) >> 8 for v in IO.philox4x32_10([ctr & IO.MASK, ctr >> 32, third, 0], [seed & IO.MASK, (seed >> 32) & IO.MASK])]


def gate_threshold(p):
    return int(F32(min(max(F32(p), F32(0)), F32(1))) * F32(16777216.0))


def geom_draw_parts(seed, key_offset, call, r0, rows, policy, p=None):
    """Per row (flip, k, s, theta, on) as the draw selects them: float64, the identity values for a component that is off"""
    bits = policy_bits(policy)
    out = []
    for i in range(rows):
        ctr = (key_offset + (((call << 24) + r0 + i) << 1)) & M64
        v = _block(seed, ctr, 2)
        on = bits
        if p is not None:
            t = gate_threshold(p)
            on &= sum(1 << j for j, g in enumerate(_block(seed, ctr, 3)) if g < t)
        flip = bool(on & 1) and v[0] < (1 << 23)
        k = (v[1] >> 22) if on & 2 else 0
        s = float(np.exp2(v[2] / 16777216.0 - 0.5)) if on & 4 else 1.0
        th = (2 * np.pi) * (v[3] / 16777216.0 - 0.5) if on & 8 else 0.0
        out.append((flip, k, s, th, on))
    return out


def record_of(flip, k, s, th, rotate_on=True):
    """M = R(theta) Q^k F / s in float64, rounded to fp32 once; no negative zero"""
    cs, sn = (np.cos(th), np.sin(th)) if rotate_on else (1.0, 0.0)
    qc, qs, f = (1.0, 0.0, -1.0, 0.0)[k], (0.0, 1.0, 0.0, -1.0)[k], (-1.0 if flip else 1.0)
    p00, p01, p10, p11 = qc, -qs * f, qs, qc * f
    m = np.array([cs * p00 + -sn * p10, cs * p01 + -sn * p11, sn * p00 + cs * p10, sn * p01 + cs * p11], np.float64) / s
    return m.astype(F32) + F32(0)


def geom_records(seed, key_offset, call, r0, rows, S, policy, p=None):
    """The records [rows, 4] float32 of rows r0 .. r0+rows-1 of call slot `call`, as lgeo_draw writes them (p: None = ungated).
    S does not enter the draw: the map is about the image centre, in pixels."""
    parts = geom_draw_parts(seed, key_offset, call, r0, rows, policy, p)
    return np.stack([record_of(flip, k, s, th, bool(on & 8)) for flip, k, s, th, on in parts]) if rows else np.zeros((0, 4), F32)


def usable(rec):
    rec = np.asarray(rec, F32)
    with np.errstate(all="ignore"):
        det = rec[0] * rec[3] - rec[1] * rec[2]
        return bool(np.isfinite(rec).all() and np.isfinite(det) and abs(det) >= F32(2.0 ** -20))


def _tent(t):
    a = np.abs(t)
    return np.where(a < 1, 1 - a, 0).astype(t.dtype)


def _taps(rec, S, dtype):
    """(index [4, S, S] into the flattened source image, -1 = no tap; weight [4, S, S]) with coordinates and weights in `dtype`, in the
    prescribed order of operations; tap order (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1)"""
    idx, w = np.full((4, S, S), -1, np.int64), np.zeros((4, S, S), dtype)
    if not usable(rec):
        return idx, w
    a, b, c, d = (dtype(v) for v in np.asarray(rec, F32))
    h = dtype(S - 1) * dtype(0.5)
    u, v = np.meshgrid(np.arange(S).astype(dtype) - h, np.arange(S).astype(dtype) - h, indexing="ij")
    with np.errstate(all="ignore"):
        sy, sx = (a * u + b * v) + h, (c * u + d * v) + h
        ok = (sy > -1) & (sy < S) & (sx > -1) & (sx < S)      # NaN fails
        y0, x0 = np.floor(np.where(ok, sy, 0)), np.floor(np.where(ok, sx, 0))
        for t in range(4):
            ti, tj = y0 + (t >> 1), x0 + (t & 1)
            wt = (_tent(sy - ti) * _tent(sx - tj)).astype(dtype)
            good = ok & (wt != 0) & (ti >= 0) & (ti < S) & (tj >= 0) & (tj < S)
            idx[t] = np.where(good, ti * S + tj, -1).astype(np.int64)
            w[t] = np.where(good, wt, 0)
    assert sy.dtype == dtype and w.dtype == dtype
    return idx, w


def geom_taps(rec, S):
    """Per destination its (index, weight) pairs, the weights in np.float32 exactly as the kernels compute them"""
    return _taps(rec, S, F32)


def _apply(x, idx, w):
    flat = np.asarray(x, np.float64).reshape(-1, x.shape[-1])
    out = np.zeros(idx.shape[1:] + (x.shape[-1],))
    for t in range(4):
        out += np.where(idx[t] >= 0, w[t].astype(np.float64), 0.0)[..., None] * flat[np.maximum(idx[t], 0)]
    return out


def geom_np(x, recs):
    """Geo(x): float64 sums over the fp32 taps; x [B, S, S, 3], recs [B, 4]"""
    return np.stack([_apply(x[n], *geom_taps(rec, x.shape[1])) for n, rec in enumerate(recs)])


def geom_def64(x, recs):
    """Geo(x) with coordinates and weights in float64 (the records are fp32 numbers)"""
    return np.stack([_apply(x[n], *_taps(rec, x.shape[1], np.float64)) for n, rec in enumerate(recs)])


def geom_adjoint_np(g, recs, stats=False):
    """Geo^T(g) as a scatter over the fp32 taps, float64.  stats: also, per source pixel, the number n of terms [B, S, S] and
    sum |w g| [B, S, S, 3] (the quantities of the device adjoint's rounding bound)"""
    g = np.asarray(g, np.float64)
    B, S = g.shape[:2]
    out, cnt, mag = np.zeros((B, S * S, 3)), np.zeros((B, S * S), np.int64), np.zeros((B, S * S, 3))
    for n, rec in enumerate(recs):
        idx, w = geom_taps(rec, S)
        for t in range(4):
            m = idx[t] >= 0
            term = w[t].astype(np.float64)[m][:, None] * g[n][m]
            np.add.at(out[n], idx[t][m], term)
            np.add.at(mag[n], idx[t][m], np.abs(term))
            np.add.at(cnt[n], idx[t][m], 1)
    out = out.reshape(g.shape)
    return (out, cnt.reshape(B, S, S), mag.reshape(g.shape)) if stats else out


def geom_torch(x, recs):
    """Geo on a float64 torch tensor with the taps as constants (differentiable): the augmentation of the whole-step oracle"""
    S = x.shape[1]
    outs = []
    for n, rec in enumerate(np.asarray(recs, F32)):
        idx, w = geom_taps(rec, S)
        flat = x[n].reshape(S * S, -1)
        acc = 0
        for t in range(4):
            wt = torch.tensor(np.where(idx[t] >= 0, w[t].astype(np.float64), 0.0).reshape(-1, 1), dtype=x.dtype)
            acc = acc + wt * flat[torch.tensor(np.maximum(idx[t], 0).reshape(-1))]
        outs.append(acc.reshape(x[n].shape))
    return torch.stack(outs)


def permutation_records():
    """The 8 records with entries in {0, +-1}: Q^k and Q^k F, with what numpy calls the result"""
    out = []
    for flip in (False, True):
        for k in range(4):
            out.append((record_of(flip, k, 1.0, 0.0, False), flip, k))
    return out


def permuted_np(x, flip, k):
    """Geo(x) under record_of(flip, k) in numpy's words; x [S, S, C].  M = Q^k F maps a destination to its source, out = x o (Q^k F):
    F (applied to the destination first) mirrors the columns of what Q^k gives, and Q sends (u, v) to (-v, u), so out(y, x) =
    in(h - v, h + u): a quarter turn clockwise, np.rot90(in, -1)"""
    out = np.rot90(x, -k, axes=(0, 1))
    return out[:, ::-1] if flip else out


def extreme_records():
    """Records at the ends of the draw's ranges and beyond: s = 2^+-1/2 with theta = +-pi/4, theta = +-pi, a flip with every k,
    generic draws, two non-finite records, det = 0, det just below 2^-20; the identity last"""
    r2 = float(np.sqrt(2.0))
    recs = [record_of(False, 0, s, th) for s in (1 / r2, r2) for th in (np.pi / 4, -np.pi / 4)]
    recs += [record_of(False, 0, 1.0, np.pi), record_of(False, 0, 1.0, -np.pi)]
    recs += [record_of(True, k, 1.0, 0.0, False) for k in range(4)]
    recs += [record_of(True, 1, 0.8, 1.0), record_of(False, 3, 1.3, -2.5), record_of(True, 2, 1 / r2, 3.0)]
    recs += [np.array([np.nan, 0, 0, 1], F32), np.array([1, np.inf, 0, 1], F32),
             np.array([1, 2, 2, 4], F32), np.array([2.0 ** -10, 0, 0, 2.0 ** -11], F32)]
    recs.append(IDENTITY.copy())
    return np.stack(recs).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [8, 16])
def test_restated_adjoint_is_autograd_of_the_restated_forward(S):
    recs = extreme_records()
    rng = np.random.default_rng(S)
    x = rng.uniform(-1, 1, (len(recs), S, S, 3))
    g = rng.uniform(-1, 1, x.shape)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yt = geom_torch(xt, recs)
    assert np.abs(yt.detach().numpy() - geom_np(x, recs)).max() <= 1e-12
    gx, = torch.autograd.grad((yt * torch.tensor(g)).sum(), xt)
    mine, cnt, mag = geom_adjoint_np(g, recs, stats=True)
    assert np.abs(mine - gx.numpy()).max() <= 1e-12
    assert cnt.max() <= 16 and (mag >= np.abs(mine) - 1e-12).all()
    unusable = [n for n, r in enumerate(recs) if not usable(r)]
    assert len(unusable) == 4 and not np.any(geom_np(x, recs)[unusable]) and not np.any(mine[unusable])


@pytest.mark.parametrize("S", [8, 16])
def test_the_eight_permutation_records_are_rot90_and_flip_bit_for_bit(S):
    x = np.random.default_rng(S).uniform(-1, 1, (1, S, S, 3)).astype(F32)
    seen = set()
    for rec, flip, k in permutation_records():
        assert set(np.abs(rec).tolist()) == {0.0, 1.0} and not np.signbit(rec[rec == 0]).any()
        idx, w = geom_taps(rec, S)
        assert ((idx >= 0).sum(0) == 1).all() and set(w[idx >= 0].tolist()) == {1.0}     # exactly one tap, of weight 1
        out = geom_np(x, rec[None]).astype(F32)
        assert np.array_equal(out[0].view(np.uint32), np.ascontiguousarray(permuted_np(x[0], flip, k)).view(np.uint32)), (flip, k)
        back = geom_adjoint_np(out, rec[None]).astype(F32)      # a permutation's adjoint is its inverse
        assert np.array_equal(back.view(np.uint32), x.view(np.uint32))
        seen.add(out.tobytes())
    assert len(seen) == 8
    assert np.array_equal(geom_np(x, IDENTITY[None]).astype(F32).view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("S", [8, 16, 128])
def test_fp32_coordinates_stay_within_their_bound_of_the_float64_definition(S):
    recs = extreme_records()
    x = np.random.default_rng(S).uniform(-1, 1, (len(recs), S, S, 3)).astype(F32)
    err = np.abs(geom_np(x, recs) - geom_def64(x, recs)).reshape(len(recs), -1).max(1)
    bound = 16 * S * 2.0 ** -24 * np.abs(x).max()
    print(f"S={S}: fp32 coordinates use {100 * err.max() / bound:.1f} % of 16 S 2^-24 max|x| (per record {np.round(err / bound, 3)})")
    assert (err <= bound).all(), (err, bound)


def test_draws_cover_their_ranges():
    seed, koff = key_of(5, 0, 3)
    parts = geom_draw_parts(seed, koff, 0, 0, 4096, FULL)
    flips, ks, ss, ths = (np.array([q[i] for q in parts]) for i in range(4))
    assert set(ks.tolist()) == {0, 1, 2, 3}
    assert ss.min() >= 2 ** -0.5 and ss.max() < 2 ** 0.5 and ss.min() < 0.72 and ss.max() > 1.40
    assert ths.min() >= -np.pi and ths.max() < np.pi and ths.min() < -3.1 and ths.max() > 3.1
    assert abs(flips.sum() - 2048) <= 4 * np.sqrt(4096 * 0.25)
    recs = geom_records(seed, koff, 0, 0, 4096, 16, FULL)
    det = recs[:, 0].astype(np.float64) * recs[:, 3] - recs[:, 1].astype(np.float64) * recs[:, 2]
    assert recs.dtype == F32 and np.allclose(np.abs(det), 1 / ss ** 2, rtol=1e-6) and ((det < 0) == flips).all()


def test_a_policy_subset_leaves_the_rest_at_identity():
    seed, koff = key_of(0, 1, 2)
    full = geom_draw_parts(seed, koff, 1, 0, 16, 15)
    ident = (False, 0, 1.0, 0.0)
    for bits in range(16):
        names = ",".join(n for n, v in BITS.items() if bits & v)
        parts = geom_draw_parts(seed, koff, 1, 0, 16, names)
        for j in range(4):
            assert [q[j] for q in parts] == [(f[j] if bits >> j & 1 else ident[j]) for f in full], (names, j)
        recs = geom_records(seed, koff, 1, 0, 16, 16, names)
        if not bits & 12:     # blits only: exact 0 / +-1
            assert set(np.abs(recs).ravel().tolist()) <= {0.0, 1.0}
    assert np.array_equal(geom_records(seed, koff, 1, 0, 4, 16, ""), np.tile(IDENTITY, (4, 1)))


def test_gates():
    seed, koff = key_of(1, 0, 4)
    ungated = geom_records(seed, koff, 0, 0, 64, 16, FULL)
    assert np.array_equal(geom_records(seed, koff, 0, 0, 64, 16, FULL, p=0.0), np.tile(IDENTITY, (64, 1)))
    assert np.array_equal(geom_records(seed, koff, 0, 0, 64, 16, FULL, p=1.0).view(np.uint32), ungated.view(np.uint32))
    n = 2048
    on = np.array([q[4] for q in geom_draw_parts(seed, koff, 0, 0, n, FULL, p=0.3)])
    p = gate_threshold(0.3) / 2.0 ** 24
    for j in range(4):
        rate = (on >> j & 1).mean()
        assert abs(rate - p) <= 4 * np.sqrt(p * (1 - p) / n), (j, rate)
    assert len({int(v) for v in on}) > 8      # the four gates are independent draws, not one


def test_a_row_range_is_the_slice_of_the_whole_and_slots_differ():
    seed, koff = key_of(2, 0, 9)
    whole = geom_records(seed, koff, 0, 0, 6, 16, FULL)
    assert np.array_equal(geom_records(seed, koff, 0, 3, 3, 16, FULL), whole[3:])
    assert np.array_equal(geom_records(seed, koff, 0, 3, 3, 16, FULL, p=0.5), geom_records(seed, koff, 0, 0, 6, 16, FULL, p=0.5)[3:])
    assert not np.array_equal(geom_records(seed, koff, 1, 0, 6, 16, FULL), whole)
    assert not np.array_equal(geom_records(*key_of(2, 0, 10), 0, 0, 6, 16, FULL), whole)
    assert np.array_equal(geom_records(seed, koff, 0, 0, 6, 128, FULL), whole)     # S does not enter the draw


# ---------------------------------------------------------------------------------------------------------------------
def test_config_key_and_its_bad_strings(tmp_path):
    from littlegan_amd import config
    assert config.DEFAULTS["geom_augment"] == "" and "geom_augment" in config.__doc__ and config.GEOM_AUGMENT_BITS == BITS
    assert config.Arg(["train", "x"], config_dir=str(tmp_path)).geom_augment == ""
    (tmp_path / "geo.config.json").write_text('{"geom_augment": "xflip,rotate"}')
    assert config.Arg(["train", "x", "-e", "geo"], config_dir=str(tmp_path)).geom_augment == "xflip,rotate"
    for names, bits in (("", 0), ("xflip", 1), ("rot90", 2), ("scale", 4), ("rotate", 8), (FULL, 15), ("rotate, xflip", 9), (None, 0)):
        assert config.geom_augment_bits(names) == bits
    for bad in ("flip", "xflip,color", "xflip;rot90", ",", "xflip,", "shear", 7):
        with pytest.raises(ValueError, match="geom_augment"):
            config.geom_augment_bits(bad)
    for still_bad in ("xflip", "color,flip", "shear"):       # the names of this key are no names of diff_augment
        with pytest.raises(ValueError, match="diff_augment"):
            config.diff_augment_bits(still_bad)
    (tmp_path / "bad.config.json").write_text('{"geom_augment": "xflip,translation"}')
    with pytest.raises(ValueError, match="geom_augment"):
        config.Arg(["train", "x", "-e", "bad"], config_dir=str(tmp_path))
    (tmp_path / "ada.config.json").write_text('{"geom_augment": "xflip", "ada_target": 0.6}')
    assert config.Arg(["train", "x", "-e", "ada"], config_dir=str(tmp_path)).ada_target == 0.6


def test_ada_settings_with_and_without_the_new_argument():
    from littlegan_amd import config
    want = {"p0": 0.5, "target": None, "interval": 4, "per_row": float(F32(1 / 500000.0))}
    assert config.ada_settings("color", 0.5) == want == config.ada_settings("color", 0.5, geom_augment="")
    assert config.ada_settings("", 0.5, geom_augment="rot90") == want == config.ada_settings("color", 0.5, geom_augment="rot90")
    assert config.ada_settings("", geom_augment="rot90") is None and config.ada_settings("", 1.0, geom_augment="rot90") is None
    assert config.ada_settings("", None, 0.6, 2, 0.048, "scale")["target"] == float(F32(0.6))
    for kw in (dict(diff_augment_p=0.5), dict(ada_target=0.6)):
        with pytest.raises(ValueError, match="need diff_augment"):
            config.ada_settings("", **kw)
        with pytest.raises(ValueError, match="need diff_augment"):
            config.ada_settings("", geom_augment="", **kw)
    with pytest.raises(ValueError, match="geom_augment"):
        config.ada_settings("", 0.5, geom_augment="shear")


def test_trainer_settings_refusals_and_the_missing_key():
    tr, _ = _cpu_trainer()
    assert tr.geom == 0 and tr.diffaug == 0 and not tr.augmenting
    tr, _ = _cpu_trainer(geom_augment="rotate,xflip")
    assert tr.geom == 9 and tr.diffaug == 0 and tr.augmenting and tr.ada is None
    tr, _ = _cpu_trainer(geom_augment="scale", diff_augment="color")
    assert tr.geom == 4 and tr.diffaug == 1 and tr.augmenting
    with pytest.raises(ValueError, match="geom_augment and use_gp"):
        _cpu_trainer(geom_augment="xflip", use_gp=True)
    with pytest.raises(ValueError, match="geom_augment and dropout_train"):
        _cpu_trainer(geom_augment="xflip", dropout_train=True)
    with pytest.raises(ValueError, match="geom_augment needs 3-channel"):
        _cpu_trainer(geom_augment="xflip", image_channel=1)
    with pytest.raises(ValueError, match="geom_augment"):
        _cpu_trainer(geom_augment="shear")
    with pytest.raises(ValueError, match="need diff_augment"):
        _cpu_trainer(ada_target=0.6)
    _cpu_trainer(geom_augment="", use_gp=True)     # off: the key alone changes nothing
    tr, _ = _cpu_trainer(geom_augment=FULL, seed=3)
    inp = {k: torch.zeros(2, 3) for k in ("real_image_1", "real_cond_1", "real_image_2", "real_cond_2", "noise", "new_image")}
    with pytest.raises(ValueError, match="geom_augment is on and inp has no 'diffaug_key'"):
        tr.train_step_from_inputs(1, inp)
    tr.rank, tr._input_step = 1, 7
    assert tr.diffaug_key_words() == key_of(3, 1, 7)      # the step's one augmentation key


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from littlegan_amd.csrc.build import build
    build(verbose=False)
    from littlegan_amd import _lib
    return _lib


def test_geom_header_declares_the_entry_points(lib):
    assert set(_protos(GEOM_HEADER)) == set(ENTRY_POINTS) == {n for n in lib.SIGNATURES if n.startswith("lgeo_")}


def test_the_source_includes_the_header_and_is_built():
    from littlegan_amd.csrc import build as B
    assert "littlegan_geom.h" in open(os.path.join(ROOT, "littlegan_amd", "csrc", "geom.hip")).read() and "geom.hip" in B.SOURCES


def test_argument_validation_without_gpu(lib):
    h = lib.load()
    d, d2, d3 = C.c_void_p(64), C.c_void_p(128), C.c_void_p(256)   # never dereferenced: every call must fail its host-side checks first
    err = lambda: h.lg_last_error()

    def refused(rc, what, name):
        return rc == -1 and what in err() and name in err()
    # lgeo_draw(key, call, r0, rows, S, policy_bits, state, geo, stream)
    n = b"lgeo_draw"
    assert refused(h.lgeo_draw(None, 0, 0, 4, 16, 15, None, d2, None), b"null pointer", n)
    assert refused(h.lgeo_draw(d, 0, 0, 4, 16, 15, None, None, None), b"null pointer", n)
    assert refused(h.lgeo_draw(d, -1, 0, 4, 16, 15, None, d2, None), b"call slot", n)
    assert refused(h.lgeo_draw(d, 4, 0, 4, 16, 15, None, d2, None), b"call slot", n)
    assert refused(h.lgeo_draw(d, 0, 0, 0, 16, 15, None, d2, None), b"rows", n)
    assert refused(h.lgeo_draw(d, 0, 0, -2, 16, 15, None, d2, None), b"rows", n)
    assert refused(h.lgeo_draw(d, 0, 0, (1 << 20) + 1, 16, 15, None, d2, None), b"rows", n)
    assert refused(h.lgeo_draw(d, 0, -1, 4, 16, 15, None, d2, None), b"rows", n)
    assert refused(h.lgeo_draw(d, 0, (1 << 24) - 2, 4, 16, 15, None, d2, None), b"rows", n)
    assert refused(h.lgeo_draw(d, 0, 0, 4, 4, 15, None, d2, None), b"image side", n)
    assert refused(h.lgeo_draw(d, 0, 0, 4, 20, 15, None, d2, None), b"image side", n)
    assert refused(h.lgeo_draw(d, 0, 0, 4, 2048, 15, None, d2, None), b"image side", n)
    assert refused(h.lgeo_draw(d, 0, 0, 4, 16, 16, None, d2, None), b"policy bits", n)
    assert refused(h.lgeo_draw(d, 0, 0, 4, 16, -1, None, d2, None), b"policy bits", n)
    assert refused(h.lgeo_draw(C.c_void_p(68), 0, 0, 4, 16, 15, None, d2, None), b"aligned", n)
    assert refused(h.lgeo_draw(d, 0, 0, 4, 16, 15, None, C.c_void_p(136), None), b"aligned", n)
    assert refused(h.lgeo_draw(d, 0, 0, 4, 16, 15, C.c_void_p(136), d2, None), b"aligned", n)
    for fn, name in ((h.lgeo_fwd, b"lgeo_fwd"), (h.lgeo_bwd, b"lgeo_bwd")):
        # (x, geo, out, rows, S, stream)
        for k in range(3):
            ptrs = [d, d2, d3]
            ptrs[k] = None
            assert refused(fn(*ptrs, 2, 16, None), b"null pointer", name)
        assert refused(fn(d, d2, d, 2, 16, None), b"in-place", name)
        assert refused(fn(d, d2, d3, 0, 16, None), b"row count", name)
        assert refused(fn(d, d2, d3, -3, 16, None), b"row count", name)
        assert refused(fn(d, d2, d3, (1 << 20) + 1, 16, None), b"row count", name)
        assert refused(fn(d, d2, d3, 2, 4, None), b"image side", name)
        assert refused(fn(d, d2, d3, 2, 12, None), b"image side", name)
        assert refused(fn(d, d2, d3, 2, 1032, None), b"image side", name)
        for k in range(3):
            ptrs = [d, d2, d3]
            ptrs[k] = C.c_void_p(ptrs[k].value + 4)
            assert refused(fn(*ptrs, 2, 16, None), b"aligned", name)
