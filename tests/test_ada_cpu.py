"""Adaptive augmentation probability (ADA) without a GPU: the restatement of the gate and of the controller (the oracle
of tests/test_ada_gpu.py), the entry points of include/littlegan_hip_ext.h (the names; validating before any launch: the whole ABI is
held to its table and its ledger by tests/test_abi.py and tests/test_guards_cpu.py), and the configuration / trainer behaviour.

The gate: row r of call slot q under {seed, key_offset} has the first counter ctr = key_offset + (((q << 24) + r) << 1); its record reads
the Philox blocks {lo(ctr), hi(ctr), 0, 0} and {lo(ctr + 1), hi(ctr + 1), 0, 0} (tests/test_diffaug_cpu.py), its gates the block
{lo(ctr), hi(ctr), 1, 0}: w_j = word_j >> 8 for j = 0 color, 1 translation, 2 cutout; with t = (unsigned)(float32(p) * 2^24) component j
is on iff w_j < t, and a component that is off gets its identity values.
The controller: state = {fp32 p, int32 sum, int32 rows, int32 steps}.
  accumulate  sum += sum_i (v_i > 0.5) - (v_i < 0.5) over column 0 of the first B rows; rows += B; steps += 1
  adjust      if steps >= interval: r = float32(sum) / float32(rows); dir = sign(r - target);
              p = min(max(p + float32(dir) * (float32(rows) * per_row), 0), 1); sum = rows = steps = 0      (each operation rounded to fp32)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import input_oracle as IO  # noqa: E402
from test_abi import ROOT, _protos  # noqa: E402
from test_diffaug_cpu import BITS, IDENTITY, M64, _cpu_trainer, draw_params, key_of, policy_bits  # noqa: E402

EXT_HEADER = os.path.join(ROOT, "include", "littlegan_hip_ext.h")
ENTRY_POINTS = ("lgx_diffaug_draw_gated", "lgx_ada_init", "lgx_ada_accumulate", "lgx_ada_adjust")
GROUPS = ((0, 1, 2), (3, 4), (5, 6, 7))    # the record's columns per gate: color, translation, cutout
P_LO, P_HI = float(np.float32(2.0 ** -24)), float(np.float32(1.0 - 2.0 ** -24))
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
def gate_words(seed, key_offset, call, r0, rows):
    """[rows, 3] of w_j = word_j >> 8 of the rows' gate block: counter words [lo(ctr), hi(ctr), 1, 0]"""
    out = np.empty((rows, 3), np.int64)
    for i in range(rows):
        ctr = (key_offset + (((call << 24) + r0 + i) << 1)) & M64
        blk = IO.philox4x32_10([ctr & IO.MASK, ctr >> 32, 1, 0], [seed & IO.MASK, (seed >> 32) & IO.MASK])
        out[i] = [int(v) >> 8 for v in blk[:3]]
    return out


def gate_threshold(p):
    t = F32(p) * F32(16777216.0)
    assert float(t) == int(t)     # exact: p is fp32 in [0, 1]
    return int(t)


def draw_params_gated(seed, key_offset, call, r0, rows, S, policy, p):
    """The records [rows, 8] float32 as lgx_diffaug_draw_gated writes them under state[0] = p"""
    out = draw_params(seed, key_offset, call, r0, rows, S, policy)
    on = gate_words(seed, key_offset, call, r0, rows) < gate_threshold(p)
    for j, cols in enumerate(GROUPS):
        for c in cols:
            out[~on[:, j], c] = IDENTITY[c]
    return out


def ada_accumulate_np(state, heads, B):
    """state = (p float32, sum, rows, steps); heads [rows >= B, ld]: column 0 of the first B rows is read"""
    p, s, n, k = state
    v = np.asarray(heads, F32)[:B, 0]
    signs = (v > F32(0.5)).astype(np.int32) - (v < F32(0.5)).astype(np.int32)     # NaN: both false
    return F32(p), int(np.int32(s) + signs.sum(dtype=np.int32)), int(np.int32(n) + np.int32(B)), int(k) + 1


def ada_adjust_np(state, interval, target, per_row):
    p, s, n, k = state
    if k < interval:
        return F32(p), int(s), int(n), int(k)
    r = F32(s) / F32(n)
    d = 1 if r > F32(target) else -1 if r < F32(target) else 0
    step = F32(d) * (F32(n) * F32(per_row))
    return min(max(F32(p) + step, F32(0.0)), F32(1.0)), 0, 0, 0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# properties of the restatement
def test_p_one_is_the_plain_draw_and_p_zero_the_identity():
    seed, koff = key_of(2, 0, 9)
    for bits in range(1, 8):
        names = ",".join(n for n, v in BITS.items() if bits & v)
        for call in (0, 1):
            plain = draw_params(seed, koff, call, 0, 16, 16, names)
            assert np.array_equal(_bits(draw_params_gated(seed, koff, call, 0, 16, 16, names, 1.0)), _bits(plain)), names
            assert np.array_equal(_bits(draw_params_gated(seed, koff, call, 0, 16, 16, names, 0.0)), _bits(np.tile(IDENTITY, (16, 1)))), names


def test_the_ends_of_the_threshold_are_restated_without_error():
    assert gate_threshold(0.0) == 0 and gate_threshold(1.0) == 1 << 24
    assert gate_threshold(P_LO) == 1 and gate_threshold(P_HI) == (1 << 24) - 1
    assert gate_threshold(0.25) == 1 << 22 and gate_threshold(0.5) == 1 << 23
    # t = 1 lets through only a word that is 0; t = 2^24 - 1 stops only the word 2^24 - 1
    seed, koff = key_of(3, 1, 7)
    w = gate_words(seed, koff, 0, 0, 64)
    full = draw_params(seed, koff, 0, 0, 64, 16, 7)
    lo, hi = draw_params_gated(seed, koff, 0, 0, 64, 16, 7, P_LO), draw_params_gated(seed, koff, 0, 0, 64, 16, 7, P_HI)
    for j, cols in enumerate(GROUPS):
        for i in range(64):
            assert np.array_equal(lo[i, cols], full[i, cols] if w[i, j] == 0 else IDENTITY[list(cols)])
            assert np.array_equal(hi[i, cols], IDENTITY[list(cols)] if w[i, j] == (1 << 24) - 1 else full[i, cols])


def test_a_row_range_is_the_slice_of_the_whole_and_slots_differ():
    seed, koff = key_of(2, 0, 9)
    whole = draw_params_gated(seed, koff, 0, 0, 6, 16, 7, 0.5)
    assert np.array_equal(_bits(draw_params_gated(seed, koff, 0, 3, 3, 16, 7, 0.5)), _bits(whole[3:]))
    assert np.array_equal(gate_words(seed, koff, 0, 3, 3), gate_words(seed, koff, 0, 0, 6)[3:])
    assert not np.array_equal(gate_words(seed, koff, 1, 0, 6), gate_words(seed, koff, 0, 0, 6))
    assert not np.array_equal(gate_words(*key_of(2, 0, 10), 0, 0, 6), gate_words(seed, koff, 0, 0, 6))


def test_the_three_gates_are_independent_bernoulli_draws():
    """4096 rows at p = 0.5: each gate on in 2048 +- 6 sigma rows (sigma = 32), each pair jointly in 1024 +- 6 sigma (sigma = 27.7), all
    three in 512 +- 6 sigma (sigma = 21.2): three gates, not one gate copied (a copy would put every pair at ~2048)."""
    seed, koff = key_of(3, 1, 7)
    for call in (0, 1):
        on = gate_words(seed, koff, call, 0, 4096) < gate_threshold(0.5)
        single = [int(on[:, j].sum()) for j in range(3)]
        pairs = [int((on[:, a] & on[:, b]).sum()) for a, b in ((0, 1), (0, 2), (1, 2))]
        triple = int(on.all(axis=1).sum())
        print(f"slot {call}: single {single} pairs {pairs} triple {triple}")
        assert all(1856 <= n <= 2240 for n in single), single
        assert all(858 <= n <= 1190 for n in pairs), pairs
        assert 386 <= triple <= 638, triple


def test_gate_words_do_not_touch_the_record_blocks():
    """The record under p = 1 is draw_params's whatever the gate block holds, and the gate block differs from both record blocks"""
    seed, koff = key_of(5, 0, 3)
    ctr = koff
    key = [seed & IO.MASK, (seed >> 32) & IO.MASK]
    blocks = [tuple(int(v) for v in IO.philox4x32_10([c & IO.MASK, c >> 32, z, 0], key)) for c, z in ((ctr, 0), (ctr + 1, 0), (ctr, 1))]
    assert len(set(blocks)) == 3
    assert [v >> 8 for v in blocks[2][:3]] == gate_words(seed, koff, 0, 0, 1)[0].tolist()


def test_controller_restatement():
    st = (F32(0.5), 0, 0, 0)
    st = ada_accumulate_np(st, np.array([[0.7, 9], [0.2, 9], [0.5, 9], [np.nan, 9], [0.9, 9]], F32), 5)
    assert st[1:] == (1, 5, 1)
    assert ada_adjust_np(st, 2, 0.6, 1 / 48) == st                       # not due: nothing changes
    up = ada_adjust_np((F32(0.5), 5, 6, 2), 2, 0.6, float(F32(1 / 48)))
    assert up == (F32(0.5) + F32(6) * F32(1 / 48), 0, 0, 0) and float(up[0]) == 0.625
    assert ada_adjust_np((F32(0.5), -6, 6, 2), 2, 0.6, float(F32(1 / 48)))[0] == F32(0.375)
    assert ada_adjust_np((F32(0.5), 3, 5, 2), 2, F32(0.6), 0.25) == (F32(0.5), 0, 0, 0)      # r == target exactly: p stays, counters reset
    assert ada_adjust_np((F32(0.9), 6, 6, 1), 1, 0.6, 0.25)[0] == F32(1.0) and ada_adjust_np((F32(0.1), -6, 6, 1), 1, 0.6, 0.25)[0] == F32(0.0)


# ---------------------------------------------------------------------------------------------------------------------
# the entry points of the extension header
@pytest.fixture(scope="module")
def lib():
    from littlegan_amd.csrc.build import build
    build(verbose=False)
    from littlegan_amd import _lib
    return _lib


def test_extension_header_declares_the_entry_points(lib):
    assert set(_protos(EXT_HEADER)) == set(ENTRY_POINTS) == {n for n in lib.SIGNATURES if n.startswith("lgx_")}


def test_argument_validation_without_gpu(lib):
    h = lib.load()
    d, d2, d3 = C.c_void_p(64), C.c_void_p(128), C.c_void_p(256)    # never dereferenced: every call below must fail its host-side checks first
    err = lambda: h.lg_last_error()
    g = h.lgx_diffaug_draw_gated                                     # (key, call, r0, rows, S, policy_bits, state, params, stream)
    assert g(None, 0, 0, 4, 16, 7, d2, d3, None) == -1 and b"null pointer" in err()
    assert g(d, 0, 0, 4, 16, 7, None, d3, None) == -1 and b"null pointer" in err()
    assert g(d, 0, 0, 4, 16, 7, d2, None, None) == -1 and b"null pointer" in err()
    assert g(C.c_void_p(68), 0, 0, 4, 16, 7, d2, d3, None) == -1 and b"aligned" in err()        # key 8-byte
    assert g(d, 0, 0, 4, 16, 7, C.c_void_p(136), d3, None) == -1 and b"aligned" in err()         # state 16-byte
    assert g(d, 0, 0, 4, 16, 7, d2, C.c_void_p(264), None) == -1 and b"aligned" in err()         # params 16-byte
    assert g(d, -1, 0, 4, 16, 7, d2, d3, None) == -1 and b"call slot" in err()
    assert g(d, 4, 0, 4, 16, 7, d2, d3, None) == -1 and b"call slot" in err()
    assert g(d, 0, 0, 0, 16, 7, d2, d3, None) == -1 and b"rows" in err()
    assert g(d, 0, -1, 4, 16, 7, d2, d3, None) == -1 and b"rows" in err()
    assert g(d, 0, (1 << 24) - 2, 4, 16, 7, d2, d3, None) == -1 and b"rows" in err()
    assert g(d, 0, 0, 4, 4, 7, d2, d3, None) == -1 and b"image side" in err()
    assert g(d, 0, 0, 4, 20, 7, d2, d3, None) == -1 and b"image side" in err()
    assert g(d, 0, 0, 4, 1032, 7, d2, d3, None) == -1 and b"image side" in err()
    assert g(d, 0, 0, 4, 16, 8, d2, d3, None) == -1 and b"policy bits" in err()
    assert g(d, 0, 0, 4, 16, -1, d2, d3, None) == -1 and b"policy bits" in err()
    assert b"lgx_diffaug_draw_gated" in err()
    init = h.lgx_ada_init                                            # (state, p0, stream)
    assert init(None, 0.5, None) == -1 and b"null pointer" in err()
    assert init(C.c_void_p(72), 0.5, None) == -1 and b"aligned" in err()
    assert init(d, -0.001, None) == -1 and b"p0" in err()
    assert init(d, 1.001, None) == -1 and b"p0" in err()
    assert init(d, float("nan"), None) == -1 and b"p0" in err() and b"lgx_ada_init" in err()
    acc = h.lgx_ada_accumulate                                       # (state, heads, ld, B, stream)
    assert acc(None, d2, 6, 3, None) == -1 and b"null pointer" in err()
    assert acc(d, None, 6, 3, None) == -1 and b"null pointer" in err()
    assert acc(C.c_void_p(72), d2, 6, 3, None) == -1 and b"aligned" in err()                    # state 16-byte
    assert acc(d, C.c_void_p(130), 6, 3, None) == -1 and b"aligned" in err()                    # heads 4-byte
    assert acc(d, d2, 0, 3, None) == -1 and b"leading dimension" in err()
    assert acc(d, d2, 6, 0, None) == -1 and b"row count" in err()
    assert acc(d, d2, 6, (1 << 20) + 1, None) == -1 and b"row count" in err() and b"lgx_ada_accumulate" in err()
    adj = h.lgx_ada_adjust                                           # (state, interval, target, per_row, stream)
    assert adj(None, 4, 0.6, 1e-3, None) == -1 and b"null pointer" in err()
    assert adj(C.c_void_p(72), 4, 0.6, 1e-3, None) == -1 and b"aligned" in err()
    assert adj(d, 0, 0.6, 1e-3, None) == -1 and b"interval" in err()
    assert adj(d, 4, 0.0, 1e-3, None) == -1 and b"target" in err()
    assert adj(d, 4, 1.0, 1e-3, None) == -1 and b"target" in err()
    assert adj(d, 4, float("nan"), 1e-3, None) == -1 and b"target" in err()
    assert adj(d, 4, 0.6, 0.0, None) == -1 and b"per_row" in err()
    assert adj(d, 4, 0.6, -1e-3, None) == -1 and b"per_row" in err()
    assert adj(d, 4, 0.6, float("inf"), None) == -1 and b"per_row" in err()
    assert adj(d, 4, 0.6, float("nan"), None) == -1 and b"per_row" in err() and b"lgx_ada_adjust" in err()


# ---------------------------------------------------------------------------------------------------------------------
# configuration and trainer
def test_config_keys_default_to_off(tmp_path):
    from littlegan_amd import config
    d = config.DEFAULTS
    assert d["diff_augment_p"] is None and d["ada_target"] is None and d["ada_interval"] == 4 and d["ada_kimg"] == 500
    for k in ("diff_augment_p", "ada_target", "ada_interval", "ada_kimg"):
        assert k in config.__doc__, k
    a = config.Arg(["train", "x"], config_dir=str(tmp_path))
    assert a.diff_augment_p is None and a.ada_target is None and a.ada_interval == 4 and a.ada_kimg == 500
    (tmp_path / "ada.config.json").write_text('{"diff_augment": "color,cutout", "diff_augment_p": 0.25, "ada_target": 0.6, "ada_kimg": 100}')
    a = config.Arg(["train", "x", "-e", "ada"], config_dir=str(tmp_path))
    assert (a.diff_augment_p, a.ada_target, a.ada_interval, a.ada_kimg) == (0.25, 0.6, 4, 100)
    # which path runs
    assert config.ada_settings("color") is None and config.ada_settings("color", 1.0) is None and config.ada_settings("") is None
    assert config.ada_settings("color", 0.5) == {"p0": 0.5, "target": None, "interval": 4, "per_row": float(F32(1 / 500000.0))}
    s = config.ada_settings("color", None, 0.6, 2, 0.048)
    assert s == {"p0": 0.0, "target": float(F32(0.6)), "interval": 2, "per_row": float(F32(1 / 48))}
    assert config.ada_settings("color", 1.0, 0.6)["p0"] == 1.0


BAD = [("diff_augment_p", -0.1), ("diff_augment_p", 1.5), ("diff_augment_p", "0.5"), ("diff_augment_p", float("nan")),
       ("ada_target", 0.0), ("ada_target", 1.0), ("ada_target", -0.6), ("ada_target", "0.6"),
       ("ada_interval", 0), ("ada_interval", -1), ("ada_interval", 2.5),
       ("ada_kimg", 0), ("ada_kimg", -500), ("ada_kimg", float("inf")), ("ada_kimg", 1e60)]


@pytest.mark.parametrize("key,value", BAD, ids=lambda v: str(v))
def test_an_out_of_range_value_raises(tmp_path, key, value):
    """... whether or not the key it belongs to is in use: a bad ada_interval is refused with ada_target null too"""
    import json
    from littlegan_amd import config
    bad = {key: value}
    with pytest.raises(ValueError, match=key):
        config.ada_settings("color,translation", **bad)
    with pytest.raises(ValueError, match=key):
        config.ada_settings("color,translation", **dict(dict(ada_target=0.6, diff_augment_p=0.5), **bad))
    (tmp_path / "bad.config.json").write_text(json.dumps(dict(bad, diff_augment="color")))
    with pytest.raises(ValueError, match=key):
        config.Arg(["train", "x", "-e", "bad"], config_dir=str(tmp_path))
    with pytest.raises(ValueError, match=key):
        _cpu_trainer(diff_augment="color", **bad)


def test_gating_without_diff_augment_raises(tmp_path):
    from littlegan_amd import config
    for kw in (dict(ada_target=0.6), dict(diff_augment_p=0.5), dict(diff_augment_p=1.0)):
        with pytest.raises(ValueError, match="need diff_augment"):
            config.ada_settings("", **kw)
        with pytest.raises(ValueError, match="need diff_augment"):
            _cpu_trainer(**kw)
        with pytest.raises(ValueError, match="need diff_augment"):
            _cpu_trainer(diff_augment="", **kw)
    (tmp_path / "t.config.json").write_text('{"ada_target": 0.6}')
    with pytest.raises(ValueError, match="need diff_augment"):
        config.Arg(["train", "x", "-e", "t"], config_dir=str(tmp_path))
    # the refused combinations of diff_augment apply unchanged
    with pytest.raises(ValueError, match="diff_augment and use_gp"):
        _cpu_trainer(diff_augment="color", ada_target=0.6, use_gp=True)
    with pytest.raises(ValueError, match="diff_augment and dropout_train"):
        _cpu_trainer(diff_augment="color", diff_augment_p=0.5, dropout_train=True)


def test_defaults_add_no_state():
    for kw in (dict(), dict(diff_augment="color,cutout"), dict(diff_augment="color", diff_augment_p=1.0),
               dict(diff_augment="color", ada_interval=7, ada_kimg=3)):
        tr, _ = _cpu_trainer(**kw)
        assert tr.ada is None and not hasattr(tr, "ada_state") and tr.ada_p() is None
        assert "ada_state" not in tr.checkpoint_state()
