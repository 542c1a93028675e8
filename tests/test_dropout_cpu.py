"""Live encoder dropout (dropout_train) without a GPU: the C ABI of the dropped norm passes (declared, exported,
bound, validating before any launch), a vectorised numpy restatement of the mask definition pinned against the oracle's
Philox4x32-10, its keep fraction against the binomial, and the configuration / trainer behaviour.

The definition (include/littlegan_hip.h): element e (flat NHWC index) of sample row r (absolute row of the encoder call's batch,
L elements per sample):
  T = round(rate * 65536), keep = (w >= T), scale = 65536 / (65536 - T) (fp32),
  offset = key_offset + (call << 34) + ((level-1) << 32) + r*(L/8) + e/8,
  P = philox4x32_10(ctr = (lo32(offset), hi32(offset), 0, 0), key = (lo32(seed), hi32(seed))),
  w = (P[(e%8) >> 1] >> (16*(e&1))) & 0xFFFF,
  seed = (args.seed << 20) ^ rank, key_offset = (input_step << 40) + (1 << 36).
`keep_mask` / `drop_mult` below are also the oracle of tests/test_dropout_gpu.py."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import input_oracle as IO  # noqa: E402
from oracle import np_oracle as O  # noqa: E402
from test_abi import _ctype, _protos  # noqa: E402

DROP_ENTRY_POINTS = ("lg_dropout_key", "lg_dropout_mask", "lg_instnorm_leaky_apply_drop", "lg_instnorm_leaky_apply_z16_drop",
                     "lg_instnorm_leaky_apply_z16_p_drop", "lg_instnorm_leaky_bwd_drop", "lg_instnorm_leaky_bwd_z16_drop")
M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
def philox_np(offsets, seed):
    """Philox4x32-10 of the blocks at the 64-bit counters `offsets` (uint64 array) under `seed` -> uint32 [n, 4]"""
    offsets = np.asarray(offsets, np.uint64)
    c = [offsets & np.uint64(IO.MASK), offsets >> np.uint64(32), np.zeros_like(offsets), np.zeros_like(offsets)]
    k0, k1 = int(seed) & IO.MASK, (int(seed) >> 32) & IO.MASK
    m32 = np.uint64(IO.MASK)
    for _ in range(10):
        p0, p1 = np.uint64(IO.M0) * c[0], np.uint64(IO.M1) * c[2]     # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + IO.W0) & IO.MASK, (k1 + IO.W1) & IO.MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def key_of(seed_arg, rank, input_step):
    """(seed, key_offset) as EagerTrainer.draw_dropout_key writes them"""
    return (int(seed_arg) << 20) ^ int(rank), (int(input_step) << 40) + (1 << 36)


def threshold(rate):
    """T as the library rounds it: the rate crosses the C ABI as a float"""
    return int(round(float(np.float32(rate)) * 65536.0))


def mask_words(seed, key_offset, call, level, r0, B, L):
    """w [B, L] (uint32 holding 16-bit values) of rows r0 .. r0+B-1 of the (call, level) slot"""
    assert L % 8 == 0
    base = (key_offset + (call << 34) + ((level - 1) << 32) + r0 * (L // 8)) & M64
    P = philox_np(np.uint64(base) + np.arange(B * (L // 8), dtype=np.uint64), seed)       # [B*L/8, 4]
    w = np.stack([P & np.uint32(0xFFFF), P >> np.uint32(16)], axis=-1)                    # [.., word, half]: e%8 = 2*word + half
    return w.reshape(B, L)


def keep_mask(seed, key_offset, call, level, r0, B, L, rate):
    return mask_words(seed, key_offset, call, level, r0, B, L) >= np.uint32(threshold(rate))


def drop_mult(seed, key_offset, call, level, r0, B, L, rate):
    """keep * scale as float32 [B, L]"""
    T = threshold(rate)
    scale = np.float32(65536.0) / np.float32(65536 - T)
    return np.where(keep_mask(seed, key_offset, call, level, r0, B, L, rate), scale, np.float32(0.0)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from littlegan_amd.csrc.build import build
    build(verbose=False)
    from littlegan_amd import _lib
    return _lib


def test_header_declares_exports_and_binds_the_dropout_entry_points(lib):
    protos = _protos()
    h = lib.load()
    for name in DROP_ENTRY_POINTS:
        assert name in protos, f"{name} not declared in include/littlegan_hip.h"
        assert hasattr(h, name), f"{name} not exported"
        res, args = lib.SIGNATURES[name]
        ret, plist = protos[name]
        assert len(args) == len(plist), name
        for a, decl in zip(args, plist):
            assert a is _ctype(decl), (name, decl)
        assert res is C.c_int and ret == "int"
    assert h.lg_abi_version() == 1


def test_dropout_argument_validation_without_gpu(lib):
    h = lib.load()
    d = C.c_void_p(16)   # never dereferenced: every call below must fail its host-side checks first
    err = lambda: h.lg_last_error()
    # lg_dropout_mask(key, call, level, r0, B, L, rate, keep, stream)
    assert h.lg_dropout_mask(None, 0, 1, 0, 2, 64, 0.5, d, None) == -1 and b"null pointer" in err()
    assert h.lg_dropout_mask(d, 0, 1, 0, 2, 64, 0.5, None, None) == -1 and b"null pointer" in err()
    assert h.lg_dropout_mask(d, 0, 1, 0, 2, 60, 0.5, d, None) == -1 and b"L % 8" in err()
    assert h.lg_dropout_mask(d, 0, 1, 0, 2, 64, 1.0, d, None) == -1 and b"outside [0, 1)" in err()
    assert h.lg_dropout_mask(d, 0, 1, 0, 2, 64, -0.1, d, None) == -1 and b"outside [0, 1)" in err()
    assert h.lg_dropout_mask(d, 0, 1, 0, 2, 64, float("nan"), d, None) == -1 and b"outside [0, 1)" in err()
    assert h.lg_dropout_mask(d, 0, 1, 0, 2, 64, 0.999999, d, None) == -1 and b"rounds to 1" in err()
    assert h.lg_dropout_mask(d, 4, 1, 0, 2, 64, 0.5, d, None) == -1 and b"call slot" in err()
    assert h.lg_dropout_mask(d, -1, 1, 0, 2, 64, 0.5, d, None) == -1 and b"call slot" in err()
    assert h.lg_dropout_mask(d, 0, 0, 0, 2, 64, 0.5, d, None) == -1 and b"level" in err()
    assert h.lg_dropout_mask(d, 0, 5, 0, 2, 64, 0.5, d, None) == -1 and b"level" in err()
    assert h.lg_dropout_mask(d, 0, 1, -1, 2, 64, 0.5, d, None) == -1 and b"first row" in err()
    assert h.lg_dropout_mask(d, 0, 1, 0, 0, 64, 0.5, d, None) == -1 and b"bad shape" in err()
    assert h.lg_dropout_mask(d, 0, 1, 0, 2, 64, 0.5, C.c_void_p(20), None) == -1 and b"8-byte aligned" in err()
    # the rows of a launch must END inside the level's window of 2^32 blocks: (r0 + B) * (L/8) <= 2^32
    assert h.lg_instnorm_leaky_apply_drop(d, d, d, None, 3, 8 << 12, 0.3, d, 0, 1, (1 << 20) - 2, 0.5, None) == -1 and b"counter window" in err()
    assert h.lg_dropout_key(None, 1, 2, None) == -1 and h.lg_dropout_key(C.c_void_p(12), 1, 2, None) == -1
    # forward twins: (x, stats, y, y16, B, L, alpha, key, call, level, r0, rate, stream)
    for fn in (h.lg_instnorm_leaky_apply_drop, h.lg_instnorm_leaky_apply_z16_drop):
        assert fn(d, d, d, None, 2, 64, 0.3, None, 0, 1, 0, 0.5, None) == -1 and b"null pointer" in err()
        assert fn(None, d, d, None, 2, 64, 0.3, d, 0, 1, 0, 0.5, None) == -1 and b"null pointer" in err()
        assert fn(d, d, None, None, 2, 64, 0.3, d, 0, 1, 0, 0.5, None) == -1 and b"null pointer" in err()
        assert fn(d, d, d, None, 2, 68, 0.3, d, 0, 1, 0, 0.5, None) == -1 and b"L % 8" in err()
        assert fn(d, d, d, None, 2, 64, 0.3, d, 0, 1, 0, 1.5, None) == -1 and b"outside [0, 1)" in err()
        assert fn(d, d, d, None, 2, 64, 0.3, d, 7, 1, 0, 0.5, None) == -1 and b"call slot" in err()
        assert fn(d, d, d, None, 2, 64, 0.3, d, 0, 9, 0, 0.5, None) == -1 and b"level" in err()
    # (z16, partials, nparts, gamma, beta, stats, y, y16, B, L, alpha, key, call, level, r0, rate, stream)
    fp = h.lg_instnorm_leaky_apply_z16_p_drop
    assert fp(d, d, 4, d, d, d, d, None, 2, 64, 0.3, None, 0, 1, 0, 0.5, None) == -1 and b"null pointer" in err()
    assert fp(d, None, 4, d, d, d, d, None, 2, 64, 0.3, d, 0, 1, 0, 0.5, None) == -1 and b"null pointer" in err()
    assert fp(d, d, 4, d, d, d, d, None, 2, 64, 0.3, d, 0, 1, 0, 2.0, None) == -1 and b"outside [0, 1)" in err()
    assert fp(d, d, 4, d, d, d, d, None, 2, 64, 0.3, d, 0, 0, 0, 0.5, None) == -1 and b"level" in err()
    # backward twins
    ws = h.lg_instnorm_bwd_db_workspace_bytes(2, 64, 0)
    # (x, stats, g, g16, dx, dx16, dgamma, dbeta, db, C, ws, ws_bytes, B, L, alpha, accumulate, key, call, level, r0, rate, stream)
    fb = h.lg_instnorm_leaky_bwd_drop
    assert fb(d, d, d, 0, d, None, None, None, None, 0, d, ws, 2, 64, 0.3, 0, None, 0, 1, 0, 0.5, None) == -1 and b"null pointer" in err()
    assert fb(d, d, None, 0, d, None, None, None, None, 0, d, ws, 2, 64, 0.3, 0, d, 0, 1, 0, 0.5, None) == -1 and b"null pointer" in err()
    assert fb(d, d, d, 0, d, None, None, None, None, 0, d, ws, 2, 60, 0.3, 0, d, 0, 1, 0, 0.5, None) == -1 and b"L % 8" in err()
    assert fb(d, d, d, 0, d, None, None, None, None, 0, d, ws, 2, 64, 0.3, 0, d, 0, 1, 0, 1.0, None) == -1 and b"outside [0, 1)" in err()
    assert fb(d, d, d, 0, d, None, None, None, None, 0, d, ws, 2, 64, 0.3, 0, d, 4, 1, 0, 0.5, None) == -1 and b"call slot" in err()
    assert fb(d, d, d, 0, d, None, None, None, None, 0, d, ws - 1, 2, 64, 0.3, 0, d, 0, 1, 0, 0.5, None) == -1 and b"workspace too small" in err()
    # (z16, stats, g, g16, dx, dx16, dgamma, dbeta, db, C, partials, nparts_in, ws, ws_bytes, B, L, alpha, accumulate, key, ...)
    fz = h.lg_instnorm_leaky_bwd_z16_drop
    assert fz(d, d, d, 1, None, d, None, None, None, 0, None, 0, d, ws, 2, 64, 0.3, 0, None, 0, 1, 0, 0.5, None) == -1 and b"null pointer" in err()
    assert fz(d, d, d, 1, None, d, None, None, None, 0, None, 0, d, ws, 2, 64, 0.3, 0, d, 0, 5, 0, 0.5, None) == -1 and b"level" in err()
    # producer-fused sums know no mask: refused unless the mask keeps everything
    assert fz(d, d, d, 1, None, d, None, None, None, 0, d, 4, d, ws, 2, 64, 0.3, 0, d, 0, 1, 0, 0.5, None) == -1 and b"no dropout mask" in err()


# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_matches_the_oracle_philox_and_the_word_order():
    seed, koff = key_of(3, 1, 7)
    assert (seed, koff) == ((3 << 20) ^ 1, (7 << 40) + (1 << 36))
    call, level, r0, B, L = 2, 3, 5, 2, 24
    w = mask_words(seed, koff, call, level, r0, B, L)
    for r, e in ((0, 0), (0, 1), (0, 7), (0, 8), (1, 13), (1, 23)):
        off = koff + (call << 34) + ((level - 1) << 32) + (r0 + r) * (L // 8) + e // 8
        P = IO.philox4x32_10([off & IO.MASK, off >> 32, 0, 0], [seed & IO.MASK, seed >> 32])
        assert int(w[r, e]) == (P[(e % 8) >> 1] >> (16 * (e & 1))) & 0xFFFF, (r, e)
    # a batch slice regenerates exactly the rows of the whole batch
    whole = mask_words(seed, koff, 0, 1, 0, 6, 64)
    assert np.array_equal(mask_words(seed, koff, 0, 1, 3, 3, 64), whole[3:])
    # known answer (Random123 kat_vectors: ctr = 0, key = 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8): elements 0..7 of the block
    # at offset 0 take the halves of the words in order x.lo x.hi y.lo y.hi z.lo z.hi w.lo w.hi
    assert IO.philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert philox_np(np.zeros(1, np.uint64), 0)[0].tolist() == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    w0 = mask_words(0, 0, 0, 1, 0, 1, 8)[0].tolist()
    assert w0 == [0xE8D5, 0x6627, 0xC58D, 0xE169, 0xAC4C, 0xBC57, 0xDBD8, 0x9B00]
    assert keep_mask(0, 0, 0, 1, 0, 1, 8, 0.5)[0].tolist() == [True, False, True, True, True, True, True, True]
    # thresholds and scales
    assert threshold(0.5) == 32768 and threshold(0.25) == 16384 and threshold(0.0) == 0 and threshold(0.3) == 19661
    m = drop_mult(0, 0, 0, 1, 0, 1, 8, 0.5)
    assert m.dtype == np.float32 and set(m.ravel().tolist()) == {0.0, 2.0}
    assert np.all(drop_mult(5, 1 << 36, 1, 2, 0, 2, 16, 0.0) == 1.0)


@pytest.mark.parametrize("rate", [0.5, 0.25])
@pytest.mark.parametrize("slot", [(1, 0, 1), (1, 2, 4), (7, 1, 2)], ids=["s1c0l1", "s1c2l4", "s7c1l2"])
def test_keep_fraction_is_binomial(rate, slot):
    """2^17 blocks = 2^20 elements, seed 0: overall and per 16-bit lane within 5 standard deviations of the binomial"""
    step, call, level = slot
    seed, koff = key_of(0, 0, step)
    nblk = 1 << 17
    keep = keep_mask(seed, koff, call, level, 0, 1, 8 * nblk, rate).reshape(nblk, 8)
    p = 1.0 - threshold(rate) / 65536.0
    n = keep.size
    z = (keep.sum() - n * p) / np.sqrt(n * p * (1 - p))
    print(f"rate {rate} slot {slot}: overall {z:+.2f} sigma")
    assert abs(z) < 5.0
    for lane in range(8):
        zl = (keep[:, lane].sum() - nblk * p) / np.sqrt(nblk * p * (1 - p))
        print(f"  lane {lane}: {zl:+.2f} sigma")
        assert abs(zl) < 5.0, lane


def test_masks_of_different_slots_differ():
    seed, koff = key_of(0, 0, 1)
    ref = keep_mask(seed, koff, 0, 1, 0, 2, 4096, 0.5)
    others = {"call": keep_mask(seed, koff, 1, 1, 0, 2, 4096, 0.5), "level": keep_mask(seed, koff, 0, 2, 0, 2, 4096, 0.5),
              "step": keep_mask(*key_of(0, 0, 2), 0, 1, 0, 2, 4096, 0.5), "rank": keep_mask(*key_of(0, 1, 1), 0, 1, 0, 2, 4096, 0.5),
              "rows": keep_mask(seed, koff, 0, 1, 2, 2, 4096, 0.5)}
    for what, m in others.items():
        agree = (m == ref).mean()
        assert 0.45 < agree < 0.55, (what, agree)   # independent fair coins agree on half of 8192 elements (sigma = 0.0055)


# ---------------------------------------------------------------------------------------------------------------------
def _cpu_trainer(**kw):
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    from test_step_gpu import make_args
    cfg = O.Cfg(init_dim=2, conv_filter=(16, 8, 8, 8, 8), cond_dim=3, noise_dim=5, batch_size=2)
    args = make_args(cfg)
    args.device = "cpu"     # construction only: no kernel runs in this file
    for k, v in kw.items():
        setattr(args, k, v)
    dec, enc = Decoder(args), Encoder(args)
    g = Generator(args, dec)
    d = Discriminator(args, enc)
    return EagerTrainer(args, g, d, Adjuster(args, d, g), None), cfg


def test_config_key_defaults_to_off():
    from littlegan_amd import config
    assert config.DEFAULTS["dropout_train"] is False and config.DEFAULTS["dropout_rate"] == 0.5
    assert "dropout_train" in config.__doc__
    tr, _ = _cpu_trainer()
    assert tr.dropout is False
    tr, _ = _cpu_trainer(dropout_train=True)
    assert tr.dropout is True and tr.dropout_rate == 0.5


def test_trainer_refuses_gp_with_dropout_and_bad_rates():
    with pytest.raises(ValueError, match="use_gp and dropout_train"):
        _cpu_trainer(dropout_train=True, use_gp=True)
    _cpu_trainer(dropout_train=False, use_gp=True)    # the key alone changes nothing
    for rate in (1.0, -0.25, 1.5):
        with pytest.raises(ValueError, match="dropout_rate"):
            _cpu_trainer(dropout_train=True, dropout_rate=rate)


def test_missing_dropout_key_raises():
    tr, cfg = _cpu_trainer(dropout_train=True)
    inp = {k: torch.zeros(2, 3) for k in ("real_image_1", "real_cond_1", "real_image_2", "real_cond_2", "noise", "new_image")}
    with pytest.raises(ValueError, match="dropout_key"):
        tr.train_step_from_inputs(1, inp)


def test_draw_dropout_key_follows_the_input_step():
    tr, _ = _cpu_trainer(dropout_train=True, seed=3)
    tr.rank, tr._input_step = 1, 7
    assert tr.dropout_key_words() == key_of(3, 1, 7)
    import inspect as _i
    assert "torch.tensor" not in _i.getsource(type(tr).draw_dropout_key)   # written on the device: no blocking host-to-device copy


def test_predict_and_sampling_never_construct_a_drop_context(monkeypatch):
    """predict (the test / random-sample / evaluate-sample modes) calls the three models without a drop context, and the sampling
    entry points (Generator, Discriminator.__call__) cannot even take one"""
    from littlegan_amd import model, ops
    tr, cfg = _cpu_trainer(dropout_train=True)
    made = []
    real_init = ops.Drop.__init__
    monkeypatch.setattr(ops.Drop, "__init__", lambda self, *a, **k: (made.append(a), real_init(self, *a, **k))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    B, H = 2, 32
    calls = []

    def stub(name, out):
        def f(inputs):          # any keyword (drop=...) is a TypeError
            calls.append(name)
            return out
        return f

    img = torch.zeros(B, H, H, 3)
    tr.generator = stub("G", img)
    tr.discriminator = stub("D", (torch.full((B, 1), 0.5), torch.full((B, cfg.cond_dim), 0.5)))
    tr.adjuster = stub("A", img)
    tr.predict(torch.zeros(B, cfg.noise_dim), torch.zeros(B, cfg.cond_dim), img)
    assert calls == ["G", "D", "D", "A", "A"] and not made
    assert "drop" not in inspect.signature(model.Generator.__call__).parameters
    assert "drop" not in inspect.signature(model.Discriminator.__call__).parameters
    assert "drop" not in inspect.signature(model.Decoder.__call__).parameters
    for fn in (model.Encoder.__call__, model.Discriminator.forward_packed, model.Adjuster.__call__):
        assert inspect.signature(fn).parameters["drop"].default is None
    src = inspect.getsource(type(tr)._init_test_data) + inspect.getsource(type(tr).predict)
    assert "drop" not in src
