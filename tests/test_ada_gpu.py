"""Adaptive augmentation probability (ADA) on the GPU.

Kernels: lgx_diffaug_draw_gated against the restatement of tests/test_ada_cpu.py bit for bit (every policy subset, both call slots, row
ranges, p at both ends of the threshold); lgx_ada_accumulate (integers: exact) below, around and above a wave and the workgroup;
lgx_ada_adjust bit for bit from hand-built states.  Whole steps at the geometry and with the references of tests/test_diffaug_gpu.py: a
fixed p = 0.5 against the float64 oracles under the gated records at that module's tolerances; the controller's trajectory eager against
graph replay and against the restated controller fed with the float64 oracle's signs, in both directions and into both clamps; a fixed p
leaves the counters alone; checkpoint resume; p = 1 without a target is the plain diff_augment step bit for bit; the data-parallel
all-reduce of the counters at world size 1.  (The memory contract of the four entry points: the ada-* rows of
tests/test_memory_contract_gpu.py, on this module's data.)"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # the spawned child imports this module by name too
from oracle import np_oracle as O  # noqa: E402
from oracle import torch_oracle as TO  # noqa: E402
from test_ada_cpu import (F32, P_HI, P_LO, ada_accumulate_np, ada_adjust_np, draw_params_gated)  # noqa: E402
from test_diffaug_cpu import BITS, IDENTITY, draw_params, key_of  # noqa: E402
from test_diffaug_gpu import FULL, SMALL, AugNet, _same_state, aug_np_oracle, build_aug, dev_key, step_reference  # noqa: E402
from test_dp_gpu import CFG as DP_CFG, _free_port, _inputs, _join_all  # noqa: E402
from test_step_gpu import TOLS, check_emu, check_grads, dev_inputs, f32_round, load_weights, make_args, perturbed  # noqa: E402

pytestmark = pytest.mark.gpu

PS = (0.0, P_LO, 0.25, 0.5, P_HI, 1.0)
HALF = F32(0.5)
SPECIAL = np.array([0.5, np.nextafter(HALF, F32(1)), np.nextafter(HALF, F32(0)), 0.0, 1.0, np.nan], np.float32)


@pytest.fixture(scope="module")
def ops():
    from littlegan_amd import ops as _ops
    return _ops


def words(p, s=0, n=0, k=0):
    """the state {p, sum, rows, steps} as its four 32-bit words (int32, host)"""
    a = np.zeros(4, np.int32)
    a.view(np.float32)[0] = p
    a[1:] = (s, n, k)
    return a


def dev_state(p, s=0, n=0, k=0):
    return torch.from_numpy(words(p, s, n, k)).cuda().view(torch.float32)


def same_read(got, want):
    """ada_read's tuple against a restated state: p bit for bit, the counters as integers"""
    return F32(got[0]).view(np.uint32) == F32(want[0]).view(np.uint32) and tuple(got[1:]) == tuple(int(v) for v in want[1:])


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------- the gated draw
@pytest.mark.parametrize("S", [8, 16, 128])
def test_gated_draws_equal_the_restatement_bit_for_bit(ops, S):
    key = dev_key(3, 1, 7)
    seed, koff = key.tolist()
    ident = np.tile(IDENTITY, (6, 1))
    for p in PS:
        state = ops.ada_init(p)
        for call in (0, 1):
            for bits in range(1, 8):
                names = ",".join(n for n, v in BITS.items() if bits & v)
                whole = ops.diffaug_draw_gated(key, call, 0, 6, S, names, state).cpu().numpy()
                want = draw_params_gated(seed, koff, call, 0, 6, S, names, p)
                assert np.array_equal(u32(whole), u32(want)), (p, call, names, whole, want)
                part = ops.diffaug_draw_gated(key, call, 3, 3, S, bits, state).cpu().numpy()
                assert np.array_equal(u32(part), u32(whole[3:])), (p, call, names)
                if p == 1.0:
                    assert torch.equal(ops.diffaug_draw_gated(key, call, 0, 6, S, bits, state), ops.diffaug_draw(key, call, 0, 6, S, bits))
                if p == 0.0:
                    assert np.array_equal(u32(whole), u32(ident)), (call, names)
            deep = ops.diffaug_draw_gated(key, call, 509, 3, S, FULL, state).cpu().numpy()   # a row range deep inside a launch-shape batch
            assert np.array_equal(u32(deep), u32(draw_params_gated(seed, koff, call, 509, 3, S, FULL, p))), (p, call)
        assert np.array_equal(ops.diffaug_draw_gated(key, 0, 0, 6, S, "", state).cpu().numpy(), ident)
        assert same_read(ops.ada_read(state), (p, 0, 0, 0))    # the draw reads the state and leaves it alone
    # a state no writer produces (only a foreign buffer could hold it): the draw clamps p, NaN reads as 0
    for raw, p in ((float("nan"), 0.0), (-0.5, 0.0), (2.0, 1.0), (float("inf"), 1.0)):
        got = ops.diffaug_draw_gated(key, 1, 0, 6, S, FULL, dev_state(raw)).cpu().numpy()
        assert np.array_equal(u32(got), u32(draw_params_gated(seed, koff, 1, 0, 6, S, FULL, p))), raw
    # the gate is live at p = 0.5: over 6 rows and 2 slots something is gated off and something is applied
    got = np.concatenate([draw_params_gated(seed, koff, c, 0, 6, S, FULL, 0.5) for c in (0, 1)])
    full = np.concatenate([draw_params(seed, koff, c, 0, 6, S, FULL) for c in (0, 1)])
    assert (got[:, 7] == 0).any() and (got[:, 7] != 0).any() and not np.array_equal(got, full)


def test_wrappers_refuse_wrong_arguments(ops):
    key = dev_key()
    st = ops.ada_init(0.5)
    for bad in (torch.zeros(4, device="cuda", dtype=torch.float64), torch.zeros(3, device="cuda"), torch.zeros(4)):
        with pytest.raises(ValueError, match="state"):
            ops.diffaug_draw_gated(key, 0, 0, 2, 16, FULL, bad)
        with pytest.raises(ValueError, match="state"):
            ops.ada_adjust(bad, 2, 0.6, 0.1)
    with pytest.raises(ValueError, match="heads"):
        ops.ada_accumulate(st, torch.zeros(3, 6, device="cuda"), 4)
    with pytest.raises(ValueError, match="diff_augment"):
        ops.diffaug_draw_gated(key, 0, 0, 2, 16, "colour", st)
    from littlegan_amd._lib import LittleGanHipError
    with pytest.raises(LittleGanHipError, match="p0"):
        ops.ada_init(1.5)
    with pytest.raises(LittleGanHipError, match="target"):
        ops.ada_adjust(st, 2, 1.0, 0.1)
    assert same_read(ops.ada_read(st), (0.5, 0, 0, 0))


# ---------------------------------------------------------------------------------------------------------------------- the controller
def heads_mix(B, ld, seed):
    """[B, ld] fp32: column 0 a seeded mix of values around 0.5 with the special ones (exactly 0.5, its two neighbours, 0, 1, NaN) at
    seeded places; the other columns hold the mirrored value 1 - v and NaN: read by mistake, they change the sum."""
    rng = np.random.default_rng(seed)
    h = np.empty((B, ld), np.float32)
    v = rng.uniform(0.0, 1.0, B).astype(np.float32)
    v[:] = np.where(rng.uniform(size=B) < 0.3, F32(0.75), v)     # a majority one way: the sum is not near 0
    spec = np.roll(SPECIAL, seed)[:min(B, len(SPECIAL))]
    v[rng.permutation(B)[:len(spec)]] = spec
    h[:, 0] = v
    for c in range(1, ld):
        h[:, c] = np.nan if c % 2 else 1.0 - np.nan_to_num(v, nan=0.25)
    return h


@pytest.mark.parametrize("ld", [1, 6, 8])
def test_accumulate_is_exact(ops, ld):
    for B in (1, 3, 63, 64, 65, 256, 257, 512, 1000):   # below a wave, around a wave, around the workgroup, above it
        state = dev_state(0.375, -2, 5, 1)
        want = (F32(0.375), -2, 5, 1)
        for call in range(3):
            h = heads_mix(B, ld, 10 * B + call)
            if B >= len(SPECIAL):
                assert np.isnan(h[:, 0]).sum() == 1 and (h[:, 0] == HALF).sum() == 1 and (h[:, 0] == 0).sum() == 1
            ops.ada_accumulate(state, torch.from_numpy(h).cuda(), B)
            want = ada_accumulate_np(want, h, B)
            got = ops.ada_read(state)
            assert same_read(got, want), (B, ld, call, got, want)
        assert want[2] == 5 + 3 * B and want[3] == 4
    # the first B rows of a taller matrix: D's packed output [2B, 1 + c] with the fake rows below
    h = heads_mix(130, ld, 7)
    state = dev_state(1.0)
    ops.ada_accumulate(state, torch.from_numpy(h).cuda(), 65)
    assert same_read(ops.ada_read(state), ada_accumulate_np((F32(1.0), 0, 0, 0), h, 65))


PER_ROW = float(F32(1 / 48))
ADJUST_CASES = [  # (p, sum, rows, steps), interval, target, per_row
    ((0.5, 4, 6, 1), 2, 0.6, PER_ROW),                    # steps < interval: all 16 bytes unchanged
    ((0.5, 4, 6, 3), 4, 0.6, PER_ROW),
    ((0.5, 4, 6, 2), 2, 0.6, PER_ROW),                    # r = 2/3 > target
    ((0.5, 3, 6, 2), 2, 0.6, PER_ROW),                    # r = 1/2 < target
    ((0.5, -6, 6, 5), 2, 0.6, PER_ROW),                   # steps > interval
    ((0.5, 3, 5, 2), 2, float(F32(0.6)), PER_ROW),        # r == target exactly: p unchanged, counters reset
    ((0.0625, -6, 6, 2), 2, 0.6, PER_ROW),                # clamps at 0
    ((0.0, -6, 6, 2), 2, 0.6, PER_ROW),
    ((0.9375, 6, 6, 2), 2, 0.6, PER_ROW),                 # clamps at 1
    ((1.0, 6, 6, 2), 2, 0.6, PER_ROW),
    ((0.3, 1, 1, 1), 1, 0.6, float(F32(1e-3))),           # interval = 1
    ((0.3, 0, 1, 1), 1, 0.5, float(F32(1e-3))),
    ((float(F32(0.7)), 123457, 1 << 20, 4), 4, 0.1, float(F32(1 / 500000.0))),   # launch-size counters, the default rate
    ((float(P_HI), 1000, 1024, 4), 4, 0.6, float(F32(1 / 500000.0))),
]


def test_adjust_equals_the_restatement_bit_for_bit(ops):
    for st, interval, target, per_row in ADJUST_CASES:
        state = dev_state(*st)
        before = state.clone()
        ops.ada_adjust(state, interval, target, per_row)
        want = ada_adjust_np((F32(st[0]),) + st[1:], interval, target, per_row)
        got = ops.ada_read(state)
        assert same_read(got, want), (st, interval, target, got, want)
        if st[3] < interval:
            assert torch.equal(state.view(torch.int32), before.view(torch.int32))
        else:
            assert got[1:] == (0, 0, 0) and 0.0 <= got[0] <= 1.0
    r = ops.ada_read(dev_state(0.5, 3, 5, 2))
    assert r == (0.5, 3, 5, 2)
    state = dev_state(0.5, 3, 5, 2)
    ops.ada_adjust(state, 2, float(F32(0.6)), PER_ROW)
    assert ops.ada_read(state) == (0.5, 0, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------- whole steps
def gated_step_records(seed, koff, B, S, p, policy=FULL):
    """The gated records of D's three calls in the order the oracles make them: D(new_image), D(fake), D(adj_image)"""
    slot0 = draw_params_gated(seed, koff, 0, 0, 2 * B, S, policy, p)
    return [slot0[:B], slot0[B:], draw_params_gated(seed, koff, 1, 0, 2 * B, S, policy, p)]


_REF = {}


def gated_reference(b):
    """Computed once per batch_no, shared by the f32 and bf16 tests: the float64 torch oracle of test_diffaug_gpu.step_reference's
    step under the records gated at p = 0.5"""
    if b not in _REF:
        cfg, W, inp, _, _, _ = step_reference(b)
        recs = gated_step_records(*key_of(0, 0, 3), cfg.batch_size, 16 * cfg.init_dim, 0.5)
        out = TO.step_gradients(AugNet(cfg, W, recs), b, {k: torch.tensor(v, dtype=torch.float64) for k, v in inp.items()})
        _REF[b] = (recs, {k: ([t.numpy() for t in v] if isinstance(v, list) else v.numpy() if torch.is_tensor(v) and v.ndim else
                              float(v) if torch.is_tensor(v) else v) for k, v in out.items()})
    return _REF[b]


@pytest.mark.parametrize("b", [1, 12], ids=["plain", "adjuster"])
@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_step_at_fixed_p_matches_the_gated_oracle(ops, mfma, b):
    """Without the feature diff_augment_p is unknown and every record is applied (the p = 1 oracle): this test fails there.
    The float64 oracle's losses: b = 1 gen 2.6065 / disc 3.3658 at p = 0.5 against 2.4726 / 3.5305 (p = 1) and 2.6628 / 3.6234 (p = 0)."""
    tol = TOLS[mfma]
    cfg, W, inp, _, ref_one, ref_zero = step_reference(b)     # p = 1: every record applied; p = 0: the un-augmented oracle
    recs, ref = gated_reference(b)
    keys = ("gen_loss", "disc_loss") + (("adj_loss",) if b > 10 else ())
    print(f"{mfma} b={b} oracle: " + "; ".join(f"{k} {ref[k]:.6f} / p=1 {ref_one[k]:.6f} / p=0 {ref_zero[k]:.6f}" for k in keys))
    # the gate matters at the bound that decides: the oracle at either end of p is at least five tolerances away in some loss
    bound = 5 * (tol["loss"] if mfma == "f32" else TOLS["bf16_emu"]["loss"])
    for other in (ref_one, ref_zero):
        assert max(abs(other[k] - ref[k]) / abs(ref[k]) for k in keys) > bound
    tr = build_aug(cfg, W, mfma, diff_augment_p=0.5)
    fake, adj, lg, ld, la = tr.train_step_from_inputs(b, dict(dev_inputs(inp), diffaug_key=dev_key(0, 0, 3)))
    torch.cuda.synchronize()
    print(f"{mfma} b={b} device: " + "; ".join(f"{k} {v.item():.6f}" for k, v in zip(keys, (lg, ld, la))))
    assert np.abs(fake.cpu().numpy() - ref["fake_image"]).max() < tol["img"]
    pairs, sets = [(lg, "gen_loss"), (ld, "disc_loss")], [("D", "dD"), ("G", "dG")]
    if b > 10:
        assert np.abs(adj.cpu().numpy() - ref["adj_image"]).max() < tol["img"]
        pairs.append((la, "adj_loss"))
        sets.append(("A", "dA"))
    else:
        assert adj is None and la is None
    for got, k in pairs:
        assert abs(got.item() - ref[k]) < tol["loss"] * abs(ref[k]), (k, got.item(), ref[k])
    only = {m: O.train_weight_indices(cfg, m, b) for m in "GDA"}
    check_grads(tr, ref, sets, tol, tag=f"ada {mfma} b={b}", only=only)
    if mfma == "bf16":   # the tight whole-step check of the bf16 path: the bf16-emulating oracle under the same gated records
        with aug_np_oracle(recs):
            check_emu(tr, cfg, W, b, inp, fake, adj, lg, ld, la, only=only)
    assert same_read(ops.ada_read(tr.ada_state), (0.5, 0, 0, 0)) and float(tr.ada_p()) == 0.5


ADAPT = dict(diff_augment_p=0.5, ada_target=0.6, ada_interval=2, ada_kimg=0.048)   # B = 3: an interval moves p by 6 / 48


@pytest.mark.parametrize("shift", [4.0, -4.0], ids=["up", "down"])
def test_controller_trajectory(ops, shift):
    """lr = 0 freezes the weights; the bias of the real/fake head is shifted so that D calls every real row real (up) or fake (down).
    Eager against graph replay bit for bit, and both against the restated controller fed with the signs of the float64 oracle's
    real_pr under the gated records of the p the device reported for the step.  10 steps: p leaves 0.5 by 0.125 per interval, reaches
    the end of its range after 4 intervals and is clamped there in the fifth."""
    cfg = O.Cfg(**{**SMALL, "lr": 0.0})
    W = perturbed(cfg, 2)
    W["D"][17] = W["D"][17] + shift                      # dense_pr's bias
    tr_e, tr_g = build_aug(cfg, W, "f32", **ADAPT), build_aug(cfg, W, "f32", **ADAPT)
    per_row = tr_e.ada["per_row"]
    assert per_row == PER_ROW and tr_e.ada["interval"] == 2 and F32(tr_e.ada["target"]) == F32(0.6)
    B, S = cfg.batch_size, 16 * cfg.init_dim
    host = f32_round(O.make_inputs(cfg, B, seed=77))
    base = dev_inputs(host)
    new_image = torch.tensor(host["new_image"], dtype=torch.float64)
    want = (F32(0.5), 0, 0, 0)
    seen = []
    for n in range(1, 11):
        p_now = ops.ada_read(tr_e.ada_state)[0]
        inp = dict(base, diffaug_key=dev_key(0, 0, n))
        _, _, lge, lde, lae = tr_e.train_step_from_inputs(12, inp)
        _, _, lgg, ldg, lag = tr_g.graph_step(12, inp)
        torch.cuda.synchronize()
        got, got_g = ops.ada_read(tr_e.ada_state), ops.ada_read(tr_g.ada_state)
        assert same_read(got_g, got) and tr_e._ada_steps == tr_g._ada_steps == got[3], (n, got, got_g)
        assert torch.equal(lge, lgg) and torch.equal(lde, ldg) and torch.equal(lae, lag), n
        recs = draw_params_gated(*key_of(0, 0, n), 0, 0, B, S, FULL, p_now)
        with torch.no_grad():
            real_pr = AugNet(cfg, W, [recs]).discriminator(new_image)[0].numpy()
        assert (np.abs(real_pr - 0.5) >= 100 * TOLS["f32"]["loss"]).all(), (n, real_pr.ravel())   # no sign hangs on the device's rounding
        want = ada_adjust_np(ada_accumulate_np(want, real_pr.reshape(B, 1), B), 2, tr_e.ada["target"], per_row)
        assert same_read(got, want), (n, got, want)
        seen.append(got[0])
    print(seen)
    assert len(tr_g._graphs) <= 2 and torch.equal(tr_e.store.flat, tr_g.store.flat)
    d = 0.125 if shift > 0 else -0.125
    assert seen == [0.5, 0.5 + d, 0.5 + d, 0.5 + 2 * d, 0.5 + 2 * d, 0.5 + 3 * d, 0.5 + 3 * d, 0.5 + 4 * d, 0.5 + 4 * d, 0.5 + 4 * d]
    assert seen[-1] == (1.0 if shift > 0 else 0.0)


def test_a_fixed_p_leaves_the_counters_alone(ops):
    cfg = O.Cfg(**SMALL)
    tr = build_aug(cfg, perturbed(cfg, 1), "f32", diff_augment_p=0.25)
    assert tr.ada["target"] is None
    for n, b in enumerate((10, 11, 12)):
        inp = dict(dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=60 + b))), diffaug_key=dev_key(0, 0, n + 1))
        tr.graph_step(b, inp)
        torch.cuda.synchronize()
        assert same_read(ops.ada_read(tr.ada_state), (0.25, 0, 0, 0)), b


def test_checkpoint_resume_continues_the_controller(ops, tmp_path):
    """ada_state is part of the checkpoint on the gated path: a restored trainer has the device state and the host mirror of the
    uninterrupted run, and lands on the same bits after the next step."""
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    cfg = O.Cfg(init_dim=2, conv_filter=(32, 32, 32, 32, 32), cond_dim=3, noise_dim=5, batch_size=2)

    def mk(restore, **kw):
        args = make_args(cfg, "f32")
        args.no_io, args.result_dir, args.restore, args.exp_name, args.epoch = False, str(tmp_path), restore, "t", 1
        args.diff_augment = FULL
        for k, v in dict(ADAPT, **kw).items():
            setattr(args, k, v)
        dec, enc = Decoder(args), Encoder(args)
        g = Generator(args, dec)
        d = Discriminator(args, enc)
        return EagerTrainer(args, g, d, Adjuster(args, d, g), None)

    data = [dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=70 + b))) for b in range(4)]

    def step(tr, b, d):
        noise, new_image = tr.draw_step_inputs(d["real_image_1"])
        tr.train_step_from_inputs(b, dict(d, noise=noise, new_image=new_image, diffaug_key=tr.draw_diffaug_key()))

    tr = mk(False)
    load_weights(tr, perturbed(cfg, 3))
    for b in range(3):
        step(tr, 9 + b, data[b])
    saved = ops.ada_read(tr.ada_state)
    assert saved[0] != 0.5 and saved[1:] != (0, 0, 0) and saved[3] == 1 == tr._ada_steps    # one interval done, one step into the next
    ck = tr.checkpoint_state()
    assert ck["ada_state"].dtype == torch.int32 and ck["ada_state"].tolist()[1:] == list(saved[1:])
    tr.save_checkpoint("7")
    step(tr, 12, data[3])
    want_flat, want_read = tr.store.flat.clone(), ops.ada_read(tr.ada_state)
    assert want_read[1:] == (0, 0, 0) and want_read[0] != saved[0]
    tr2 = mk(True)   # restores in the constructor
    assert same_read(ops.ada_read(tr2.ada_state), saved) and tr2._ada_steps == 1
    step(tr2, 12, data[3])
    assert torch.equal(tr2.store.flat, want_flat) and same_read(ops.ada_read(tr2.ada_state), want_read) and tr2._ada_steps == 0
    # a run that gates nothing ignores the key; a checkpoint without it starts from the configured p
    tr3 = mk(True, diff_augment_p=None, ada_target=None)
    assert tr3.ada is None and not hasattr(tr3, "ada_state")
    tr3.save_checkpoint("8")
    assert "ada_state" not in torch.load(os.path.join(str(tmp_path), "checkpoint", "ckpt-8.pt"), weights_only=True)
    tr4 = mk(True, diff_augment_p=0.75)
    assert same_read(ops.ada_read(tr4.ada_state), (0.75, 0, 0, 0)) and tr4._ada_steps == 0
    # a state that is none (p outside [0, 1] or NaN, negative counters, another length) is refused on restore, not loaded
    good = os.path.join(str(tmp_path), "checkpoint", "ckpt-7.pt")
    for bad in (words(float("nan")), words(1.5), words(-0.25), words(0.5, 0, -4, 1), words(0.5, 0, 4, -1), words(0.5)[:3]):
        ck = torch.load(good, weights_only=True)
        ck["ada_state"] = torch.from_numpy(np.ascontiguousarray(bad))
        torch.save(ck, os.path.join(str(tmp_path), "bad.pt"))
        with pytest.raises(ValueError, match="ada_state"):
            tr4.load_checkpoint(os.path.join(str(tmp_path), "bad.pt"))
    tr4.load_checkpoint(good)
    assert same_read(ops.ada_read(tr4.ada_state), saved) and tr4._ada_steps == 1


def test_p_one_without_a_target_is_the_plain_step(ops):
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 1)
    tr_a, tr_b = build_aug(cfg, W, "f32", diff_augment_p=1.0, ada_target=None), build_aug(cfg, W, "f32")
    assert tr_a.ada is None and not hasattr(tr_a, "ada_state") and tr_a.ada_p() is None
    for n, b in enumerate((1, 12)):
        inp = dict(dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=5 + b))), diffaug_key=dev_key(0, 0, n + 1))
        ra, rb = tr_a.train_step_from_inputs(b, inp), tr_b.train_step_from_inputs(b, inp)
        torch.cuda.synchronize()
        assert all((u is None) == (v is None) and (u is None or torch.equal(u, v)) for u, v in zip(ra, rb)), b
        assert _same_state(tr_a, tr_b), b
    assert "ada_state" not in tr_a.checkpoint_state()


# ---------------------------------------------------------------------------------------------------------------------- data parallel
def _rccl_ada_worker(outdir):
    """Fresh process (no GPU call before init_process_group): a world-size-1 `nccl` (= RCCL) group on cuda:0, as
    tests/test_dp_gpu.py::_rccl_single_worker builds it."""
    import datetime
    import json
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0), timeout=datetime.timedelta(seconds=120))
    try:
        from littlegan_amd import ops
        cfg = O.Cfg(**DP_CFG)
        W = perturbed(cfg, 23)
        tr_p, tr_s = build_aug(cfg, W, "bf16", **ADAPT), build_aug(cfg, W, "bf16", **ADAPT)
        assert not tr_p.sync.enabled
        tr_s.sync.force_enable()
        assert tr_s.sync.enabled and tr_s.sync.world_size == 1
        traj = []
        for n, b in enumerate((10, 11, 12, 13)):
            inp = dict(dev_inputs(_inputs(cfg, 1, b)), diffaug_key=dev_key(0, 0, n + 1))
            rp = tr_p.train_step_from_inputs(b, inp)
            rs = tr_s.train_step_from_inputs(b, inp)
            torch.cuda.synchronize()
            a, s = ops.ada_read(tr_p.ada_state), ops.ada_read(tr_s.ada_state)
            assert same_read(s, a) and tr_p._ada_steps == tr_s._ada_steps == a[3], (b, a, s)
            for x, y in zip(rp, rs):
                assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), b
            assert torch.equal(tr_p.store.flat, tr_s.store.flat), b
            traj.append(list(a))
        with open(os.path.join(outdir, "ada_traj.json"), "w") as f:
            json.dump(traj, f)
    finally:
        dist.destroy_process_group()


def test_rccl_world_size_one_keeps_the_trajectory(tmp_path):
    """On the step that completes an interval the counters {sum, rows} go through an all-reduce on the compute stream between
    accumulate and adjust: over one rank it is the identity, and the p trajectory of 4 steps (two intervals) equals, bit for bit, the
    one of a trainer without the process group."""
    import json
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_rccl_ada_worker, args=(str(tmp_path),))
    p.start()
    _join_all([p], 300)
    traj = json.loads((tmp_path / "ada_traj.json").read_text())
    assert [t[3] for t in traj] == [1, 0, 1, 0] and [t[1:3] for t in traj][1::2] == [[0, 0], [0, 0]], traj
    assert traj[0][0] == 0.5 and traj[1][0] != 0.5 and traj[2][0] == traj[1][0] and traj[3][0] != traj[2][0], traj   # B = 2: r is never 0.6
