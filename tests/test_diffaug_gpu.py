"""Differentiable augmentation of D's inputs (diff_augment) on the GPU.

Kernels: lg_diffaug_draw against the restatement of tests/test_diffaug_cpu.py bit for bit (every policy subset, both call slots, a row
range); lg_diffaug_fwd / lg_diffaug_bwd against the float64 definition and its adjoint under hand-built records at the ends of every
range, at (B, S) = (3, 8) (M = 1, cut = 4: the smallest image where every branch exists), (5, 16) and (2, 128) (the workload's row
length), within 5e-6 x the absolute coefficient sum of the affine map per sample (the bound tests/test_inputs.py holds the augment kernel
to at unit coefficients); the identity record bit for bit; <T(x) - T(0), g> = <x, T^T g> on the device's own outputs to a relative 1e-5
(fp32 rounding of ~10 operations per element, independent of the restatement); row slices and repeated calls bit for bit.
Whole steps at the small geometry of tests/test_step_gpu.py (batch_no 1 and 12: without and with the Adjuster branch): against
oracle.torch_oracle.Net whose discriminator applies the restated T in float64 to what it is given, with the records of slot 0 rows
0..B, slot 0 rows B..2B and slot 1 in the order step_gradients calls it, at TOLS["f32"] / TOLS["bf16"]; the bf16 path also against the
bf16-emulating numpy oracle with its discriminator forward / backward wrapped the same way, at TOLS["bf16_emu"]; eager against graph
replay, replays under other keys, checkpoint resume, the refused combinations."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import np_oracle as O  # noqa: E402
from oracle import torch_oracle as TO  # noqa: E402
from test_diffaug_cpu import (BITS, IDENTITY, diffaug_adjoint_np, diffaug_np, diffaug_torch, draw_params, extreme_records,  # noqa: E402
                              key_of)
from test_step_gpu import TOLS, check_emu, check_grads, dev_inputs, f32_round, load_weights, make_args, perturbed  # noqa: E402

pytestmark = pytest.mark.gpu

FULL = "color,translation,cutout"
SMALL = dict(init_dim=2, conv_filter=(64, 32, 32, 32, 32), cond_dim=5, noise_dim=11, batch_size=3)
SHAPES = [(3, 8), (5, 16), (2, 128)]


@pytest.fixture(scope="module")
def ops():
    from littlegan_amd import ops as _ops
    return _ops


def dev_key(seed_arg=0, rank=0, step=1):
    return torch.tensor(key_of(seed_arg, rank, step), dtype=torch.int64, device="cuda")


def dev(a):
    return torch.tensor(np.asarray(a, np.float32), device="cuda").contiguous()


def coef_sum(recs):
    b, s, c = (np.asarray(recs, np.float64)[:, k] for k in range(3))
    return np.maximum(1.0, np.abs(c * s) + np.abs(c * (1 - s)) + np.abs(1 - c) + np.abs(b))


def batches_of(B, S):
    """The extreme records in batches of B (cyclically: every record is used at every shape)"""
    ext = extreme_records(S)
    return [ext[(start + np.arange(B)) % len(ext)] for start in range(0, len(ext), B)]


# ---------------------------------------------------------------------------------------------------------------------- the draws
@pytest.mark.parametrize("S", [8, 16, 128])
def test_draws_equal_the_restatement_bit_for_bit(ops, S):
    key = dev_key(3, 1, 7)
    seed, koff = key.tolist()
    for call in (0, 1):
        for bits in range(1, 8):
            names = ",".join(n for n, v in BITS.items() if bits & v)
            whole = ops.diffaug_draw(key, call, 0, 6, S, names).cpu().numpy()
            want = draw_params(seed, koff, call, 0, 6, S, names)
            assert np.array_equal(whole.view(np.uint32), want.view(np.uint32)), (call, names, whole, want)
            part = ops.diffaug_draw(key, call, 3, 3, S, bits).cpu().numpy()
            assert np.array_equal(part.view(np.uint32), whole[3:].view(np.uint32)), (call, names)
    assert np.array_equal(ops.diffaug_draw(key, 0, 0, 6, S, "").cpu().numpy(), np.tile(IDENTITY, (6, 1)))
    deep = ops.diffaug_draw(key, 1, 509, 3, S, FULL).cpu().numpy()   # a row range deep inside a launch-shape batch
    assert np.array_equal(deep.view(np.uint32), draw_params(seed, koff, 1, 509, 3, S, FULL).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------- T and its adjoint
@pytest.mark.parametrize("B,S", SHAPES)
def test_forward_and_backward_match_the_definition(ops, B, S):
    rng = np.random.default_rng(100 + S)
    for recs in batches_of(B, S):
        x = rng.uniform(-1, 1, (B, S, S, 3)).astype(np.float32)
        g = rng.uniform(-1, 1, (B, S, S, 3)).astype(np.float32)
        out = ops.diffaug_fwd(dev(x), dev(recs)).cpu().numpy().astype(np.float64)
        gx = ops.diffaug_bwd(dev(g), dev(recs)).cpu().numpy().astype(np.float64)
        ref, gref = diffaug_np(x, recs), diffaug_adjoint_np(g, recs)
        tol = 5e-6 * coef_sum(recs)
        ef = np.abs(out - ref).reshape(B, -1).max(axis=1)
        eb = np.abs(gx - gref).reshape(B, -1).max(axis=1)
        gmax = np.abs(g).reshape(B, -1).max(axis=1)
        print(f"B={B} S={S}: fwd err / tol {np.round(ef / tol, 3)}, bwd err / tol {np.round(eb / (tol * gmax), 3)}")
        assert (ef <= tol).all(), (recs, ef, tol)
        assert (eb <= tol * gmax).all(), (recs, eb, tol * gmax)
        # the zeros are exact: cut pixels and the shifted-in band hold +0, not a rounded remainder
        assert np.array_equal(out == 0, ref == 0)


@pytest.mark.parametrize("B,S", SHAPES)
def test_identity_record_returns_its_input_bit_for_bit(ops, B, S):
    rng = np.random.default_rng(S)
    x, g = dev(rng.uniform(-1, 1, (B, S, S, 3))), dev(rng.standard_normal((B, S, S, 3)))
    ident = dev(np.tile(IDENTITY, (B, 1)))
    assert torch.equal(ops.diffaug_fwd(x, ident), x)
    assert torch.equal(ops.diffaug_bwd(g, ident), g)


@pytest.mark.parametrize("B,S", SHAPES)
def test_backward_is_the_adjoint_of_the_forward_on_the_device(ops, B, S):
    """<T(x) - T(0), g> = <x, T^T g> per sample, both sides accumulated in float64 on the host, to a relative 1e-5.  g is the forward's
    own linear part plus half a uniform field, g = (T(x) - T(0)) + u / 2: the left side is then |T(x) - T(0)|^2 plus a smaller term, so
    the comparison is never one of two sums that happen to cancel (with independent x and g, |<.,.>| falls below 1/20 of its typical
    size in one sample out of thirty, and a relative bound on it then measures the cancellation, not the kernels)."""
    rng = np.random.default_rng(7 * S)
    for recs in batches_of(B, S):
        x = dev(rng.uniform(-1, 1, (B, S, S, 3)))
        p = dev(recs)
        t = ops.diffaug_fwd(x, p).cpu().numpy().astype(np.float64) - ops.diffaug_fwd(torch.zeros_like(x), p).cpu().numpy().astype(np.float64)
        g = dev(t + 0.5 * rng.uniform(-1, 1, t.shape))
        gx = ops.diffaug_bwd(g, p).cpu().numpy().astype(np.float64)
        xd, gd = x.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
        for n in range(B):
            lhs, rhs = float((t[n] * gd[n]).sum()), float((xd[n] * gx[n]).sum())
            print(f"B={B} S={S} record {recs[n].tolist()}: <Tx - T0, g> {lhs:.9e}  <x, T^T g> {rhs:.9e}  rel {abs(lhs - rhs) / max(abs(lhs), abs(rhs)):.2e}")
            assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (n, recs[n], lhs, rhs)


@pytest.mark.parametrize("B,S", SHAPES)
def test_row_slices_and_repeated_calls_are_bit_identical(ops, B, S):
    rng = np.random.default_rng(3 * S)
    ext = extreme_records(S)
    recs = dev(ext[np.arange(2 * B) % len(ext)])
    x, g = dev(rng.uniform(-1, 1, (2 * B, S, S, 3))), dev(rng.uniform(-1, 1, (2 * B, S, S, 3)))
    whole_f, whole_b = ops.diffaug_fwd(x, recs), ops.diffaug_bwd(g, recs)
    assert torch.equal(ops.diffaug_fwd(x[B:], recs[B:]), whole_f[B:])
    assert torch.equal(ops.diffaug_bwd(g[B:], recs[B:]), whole_b[B:])
    assert torch.equal(ops.diffaug_fwd(x, recs), whole_f) and torch.equal(ops.diffaug_bwd(g, recs), whole_b)


def test_wrappers_refuse_wrong_shapes(ops):
    x = torch.zeros(2, 16, 16, 3, device="cuda")
    p = torch.zeros(2, 8, device="cuda")
    for bad_x, bad_p in ((torch.zeros(2, 16, 8, 3, device="cuda"), p), (torch.zeros(2, 16, 16, 4, device="cuda"), p),
                         (x, torch.zeros(3, 8, device="cuda")), (x.double(), p)):
        with pytest.raises(ValueError):
            ops.diffaug_fwd(bad_x, bad_p)
    from littlegan_amd._lib import LittleGanHipError
    with pytest.raises(LittleGanHipError, match="image side"):
        ops.diffaug_fwd(torch.zeros(2, 12, 12, 3, device="cuda"), p)
    with pytest.raises(LittleGanHipError, match="in-place"):
        ops.diffaug_fwd(x, p, out=x)
    with pytest.raises(ValueError, match="diff_augment"):
        ops.diffaug_draw(dev_key(), 0, 0, 2, 16, "colour")


# ---------------------------------------------------------------------------------------------------------------------- whole steps
def build_aug(cfg, W, mfma, policy=FULL, **kw):
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    args = make_args(cfg, mfma)
    args.diff_augment = policy
    for k, v in kw.items():
        setattr(args, k, v)
    decoder, encoder = Decoder(args), Encoder(args)
    g = Generator(args, decoder)
    d = Discriminator(args, encoder)
    tr = EagerTrainer(args, g, d, Adjuster(args, d, g), None)
    load_weights(tr, W)
    return tr


def step_records(seed, koff, B, S, policy=FULL):
    """The records of D's three calls in the order the oracles make them: D(new_image), D(fake), D(adj_image)"""
    slot0 = draw_params(seed, koff, 0, 0, 2 * B, S, policy)
    return [slot0[:B], slot0[B:], draw_params(seed, koff, 1, 0, 2 * B, S, policy)]


class AugNet(TO.Net):
    """oracle.torch_oracle.Net whose discriminator reads T(image) under the next records"""

    def __init__(self, cfg, W_np, recs):
        super().__init__(cfg, W_np, torch.float64)
        self.recs = list(recs)

    def discriminator(self, image):
        return super().discriminator(diffaug_torch(image, self.recs.pop(0)))


class aug_np_oracle:
    """While active, oracle.np_oracle's discriminator forward reads T(image) and its backward returns T^T of the image gradient, under
    the next records of `recs` (the way masked_np_oracle of tests/test_dropout_gpu.py wraps the encoder)."""

    def __init__(self, recs):
        self.recs = recs

    def _fwd(self, cfg, Wd, image):
        par = self.todo.pop(0)
        out, cache = self.saved[0](cfg, Wd, diffaug_np(image, par))
        return out, (cache, par)

    def _bwd(self, cfg, Wd, cache, d_pr, d_c, need_wgrad=True, need_input_grad=False):
        inner, par = cache
        grads, d_in = self.saved[1](cfg, Wd, inner, d_pr, d_c, need_wgrad=need_wgrad, need_input_grad=need_input_grad)
        return grads, (None if d_in is None else diffaug_adjoint_np(d_in, par))

    def __enter__(self):
        self.saved = (O.discriminator_fwd, O.discriminator_bwd)
        self.todo = list(self.recs)
        O.discriminator_fwd, O.discriminator_bwd = self._fwd, self._bwd
        return self

    def __exit__(self, *exc):
        O.discriminator_fwd, O.discriminator_bwd = self.saved


_REF = {}


def step_reference(b):
    """Computed once per batch_no and shared, unchanged, by the f32 and bf16 tests: inputs, the float64 torch oracle under the
    restated records, the two float64 restatements pinned against each other, and the un-augmented oracle."""
    if b not in _REF:
        cfg = O.Cfg(**SMALL)
        W = perturbed(cfg, 1)
        inp = f32_round(O.make_inputs(cfg, cfg.batch_size, seed=50 + b))
        seed, koff = key_of(0, 0, 3)
        recs = step_records(seed, koff, cfg.batch_size, 16 * cfg.init_dim)
        out = TO.step_gradients(AugNet(cfg, W, recs), b, {k: torch.tensor(v, dtype=torch.float64) for k, v in inp.items()})
        ref = {k: ([t.numpy() for t in v] if isinstance(v, list) else v.numpy() if torch.is_tensor(v) and v.ndim else
                   float(v) if torch.is_tensor(v) else v) for k, v in out.items()}
        plain = O.step_gradients(cfg, W, b, inp)
        with aug_np_oracle(recs):
            ref_np = O.step_gradients(cfg, W, b, inp)
        for k in ("gen_loss", "disc_loss") + (("adj_loss",) if b > 10 else ()):
            assert abs(ref_np[k] - ref[k]) < 1e-10, k
        for key in ("dD", "dG") + (("dA",) if b > 10 else ()):
            for i, (u, v) in enumerate(zip(ref_np[key], ref[key])):
                assert np.abs(np.asarray(u).ravel() - np.asarray(v).ravel()).max() <= 1e-9 * (1 + np.abs(v).max()), (key, i)
        _REF[b] = (cfg, W, inp, recs, ref, plain)
    return _REF[b]


@pytest.mark.parametrize("b", [1, 12], ids=["plain", "adjuster"])
@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_step_matches_the_augmenting_oracle(mfma, b):
    """Without the feature the key is ignored and the losses are those of the un-augmented oracle: this test fails there."""
    tol = TOLS[mfma]
    cfg, W, inp, recs, ref, plain = step_reference(b)
    tr = build_aug(cfg, W, mfma)
    fake, adj, lg, ld, la = tr.train_step_from_inputs(b, dict(dev_inputs(inp), diffaug_key=dev_key(0, 0, 3)))
    torch.cuda.synchronize()
    keys = ("gen_loss", "disc_loss") + (("adj_loss",) if b > 10 else ())
    print(f"{mfma} b={b}: " + "; ".join(f"{k} {v.item():.6f} / oracle {ref[k]:.6f} / un-augmented {plain[k]:.6f}"
                                        for k, v in zip(keys, (lg, ld, la))))
    # the augmentation matters at the bound that decides: some loss of the un-augmented oracle is at least five tolerances away (the
    # float64 oracle's on the f32 path, the bf16-emulating oracle's on the bf16 path)
    assert max(abs(plain[k] - ref[k]) / abs(ref[k]) for k in keys) > 5 * (tol["loss"] if mfma == "f32" else TOLS["bf16_emu"]["loss"])
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
    check_grads(tr, ref, sets, tol, tag=f"diffaug {mfma} b={b}", only=only)
    if mfma == "bf16":   # the tight whole-step check of the bf16 path: the bf16-emulating oracle under the same records
        with aug_np_oracle(recs):
            check_emu(tr, cfg, W, b, inp, fake, adj, lg, ld, la, only=only)


def _same_state(a, b):
    return all(torch.equal(x, y) for x, y in ((a.store.flat, b.store.flat), (a.store.m, b.store.m), (a.store.v, b.store.v))) and \
        all(torch.equal(a.opt_state[m], b.opt_state[m]) for m in "GDA")


def test_graph_replay_is_bit_exact_with_diff_augment():
    """graph_step against the eager path, a fresh key every step: both step kinds eager, captured and replayed"""
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 5)
    tr_e, tr_g = build_aug(cfg, W, "bf16"), build_aug(cfg, W, "bf16")
    for n, b in enumerate([7, 8, 9, 11, 12, 13, 14]):
        inp = dict(dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=400 + b))), diffaug_key=dev_key(0, 0, n + 1))
        fe, ae, lge, lde, lae = tr_e.train_step_from_inputs(b, inp)
        fg, ag, lgg, ldg, lag = tr_g.graph_step(b, inp)
        torch.cuda.synchronize()
        assert torch.equal(fe, fg) and torch.equal(lge, lgg) and torch.equal(lde, ldg), b
        assert (ae is None) == (ag is None) and (ae is None or (torch.equal(ae, ag) and torch.equal(lae, lag))), b
        assert _same_state(tr_e, tr_g), b
    assert len(tr_g._graphs) == 2


def test_replays_of_one_graph_draw_new_records():
    """lr = 0 freezes the weights, so a step's losses depend on its inputs and records alone: replays of ONE captured graph with the
    same inputs give the same losses under the same key and other losses under another."""
    cfg = O.Cfg(**{**SMALL, "lr": 0.0})
    tr = build_aug(cfg, perturbed(cfg, 2), "bf16")
    base = dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=77)))
    w0 = tr.store.flat.clone()
    seen = []
    for k in (1, 1, 1, 2, 1, 3):     # eager, capture + replay, replay, ...
        _, _, lg, ld, la = tr.graph_step(11, dict(base, diffaug_key=dev_key(0, 0, k)))
        torch.cuda.synchronize()
        seen.append((k, lg.item(), ld.item(), la.item()))
    assert len(tr._graphs) == 1 and torch.equal(tr.store.flat, w0)
    print(seen)
    assert seen[0][1:] == seen[1][1:] == seen[2][1:] == seen[4][1:]          # key 1: eager == replays, bit for bit
    for i in (1, 2, 3):                                                        # gen, disc and adj loss under keys 2 and 3
        assert seen[3][i] != seen[2][i] and seen[5][i] != seen[3][i] and seen[5][i] != seen[2][i], i


def test_checkpoint_resume_continues_the_record_stream(tmp_path):
    """input_step is part of the checkpoint: a restored trainer draws the inputs AND the augmentation key of the next step as the
    uninterrupted run does, and lands on the same bits."""
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    cfg = O.Cfg(init_dim=2, conv_filter=(32, 32, 32, 32, 32), cond_dim=3, noise_dim=5, batch_size=2)

    def mk(restore):
        args = make_args(cfg, "f32")
        args.no_io, args.result_dir, args.restore, args.exp_name, args.epoch = False, str(tmp_path), restore, "t", 1
        args.diff_augment = FULL
        dec, enc = Decoder(args), Encoder(args)
        g = Generator(args, dec)
        d = Discriminator(args, enc)
        return EagerTrainer(args, g, d, Adjuster(args, d, g), None)

    data = [dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=70 + b))) for b in range(4)]

    def step(tr, b, d):
        noise, new_image = tr.draw_step_inputs(d["real_image_1"])
        inp = dict(d, noise=noise, new_image=new_image, diffaug_key=tr.draw_diffaug_key())
        tr.train_step_from_inputs(b, inp)
        return inp["diffaug_key"].tolist()

    tr = mk(False)
    load_weights(tr, perturbed(cfg, 3))
    keys = [step(tr, 9 + b, data[b]) for b in range(3)]
    assert len({tuple(k) for k in keys}) == 3 and keys[2] == list(key_of(0, 0, 3))
    tr.save_checkpoint("7")
    k4 = step(tr, 12, data[3])
    want = tr.store.flat.clone()
    tr2 = mk(True)   # restores in the constructor
    assert tr2._input_step == 3
    assert step(tr2, 12, data[3]) == k4 == list(key_of(0, 0, 4))
    assert torch.equal(tr2.store.flat, want)


def test_refused_combinations_and_the_missing_key():
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 1)
    with pytest.raises(ValueError, match="diff_augment and use_gp"):
        build_aug(cfg, W, "f32", use_gp=True)
    with pytest.raises(ValueError, match="diff_augment and dropout_train"):
        build_aug(cfg, W, "f32", dropout_train=True)
    with pytest.raises(ValueError, match="diff_augment"):
        build_aug(cfg, W, "f32", policy="color,rotate")
    tr = build_aug(cfg, W, "f32")
    inp = dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=5)))
    with pytest.raises(ValueError, match="diffaug_key"):
        tr.train_step_from_inputs(1, inp)
    # off: the key is ignored and the step is the un-augmented one, bit for bit
    off_a, off_b = build_aug(cfg, W, "f32", policy=""), build_aug(cfg, W, "f32", policy="")
    ra = off_a.train_step_from_inputs(12, dict(inp, diffaug_key=dev_key(0, 0, 1)))
    rb = off_b.train_step_from_inputs(12, inp)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(ra, rb)) and _same_state(off_a, off_b)
