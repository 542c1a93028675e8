"""Geometric augmentation of D's inputs (geom_augment) on the GPU.

Kernels: lgeo_draw against the restatement of tests/test_geom_cpu.py — rows without scale / rotate (blit-only policies, gated-off rows)
as exact numbers, the others within one fp32 ulp of the float64 restatement, 2^-23 max(1, |entry|) — for all 15 policy subsets, both call
slots, S = 8 / 16 / 128, ungated and at p = 0.3; lgeo_fwd against geom_np (the same fp32 weights, float64 sums) within
8 2^-24 max|x| per row (one rounding per weight product, per term and per add: 4 taps whose weights sum to 1), lgeo_bwd against the
scatter adjoint within (n + 3) 2^-24 sum |w g| per source pixel (n terms: one rounding per product, per term, per add), at
(B, S) = (3, 8), (5, 16), (2, 128): the smallest shapes at which the 4-pixel groups, the row stride and a multi-block grid can each go
wrong; the 8 permutation records and the identity bit for bit, both passes; <Geo x, g> = <x, Geo^T g> on the device's own outputs to a
relative 1e-5; row slices and repeated calls bit for bit; unusable records give zeros.
Whole steps at SMALL of tests/test_diffaug_gpu.py (S = 32), batch_no 1 and 12, with geom_augment alone and with both keys: against
oracle.torch_oracle.Net with geom_torch (then diffaug_torch) in front of its discriminator at TOLS["f32"] / TOLS["bf16"], the bf16 path
also against the bf16-emulating numpy oracle wrapped the same way at TOLS["bf16_emu"]; the feature off; eager against graph replay,
replays under new keys, checkpoint resume, the gated path, R1 on a penalty step."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import np_oracle as O  # noqa: E402
from oracle import torch_oracle as TO  # noqa: E402
from guards import called  # noqa: E402
from test_diffaug_cpu import diffaug_adjoint_np, diffaug_np, diffaug_torch, draw_params  # noqa: E402
from test_diffaug_gpu import FULL as DIFF_FULL, SMALL, _same_state, dev, dev_key  # noqa: E402
from test_geom_cpu import (BITS, FULL, IDENTITY, extreme_records, geom_adjoint_np, geom_np, geom_records, geom_torch, key_of,  # noqa: E402
                           permutation_records, permuted_np, usable)
from test_step_gpu import TOLS, check_emu, check_grads, dev_inputs, f32_round, load_weights, make_args, perturbed  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(3, 8), (5, 16), (2, 128)]


@pytest.fixture(scope="module")
def ops():
    from littlegan_amd import ops as _ops
    return _ops


def batches_of(B):
    """The extreme records in batches of B (cyclically: every record is used at every shape)"""
    ext = extreme_records()
    return [ext[(start + np.arange(B)) % len(ext)] for start in range(0, len(ext), B)]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------- the draws
_WANT = {}


def want_records(seed, koff, call, bits, p):
    k = (seed, koff, call, bits, p)
    if k not in _WANT:       # the draw does not read S: one restatement serves the three sizes
        _WANT[k] = geom_records(seed, koff, call, 0, 6, 16, bits, p)
    return _WANT[k]


@pytest.mark.parametrize("S", [8, 16, 128])
def test_draws_match_the_restatement(ops, S):
    key = dev_key(3, 1, 7)
    seed, koff = key.tolist()
    state = ops.ada_init(0.3, device="cuda")
    worst = 0.0
    for call in (0, 1):
        for bits in range(1, 16):
            for p, st in ((None, None), (0.3, state)):
                whole = ops.geom_draw(key, call, 0, 6, S, bits, state=st).cpu().numpy()
                want = want_records(seed, koff, call, bits, p)
                blit = (np.isin(np.abs(want), (0.0, 1.0))).all(axis=1)      # no scale, no rotate on this row: exact 0 / +-1
                assert bits & 12 or blit.all()
                assert np.array_equal(whole[blit], want[blit]) and not np.signbit(whole[whole == 0]).any(), (call, bits, p, whole, want)
                err = np.abs(whole.astype(np.float64) - want) / (2.0 ** -23 * np.maximum(1, np.abs(want)))
                worst = max(worst, float(err.max()))
                assert (err <= 1).all(), (call, bits, p, whole, want)
                part = ops.geom_draw(key, call, 3, 3, S, bits, state=st).cpu().numpy()
                assert np.array_equal(u32(part), u32(whole[3:])), (call, bits, p)
    print(f"S={S}: worst draw error {worst:.3f} of one fp32 ulp")
    assert np.array_equal(ops.geom_draw(key, 0, 0, 6, S, "").cpu().numpy(), np.tile(IDENTITY, (6, 1)))
    assert np.array_equal(ops.geom_draw(key, 0, 0, 6, S, FULL, state=ops.ada_init(0.0, device="cuda")).cpu().numpy(), np.tile(IDENTITY, (6, 1)))
    assert torch.equal(ops.geom_draw(key, 1, 0, 6, S, FULL, state=ops.ada_init(1.0, device="cuda")), ops.geom_draw(key, 1, 0, 6, S, FULL))
    deep = ops.geom_draw(key, 1, 509, 3, S, FULL).cpu().numpy()   # a row range deep inside a launch-shape batch, in the second block
    assert np.array_equal(u32(deep), u32(ops.geom_draw(key, 1, 0, 512, S, 15).cpu().numpy()[509:]))
    want = geom_records(seed, koff, 1, 509, 3, S, FULL)
    assert (np.abs(deep.astype(np.float64) - want) <= 2.0 ** -23 * np.maximum(1, np.abs(want))).all()


# ---------------------------------------------------------------------------------------------------------------------- Geo and its adjoint
@pytest.mark.parametrize("B,S", SHAPES)
def test_forward_and_backward_match_the_restatement(ops, B, S):
    rng = np.random.default_rng(100 + S)
    for recs in batches_of(B):
        x = rng.uniform(-1, 1, (B, S, S, 3)).astype(np.float32)
        g = rng.uniform(-1, 1, (B, S, S, 3)).astype(np.float32)
        out = ops.geom_fwd(dev(x), dev(recs)).cpu().numpy().astype(np.float64)
        gx = ops.geom_bwd(dev(g), dev(recs)).cpu().numpy().astype(np.float64)
        ref = geom_np(x, recs)
        gref, cnt, mag = geom_adjoint_np(g, recs, stats=True)
        tol_f = 8 * 2.0 ** -24 * np.abs(x).reshape(B, -1).max(axis=1)
        ef = np.abs(out - ref).reshape(B, -1).max(axis=1)
        tol_b = (cnt[..., None] + 3) * 2.0 ** -24 * mag
        eb = np.abs(gx - gref)
        share_b = float((eb / np.maximum(tol_b, 1e-300)).max())
        print(f"B={B} S={S}: fwd err / bound {np.round(ef / tol_f, 3)}, bwd worst err / bound {share_b:.3f}, most terms {int(cnt.max())}")
        assert (ef <= tol_f).all(), (recs, ef, tol_f)
        assert (eb <= tol_b).all(), (recs, share_b)
        # the zeros are exact: what no tap reaches holds +0
        assert np.array_equal(out == 0, ref == 0) and np.array_equal(gx == 0, gref == 0)


@pytest.mark.parametrize("B,S", SHAPES)
def test_permutation_and_identity_records_bit_for_bit(ops, B, S):
    rng = np.random.default_rng(S)
    x = rng.uniform(-1, 1, (9, S, S, 3)).astype(np.float32)
    g = rng.standard_normal((9, S, S, 3)).astype(np.float32)
    perms = permutation_records()
    recs = np.stack([r for r, _, _ in perms] + [IDENTITY])
    want = np.stack([permuted_np(x[n], flip, k) for n, (_, flip, k) in enumerate(perms)] + [x[8]])
    out = ops.geom_fwd(dev(x), dev(recs))
    assert np.array_equal(u32(out.cpu().numpy()), u32(want))
    # a permutation's adjoint is its inverse: Geo^T(Geo(g)) = g, and Geo^T(g) is g moved the other way
    assert np.array_equal(u32(ops.geom_bwd(ops.geom_fwd(dev(g), dev(recs)), dev(recs)).cpu().numpy()), u32(g))
    assert np.array_equal(u32(ops.geom_bwd(dev(g), dev(recs)).cpu().numpy()), u32(geom_adjoint_np(g, recs).astype(np.float32)))
    ident = dev(np.tile(IDENTITY, (B, 1)))
    xb, gb = dev(x[:B]), dev(g[:B])
    assert torch.equal(ops.geom_fwd(xb, ident), xb) and torch.equal(ops.geom_bwd(gb, ident), gb)


@pytest.mark.parametrize("B,S", SHAPES)
def test_backward_is_the_adjoint_of_the_forward_on_the_device(ops, B, S):
    """<Geo x, g> = <x, Geo^T g> per sample, both sides accumulated in float64 on the host, to a relative 1e-5.  g is the forward's own
    output plus half a uniform field: the left side is |Geo x|^2 plus a smaller term, never a sum that happens to cancel."""
    rng = np.random.default_rng(7 * S)
    for recs in batches_of(B):
        x = dev(rng.uniform(-1, 1, (B, S, S, 3)))
        p = dev(recs)
        t = ops.geom_fwd(x, p).cpu().numpy().astype(np.float64)
        g = dev(t + 0.5 * rng.uniform(-1, 1, t.shape))
        gx = ops.geom_bwd(g, p).cpu().numpy().astype(np.float64)
        xd, gd = x.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
        for n in range(B):
            lhs, rhs = float((t[n] * gd[n]).sum()), float((xd[n] * gx[n]).sum())
            if not usable(recs[n]):
                assert lhs == 0 and rhs == 0
                continue
            print(f"B={B} S={S} record {recs[n].tolist()}: <Geo x, g> {lhs:.9e}  <x, Geo^T g> {rhs:.9e}  rel {abs(lhs - rhs) / max(abs(lhs), abs(rhs)):.2e}")
            assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (n, recs[n], lhs, rhs)


@pytest.mark.parametrize("B,S", SHAPES)
def test_row_slices_and_repeated_calls_are_bit_identical(ops, B, S):
    rng = np.random.default_rng(3 * S)
    ext = extreme_records()
    recs = dev(ext[np.arange(2 * B) % len(ext)])
    x, g = dev(rng.uniform(-1, 1, (2 * B, S, S, 3))), dev(rng.uniform(-1, 1, (2 * B, S, S, 3)))
    whole_f, whole_b = ops.geom_fwd(x, recs), ops.geom_bwd(g, recs)
    assert torch.equal(ops.geom_fwd(x[B:], recs[B:]), whole_f[B:])
    assert torch.equal(ops.geom_bwd(g[B:], recs[B:]), whole_b[B:])
    assert torch.equal(ops.geom_fwd(x, recs), whole_f) and torch.equal(ops.geom_bwd(g, recs), whole_b)


def test_unusable_records_give_zeros_and_wrappers_refuse_wrong_shapes(ops):
    ext = extreme_records()
    dead = ext[[not usable(r) for r in ext]]
    assert len(dead) == 4
    x = torch.rand(len(dead), 16, 16, 3, device="cuda") + 1
    assert not ops.geom_fwd(x, dev(dead)).any() and not ops.geom_bwd(x, dev(dead)).any()
    x = torch.zeros(2, 16, 16, 3, device="cuda")
    p = torch.zeros(2, 4, device="cuda")
    for bad_x, bad_p in ((torch.zeros(2, 16, 8, 3, device="cuda"), p), (torch.zeros(2, 16, 16, 4, device="cuda"), p),
                         (x, torch.zeros(3, 4, device="cuda")), (x, torch.zeros(2, 8, device="cuda")), (x.double(), p)):
        with pytest.raises(ValueError):
            ops.geom_fwd(bad_x, bad_p)
    from littlegan_amd._lib import LittleGanHipError
    with pytest.raises(LittleGanHipError, match="lgeo_fwd: image side"):
        ops.geom_fwd(torch.zeros(2, 12, 12, 3, device="cuda"), p)
    with pytest.raises(LittleGanHipError, match="lgeo_bwd: in-place"):
        ops.geom_bwd(x, p, out=x)
    with pytest.raises(ValueError, match="geom_augment"):
        ops.geom_draw(dev_key(), 0, 0, 2, 16, "flip")
    with pytest.raises(LittleGanHipError, match="policy bits"):
        ops.geom_draw(dev_key(), 0, 0, 2, 16, 16)


# ---------------------------------------------------------------------------------------------------------------------- whole steps
def build_geo(cfg, W, mfma, geom=FULL, diff="", **kw):
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    args = make_args(cfg, mfma)
    args.geom_augment, args.diff_augment = geom, diff
    for k, v in kw.items():
        setattr(args, k, v)
    decoder, encoder = Decoder(args), Encoder(args)
    g = Generator(args, decoder)
    d = Discriminator(args, encoder)
    tr = EagerTrainer(args, g, d, Adjuster(args, d, g), None)
    load_weights(tr, W)
    return tr


def step_records(seed, koff, B, S, geom=FULL, diff="", p=None):
    """(geometric records, diff_augment records | None) of D's three calls in the order the oracles make them: D(new_image), D(fake),
    D(adj_image)"""
    g0 = geom_records(seed, koff, 0, 0, 2 * B, S, geom, p)
    geo = [g0[:B], g0[B:], geom_records(seed, koff, 1, 0, 2 * B, S, geom, p)]
    if not diff:
        return [(g, None) for g in geo]
    d0 = draw_params(seed, koff, 0, 0, 2 * B, S, diff)
    return list(zip(geo, [d0[:B], d0[B:], draw_params(seed, koff, 1, 0, 2 * B, S, diff)]))


class GeoNet(TO.Net):
    """oracle.torch_oracle.Net whose discriminator reads T(Geo(image)) under the next records"""

    def __init__(self, cfg, W_np, recs):
        super().__init__(cfg, W_np, torch.float64)
        self.recs = list(recs)

    def discriminator(self, image):
        geo, par = self.recs.pop(0)
        image = geom_torch(image, geo)
        return super().discriminator(image if par is None else diffaug_torch(image, par))


class geo_np_oracle:
    """While active, oracle.np_oracle's discriminator forward reads T(Geo(image)) and its backward returns Geo^T(T^T(.)) of the image
    gradient, under the next records (the way aug_np_oracle of tests/test_diffaug_gpu.py wraps it)."""

    def __init__(self, recs):
        self.recs = recs

    def _fwd(self, cfg, Wd, image):
        geo, par = self.todo.pop(0)
        image = geom_np(image, geo)
        out, cache = self.saved[0](cfg, Wd, image if par is None else diffaug_np(image, par))
        return out, (cache, geo, par)

    def _bwd(self, cfg, Wd, cache, d_pr, d_c, need_wgrad=True, need_input_grad=False):
        inner, geo, par = cache
        grads, d_in = self.saved[1](cfg, Wd, inner, d_pr, d_c, need_wgrad=need_wgrad, need_input_grad=need_input_grad)
        if d_in is not None:
            d_in = geom_adjoint_np(d_in if par is None else diffaug_adjoint_np(d_in, par), geo)
        return grads, d_in

    def __enter__(self):
        self.saved = (O.discriminator_fwd, O.discriminator_bwd)
        self.todo = list(self.recs)
        O.discriminator_fwd, O.discriminator_bwd = self._fwd, self._bwd
        return self

    def __exit__(self, *exc):
        O.discriminator_fwd, O.discriminator_bwd = self.saved


_REF = {}


def step_reference(b, diff="", p=None):
    """Computed once per (batch_no, diff_augment, p) and shared, unchanged, by the f32 and bf16 tests: inputs, the float64 torch oracle
    under the restated records, the two float64 restatements pinned against each other, and the un-augmented oracle."""
    if (b, diff, p) not in _REF:
        cfg = O.Cfg(**SMALL)
        W = perturbed(cfg, 1)
        inp = f32_round(O.make_inputs(cfg, cfg.batch_size, seed=50 + b))
        seed, koff = key_of(0, 0, 3)
        recs = step_records(seed, koff, cfg.batch_size, 16 * cfg.init_dim, FULL, diff, p)
        out = TO.step_gradients(GeoNet(cfg, W, recs), b, {k: torch.tensor(v, dtype=torch.float64) for k, v in inp.items()})
        ref = {k: ([t.numpy() for t in v] if isinstance(v, list) else v.numpy() if torch.is_tensor(v) and v.ndim else
                   float(v) if torch.is_tensor(v) else v) for k, v in out.items()}
        plain = O.step_gradients(cfg, W, b, inp)
        with geo_np_oracle(recs):
            ref_np = O.step_gradients(cfg, W, b, inp)
        for k in ("gen_loss", "disc_loss") + (("adj_loss",) if b > 10 else ()):
            assert abs(ref_np[k] - ref[k]) < 1e-10, k
        for key in ("dD", "dG") + (("dA",) if b > 10 else ()):
            for i, (u, v) in enumerate(zip(ref_np[key], ref[key])):
                assert np.abs(np.asarray(u).ravel() - np.asarray(v).ravel()).max() <= 1e-9 * (1 + np.abs(v).max()), (key, i)
        _REF[(b, diff, p)] = (cfg, W, inp, recs, ref, plain)
    return _REF[(b, diff, p)]


def check_step(tr, mfma, b, cfg, W, inp, recs, ref, plain, tag):
    tol = TOLS[mfma]
    fake, adj, lg, ld, la = tr.train_step_from_inputs(b, dict(dev_inputs(inp), diffaug_key=dev_key(0, 0, 3)))
    torch.cuda.synchronize()
    keys = ("gen_loss", "disc_loss") + (("adj_loss",) if b > 10 else ())
    print(f"{tag} {mfma} b={b}: " + "; ".join(f"{k} {v.item():.6f} / oracle {ref[k]:.6f} / un-augmented {plain[k]:.6f}"
                                                for k, v in zip(keys, (lg, ld, la))))
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
    check_grads(tr, ref, sets, tol, tag=f"{tag} {mfma} b={b}", only=only)
    if mfma == "bf16":   # the tight whole-step check of the bf16 path: the bf16-emulating oracle under the same records
        with geo_np_oracle(recs):
            check_emu(tr, cfg, W, b, inp, fake, adj, lg, ld, la, only=only)


@pytest.mark.parametrize("b", [1, 12], ids=["plain", "adjuster"])
@pytest.mark.parametrize("mfma", ["f32", "bf16"])
@pytest.mark.parametrize("diff", ["", DIFF_FULL], ids=["geom", "geom+diff"])
def test_step_matches_the_augmenting_oracle(diff, mfma, b):
    """Without the feature the key is ignored and the losses are those of the un-augmented (diff: the diff_augment-only) oracle: this
    test fails there."""
    cfg, W, inp, recs, ref, plain = step_reference(b, diff)
    keys = ("gen_loss", "disc_loss") + (("adj_loss",) if b > 10 else ())
    # the augmentation matters at the bound that decides: some loss of the un-augmented oracle is more than five tolerances away
    assert max(abs(plain[k] - ref[k]) / abs(ref[k]) for k in keys) > 5 * (TOLS["f32"]["loss"] if mfma == "f32" else TOLS["bf16_emu"]["loss"])
    if diff:   # ... and so is the oracle that applies diff_augment alone: the geometry is what this run adds
        from test_diffaug_gpu import step_reference as diff_reference
        only_t = diff_reference(b)[4]
        assert max(abs(only_t[k] - ref[k]) / abs(ref[k]) for k in keys) > 5 * (TOLS["f32"]["loss"] if mfma == "f32" else TOLS["bf16_emu"]["loss"])
    check_step(build_geo(cfg, W, mfma, FULL, diff), mfma, b, cfg, W, inp, recs, ref, plain, "geom" + ("+diff" if diff else ""))


def test_feature_off_is_the_step_without_the_key(ops, monkeypatch):
    """geom_augment "" : bit-identical to a trainer built without the key, and no lgeo_ function is fetched from the library"""
    from test_step_gpu import build
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 1)
    inp = dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=5)))
    fetched = called(monkeypatch, ops)
    off, never = build_geo(cfg, W, "f32", geom=""), build(cfg, W, "f32")
    assert not hasattr(make_args(cfg, "f32"), "geom_augment") and off.geom == 0 and not off.augmenting
    for b in (1, 12):
        ra = off.train_step_from_inputs(b, dict(inp, diffaug_key=dev_key(0, 0, 1)))
        rb = never.train_step_from_inputs(b, inp)
        torch.cuda.synchronize()
        assert all((u is None and v is None) or torch.equal(u, v) for u, v in zip(ra, rb)) and _same_state(off, never), b
    assert fetched and not [n for n in fetched if n.startswith("lgeo_")]
    # diff_augment alone: the launches of the diff_augment step, none of this feature's
    del fetched[:]
    build_geo(cfg, W, "f32", geom="", diff=DIFF_FULL).train_step_from_inputs(12, dict(inp, diffaug_key=dev_key(0, 0, 1)))
    torch.cuda.synchronize()
    assert "lg_diffaug_fwd" in fetched and not [n for n in fetched if n.startswith("lgeo_")]
    del fetched[:]
    build_geo(cfg, W, "f32").train_step_from_inputs(12, dict(inp, diffaug_key=dev_key(0, 0, 1)))
    torch.cuda.synchronize()
    assert {"lgeo_draw", "lgeo_fwd", "lgeo_bwd"} <= set(fetched) and "lg_diffaug_fwd" not in fetched


@pytest.mark.parametrize("diff", ["", DIFF_FULL], ids=["geom", "geom+diff"])
def test_graph_replay_is_bit_exact_with_geom_augment(diff):
    """graph_step against the eager path, a fresh key every step: both step kinds eager, captured and replayed"""
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 5)
    tr_e, tr_g = build_geo(cfg, W, "bf16", FULL, diff), build_geo(cfg, W, "bf16", FULL, diff)
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
    tr = build_geo(cfg, perturbed(cfg, 2), "bf16")
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
    uninterrupted run does, and lands on the same bits.  There is no state of this feature's own."""
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    cfg = O.Cfg(init_dim=2, conv_filter=(32, 32, 32, 32, 32), cond_dim=3, noise_dim=5, batch_size=2)

    def mk(restore):
        args = make_args(cfg, "f32")
        args.no_io, args.result_dir, args.restore, args.exp_name, args.epoch = False, str(tmp_path), restore, "t", 1
        args.geom_augment = FULL
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


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_gated_step_follows_p(mfma):
    """diff_augment_p with geom_augment alone: p = 0.5 against the oracle under the gated records; p = 0 against the un-augmented
    oracle (every record is the identity); p = 1 is the ungated step bit for bit."""
    b = 12
    cfg, W, inp, recs, ref, plain = step_reference(b, "", 0.5)
    _, _, _, recs1, _, _ = step_reference(b)
    assert any(not np.array_equal(g, g1) for (g, _), (g1, _) in zip(recs, recs1))
    tr = build_geo(cfg, W, mfma, diff_augment_p=0.5)
    assert tr.ada is not None and tr.ada["target"] is None and tr.diffaug == 0
    check_step(tr, mfma, b, cfg, W, inp, recs, ref, plain, "geom p=0.5")
    B = cfg.batch_size
    ident = [(np.tile(IDENTITY, (n, 1)), None) for n in (B, B, 2 * B)]
    check_step(build_geo(cfg, W, mfma, diff_augment_p=0.0), mfma, b, cfg, W, inp, ident, plain, plain, "geom p=0")
    di = dict(dev_inputs(inp), diffaug_key=dev_key(0, 0, 3))
    one, full = build_geo(cfg, W, mfma, diff_augment_p=0.999999, ada_target=None), build_geo(cfg, W, mfma)
    one.ada_state[:1].fill_(1.0)
    ro, rf = one.train_step_from_inputs(b, di), full.train_step_from_inputs(b, di)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(ro, rf)) and _same_state(one, full)


def test_adaptive_p_moves_under_geom_augment_alone():
    """ada_target with geom_augment alone: the controller runs where it runs under diff_augment and p leaves its start"""
    cfg = O.Cfg(**SMALL)
    tr = build_geo(cfg, perturbed(cfg, 4), "bf16", diff_augment_p=0.5, ada_target=0.6, ada_interval=2, ada_kimg=0.05)
    ps = []
    for n, b in enumerate([5, 6, 11, 12]):
        inp = dict(dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=5 + b))), diffaug_key=dev_key(0, 0, n + 1))
        tr.graph_step(b, inp)
        ps.append(float(tr.ada_p()))
    print(ps)
    assert ps[0] == 0.5 and ps[1] != 0.5 and ps[2] == ps[1] and ps[3] != ps[2] and all(0.0 <= v <= 1.0 for v in ps)   # B = 3: r is never 0.6


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_r1_penalty_step_under_geom_augment(ops, mfma):
    """The penalty under geom_augment is taken on Geo(new_image), with respect to it: the reference is the augmenting
    oracle plus np_r1 of tests/test_r1_gpu.py on the device's own Geo(new_image), read back."""
    from test_r1_gpu import GAMMA, _with_r1
    tol = TOLS[mfma]
    b = 1
    cfg, W, inp, _, ref, _ = step_reference(b)
    B, S = cfg.batch_size, 16 * cfg.init_dim
    tr = build_geo(cfg, W, mfma, r1_gamma=GAMMA, r1_interval=1)
    key = dev_key(0, 0, 3)
    di = dev_inputs(inp)
    fake, adj, lg, ld, la = tr.train_step_from_inputs(b, dict(di, diffaug_key=key))
    x_aug = ops.geom_fwd(di["new_image"], ops.geom_draw(key, 0, 0, B, S, tr.geom))
    torch.cuda.synchronize()
    assert not torch.equal(x_aug, di["new_image"])
    ref2, term = _with_r1(ref, cfg, W, x_aug.cpu().double().numpy(), GAMMA)
    want = ref["disc_loss"] + term
    print(f"{mfma}: disc {ld.item():.7g} / {want:.7g}, r1 {float(tr.losses['r1']):.7g} / {term:.7g}")
    assert abs(lg.item() - ref["gen_loss"]) < tol["loss"] * abs(ref["gen_loss"])
    assert abs(ld.item() - want) < tol["loss"] * abs(want)
    assert abs(float(tr.losses["r1"]) - term) < max(tol["loss"], 1e-4) * abs(term) + 1e-7
    check_grads(tr, ref2, [("D", "dD"), ("G", "dG")], tol, tag=f"r1 geom {mfma}", only={m: O.train_weight_indices(cfg, m, b) for m in "GDA"})
