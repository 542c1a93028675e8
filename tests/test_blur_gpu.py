"""The faded blur of D's inputs (blur_init_sigma, blur_fade_kimg) on the GPU.

Kernels: lgblur_apply against blur_np of tests/test_blur_cpu.py (the fp32 taps of config.blur_taps, float64 sums) within
8 (R + 2) 2^-24 max|x| — two passes of 2R + 1 terms whose weights sum to at most 1, one rounding per product and per add, plus the
rounding of the device's own taps, with a factor of two over it — at (rows, S) = (1, 8), (3, 16), (2, 24), (2, 40), (1, 136) and
sigma = 0.2, 0.34, 1, 2.7, 10 (R = 0, 1, 3, 8, 30; S = 8 under R = 30 puts most taps outside the image; 24 and 40 are no multiple of the
32-pixel tile, 40 and 136 take more than one tile a side), and once at (1, 1024); R = 0 bit for bit; the impulse response bit-symmetric
and within 4 ulp of the product of the restated taps; <Blur x, g> = <x, Blur g> on the device's own outputs within the same bound; row
slices and repeated calls bit for bit; lgblur_step against config.blur_restate bit for bit; unusable sigmas.  (Every pointer-taking call
inside guard bands: the blur-* rows of tests/test_memory_contract_gpu.py, on this module's data.)
Whole steps at SMALL of tests/test_diffaug_gpu.py (S = 32, B = 3), batch_no 1 and 12, with the blur alone and on top of geom_augment +
diff_augment: against oracle.np_oracle whose discriminator reads the restated Blur (then Geo, then T) and whose backward blurs the
image gradient, at the tolerances of tests/test_geom_gpu.py; the key off; the fade-out; eager against graph replay across the fade;
checkpoint resume; R1 on a penalty step."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import np_oracle as O  # noqa: E402
from guards import called  # noqa: E402
from test_blur_cpu import SIGMAS, blur_np  # noqa: E402
from test_diffaug_cpu import diffaug_adjoint_np, diffaug_np  # noqa: E402
from test_diffaug_gpu import FULL as DIFF_FULL, SMALL, _same_state, dev, dev_key  # noqa: E402
from test_geom_cpu import FULL as GEOM_FULL, geom_adjoint_np, geom_np, key_of  # noqa: E402
from test_geom_gpu import TOLS, geo_np_oracle, step_records  # noqa: E402
from test_step_gpu import build, check_emu, check_grads, dev_inputs, f32_round, load_weights, make_args, perturbed  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SHAPES = [(1, 8), (3, 16), (2, 24), (2, 40), (1, 136)]
CASES = [(rows, S, sigma, R) for rows, S in SHAPES for sigma, R in SIGMAS] + [(1, 1024, 10.0, 30)]


@pytest.fixture(scope="module")
def ops():
    from littlegan_amd import ops as _ops
    return _ops


def bound(R, xmax):
    return 8.0 * (R + 2) * 2.0 ** -24 * xmax


def state_words(sigma, k=0, w2=0, w3=0):
    """the 16-byte state as four 32-bit words, host side"""
    return np.array([k, int(np.array(sigma, F32).view(np.int32)), w2, w3], np.int64).astype(np.uint32).view(np.int32)


def state_of(sigma, k=0):
    return torch.tensor(state_words(sigma, k), dtype=torch.int32, device="cuda").view(torch.float32)


_X = {}


def images(rows, S, seed=0):
    """random inputs in [-1, 1], drawn once per shape"""
    if (rows, S, seed) not in _X:
        _X[(rows, S, seed)] = np.random.default_rng(1000 * S + rows + seed).uniform(-1, 1, (rows, S, S, 3)).astype(F32)
    return _X[(rows, S, seed)]


def blur_names(fetched):
    """the lgblur_ names among the ABI names guards.called recorded, in order"""
    return [n for n in fetched if n.startswith("lgblur_")]


def bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------- the operator
@pytest.mark.parametrize("rows,S,sigma,R", CASES, ids=lambda v: str(v))
def test_apply_matches_the_restatement(ops, rows, S, sigma, R):
    from littlegan_amd import config
    assert config.blur_radius(sigma) == R
    x = images(rows, S)
    got = ops.blur_apply(dev(x), state_of(sigma))
    torch.cuda.synchronize()
    if R == 0:
        assert torch.equal(bits(got), bits(dev(x)))
        return
    want = blur_np(x, sigma)
    err = np.abs(got.cpu().numpy().astype(F64) - want).max()
    print(f"rows {rows} S {S} sigma {sigma} R {R}: max err {err:.3e}, bound {bound(R, np.abs(x).max()):.3e}")
    assert err <= bound(R, np.abs(x).max())


def blur_f32(x, sigma):
    """Blur(x) as the definition orders it, in fp32: every sum from +0, the taps in ascending order, one rounding per multiply and per
    add, zeros outside the image (adding +0 changes no bit).  The taps are the host's (config.blur_taps)."""
    from littlegan_amd.config import blur_taps
    R, w = blur_taps(F32(sigma))
    out, S = np.asarray(x, F32), x.shape[1]
    for axis in (2, 1):   # H, then V
        pad = [(0, 0)] * 4
        pad[axis] = (R, R)
        xp = np.pad(out, pad)
        acc = np.zeros_like(out)
        for i in range(-R, R + 1):
            sl = [slice(None)] * 4
            sl[axis] = slice(R + i, R + i + S)
            acc = (acc + (w[abs(i)] * xp[tuple(sl)]).astype(F32)).astype(F32)
        out = acc
    return out


@pytest.mark.parametrize("sigma", [0.34, 1.0, 10.0])
def test_apply_gives_the_bits_of_the_definition(ops, sigma):
    """The bits of an output pixel depend on its image, sigma and S only: the device equals the sequential fp32 restatement bit for bit
    at S = 128 (four strips, four chunks a strip), so neither the strip nor the chunk geometry shows."""
    x = images(1, 128)
    got = ops.blur_apply(dev(x), state_of(sigma)).cpu().numpy()
    assert np.array_equal(got.view(np.int32), blur_f32(x, sigma).view(np.int32))


@pytest.mark.parametrize("S", [8, 24])
def test_impulse_response_is_symmetric_and_the_product_of_the_taps(ops, S):
    from littlegan_amd import config
    n = S * S
    eye = torch.zeros(n, S, S, 3, device="cuda")
    eye.view(n, n, 3)[torch.arange(n), torch.arange(n)] = 1.0
    yy, xx = np.divmod(np.arange(n), S)
    dy, dx = np.abs(yy[:, None] - yy[None, :]), np.abs(xx[:, None] - xx[None, :])
    for sigma, R in SIGMAS[1:]:
        out = ops.blur_apply(eye, state_of(sigma))
        torch.cuda.synchronize()
        for c in range(3):
            M = out[..., c].reshape(n, n).cpu().numpy()       # row p: the response to a one-hot pixel p, read at every q
            assert np.array_equal(M.view(np.int32), M.T.view(np.int32)), (sigma, c)
            w = np.concatenate([config.blur_taps(sigma)[1], np.zeros(S, F32)])
            E = (w[np.minimum(dy, R + 1)] * w[np.minimum(dx, R + 1)]).astype(F32)      # fp32 product of fp32 taps; 0 beyond R
            assert np.all(np.abs(M.astype(F64) - E.astype(F64)) <= 4 * np.spacing(E).astype(F64)), (sigma, c)
            assert np.array_equal(M == 0, E == 0)


@pytest.mark.parametrize("rows,S,sigma,R", [(3, 16, 1.0, 3), (2, 40, 10.0, 30), (1, 136, 2.7, 8)], ids=lambda v: str(v))
def test_apply_is_its_own_adjoint_on_the_device(ops, rows, S, sigma, R):
    x, g = images(rows, S), images(rows, S, seed=7)
    st = state_of(sigma)
    bx, bg = ops.blur_apply(dev(x), st).cpu().numpy().astype(F64), ops.blur_apply(dev(g), st).cpu().numpy().astype(F64)
    a, b = np.sum(bx * g.astype(F64)), np.sum(x.astype(F64) * bg)
    tol = bound(R, np.abs(x).max()) * np.abs(g).sum() + bound(R, np.abs(g).max()) * np.abs(x).sum()
    print(f"<Blur x, g> {a:.9f}  <x, Blur g> {b:.9f}  bound {tol:.3e}")
    assert abs(a - b) <= tol


@pytest.mark.parametrize("S,sigma", [(16, 1.0), (40, 10.0), (136, 2.7)])
def test_row_slices_and_repeated_calls_are_bit_identical(ops, S, sigma):
    x = dev(images(5, S, seed=3))
    st = state_of(sigma)
    whole, again, part = ops.blur_apply(x, st), ops.blur_apply(x, st), ops.blur_apply(x[1:4], st)
    torch.cuda.synchronize()
    assert torch.equal(bits(whole), bits(again)) and torch.equal(bits(whole[1:4]), bits(part))


def test_state_follows_the_restatement_and_unusable_sigmas_copy(ops):
    from littlegan_amd import config
    from littlegan_amd._lib import LittleGanHipError
    st = config.blur_settings(2.7, 0.01)      # F = 10 images, n = 2: the fade ends at k = 5
    state = ops.blur_init(0)
    assert ops.blur_read(state) == (0, 0.0)
    for k in range(6):
        ops.blur_step(state, st["sigma0"], 2, st["fade_images"])
        k1, sigma = ops.blur_read(state)
        want = config.blur_restate(k, 2, st)[0]
        assert k1 == k + 1 and F32(sigma).view(np.int32) == want.view(np.int32), (k, sigma, want)
    assert sigma == 0.0 and torch.equal(state.view(torch.int32)[2:].cpu(), torch.zeros(2, dtype=torch.int32))
    top = (1 << 31) - 1
    ops.blur_init(top, out=state)
    ops.blur_step(state, 2.7, 2, 10)
    assert ops.blur_read(state) == (top, 0.0)      # k saturates, and sigma stays 0 that far past the fade
    x = dev(images(2, 24))
    for bad in (float("nan"), float("inf"), -1.0):
        assert torch.equal(bits(ops.blur_apply(x, state_of(bad))), bits(x)), bad
    box = ops.blur_apply(x, state_of(1e30)).cpu().numpy()
    assert np.isfinite(box).all() and np.abs(box.astype(F64) - blur_np(images(2, 24), 1e30)).max() <= bound(30, 1.0)      # the 61-tap box
    with pytest.raises(ValueError, match="3-channel"):
        ops.blur_apply(torch.zeros(2, 8, 8, 4, device="cuda"), state)
    with pytest.raises(ValueError, match="blur's state"):
        ops.blur_apply(x, torch.zeros(8, device="cuda"))
    with pytest.raises(LittleGanHipError, match="in-place"):
        ops.blur_apply(x, state, out=x)
    with pytest.raises(LittleGanHipError, match="image side"):
        ops.blur_apply(torch.zeros(1, 12, 12, 3, device="cuda"), state)


# ---------------------------------------------------------------------------------------------------------------------- whole steps
SIGMA0 = 1.0      # k = 0 of a 200-kimg fade: sigma = 1 exactly, R = 3


def build_blur(cfg, W, mfma, sigma0=SIGMA0, kimg=200, geom="", diff="", **kw):
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    args = make_args(cfg, mfma)
    args.blur_init_sigma, args.blur_fade_kimg, args.geom_augment, args.diff_augment = sigma0, kimg, geom, diff
    for k, v in kw.items():
        setattr(args, k, v)
    decoder, encoder = Decoder(args), Encoder(args)
    g = Generator(args, decoder)
    d = Discriminator(args, encoder)
    tr = EagerTrainer(args, g, d, Adjuster(args, d, g), None)
    load_weights(tr, W)
    return tr


class blur_np_oracle:
    """While active, oracle.np_oracle's discriminator forward reads T(Geo(Blur(image))) and its backward returns Blur(Geo^T(T^T(.))) of
    the image gradient: the restated Blur under `sigma`, and, with records, geom_augment / diff_augment under the next ones (the way
    geo_np_oracle of tests/test_geom_gpu.py wraps it)."""

    def __init__(self, sigma, recs=None):
        self.sigma, self.recs = sigma, recs

    def _fwd(self, cfg, Wd, image):
        image = blur_np(image, self.sigma)
        geo = par = None
        if self.recs is not None:
            geo, par = self.todo.pop(0)
            image = geom_np(image, geo)
            if par is not None:
                image = diffaug_np(image, par)
        out, cache = self.saved[0](cfg, Wd, image)
        return out, (cache, geo, par)

    def _bwd(self, cfg, Wd, cache, d_pr, d_c, need_wgrad=True, need_input_grad=False):
        inner, geo, par = cache
        grads, d_in = self.saved[1](cfg, Wd, inner, d_pr, d_c, need_wgrad=need_wgrad, need_input_grad=need_input_grad)
        if d_in is not None:
            if geo is not None:
                d_in = geom_adjoint_np(d_in if par is None else diffaug_adjoint_np(d_in, par), geo)
            d_in = blur_np(d_in, self.sigma)
        return grads, d_in

    def __enter__(self):
        self.saved = (O.discriminator_fwd, O.discriminator_bwd)
        self.todo = list(self.recs or [])
        O.discriminator_fwd, O.discriminator_bwd = self._fwd, self._bwd
        return self

    def __exit__(self, *exc):
        O.discriminator_fwd, O.discriminator_bwd = self.saved


_REF = {}


def step_reference(b, aug):
    """Computed once per (batch_no, with geom_augment + diff_augment) and shared, unchanged, by the f32 and bf16 tests: inputs, the
    float64 oracle under the restated blur, and the oracle without the blur."""
    if (b, aug) not in _REF:
        cfg = O.Cfg(**SMALL)
        W = perturbed(cfg, 1)
        inp = f32_round(O.make_inputs(cfg, cfg.batch_size, seed=50 + b))
        recs = step_records(*key_of(0, 0, 3), cfg.batch_size, 16 * cfg.init_dim, GEOM_FULL, DIFF_FULL) if aug else None
        with blur_np_oracle(SIGMA0, recs):
            ref = O.step_gradients(cfg, W, b, inp)
        if aug:
            with geo_np_oracle(recs):
                plain = O.step_gradients(cfg, W, b, inp)
        else:
            plain = O.step_gradients(cfg, W, b, inp)
        _REF[(b, aug)] = (cfg, W, inp, recs, ref, plain)
    return _REF[(b, aug)]


def step_inputs(inp, aug):
    return dict(dev_inputs(inp), diffaug_key=dev_key(0, 0, 3)) if aug else dev_inputs(inp)


@pytest.mark.parametrize("b", [1, 12], ids=["plain", "adjuster"])
@pytest.mark.parametrize("mfma", ["f32", "bf16"])
@pytest.mark.parametrize("aug", [False, True], ids=["blur", "blur+geom+diff"])
def test_step_matches_the_blurring_oracle(aug, mfma, b):
    """Without the feature the keys are ignored and the losses are those of the un-blurred oracle: this test fails there."""
    from littlegan_amd import config
    cfg, W, inp, recs, ref, plain = step_reference(b, aug)
    keys = ("gen_loss", "disc_loss") + (("adj_loss",) if b > 10 else ())
    tol = TOLS[mfma]
    # the blur matters at the bound that decides: some loss of the un-blurred oracle is more than five tolerances away
    assert max(abs(plain[k] - ref[k]) / abs(ref[k]) for k in keys) > 5 * (TOLS["f32"]["loss"] if mfma == "f32" else TOLS["bf16_emu"]["loss"])
    tr = build_blur(cfg, W, mfma, geom=GEOM_FULL if aug else "", diff=DIFF_FULL if aug else "")
    assert config.blur_restate(0, cfg.batch_size, tr.blur)[1] >= 2 and tr.blur_live()
    fake, adj, lg, ld, la = tr.train_step_from_inputs(b, step_inputs(inp, aug))
    torch.cuda.synchronize()
    print(f"{'blur+geom+diff' if aug else 'blur'} {mfma} b={b}: " + "; ".join(
        f"{k} {v.item():.6f} / oracle {ref[k]:.6f} / un-blurred {plain[k]:.6f}" for k, v in zip(keys, (lg, ld, la))))
    assert ops_read_sigma(tr) == (1, SIGMA0)
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
    check_grads(tr, ref, sets, tol, tag=f"blur {mfma} b={b}", only=only)
    if mfma == "bf16":   # the tight whole-step check of the bf16 path: the bf16-emulating oracle under the same blur and records
        with blur_np_oracle(SIGMA0, recs):
            check_emu(tr, cfg, W, b, inp, fake, adj, lg, ld, la, only=only)


def ops_read_sigma(tr):
    from littlegan_amd import ops as _ops
    return _ops.blur_read(tr.blur_state)


def test_key_off_is_the_step_without_the_key(ops, monkeypatch):
    """blur_init_sigma 0: bit-identical to a trainer built without the key, and no lgblur_ function is fetched from the library"""
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 1)
    inp = dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=5)))
    fetched = called(monkeypatch, ops)
    off, never = build_blur(cfg, W, "f32", sigma0=0.0), build(cfg, W, "f32")
    assert not hasattr(make_args(cfg, "f32"), "blur_init_sigma") and off.blur is None and not hasattr(off, "blur_state")
    for b in (1, 12):
        assert off.step_kind(b) == never.step_kind(b) and len(off.step_kind(b)) == 3
        ra, rb = off.train_step_from_inputs(b, inp), never.train_step_from_inputs(b, inp)
        torch.cuda.synchronize()
        assert all((u is None and v is None) or torch.equal(u, v) for u, v in zip(ra, rb)) and _same_state(off, never), b
    assert not blur_names(fetched), fetched
    build_blur(cfg, W, "f32").train_step_from_inputs(12, inp)
    torch.cuda.synchronize()
    names = blur_names(fetched)
    assert names[:2] == ["lgblur_init", "lgblur_step"] and names.count("lgblur_step") == 1
    assert names.count("lgblur_apply") == 4      # D's two inputs and the two image gradients


def copy_training_state(dst, src):
    dst.store.flat.copy_(src.store.flat)
    dst.store.m.copy_(src.store.m)
    dst.store.v.copy_(src.store.v)
    for m in "GDA":
        dst.opt_state[m].copy_(src.opt_state[m])
    dst.store.bump()


def test_fade_out_is_the_step_without_the_key(ops, monkeypatch):
    """F = 3 n: k = 0, 1, 2 blur (sigma 2, 4/3, 2/3), k = 3 has sigma 0.  From there on no lgblur_ name is fetched, the steps are those of
    a trainer without the key started from the same weights and Adam state, bit for bit, and D hands its maps to the Adjuster again."""
    from littlegan_amd import config
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 2)
    n = cfg.batch_size
    tr = build_blur(cfg, W, "bf16", sigma0=2.0, kimg=3 * n / 1000)
    assert tr.blur == {"sigma0": 2.0, "fade_images": 3 * n}
    assert [config.blur_restate(k, n, tr.blur)[1] for k in range(5)] == [6, 4, 2, 0, 0]
    kept = []
    fwd = tr.discriminator.forward_packed
    monkeypatch.setattr(tr.discriminator, "forward_packed", lambda *a, **k: (kept.append(k.get("keep_maps")), fwd(*a, **k))[1])
    data = lambda b: dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=300 + b)))
    for k, b in enumerate((9, 11, 12)):
        assert tr.blur_live() and len(tr.step_kind(b)) == 4 and tr.step_kind(b)[3] is True
        tr.train_step_from_inputs(b, data(b))
        assert ops.blur_read(tr.blur_state) == (k + 1, float(config.blur_restate(k, n, tr.blur)[0]))
    assert kept == [False, False, False, False, False] and not tr.blur_live()     # live: no maps kept, the Adjuster encodes `fake` itself
    never = build(cfg, W, "bf16")
    copy_training_state(never, tr)
    del kept[:]
    fetched = called(monkeypatch, ops)
    for b in (13, 14, 6):
        assert tr.step_kind(b) == never.step_kind(b) + (False,)
        ra, rb = tr.train_step_from_inputs(b, data(b)), never.train_step_from_inputs(b, data(b))
        torch.cuda.synchronize()
        assert all((u is None and v is None) or torch.equal(u, v) for u, v in zip(ra, rb)) and _same_state(tr, never), b
    assert not blur_names(fetched), fetched
    assert kept == [True, False, True, False, False]      # 13, 14: D keeps the maps of `fake` for the Adjuster; D on the Adjuster's output; 6
    assert tr._blur_k == 6 and ops.blur_read(tr.blur_state)[0] == 3      # the host mirror walks on; the device state rests
    assert tr.checkpoint_state()["blur_state"] == 6


def test_graph_replay_across_the_fade_is_bit_exact(ops):
    """graph_step against the eager path: F = 6 n, six live steps (two kinds: eager, captured + replayed, replayed — each replay under
    the sigma of ITS step), then six faded ones (two more kinds, none of which holds a blur launch)."""
    from littlegan_amd import config
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 5)
    n = cfg.batch_size
    kw = dict(sigma0=4.0, kimg=6 * n / 1000)
    tr_e, tr_g = build_blur(cfg, W, "bf16", **kw), build_blur(cfg, W, "bf16", **kw)
    sigmas = []
    for k, b in enumerate([7, 8, 9, 11, 12, 13, 14, 16, 17, 6, 7, 8]):
        inp = dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=400 + b)))
        fe, ae, lge, lde, lae = tr_e.train_step_from_inputs(b, inp)
        fg, ag, lgg, ldg, lag = tr_g.graph_step(b, inp)
        torch.cuda.synchronize()
        assert torch.equal(fe, fg) and torch.equal(lge, lgg) and torch.equal(lde, ldg), b
        assert (ae is None) == (ag is None) and (ae is None or (torch.equal(ae, ag) and torch.equal(lae, lag))), b
        assert _same_state(tr_e, tr_g), b
        assert ops.blur_read(tr_e.blur_state) == ops.blur_read(tr_g.blur_state)
        if k < 6:
            want = config.blur_restate(k, n, tr_g.blur)
            assert want[1] >= 2 and ops.blur_read(tr_g.blur_state) == (k + 1, float(want[0])), k
            sigmas.append(float(tr_g.blur_sigma_now()))
        assert tr_g._blur_k == k + 1 and tr_g.blur_live() == (k + 1 < 6)
    assert len(tr_g._graphs) == 4 and sorted(kd[3] for kd in tr_g._graphs) == [False, False, True, True]
    assert sigmas == sorted(sigmas, reverse=True) and len(set(sigmas)) == 6      # a new sigma every step, replays included
    assert ops.blur_read(tr_g.blur_state)[0] == 6


def test_checkpoint_resume_continues_the_fade(ops, tmp_path, capsys):
    """blur_state (the host's k) is part of the checkpoint: a restored trainer blurs the next step by the sigma the uninterrupted run
    uses and lands on the same bits; a checkpoint without the field starts the fade at k = 0 and says so."""
    from littlegan_amd import config
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    cfg = O.Cfg(init_dim=2, conv_filter=(32, 32, 32, 32, 32), cond_dim=3, noise_dim=5, batch_size=2)

    def mk(restore, sub, sigma0=3.0):
        args = make_args(cfg, "f32")
        args.no_io, args.result_dir, args.restore, args.exp_name, args.epoch = False, str(tmp_path / sub), restore, "t", 1
        args.blur_init_sigma, args.blur_fade_kimg = sigma0, 0.02      # F = 20 images, n = 2: ten steps
        dec, enc = Decoder(args), Encoder(args)
        g = Generator(args, dec)
        d = Discriminator(args, enc)
        return EagerTrainer(args, g, d, Adjuster(args, d, g), None)

    data = [dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=70 + b))) for b in range(4)]

    def step(tr, b, d):
        noise, new_image = tr.draw_step_inputs(d["real_image_1"])
        tr.train_step_from_inputs(b, dict(d, noise=noise, new_image=new_image))
        return ops.blur_read(tr.blur_state)

    tr = mk(False, "a")
    load_weights(tr, perturbed(cfg, 3))
    seen = [step(tr, 9 + b, data[b]) for b in range(3)]
    assert seen == [(k + 1, float(config.blur_restate(k, 2, tr.blur)[0])) for k in range(3)]
    tr.save_checkpoint("7")
    assert tr.checkpoint_state()["blur_state"] == 3
    s4 = step(tr, 12, data[3])
    want = tr.store.flat.clone()
    tr2 = mk(True, "a")   # restores in the constructor
    assert tr2._blur_k == 3 and ops.blur_read(tr2.blur_state) == (3, 0.0)
    assert step(tr2, 12, data[3]) == s4 == (4, float(config.blur_restate(3, 2, tr.blur)[0]))
    assert torch.equal(tr2.store.flat, want)
    # a checkpoint of a run without the key: the field is absent, and a blurring run that restores it starts at k = 0 with a line
    plain = mk(False, "b", sigma0=0.0)
    assert "blur_state" not in plain.checkpoint_state()
    plain.save_checkpoint("1")
    capsys.readouterr()
    tr3 = mk(True, "b")
    assert "no blur step counter" in capsys.readouterr().out and tr3._blur_k == 0 and ops.blur_read(tr3.blur_state) == (0, 0.0)
    # ... and the other way round the counter is ignored, with a line; a counter that is none is refused before anything is loaded
    mk(True, "a", sigma0=0.0)
    assert "does not blur" in capsys.readouterr().out
    ck = torch.load(tr.latest_checkpoint(), weights_only=True)
    ck["blur_state"] = -1
    torch.save(ck, str(tmp_path / "bad.pt"))
    w0 = tr3.store.flat.clone()
    with pytest.raises(ValueError, match="blur_state"):
        tr3.load_checkpoint(str(tmp_path / "bad.pt"))
    assert torch.equal(tr3.store.flat, w0)


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_r1_penalty_step_under_blur(ops, mfma):
    """The penalty under live blur is taken on Blur(new_image), with respect to it (DESIGN.md §24's rule): the reference is the blurring
    oracle plus np_r1 of tests/test_r1_gpu.py on the device's own Blur(new_image), read back."""
    from test_r1_gpu import GAMMA, _with_r1
    tol = TOLS[mfma]
    b = 1
    cfg, W, inp, _, ref, _ = step_reference(b, False)
    tr = build_blur(cfg, W, mfma, r1_gamma=GAMMA, r1_interval=1)
    di = dev_inputs(inp)
    fake, adj, lg, ld, la = tr.train_step_from_inputs(b, di)
    x_blur = ops.blur_apply(di["new_image"], tr.blur_state)
    torch.cuda.synchronize()
    assert not torch.equal(x_blur, di["new_image"])
    ref2, term = _with_r1(ref, cfg, W, x_blur.cpu().double().numpy(), GAMMA)
    _, term_plain = _with_r1(ref, cfg, W, inp["new_image"], GAMMA)
    want = ref["disc_loss"] + term
    print(f"{mfma}: disc {ld.item():.7g} / {want:.7g}, r1 {float(tr.losses['r1']):.7g} / {term:.7g} (on the un-blurred rows {term_plain:.7g})")
    assert abs(term_plain - term) > 5 * max(tol["loss"], 1e-4) * abs(term)      # the blurred rows are what decides
    assert abs(lg.item() - ref["gen_loss"]) < tol["loss"] * abs(ref["gen_loss"])
    assert abs(ld.item() - want) < tol["loss"] * abs(want)
    assert abs(float(tr.losses["r1"]) - term) < max(tol["loss"], 1e-4) * abs(term) + 1e-7
    check_grads(tr, ref2, [("D", "dD"), ("G", "dG")], tol, tag=f"r1 blur {mfma}", only={m: O.train_weight_indices(cfg, m, b) for m in "GDA"})
