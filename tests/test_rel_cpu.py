"""Relativistic pairing and the R2 penalty (relativistic / r2_gamma) without a GPU: the float64 restatement that
tests/test_rel_gpu.py holds the device to (the autograd gradient of "relativistic terms minus the kind's §25 terms", per tape, composed
with tests/test_gan_loss_cpu.py::step_reference, anchored against a direct torch restatement of the whole step; R1 + R2 by one double
backward over 2B rows against two tests/test_r1_cpu.py::torch_r1 calls); the names of the header include/littlegan_rel.h
(its types, exports, binding and guard-band rows are tests/test_abi.py's and the ledger's); every host-side refusal of its entry points; the configuration keys and the trainer's refusals; and the data of
the exact-arithmetic kernel cases with the conditions under which "bit for bit" is a fair demand.

The definition (this project's): f0 = the D-real function of the kind — logistic softplus(-t), hinge max(0, 1 - t), lsgan (t - 1)^2 / 2;
  disc  mean_b f0(z_r[b] - z_f[b])        gen  mean_b f0(z_f[b] - z_r[b]), z_r constant        adj  mean_i f0(z_a[i] - z_r[i mod B])"""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import np_oracle as O  # noqa: E402
from oracle import torch_oracle as TO  # noqa: E402
from test_abi import ROOT, _protos  # noqa: E402
from test_diffaug_cpu import _cpu_trainer, diffaug_torch  # noqa: E402
from test_gan_loss_cpu import (ROLE_D_FAKE, ROLE_D_REAL, ROLE_G, _logit, _np_grads, _t64, _tiny_step, np_term, step_reference, term,  # noqa: E402
                               with_objective)
from test_gp_cpu import _tiny_case  # noqa: E402
from test_r1_cpu import ZERO_GRADS, np_r1, torch_r1  # noqa: E402

REL_HEADER = os.path.join(ROOT, "include", "littlegan_rel.h")
ENTRY_POINTS = ("lgrel_pair_heads_loss_fwd_bwd", "lgrel_r12_workspace_bytes", "lgrel_r12_seed")
REL_KINDS = ("logistic", "hinge", "lsgan")          # kind 1..3, in this order
KIND_NO = {k: i + 1 for i, k in enumerate(REL_KINDS)}
SIDE_SELF, SIDE_OTHER = 0, 1
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# the pairing in float64
def pair_term(kind, t):
    """mean over the pairs of f0(t): the kind's D-real function (tests/test_gan_loss_cpu.py::term at role 0) on the difference"""
    assert kind in REL_KINDS, kind
    return term(kind, ROLE_D_REAL, t)


def np_pair_term(kind, t):
    """-> (f0(t), f0'(t)) elementwise in float64; the subgradient at hinge's kink t == 1 is 0"""
    assert kind in REL_KINDS, kind
    return np_term(kind, ROLE_D_REAL, t)


def relativistic_delta(cfg, W, b, inp, kind, detach_real=True, recs=None):
    """The float64 autograd gradient of (relativistic terms - the kind's §25 terms), per tape, and the same difference of the losses:
    what turns test_gan_loss_cpu.step_reference(kind) into the relativistic step.  detach_real=False leaves z_r attached on the gen
    and adj tapes (it depends on none of their weights: the result must not change).  recs: the three record sets of D's calls under
    diff_augment (D reads T(image)), as test_gan_loss_cpu.objective_delta takes them."""
    net = TO.Net(cfg, W)
    t = _t64({k: v for k, v in inp.items() if k != "gp_eps"})
    T = (lambda img, i: img) if recs is None else (lambda img, i: diffaug_torch(img, recs[i]))
    fake = net.generator(t["noise"], t["real_cond_2"])
    z_r, z_f = _logit(net, T(t["new_image"], 0)), _logit(net, T(fake, 1))
    z_rc = z_r.detach() if detach_real else z_r
    d_disc = pair_term(kind, z_r - z_f) - (term(kind, ROLE_D_REAL, z_r) + term(kind, ROLE_D_FAKE, z_f))
    d_gen = pair_term(kind, z_f - z_rc) - term(kind, ROLE_G, z_f)
    out = dict(disc_loss=float(d_disc.detach()), gen_loss=float(d_gen.detach()), adj_loss=None, dA=None,
               dD=_np_grads(torch.autograd.grad(d_disc, net.W["D"], retain_graph=True, allow_unused=True), net.W["D"]),
               dG=_np_grads(torch.autograd.grad(d_gen, net.W["G"], retain_graph=True, allow_unused=True), net.W["G"]))
    if cfg.train_adj and b > 10:
        c1, c2 = t["real_cond_1"], t["real_cond_2"]
        adj_img = net.adjuster(torch.cat([t["real_image_1"], fake.detach()], 0), (torch.cat([c2, c1], 0) + 1.0) * 0.5)
        z_a = _logit(net, T(adj_img, 2))
        d_adj = pair_term(kind, z_a - torch.cat([z_rc, z_rc], 0)) - term(kind, ROLE_G, z_a)
        out.update(adj_loss=float(d_adj.detach()), dA=_np_grads(torch.autograd.grad(d_adj, net.W["A"], allow_unused=True), net.W["A"]))
    return out


def rel_step_reference(cfg, W, b, inp, kind):
    """the whole relativistic step: np_oracle.step_gradients + objective_delta(kind) + relativistic_delta(kind)"""
    return with_objective(step_reference(cfg, W, b, inp, kind), relativistic_delta(cfg, W, b, inp, kind))


def torch_rel_step(cfg, W, b, inp, kind):
    """tests/test_gan_loss_cpu.py::torch_step under relativistic pairing, directly: the whole step in torch float64"""
    net = TO.Net(cfg, W)
    t = _t64(inp)
    img1, c1, img2, c2 = t["real_image_1"], t["real_cond_1"], t["real_image_2"], t["real_cond_2"]
    Wd = net.W["D"]

    def disc(image):
        x = net.encoder(image)[-1].reshape(image.shape[0], -1)
        return (x @ Wd[16] + Wd[17]), torch.sigmoid(x @ Wd[18] + Wd[19])

    fake = net.generator(t["noise"], c2)
    z_r, real_c = disc(t["new_image"])
    z_f, fake_c = disc(fake)
    disc_loss = 2.0 * TO.bce_mean(c1, real_c) + pair_term(kind, z_r - z_f)
    gen_loss = pair_term(kind, z_f - z_r.detach()) + TO.bce_mean(c2, fake_c) + cfg.l1_lambda * (img2 - fake).abs().mean()
    out = dict(disc_loss=float(disc_loss.detach()), gen_loss=float(gen_loss.detach()), adj_loss=None, dA=None,
               dD=_np_grads(torch.autograd.grad(disc_loss, Wd, retain_graph=True), Wd),
               dG=_np_grads(torch.autograd.grad(gen_loss, net.W["G"]), net.W["G"]))
    if cfg.train_adj and b > 10:
        t_cond = torch.cat([c2, c1], 0)
        adj_img = net.adjuster(torch.cat([img1, fake.detach()], 0), (t_cond + 1.0) * 0.5)
        z_a, adj_c = disc(adj_img)
        zr2 = torch.cat([z_r, z_r], 0).detach()
        adj_loss = pair_term(kind, z_a - zr2) + TO.bce_mean(t_cond, adj_c) + cfg.l1_lambda * (torch.cat([img2, img1], 0) - adj_img).abs().mean()
        out.update(adj_loss=float(adj_loss.detach()), dA=_np_grads(torch.autograd.grad(adj_loss, net.W["A"]), net.W["A"]))
    return out


def torch_r12(cfg, Wd, x_all, w_real, w_fake):
    """R1 + R2 by ONE autograd double backward over the 2B rows D read: -> (term_real, term_fake, r2 [2B], 20 gradients), float64"""
    net = TO.Net(cfg, {"D": Wd})
    x = torch.tensor(np.asarray(x_all, np.float64), requires_grad=True)
    B = x.shape[0] // 2
    g, = torch.autograd.grad(_logit(net, x).sum(), x, create_graph=True)
    r2 = (g.flatten(1) ** 2).sum(1)
    t_real, t_fake = 0.5 * w_real * r2[:B].mean(), 0.5 * w_fake * r2[B:].mean()
    dD = torch.autograd.grad(t_real + t_fake, net.W["D"], allow_unused=True)
    return float(t_real.detach()), float(t_fake.detach()), r2.detach().numpy(), _np_grads(dD, net.W["D"])


# ---------------------------------------------------------------------------------------------------------------------
# the step reference, anchored
def _close_grads(ref, direct, keys):
    for key in keys:
        gmax = max(np.abs(e).max() for e in direct[key])
        for i, (got, exp) in enumerate(zip(ref[key], direct[key])):
            scale = max(np.abs(exp).max(), 1e-30) if exp.size > 1 else gmax     # (as tests/test_gan_loss_cpu.py: a 1-element gradient may cancel)
            assert np.abs(np.asarray(got).ravel() - exp.ravel()).max() <= 1e-10 * scale + 1e-18, (key, i, scale)


@pytest.mark.parametrize("b", [4, 5, 11], ids=["full", "partition", "adjuster"])
@pytest.mark.parametrize("kind", REL_KINDS)
def test_composition_equals_the_direct_restatement(kind, b):
    cfg, W, inp = _tiny_step(b)
    ref, direct = rel_step_reference(cfg, W, b, inp, kind), torch_rel_step(cfg, W, b, inp, kind)
    plain = step_reference(cfg, W, b, inp, kind)
    keys = ("disc_loss", "gen_loss") + (("adj_loss",) if b > 10 else ())
    for k in keys:
        assert abs(ref[k] - direct[k]) <= 1e-12 * max(1.0, abs(direct[k])), (k, ref[k], direct[k])
    assert max(abs(plain[k] - direct[k]) for k in keys) > 1e-3      # the pairing is not the kind's own objective
    _close_grads(ref, direct, ("dD", "dG") + (("dA",) if b > 10 else ()))
    assert ref["dA"] is None or len(ref["dA"]) == 4


@pytest.mark.parametrize("kind", REL_KINDS)
def test_gen_and_adj_tapes_get_nothing_through_the_real_logit(kind):
    """z_r depends on none of the weights the gen and adj tapes differentiate: attached or detached, their gradients are the same"""
    cfg, W, inp = _tiny_step(11)
    a, d = relativistic_delta(cfg, W, 11, inp, kind, detach_real=False), relativistic_delta(cfg, W, 11, inp, kind)
    for key in ("dG", "dA"):
        assert all(np.array_equal(x, y) for x, y in zip(a[key], d[key])), key
    # (hinge: where every pair sits below the kink, f0'(z_f - z_r) = -1 is the derivative of §25's -z_f and the difference is zero)
    assert kind == "hinge" or (any(np.any(g) for g in d["dG"]) and any(np.any(g) for g in d["dA"]))


def test_pair_terms_against_their_definition():
    t = np.linspace(-8, 8, 65)
    for kind, f0 in (("logistic", lambda v: np.log1p(np.exp(-v))), ("hinge", lambda v: np.maximum(0, 1 - v)), ("lsgan", lambda v: 0.5 * (v - 1) ** 2)):
        f, g = np_pair_term(kind, t)
        assert np.abs(f - f0(t)).max() < 1e-12
        num = (f0(t + 1e-6) - f0(t - 1e-6)) / 2e-6
        away = np.abs(t - 1) > 1e-3 if kind == "hinge" else np.ones_like(t, bool)
        assert np.abs(g - num)[away].max() < 1e-6
        assert abs(float(pair_term(kind, torch.tensor(t))) - f.mean()) < 1e-12
    assert np_pair_term("hinge", np.array([1.0]))[1][0] == 0.0
    # f0 of a wgan difference would be wgan itself: it is no kind of the pairing
    with pytest.raises(AssertionError):
        np_pair_term("wgan", t)


def test_r1_plus_r2_in_one_double_backward_is_the_sum_of_two():
    cfg, Wd, x = _tiny_case(3)
    rng = np.random.default_rng(31)
    x_all = np.concatenate([x, rng.uniform(-1, 1, x.shape)], 0)
    B = x.shape[0]
    w1, w2 = 160.0, 48.0
    t1, t2, r2, grads = torch_r12(cfg, Wd, x_all, w1, w2)
    (a_t, a_r2, a_g), (b_t, b_r2, b_g) = torch_r1(cfg, Wd, x_all[:B], w1), torch_r1(cfg, Wd, x_all[B:], w2)
    assert abs(t1 - a_t) <= 1e-12 * a_t and abs(t2 - b_t) <= 1e-12 * b_t and t1 > 0 and t2 > 0
    assert np.abs(r2 - np.concatenate([a_r2, b_r2])).max() <= 1e-12 * np.abs(r2).max()
    for i, (g, ga, gb) in enumerate(zip(grads, a_g, b_g)):
        exp = ga + gb
        assert np.abs(g - exp).max() <= 1e-10 * max(np.abs(exp).max(), 1e-30) + 1e-18, i
        assert bool(np.any(g)) == (i not in ZERO_GRADS), i
    # R2 is the restated R1 (tests/test_r1_cpu.py::np_r1) on the fake rows
    n_t, n_r2, n_g = np_r1(cfg, Wd, x_all[B:], w2)
    assert abs(n_t - t2) <= 1e-12 * t2 and np.abs(n_r2 - r2[B:]).max() <= 1e-12 * np.abs(r2).max()
    assert all(np.abs(g - gb).max() <= 1e-10 * max(np.abs(gb).max(), 1e-30) + 1e-18 for g, gb in zip(n_g, b_g))
    # w_fake == 0 is R1 alone
    _, t0, _, g0 = torch_r12(cfg, Wd, x_all, w1, 0.0)
    assert t0 == 0.0 and all(np.abs(g - ga).max() <= 1e-10 * max(np.abs(ga).max(), 1e-30) + 1e-18 for g, ga in zip(g0, a_g))


# ---------------------------------------------------------------------------------------------------------------------
# the header include/littlegan_rel.h
@pytest.fixture(scope="module")
def lib():
    from littlegan_amd.csrc.build import build
    build(verbose=False)
    from littlegan_amd import _lib
    return _lib


def test_rel_header_declares_the_entry_points(lib):
    assert set(_protos(REL_HEADER)) == set(ENTRY_POINTS) == {n for n in lib.SIGNATURES if n.startswith("lgrel_")}


def test_the_sources_include_the_header_and_are_built():
    from littlegan_amd.csrc import build as B
    for name in ("objective.hip", "r1.hip"):
        assert "littlegan_rel.h" in open(os.path.join(ROOT, "littlegan_amd", "csrc", name)).read() and name in B.SOURCES


def test_the_shared_device_code_has_one_definition():
    """the kernels sit beside the code they share (gan_term in objective.hip, the seed's pass in r1.hip): ONE definition, two call sites"""
    obj = open(os.path.join(ROOT, "littlegan_amd", "csrc", "objective.hip")).read()
    assert len(re.findall(r"\bvoid gan_term\(", obj)) == 1 and len(re.findall(r"\bgan_term\(kind, LGO_ROLE_D_REAL,", obj)) == 2
    r1 = open(os.path.join(ROOT, "littlegan_amd", "csrc", "r1.hip")).read()
    assert len(re.findall(r"\bvoid r1_seed_kernel\(", r1)) == 1 and len(re.findall(r"hipLaunchKernelGGL\(r1_seed_kernel,", r1)) == 2


def test_argument_validation_without_gpu(lib):
    """every refusal happens on the host, before any launch: the pointers are never dereferenced (there is no device here)"""
    h = lib.load()
    err = lambda: h.lg_last_error()
    pair = h.lgrel_pair_heads_loss_fwd_bwd   # (p, z, z_ref, t_c, kind, side, w_pr, w_c, loss, dz, n, m, c, accumulate, stream)
    who = b"lgrel_pair_heads_loss_fwd_bwd"
    p, z, zr, tc, ls, dz = (C.c_void_p(256 * (i + 1)) for i in range(6))

    def call(p=p, z=z, zr=zr, tc=tc, kind=2, side=0, w_pr=1.0, w_c=1.0, ls=ls, dz=dz, n=4, m=4, c=5):
        return pair(p, z, zr, tc, kind, side, w_pr, w_c, ls, dz, n, m, c, 0, None)

    for kw in (dict(p=None), dict(z=None), dict(zr=None), dict(ls=None), dict(dz=None)):
        assert call(**kw) == -1 and b"null pointer" in err() and who in err(), kw
    for kw in (dict(p=C.c_void_p(258)), dict(z=C.c_void_p(513)), dict(zr=C.c_void_p(770)), dict(tc=C.c_void_p(1027)),
               dict(ls=C.c_void_p(1281)), dict(dz=C.c_void_p(1538))):
        assert call(**kw) == -1 and b"aligned" in err() and who in err(), kw
    for kind in (0, 4, 5, -1, 1 << 20):
        assert call(kind=kind) == -1 and b"bad kind" in err() and who in err(), kind
    for side in (-1, 2, 1 << 20):
        assert call(side=side) == -1 and b"bad side" in err() and who in err(), side
    for n, c in ((0, 5), (-3, 5), (4, 0), (4, -1), (1 << 30, 40)):
        assert call(n=n, m=1 if n > 0 else 4, c=c) == -1 and b"bad shape" in err() and who in err(), (n, c)
    for n, m in ((4, 3), (4, 8), (6, 4), (4, 0), (4, -2)):
        assert call(n=n, m=m) == -1 and b"multiple of m" in err() and who in err(), (n, m)
    assert call(tc=None) == -1 and b"t_c is null" in err() and who in err()
    for w in (float("nan"), float("inf"), float("-inf")):
        assert call(w_pr=w) == -1 and b"finite" in err() and who in err(), w
        assert call(w_c=w) == -1 and b"finite" in err() and who in err(), w
    seed = h.lgrel_r12_seed       # (g, u0, r2, loss, r1_loss, r2_loss, w_real, w_fake, workspace, ws_bytes, B, L, stream)
    who = b"lgrel_r12_seed"
    d, d2, d3, dw = C.c_void_p(64), C.c_void_p(128), C.c_void_p(256), C.c_void_p(512)
    ws = h.lgrel_r12_workspace_bytes(4, 8192)
    for args in ((None, d2, d3), (d, None, d3), (d, d2, None)):
        assert seed(*args, None, None, None, 4.0, 2.0, dw, ws, 4, 8192, None) == -1 and b"null pointer" in err() and who in err()
    assert seed(d, d2, d3, None, None, None, 4.0, 2.0, None, ws, 4, 8192, None) == -1 and b"null pointer" in err() and who in err()
    for args in ((C.c_void_p(68), d2, d3, None, None, None, dw), (d, C.c_void_p(136), d3, None, None, None, dw), (d, d2, C.c_void_p(258), None, None, None, dw),
                 (d, d2, d3, C.c_void_p(1025), None, None, dw), (d, d2, d3, None, C.c_void_p(1026), None, dw), (d, d2, d3, None, None, C.c_void_p(1027), dw),
                 (d, d2, d3, None, None, None, C.c_void_p(516))):
        assert seed(*args[:6], 4.0, 2.0, args[6], ws, 4, 8192, None) == -1 and b"aligned" in err() and who in err(), args
    for B, L in ((4, 8190), (4, 8191), (0, 8192), (-1, 8192), (4, 0), (4, -4), (32768, 131072), (1, 1 << 33), (3, 1 << 40)):
        assert seed(d, d2, d3, None, None, None, 4.0, 2.0, dw, 1 << 40, B, L, None) == -1 and b"bad shape" in err() and who in err(), (B, L)
    assert 2 * 32768 * (131072 // 4) == 1 << 31
    assert seed(d, d2, d3, None, None, None, 4.0, 2.0, dw, ws - 1, 4, 8192, None) == -1 and b"workspace too small" in err() and who in err()
    for w in (float("nan"), -1.0, float("inf"), float("-inf"), -1e-30):
        assert seed(d, d2, d3, None, None, None, w, 2.0, dw, ws, 4, 8192, None) == -1 and b"weights" in err() and who in err(), w
        assert seed(d, d2, d3, None, None, None, 4.0, w, dw, ws, 4, 8192, None) == -1 and b"weights" in err() and who in err(), w


def test_workspace_bytes(lib):
    h = lib.load()
    fn = h.lgrel_r12_workspace_bytes
    for s in [(1, 4), (4, 4100), (8, 49152), (512, 64), (128, 49152)]:
        assert fn(*s) > 0 and fn(*s) == fn(*s), s
        # the partials of 2B rows: never less than the two halves' own (each rounded up to 256 bytes on its own)
        assert 2 * s[0] * ((s[1] + 4095) // 4096) * 8 <= fn(*s) <= 2 * h.lgr_r1_workspace_bytes(*s), s
    for s in [(0, 64), (-1, 64), (4, 0), (4, -4)]:
        assert fn(*s) == 0, s
    assert fn(128, 49152) == 2 * 128 * 12 * 8 == h.lgr_r1_workspace_bytes(256, 49152)


# ---------------------------------------------------------------------------------------------------------------------
# configuration and trainer
def test_config_keys_default_to_off(tmp_path):
    from littlegan_amd import config
    d = config.DEFAULTS
    assert d["relativistic"] is False and d["r2_gamma"] == 0.0
    assert "relativistic" in config.__doc__ and "r2_gamma" in config.__doc__
    assert set(config.GAN_LOSS_KINDS) == {"bce", "logistic", "hinge", "lsgan", "wgan"}     # pairing is a key of its own, no sixth kind
    a = config.Arg(["train", "x"], config_dir=str(tmp_path))
    assert a.relativistic is False and a.r2_gamma == 0.0
    (tmp_path / "r.config.json").write_text('{"gan_loss": "logistic", "relativistic": true, "r1_gamma": 10, "r2_gamma": 5, "r1_interval": 4}')
    a = config.Arg(["train", "x", "-e", "r"], config_dir=str(tmp_path))
    assert (a.gan_loss, a.relativistic, a.r1_gamma, a.r2_gamma, a.r1_interval) == ("logistic", True, 10, 5, 4)
    assert config.r2_settings() is None and config.r2_settings(0.0, 16) is None and config.r2_settings(0, 1) is None
    assert config.r2_settings(10.0, 16) == {"gamma": 10.0, "interval": 16, "weight": 160.0}
    assert config.r2_settings(0.5, 1) == {"gamma": 0.5, "interval": 1, "weight": 0.5}
    assert config.relativistic_setting() is False and config.relativistic_setting(False, "bce") is False
    assert all(config.relativistic_setting(True, k) is True for k in REL_KINDS)


BAD = [("r2_gamma", -1.0), ("r2_gamma", float("nan")), ("r2_gamma", float("inf")), ("r2_gamma", True), ("r2_gamma", "10"),
       ("r2_gamma", None), ("r2_gamma", [1.0]), ("relativistic", 1), ("relativistic", "true"), ("relativistic", None), ("relativistic", 0.0)]


@pytest.mark.parametrize("key,value", BAD, ids=lambda v: str(v))
def test_a_bad_value_raises(tmp_path, key, value):
    from littlegan_amd import config
    fn = config.r2_settings if key == "r2_gamma" else (lambda relativistic: config.relativistic_setting(relativistic, "hinge"))
    with pytest.raises(ValueError, match=key):
        fn(**{key: value})
    (tmp_path / "bad.config.json").write_text(json.dumps({"gan_loss": "hinge", key: value}))
    with pytest.raises(ValueError, match=key):
        config.Arg(["train", "x", "-e", "bad"], config_dir=str(tmp_path))
    with pytest.raises(ValueError, match=key):
        _cpu_trainer(gan_loss="hinge", **{key: value})


def test_relativistic_needs_a_pairable_objective(tmp_path):
    from littlegan_amd import config
    for kw, why in ((dict(), "no logit"), (dict(gan_loss="bce"), "no logit"), (dict(gan_loss="wgan", use_gp=True), "wgan objective itself")):
        with pytest.raises(ValueError, match=why):
            config.relativistic_setting(True, kw.get("gan_loss", "bce"))
        (tmp_path / "bad.config.json").write_text(json.dumps(dict(kw, relativistic=True)))
        with pytest.raises(ValueError, match=why):
            config.Arg(["train", "x", "-e", "bad"], config_dir=str(tmp_path))
        with pytest.raises(ValueError, match=why):
            _cpu_trainer(relativistic=True, **kw)


def test_trainer_refusals_and_allowed_combinations():
    base, _ = _cpu_trainer()
    assert base.relativistic is False and base.r2 is None and "r2" not in base.losses
    assert not any(base.r2_step(b) for b in range(40))
    for kw, why in ((dict(), "r2_gamma and use_gp"), (dict(r1_gamma=10.0), "r1_gamma and use_gp")):    # (R1's own refusal comes first)
        with pytest.raises(ValueError, match=why):
            _cpu_trainer(r2_gamma=5.0, use_gp=True, **kw)
    with pytest.raises(ValueError, match="r2_gamma and dropout_train"):
        _cpu_trainer(r2_gamma=5.0, dropout_train=True, dropout_rate=0.25)
    zero, _ = _cpu_trainer(r2_gamma=0, relativistic=False)
    assert zero.r2 is None and [zero.step_kind(b) for b in range(40)] == [base.step_kind(b) for b in range(40)]
    for name in REL_KINDS:
        tr, _ = _cpu_trainer(gan_loss=name, relativistic=True)
        assert tr.relativistic is True and tr.gan_kind == KIND_NO[name] and set(tr.losses) == set(base.losses)
        assert [tr.step_kind(b) for b in range(40)] == [base.step_kind(b) for b in range(40)]      # launch-count neutral: no new kind
        assert "relativistic" not in "".join(tr.checkpoint_state())
    # the penalty on the logit does not read the objective: use_gp is allowed, and so is everything a logit-side gan_loss goes with
    tr, _ = _cpu_trainer(gan_loss="logistic", relativistic=True, use_gp=True)
    assert tr.relativistic and tr.use_gp and "gp" in tr.losses
    tr, _ = _cpu_trainer(gan_loss="hinge", relativistic=True, dropout_train=True, dropout_rate=0.25)
    assert tr.relativistic and tr.dropout
    # the recipe; R2 follows R1's schedule, the third element of step_kind means "a penalty step" for either
    tr, _ = _cpu_trainer(gan_loss="logistic", relativistic=True, r1_gamma=10.0, r2_gamma=5.0, r1_interval=4, diff_augment="color,cutout", ema_decay=0.99)
    assert tr.r1["weight"] == 40.0 and tr.r2 == {"gamma": 5.0, "interval": 4, "weight": 20.0}
    assert tuple(tr.losses["r1"].shape) == tuple(tr.losses["r2"].shape) == (1,)
    assert [b for b in range(1, 20) if tr.r2_step(b)] == [b for b in range(1, 20) if tr.r1_step(b)] == [4, 8, 12, 16]
    alone, _ = _cpu_trainer(r2_gamma=5.0, r1_interval=4)          # R2 alone, under the reference's objective
    assert alone.r1 is None and alone.r2["weight"] == 20.0 and "r1" not in alone.losses and "r2" in alone.losses
    for t in (tr, alone):
        assert all(t.step_kind(b)[2] == (b % 4 == 0) and t.step_kind(b)[:2] == base.step_kind(b)[:2] for b in range(1, 40))
        assert "r2" not in "".join(t.checkpoint_state())   # stateless: no checkpoint field


# ---------------------------------------------------------------------------------------------------------------------
# the exact-arithmetic kernel cases of tests/test_rel_gpu.py: data, expected results, and why "bit for bit" is fair
EXACT_KINDS = ("hinge", "lsgan")
EXACT_SHAPES = [(1, 1, 1), (512, 512, 40), (1024, 512, 40)]     # (n, m, c): one busy thread; 21 trips; 41 trips with every z_ref read twice
EXACT_W_PR, EXACT_LOSS0 = 2.0, 3.0


def exact_pair_data(n, m, side):
    """-> (z ints [n], z_ref ints [m]) in quarter units, in [-16, 16], with t == 1 planted at pairs 0 and 1 (every row of the pair)"""
    rng = np.random.default_rng(7000 + 5 * n + 3 * m + side)
    zi, ri = rng.integers(-16, 17, size=n), rng.integers(-16, 17, size=m)
    for j, v in ((0, 3), (1, -5)):
        if j < m:
            ri[j] = v
            zi[j::m] = v + 4 if side == SIDE_SELF else v - 4
    return zi, ri


def exact_pair_case(kind, side, n, m):
    """-> (z fp32, z_ref fp32, expected dz[:, 0] fp32, the term column 0 adds to the loss fp32 (0 for OTHER)), each exact"""
    zi, ri = exact_pair_data(n, m, side)
    ref = ri[np.arange(n) % m]
    t = (zi - ref) * 0.25 if side == SIDE_SELF else (ref - zi) * 0.25
    f, g = np_pair_term(kind, t)
    s = EXACT_W_PR / n
    if side == SIDE_SELF:
        return (zi * 0.25).astype(F32), (ri * 0.25).astype(F32), (s * g).astype(F32), F32(s * f.sum())
    return (zi * 0.25).astype(F32), (ri * 0.25).astype(F32), (-(s * g)).astype(F32), F32(0.0)


def test_conditions_of_the_exact_cases():
    assert np.frexp(EXACT_W_PR)[0] == 0.5
    for n, m, c in EXACT_SHAPES:
        assert n & (n - 1) == 0 and n % m == 0 and n * (c + 1) <= 1024 * 41
        s = EXACT_W_PR / n
        assert np.frexp(s)[0] == 0.5 and float(F32(s)) == s          # a power of two: the scale rounds nothing
        for side in (SIDE_SELF, SIDE_OTHER):
            zi, ri = exact_pair_data(n, m, side)
            assert np.abs(zi).max() <= 16 and np.abs(ri).max() <= 16
            ref = ri[np.arange(n) % m]
            t = (zi - ref) * 0.25 if side == SIDE_SELF else (ref - zi) * 0.25
            assert np.abs(t).max() <= 8 and t[0] == 1.0 and (m < 2 or np.all(t[1::m] == 1.0)) and np.all(t[0::m] == 1.0)
            for kind in EXACT_KINDS:
                z, zr, dz, term_ = exact_pair_case(kind, side, n, m)
                assert np.array_equal(z.astype(np.float64), zi * 0.25) and np.array_equal(zr.astype(np.float64), ri * 0.25)
                # the difference of two multiples of 2^-2 below 2^3 is exact in fp32
                assert np.array_equal((z - zr[np.arange(n) % m]).astype(np.float64), (zi - ref) * 0.25)
                f, g = np_pair_term(kind, t)
                # every summand s f0(t) is an integer multiple of u = s / 32 ((t - 1)^2 / 2 has 5 fractional bits), and the magnitudes sum
                # below 2^24 u together with the loss accumulated onto: every fp32 partial sum, in any order, is exact
                u = s / 32.0
                units = s * f / u
                assert np.array_equal(units, np.round(units)) and np.abs(units).sum() + EXACT_LOSS0 / u < 2 ** 24
                assert EXACT_LOSS0 / u == round(EXACT_LOSS0 / u)
                if side == SIDE_SELF:
                    assert float(term_) == float((s * f).sum()) and float(F32(EXACT_LOSS0 + float(term_))) == EXACT_LOSS0 + float((s * f).sum())
                else:
                    assert float(term_) == 0.0
                sign = 1.0 if side == SIDE_SELF else -1.0
                assert np.array_equal(dz.astype(np.float64), sign * s * g)
                if kind == "hinge":
                    assert dz[0] == 0 and f[0] == 0 and (m < 2 or (dz[1] == 0 and f[1] == 0))      # the kink: subgradient 0
                    assert np.any(dz != 0) or n == 1
                else:
                    assert dz[0] == 0 and f[0] == 0                                               # lsgan's minimum sits at the same t
