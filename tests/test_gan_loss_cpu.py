"""Logit-side GAN objectives (gan_loss) without a GPU: the entry points of include/littlegan_hip_obj.h (the names, the kind
numbers, validating before any launch: the whole ABI is held to its table and its ledger by tests/test_abi.py and
tests/test_guards_cpu.py); the configuration key and the trainer's refusals; the float64 step reference of tests/test_gan_loss_gpu.py
(oracle.np_oracle.step_gradients plus the autograd gradient of "new real / fake terms minus the BCE ones", per tape) anchored against a
direct torch restatement of the whole step under each objective; the logit-side gradient penalty by torch double backward; and the data
of the exact-arithmetic kernel cases with the conditions under which "bit for bit" is a fair demand.

The objectives are this project's definition (the reference has only the first row), z = the pre-sigmoid value of output_pr:
  kind       D on real rows    D on fake rows    G / Adjuster
  bce        BCE(.98, s(z))    BCE(.02, s(z))    BCE(.98, s(z))
  logistic   softplus(-z)      softplus(z)       softplus(-z)
  hinge      max(0, 1 - z)     max(0, 1 + z)     -z
  lsgan      (z - 1)^2 / 2     z^2 / 2           (z - 1)^2 / 2
  wgan       -z                z                 -z"""
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
from test_gp_cpu import TINY, _tiny_case  # noqa: E402
from test_r1_cpu import ZERO_GRADS  # noqa: E402

OBJ_HEADER = os.path.join(ROOT, "include", "littlegan_hip_obj.h")
ENTRY_POINTS = ("lgo_heads_fwd", "lgo_gan_heads_loss_fwd_bwd")
KINDS = ("logistic", "hinge", "lsgan", "wgan")           # kind 1..4 of lgo_gan_heads_loss_fwd_bwd, in this order
KIND_NO = {k: i + 1 for i, k in enumerate(KINDS)}
ROLE_D_REAL, ROLE_D_FAKE, ROLE_G = 0, 1, 2
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# the objectives in float64: torch (differentiable, for the step reference) and numpy (values and derivatives, for the kernel tests)
def term(kind, role, z):
    """mean over the rows of f(z) for (kind, role); z a torch tensor of logits.  "bce" is the reference's term on sigmoid(z)."""
    fake = role == ROLE_D_FAKE
    if kind == "bce":
        return TO.bce_mean(TO.soft(0.0) if fake else TO.soft(1.0), torch.sigmoid(z))
    if kind == "logistic":
        f = torch.nn.functional.softplus(z if fake else -z)
    elif kind == "hinge":
        f = -z if role == ROLE_G else torch.relu(1.0 + z if fake else 1.0 - z)
    elif kind == "lsgan":
        f = 0.5 * (z if fake else z - 1.0) ** 2
    else:
        assert kind == "wgan", kind
        f = z if fake else -z
    return f.mean()


def np_term(kind, role, z):
    """-> (f(z), f'(z)) elementwise in float64; the subgradient at the hinge kink is 0"""
    z = np.asarray(z, np.float64)
    fake = role == ROLE_D_FAKE
    if kind == "logistic":
        x = z if fake else -z
        e = np.exp(-np.abs(x))
        sg = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        return np.maximum(x, 0.0) + np.log1p(e), sg if fake else -sg
    if kind == "hinge":
        if role == ROLE_G:
            return -z, -np.ones_like(z)
        t = 1.0 + z if fake else 1.0 - z
        return np.maximum(t, 0.0), np.where(t > 0, 1.0 if fake else -1.0, 0.0)
    if kind == "lsgan":
        d = z if fake else z - 1.0
        return 0.5 * d * d, d
    assert kind == "wgan", kind
    return (z, np.ones_like(z)) if fake else (-z, -np.ones_like(z))


def _t64(inp):
    return {k: torch.tensor(np.asarray(v, np.float64)) for k, v in inp.items()}


def _logit(net, image):
    Wd = net.W["D"]
    return net.encoder(image)[-1].reshape(image.shape[0], -1) @ Wd[16] + Wd[17]


def _np_grads(gs, ws):
    return [np.zeros(tuple(w.shape)) if g is None else g.detach().numpy() for g, w in zip(gs, ws)]


def objective_delta(cfg, W, b, inp, kind, recs=None):
    """The float64 autograd gradient of (real / fake terms of `kind` - those of the BCE form), per tape, and the same difference of the
    losses: what turns oracle.np_oracle.step_gradients into the step under `kind` (the gradients are linear in the top gradient, and the
    attribute and L1 terms are common to both).  recs: the three record sets of D's calls under diff_augment (D reads T(image))."""
    net = TO.Net(cfg, W)
    t = _t64({k: v for k, v in inp.items() if k != "gp_eps"})
    T = (lambda img, i: img) if recs is None else (lambda img, i: diffaug_torch(img, recs[i]))
    fake = net.generator(t["noise"], t["real_cond_2"])
    z_r, z_f = _logit(net, T(t["new_image"], 0)), _logit(net, T(fake, 1))
    d_disc = (term(kind, ROLE_D_REAL, z_r) + term(kind, ROLE_D_FAKE, z_f)) - (term("bce", ROLE_D_REAL, z_r) + term("bce", ROLE_D_FAKE, z_f))
    d_gen = term(kind, ROLE_G, z_f) - term("bce", ROLE_G, z_f)
    out = dict(disc_loss=float(d_disc.detach()), gen_loss=float(d_gen.detach()), adj_loss=None, dA=None,
               dD=_np_grads(torch.autograd.grad(d_disc, net.W["D"], retain_graph=True, allow_unused=True), net.W["D"]),
               dG=_np_grads(torch.autograd.grad(d_gen, net.W["G"], allow_unused=True), net.W["G"]))
    if cfg.train_adj and b > 10:
        c1, c2 = t["real_cond_1"], t["real_cond_2"]
        adj_img = net.adjuster(torch.cat([t["real_image_1"], fake.detach()], 0), (torch.cat([c2, c1], 0) + 1.0) * 0.5)
        z_a = _logit(net, T(adj_img, 2))
        d_adj = term(kind, ROLE_G, z_a) - term("bce", ROLE_G, z_a)
        out.update(adj_loss=float(d_adj.detach()), dA=_np_grads(torch.autograd.grad(d_adj, net.W["A"], allow_unused=True), net.W["A"]))
    return out


def with_objective(ref, delta):
    """a step reference (np_oracle.step_gradients' dict, or any of its shape) plus objective_delta's: the step under that objective"""
    out = dict(ref)
    for k in ("disc_loss", "gen_loss", "adj_loss"):
        if delta[k] is not None:
            out[k] = float(ref[k]) + delta[k]
    for k in ("dD", "dG", "dA"):
        if delta[k] is not None:
            out[k] = [np.asarray(a, np.float64) + d.reshape(np.asarray(a).shape) for a, d in zip(ref[k], delta[k])]
    return out


def step_reference(cfg, W, b, inp, kind):
    return with_objective(O.step_gradients(cfg, W, b, {k: v for k, v in inp.items() if k != "gp_eps"}), objective_delta(cfg, W, b, inp, kind))


def torch_step(cfg, W, b, inp, kind):
    """oracle.torch_oracle.step_gradients restated under `kind`, directly: the whole step in torch float64"""
    net = TO.Net(cfg, W)
    t = _t64(inp)
    img1, c1, img2, c2 = t["real_image_1"], t["real_cond_1"], t["real_image_2"], t["real_cond_2"]
    Wd = net.W["D"]

    def disc(image):
        x = net.encoder(image)[-1].reshape(image.shape[0], -1)
        return x @ Wd[16] + Wd[17], torch.sigmoid(x @ Wd[18] + Wd[19])

    fake = net.generator(t["noise"], c2)
    z_r, real_c = disc(t["new_image"])
    z_f, fake_c = disc(fake)
    disc_loss = 2.0 * TO.bce_mean(c1, real_c) + term(kind, ROLE_D_REAL, z_r) + term(kind, ROLE_D_FAKE, z_f)
    gen_loss = term(kind, ROLE_G, z_f) + TO.bce_mean(c2, fake_c) + cfg.l1_lambda * (img2 - fake).abs().mean()
    out = dict(disc_loss=float(disc_loss.detach()), gen_loss=float(gen_loss.detach()), adj_loss=None, dA=None,
               dD=_np_grads(torch.autograd.grad(disc_loss, Wd, retain_graph=True), Wd),
               dG=_np_grads(torch.autograd.grad(gen_loss, net.W["G"]), net.W["G"]))
    if cfg.train_adj and b > 10:
        t_cond = torch.cat([c2, c1], 0)
        adj_img = net.adjuster(torch.cat([img1, fake.detach()], 0), (t_cond + 1.0) * 0.5)
        z_a, adj_c = disc(adj_img)
        adj_loss = term(kind, ROLE_G, z_a) + TO.bce_mean(t_cond, adj_c) + cfg.l1_lambda * (torch.cat([img2, img1], 0) - adj_img).abs().mean()
        out.update(adj_loss=float(adj_loss.detach()), dA=_np_grads(torch.autograd.grad(adj_loss, net.W["A"]), net.W["A"]))
    return out


def torch_gp_logit(cfg, Wd, xhat, gp_weight):
    """tests/test_gp_cpu.py::torch_gp on the LOGIT of output_pr: gp_weight mean_b (|dl_b/dx^_b| - 1)^2 by autograd double backward
    -> (term, r [B], 20 gradients w.r.t. Discriminator.weights), float64"""
    net = TO.Net(cfg, {"D": Wd})
    x = torch.tensor(np.asarray(xhat, np.float64), requires_grad=True)
    g, = torch.autograd.grad(_logit(net, x).sum(), x, create_graph=True)
    r = g.flatten(1).norm(dim=1)
    pen = gp_weight * ((r - 1) ** 2).mean()
    dD = torch.autograd.grad(pen, net.W["D"], allow_unused=True)
    return float(pen.detach()), r.detach().numpy(), _np_grads(dD, net.W["D"])


# ---------------------------------------------------------------------------------------------------------------------
# the step reference, anchored
def _tiny_step(b):
    cfg = O.Cfg(**TINY)
    W = O.init_weights(cfg, 5)
    rng = np.random.default_rng(12)
    W = {m: [w + 0.1 * rng.standard_normal(w.shape) if w.ndim == 1 else w for w in ws] for m, ws in W.items()}
    return cfg, W, O.make_inputs(cfg, cfg.batch_size, seed=40 + b)


@pytest.mark.parametrize("b", [4, 5, 11], ids=["full", "partition", "adjuster"])
def test_bce_difference_is_identically_zero(b):
    cfg, W, inp = _tiny_step(b)
    d = objective_delta(cfg, W, b, inp, "bce")
    assert d["disc_loss"] == 0.0 and d["gen_loss"] == 0.0 and (b <= 10 or d["adj_loss"] == 0.0)
    for key in ("dD", "dG") + (("dA",) if b > 10 else ()):
        assert all(not np.any(g) for g in d[key]), key
    assert (d["dA"] is None) == (b <= 10)


@pytest.mark.parametrize("b", [4, 5, 11], ids=["full", "partition", "adjuster"])
@pytest.mark.parametrize("kind", KINDS)
def test_composition_equals_the_direct_restatement(kind, b):
    cfg, W, inp = _tiny_step(b)
    ref, direct = step_reference(cfg, W, b, inp, kind), torch_step(cfg, W, b, inp, kind)
    plain = O.step_gradients(cfg, W, b, inp)
    keys = ("disc_loss", "gen_loss") + (("adj_loss",) if b > 10 else ())
    for k in keys:
        assert abs(ref[k] - direct[k]) <= 1e-12 * max(1.0, abs(direct[k])), (k, ref[k], direct[k])
    assert max(abs(plain[k] - direct[k]) for k in keys) > 1e-3      # the objective is not the BCE one: the composition adds something
    for key in ("dD", "dG") + (("dA",) if b > 10 else ()):
        gmax = max(np.abs(e).max() for e in direct[key])
        for i, (got, exp) in enumerate(zip(ref[key], direct[key])):
            # a 1-element gradient (a bias, gamma, beta) is a sum of rows that may cancel to exactly 0 (dense_pr.bias under hinge: the
            # +-1/B of the rows): its error is measured against the model's largest gradient, as test_step_gpu.check_grads does
            scale = max(np.abs(exp).max(), 1e-30) if exp.size > 1 else gmax
            assert np.abs(np.asarray(got).ravel() - exp.ravel()).max() <= 1e-10 * scale + 1e-18, (key, i, scale)
    assert ref["dA"] is None or len(ref["dA"]) == 4


def test_logit_penalty_by_double_backward():
    cfg, Wd, xhat = _tiny_case(3)
    pen, r, grads = torch_gp_logit(cfg, Wd, xhat, 5.0)
    assert pen > 0 and np.all(r > 0) and r.shape == (cfg.batch_size,)
    for i, g in enumerate(grads):
        assert g.shape == np.asarray(Wd[i]).shape
        if i in ZERO_GRADS:      # norm4.beta, dense_pr.bias, dense_cond.*: the logit's image gradient does not depend on them
            assert not np.any(g), i
        else:
            assert np.any(g), i
    # the penalty on the logit is not the one on the sigmoid output
    from test_gp_cpu import torch_gp
    assert abs(torch_gp(cfg, Wd, xhat, 5.0)[0] - pen) > 1e-3 * pen


# ---------------------------------------------------------------------------------------------------------------------
# the entry points of include/littlegan_hip_obj.h
@pytest.fixture(scope="module")
def lib():
    from littlegan_amd.csrc.build import build
    build(verbose=False)
    from littlegan_amd import _lib
    return _lib


def test_obj_header_declares_the_entry_points_and_the_kinds(lib):
    assert set(_protos(OBJ_HEADER)) == set(ENTRY_POINTS) == {n for n in lib.SIGNATURES if n.startswith("lgo_")}
    # the two kind tables agree: config's names are the header's numbers
    from littlegan_amd import config
    assert config.GAN_LOSS_KINDS == dict(KIND_NO, bce=0)
    hdr = open(OBJ_HEADER).read()
    for name, no in KIND_NO.items():
        assert re.search(rf"#define LGO_KIND_{name.upper()} {no}\b", hdr), name


def test_argument_validation_without_gpu(lib):
    """every refusal happens on the host, before any launch: the pointers are never dereferenced (there is no device here)"""
    h = lib.load()
    a = [C.c_void_p(256 * (i + 1)) for i in range(8)]
    err = lambda: h.lg_last_error()
    fwd = h.lgo_heads_fwd          # (x, wpr, bpr, wc, bc, p, z_pr, workspace, ws_bytes, B, K, c, stream)
    ws = h.lg_heads_fwd_workspace_bytes(4, 64, 5)
    assert ws > 0
    for k in range(8):
        ptrs = list(a)
        ptrs[k] = None
        assert fwd(*ptrs, ws, 4, 64, 5, None) == -1 and b"null pointer" in err() and b"lgo_heads_fwd" in err(), k
    for B, K, c in ((0, 64, 5), (-1, 64, 5), (4, 0, 5), (4, -4, 5), (4, 62, 5), (4, 64, 0), (4, 64, -1), (4, 64, 41)):
        assert fwd(*a, 1 << 40, B, K, c, None) == -1 and b"bad shape" in err() and b"lgo_heads_fwd" in err(), (B, K, c)
    assert fwd(*a, ws - 1, 4, 64, 5, None) == -1 and b"workspace too small" in err() and b"lgo_heads_fwd" in err()
    loss = h.lgo_gan_heads_loss_fwd_bwd   # (p, z_pr, t_c, kind, role, w_pr, w_c, loss, dz, B, c, accumulate, stream)
    p, z, tc, ls, dz = a[:5]
    who = b"lgo_gan_heads_loss_fwd_bwd"
    for args in ((None, z, tc, 2, 0, 1.0, 1.0, ls, dz, 4, 5, 0, None), (p, None, tc, 2, 0, 1.0, 1.0, ls, dz, 4, 5, 0, None),
                 (p, z, tc, 2, 0, 1.0, 1.0, None, dz, 4, 5, 0, None), (p, z, tc, 2, 0, 1.0, 1.0, ls, None, 4, 5, 0, None)):
        assert loss(*args) == -1 and b"null pointer" in err() and who in err()
    for kind in (0, 5, -1, 1 << 20):
        assert loss(p, z, tc, kind, 0, 1.0, 1.0, ls, dz, 4, 5, 0, None) == -1 and b"bad kind" in err() and who in err(), kind
    for role in (-1, 3, 1 << 20):
        assert loss(p, z, tc, 2, role, 1.0, 1.0, ls, dz, 4, 5, 0, None) == -1 and b"bad role" in err() and who in err(), role
    for B, c in ((0, 5), (-3, 5), (4, 0), (4, -1), (1 << 30, 40)):
        assert loss(p, z, tc, 2, 0, 1.0, 1.0, ls, dz, B, c, 0, None) == -1 and b"bad shape" in err() and who in err(), (B, c)
    assert loss(p, z, None, 2, 0, 1.0, 1.0, ls, dz, 4, 5, 0, None) == -1 and b"t_c is null" in err() and who in err()
    assert loss(p, z, None, 2, 0, 1.0, -0.5, ls, dz, 4, 5, 0, None) == -1 and b"t_c is null" in err()
    for w in (float("nan"), float("inf"), float("-inf")):
        assert loss(p, z, tc, 2, 0, w, 1.0, ls, dz, 4, 5, 0, None) == -1 and b"finite" in err() and who in err(), w
        assert loss(p, z, tc, 2, 0, 1.0, w, ls, dz, 4, 5, 0, None) == -1 and b"finite" in err() and who in err(), w
        assert loss(p, z, None, 2, 0, 1.0, w, ls, dz, 4, 5, 0, None) == -1 and who in err(), w


# ---------------------------------------------------------------------------------------------------------------------
# configuration and trainer
def test_config_key_defaults_to_bce(tmp_path):
    from littlegan_amd import config
    assert config.DEFAULTS["gan_loss"] == "bce" and "gan_loss" in config.__doc__
    assert config.Arg(["train", "x"], config_dir=str(tmp_path)).gan_loss == "bce"
    assert config.gan_loss_kind("bce") == 0 and [config.gan_loss_kind(k) for k in KINDS] == [1, 2, 3, 4]
    assert config.gan_loss_kind("wgan", use_gp=True) == 4 and config.gan_loss_kind("hinge", use_gp=False) == 2
    (tmp_path / "h.config.json").write_text('{"gan_loss": "hinge"}')
    assert config.Arg(["train", "x", "-e", "h"], config_dir=str(tmp_path)).gan_loss == "hinge"
    (tmp_path / "w.config.json").write_text('{"gan_loss": "wgan", "use_gp": true}')
    a = config.Arg(["train", "x", "-e", "w"], config_dir=str(tmp_path))
    assert a.gan_loss == "wgan" and a.use_gp is True


@pytest.mark.parametrize("value", ["Hinge", "hinge ", "", "ns", "wgan-gp", None, 2, 2.0, True, False, ["hinge"]], ids=lambda v: repr(v))
def test_a_bad_value_raises(tmp_path, value):
    from littlegan_amd import config
    with pytest.raises(ValueError, match="gan_loss"):
        config.gan_loss_kind(value)
    (tmp_path / "bad.config.json").write_text(json.dumps({"gan_loss": value}))
    with pytest.raises(ValueError, match="gan_loss"):
        config.Arg(["train", "x", "-e", "bad"], config_dir=str(tmp_path))
    with pytest.raises(ValueError, match="gan_loss"):
        _cpu_trainer(gan_loss=value)


def test_wgan_without_the_penalty_raises(tmp_path):
    from littlegan_amd import config
    with pytest.raises(ValueError, match="use_gp"):
        config.gan_loss_kind("wgan", use_gp=False)
    (tmp_path / "w.config.json").write_text('{"gan_loss": "wgan"}')
    with pytest.raises(ValueError, match="gan_loss 'wgan' needs use_gp"):
        config.Arg(["train", "x", "-e", "w"], config_dir=str(tmp_path))
    with pytest.raises(ValueError, match="gan_loss 'wgan' needs use_gp"):
        _cpu_trainer(gan_loss="wgan")


def test_trainer_refusals_and_allowed_combinations():
    base, _ = _cpu_trainer()
    assert base.gan_loss == "bce" and base.gan_kind == 0
    explicit, _ = _cpu_trainer(gan_loss="bce")
    assert explicit.gan_kind == 0
    for name in KINDS[:3]:
        tr, _ = _cpu_trainer(gan_loss=name)
        assert (tr.gan_loss, tr.gan_kind) == (name, KIND_NO[name])
        assert [tr.step_kind(b) for b in range(40)] == [base.step_kind(b) for b in range(40)]   # constant over a run: no new kind
        assert set(tr.losses) == set(base.losses)
        assert "gan_loss" not in "".join(tr.checkpoint_state())   # stateless: no checkpoint field
    tr, _ = _cpu_trainer(gan_loss="wgan", use_gp=True)
    assert tr.gan_kind == 4 and tr.use_gp and "gp" in tr.losses
    tr, _ = _cpu_trainer(gan_loss="logistic", use_gp=True)     # the penalty is then on the logit
    assert tr.gan_kind == 1 and tr.use_gp
    # allowed with the neighbours (the gated draw needs a device: tests/test_gan_loss_gpu.py)
    tr, _ = _cpu_trainer(gan_loss="logistic", r1_gamma=10.0, r1_interval=4, diff_augment="color,cutout", ema_decay=0.99)
    assert tr.gan_kind == 1 and tr.r1 is not None and tr.diffaug == 5 and tr.ema_decay == 0.99
    tr, _ = _cpu_trainer(gan_loss="hinge", dropout_train=True, dropout_rate=0.25)
    assert tr.gan_kind == 2 and tr.dropout
    # the exclusions of use_gp stand under every objective
    for kw, why in ((dict(diff_augment="color"), "diff_augment and use_gp"), (dict(dropout_train=True, dropout_rate=0.25), "use_gp and dropout_train"),
                    (dict(r1_gamma=10.0), "r1_gamma and use_gp")):
        with pytest.raises(ValueError, match=why):
            _cpu_trainer(gan_loss="wgan", use_gp=True, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the exact-arithmetic kernel cases of tests/test_gan_loss_gpu.py: data, expected results, and why "bit for bit" is fair
EXACT_KINDS = ("hinge", "lsgan", "wgan")
EXACT_SHAPES = [(1, 1), (512, 40), (1024, 40)]     # one busy thread, then 21 and 41 trips of the 1024-thread block
EXACT_W_PR, EXACT_LOSS0 = 2.0, 3.0


def exact_z(B, role):
    """z = integers in [-16, 16] times 2^-2 with the hinge kinks planted: z[0] = the kink of the role (+1 real / G, -1 fake), z[1] the
    other one where B has room"""
    n = np.random.default_rng(5000 + 3 * B + role).integers(-16, 17, size=B)
    n[0] = -4 if role == ROLE_D_FAKE else 4
    if B > 1:
        n[1] = -n[0]
    return n


def exact_case(kind, role, B):
    """-> (z fp32, expected dz[:, 0] fp32, term fp32, loss after accumulating onto EXACT_LOSS0 fp32), each exact"""
    n = exact_z(B, role)
    f, g = np_term(kind, role, n * 0.25)
    t = EXACT_W_PR * f.sum() / B
    return (n * 0.25).astype(F32), ((EXACT_W_PR / B) * g).astype(F32), F32(t), F32(EXACT_LOSS0 + t)


def test_conditions_of_the_exact_cases():
    assert np.frexp(EXACT_W_PR)[0] == 0.5
    for B, c in EXACT_SHAPES:
        assert B & (B - 1) == 0 and B * (c + 1) <= 1024 * 41
        s = EXACT_W_PR / B
        assert np.frexp(s)[0] == 0.5 and float(F32(s)) == s          # a power of two: the scale rounds nothing
        for role in (ROLE_D_REAL, ROLE_D_FAKE, ROLE_G):
            n = exact_z(B, role)
            assert np.abs(n).max() <= 16 and (4 in n or -4 in n) and (B == 1 or (4 in n and -4 in n))
            for kind in EXACT_KINDS:
                z, dz, t, loss = exact_case(kind, role, B)
                assert np.array_equal(z.astype(np.float64), n * 0.25)
                f, g = np_term(kind, role, n * 0.25)
                # every summand s f(z_b) is an integer multiple of u = s / 32 ((z - 1)^2 / 2 has 5 fractional bits), and the sum of their
                # magnitudes is below 2^24 u: every partial sum, in any order, is an fp32 number — the fp32 sum is the exact one
                u = s / 32.0
                units = s * f / u
                assert np.array_equal(units, np.round(units)) and np.abs(units).sum() < 2 ** 24
                exact_t = float((s * f).sum())
                assert float(t) == exact_t and float(loss) == EXACT_LOSS0 + exact_t
                assert float(F32(EXACT_LOSS0)) + float(t) == float(loss)
                assert np.array_equal(dz.astype(np.float64), s * g)                  # s f'(z): a power of two times a small integer
                if kind == "hinge" and role != ROLE_G:
                    assert dz[0] == 0 and f[0] == 0                                # the kink: subgradient 0
                    assert np.any(dz != 0) or B == 1
