"""Logit-side GAN objectives (gan_loss; this project's definition) on the GPU.

Kernels: the loss kernel bit for bit in exact arithmetic (hinge, lsgan, wgan in each role; tests/test_gan_loss_cpu.py::
test_conditions_of_the_exact_cases), its attribute part bit for bit against ops.bce_heads_loss, every kind on random data against fp64 at
the bounds of tests/test_tail_ops_gpu.py::test_bce_heads_loss_sizes; the heads forward that keeps the logit on both GEMM routes.  (The
memory contract of both entry points: the heads-fwd-logit-* and gan-loss-* rows of tests/test_memory_contract_gpu.py, on this module's data.)
Steps: whole steps against np_oracle.step_gradients + the autograd gradient of the objectives' difference (tests/test_gan_loss_cpu.py::
step_reference) at the whole-step tolerances of tests/test_step_gpu.py, the Wasserstein objective with the penalty on the logit, the
neighbours (r1_gamma, diff_augment at p = 0.5), the defaults, bit-determinism, graph replay, two gloo ranks and the CLI."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # the spawned ranks import this module by name too
from oracle import np_oracle as O  # noqa: E402
from guards import called  # noqa: E402
from test_gan_loss_cpu import (ENTRY_POINTS, EXACT_KINDS, EXACT_LOSS0, EXACT_SHAPES, EXACT_W_PR, KIND_NO, KINDS, ROLE_D_FAKE, ROLE_D_REAL,  # noqa: E402
                               ROLE_G, exact_case, np_term, objective_delta, step_reference, torch_gp_logit, with_objective)
from test_r1_cpu import ZERO_GRADS, np_r1  # noqa: E402
from test_r1_gpu import SMALL  # noqa: E402
from test_skinny_gpu import HEADS_FWD, M, V, draw, launched  # noqa: E402
from test_step_gpu import TOLS, check_grads, dev_inputs, f32_round, grads_of, load_weights, make_args, perturbed  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLES = (ROLE_D_REAL, ROLE_D_FAKE, ROLE_G)
F32 = np.float32


@pytest.fixture(scope="module")
def ops():
    from littlegan_amd import ops as _ops
    return _ops


def _rel_rms(got, exp):
    got, exp = np.asarray(got, np.float64).ravel(), np.asarray(exp, np.float64).ravel()
    return np.sqrt(np.mean((got - exp) ** 2)) / (np.sqrt(np.mean(exp ** 2)) + 1e-30)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _np_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def f64(t):
    return t.detach().cpu().double().numpy()


def rel(got, exp):
    """the measure of tests/test_tail_ops_gpu.py: max-abs error relative to the max-abs of the fp64 result"""
    got = f64(got) if torch.is_tensor(got) else np.asarray(got)
    return float(np.abs(got - exp).max() / (np.abs(exp).max() + 1e-30))


def _heads_data(B, c, seed):
    """p in (0.02, 0.98) with saturated entries planted, smoothed attribute targets: the data of test_bce_heads_loss_sizes"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.02, 0.98, (B, 1 + c)).astype(F32).astype(np.float64)
    p[B - 1, c] = 1.0
    if B > 1 and c > 1:
        p[1, 2], p[B // 2, c] = 1.0, 0.0
    t_c = O.soft(2.0 * rng.integers(0, 2, (B, c)) - 1.0).astype(F32).astype(np.float64)
    return p, t_c


# ---------------------------------------------------------------------------------------------------------------- loss kernel, exact
@pytest.mark.parametrize("B,c", EXACT_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", EXACT_KINDS)
def test_loss_kernel_is_exact(ops, kind, B, c):
    p, _ = _heads_data(B, c, 11 * B + c)
    pd = dev(p)
    for role in ROLES:
        z, dz_w, term_w, loss_w = exact_case(kind, role, B)
        zd = dev(z)
        for accumulate, want in ((False, term_w), (True, loss_w)):
            loss = torch.full((1,), EXACT_LOSS0, device="cuda")
            dz = torch.full((B, 1 + c), 9.0, device="cuda")
            ops._lib.load().lg_clear_kernel()
            ops.gan_heads_loss(pd, zd, None, KIND_NO[kind], role, EXACT_W_PR, 0.0, loss, dz, accumulate)
            assert ops.last_kernel() == "gan_heads_kernel"
            torch.cuda.synchronize()
            assert np.array_equal(_bits(loss), _np_bits([want])), (kind, role, accumulate, float(loss), float(want))
            assert np.array_equal(_bits(dz[:, 0]), _np_bits(dz_w)), (kind, role)
            assert float(dz[:, 1:].abs().max()) == 0.0
        if kind == "hinge" and role != ROLE_G:   # the kinks were planted: z[0] = the role's, subgradient exactly 0 (+0.0)
            kink = -1.0 if role == ROLE_D_FAKE else 1.0
            assert z[0] == kink and _bits(dz[:1, 0])[0] == 0
            assert B == 1 or float(dz[1, 0]) != 0.0    # the other role's kink is this role's interior
        assert torch.equal(zd.cpu(), torch.from_numpy(z))


# ---------------------------------------------------------------------------------------------------------------- loss kernel, attribute part
@pytest.mark.parametrize("B,c", EXACT_SHAPES + [(3, 7)], ids=lambda v: str(v))
def test_attribute_part_equals_the_bce_kernel_bit_for_bit(ops, B, c):
    p, t_c = _heads_data(B, c, 13 * B + c)
    pd, td = dev(p), dev(t_c)
    zd = dev(np.random.default_rng(B).standard_normal(B) * 3)
    for w_c, acc in ((2.0, False), (1.0, True)):
        l0, d0 = torch.full((1,), 3.0, device="cuda"), torch.full((B, 1 + c), 9.0, device="cuda")
        ops.bce_heads_loss(pd, td, O.soft(1.0), 0.0, w_c, l0, d0, acc)
        for kind in KINDS:
            for role in ROLES:
                l1, d1 = torch.full((1,), 3.0, device="cuda"), torch.full((B, 1 + c), -9.0, device="cuda")
                ops.gan_heads_loss(pd, zd, td, KIND_NO[kind], role, 0.0, w_c, l1, d1, acc)
                assert np.array_equal(_bits(l1), _bits(l0)) and np.array_equal(_bits(d1), _bits(d0)), (kind, role, w_c)
        # (at (1, 1) the one attribute entry is the saturated one planted by _heads_data: its gradient is zero, its loss is not)
        assert float(d0[:, 0].abs().max()) == 0.0 and (B * c == 1 or float(d0[:, 1:].abs().max()) > 0.0) and float(l0) != 3.0 * (not acc)


# ---------------------------------------------------------------------------------------------------------------- loss kernel, fp32 data
@pytest.mark.parametrize("B,c", EXACT_SHAPES + [(3, 7)], ids=lambda v: str(v))
@pytest.mark.parametrize("kind", KINDS)
def test_loss_kernel_on_random_data_against_fp64(ops, kind, B, c):
    """Tolerances of tests/test_tail_ops_gpu.py::test_bce_heads_loss_sizes: loss 2e-6 relative + 1e-6, dz 1e-5 by its `rel`.  The
    logistic kind gets z = +-20 and +-100 planted: everything finite and inside the same bounds."""
    p, t_c = _heads_data(B, c, 17 * B + c)
    rng = np.random.default_rng(19 * B + c)
    z = (rng.standard_normal(B) * 3).astype(F32).astype(np.float64)
    variants = [z]
    if kind == "logistic":   # +-20 and +-100 in every role: the plants that fit, then the same rows negated
        for i, v in enumerate((100.0, -20.0, 20.0, -100.0)[:B]):
            z[(i * 7) % B if B > 4 else i] = v
        variants = [z, -z] + ([np.array([20.0]), np.array([-20.0])] if B == 1 else [])
        assert {20.0, -20.0, 100.0, -100.0} <= set(np.concatenate(variants).tolist())
    pd, td = dev(p), dev(t_c)
    attr = 2.0 * O.bce_mean(t_c, p[:, 1:])
    d_attr = 2.0 * O.bce_mean_bwd(t_c, p[:, 1:]) * p[:, 1:] * (1 - p[:, 1:])
    for role in ROLES:
        for zz in variants:
            zd = dev(zz)
            f, g = np_term(kind, role, zz)
            exp = 1.5 * f.mean() + attr
            loss, dz = torch.full((1,), 3.0, device="cuda"), torch.full((B, 1 + c), 9.0, device="cuda")
            ops.gan_heads_loss(pd, zd, td, KIND_NO[kind], role, 1.5, 2.0, loss, dz, False)
            e1, ez = abs(loss.item() - exp), rel(dz, np.concatenate([(1.5 / B) * g[:, None], d_attr], 1))
            print(f"{kind} role {role} B={B} c={c}: |loss err| {e1:.2e} (loss {exp:.5f}) dz {ez:.2e}")
            assert torch.isfinite(loss).all() and torch.isfinite(dz).all()
            assert e1 < 2e-6 * abs(exp) + 1e-6, (loss.item(), exp)
            assert ez < 1e-5
            # the real / fake column alone under the same measure (the attribute columns are 2 / c times smaller or larger)
            assert rel(dz[:, 0], (1.5 / B) * g) < 1e-5
            ops.gan_heads_loss(pd, zd, None, KIND_NO[kind], role, 0.5, 0.0, loss, dz, True)   # no attribute targets, weight 0; accumulate
            exp2 = exp + 0.5 * f.mean()
            assert abs(loss.item() - exp2) < 2e-6 * abs(exp2) + 1e-6, (loss.item(), exp2)
            assert float(dz[:, 1:].abs().max()) == 0.0 and rel(dz[:, 0], (0.5 / B) * g) < 1e-5


def test_nan_in_gives_nan_out_and_wrappers_refuse_wrong_shapes(ops):
    B, c = 4, 3
    p, t_c = _heads_data(B, c, 5)
    z = np.array([0.5, np.nan, -2.0, 1.0])
    for kind in KINDS:
        for role in ROLES:
            loss, dz = torch.zeros(1, device="cuda"), torch.zeros(B, 1 + c, device="cuda")
            ops.gan_heads_loss(dev(p), dev(z), dev(t_c), KIND_NO[kind], role, 1.0, 1.0, loss, dz, False)
            assert torch.isnan(loss).all() and torch.isnan(dz[1, 0]) and torch.isfinite(dz[[0, 2, 3], 0]).all(), (kind, role)
            assert torch.isfinite(dz[:, 1:]).all()
    pd, zd, loss, dz = dev(p), dev(z), torch.zeros(1, device="cuda"), torch.zeros(B, 1 + c, device="cuda")
    with pytest.raises(ValueError):
        ops.gan_heads_loss(pd, zd[:3], None, 2, 0, 1.0, 0.0, loss, dz, False)
    with pytest.raises(ValueError):
        ops.gan_heads_loss(pd, zd.view(B, 1), None, 2, 0, 1.0, 0.0, loss, dz, False)
    with pytest.raises(ValueError):
        ops.gan_heads_loss(pd, zd, None, 2, 0, 1.0, 0.0, loss, dz[:, :3], False)
    with pytest.raises(ValueError):
        ops.gan_heads_loss(pd, zd.double(), None, 2, 0, 1.0, 0.0, loss, dz, False)
    with pytest.raises(ValueError):
        ops.gan_heads_loss(pd, zd, dev(t_c)[:, :2], 2, 0, 1.0, 1.0, loss, dz, False)
    with pytest.raises(ops._lib.LittleGanHipError, match="lgo_gan_heads_loss_fwd_bwd"):
        ops.gan_heads_loss(pd, zd, None, 5, 0, 1.0, 0.0, loss, dz, False)
    with pytest.raises(ops._lib.LittleGanHipError, match="lgo_gan_heads_loss_fwd_bwd"):
        ops.gan_heads_loss(pd, zd, None, 2, 0, 1.0, 1.0, loss, dz, False)      # w_c != 0 without targets
    x = torch.zeros(2, 8, device="cuda")
    w = (torch.zeros(8, 1, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(8, 3, device="cuda"), torch.zeros(3, device="cuda"))
    with pytest.raises(ValueError):
        ops.heads_fwd_logit(x, w[0].view(8), *w[1:])
    with pytest.raises(ValueError):
        ops.heads_fwd_logit(x, *w, z_out=torch.zeros(3, device="cuda"))
    with pytest.raises(ops._lib.LittleGanHipError, match="lgo_heads_fwd"):
        ops.heads_fwd_logit(torch.zeros(2, 6, device="cuda"), torch.zeros(6, 1, device="cuda"), w[1], torch.zeros(6, 3, device="cuda"), w[3])


# ---------------------------------------------------------------------------------------------------------------- heads_fwd_logit
HEADS_CASES = [(32, 512, 40, M), (64, 1536, 40, M), (63, 1024, 40, V), (250, 1028, 7, V), (1, 4, 1, V)]


def _heads_operands(case, mode):
    B, K, c, _ = case
    rng = np.random.default_rng(1000 * B + K + c + (mode == "rand"))
    u = 2.0 ** -10   # integer form (tests/test_skinny_gpu.py): weights and biases multiples of 2^-10, the logits stay exact
    return (draw(rng, mode, B, K), draw(rng, mode, K, 1, scale=0.02, unit=u), draw(rng, mode, 1, unit=u),
            draw(rng, mode, K, c, scale=0.02, unit=u), draw(rng, mode, c, unit=u))


@pytest.mark.parametrize("mode", ["int", "rand"])
@pytest.mark.parametrize("case", HEADS_CASES, ids=lambda v: str(v))
def test_heads_fwd_logit(ops, case, mode):
    B, K, c, route = case
    assert (route == M) == (B % 32 == 0 and K % 512 == 0)
    x, wpr, bpr, wc, bc = _heads_operands(case, mode)
    d = [dev(a) for a in (x, wpr, bpr, wc, bc)]
    p0 = launched(ops, HEADS_FWD[route], lambda: ops.heads_fwd(*d))
    p, z = launched(ops, HEADS_FWD[route], lambda: ops.heads_fwd_logit(*d))
    torch.cuda.synchronize()
    assert tuple(p.shape) == (B, 1 + c) and tuple(z.shape) == (B,)
    assert np.array_equal(_bits(p), _bits(p0))                                   # the same partials, the same finalising expression
    z_e = (x @ wpr + bpr)[:, 0]
    if mode == "int":
        assert np.abs(z_e).max() < 2 ** 9 and np.array_equal(z_e.astype(F32).astype(np.float64), z_e)
        assert np.array_equal(_bits(z), _np_bits(z_e))
    else:
        print(f"heads_fwd_logit {case[:3]}: z {rel(z, z_e):.2e}")
        assert rel(z, z_e) < 1e-5
    # z is exactly the value whose sigmoid went into column 0
    assert rel(p[:, 0], O.sigmoid(f64(z))) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- whole steps
GP_WEIGHT = 5.0


def _build(cfg, W, mfma, gan_loss="hinge", **kw):
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    args = make_args(cfg, mfma)
    if gan_loss is not None:
        args.gan_loss = gan_loss
    if gan_loss == "wgan":
        args.use_gp, args.gp_weight = True, GP_WEIGHT
    for k, v in kw.items():
        setattr(args, k, v)
    decoder, encoder = Decoder(args), Encoder(args)
    g = Generator(args, decoder)
    d = Discriminator(args, encoder)
    tr = EagerTrainer(args, g, d, Adjuster(args, d, g), None)
    load_weights(tr, W)
    return tr


def _step_inputs(cfg, b):
    inp = f32_round(O.make_inputs(cfg, cfg.batch_size, seed=70 + b))
    inp["gp_eps"] = np.random.default_rng(b).uniform(0, 1, cfg.batch_size).astype(np.float32).astype(np.float64)
    return inp


_REF = {}


def _reference(kind, b):
    """computed once per (kind, batch_no), shared unchanged by the f32 and bf16 cases"""
    if (kind, b) not in _REF:
        cfg = O.Cfg(**SMALL)
        W = perturbed(cfg, 6)
        inp = _step_inputs(cfg, b)
        _REF[(kind, b)] = (cfg, W, inp, step_reference(cfg, W, b, inp, kind), O.step_gradients(cfg, W, b, {k: v for k, v in inp.items() if k != "gp_eps"}))
    return _REF[(kind, b)]


STEPS = {"logistic": (4, 11), "hinge": (4, 5, 10, 11, 15), "lsgan": (4, 11), "wgan": (4, 11)}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_whole_step_matches_the_step_reference(mfma, kind):
    """b = 4 full step, 11 full step with the Adjuster branch; hinge also 5 / 10 / 15, the three partition groups.  wgan runs with
    use_gp: the penalty on the logit at the device's own interpolate is added to the reference (as tests/test_gp_gpu.py adds np_gp)."""
    tol = TOLS[mfma]
    tr = None
    for b in STEPS[kind]:
        cfg, W, inp, ref, plain = _reference(kind, b)
        tr = tr or _build(cfg, W, mfma, kind)
        load_weights(tr, W)
        di = dev_inputs(inp)
        if kind != "wgan":
            di.pop("gp_eps")
        fake, adj, lg, ld, la = tr.train_step_from_inputs(b, di)
        torch.cuda.synchronize()
        pen = 0.0
        if kind == "wgan":
            e = inp["gp_eps"][:, None, None, None]
            pen, _, gpg = torch_gp_logit(cfg, W["D"], e * inp["new_image"] + (1 - e) * fake.cpu().double().numpy(), GP_WEIGHT)
            ref = dict(ref, dD=[a + g for a, g in zip(ref["dD"], gpg)])
            assert abs(float(tr.losses["gp"]) - pen) < max(tol["loss"], 1e-4) * abs(pen) + 1e-7
        keys = [("gen_loss", lg), ("disc_loss", ld)] + ([("adj_loss", la)] if b > 10 else [])
        print(f"{mfma} {kind} b={b}: " + "; ".join(f"{k} {v.item():.7g} / {ref[k] + (pen if k == 'disc_loss' else 0.0):.7g} (bce {plain[k]:.7g})"
                                                   for k, v in keys))
        for k, v in keys:
            want = ref[k] + (pen if k == "disc_loss" else 0.0)
            assert abs(v.item() - want) < tol["loss"] * abs(want), (b, k, v.item(), want)
        # the objective matters at the bound that decides: the BCE oracle's losses are far away
        # (against the f32 bound: logistic sits within 1 % of the smoothed BCE it replaces, inside what the bf16 path is held to)
        assert max(abs(plain[k] - ref[k]) / abs(ref[k]) for k, _ in keys) > 5 * TOLS["f32"]["loss"]
        only = {m: O.train_weight_indices(cfg, m, b) for m in "GDA"}
        sets = [("D", "dD"), ("G", "dG")] + ([("A", "dA")] if b > 10 else [])
        check_grads(tr, ref, sets, tol, tag=f"{kind} b={b}", only=only)


_ALONE = {}


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_logit_penalty_alone_against_torch_double_backward(mfma):
    """The assertions of tests/test_gp_gpu.py::test_penalty_alone_against_torch_double_backward, on its weights and interpolate"""
    from test_gp_gpu import _xhat
    from littlegan_amd import ops
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 4)
    real, fake, eps = _xhat(cfg, 9)
    if not _ALONE:
        _ALONE["v"] = torch_gp_logit(cfg, W["D"], eps[:, None, None, None] * real + (1 - eps[:, None, None, None]) * fake, GP_WEIGHT)
    term, r_ref, grads = _ALONE["v"]
    tr = _build(cfg, W, mfma, "wgan")
    tr.store.grad.zero_()
    xh = ops.gp_interp(*(torch.tensor(a, dtype=torch.float32, device="cuda").contiguous() for a in (real, fake, eps)))
    loss = torch.zeros(1, device="cuda")
    r = tr.discriminator.gradient_penalty(xh, GP_WEIGHT, loss, tr.losses["gp"], logit=True)
    torch.cuda.synchronize()
    tol = TOLS[mfma]
    print(f"{mfma}: term {float(tr.losses['gp']):.8g} / oracle {term:.8g}; |g| {r.cpu().numpy()} / {r_ref}")
    assert abs(float(tr.losses["gp"]) - term) <= tol["loss"] * abs(term) and float(loss) == float(tr.losses["gp"])
    assert np.abs(r.cpu().numpy() - r_ref).max() <= tol["loss"] * np.abs(r_ref).max()
    got = grads_of(tr, "D")
    maxrel = []
    for i, exp in enumerate(grads):
        exp = exp.ravel()
        d = got[i][:exp.size] - exp
        if i in ZERO_GRADS:
            assert not np.any(exp) and not np.any(got[i]), f"D weight {i} must receive exactly nothing from the penalty"
            continue
        if exp.size == 1:
            assert abs(d[0]) <= tol["grad_rms"] * abs(exp[0]) + tol["sfloor"] * max(np.abs(e).max() for e in grads), (i, d, exp)
        else:
            assert _rel_rms(got[i][:exp.size], exp) <= tol["grad_rms"], (i, _rel_rms(got[i][:exp.size], exp))
            maxrel.append(np.abs(d).max() / np.abs(exp).max())
    assert np.median(maxrel) <= tol["grad_med"], sorted(maxrel)


# ---------------------------------------------------------------------------------------------------------------- with the neighbours
@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_logistic_step_under_r1(mfma):
    tol = TOLS[mfma]
    b, gamma = 4, 10.0
    cfg, W, inp, ref, _ = _reference("logistic", b)
    tr = _build(cfg, W, mfma, "logistic", r1_gamma=gamma, r1_interval=1)
    di = dev_inputs(inp)
    di.pop("gp_eps")
    fake, adj, lg, ld, la = tr.train_step_from_inputs(b, di)
    torch.cuda.synchronize()
    term, _, g = np_r1(cfg, W["D"], inp["new_image"], gamma)
    ref = dict(ref, dD=[a + d for a, d in zip(ref["dD"], g)])
    want = ref["disc_loss"] + term
    print(f"{mfma}: disc {ld.item():.7g} / {want:.7g}, r1 {float(tr.losses['r1']):.7g} / {term:.7g}, gen {lg.item():.7g} / {ref['gen_loss']:.7g}")
    assert abs(ld.item() - want) < tol["loss"] * abs(want) and abs(lg.item() - ref["gen_loss"]) < tol["loss"] * abs(ref["gen_loss"])
    assert abs(float(tr.losses["r1"]) - term) < max(tol["loss"], 1e-4) * abs(term) + 1e-7
    check_grads(tr, ref, [("D", "dD"), ("G", "dG")], tol, tag=f"logistic r1 {mfma}", only={m: O.train_weight_indices(cfg, m, b) for m in "GDA"})


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_logistic_step_under_augmentation(ops, mfma):
    """diff_augment with diff_augment_p 0.5: the reference is tests/test_ada_gpu.py's gated oracle plus the objectives' difference taken
    through the same restated records; the device's own T(new_image) is read back and must be the restated one."""
    from test_ada_gpu import gated_reference
    from test_diffaug_cpu import diffaug_np
    from test_diffaug_gpu import build_aug, dev_key
    from test_diffaug_gpu import step_reference as aug_reference
    tol = TOLS[mfma]
    b = 1
    cfg, W, inp, _, _, _ = aug_reference(b)
    recs, gated = gated_reference(b)
    if "d" not in _ALONE:
        _ALONE["d"] = objective_delta(cfg, W, b, inp, "logistic", recs=recs)
    ref = with_objective(gated, _ALONE["d"])
    B, S = cfg.batch_size, 16 * cfg.init_dim
    tr = build_aug(cfg, W, mfma, diff_augment_p=0.5, gan_loss="logistic")
    key = dev_key(0, 0, 3)
    di = dev_inputs(inp)
    fake, adj, lg, ld, la = tr.train_step_from_inputs(b, dict(di, diffaug_key=key))
    x_aug = ops.diffaug_fwd(di["new_image"], ops.diffaug_draw_gated(key, 0, 0, B, S, tr.diffaug, ops.ada_init(0.5, device="cuda")))
    torch.cuda.synchronize()
    assert not torch.equal(x_aug, di["new_image"])
    assert np.abs(f64(x_aug) - diffaug_np(inp["new_image"], recs[0])).max() < 1e-5
    print(f"{mfma}: gen {lg.item():.7g} / {ref['gen_loss']:.7g} (bce {gated['gen_loss']:.7g}), disc {ld.item():.7g} / {ref['disc_loss']:.7g} "
          f"(bce {gated['disc_loss']:.7g})")
    for got, k in ((lg, "gen_loss"), (ld, "disc_loss")):
        assert abs(got.item() - ref[k]) < tol["loss"] * abs(ref[k]), (k, got.item(), ref[k])
    assert max(abs(gated[k] - ref[k]) / abs(ref[k]) for k in ("gen_loss", "disc_loss")) > 5 * TOLS["f32"]["loss"]   # (as in the whole-step test)
    check_grads(tr, ref, [("D", "dD"), ("G", "dG")], tol, tag=f"logistic aug {mfma}", only={m: O.train_weight_indices(cfg, m, b) for m in "GDA"})


# ---------------------------------------------------------------------------------------------------------------- defaults, determinism, graphs
def test_defaults_fetch_nothing_and_agree(ops, monkeypatch):
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 2)
    absent, bce, hinge = _build(cfg, W, "f32", None), _build(cfg, W, "f32", "bce"), _build(cfg, W, "f32", "hinge")
    assert not hasattr(absent.args, "gan_loss") and absent.gan_kind == 0 and bce.gan_kind == 0 and hinge.gan_kind == 2
    fetched = called(monkeypatch, ops)
    names = lambda: [n for n in fetched if n.startswith("lgo_")]   # noqa: E731
    for b in (1, 5, 11):
        inp = dev_inputs(_step_inputs(cfg, b))
        inp.pop("gp_eps")
        absent.train_step_from_inputs(b, inp)
        bce.train_step_from_inputs(b, inp)
    torch.cuda.synchronize()
    assert fetched and names() == []
    assert torch.equal(absent.store.flat, bce.store.flat) and torch.equal(absent.store.grad, bce.store.grad)
    inp = dev_inputs(_step_inputs(cfg, 11))
    inp.pop("gp_eps")
    hinge.train_step_from_inputs(11, inp)
    torch.cuda.synchronize()
    assert set(names()) == set(ENTRY_POINTS) and names().count("lgo_gan_heads_loss_fwd_bwd") == 4 and names().count("lgo_heads_fwd") == 2
    assert not torch.equal(hinge.store.grad, bce.store.grad)


def test_hinge_steps_are_bit_identical_and_graph_replay_matches():
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 8)
    for mfma in ("f32", "bf16"):
        outs = []
        for _ in range(2):
            tr = _build(cfg, W, mfma, "hinge")
            for b in (10, 11, 12):
                i = dev_inputs(_step_inputs(cfg, b))
                i.pop("gp_eps")
                tr.train_step_from_inputs(b, i)
            torch.cuda.synchronize()
            outs.append((tr.store.flat.cpu().clone(), tr.store.grad.cpu().clone()) + tuple(tr.losses[k].cpu().clone() for k in ("gen", "disc", "adj")))
        assert all(torch.equal(a, b) for a, b in zip(*outs)), mfma
        tg, te = _build(cfg, W, mfma, "hinge"), _build(cfg, W, mfma, "hinge")
        steps = range(6, 15)
        kinds = [tg.step_kind(b) for b in steps]
        assert {k[1] for k in kinds} == {False, True}
        for b in steps:
            i = dev_inputs(_step_inputs(cfg, b))
            i.pop("gp_eps")
            tg.graph_step(b, i)
            te.train_step_from_inputs(b, i)
            torch.cuda.synchronize()
            assert torch.equal(tg.store.flat, te.store.flat) and torch.equal(tg.store.grad, te.store.grad), (mfma, b)
            assert all(torch.equal(tg.losses[k], te.losses[k]) for k in ("gen", "disc", "adj")), (mfma, b)
        for adj_on in (False, True):   # each of the two kinds was replayed at least once (seen three times or more)
            assert max(kinds.count(k) for k in set(kinds) if k[1] == adj_on and k[0] == -1) >= 3
        assert len(tg._graphs) == sum(1 for k in set(kinds) if kinds.count(k) >= 2)


# ---------------------------------------------------------------------------------------------------------------- data parallel
DP = dict(init_dim=2, conv_filter=(64, 32, 32, 32, 32), cond_dim=5, noise_dim=11, batch_size=2)
DP_STEPS = (10, 11)


def _dp_inputs(cfg, world, b):
    return f32_round(O.make_inputs(cfg, cfg.batch_size * world, seed=300 + b))


def _dp_worker(rank, world, port, mfma, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = O.Cfg(**DP)
        tr = _build(cfg, perturbed(cfg, 21), mfma, "hinge")
        assert tr.sync.enabled
        B = cfg.batch_size
        for b in DP_STEPS:
            full = _dp_inputs(cfg, world, b)
            tr.train_step_from_inputs(b, dev_inputs({k: v[rank * B:(rank + 1) * B] for k, v in full.items()}))
        torch.cuda.synchronize()
        np.save(os.path.join(outdir, f"flat_{rank}.npy"), tr.store.flat.cpu().numpy())
        np.save(os.path.join(outdir, f"grad_{rank}.npy"), tr.store.grad.cpu().numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_two_ranks_with_hinge_equal_one_rank(tmp_path, mfma):
    """each rank takes the mean over its own rows: the all-reduced mean of the two is the objective of the double batch.  The bounds
    of tests/test_r1_gpu.py::test_two_ranks_with_penalty_equal_one_rank."""
    world = 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, mfma, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    try:
        for p in procs:
            p.join(timeout=600)
            assert p.exitcode == 0, f"rank process exit code {p.exitcode}"
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=20)
    flat = [np.load(tmp_path / f"flat_{r}.npy") for r in range(world)]
    grad = [np.load(tmp_path / f"grad_{r}.npy") for r in range(world)]
    assert np.array_equal(flat[0], flat[1]) and np.array_equal(grad[0], grad[1])
    cfg = O.Cfg(**DP)
    big = O.Cfg(**{**DP, "batch_size": cfg.batch_size * world})
    tr, off = _build(big, perturbed(cfg, 21), mfma, "hinge"), _build(big, perturbed(cfg, 21), mfma, "bce")
    for b in DP_STEPS:
        tr.train_step_from_inputs(b, dev_inputs(_dp_inputs(cfg, world, b)))
        off.train_step_from_inputs(b, dev_inputs(_dp_inputs(cfg, world, b)))
    torch.cuda.synchronize()
    g1 = tr.store.grad.cpu().numpy()
    gd = grad[0] / world
    tol = 2e-5 if mfma == "f32" else 2e-3
    s_, e_ = tr.store.model_range("D")
    assert _rel_rms(gd[s_:e_], g1[s_:e_]) < tol
    vis = _rel_rms(off.store.grad.cpu().numpy()[s_:e_], g1[s_:e_])
    print(f"{mfma}: two ranks against one {_rel_rms(gd[s_:e_], g1[s_:e_]):.3g}, with the BCE objective {vis:.3g}")
    assert vis > tol   # swapping in the BCE objective moves what is compared by more than the bound: the comparison sees the objective


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_main_train_with_hinge(tmp_path):
    cfgdir = tmp_path / "cfg"
    cfgdir.mkdir()
    res = tmp_path / "results"
    with open(os.path.join(ROOT, "e2e.config.json")) as f:
        base = json.load(f)
    base.update(all_result_dir=str(res), test_data_dir=str(tmp_path / "td"), epoch=1, gan_loss="hinge", restore=False, image_dim=32, init_dim=2,
                conv_filter=[64, 32, 32, 32, 32], synthetic_images=48, batch_size=4, freq_test=100)
    (cfgdir / "sample.config.json").write_text(json.dumps({"synthetic": True}))
    (cfgdir / "h.config.json").write_text(json.dumps(base))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "train", "exp", "-e", "h", "--debug"],
                       env=dict(os.environ, LITTLEGAN_CONFIG_DIR=str(cfgdir)), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if "LossD" in ln]
    assert lines
    for ln in lines:
        words = ln.split()
        assert all(np.isfinite(float(words[words.index(k) + 1])) for k in ("LossG", "LossD")), ln
    assert (res / "exp" / "checkpoint" / "ckpt-1.pt").is_file()
    # an unknown objective fails at start-up, before any device work
    (cfgdir / "x.config.json").write_text(json.dumps(dict(base, gan_loss="hing")))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "train", "exp", "-e", "x", "--debug"],
                       env=dict(os.environ, LITTLEGAN_CONFIG_DIR=str(cfgdir)), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "gan_loss" in r.stderr
