"""Relativistic pairing and the R2 penalty (relativistic / r2_gamma; this project's definition) on the GPU.

Kernels: lgrel_pair_heads_loss_fwd_bwd bit for bit in exact arithmetic (tests/test_rel_cpu.py::test_conditions_of_the_exact_cases),
bit for bit against lgo_gan_heads_loss_fwd_bwd where the two must agree (SELF against an all-zero z_ref is role 0), the two halves of a
pair against each other, on random data against fp64 (the bounds of tests/test_tail_ops_gpu.py::test_bce_heads_loss_sizes), NaNs;
lgrel_r12_seed bit for bit against two lgr_r1_seed calls on the halves and against exact arithmetic, repeated and under a one-CU budget.
Their memory contract: the rel-* rows of tests/test_memory_contract_gpu.py.
Whole steps against the float64 reference of tests/test_rel_cpu.py at the tolerances of tests/test_step_gpu.py; the joint R1 + R2 pass
alone against the torch double backward over 2B rows and against two r1_penalty passes; the off state; determinism, graph replay, two
gloo ranks and the CLI."""
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
from test_gan_loss_cpu import objective_delta, with_objective  # noqa: E402
from test_gan_loss_gpu import _heads_data, rel  # noqa: E402
from test_r1_cpu import EXACT_LOSS0 as SEED_LOSS0, EXACT_WEIGHT, SEED_SHAPES, ZERO_GRADS, exact_seed_case, torch_r1  # noqa: E402
from test_r1_gpu import one_cu  # noqa: E402
from test_rel_cpu import (EXACT_KINDS, EXACT_LOSS0, EXACT_SHAPES, EXACT_W_PR, KIND_NO, REL_KINDS, SIDE_OTHER, SIDE_SELF, exact_pair_case,  # noqa: E402
                          np_pair_term, rel_step_reference, relativistic_delta, torch_r12)
from test_step_gpu import TOLS, check_grads, dev_inputs, f32_round, grads_of, load_weights, make_args, perturbed  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(init_dim=2, conv_filter=(64, 32, 32, 32, 32), cond_dim=5, noise_dim=11, batch_size=3)
F32 = np.float32
G1, G2 = 10.0, 6.0      # r1_gamma, r2_gamma of the step tests


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


# ---------------------------------------------------------------------------------------------------------------- pair kernel, exact
@pytest.mark.parametrize("n,m,c", EXACT_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", EXACT_KINDS)
def test_pair_kernel_is_exact(ops, kind, n, m, c):
    p, _ = _heads_data(n, c, 11 * n + c)
    pd = dev(p)
    for side in (SIDE_SELF, SIDE_OTHER):
        z, zr, dz_w, term_w = exact_pair_case(kind, side, n, m)
        zd, zrd = dev(z), dev(zr)
        for accumulate in (False, True):
            want = F32((EXACT_LOSS0 if accumulate else 0.0) + float(term_w))
            loss = torch.full((1,), EXACT_LOSS0, device="cuda")
            dz = torch.full((n, 1 + c), 9.0, device="cuda")
            ops._lib.load().lg_clear_kernel()
            ops.pair_heads_loss(pd, zd, zrd, None, KIND_NO[kind], side, EXACT_W_PR, 0.0, loss, dz, accumulate)
            assert ops.last_kernel() == "pair_heads_kernel"
            torch.cuda.synchronize()
            assert np.array_equal(_bits(loss), _np_bits([want])), (kind, side, accumulate, float(loss), float(want))
            assert torch.equal(dz[:, 0].cpu(), torch.from_numpy(dz_w)), (kind, side)      # (-0.0 == 0.0: the sign of a zero is free)
            assert float(dz[:, 1:].abs().max()) == 0.0
        # the planted kinks t == 1: pairs 0 and 1, every row of the pair — the subgradient (and lsgan's gradient) is exactly 0
        rows = [i for i in range(n) if i % m in (0, 1)]
        assert float(dz[rows, 0].abs().max()) == 0.0 and (n == 1 or float(dz[:, 0].abs().max()) > 0.0)
        assert torch.equal(zd.cpu(), torch.from_numpy(z)) and torch.equal(zrd.cpu(), torch.from_numpy(zr))


# ---------------------------------------------------------------------------------------------------------------- pair kernel against the existing one
def _planted_z(n, seed):
    z = (np.random.default_rng(seed).standard_normal(n) * 3).astype(F32)
    for i, v in enumerate((100.0, -20.0, 20.0, -100.0)[:n]):
        z[(i * 7) % n if n > 4 else i] = v
    return z


@pytest.mark.parametrize("n,c", [(1, 1), (512, 40), (1024, 40), (3, 7)], ids=lambda v: str(v))
@pytest.mark.parametrize("kind", REL_KINDS)
def test_self_against_a_zero_reference_is_the_existing_kernel_bit_for_bit(ops, kind, n, c):
    """t = z - (+0.0) is z: SELF must give lgo_gan_heads_loss_fwd_bwd at role 0 (D real) — loss and every column of dz"""
    p, t_c = _heads_data(n, c, 13 * n + c)
    pd, td = dev(p), dev(t_c)
    for z in (_planted_z(n, 3 * n + c), -_planted_z(n, 3 * n + c)):
        zd = dev(z)
        for m in sorted({n, (n + 1) // 2 if n % 2 == 0 else n}):
            zero = torch.zeros(m, device="cuda")
            for (w_pr, w_c, acc) in ((1.0, 2.0, False), (1.5, 1.0, True)):
                l0, d0 = torch.full((1,), 3.0, device="cuda"), torch.full((n, 1 + c), 9.0, device="cuda")
                l1, d1 = torch.full((1,), 3.0, device="cuda"), torch.full((n, 1 + c), -9.0, device="cuda")
                ops.gan_heads_loss(pd, zd, td, KIND_NO[kind], 0, w_pr, w_c, l0, d0, acc)
                ops.pair_heads_loss(pd, zd, zero, td, KIND_NO[kind], SIDE_SELF, w_pr, w_c, l1, d1, acc)
                torch.cuda.synchronize()
                assert np.array_equal(_bits(l1), _bits(l0)) and np.array_equal(_bits(d1), _bits(d0)), (kind, m, w_pr)
                assert torch.isfinite(l1).all() and torch.isfinite(d1).all()


@pytest.mark.parametrize("kind", REL_KINDS)
def test_the_two_rows_of_a_pair_see_the_same_t(ops, kind):
    """dz of the fake row (OTHER, z_ref = z_r) is minus dz of the real row (SELF, z_ref = z_f), bit for bit"""
    for B, c in ((3, 7), (512, 40), (1000, 5)):
        rng = np.random.default_rng(B + c)
        z_r, z_f = dev(rng.standard_normal(B) * 3), dev(rng.standard_normal(B) * 3)
        p, _ = _heads_data(B, c, 29 * B + c)
        pd = dev(p)
        ds, do = torch.empty(B, 1 + c, device="cuda"), torch.empty(B, 1 + c, device="cuda")
        loss = torch.zeros(1, device="cuda")
        ops.pair_heads_loss(pd, z_r, z_f, None, KIND_NO[kind], SIDE_SELF, 1.0, 0.0, loss, ds, False)
        l_self = loss.clone()
        ops.pair_heads_loss(pd, z_f, z_r, None, KIND_NO[kind], SIDE_OTHER, 1.0, 0.0, loss, do, True)
        torch.cuda.synchronize()
        assert torch.equal(do[:, 0], -ds[:, 0]) and float(ds[:, 0].abs().max()) > 0
        assert torch.equal(loss, l_self)          # OTHER's column 0 adds nothing (accumulate: the SELF call's loss stays)


# ---------------------------------------------------------------------------------------------------------------- pair kernel, fp32 data
@pytest.mark.parametrize("n,m,c", EXACT_SHAPES + [(3, 3, 7), (6, 3, 7)], ids=lambda v: str(v))
@pytest.mark.parametrize("kind", REL_KINDS)
def test_pair_kernel_on_random_data_against_fp64(ops, kind, n, m, c):
    """Tolerances of tests/test_tail_ops_gpu.py::test_bce_heads_loss_sizes: loss 2e-6 relative + 1e-6, dz 1e-5 by its `rel`.  The
    difference is taken in fp32 on the device; the reference takes f0 of that fp32 difference (one rounding of t is the definition's)."""
    p, t_c = _heads_data(n, c, 17 * n + c)
    rng = np.random.default_rng(19 * n + m)
    z, zr = _planted_z(n, 5 * n + m), (rng.standard_normal(m) * 3).astype(F32)
    if m > 1:
        zr[1] = 50.0
    pd, td, zd, zrd = dev(p), dev(t_c), dev(z), dev(zr)
    attr = 2.0 * O.bce_mean(t_c, p[:, 1:])
    d_attr = 2.0 * O.bce_mean_bwd(t_c, p[:, 1:]) * p[:, 1:] * (1 - p[:, 1:])
    ref = zr[np.arange(n) % m]
    for side in (SIDE_SELF, SIDE_OTHER):
        t = (z - ref if side == SIDE_SELF else ref - z).astype(np.float64)       # the fp32 difference, as the device forms it
        f, g = np_pair_term(kind, t)
        sign = 1.0 if side == SIDE_SELF else -1.0
        exp = (1.5 * f.mean() if side == SIDE_SELF else 0.0) + attr
        loss, dz = torch.full((1,), 3.0, device="cuda"), torch.full((n, 1 + c), 9.0, device="cuda")
        ops.pair_heads_loss(pd, zd, zrd, td, KIND_NO[kind], side, 1.5, 2.0, loss, dz, False)
        e1, ez = abs(loss.item() - exp), rel(dz, np.concatenate([sign * (1.5 / n) * g[:, None], d_attr], 1))
        print(f"{kind} side {side} n={n} m={m} c={c}: |loss err| {e1:.2e} (loss {exp:.5f}) dz {ez:.2e}")
        assert torch.isfinite(loss).all() and torch.isfinite(dz).all()
        assert e1 < 2e-6 * abs(exp) + 1e-6, (loss.item(), exp)
        assert ez < 1e-5 and rel(dz[:, 0], sign * (1.5 / n) * g) < 1e-5
        ops.pair_heads_loss(pd, zd, zrd, None, KIND_NO[kind], side, 0.5, 0.0, loss, dz, True)
        exp2 = exp + (0.5 * f.mean() if side == SIDE_SELF else 0.0)
        assert abs(loss.item() - exp2) < 2e-6 * abs(exp2) + 1e-6, (loss.item(), exp2)
        assert float(dz[:, 1:].abs().max()) == 0.0 and rel(dz[:, 0], sign * (0.5 / n) * g) < 1e-5


def test_a_nan_poisons_exactly_its_pair_and_wrappers_refuse_wrong_shapes(ops):
    n, m, c = 8, 4, 3
    p, t_c = _heads_data(n, c, 5)
    pd, td = dev(p), dev(t_c)
    z = np.linspace(-2, 2, n)
    zr = np.linspace(-1, 1, m)
    z_nan, zr_nan = z.copy(), zr.copy()
    z_nan[1] = np.nan          # row 1 alone
    zr_nan[2] = np.nan         # pair 2: rows 2 and 6
    for kind in REL_KINDS:
        for side in (SIDE_SELF, SIDE_OTHER):
            for zz, rr, bad in ((z_nan, zr, [1]), (z, zr_nan, [2, 6]), (z_nan, zr_nan, [1, 2, 6])):
                loss, dz = torch.zeros(1, device="cuda"), torch.zeros(n, 1 + c, device="cuda")
                ops.pair_heads_loss(pd, dev(zz), dev(rr), td, KIND_NO[kind], side, 1.0, 1.0, loss, dz, False)
                good = [i for i in range(n) if i not in bad]
                assert torch.isnan(dz[bad, 0]).all() and torch.isfinite(dz[good, 0]).all() and torch.isfinite(dz[:, 1:]).all(), (kind, side, bad)
                assert bool(torch.isnan(loss).all()) == (side == SIDE_SELF), (kind, side)     # OTHER's column 0 is no part of the loss
    zd, zrd, loss, dz = dev(z), dev(zr), torch.zeros(1, device="cuda"), torch.zeros(n, 1 + c, device="cuda")
    with pytest.raises(ValueError):
        ops.pair_heads_loss(pd, zd[:3], zrd, None, 2, 0, 1.0, 0.0, loss, dz, False)
    with pytest.raises(ValueError):
        ops.pair_heads_loss(pd, zd, zrd.double(), None, 2, 0, 1.0, 0.0, loss, dz, False)
    with pytest.raises(ValueError):
        ops.pair_heads_loss(pd, zd, zrd, None, 2, 0, 1.0, 0.0, loss, dz[:, :3], False)
    with pytest.raises(ops._lib.LittleGanHipError, match="lgrel_pair_heads_loss_fwd_bwd"):
        ops.pair_heads_loss(pd, zd, zrd[:3].contiguous(), None, 2, 0, 1.0, 0.0, loss, dz, False)      # 8 % 3 != 0
    with pytest.raises(ops._lib.LittleGanHipError, match="lgrel_pair_heads_loss_fwd_bwd"):
        ops.pair_heads_loss(pd, zd, zrd, None, 4, 0, 1.0, 0.0, loss, dz, False)                      # wgan has no pairing
    with pytest.raises(ops._lib.LittleGanHipError, match="lgrel_pair_heads_loss_fwd_bwd"):
        ops.pair_heads_loss(pd, zd, zrd, None, 2, 2, 1.0, 0.0, loss, dz, False)
    with pytest.raises(ValueError):
        ops.r12_seed(torch.zeros(3, 16, device="cuda"), 1.0, 1.0)
    with pytest.raises(ops._lib.LittleGanHipError, match="lgrel_r12_seed"):
        ops.r12_seed(torch.zeros(2, 6, device="cuda"), 1.0, 1.0)
    with pytest.raises(ops._lib.LittleGanHipError, match="lgrel_r12_seed"):
        ops.r12_seed(torch.zeros(2, 8, device="cuda"), 1.0, -1.0)


# ---------------------------------------------------------------------------------------------------------------- the joint seed
W_FAKE = EXACT_WEIGHT / 2      # a second power of two: halving u0 and the term rounds nothing


def _seed_halves(B, L):
    """the exact case of tests/test_r1_cpu.py as the real half; its rows reversed and negated as the fake half, at half the weight"""
    g, u0, r2, term, loss = exact_seed_case(B, L)
    t2 = F32(0.5) * term
    return (np.concatenate([g, -g[::-1]]), np.concatenate([u0, F32(-0.5) * u0[::-1]]), np.concatenate([r2, r2[::-1]]), term, t2,
            F32(F32(loss) + t2))


@pytest.mark.parametrize("B,L", SEED_SHAPES, ids=lambda v: str(v))
def test_joint_seed_is_two_r1_seeds_bit_for_bit_and_exact(ops, B, L):
    g, u0_w, r2_w, t1_w, t2_w, loss_w = _seed_halves(B, L)
    gd = dev(g)

    def run(with_loss=True, with_r1=True, with_r2=True, w_fake=W_FAKE):
        loss, r1l, r2l = (torch.full((1,), v, device="cuda") if on else None for v, on in ((SEED_LOSS0, with_loss), (-7.0, with_r1), (-8.0, with_r2)))
        ops._lib.load().lg_clear_kernel()
        u0, r2 = ops.r12_seed(gd, EXACT_WEIGHT, w_fake, loss, r1l, r2l)
        assert ops.last_kernel() == "r12_seed_final_kernel"
        torch.cuda.synchronize()
        return u0, r2, loss, r1l, r2l

    # the two lgr_r1_seed calls on the halves, accumulating onto the same loss in the same order
    loss2, a, b = torch.full((1,), SEED_LOSS0, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    ua, ra = ops.r1_seed(gd[:B], EXACT_WEIGHT, loss2, a)
    ub, rb = ops.r1_seed(gd[B:], W_FAKE, loss2, b)
    runs = [run(), run()]
    with one_cu(ops):
        runs.append(run())
    for u0, r2, loss, r1l, r2l in runs:
        assert torch.equal(u0[:B], ua) and torch.equal(u0[B:], ub) and torch.equal(r2[:B], ra) and torch.equal(r2[B:], rb)
        assert torch.equal(loss, loss2) and torch.equal(r1l, a) and torch.equal(r2l, b)
        assert np.array_equal(_bits(u0), _np_bits(u0_w)) and np.array_equal(_bits(r2), _np_bits(r2_w))
        assert np.array_equal(_bits(r1l), _np_bits([t1_w])) and np.array_equal(_bits(r2l), _np_bits([t2_w]))
        assert np.array_equal(_bits(loss), _np_bits([loss_w]))
    assert torch.equal(gd.cpu(), torch.from_numpy(g))
    for flags in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        u0, r2, loss, r1l, r2l = run(*flags)
        assert np.array_equal(_bits(u0), _np_bits(u0_w)) and np.array_equal(_bits(r2), _np_bits(r2_w))
        assert loss is None or np.array_equal(_bits(loss), _np_bits([loss_w]))
        assert r1l is None or np.array_equal(_bits(r1l), _np_bits([t1_w]))
        assert r2l is None or np.array_equal(_bits(r2l), _np_bits([t2_w]))
    # w_fake == 0: the fake half's adjoint and term are zero, r2 is still written, the loss is R1's
    u0, r2, loss, r1l, r2l = run(w_fake=0.0)
    assert float(u0[B:].abs().max()) == 0.0 and float(r2l) == 0.0 and np.array_equal(_bits(r2), _np_bits(r2_w))
    assert np.array_equal(_bits(u0[:B]), _np_bits(u0_w[:B])) and np.array_equal(_bits(loss), _np_bits([F32(SEED_LOSS0) + t1_w]))


@pytest.mark.parametrize("B,L", [(3, 3072), (128, 49152)], ids=lambda v: str(v))
def test_joint_seed_on_random_data(ops, B, L):
    gen = torch.Generator(device="cuda").manual_seed(B + L)
    g = torch.randn(2 * B, L, device="cuda", generator=gen) * 0.02
    w1, w2 = 160.0, 96.0
    loss, r1l, r2l = torch.full((1,), 0.5, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    u0, r2 = ops.r12_seed(g, w1, w2, loss, r1l, r2l)
    loss2, a, b = torch.full((1,), 0.5, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    ua, ra = ops.r1_seed(g[:B], w1, loss2, a)
    ub, rb = ops.r1_seed(g[B:], w2, loss2, b)
    with one_cu(ops):
        u0c, r2c = ops.r12_seed(g, w1, w2)
    torch.cuda.synchronize()
    assert torch.equal(u0, torch.cat([ua, ub])) and torch.equal(r2, torch.cat([ra, rb])) and torch.equal(u0c, u0) and torch.equal(r2c, r2)
    assert torch.equal(loss, loss2) and torch.equal(r1l, a) and torch.equal(r2l, b)
    gd = g.double()
    r2d = (gd ** 2).sum(1)
    scale = torch.cat([torch.full((B,), w1 / B), torch.full((B,), w2 / B)]).double().cuda()[:, None]
    assert _rel_rms(u0.double().cpu(), (scale * gd).cpu()) < 1e-5 and _rel_rms(r2.double().cpu(), r2d.cpu()) < 1e-5
    for got, w, rows in ((r1l, w1, r2d[:B]), (r2l, w2, r2d[B:])):
        term = 0.5 * w * float(rows.mean())
        assert abs(float(got) - term) <= 1e-5 * abs(term)


# ---------------------------------------------------------------------------------------------------------------- whole steps
def _build(cfg, W, mfma, gan_loss="logistic", relativistic=True, **kw):
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    args = make_args(cfg, mfma)
    if gan_loss is not None:
        args.gan_loss = gan_loss
    if relativistic is not None:
        args.relativistic = relativistic
    for k, v in kw.items():
        setattr(args, k, v)
    decoder, encoder = Decoder(args), Encoder(args)
    g = Generator(args, decoder)
    d = Discriminator(args, encoder)
    tr = EagerTrainer(args, g, d, Adjuster(args, d, g), None)
    load_weights(tr, W)
    return tr


def _step_inputs(cfg, b):
    return f32_round(O.make_inputs(cfg, cfg.batch_size, seed=70 + b))


_REF = {}


def _reference(kind, b):
    """computed once per (kind, batch_no), shared unchanged by the f32 and bf16 cases and by the penalty tests"""
    if (kind, b) not in _REF:
        cfg = O.Cfg(**SMALL)
        W = perturbed(cfg, 6)
        inp = _step_inputs(cfg, b)
        _REF[(kind, b)] = (cfg, W, inp, rel_step_reference(cfg, W, b, inp, kind))
    return _REF[(kind, b)]


def _check_step(tr, cfg, ref, b, outs, tol, tag, extra_disc=0.0):
    fake, adj, lg, ld, la = outs
    keys = [("gen_loss", lg), ("disc_loss", ld)] + ([("adj_loss", la)] if b > 10 else [])
    print(f"{tag}: " + "; ".join(f"{k} {v.item():.7g} / {ref[k] + (extra_disc if k == 'disc_loss' else 0.0):.7g}" for k, v in keys))
    for k, v in keys:
        want = ref[k] + (extra_disc if k == "disc_loss" else 0.0)
        assert abs(v.item() - want) < tol["loss"] * abs(want), (tag, k, v.item(), want)
    only = {m: O.train_weight_indices(cfg, m, b) for m in "GDA"}
    sets = [("D", "dD"), ("G", "dG")] + ([("A", "dA")] if b > 10 else [])
    check_grads(tr, ref, sets, tol, tag=tag, only=only)


STEPS = {"logistic": (1, 12), "hinge": (1, 5, 10, 12, 15), "lsgan": (1, 12)}


@pytest.mark.parametrize("kind", REL_KINDS)
@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_whole_relativistic_step_matches_the_reference(mfma, kind):
    """b = 1 full step, 12 with the Adjuster branch; hinge also 5 / 10 / 15, the three partition groups of D"""
    tr = None
    for b in STEPS[kind]:
        cfg, W, inp, ref = _reference(kind, b)
        tr = tr or _build(cfg, W, mfma, kind)
        load_weights(tr, W)
        outs = tr.train_step_from_inputs(b, dev_inputs(inp))
        torch.cuda.synchronize()
        _check_step(tr, cfg, ref, b, outs, TOLS[mfma], f"{mfma} rel {kind} b={b}")


_PEN = {}


def _penalty_reference(cfg, W, x_all, w1, w2, key):
    if key not in _PEN:
        _PEN[key] = torch_r12(cfg, W["D"], x_all, w1, w2)
    return _PEN[key]


def _check_penalty_step(tr, cfg, W, ref, b, outs, tol, tag, x_all, w1, w2, key):
    t1, t2, _, g = _penalty_reference(cfg, W, x_all, w1, w2, key)
    ref = dict(ref, dD=[a + d for a, d in zip(ref["dD"], g)])
    for name, want in (("r1", t1), ("r2", t2)):
        if name in tr.losses:
            print(f"{tag}: {name} {float(tr.losses[name]):.7g} / {want:.7g}")
            assert abs(float(tr.losses[name]) - want) < max(tol["loss"], 1e-4) * abs(want) + 1e-7, (tag, name)
    _check_step(tr, cfg, ref, b, outs, tol, tag, extra_disc=t1 + t2)


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_the_recipe_step(ops, monkeypatch, mfma):
    """logistic + relativistic + r1_gamma + r2_gamma at r1_interval 1: the terms r1 and r2, the disc loss and D's gradients; the penalty
    is ONE joint pass (lgrel_r12_seed once, no lgr_r1_seed).  The fake half is the device's own `fake`, read back."""
    b = 4
    cfg, W, inp, ref = _reference("logistic", b)
    tr = _build(cfg, W, mfma, "logistic", r1_gamma=G1, r2_gamma=G2, r1_interval=1)
    names = called(monkeypatch, ops)
    outs = tr.train_step_from_inputs(b, dev_inputs(inp))
    torch.cuda.synchronize()
    assert names.count("lgrel_r12_seed") == 1 and "lgr_r1_seed" not in names and names.count("lgrel_pair_heads_loss_fwd_bwd") == 3
    assert "lgo_gan_heads_loss_fwd_bwd" not in names
    x_all = np.concatenate([inp["new_image"], outs[0].cpu().double().numpy()], 0)
    _check_penalty_step(tr, cfg, W, ref, b, outs, TOLS[mfma], f"{mfma} recipe", x_all, G1, G2, ("recipe", mfma))


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_r2_alone(ops, monkeypatch, mfma):
    """r2_gamma without r1_gamma, under the relativistic hinge: the existing R1 pass on the fake rows, reported as losses['r2']"""
    b = 12
    cfg, W, inp, ref = _reference("hinge", b)
    tr = _build(cfg, W, mfma, "hinge", r2_gamma=G2, r1_interval=1)
    assert tr.r1 is None and "r1" not in tr.losses
    names = called(monkeypatch, ops)
    outs = tr.train_step_from_inputs(b, dev_inputs(inp))
    torch.cuda.synchronize()
    assert names.count("lgr_r1_seed") == 1 and "lgrel_r12_seed" not in names
    x_all = np.concatenate([inp["new_image"], outs[0].cpu().double().numpy()], 0)
    _check_penalty_step(tr, cfg, W, ref, b, outs, TOLS[mfma], f"{mfma} r2 alone", x_all, 0.0, G2, ("r2", mfma))


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_lazy_interval(ops, monkeypatch, mfma):
    """r1_interval 2: b = 1 carries no penalty (no penalty function is fetched, the terms stay, the bits are those of a trainer without
    the gammas), b = 4 carries both with weight 2 gamma"""
    cfg, W, inp, ref1 = _reference("logistic", 1)
    tr, off = _build(cfg, W, mfma, r1_gamma=G1, r2_gamma=G2, r1_interval=2), _build(cfg, W, mfma)
    assert tr.r1["weight"] == 2 * G1 and tr.r2["weight"] == 2 * G2 and tr.step_kind(1)[2] is False and tr.step_kind(4)[2] is True
    tr.losses["r1"].fill_(7.0)
    tr.losses["r2"].fill_(8.0)
    with monkeypatch.context() as mp_:
        names = called(mp_, ops)
        tr.train_step_from_inputs(1, dev_inputs(inp))
        off.train_step_from_inputs(1, dev_inputs(inp))
        torch.cuda.synchronize()
    assert not [n for n in names if n.startswith("lgr_") or n == "lgrel_r12_seed"]
    assert float(tr.losses["r1"]) == 7.0 and float(tr.losses["r2"]) == 8.0
    assert torch.equal(tr.store.grad, off.store.grad) and torch.equal(tr.store.flat, off.store.flat)
    assert torch.equal(tr.losses["disc"], off.losses["disc"])
    cfg, W, inp, ref = _reference("logistic", 4)
    load_weights(tr, W)
    outs = tr.train_step_from_inputs(4, dev_inputs(inp))
    torch.cuda.synchronize()
    x_all = np.concatenate([inp["new_image"], outs[0].cpu().double().numpy()], 0)
    _check_penalty_step(tr, cfg, W, ref, 4, outs, TOLS[mfma], f"{mfma} lazy b=4", x_all, 2 * G1, 2 * G2, ("lazy", mfma))


_AUG = {}


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_recipe_step_under_augmentation(ops, mfma):
    """diff_augment at diff_augment_p 0.5: the reference is tests/test_ada_gpu.py's gated oracle plus the two objective differences taken
    through the same restated records; the penalties are taken on the rows D read — the device's own T([new_image ; fake]), read back"""
    from test_ada_gpu import gated_reference
    from test_diffaug_gpu import build_aug, dev_key
    from test_diffaug_gpu import step_reference as aug_reference
    b = 1
    cfg, W, inp, _, _, _ = aug_reference(b)
    recs, gated = gated_reference(b)
    if "d" not in _AUG:
        _AUG["d"] = with_objective(with_objective(gated, objective_delta(cfg, W, b, inp, "logistic", recs=recs)),
                                   relativistic_delta(cfg, W, b, inp, "logistic", recs=recs))
    ref = _AUG["d"]
    B, S = cfg.batch_size, 16 * cfg.init_dim
    tr = build_aug(cfg, W, mfma, diff_augment_p=0.5, gan_loss="logistic", relativistic=True, r1_gamma=G1, r2_gamma=G2, r1_interval=1)
    key = dev_key(0, 0, 3)
    di = dev_inputs(inp)
    outs = tr.train_step_from_inputs(b, dict(di, diffaug_key=key))
    par = ops.diffaug_draw_gated(key, 0, 0, 2 * B, S, tr.diffaug, ops.ada_init(0.5, device="cuda"))
    x_aug = ops.diffaug_fwd(torch.cat([di["new_image"], outs[0]], 0).contiguous(), par)
    torch.cuda.synchronize()
    assert not torch.equal(x_aug[B:], outs[0])
    _check_penalty_step(tr, cfg, W, ref, b, outs, TOLS[mfma], f"{mfma} recipe aug", x_aug.cpu().double().numpy(), G1, G2, ("aug", mfma))


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_relativistic_step_with_use_gp(mfma):
    """use_gp under a relativistic objective penalises the logit and does not read the objective: the reference adds the logit penalty
    of tests/test_gan_loss_cpu.py at the device's own interpolate"""
    from test_gan_loss_cpu import torch_gp_logit
    b, gpw = 4, 5.0
    cfg, W, inp, ref = _reference("lsgan", b)
    tol = TOLS[mfma]
    tr = _build(cfg, W, mfma, "lsgan", use_gp=True, gp_weight=gpw)
    eps = np.random.default_rng(b).uniform(0, 1, cfg.batch_size).astype(np.float32).astype(np.float64)
    outs = tr.train_step_from_inputs(b, dict(dev_inputs(inp), gp_eps=dev(eps)))
    torch.cuda.synchronize()
    e = eps[:, None, None, None]
    pen, _, gpg = torch_gp_logit(cfg, W["D"], e * inp["new_image"] + (1 - e) * outs[0].cpu().double().numpy(), gpw)
    assert abs(float(tr.losses["gp"]) - pen) < max(tol["loss"], 1e-4) * abs(pen) + 1e-7
    _check_step(tr, cfg, dict(ref, dD=[a + g for a, g in zip(ref["dD"], gpg)]), b, outs, tol, f"{mfma} rel lsgan gp", extra_disc=pen)


# ---------------------------------------------------------------------------------------------------------------- the joint pass alone
_ALONE = {}


def _interpolates(cfg, seed):
    """the input of tests/test_gp_gpu.py's and tests/test_r1_gpu.py's penalty-alone tests: the interpolate of two uniform images"""
    rng = np.random.default_rng(seed)
    shp = (cfg.batch_size, cfg.image_dim, cfg.image_dim, 3)
    real, fake, eps = (a.astype(np.float32).astype(np.float64) for a in (rng.uniform(-1, 1, shp), rng.uniform(-1, 1, shp), rng.uniform(0, 1, cfg.batch_size)))
    e = eps[:, None, None, None]
    return (e * real + (1 - e) * fake).astype(np.float32).astype(np.float64)


def _alone_reference():
    """computed once, shared by the f32 and bf16 cases.  The bounds are those of tests/test_r1_gpu.py's penalty-alone test, so the data
    is too: its weights, its input (seed 9) as the real half, a second draw of the same kind (seed 10) as the fake half"""
    if not _ALONE:
        cfg = O.Cfg(**SMALL)
        W = perturbed(cfg, 4)
        x = np.concatenate([_interpolates(cfg, 9), _interpolates(cfg, 10)], 0)
        _ALONE["v"] = (cfg, W, x, torch_r12(cfg, W["D"], x, G1, G2))
    return _ALONE["v"]


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_joint_penalty_alone_against_torch_double_backward_and_two_passes(mfma):
    """The assertions of tests/test_r1_gpu.py::test_penalty_alone_against_torch_double_backward over 2B rows, and the weight gradients
    against the sum of two r1_penalty passes on the halves at the same tolerance (the column sum's slab order differs)."""
    cfg, W, x, (t1, t2, r2_ref, grads) = _alone_reference()
    B = cfg.batch_size
    tr = _build(cfg, W, mfma, r1_gamma=G1, r2_gamma=G2, r1_interval=1)
    D = tr.discriminator
    xd = dev(x)
    tr.store.grad.zero_()
    loss = torch.zeros(1, device="cuda")
    r2 = D.r12_penalty(xd, G1, G2, loss, tr.losses["r1"], tr.losses["r2"])
    torch.cuda.synchronize()
    got = [g.copy() for g in grads_of(tr, "D")]
    tr.store.grad.zero_()
    loss2, a, b = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    ra = D.r1_penalty(xd[:B], G1, loss2, a)
    rb = D.r1_penalty(xd[B:], G2, loss2, b)
    torch.cuda.synchronize()
    two = [g.copy() for g in grads_of(tr, "D")]
    tol = TOLS[mfma]
    print(f"{mfma}: r1 {float(tr.losses['r1']):.8g} / {t1:.8g}, r2 {float(tr.losses['r2']):.8g} / {t2:.8g}")
    assert abs(float(tr.losses["r1"]) - t1) <= tol["loss"] * t1 and abs(float(tr.losses["r2"]) - t2) <= tol["loss"] * t2
    # against the two passes: per-row quantities, at the float tolerance (a 2B-row batch may take other conv routes than a B-row one)
    assert abs(float(a) - float(tr.losses["r1"])) <= tol["loss"] * t1 and abs(float(b) - float(tr.losses["r2"])) <= tol["loss"] * t2
    assert abs(float(loss) - float(loss2)) <= tol["loss"] * (t1 + t2) and float(loss) > 0
    assert np.abs(np.sqrt(r2.cpu().double().numpy()) - np.sqrt(torch.cat([ra, rb]).cpu().double().numpy())).max() <= tol["loss"] * np.sqrt(r2_ref).max()
    r, r_ref = np.sqrt(r2.cpu().double().numpy()), np.sqrt(r2_ref)
    assert np.abs(r - r_ref).max() <= tol["loss"] * np.abs(r_ref).max()
    for name, other in (("torch", [e.ravel() for e in grads]), ("two passes", two)):
        maxrel = []
        for i, exp in enumerate(other):
            exp = np.asarray(exp, np.float64).ravel()[:grads[i].size]
            d = got[i][:exp.size] - exp
            if i in ZERO_GRADS:
                assert not np.any(exp) and not np.any(got[i]), f"D weight {i} must receive exactly nothing from the penalty ({name})"
                continue
            if exp.size == 1:
                assert abs(d[0]) <= tol["grad_rms"] * abs(exp[0]) + tol["sfloor"] * max(np.abs(e).max() for e in grads), (name, i, d, exp)
            else:
                assert _rel_rms(got[i][:exp.size], exp) <= tol["grad_rms"], (name, i, _rel_rms(got[i][:exp.size], exp))
                maxrel.append(np.abs(d).max() / np.abs(exp).max())
        assert np.median(maxrel) <= tol["grad_med"], (name, sorted(maxrel))


# ---------------------------------------------------------------------------------------------------------------- the off state
def test_defaults_fetch_nothing_and_agree(ops, monkeypatch):
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 2)
    absent, off = _build(cfg, W, "f32", None, None), _build(cfg, W, "f32", "bce", False, r2_gamma=0.0)
    assert not hasattr(absent.args, "relativistic") and not hasattr(absent.args, "r2_gamma")
    assert absent.relativistic is False and absent.r2 is None and off.relativistic is False and off.r2 is None and "r2" not in off.losses
    names = called(monkeypatch, ops)
    for b in (1, 5, 12, 16):
        inp = dev_inputs(_step_inputs(cfg, b))
        absent.train_step_from_inputs(b, inp)
        off.train_step_from_inputs(b, inp)
    torch.cuda.synchronize()
    assert names and not [n for n in names if n.startswith("lgrel_")]
    assert torch.equal(absent.store.flat, off.store.flat) and torch.equal(absent.store.grad, off.store.grad)


def test_r1_alone_keeps_its_launches_and_bits(ops, monkeypatch):
    """r1_gamma alone: no lgrel_* function, the entry points of the R1 step in its order, and the bits of a trainer that never heard of
    the new keys"""
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 2)
    new, old = _build(cfg, W, "bf16", "hinge", False, r1_gamma=G1, r1_interval=1, r2_gamma=0.0), _build(cfg, W, "bf16", "hinge", None, r1_gamma=G1, r1_interval=1)
    seen = []
    for tr in (new, old):
        with monkeypatch.context() as mp_:
            names = called(mp_, ops)
            for b in (4, 12):
                tr.train_step_from_inputs(b, dev_inputs(_step_inputs(cfg, b)))
            torch.cuda.synchronize()
        seen.append(list(names))
    assert seen[0] == seen[1] and not [n for n in seen[0] if n.startswith("lgrel_")] and seen[0].count("lgr_r1_seed") == 2
    assert torch.equal(new.store.flat, old.store.flat) and torch.equal(new.store.grad, old.store.grad)
    assert torch.equal(new.losses["r1"], old.losses["r1"]) and torch.equal(new.losses["disc"], old.losses["disc"])


# ---------------------------------------------------------------------------------------------------------------- determinism, graphs
def test_recipe_steps_are_bit_identical_and_graph_replay_matches():
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 8)
    kw = dict(r1_gamma=G1, r2_gamma=G2, r1_interval=2)
    for mfma in ("f32", "bf16"):
        outs = []
        for _ in range(2):
            tr = _build(cfg, W, mfma, **kw)
            for b in (10, 11, 12):
                tr.train_step_from_inputs(b, dev_inputs(_step_inputs(cfg, b)))
            torch.cuda.synchronize()
            outs.append((tr.store.flat.cpu().clone(), tr.store.grad.cpu().clone()) + tuple(tr.losses[k].cpu().clone() for k in ("gen", "disc", "adj", "r1", "r2")))
        assert all(torch.equal(a, b) for a, b in zip(*outs)), mfma
        assert float(outs[0][5]) > 0 and float(outs[0][6]) > 0
        tg, te = _build(cfg, W, mfma, **kw), _build(cfg, W, mfma, **kw)
        steps = range(1, 9)
        kinds = [tg.step_kind(b) for b in steps]
        assert {k[2] for k in kinds} == {False, True}
        for b in steps:
            i = dev_inputs(_step_inputs(cfg, b))
            tg.graph_step(b, i)
            te.train_step_from_inputs(b, i)
            torch.cuda.synchronize()
            assert torch.equal(tg.store.flat, te.store.flat) and torch.equal(tg.store.grad, te.store.grad), (mfma, b)
            assert all(torch.equal(tg.losses[k], te.losses[k]) for k in ("gen", "disc", "r1", "r2")), (mfma, b)
        assert len(tg._graphs) == sum(1 for k in set(kinds) if kinds.count(k) >= 2)
        for pen in (False, True):   # each of the two kinds was replayed at least once (seen three times or more)
            assert max(kinds.count(k) for k in set(kinds) if k[2] == pen) >= 3


# ---------------------------------------------------------------------------------------------------------------- data parallel
DP = dict(init_dim=2, conv_filter=(64, 32, 32, 32, 32), cond_dim=5, noise_dim=11, batch_size=2)
DP_STEPS = (10, 11)
DP_KW = dict(r1_gamma=G1, r2_gamma=G2, r1_interval=1)


def _dp_inputs(cfg, world, b):
    return f32_round(O.make_inputs(cfg, cfg.batch_size * world, seed=300 + b))


def _dp_worker(rank, world, port, mfma, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = O.Cfg(**DP)
        tr = _build(cfg, perturbed(cfg, 21), mfma, **DP_KW)
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
def test_two_ranks_equal_one_rank(tmp_path, mfma):
    """each rank pairs and penalises its own rows: rank r's pairs are pairs r B .. r B + B - 1 of the double batch"""
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
    tr = _build(big, perturbed(cfg, 21), mfma, **DP_KW)
    off = _build(big, perturbed(cfg, 21), mfma, "logistic", False)
    for b in DP_STEPS:
        tr.train_step_from_inputs(b, dev_inputs(_dp_inputs(cfg, world, b)))
        off.train_step_from_inputs(b, dev_inputs(_dp_inputs(cfg, world, b)))
    torch.cuda.synchronize()
    g1 = tr.store.grad.cpu().numpy()
    gd = grad[0] / world
    tol = 2e-5 if mfma == "f32" else 2e-3
    s_, e_ = tr.store.model_range("D")
    vis = _rel_rms(off.store.grad.cpu().numpy()[s_:e_], g1[s_:e_])
    print(f"{mfma}: two ranks against one {_rel_rms(gd[s_:e_], g1[s_:e_]):.3g}, without the new keys {vis:.3g}")
    assert _rel_rms(gd[s_:e_], g1[s_:e_]) < tol
    assert vis > tol   # leaving the pairing and the penalties out moves what is compared by more than the bound


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_main_train_with_the_recipe(tmp_path):
    cfgdir = tmp_path / "cfg"
    cfgdir.mkdir()
    base = {"synthetic": True, "synthetic_images": 48, "all_result_dir": str(tmp_path / "results"), "test_data_dir": str(tmp_path / "td"),
            "batch_size": 4, "epoch": 1, "freq_gen": 2, "freq_test": 100, "mfma_dtype": "bf16", "train_adj": True, "image_dim": 32,
            "init_dim": 2, "conv_filter": [64, 32, 32, 32, 32], "noise_dim": 7, "restore": False,
            "gan_loss": "logistic", "relativistic": True, "r1_gamma": 10.0, "r2_gamma": 10.0, "r1_interval": 2}
    (cfgdir / "sample.config.json").write_text(json.dumps({"synthetic": True}))
    (cfgdir / "t.config.json").write_text(json.dumps(base))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "train", "exp", "-e", "t", "--debug"],
                       env=dict(os.environ, LITTLEGAN_CONFIG_DIR=str(cfgdir)), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if "LossD" in ln]
    assert lines
    for ln in lines:
        words = ln.split()
        assert "R1" in words and "R2" in words, ln
        vals = [float(words[words.index(k) + 1]) for k in ("LossG", "LossD", "R1", "R2")]
        assert all(np.isfinite(vals)) and vals[2] > 0 and vals[3] > 0, ln
