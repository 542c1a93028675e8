"""R1 gradient penalty (r1_gamma / r1_interval; this project's definition) on the GPU.

Kernels: the three lgr_* entry points bit for bit in exact arithmetic (integers in [-4, 4] times a power of two, weight and B powers of
two: tests/test_r1_cpu.py::test_conditions_of_the_exact_cases) at every chunk / slab edge, as launched, repeated and under a one-CU
budget; on random fp32 data against fp64 (the bounds of tests/test_gp_gpu.py).  (Their memory contract: the r1-* rows of
tests/test_memory_contract_gpu.py, on this module's data.)
Penalty: its value and D weight gradients alone against the torch float64 double-backward oracle (tests/test_r1_cpu.py::torch_r1),
then whole steps against np_oracle.step_gradients + np_r1 (full step, each partition group, the Adjuster branch, under diff_augment
and a fixed augmentation probability), the lazy interval, bit-determinism, graph replay, the defaults, two gloo ranks and the CLI.
Tolerances: the whole-step ones of tests/test_step_gpu.py."""
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
from test_r1_cpu import (COLSUM_SHAPES, EXACT_LOSS0, EXACT_WEIGHT, HEADS_SEED_SHAPES, SEED_SHAPES, ZERO_GRADS, exact_colsum_case,  # noqa: E402
                         exact_seed_case, heads_seed_wpr, np_r1, torch_r1)
from test_step_gpu import TOLS, check_grads, dev_inputs, f32_round, grads_of, load_weights, make_args, perturbed  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(init_dim=2, conv_filter=(64, 32, 32, 32, 32), cond_dim=5, noise_dim=11, batch_size=3)   # = tests/test_gp_gpu.py's
GAMMA = 10.0


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


class one_cu:
    """While active the persistent grids are sized to ONE compute unit (lg_set_reserved_cus); the budget found is put back"""

    def __init__(self, ops):
        self.lib = ops._lib.load()

    def __enter__(self):
        self.was = self.lib.lg_device_cus() - self.lib.lg_grid_cus()
        assert self.lib.lg_set_reserved_cus(self.lib.lg_device_cus() - 1) == 0 and self.lib.lg_grid_cus() == 1

    def __exit__(self, *exc):
        assert self.lib.lg_set_reserved_cus(self.was) == 0


# ---------------------------------------------------------------------------------------------------------------- kernels, exact
@pytest.mark.parametrize("B,L", SEED_SHAPES, ids=lambda v: str(v))
def test_seed_is_exact_at_every_chunk_edge(ops, B, L):
    g, u0_w, r2_w, term_w, loss_w = exact_seed_case(B, L)
    gd = dev(g)

    def run(with_loss=True, with_r1=True):
        loss = torch.full((1,), EXACT_LOSS0, device="cuda") if with_loss else None
        r1l = torch.full((1,), -7.0, device="cuda") if with_r1 else None
        ops._lib.load().lg_clear_kernel()
        u0, r2 = ops.r1_seed(gd, EXACT_WEIGHT, loss, r1l)
        assert ops.last_kernel() == "r1_seed_kernel"
        torch.cuda.synchronize()
        return u0, r2, loss, r1l

    runs = [run(), run()]
    with one_cu(ops):
        runs.append(run())
    for u0, r2, loss, r1l in runs:
        assert np.array_equal(_bits(u0), _np_bits(u0_w))
        assert np.array_equal(_bits(r2), _np_bits(r2_w))
        assert np.array_equal(_bits(r1l), _np_bits([term_w])) and np.array_equal(_bits(loss), _np_bits([loss_w]))
    assert torch.equal(gd.cpu(), torch.from_numpy(g))
    # each of loss / r1_loss may be null: the other results are the same bits
    for with_loss, with_r1 in ((False, True), (True, False), (False, False)):
        u0, r2, loss, r1l = run(with_loss, with_r1)
        assert np.array_equal(_bits(u0), _np_bits(u0_w)) and np.array_equal(_bits(r2), _np_bits(r2_w))
        assert loss is None or np.array_equal(_bits(loss), _np_bits([loss_w]))
        assert r1l is None or np.array_equal(_bits(r1l), _np_bits([term_w]))


@pytest.mark.parametrize("B,K", COLSUM_SHAPES, ids=lambda v: str(v))
def test_colsum_is_exact_at_every_slab_edge(ops, B, K):
    u, d0, want = exact_colsum_case(B, K)
    ud = dev(u)

    def run():
        dw = dev(d0)
        ops._lib.load().lg_clear_kernel()
        assert ops.r1_heads_colsum(ud, dw) is dw and ops.last_kernel() == "r1_colsum_kernel"
        torch.cuda.synchronize()
        return dw

    runs = [run(), run()]
    with one_cu(ops):
        runs.append(run())
    for dw in runs:
        assert np.array_equal(_bits(dw), _np_bits(want))
    assert torch.equal(ud.cpu(), torch.from_numpy(u))


@pytest.mark.parametrize("B,K", HEADS_SEED_SHAPES, ids=lambda v: str(v))
def test_heads_seed_copies_every_row_bit_for_bit(ops, B, K):
    w = heads_seed_wpr(K)
    wd = dev(w).view(K, 1)
    assert np.array_equal(_bits(wd).ravel(), w.view(np.int32))   # the NaN's payload and the -0.0 reached the device
    ops._lib.load().lg_clear_kernel()
    g = ops.r1_heads_seed(wd, B)
    assert ops.last_kernel() == ("r1_heads_seed_kernel<v4>" if K % 4 == 0 else "r1_heads_seed_kernel<v1>")
    with one_cu(ops):
        g1 = ops.r1_heads_seed(wd, B)
    torch.cuda.synchronize()
    assert tuple(g.shape) == (B, K)
    for got in (g, g1):
        assert np.array_equal(_bits(got), np.broadcast_to(w.view(np.int32), (B, K)))


# ---------------------------------------------------------------------------------------------------------------- kernels, fp32 data
@pytest.mark.parametrize("B,L", [(3, 3072), (256, 49152)], ids=lambda v: str(v))
def test_kernels_on_random_data_against_fp64(ops, B, L):
    gen = torch.Generator(device="cuda").manual_seed(B + L)
    g = torch.randn(B, L, device="cuda", generator=gen) * 0.02
    w = 160.0
    loss, r1l = torch.full((1,), 0.5, device="cuda"), torch.zeros(1, device="cuda")
    u0, r2 = ops.r1_seed(g, w, loss, r1l)
    gd = g.double()
    r2d = (gd ** 2).sum(1)
    term = 0.5 * w * float(r2d.mean())
    assert _rel_rms(u0.double().cpu(), ((w / B) * gd).cpu()) < 1e-5
    assert _rel_rms(r2.double().cpu(), r2d.cpu()) < 1e-5
    l2 = float((0.5 * w / B) * (gd ** 2).norm())   # the L2 of the term's summands
    print(f"({B}, {L}): term {float(r1l):.9g} / fp64 {term:.9g}, loss {float(loss):.9g}")
    assert abs(float(r1l) - term) <= 1e-5 * abs(term) + 1e-6 * l2
    assert abs(float(loss) - (0.5 + term)) <= 1e-5 * abs(0.5 + term) + 1e-6 * l2
    # the heads' column sum and seed, at (B, K) = the same pair
    K = L
    u = torch.randn(B, K, device="cuda", generator=gen)
    dw0 = torch.randn(K, 1, device="cuda", generator=gen)
    dw = dw0.clone()
    ops.r1_heads_colsum(u, dw)
    assert _rel_rms(dw.double().view(K).cpu(), (dw0.double().view(K) + u.double().sum(0)).cpu()) < 1e-5
    wpr = torch.randn(K, 1, device="cuda", generator=gen)
    gs = ops.r1_heads_seed(wpr, B)
    assert torch.equal(gs, wpr.view(1, K).expand(B, K))


def test_wrappers_refuse_wrong_shapes(ops):
    g = torch.zeros(2, 16, device="cuda")
    with pytest.raises(ValueError):
        ops.r1_seed(g, 1.0, torch.zeros(2, device="cuda"))
    with pytest.raises(ValueError):
        ops.r1_seed(g.double(), 1.0)
    with pytest.raises(ValueError):
        ops.r1_heads_colsum(g, torch.zeros(8, 1, device="cuda"))
    with pytest.raises(ValueError):
        ops.r1_heads_seed(torch.zeros(16, device="cuda"), 2)
    with pytest.raises(ops._lib.LittleGanHipError, match="lgr_r1_seed"):
        ops.r1_seed(torch.zeros(2, 6, device="cuda"), 1.0)            # L % 4 != 0: refused by the library, before any launch
    with pytest.raises(ops._lib.LittleGanHipError, match="lgr_r1_seed"):
        ops.r1_seed(g, float("nan"))


# ---------------------------------------------------------------------------------------------------------------- penalty
def _build_r1(cfg, W, mfma, r1_gamma=GAMMA, r1_interval=1, **kw):
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    args = make_args(cfg, mfma)
    if r1_gamma is not None:
        args.r1_gamma, args.r1_interval = r1_gamma, r1_interval
    for k, v in kw.items():
        setattr(args, k, v)
    decoder, encoder = Decoder(args), Encoder(args)
    g = Generator(args, decoder)
    d = Discriminator(args, encoder)
    tr = EagerTrainer(args, g, d, Adjuster(args, d, g), None)
    load_weights(tr, W)
    return tr


_ALONE = {}


def _alone_reference():
    """computed once, shared by the f32 and bf16 cases: the weights and the input of tests/test_gp_gpu.py's penalty-alone test (its
    interpolate of two uniform images), so that the two penalties are held to the same bounds on the same data"""
    if not _ALONE:
        cfg = O.Cfg(**SMALL)
        W = perturbed(cfg, 4)
        rng = np.random.default_rng(9)
        shp = (cfg.batch_size, cfg.image_dim, cfg.image_dim, 3)
        real, fake, eps = (a.astype(np.float32).astype(np.float64) for a in (rng.uniform(-1, 1, shp), rng.uniform(-1, 1, shp),
                                                                             rng.uniform(0, 1, cfg.batch_size)))
        e = eps[:, None, None, None]
        x = (e * real + (1 - e) * fake).astype(np.float32).astype(np.float64)
        _ALONE["v"] = (cfg, W, x, torch_r1(cfg, W["D"], x, GAMMA))
    return _ALONE["v"]


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_penalty_alone_against_torch_double_backward(mfma):
    """The assertions of tests/test_gp_gpu.py::test_penalty_alone_against_torch_double_backward.  That test bounds the gradient NORM
    r_b = |g_b| by tol * max r; the kernel here returns r2_b = r_b^2, whose relative error is twice the norm's, so the same bound is
    put on sqrt(r2_b): the same quantity held to the same tolerance."""
    cfg, W, x, (term, r2_ref, grads) = _alone_reference()
    tr = _build_r1(cfg, W, mfma)
    tr.store.grad.zero_()
    loss = torch.zeros(1, device="cuda")
    r2 = tr.discriminator.r1_penalty(dev(x), GAMMA, loss, tr.losses["r1"])
    torch.cuda.synchronize()
    tol = TOLS[mfma]
    print(f"{mfma}: term {float(tr.losses['r1']):.8g} / oracle {term:.8g}")
    assert abs(float(tr.losses["r1"]) - term) <= tol["loss"] * abs(term) and float(loss) == float(tr.losses["r1"])
    r, r_ref = np.sqrt(r2.cpu().double().numpy()), np.sqrt(r2_ref)
    print(f"{mfma}: |g| {r} / oracle {r_ref}")
    assert np.abs(r - r_ref).max() <= tol["loss"] * np.abs(r_ref).max()
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


def _step_inputs(cfg, b):
    return f32_round(O.make_inputs(cfg, cfg.batch_size, seed=70 + b))


def _with_r1(ref, cfg, W, x, weight):
    term, _, g = np_r1(cfg, W["D"], x, weight)
    out = dict(ref)
    out["dD"] = [a + d for a, d in zip(ref["dD"], g)]
    return out, term


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_whole_step_with_penalty_matches_oracle(mfma):
    """r1_interval 1: b = 4 full step, 5 / 10 / 15 the three partition groups of D, 11 full step with the Adjuster branch."""
    tol = TOLS[mfma]
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 6)
    tr = _build_r1(cfg, W, mfma)
    for b in (4, 5, 10, 11, 15):
        inp = _step_inputs(cfg, b)
        load_weights(tr, W)
        fake, adj, lg, ld, la = tr.train_step_from_inputs(b, dev_inputs(inp))
        ref, term = _with_r1(O.step_gradients(cfg, W, b, inp), cfg, W, inp["new_image"], GAMMA)
        want = ref["disc_loss"] + term
        print(f"{mfma} b={b}: disc {ld.item():.7g} / {want:.7g}, r1 {float(tr.losses['r1']):.7g} / {term:.7g}")
        assert abs(ld.item() - want) < tol["loss"] * abs(want), (b, ld.item(), ref["disc_loss"], term)
        assert abs(float(tr.losses["r1"]) - term) < max(tol["loss"], 1e-4) * abs(term) + 1e-7
        only = {m: O.train_weight_indices(cfg, m, b) for m in "GDA"}
        sets = [("D", "dD"), ("G", "dG")] + ([("A", "dA")] if b > 10 else [])
        check_grads(tr, ref, sets, tol, tag=f"r1 b={b}", only=only)


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_lazy_interval(ops, monkeypatch, mfma):
    """r1_interval 2: b = 3 carries no penalty (no lgr_* function is fetched, losses["r1"] stays, the gradients are those of a trainer
    without R1 bit for bit), b = 4 carries it with weight 2 r1_gamma."""
    tol = TOLS[mfma]
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 6)
    tr, off = _build_r1(cfg, W, mfma, r1_interval=2), _build_r1(cfg, W, mfma, r1_gamma=None)
    assert tr.r1["weight"] == 2 * GAMMA and off.r1 is None
    tr.losses["r1"].fill_(7.0)
    inp = dev_inputs(_step_inputs(cfg, 3))
    with monkeypatch.context() as mp_:
        names = called(mp_, ops)
        tr.train_step_from_inputs(3, inp)
        off.train_step_from_inputs(3, inp)
        torch.cuda.synchronize()
    assert not [n for n in names if n.startswith("lgr_")] and float(tr.losses["r1"]) == 7.0
    assert torch.equal(tr.store.grad, off.store.grad) and torch.equal(tr.store.flat, off.store.flat)
    assert torch.equal(tr.losses["disc"], off.losses["disc"])
    host = _step_inputs(cfg, 4)
    load_weights(tr, W)
    with monkeypatch.context() as mp_:
        names = called(mp_, ops)
        _, _, _, ld, _ = tr.train_step_from_inputs(4, dev_inputs(host))
        torch.cuda.synchronize()
    assert {"lgr_r1_heads_seed", "lgr_r1_seed", "lgr_r1_heads_colsum"} <= set(names)
    ref, term = _with_r1(O.step_gradients(cfg, W, 4, host), cfg, W, host["new_image"], 2 * GAMMA)
    assert abs(float(tr.losses["r1"]) - term) < max(tol["loss"], 1e-4) * abs(term) + 1e-7
    assert abs(ld.item() - (ref["disc_loss"] + term)) < tol["loss"] * abs(ref["disc_loss"] + term)
    check_grads(tr, ref, [("D", "dD"), ("G", "dG")], tol, tag="r1 lazy b=4", only={m: O.train_weight_indices(cfg, m, 4) for m in "GDA"})


@pytest.mark.parametrize("gated", [False, True], ids=["diff_augment", "diff_augment_p"])
@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_step_under_augmentation(ops, mfma, gated):
    """The penalty under diff_augment is taken on T(new_image), with respect to it: the reference is the augmenting oracle of
    tests/test_diffaug_gpu.py (tests/test_ada_gpu.py's at p = 0.5) plus np_r1 on the device's own T(new_image), read back."""
    from test_diffaug_gpu import FULL, build_aug, dev_key, step_reference
    tol = TOLS[mfma]
    b = 1
    cfg, W, inp, _, ref, _ = step_reference(b)
    B, S = cfg.batch_size, 16 * cfg.init_dim
    if gated:
        from test_ada_gpu import gated_reference
        _, ref = gated_reference(b)
    kw = dict(diff_augment_p=0.5) if gated else {}
    tr = build_aug(cfg, W, mfma, r1_gamma=GAMMA, r1_interval=1, **kw)
    key = dev_key(0, 0, 3)
    di = dev_inputs(inp)
    fake, adj, lg, ld, la = tr.train_step_from_inputs(b, dict(di, diffaug_key=key))
    bits = tr.diffaug
    par = ops.diffaug_draw_gated(key, 0, 0, B, S, bits, ops.ada_init(0.5, device="cuda")) if gated else ops.diffaug_draw(key, 0, 0, B, S, bits)
    x_aug = ops.diffaug_fwd(di["new_image"], par)
    torch.cuda.synchronize()
    assert FULL == "color,translation,cutout" and not torch.equal(x_aug, di["new_image"])
    ref2, term = _with_r1(ref, cfg, W, x_aug.cpu().double().numpy(), GAMMA)
    want = ref["disc_loss"] + term
    print(f"{mfma} gated={gated}: disc {ld.item():.7g} / {want:.7g}, r1 {float(tr.losses['r1']):.7g} / {term:.7g}")
    assert abs(lg.item() - ref["gen_loss"]) < tol["loss"] * abs(ref["gen_loss"])
    assert abs(ld.item() - want) < tol["loss"] * abs(want)
    assert abs(float(tr.losses["r1"]) - term) < max(tol["loss"], 1e-4) * abs(term) + 1e-7
    check_grads(tr, ref2, [("D", "dD"), ("G", "dG")], tol, tag=f"r1 aug {mfma}", only={m: O.train_weight_indices(cfg, m, b) for m in "GDA"})


# ---------------------------------------------------------------------------------------------------------------- determinism, graphs
def test_penalty_steps_are_bit_identical_and_graph_replay_matches():
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 8)
    for mfma in ("f32", "bf16"):
        tr = _build_r1(cfg, W, mfma)
        inp = dev_inputs(_step_inputs(cfg, 4))
        outs = []
        for _ in range(3):
            load_weights(tr, W)
            tr.train_step_from_inputs(4, inp)
            torch.cuda.synchronize()
            outs.append((tr.store.grad.cpu().clone(), tr.losses["disc"].cpu().clone(), tr.losses["r1"].cpu().clone()))
        for o in outs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(outs[0], o)), mfma
        assert float(outs[0][2]) > 0
        # graph replay with the lazy interval: every kind eager once, captured at its second step, replayed afterwards
        tg, te = _build_r1(cfg, W, mfma, r1_interval=2), _build_r1(cfg, W, mfma, r1_interval=2)
        steps = range(1, 9)
        kinds = [tg.step_kind(b) for b in steps]
        assert {k[2] for k in kinds} == {False, True}
        for b in steps:
            i = dev_inputs(_step_inputs(cfg, b))
            tg.graph_step(b, i)
            te.train_step_from_inputs(b, i)
            torch.cuda.synchronize()
            assert torch.equal(tg.store.flat, te.store.flat) and torch.equal(tg.store.grad, te.store.grad), (mfma, b)
            assert torch.equal(tg.losses["r1"], te.losses["r1"]) and torch.equal(tg.losses["disc"], te.losses["disc"]), (mfma, b)
        assert len(tg._graphs) == sum(1 for k in set(kinds) if kinds.count(k) >= 2)
        for pen in (False, True):   # each of the two kinds was replayed at least once (seen three times or more)
            assert max(kinds.count(k) for k in set(kinds) if k[2] == pen) >= 3


def test_defaults_fetch_nothing_and_agree(ops, monkeypatch):
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 2)
    absent, zero = _build_r1(cfg, W, "f32", r1_gamma=None), _build_r1(cfg, W, "f32", r1_gamma=0, r1_interval=1)
    assert not hasattr(absent.args, "r1_gamma") and absent.r1 is None and zero.r1 is None
    assert "r1" not in absent.losses and "r1" not in zero.losses
    names = called(monkeypatch, ops)
    for b in (1, 2, 16):
        inp = dev_inputs(_step_inputs(cfg, b))
        absent.train_step_from_inputs(b, inp)
        zero.train_step_from_inputs(b, inp)
    torch.cuda.synchronize()
    assert names and not [n for n in names if n.startswith("lgr_")]
    assert torch.equal(absent.store.flat, zero.store.flat) and torch.equal(absent.store.grad, zero.store.grad)


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
        tr = _build_r1(cfg, perturbed(cfg, 21), mfma)
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
def test_two_ranks_with_penalty_equal_one_rank(tmp_path, mfma):
    """each rank penalises its own B rows: the all-reduced mean of the two is the penalty of the double batch"""
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
    tr = _build_r1(O.Cfg(**{**DP, "batch_size": cfg.batch_size * world}), perturbed(cfg, 21), mfma)
    off = _build_r1(O.Cfg(**{**DP, "batch_size": cfg.batch_size * world}), perturbed(cfg, 21), mfma, r1_gamma=None)
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
    print(f"{mfma}: two ranks against one {_rel_rms(gd[s_:e_], g1[s_:e_]):.3g}, without the penalty {vis:.3g}")
    assert vis > tol   # leaving the penalty out moves what is compared by more than the bound: the comparison sees it


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_main_train_with_r1(tmp_path):
    cfgdir = tmp_path / "cfg"
    cfgdir.mkdir()
    res = tmp_path / "results"
    base = {"synthetic": True, "synthetic_images": 48, "all_result_dir": str(res), "test_data_dir": str(tmp_path / "td"),
            "batch_size": 4, "epoch": 1, "freq_gen": 2, "freq_test": 100, "mfma_dtype": "bf16", "train_adj": True, "image_dim": 32,
            "init_dim": 2, "conv_filter": [64, 32, 32, 32, 32], "noise_dim": 7, "r1_gamma": 10.0, "r1_interval": 2}
    (cfgdir / "sample.config.json").write_text(json.dumps({"synthetic": True}))
    (cfgdir / "t.config.json").write_text(json.dumps(dict(base, restore=False)))
    (cfgdir / "u.config.json").write_text(json.dumps(dict(base, restore=True)))
    env = dict(os.environ, LITTLEGAN_CONFIG_DIR=str(cfgdir))
    for name, restored in (("t", False), ("u", True)):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "train", "exp", "-e", name, "--debug"], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        assert ("Loading Checkpoint..." in r.stdout) == restored, r.stdout[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if "LossD" in ln]
        assert lines
        for ln in lines:
            words = ln.split()
            assert "R1" in words, ln
            vals = [float(words[words.index(k) + 1]) for k in ("LossG", "LossD", "R1")]
            assert all(np.isfinite(vals)) and vals[2] > 0, ln
