"""Gradient penalty (use_gp / gp_weight; this project's definition) on the GPU.

Kernels: each gp.hip entry point on its own inputs against fp64, at the encoder-level shapes the step launches (C3: bf16, B = 256;
C2: f32, B = 64) and on a small case.  Penalty: its value and D weight gradients alone against the torch float64 double-backward
oracle (tests/test_gp_cpu.py::torch_gp), then whole steps against np_oracle.step_gradients + the oracle's penalty gradients
(full step, each partition group, the Adjuster branch), bit-determinism, graph replay, two gloo ranks and the CLI.
Tolerances: the whole-step ones of tests/test_step_gpu.py (f32: median tensor 2e-5 max-abs relative, every tensor 5e-3 rms;
bf16 against fp64: 0.2 / 0.5, scalar gamma / beta bounded against the L2 of their summands)."""
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
from test_gp_cpu import np_gp, torch_gp  # noqa: E402
from test_step_gpu import TOLS, check_grads, dev_inputs, f32_round, grads_of, load_weights, perturbed  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(init_dim=2, conv_filter=(64, 32, 32, 32, 32), cond_dim=5, noise_dim=11, batch_size=3)


def _rel_rms(got, exp):
    got, exp = np.asarray(got, np.float64).ravel(), np.asarray(exp, np.float64).ravel()
    return np.sqrt(np.mean((got - exp) ** 2)) / (np.sqrt(np.mean(exp ** 2)) + 1e-30)


# ---------------------------------------------------------------------------------------------------------------- kernels
def _level(B, H, C, bf16, seed):
    """raw conv output z of a level (fp32, or its bf16 copy) with the statistics records of the fp32 values"""
    from littlegan_amd import ops
    g = torch.Generator(device="cuda").manual_seed(seed)
    z = torch.randn(B, H, H, C, device="cuda", generator=g) * 0.7 + 0.1
    gamma = torch.tensor([1.2], device="cuda")
    beta = torch.tensor([0.1], device="cuda")
    st = ops.instnorm_stats(z, gamma, beta, 0, 0.3)
    if bf16:
        z = z.to(torch.bfloat16)
    return z, st, gamma, beta


def _ref_level(z, st, gamma, alpha):
    """fp64 (c, sigma, s, m) of the kernels' own inputs: the stored z, the record's mean and sigma"""
    B = z.shape[0]
    zd = z.double().reshape(B, -1)
    std = st.double()
    c = (zd - std[:, 0:1]) - std[:, 4:5]
    sigma = std[:, 1:2]
    s = sigma + 1e-3
    n = (gamma.double() / s) * c + std[:, 3:4]
    m = torch.where(n > 0, 1.0, alpha).double()
    return c, sigma, s, m


LEVELS = [pytest.param(256, 64, 64, True, id="C3-L1-bf16"), pytest.param(256, 32, 128, True, id="C3-L2-bf16"),
          pytest.param(256, 16, 256, True, id="C3-L3-bf16"), pytest.param(256, 8, 384, True, id="C3-L4-bf16"),
          pytest.param(64, 64, 64, False, id="C2-L1-f32"), pytest.param(64, 32, 128, False, id="C2-L2-f32"),
          pytest.param(64, 16, 256, False, id="C2-L3-f32"), pytest.param(64, 8, 384, False, id="C2-L4-f32"),
          pytest.param(3, 4, 32, False, id="small-f32"), pytest.param(3, 4, 32, True, id="small-bf16")]


@pytest.mark.parametrize("B,H,C,bf16", LEVELS)
def test_norm_kernels_against_fp64(B, H, C, bf16):
    from littlegan_amd import ops
    alpha = 0.3
    z, st, gamma, _ = _level(B, H, C, bf16, 1)
    gen = torch.Generator(device="cuda").manual_seed(2)
    g = torch.randn(z.shape, device="cuda", generator=gen)
    u = torch.randn(z.shape, device="cuda", generator=gen)
    add = torch.randn(z.shape, device="cuda", generator=gen)
    dgm = torch.zeros(1, device="cuda")
    dbt = torch.zeros(1, device="cuda")
    dz = ops.gp_norm_bwd(z, st, gamma, g, alpha, add=add, dgamma=dgm, dbeta=dbt)
    dgm2 = torch.zeros(1, device="cuda")
    uh, uz2 = ops.gp_norm_dd(z, st, gamma, g, u, alpha, dgamma=dgm2)
    c, sigma, s, m = _ref_level(z, st, gamma, alpha)
    N = c.shape[1]
    gm = float(gamma)
    gn = g.double().reshape(B, -1) * m
    ud = u.double().reshape(B, -1)
    A, M = gn.mean(1, keepdim=True), (gn * c).mean(1, keepdim=True)
    dz_ref = (gm / s) * (gn - A - c * M / (s * sigma)) + add.double().reshape(B, -1)
    U, P = ud.sum(1, keepdim=True), (ud * c).sum(1, keepdim=True)
    T1 = (ud * gn).sum(1, keepdim=True) - A * U
    uh_ref = m * (gm / s) * (ud - U / N - c * (P / N) / (s * sigma))
    uz_ref = (-gm * T1 * c / (N * s ** 2 * sigma) - gm / (s ** 2 * sigma) * (P * (gn - A) / N + M * (ud - U / N))
              + gm * M * P * (2 / s + 1 / sigma) * c / (N * s ** 2 * sigma ** 2))
    for got, ref in ((dz, dz_ref), (uh, uh_ref), (uz2, uz_ref)):
        assert _rel_rms(got.double().reshape(B, -1).cpu(), ref.cpu()) < 1e-5
    # scalars: against the L2 norm of their summands
    tg, tb = gn * c / s, gn
    for got, exp, l2 in ((dgm, (gn * c / s).sum(), tg.norm()), (dbt, gn.sum(), tb.norm()),
                         (dgm2, ((T1 - M * P / (s * sigma)) / s).sum(), ((ud * gn) / s).norm() + (ud * c * M / (s * s * sigma)).norm())):
        assert abs(float(got) - float(exp)) <= 1e-5 * abs(float(exp)) + 1e-6 * float(l2), (float(got), float(exp))
    # bf16 mirror of dz: the RNE rounding of the fp32 result
    dz16 = torch.empty(z.shape, dtype=torch.bfloat16, device="cuda")
    ops.gp_norm_bwd(z, st, gamma, g, alpha, add=add, out16=dz16, want_f32=False)
    assert torch.equal(dz16, dz.to(torch.bfloat16))


@pytest.mark.parametrize("B,H", [(256, 128), (64, 128), (3, 32)])
def test_interp_seed_and_heads_kernels_against_fp64(B, H):
    from littlegan_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(5)
    real = torch.rand(B, H, H, 3, device="cuda", generator=gen) * 2 - 1
    fake = torch.rand(B, H, H, 3, device="cuda", generator=gen) * 2 - 1
    eps = torch.rand(B, device="cuda", generator=gen)
    xh = ops.gp_interp(real, fake, eps)
    e = eps.double().view(B, 1, 1, 1)
    assert (xh.double() - (e * real.double() + (1 - e) * fake.double())).abs().max() < 1e-6
    g = torch.randn(B, H, H, 3, device="cuda", generator=gen) * 0.02
    g[0] = 0.0   # r = 0: the seed factor is 0, not NaN
    loss = torch.full((1,), 0.5, device="cuda")
    gp_loss = torch.zeros(1, device="cuda")
    u0, r = ops.gp_seed(g, 5.0, loss, gp_loss)
    rd = g.double().reshape(B, -1).norm(dim=1)
    term = 5.0 * ((rd - 1) ** 2).mean()
    assert (r.double() - rd).abs().max() < 1e-6 * rd.max()
    assert abs(float(gp_loss) - float(term)) < 1e-6 * float(term) and abs(float(loss) - 0.5 - float(term)) < 1e-6 * float(term)
    k = (2 * 5.0 / B) * (rd - 1) / rd.clamp(min=1e-12)
    assert torch.isfinite(u0).all() and _rel_rms(u0.double().cpu(), (k.view(B, 1, 1, 1) * g.double()).cpu()) < 1e-6
    # heads, at K = 8 x 8 x 384 (the step's), c = 40
    K, c = 8 * 8 * 384, 40
    p = torch.rand(B, 1 + c, device="cuda", generator=gen) * 0.9 + 0.05
    wpr = torch.randn(K, 1, device="cuda", generator=gen) * 0.01
    x = torch.randn(B, K, device="cuda", generator=gen)
    uu = torch.randn(B, K, device="cuda", generator=gen)
    gs = ops.gp_heads_seed(p, wpr)
    pd = p[:, 0].double()
    sp, spp = pd * (1 - pd), pd * (1 - pd) * (1 - 2 * pd)
    assert _rel_rms(gs.double().cpu(), (sp[:, None] * wpr.double().view(1, K)).cpu()) < 1e-6
    dw = torch.full((K, 1), 0.25, device="cuda")
    db = torch.full((1,), -0.5, device="cuda")
    t, g2 = ops.gp_heads_2nd(p, wpr, x, uu, dwpr=dw, dbpr=db)
    td = spp * (uu.double() @ wpr.double().view(K))
    assert _rel_rms(t.double().cpu(), td.cpu()) < 1e-6
    assert _rel_rms(g2.double().cpu(), (td[:, None] * wpr.double().view(1, K)).cpu()) < 1e-6
    dwd = 0.25 + (sp[:, None] * uu.double()).sum(0) + x.double().T @ td
    assert _rel_rms(dw.double().view(K).cpu(), dwd.cpu()) < 1e-6
    assert abs(float(db) - (-0.5 + float(td.sum()))) < 1e-5 * float(td.abs().sum())


# ---------------------------------------------------------------------------------------------------------------- penalty
def _build_gp(cfg, W, mfma, gp_weight=5.0):
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    import test_step_gpu as T
    args = T.make_args(cfg, mfma)
    args.use_gp, args.gp_weight = True, gp_weight
    decoder, encoder = Decoder(args), Encoder(args)
    g = Generator(args, decoder)
    d = Discriminator(args, encoder)
    tr = EagerTrainer(args, g, d, Adjuster(args, d, g), None)
    load_weights(tr, W)
    return tr


def _xhat(cfg, seed):
    rng = np.random.default_rng(seed)
    shp = (cfg.batch_size, cfg.image_dim, cfg.image_dim, 3)
    real, fake = rng.uniform(-1, 1, shp), rng.uniform(-1, 1, shp)
    eps = rng.uniform(0, 1, cfg.batch_size)
    return [a.astype(np.float32).astype(np.float64) for a in (real, fake, eps)]


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_penalty_alone_against_torch_double_backward(mfma):
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 4)
    tr = _build_gp(cfg, W, mfma)
    real, fake, eps = _xhat(cfg, 9)
    from littlegan_amd import ops
    tr.store.grad.zero_()
    xh = ops.gp_interp(*(torch.tensor(a, dtype=torch.float32, device="cuda").contiguous() for a in (real, fake, eps)))
    loss = torch.zeros(1, device="cuda")
    r = tr.discriminator.gradient_penalty(xh, 5.0, loss, tr.losses["gp"])
    xhat = eps[:, None, None, None] * real + (1 - eps[:, None, None, None]) * fake
    term, r_ref, grads = torch_gp(cfg, W["D"], xhat, 5.0)
    tol = TOLS[mfma]
    assert abs(float(tr.losses["gp"]) - term) <= tol["loss"] * abs(term) and float(loss) == float(tr.losses["gp"])
    assert np.abs(r.cpu().numpy() - r_ref).max() <= tol["loss"] * np.abs(r_ref).max()
    got = grads_of(tr, "D")
    maxrel = []
    for i, exp in enumerate(grads):
        exp = exp.ravel()
        d = got[i][:exp.size] - exp
        if i in (18, 19):
            assert not np.any(got[i]), "dense_cond must receive nothing from the penalty"
            continue
        if exp.size == 1:
            assert abs(d[0]) <= tol["grad_rms"] * abs(exp[0]) + tol["sfloor"] * max(np.abs(e).max() for e in grads), (i, d, exp)
        else:
            assert _rel_rms(got[i][:exp.size], exp) <= tol["grad_rms"], (i, _rel_rms(got[i][:exp.size], exp))
            maxrel.append(np.abs(d).max() / np.abs(exp).max())
    assert np.median(maxrel) <= tol["grad_med"], sorted(maxrel)


def _step_inputs(cfg, b):
    inp = f32_round(O.make_inputs(cfg, cfg.batch_size, seed=70 + b))
    inp["gp_eps"] = np.random.default_rng(b).uniform(0, 1, cfg.batch_size).astype(np.float32).astype(np.float64)
    return inp


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_whole_step_with_penalty_matches_oracle(mfma):
    """b = 4 full step, 5 / 10 / 15 the three partition groups of D, 11 full step with the Adjuster branch."""
    tol = TOLS[mfma]
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 6)
    tr = _build_gp(cfg, W, mfma)
    for b in (4, 5, 10, 11, 15):
        inp = _step_inputs(cfg, b)
        load_weights(tr, W)
        fake, adj, lg, ld, la = tr.train_step_from_inputs(b, dev_inputs(inp))
        ref = O.step_gradients(cfg, W, b, {k: v for k, v in inp.items() if k != "gp_eps"})
        e = inp["gp_eps"][:, None, None, None]
        xhat = e * inp["new_image"] + (1 - e) * fake.cpu().double().numpy()
        term, _, gpg = np_gp(cfg, W["D"], xhat, 5.0)
        ref["dD"] = [a + g for a, g in zip(ref["dD"], gpg)]
        assert abs(ld.item() - (ref["disc_loss"] + term)) < tol["loss"] * abs(ref["disc_loss"] + term), (b, ld.item(), ref["disc_loss"], term)
        assert abs(float(tr.losses["gp"]) - term) < max(tol["loss"], 1e-4) * abs(term) + 1e-7
        only = {m: O.train_weight_indices(cfg, m, b) for m in "GDA"}
        sets = [("D", "dD"), ("G", "dG")] + ([("A", "dA")] if b > 10 else [])
        check_grads(tr, ref, sets, tol, tag=f"gp b={b}", only=only)


def test_penalty_steps_are_bit_identical_and_graph_replay_matches():
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 8)
    for mfma in ("f32", "bf16"):
        tr = _build_gp(cfg, W, mfma)
        inp = dev_inputs(_step_inputs(cfg, 4))
        outs = []
        for _ in range(3):
            load_weights(tr, W)
            tr.train_step_from_inputs(4, inp)
            torch.cuda.synchronize()
            # (the weights after Adam differ: the Adam slots and beta powers move on from step to step)
            outs.append((tr.store.grad.cpu().clone(), tr.losses["disc"].cpu().clone(), tr.losses["gp"].cpu().clone()))
        for o in outs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(outs[0], o)), mfma
        # graph replay: step 1 eager, step 2 captured + replayed, against the same eager steps of a second trainer
        tg, te = _build_gp(cfg, W, mfma), _build_gp(cfg, W, mfma)
        for b in (1, 2, 3):
            i = dev_inputs(_step_inputs(cfg, b))
            tg.graph_step(b, i)
            te.train_step_from_inputs(b, i)
        torch.cuda.synchronize()
        assert torch.equal(tg.store.flat, te.store.flat) and torch.equal(tg.store.grad, te.store.grad), mfma
        assert torch.equal(tg.losses["gp"], te.losses["gp"]) and torch.equal(tg.losses["disc"], te.losses["disc"])


def test_missing_eps_is_an_error():
    cfg = O.Cfg(**SMALL)
    tr = _build_gp(cfg, perturbed(cfg, 1), "f32")
    inp = _step_inputs(cfg, 4)
    del inp["gp_eps"]
    with pytest.raises(ValueError, match="gp_eps"):
        tr.train_step_from_inputs(4, dev_inputs(inp))


# ---------------------------------------------------------------------------------------------------------------- data parallel
DP = dict(init_dim=2, conv_filter=(64, 32, 32, 32, 32), cond_dim=5, noise_dim=11, batch_size=2)
DP_STEPS = (10, 11)


def _dp_inputs(cfg, world, b):
    inp = f32_round(O.make_inputs(cfg, cfg.batch_size * world, seed=300 + b))
    inp["gp_eps"] = np.random.default_rng(b).uniform(0, 1, cfg.batch_size * world).astype(np.float32).astype(np.float64)
    return inp


def _dp_worker(rank, world, port, mfma, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = O.Cfg(**DP)
        tr = _build_gp(cfg, perturbed(cfg, 21), mfma)
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
    tr = _build_gp(O.Cfg(**{**DP, "batch_size": cfg.batch_size * world}), perturbed(cfg, 21), mfma)
    for b in DP_STEPS:
        tr.train_step_from_inputs(b, dev_inputs(_dp_inputs(cfg, world, b)))
    torch.cuda.synchronize()
    g1 = tr.store.grad.cpu().numpy()
    gd = grad[0] / world
    tol = 2e-5 if mfma == "f32" else 2e-3
    s_, e_ = tr.store.model_range("D")
    assert _rel_rms(gd[s_:e_], g1[s_:e_]) < tol


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_main_train_with_penalty(tmp_path):
    cfgdir = tmp_path / "cfg"
    cfgdir.mkdir()
    res = tmp_path / "results"
    (cfgdir / "sample.config.json").write_text(json.dumps({"synthetic": True}))
    (cfgdir / "t.config.json").write_text(json.dumps({
        "synthetic": True, "synthetic_images": 48, "all_result_dir": str(res), "test_data_dir": str(tmp_path / "td"),
        "batch_size": 4, "epoch": 1, "freq_gen": 2, "freq_test": 100, "mfma_dtype": "bf16", "train_adj": True, "image_dim": 32,
        "init_dim": 2, "conv_filter": [64, 32, 32, 32, 32], "noise_dim": 7, "use_gp": True, "gp_weight": 5.0, "restore": False}))
    env = dict(os.environ, LITTLEGAN_CONFIG_DIR=str(cfgdir))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "train", "exp", "-e", "t", "--debug"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if "LossD" in ln]
    assert lines
    for ln in lines:
        vals = [float(v) for v in ln.split()[2::2]][:2]   # LossG, LossD (LossA is nan before the Adjuster branch starts)
        assert all(np.isfinite(vals)), ln
