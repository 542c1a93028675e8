"""R1 gradient penalty (r1_gamma / r1_interval) without a GPU: a float64 numpy restatement of the pass the kernels
implement, checked against torch autograd double backward on the logit of oracle.torch_oracle.Net; the entry points of
include/littlegan_hip_reg.h (the names; validating before any launch; the sizing functions: the whole ABI is held to its table and
its ledger by tests/test_abi.py and tests/test_guards_cpu.py); the configuration and the trainer's refusals; and the data of the
exact-arithmetic kernel cases of tests/test_r1_gpu.py with the conditions under which "bit for bit" is a fair demand.

The penalty is this project's definition (the reference has none):
  x_b = row b of D's real batch,  l_b = <w_pr, h4(x_b)> + b_pr (pre-sigmoid),  g_b = dl_b/dx_b,  r2_b = |g_b|^2,
  r1 = (weight / 2) mean_b r2_b,  weight = r1_gamma * r1_interval,  disc_loss += r1 on steps with batch_no % r1_interval == 0.
`np_r1` below is also the oracle of tests/test_r1_gpu.py."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import np_oracle as O  # noqa: E402
from test_abi import ROOT, _protos  # noqa: E402
from test_diffaug_cpu import _cpu_trainer  # noqa: E402
from test_gp_cpu import TINY, _norm_dd, _tiny_case  # noqa: E402

REG_HEADER = os.path.join(ROOT, "include", "littlegan_hip_reg.h")
ENTRY_POINTS = ("lgr_r1_workspace_bytes", "lgr_r1_heads_seed", "lgr_r1_seed", "lgr_r1_colsum_workspace_bytes", "lgr_r1_heads_colsum")
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatement of the seven steps: np_gp of tests/test_gp_cpu.py with the sigmoid taken out
def np_r1(cfg, Wd, x_in, weight):
    """-> ((weight / 2) mean r2, r2 [B], 20 gradients of the term w.r.t. Discriminator.weights), all float64"""
    a = cfg.leaky_alpha
    B = x_in.shape[0]
    xs, caches = [], []
    x = np.asarray(x_in, np.float64)
    for i in range(4):   # 1: forward, context kept
        k, b, g, be = Wd[4 * i:4 * i + 4]
        z = O.conv2d(x, k, b, 2)
        y, (c, sigma, s) = O.instnorm(z, g[0], be[0])
        m = np.where(y.reshape(B, -1) > 0, 1.0, np.float64(a))
        xs.append(x)
        caches.append((z.shape, c, sigma, s, m))
        x = O.leaky(y, a)
    wpr = np.asarray(Wd[16], np.float64)[:, 0]
    # 2: top seed = w_pr for every row; 3: first backward to the image, recording g_h and dz of every level
    gh, dzs = {}, {}
    g = np.broadcast_to(wpr[None, :], (B, wpr.size)).reshape(x.shape)
    for i in range(3, -1, -1):
        shp, c, sigma, s, m = caches[i]
        gn = g.reshape(B, -1) * m
        dz, _, _ = O.instnorm_bwd((c, sigma, s), Wd[4 * i + 2][0], gn.reshape(shp))
        gh[i], dzs[i] = g.reshape(B, -1), dz
        g = O.conv_bwd_input(dz, Wd[4 * i], 2, xs[i].shape[1:3])
    # 4: seed
    r2 = (g.reshape(B, -1) ** 2).sum(1)
    term = 0.5 * weight * r2.mean()
    u = (weight / B) * g
    grads = [np.zeros_like(w, dtype=np.float64) for w in Wd]
    # 5: adjoint sweep upward
    uz2 = {}
    for i in range(4):
        shp, c, sigma, s, m = caches[i]
        ud = O.conv_fwd(u, Wd[4 * i], 2)
        grads[4 * i] += O.conv_bwd_filter(u, dzs[i], 2, 5)
        uh, uz, dgam = _norm_dd(gh[i] * m, c, sigma, s, ud.reshape(B, -1), Wd[4 * i + 2][0], m)
        grads[4 * i + 2] += dgam.sum()
        uz2[i] = uz.reshape(shp)
        u = uh.reshape(shp)
    # 6: heads — l is bilinear in (w_pr, h4): a column sum, nothing for the bias, no second-order scalar
    grads[16][:, 0] += u.reshape(B, -1).sum(0)
    # 7: second backward from a ZERO top gradient, driven by the injected adjoints
    g = np.zeros(x.shape)
    for i in range(3, -1, -1):
        shp, c, sigma, s, m = caches[i]
        dz, dg, db = O.instnorm_bwd((c, sigma, s), Wd[4 * i + 2][0], (g.reshape(B, -1) * m).reshape(shp))
        dz = dz + uz2[i]
        grads[4 * i] += O.conv_bwd_filter(xs[i], dz, 2, 5)
        grads[4 * i + 1] += dz.sum(axis=(0, 1, 2))
        grads[4 * i + 2] += dg
        grads[4 * i + 3] += db
        if i > 0:
            g = O.conv_bwd_input(dz, Wd[4 * i], 2, xs[i].shape[1:3])
    return term, r2, grads


def torch_r1(cfg, Wd, x_in, weight):
    """the same by autograd double backward (create_graph=True) on the logit of the float64 torch oracle"""
    from oracle.torch_oracle import Net
    net = Net(cfg, {"D": Wd})
    x = torch.tensor(np.asarray(x_in, np.float64), requires_grad=True)
    wpr, bpr = net.W["D"][16:18]
    logit = net.encoder(x)[-1].reshape(x.shape[0], -1) @ wpr + bpr
    g, = torch.autograd.grad(logit.sum(), x, create_graph=True)
    r2 = (g.flatten(1) ** 2).sum(1)
    term = 0.5 * weight * r2.mean()
    dD = torch.autograd.grad(term, net.W["D"], allow_unused=True)
    return (float(term.detach()), r2.detach().numpy(),
            [np.zeros(w.shape) if d is None else d.detach().numpy() for d, w in zip(dD, Wd)])


ZERO_GRADS = (15, 17, 18, 19)   # norm4.beta, dense_pr.bias, dense_cond.*: exactly nothing, by construction


@pytest.fixture(scope="module")
def tiny_pair():
    cfg, Wd, x = _tiny_case(3)
    assert dict(init_dim=cfg.init_dim, conv_filter=tuple(cfg.conv_filter), batch_size=cfg.batch_size) == {k: TINY[k] for k in
                                                                                                             ("init_dim", "conv_filter", "batch_size")}
    return np_r1(cfg, Wd, x, 160.0), torch_r1(cfg, Wd, x, 160.0)


@pytest.mark.parametrize("group", [(0, 20), (0, 12), (12, 16), (16, 20)], ids=["full", "levels1-3", "level4", "heads"])
def test_restatement_matches_torch_double_backward(tiny_pair, group):
    (term, r2, grads), (t_term, t_r2, t_grads) = tiny_pair
    assert t_term > 0 and np.all(t_r2 > 0)
    assert abs(term - t_term) <= 1e-12 * max(1.0, abs(t_term))
    assert np.abs(r2 - t_r2).max() <= 1e-12 * np.abs(t_r2).max()
    lo, hi = group
    for i in range(lo, hi):
        exp = t_grads[i]
        scale = max(np.abs(exp).max(), 1e-30)
        assert np.abs(grads[i] - exp).max() <= 1e-10 * scale + 1e-18, (i, np.abs(grads[i] - exp).max(), scale)
        if i in ZERO_GRADS:
            assert not np.any(t_grads[i]) and not np.any(grads[i]), i
        else:
            assert np.any(t_grads[i]), i


# ---------------------------------------------------------------------------------------------------------------------
# the entry points of include/littlegan_hip_reg.h
@pytest.fixture(scope="module")
def lib():
    from littlegan_amd.csrc.build import build
    build(verbose=False)
    from littlegan_amd import _lib
    return _lib


def test_reg_header_declares_the_entry_points(lib):
    assert set(_protos(REG_HEADER)) == set(ENTRY_POINTS) == {n for n in lib.SIGNATURES if n.startswith("lgr_")}


def test_argument_validation_without_gpu(lib):
    h = lib.load()
    d, d2, d3, dw = C.c_void_p(64), C.c_void_p(128), C.c_void_p(256), C.c_void_p(512)   # never dereferenced: every call fails on the host
    err = lambda: h.lg_last_error()
    ws = h.lgr_r1_workspace_bytes(4, 8192)
    seed = h.lgr_r1_seed                     # (g, u0, r2, loss, r1_loss, weight, workspace, ws_bytes, B, L, stream)
    for args in ((None, d2, d3, None, None, 4.0, dw, ws, 4, 8192, None), (d, None, d3, None, None, 4.0, dw, ws, 4, 8192, None),
                 (d, d2, None, None, None, 4.0, dw, ws, 4, 8192, None), (d, d2, d3, None, None, 4.0, None, ws, 4, 8192, None)):
        assert seed(*args) == -1 and b"null pointer" in err() and b"lgr_r1_seed" in err()
    assert seed(C.c_void_p(68), d2, d3, None, None, 4.0, dw, ws, 4, 8192, None) == -1 and b"aligned" in err()
    assert seed(d, C.c_void_p(136), d3, None, None, 4.0, dw, ws, 4, 8192, None) == -1 and b"aligned" in err()
    for B, L in ((4, 8190), (4, 8191), (0, 8192), (-1, 8192), (4, 0), (4, -4), (65536, 131072), (1, 1 << 33), (3, 1 << 40)):
        assert seed(d, d2, d3, None, None, 4.0, dw, 1 << 40, B, L, None) == -1 and b"bad shape" in err() and b"lgr_r1_seed" in err(), (B, L)
    assert (65536 * 131072) // 4 == 1 << 31
    assert seed(d, d2, d3, None, None, 4.0, dw, ws - 1, 4, 8192, None) == -1 and b"workspace too small" in err() and b"lgr_r1_seed" in err()
    for w in (float("nan"), -1.0, float("inf"), float("-inf"), -1e-30):
        assert seed(d, d2, d3, None, None, w, dw, ws, 4, 8192, None) == -1 and b"weight" in err() and b"lgr_r1_seed" in err(), w
    hs = h.lgr_r1_heads_seed                 # (wpr, g, B, K, stream)
    assert hs(None, d2, 3, 16, None) == -1 and b"null pointer" in err() and b"lgr_r1_heads_seed" in err()
    assert hs(d, None, 3, 16, None) == -1 and b"null pointer" in err()
    assert hs(C.c_void_p(66), d2, 3, 16, None) == -1 and b"aligned" in err()
    for B, K in ((0, 16), (-2, 16), (3, 0), (3, -1), (1 << 16, 1 << 15)):
        assert hs(d, d2, B, K, None) == -1 and b"bad shape" in err() and b"lgr_r1_heads_seed" in err(), (B, K)
    cs = h.lgr_r1_heads_colsum               # (u, dwpr, workspace, ws_bytes, B, K, stream)
    wc = h.lgr_r1_colsum_workspace_bytes(40, 100)
    assert cs(None, d2, dw, wc, 40, 100, None) == -1 and b"null pointer" in err() and b"lgr_r1_heads_colsum" in err()
    assert cs(d, None, dw, wc, 40, 100, None) == -1 and b"null pointer" in err()
    assert cs(d, d2, None, wc, 40, 100, None) == -1 and b"null pointer" in err()
    assert cs(d, d2, C.c_void_p(516), wc, 40, 100, None) == -1 and b"aligned" in err()
    for B, K in ((0, 100), (-1, 100), (40, 0), (40, -3), (1 << 16, 1 << 15)):
        assert cs(d, d2, dw, 1 << 40, B, K, None) == -1 and b"bad shape" in err() and b"lgr_r1_heads_colsum" in err(), (B, K)
    assert cs(d, d2, dw, wc - 1, 40, 100, None) == -1 and b"workspace too small" in err() and b"lgr_r1_heads_colsum" in err()


def test_sizing_functions(lib):
    h = lib.load()
    for fn, shapes, empty in ((h.lgr_r1_workspace_bytes, [(1, 4), (4, 4100), (8, 49152), (512, 64), (256, 49152)], [(0, 64), (-1, 64), (4, 0), (4, -4)]),
                              (h.lgr_r1_colsum_workspace_bytes, [(1, 4), (5, 100), (257, 260), (256, 24576)], [(0, 4), (-1, 4), (4, 0), (4, -1)])):
        for s in shapes:
            assert fn(*s) > 0 and fn(*s) == fn(*s), s
        for s in empty:
            assert fn(*s) == 0, s
    # one double per 4096-element chunk of a row / per column and 32-row slab: the layout is the shape's alone
    assert h.lgr_r1_workspace_bytes(4, 4100) >= 4 * 2 * 8 and h.lgr_r1_workspace_bytes(256, 49152) == 256 * 12 * 8
    assert h.lgr_r1_colsum_workspace_bytes(257, 260) >= 9 * 260 * 8 and h.lgr_r1_colsum_workspace_bytes(256, 24576) == 8 * 24576 * 8


# ---------------------------------------------------------------------------------------------------------------------
# configuration and trainer
def test_config_keys_default_to_off(tmp_path):
    from littlegan_amd import config
    d = config.DEFAULTS
    assert d["r1_gamma"] == 0.0 and d["r1_interval"] == 16
    assert "r1_gamma" in config.__doc__ and "r1_interval" in config.__doc__
    a = config.Arg(["train", "x"], config_dir=str(tmp_path))
    assert a.r1_gamma == 0.0 and a.r1_interval == 16
    (tmp_path / "r1.config.json").write_text('{"r1_gamma": 10, "r1_interval": 4}')
    a = config.Arg(["train", "x", "-e", "r1"], config_dir=str(tmp_path))
    assert (a.r1_gamma, a.r1_interval) == (10, 4)
    assert config.r1_settings() is None and config.r1_settings(0.0, 16) is None and config.r1_settings(0, 1) is None
    assert config.r1_settings(10.0, 16) == {"gamma": 10.0, "interval": 16, "weight": 160.0}
    assert config.r1_settings(0.5, 1) == {"gamma": 0.5, "interval": 1, "weight": 0.5}


BAD = [("r1_gamma", -1.0), ("r1_gamma", float("nan")), ("r1_gamma", float("inf")), ("r1_gamma", True), ("r1_gamma", "10"),
       ("r1_interval", 0), ("r1_interval", -16), ("r1_interval", 2.5), ("r1_interval", True), ("r1_interval", "16")]


@pytest.mark.parametrize("key,value", BAD, ids=lambda v: str(v))
def test_an_out_of_range_value_raises(tmp_path, key, value):
    """... at start-up, and whether or not the penalty is on: a bad r1_interval is refused with r1_gamma 0 too"""
    from littlegan_amd import config
    with pytest.raises(ValueError, match=key):
        config.r1_settings(**{key: value})
    with pytest.raises(ValueError, match=key):
        config.r1_settings(**dict(dict(r1_gamma=10.0, r1_interval=16), **{key: value}))
    (tmp_path / "bad.config.json").write_text(json.dumps({key: value}))
    with pytest.raises(ValueError, match=key):
        config.Arg(["train", "x", "-e", "bad"], config_dir=str(tmp_path))
    with pytest.raises(ValueError, match=key):
        _cpu_trainer(**{key: value})


def test_trainer_refusals_and_the_penalty_steps():
    with pytest.raises(ValueError, match="r1_gamma and use_gp"):
        _cpu_trainer(r1_gamma=10.0, use_gp=True)
    with pytest.raises(ValueError, match="r1_gamma and dropout_train"):
        _cpu_trainer(r1_gamma=10.0, dropout_train=True, dropout_rate=0.25)
    # off: no state, no loss slot, the step kinds of today with a constant third element
    tr, _ = _cpu_trainer()
    assert tr.r1 is None and "r1" not in tr.losses and not any(tr.r1_step(b) for b in range(40))
    assert {tr.step_kind(b)[2] for b in range(40)} == {False}
    tr0, _ = _cpu_trainer(r1_gamma=0, r1_interval=3)
    assert tr0.r1 is None and "r1" not in tr0.losses
    assert [tr0.step_kind(b) for b in range(40)] == [tr.step_kind(b) for b in range(40)]
    # on: allowed with diff_augment and the weight average (the gated draw needs a device: tests/test_r1_gpu.py); penalty steps are
    # those with batch_no % interval == 0
    tr, _ = _cpu_trainer(r1_gamma=10.0, r1_interval=4, diff_augment="color,cutout", ema_decay=0.99)
    assert tr.r1 == {"gamma": 10.0, "interval": 4, "weight": 40.0} and tuple(tr.losses["r1"].shape) == (1,)
    assert [b for b in range(1, 20) if tr.r1_step(b)] == [4, 8, 12, 16]
    assert all(tr.step_kind(b)[2] == (b % 4 == 0) and tr.step_kind(b)[:2] == tr0.step_kind(b)[:2] for b in range(1, 40))
    assert "r1" not in "".join(tr.checkpoint_state())   # stateless: no checkpoint field


# ---------------------------------------------------------------------------------------------------------------------
# the exact-arithmetic kernel cases of tests/test_r1_gpu.py: data, expected results, and why "bit for bit" is fair
SEED_SHAPES = [(1, 4), (4, 3072), (4, 4100), (2, 8192), (8, 49152), (512, 64)]
COLSUM_SHAPES = [(1, 4), (3, 256), (5, 100), (257, 260), (256, 24576)]
HEADS_SEED_SHAPES = [(1, 1), (3, 256), (5, 100), (256, 24576)]
EXACT_WEIGHT, EXACT_LOSS0 = 4.0, 3.0


def exact_ints(seed, *shape):
    return np.random.default_rng(seed).integers(-4, 5, size=shape)


def exact_seed_case(B, L):
    """g = integers in [-4, 4] times 2^-3 -> (g fp32, expected u0, r2, term, loss after, each fp32 and exact)"""
    n = exact_ints(1000 + 7 * B + L, B, L)
    g = (n * 0.125).astype(F32)
    u0 = F32(EXACT_WEIGHT / B) * g
    r2 = (n.astype(np.int64) ** 2).sum(1) / 64.0
    term = 0.5 * EXACT_WEIGHT * r2.sum() / B
    return g, u0, r2.astype(F32), F32(term), F32(EXACT_LOSS0 + term)


def exact_colsum_case(B, K):
    """u = integers in [-4, 4] times 2^-2, dwpr starts from non-zero integers -> (u, dwpr0, expected dwpr)"""
    n = exact_ints(2000 + 5 * B + K, B, K)
    d0 = np.random.default_rng(3000 + K).integers(1, 9, size=(K, 1))
    return (n * 0.25).astype(F32), d0.astype(F32), (d0[:, 0] + n.sum(0) * 0.25).astype(F32).reshape(K, 1)


def heads_seed_wpr(K):
    """K fp32 words with a NaN of a chosen payload and a -0.0 planted (where K has room)"""
    w = np.random.default_rng(4000 + K).standard_normal(K).astype(F32)
    bits = w.view(np.uint32)
    bits[0] = 0x7FC01234
    if K > 1:
        bits[K // 2] = 0x80000000
    return w


def test_conditions_of_the_exact_cases():
    for B, L in SEED_SHAPES:
        assert L % 4 == 0 and B & (B - 1) == 0
        for v in (EXACT_WEIGHT / B, EXACT_WEIGHT / (2 * B)):    # powers of two: the scale and the mean's factor round nothing
            m, _ = np.frexp(v)
            assert m == 0.5 and float(F32(v)) == v
        n = exact_ints(1000 + 7 * B + L, B, L)
        total = int((n.astype(np.int64) ** 2).sum())
        assert 0 < total < 2 ** 53 and int((n.astype(np.int64) ** 2).sum(1).max()) < 2 ** 24   # integer sums: exact in fp64, r2 exact in fp32
        g, u0, r2, term, loss = exact_seed_case(B, L)
        assert np.array_equal(g.astype(np.float64), n * 0.125)
        assert np.array_equal(u0.astype(np.float64), (EXACT_WEIGHT / B) * (n * 0.125))
        assert np.array_equal(r2.astype(np.float64), (n.astype(np.int64) ** 2).sum(1) / 64.0)
        exact_term = 0.5 * EXACT_WEIGHT * total / 64.0 / B
        assert float(term) == exact_term and float(loss) == EXACT_LOSS0 + exact_term and float(term) > 0
    for B, K in COLSUM_SHAPES:
        u, d0, want = exact_colsum_case(B, K)
        n = exact_ints(2000 + 5 * B + K, B, K)
        assert np.abs(n.sum(0)).max() < 2 ** 20 and np.all(d0 != 0)
        assert np.array_equal(want.astype(np.float64)[:, 0], d0[:, 0].astype(np.float64) + u.astype(np.float64).sum(0))
    for B, K in HEADS_SEED_SHAPES:
        w = heads_seed_wpr(K)
        assert np.isnan(w[0]) and (K == 1 or (w[K // 2] == 0 and np.signbit(w[K // 2])))
