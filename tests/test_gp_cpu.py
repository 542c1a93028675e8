"""Gradient penalty (use_gp / gp_weight) without a GPU: the C ABI of gp.hip (declared, exported, bound, validating its
arguments before any launch) and a float64 numpy restatement of the reverse-over-reverse pass structure the kernels implement
(DESIGN.md §12), checked against torch autograd double backward on oracle.torch_oracle.Net.

The penalty is this project's definition (the reference raises, eager_trainer.py:141-143):
  x^_b = eps_b new_image_b + (1 - eps_b) fake_b,  p_b = output_pr(x^_b),  g_b = dp_b/dx^_b,  r_b = |g_b|_2,
  gp = mean_b (r_b - 1)^2,  disc_loss += gp_weight gp;  seed factor (r_b - 1)/max(r_b, 1e-12).
`np_gp` below is also the oracle of tests/test_gp_gpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import np_oracle as O  # noqa: E402
from test_abi import _ctype, _protos  # noqa: E402

GP_ENTRY_POINTS = ("lg_gp_draw_eps", "lg_gp_interp", "lg_gp_workspace_bytes", "lg_gp_seed", "lg_gp_norm_bwd", "lg_gp_norm_dd",
                   "lg_gp_heads_seed", "lg_gp_heads_2nd")


@pytest.fixture(scope="module")
def lib():
    from littlegan_amd.csrc.build import build
    build(verbose=False)
    from littlegan_amd import _lib
    return _lib


def test_header_declares_exports_and_binds_the_gp_entry_points(lib):
    protos = _protos()
    h = lib.load()
    for name in GP_ENTRY_POINTS:
        assert name in protos, f"{name} not declared in include/littlegan_hip.h"
        assert hasattr(h, name), f"{name} not exported"
        res, args = lib.SIGNATURES[name]
        ret, plist = protos[name]
        assert len(args) == len(plist), name
        for a, decl in zip(args, plist):
            assert a is _ctype(decl), (name, decl)
        assert res is {"int": C.c_int, "size_t": C.c_size_t}[ret]
    assert h.lg_abi_version() == 1


def test_gp_argument_validation_without_gpu(lib):
    h = lib.load()
    dummy = C.c_void_p(16)   # never dereferenced: every call below must fail its host-side checks first
    assert h.lg_gp_interp(None, dummy, dummy, dummy, 2, 48, None) == -1
    assert b"null pointer" in h.lg_last_error()
    assert h.lg_gp_interp(dummy, dummy, dummy, dummy, 2, 47, None) == -1          # L % 4 != 0
    assert b"bad shape" in h.lg_last_error()
    assert h.lg_gp_draw_eps(None, 4, 0, 0, None) == -1
    ws = h.lg_gp_workspace_bytes(4, 1024)
    assert ws >= 4 * 5 * 8 and h.lg_gp_workspace_bytes(0, 1024) == 0
    assert h.lg_gp_seed(dummy, dummy, None, None, None, 5.0, dummy, ws, 4, 1024, None) == -1
    assert h.lg_gp_seed(dummy, dummy, dummy, None, None, 5.0, dummy, ws - 1, 4, 1024, None) == -1
    assert b"workspace too small" in h.lg_last_error()
    # exactly one of z (fp32) and z16 (bf16)
    assert h.lg_gp_norm_bwd(dummy, dummy, dummy, dummy, dummy, None, dummy, None, None, None, dummy, ws, 4, 1024, 0.3, None) == -1
    assert h.lg_gp_norm_bwd(None, None, dummy, dummy, dummy, None, dummy, None, None, None, dummy, ws, 4, 1024, 0.3, None) == -1
    assert h.lg_gp_norm_bwd(dummy, None, dummy, dummy, dummy, None, None, None, None, None, dummy, ws, 4, 1024, 0.3, None) == -1
    assert h.lg_gp_norm_dd(dummy, None, dummy, dummy, dummy, None, dummy, None, None, dummy, ws, 4, 1024, 0.3, None) == -1
    assert h.lg_gp_norm_dd(dummy, None, dummy, dummy, dummy, dummy, dummy, None, None, dummy, ws, 0, 1024, 0.3, None) == -1
    assert h.lg_gp_heads_seed(dummy, None, dummy, 4, 64, 5, None) == -1
    assert h.lg_gp_heads_2nd(dummy, dummy, None, dummy, dummy, dummy, dummy, None, 4, 64, 5, None) == -1   # dwpr needs x
    assert b"needs the heads input" in h.lg_last_error()
    assert h.lg_gp_heads_2nd(dummy, dummy, None, dummy, dummy, dummy, None, None, 0, 64, 5, None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatement of the kernels' pass structure (steps 3-7 of DESIGN.md §12)
def _norm_dd(gn, c, sigma, s, u, gamma, m):
    """per-sample rows: -> (u_h, u_z2, dgamma contributions [B])"""
    N = c.shape[1]
    A = gn.mean(1, keepdims=True)
    M = (gn * c).mean(1, keepdims=True)
    U = u.sum(1, keepdims=True)
    P = (u * c).sum(1, keepdims=True)
    T1 = (u * gn).sum(1, keepdims=True) - A * U
    uh = m * (gamma / s) * (u - U / N - c * (P / N) / (s * sigma))
    uz2 = (-gamma * T1 * c / (N * s ** 2 * sigma) - gamma / (s ** 2 * sigma) * (P * (gn - A) / N + M * (u - U / N))
           + gamma * M * P * (2 / s + 1 / sigma) * c / (N * s ** 2 * sigma ** 2))
    dgam = ((T1 - M * P / (s * sigma)) / s)[:, 0]
    return uh, uz2, dgam


def np_gp(cfg, Wd, xhat, gp_weight):
    """-> (gp_weight * gp, r [B], 20 gradients of gp_weight * gp w.r.t. Discriminator.weights), all float64"""
    a = cfg.leaky_alpha
    B = xhat.shape[0]
    xs, caches = [], []
    x = np.asarray(xhat, np.float64)
    for i in range(4):
        k, b, g, be = Wd[4 * i:4 * i + 4]
        z = O.conv2d(x, k, b, 2)
        y, (c, sigma, s) = O.instnorm(z, g[0], be[0])
        m = np.where(y.reshape(B, -1) > 0, 1.0, np.float64(a))   # the leaky mask in float64
        xs.append(x)
        caches.append((z.shape, c, sigma, s, m))
        x = O.leaky(y, a)
    hx = x.reshape(B, -1)
    wpr = Wd[16][:, 0]
    p = O.sigmoid(hx @ wpr + Wd[17][0])
    sp, spp = p * (1 - p), p * (1 - p) * (1 - 2 * p)
    # 3: first backward to the image, recording g_h and dz of every level
    gh, dzs = {}, {}
    g = (sp[:, None] * wpr[None, :]).reshape(x.shape)
    for i in range(3, -1, -1):
        shp, c, sigma, s, m = caches[i]
        gn = g.reshape(B, -1) * m
        dz, _, _ = O.instnorm_bwd((c, sigma, s), Wd[4 * i + 2][0], gn.reshape(shp))
        gh[i], dzs[i] = g.reshape(B, -1), dz
        g = O.conv_bwd_input(dz, Wd[4 * i], 2, xs[i].shape[1:3])
    # 4: seed
    r = np.sqrt((g.reshape(B, -1) ** 2).sum(1))
    term = gp_weight * ((r - 1) ** 2).mean()
    u = (2 * gp_weight / B) * ((r - 1) / np.maximum(r, 1e-12))[:, None, None, None] * g
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
    # 6: heads, second order
    u4 = u.reshape(B, -1)
    t = spp * (u4 @ wpr)
    grads[16][:, 0] += (sp[:, None] * u4).sum(0) + hx.T @ t
    grads[17] += t.sum()
    # 7: second backward with the injected adjoints
    g = (t[:, None] * wpr[None, :]).reshape(x.shape)
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
    return term, r, grads


def torch_gp(cfg, Wd, xhat, gp_weight):
    """the same by autograd double backward (create_graph=True) on the float64 torch oracle"""
    from oracle.torch_oracle import Net
    net = Net(cfg, {"D": Wd})
    x = torch.tensor(np.asarray(xhat, np.float64), requires_grad=True)
    pr, _ = net.discriminator(x)
    g, = torch.autograd.grad(pr.sum(), x, create_graph=True)
    r = g.flatten(1).norm(dim=1)
    term = gp_weight * ((r - 1) ** 2).mean()
    dD = torch.autograd.grad(term, net.W["D"], allow_unused=True)
    return (float(term.detach()), r.detach().numpy(),
            [np.zeros(w.shape) if d is None else d.detach().numpy() for d, w in zip(dD, Wd)])


TINY = dict(init_dim=2, conv_filter=(16, 8, 8, 8, 8), cond_dim=3, noise_dim=5, batch_size=3)


def _tiny_case(seed):
    cfg = O.Cfg(**TINY)
    W = O.init_weights(cfg, seed)
    rng = np.random.default_rng(seed + 7)
    Wd = [w + 0.1 * rng.standard_normal(w.shape) if w.ndim == 1 else w for w in W["D"]]
    real = rng.uniform(-1, 1, (cfg.batch_size, cfg.image_dim, cfg.image_dim, 3))
    fake = rng.uniform(-1, 1, real.shape)
    eps = rng.uniform(0, 1, cfg.batch_size)
    xhat = eps[:, None, None, None] * real + (1 - eps[:, None, None, None]) * fake
    return cfg, Wd, xhat


@pytest.mark.parametrize("group", [(0, 20), (0, 12), (12, 16), (16, 20)], ids=["full", "levels1-3", "level4", "heads"])
def test_restatement_matches_torch_double_backward(group):
    cfg, Wd, xhat = _tiny_case(3)
    term, r, grads = np_gp(cfg, Wd, xhat, 5.0)
    t_term, t_r, t_grads = torch_gp(cfg, Wd, xhat, 5.0)
    assert abs(term - t_term) <= 1e-12 * max(1.0, abs(t_term))
    assert np.abs(r - t_r).max() <= 1e-12 * np.abs(t_r).max()
    lo, hi = group
    for i in range(lo, hi):
        exp = t_grads[i]
        scale = max(np.abs(exp).max(), 1e-30)
        assert np.abs(grads[i] - exp).max() <= 1e-10 * scale + 1e-18, (i, np.abs(grads[i] - exp).max(), scale)
    if hi == 20:   # dense_cond gets nothing from the penalty
        assert not np.any(t_grads[18]) and not np.any(t_grads[19]) and not np.any(grads[18]) and not np.any(grads[19])


def test_instnorm_double_backward_formulas():
    """Step 5 on its own: u_h, u_z2 and dgamma of one InstanceNorm + LeakyReLU level against autograd of <u, dz(z, g, gamma)>."""
    rng = np.random.default_rng(11)
    B, N, alpha = 3, 40, 0.3
    z = rng.standard_normal((B, N))
    g = rng.standard_normal((B, N))
    u = rng.standard_normal((B, N))
    gamma, beta = 1.3, 0.2
    zt = torch.tensor(z, requires_grad=True)
    gt = torch.tensor(g, requires_grad=True)
    gmt = torch.tensor(gamma, dtype=torch.float64, requires_grad=True)
    mu = zt.mean(1, keepdim=True)
    c = zt - mu
    sigma = (c * c).mean(1, keepdim=True).sqrt()
    n = gmt * c / (sigma + 1e-3) + beta
    y = torch.nn.functional.leaky_relu(n, alpha)
    dz, = torch.autograd.grad((y * gt).sum(), zt, create_graph=True)
    v_z, v_g, v_gm = torch.autograd.grad((dz * torch.tensor(u)).sum(), (zt, gt, gmt))
    cn = z - z.mean(1, keepdims=True)
    sg = np.sqrt((cn * cn).mean(1, keepdims=True))
    m = np.where(gamma * cn / (sg + 1e-3) + beta > 0, 1.0, np.float64(alpha))
    uh, uz2, dgam = _norm_dd(g * m, cn, sg, sg + 1e-3, u, gamma, m)
    assert np.abs(uh - v_g.numpy()).max() <= 1e-13
    assert np.abs(uz2 - v_z.numpy()).max() <= 1e-13
    assert abs(dgam.sum() - float(v_gm)) <= 1e-13
