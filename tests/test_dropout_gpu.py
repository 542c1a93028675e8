"""Live encoder dropout (dropout_train) on the GPU.

Kernels: lg_dropout_mask against the numpy restatement of tests/test_dropout_cpu.py bit for bit; every dropped norm pass against
its plain twin (forward: plain fp32 output times keep * scale, bit for bit, the bf16 mirror its round-to-nearest-even; backward: the
plain backward fed the pre-multiplied fp32 gradient, at the tolerances tests/test_ops_gpu.py uses for that pass), at a small shape
and at the encoder-level shapes the C3 step launches (B = 256, and 512 for D's [new_image ; fake] pass).  At those shapes the
mask comes from lg_dropout_mask, which the first test pins to the restatement (including a row range deep inside such a batch).
Whole steps: rate 0 under dropout_train is bit-identical to the feature off; rate 0.5 against a float64 torch oracle whose encoder
multiplies each level by the restated masks (call slots 0 / 1 / 2, the Adjuster's `tails` rows under call 0's masks) at the TOLS of
tests/test_step_gpu.py; the bf16 path also, as in that file, against the bf16-EMULATING numpy oracle at TOLS["bf16_emu"], its encoder
forward and backward wrapped with the same masks (`masked_np_oracle`), at the small geometry and at the C3 geometry, where the fused
routes the masked encoder leaves are otherwise in use; eager against graph replay, replays with fresh keys, checkpoint resume, two
gloo ranks."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # the spawned ranks import this module by name too
from oracle import np_oracle as O  # noqa: E402
from oracle import torch_oracle as TO  # noqa: E402
from test_dropout_cpu import drop_mult, keep_mask, key_of, threshold  # noqa: E402
from test_step_gpu import TOLS, check_emu, check_grads, dev_inputs, f32_round, load_weights, make_args, perturbed  # noqa: E402

pytestmark = pytest.mark.gpu

ALPHA = 0.3
SMALL = dict(init_dim=2, conv_filter=(64, 32, 32, 32, 32), cond_dim=5, noise_dim=11, batch_size=3)
# encoder levels of the C3 step (128 x 128 images, conv_filter 384..32): D's pass on [new_image ; fake] has 2B = 512 rows
# (calls 0 and 2), the Adjuster's own pass B = 256 (call 1): every level at both
C3_LEVELS = [(B, H, H, C) for B in (256, 512) for H, C in ((64, 64), (32, 128), (16, 256), (8, 384))]


@pytest.fixture(scope="module")
def ops():
    from littlegan_amd import ops as _ops
    return _ops


def dev_key(seed_arg=0, rank=0, step=1):
    return torch.tensor(key_of(seed_arg, rank, step), dtype=torch.int64, device="cuda")


def _mult(ops, key, call, level, r0, B, L, rate, device_mask):
    """keep * scale [B, L] fp32 on the device: from the numpy restatement, or (launch shapes) from lg_dropout_mask"""
    T = threshold(rate)
    scale = np.float32(65536.0) / np.float32(65536 - T)
    if device_mask:
        keep = ops.dropout_mask(key, call, level, r0, B, L, rate)
        return torch.where(keep.bool(), torch.tensor(float(scale), device="cuda"), torch.tensor(0.0, device="cuda"))
    seed, koff = key.tolist()
    return torch.tensor(drop_mult(seed, koff, call, level, r0, B, L, rate), device="cuda")


# ---------------------------------------------------------------------------------------------------------------- 5: the mask
@pytest.mark.parametrize("rate", [0.5, 0.25, 0.3])
def test_mask_kernel_equals_the_restatement(ops, rate):
    key = dev_key(3, 1, 7)
    seed, koff = key.tolist()
    B, L = 3, 4096
    for call, level in ((0, 1), (2, 4), (1, 2)):
        whole = ops.dropout_mask(key, call, level, 0, 2 * B, L, rate).cpu().numpy()
        assert np.array_equal(whole.astype(bool), keep_mask(seed, koff, call, level, 0, 2 * B, L, rate)), (call, level)
        part = ops.dropout_mask(key, call, level, B, B, L, rate).cpu().numpy()          # rows = slice(B, 2B)
        assert np.array_equal(part, whole[B:]), (call, level)
        assert set(np.unique(whole).tolist()) <= {0, 1}
    # a row range deep inside a launch-shape batch (level 1 of the C3 step: L = 64*64*64), and a small odd L / 8
    got = ops.dropout_mask(key, 0, 1, 509, 3, 64 * 64 * 64, rate).cpu().numpy().astype(bool)
    assert np.array_equal(got, keep_mask(seed, koff, 0, 1, 509, 3, 64 * 64 * 64, rate))
    got = ops.dropout_mask(key, 1, 3, 2, 5, 8 * 37, rate).cpu().numpy().astype(bool)
    assert np.array_equal(got, keep_mask(seed, koff, 1, 3, 2, 5, 8 * 37, rate))
    frac = got.mean()
    print(f"rate {rate}: T = {threshold(rate)}, kept {frac:.4f} of {got.size}")


# ---------------------------------------------------------------------------------------------------------------- 6: forward
def _rand(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, device="cuda", generator=g) * scale + shift


def _synthetic_moments(ops, z, gm, bt, nparts):
    """The [B][nparts][3] records {count, mean, M2} a conv epilogue would leave for z, as an ops.Moments (unfinished)"""
    B = z.shape[0]
    zz = z.double().reshape(B, nparts, -1)
    mean = zz.mean(2)
    rec = torch.stack([torch.full_like(mean, zz.shape[2]), mean, ((zz - mean[..., None]) ** 2).sum(2)], dim=-1).contiguous()
    return ops.Moments(rec, nparts, gm, bt, B)


FWD_SHAPES = [pytest.param((3, 8, 8, 32), False, id="small"), pytest.param((5, 4, 2, 40), False, id="small-odd")] + \
             [pytest.param(s, True, id="C3-B%d-%dx%dx%d" % s) for s in C3_LEVELS]


@pytest.mark.parametrize("shape,big", FWD_SHAPES)
@pytest.mark.parametrize("path", ["f32", "bf16", "bf16-finalising"])
def test_dropped_apply_is_plain_apply_times_the_mask(ops, path, shape, big):
    B = shape[0]
    L = int(np.prod(shape[1:]))
    rate, call, level, r0 = 0.5, 2, 3, 0
    key = dev_key(1, 0, 5)
    x = _rand(shape, 11, 1.5, 0.7)
    gm, bt = torch.tensor([1.3], device="cuda"), torch.tensor([-0.2], device="cuda")
    if path != "f32":
        x = x.to(torch.bfloat16)
    st = ops.instnorm_stats(x.float(), gm, bt, 0, ALPHA)
    d = ops.Drop(key, call, level, r0, rate)
    y16, yd16 = (torch.empty(shape, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    if path == "bf16-finalising":
        m0, m1 = _synthetic_moments(ops, x, gm, bt, 4), _synthetic_moments(ops, x, gm, bt, 4)
        y = ops.instnorm_apply(x, m0, None, 0, 1, ALPHA, out16=y16)
        yd = ops.instnorm_apply(x, m1, None, 0, 1, ALPHA, out16=yd16, drop=d)
        assert m0.covered == B and m1.covered == B
        assert torch.equal(m0.stats, m1.stats)                      # the finished records: the plain twin's, bit for bit
        assert float((m0.stats[:, 0] - st[:, 0]).abs().max()) < 1e-5
    else:
        y = ops.instnorm_apply(x, st, None, 0, 1, ALPHA, out16=y16)
        yd = ops.instnorm_apply(x, st, None, 0, 1, ALPHA, out16=yd16, drop=d)
    m = _mult(ops, key, call, level, r0, B, L, rate, big).view(shape)
    want = y * m
    assert torch.equal(yd, want)
    assert torch.equal(yd16, want.to(torch.bfloat16))               # the mirror: RNE of that fp32 value
    assert torch.equal(y16, y.to(torch.bfloat16))
    kept = float((m != 0).float().mean())
    assert abs(kept - 0.5) < 5 * 0.5 / np.sqrt(m.numel())
    # only the mirror (want_f32=False), as the step's levels 1-3 run it
    only16 = torch.empty(shape, dtype=torch.bfloat16, device="cuda")
    if path == "bf16-finalising":
        assert ops.instnorm_apply(x, _synthetic_moments(ops, x, gm, bt, 4), None, 0, 1, ALPHA, out16=only16, want_f32=False, drop=d) is None
    else:
        assert ops.instnorm_apply(x, st, None, 0, 1, ALPHA, out16=only16, want_f32=False, drop=d) is None
    assert torch.equal(only16, yd16)


def test_drop_argument_is_refused_outside_the_encoder_form(ops):
    x = _rand((2, 4, 4, 16), 1)
    gm, bt = torch.ones(1, device="cuda"), torch.zeros(1, device="cuda")
    st = ops.instnorm_stats(x, gm, bt, 0, ALPHA)
    d = ops.Drop(dev_key(), 0, 1, 0, 0.5)
    with pytest.raises(ValueError, match="encoder's form"):
        ops.instnorm_apply(x, st, x, 0, 1, ALPHA, drop=d)
    with pytest.raises(ValueError, match="encoder's form"):
        ops.instnorm_apply(x, st, None, 1, 0, ALPHA, drop=d)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.instnorm_apply(_rand((2, 3, 4), 1), st, None, 0, 1, ALPHA, drop=d)
    with pytest.raises(ValueError, match="encoder's form"):
        ops.instnorm_bwd(x, st, x, None, None, 1, 0, ALPHA, drop=d)
    with pytest.raises(ValueError, match="int64"):
        ops.Drop(torch.zeros(2, device="cuda"), 0)


# ---------------------------------------------------------------------------------------------------------------- 7: backward
def _rel(got, exp):
    got, exp = got.detach().double().cpu().numpy(), exp.detach().double().cpu().numpy()
    return np.abs(got - exp).max() / (np.abs(exp).max() + 1e-30)


BWD_SHAPES = [pytest.param((4, 8, 8, 32), False, id="small"), pytest.param((256, 16, 16, 256), True, id="C3-B256-16x16x256"),
              pytest.param((512, 8, 8, 384), True, id="C3-B512-8x8x384"), pytest.param((256, 32, 32, 128), True, id="C3-B256-32x32x128")]


@pytest.mark.parametrize("shape,big", BWD_SHAPES)
@pytest.mark.parametrize("g16", [False, True], ids=["g-f32", "g-bf16"])
@pytest.mark.parametrize("x16", [False, True], ids=["z-f32", "z-bf16"])
def test_dropped_backward_is_plain_backward_of_the_masked_gradient(ops, x16, g16, shape, big):
    B, C = shape[0], shape[-1]
    L = int(np.prod(shape[1:]))
    rate, call, level = 0.5, 0, 2
    key = dev_key(2, 0, 9)
    x = _rand(shape, 21, 1.5, 0.7)
    g = _rand(shape, 22)
    gm, bt = torch.tensor([1.3], device="cuda"), torch.tensor([-0.2], device="cuda")
    if x16:
        x = x.to(torch.bfloat16)
    if g16:
        g = g.to(torch.bfloat16)
    st = ops.instnorm_stats(x.float(), gm, bt, 0, ALPHA)
    m = _mult(ops, key, call, level, 0, B, L, rate, big).view(shape)
    g_pre = g.float() * m                                            # the pre-multiplied fp32 gradient
    d = ops.Drop(key, call, level, 0, rate)

    def run(grad, drop, with_db, rows=None):
        xs, ss, gs = (x, st, grad) if rows is None else (x[rows], st[rows].contiguous(), grad[rows])
        dg, dbeta = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
        db = torch.zeros(C, device="cuda") if with_db else None
        o16 = torch.empty(xs.shape, dtype=torch.bfloat16, device="cuda")
        dx = ops.instnorm_bwd(xs, ss, gs, dg, dbeta, 0, 1, ALPHA, out16=o16, db=db, drop=drop)
        return dx, o16, dg, dbeta, db

    for with_db in (False, True):
        dx_p, o16_p, dg_p, dbt_p, db_p = run(g_pre, None, with_db)
        dx_d, o16_d, dg_d, dbt_d, db_d = run(g, d, with_db)
        e_dx = _rel(dx_d, dx_p)
        print(f"db={with_db}: dx rel {e_dx:.2e} dgamma {dg_d.item():.6e}/{dg_p.item():.6e} dbeta {dbt_d.item():.6e}/{dbt_p.item():.6e}"
              f" bit-equal dx {torch.equal(dx_d, dx_p)}")
        assert e_dx < 2e-5                                           # tests/test_ops_gpu.py::test_instnorm_stats_apply_bwd
        assert abs(dg_d.item() - dg_p.item()) < 2e-5 * max(1.0, abs(dg_p.item())) * 10
        assert abs(dbt_d.item() - dbt_p.item()) < 2e-5 * max(1.0, abs(dbt_p.item())) * 10
        assert torch.equal(o16_d, dx_d.to(torch.bfloat16))
        if with_db:
            assert _rel(db_d, db_p) < 3e-5                           # the bias-gradient bound of tests/test_ops_gpu.py
    # the masked gradient is what flows: against the norm backward of the oracle on a few samples
    idx = [0, B - 1]
    zz = x[idx].double().cpu().numpy()
    y_e, cache = O.instnorm(zz, 1.3, -0.2)
    dz_e, _, _ = O.instnorm_bwd(cache, 1.3, O.leaky_bwd(y_e, g_pre[idx].double().cpu().numpy(), ALPHA))
    assert np.abs(dx_d[idx].double().cpu().numpy() - dz_e).max() < 2e-4 * np.abs(dz_e).max()
    # a rows slice regenerates the masks of exactly those rows: dx of the second half, bit for bit
    half = B // 2
    rows = slice(half, B)
    dx_r, o16_r, _, _, _ = run(g, d.at(r0=half), False, rows)
    assert torch.equal(dx_r, dx_d[rows]) and torch.equal(o16_r, o16_d[rows])
    dx_w, _, _, _, _ = run(g, d.at(r0=0), False, rows)                # the wrong first row gives other masks
    assert not torch.equal(dx_w, dx_d[rows])


# ---------------------------------------------------------------------------------------------------------------- whole steps
def build_drop(cfg, W, mfma, dropout_train=True, rate=0.5, **kw):
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    args = make_args(cfg, mfma)
    args.dropout_train, args.dropout_rate = dropout_train, rate
    for k, v in kw.items():
        setattr(args, k, v)
    decoder, encoder = Decoder(args), Encoder(args)
    g = Generator(args, decoder)
    d = Discriminator(args, encoder)
    tr = EagerTrainer(args, g, d, Adjuster(args, d, g), None)
    load_weights(tr, W)
    return tr


def _same_state(a, b):
    return all(torch.equal(x, y) for x, y in ((a.store.flat, b.store.flat), (a.store.m, b.store.m), (a.store.v, b.store.v))) and \
        all(torch.equal(a.opt_state[m], b.opt_state[m]) for m in "GDA")


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_rate_zero_is_bit_identical_to_the_feature_off(mfma):
    """dropout_train with dropout_rate = 0: the key is drawn and handed down, the call slots are assigned, every encoder level runs
    its DROPPED kernels (masks that keep everything, scale 1) — and weights, Adam slots, losses and images are those of the feature
    off, bit for bit.  (The fused routes are bypassed only under an active mask: their first-pass sums differ from the stand-alone
    pass in the last bits, tests/test_launch_shapes_gpu.py, so bypassing them at rate 0 could not be bit-identical.)"""
    from littlegan_amd import ops
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 1)
    off, on = build_drop(cfg, W, mfma, dropout_train=False), build_drop(cfg, W, mfma, rate=0.0)
    assert not off.dropout and on.dropout
    made = []
    real_init = ops.Drop.__init__

    def counting(self, *a, **k):
        made.append(1)
        real_init(self, *a, **k)
    ops.Drop.__init__ = counting
    try:
        for n, b in enumerate((4, 5, 10, 11, 15)):
            inp = dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=50 + b)))
            f0, a0, lg0, ld0, la0 = off.train_step_from_inputs(b, inp)
            before = len(made)
            f1, a1, lg1, ld1, la1 = on.train_step_from_inputs(b, dict(inp, dropout_key=dev_key(0, 0, n + 1)))
            assert len(made) > before                                   # the plumbing ran
            torch.cuda.synchronize()
            assert torch.equal(f0, f1) and torch.equal(lg0, lg1) and torch.equal(ld0, ld1), b
            assert (a0 is None) == (a1 is None) and (a0 is None or (torch.equal(a0, a1) and torch.equal(la0, la1))), b
            assert _same_state(off, on), b
    finally:
        ops.Drop.__init__ = real_init


def test_rate_zero_is_bit_identical_at_the_c3_geometry():
    """The same at the reference channel widths and 128 x 128 images (bf16, Adjuster branch on): here the fused routes (the
    normalising conv of D's pass on the Adjuster output, the producer-fused first-pass sums) are in use on both sides."""
    cfg = O.Cfg(init_dim=8, cond_dim=40, batch_size=2)
    W = perturbed(cfg, 7)
    off, on = build_drop(cfg, W, "bf16", dropout_train=False), build_drop(cfg, W, "bf16", rate=0.0)
    inp = dev_inputs(f32_round(O.make_inputs(cfg, 2, seed=9)))
    for n, b in enumerate((11, 15)):
        f0, a0, lg0, ld0, la0 = off.train_step_from_inputs(b, inp)
        f1, a1, lg1, ld1, la1 = on.train_step_from_inputs(b, dict(inp, dropout_key=dev_key(0, 0, n + 1)))
        torch.cuda.synchronize()
        assert torch.equal(f0, f1) and torch.equal(a0, a1) and torch.equal(lg0, lg1) and torch.equal(ld0, ld1) and torch.equal(la0, la1)
        assert _same_state(off, on), b


# ---- 9: the float64 oracle with the restated masks
class DropNet(TO.Net):
    """oracle.torch_oracle.Net whose encoder multiplies each level by the restated masks.  `rows` = [(call, first row, rows)]
    names, for the batch the next encoder call sees, which call slot and absolute rows its samples take their masks from."""

    def __init__(self, cfg, W_np, seed, key_offset, rate):
        super().__init__(cfg, W_np, torch.float64)
        self.seed, self.key_offset, self.rate, self.rows = seed, key_offset, rate, None

    def encoder(self, x):
        We, a = self.W["D"], self.cfg.leaky_alpha
        outs = []
        for i in range(4):
            k, b, g, be = We[4 * i:4 * i + 4]
            x = F.leaky_relu(TO.instnorm(TO.conv2d_same(x, k, b, 2), g, be), a)
            L = int(np.prod(x.shape[1:]))
            assert sum(n for _, _, n in self.rows) == x.shape[0]
            m = np.concatenate([drop_mult(self.seed, self.key_offset, call, i + 1, r0, n, L, self.rate) for call, r0, n in self.rows])
            x = x * torch.tensor(m.astype(np.float64)).view(x.shape)
            outs.append(x)
        return outs


def drop_step_gradients(net, batch_no, inp):
    """oracle.torch_oracle.step_gradients with the call slots of the training step"""
    cfg, W = net.cfg, net.W
    img1, c1, img2, c2 = inp["real_image_1"], inp["real_cond_1"], inp["real_image_2"], inp["real_cond_2"]
    B = img1.shape[0]
    fake = net.generator(inp["noise"], c2)
    net.rows = [(0, 0, B)]                       # call 0 = D on [new_image ; fake]: rows 0..B-1 real, B..2B-1 fake
    real_pr, real_c = net.discriminator(inp["new_image"])
    net.rows = [(0, B, B)]
    fake_pr, fake_c = net.discriminator(fake)
    disc_loss = 2.0 * TO.bce_mean(c1, real_c) + TO.bce_mean(TO.soft(1.0), real_pr) + TO.bce_mean(TO.soft(0.0), fake_pr)
    gen_loss = TO.bce_mean(TO.soft(1.0), fake_pr) + TO.bce_mean(c2, fake_c) + cfg.l1_lambda * (img2 - fake).abs().mean()
    dD = torch.autograd.grad(disc_loss, W["D"], retain_graph=True)
    dG = torch.autograd.grad(gen_loss, W["G"])
    out = dict(fake_image=fake.detach().numpy(), gen_loss=float(gen_loss.detach()), disc_loss=float(disc_loss.detach()),
               dD=[t.numpy() for t in dD], dG=[t.numpy() for t in dG], adj_image=None, adj_loss=None, dA=None)
    if cfg.train_adj and batch_no > 10:
        fk = fake.detach()
        adj_t_cond = torch.cat([c2, c1], 0)
        net.rows = [(1, 0, B), (0, B, B)]        # call 1 = the Adjuster's own pass on img1; fake's maps keep call 0's masks
        adj_img = net.adjuster(torch.cat([img1, fk], 0), (adj_t_cond + 1.0) * 0.5)
        net.rows = [(2, 0, 2 * B)]               # call 2 = D on the Adjuster's output
        adj_pr, adj_c = net.discriminator(adj_img)
        adj_loss = (TO.bce_mean(TO.soft(1.0), adj_pr) + TO.bce_mean(adj_t_cond, adj_c)
                    + cfg.l1_lambda * (torch.cat([img2, img1], 0) - adj_img).abs().mean())
        dA = torch.autograd.grad(adj_loss, W["A"])
        out.update(adj_image=adj_img.detach().numpy(), adj_loss=float(adj_loss.detach()), dA=[t.numpy() for t in dA])
    return out


class masked_np_oracle:
    """While active, oracle.np_oracle's encoder forward / backward apply the restated masks: h = leaky(y) * keep * scale (then the
    bf16 rounding of maps 1-3 under emulate_bf16, where the kernels round), and the arriving gradient times the same multipliers.
    The encoder calls of O.step_gradients come in the order D(new_image), D(fake), [Adjuster([img1 ; fake]), D(adj_image)]: each takes
    the next row specification [(call, first row, rows)] of the training step's call slots."""

    def __init__(self, seed, key_offset, rate, B):
        self.seed, self.key_offset, self.rate = seed, key_offset, rate
        self.specs = [[(0, 0, B)], [(0, B, B)], [(1, 0, B), (0, B, B)], [(2, 0, 2 * B)]]

    def _fwd(self, cfg, We, x):
        rows = self.todo.pop(0)
        assert sum(n for _, _, n in rows) == x.shape[0]
        outs, caches = [], []
        emu = getattr(cfg, "emulate_bf16", False)
        for i in range(4):
            k, b, g, be = We[4 * i:4 * i + 4]
            x = O._q(cfg, x)
            z = O.conv2d(x, O._q(cfg, k), b, 2)
            y, nc = O.instnorm(z, g[0], be[0], xq=O._q(cfg, z) if emu else None)
            L = int(np.prod(y.shape[1:]))
            m = np.concatenate([drop_mult(self.seed, self.key_offset, c, i + 1, r0, n, L, self.rate) for c, r0, n in rows])
            m = m.astype(np.float64).reshape(y.shape)
            h = O.leaky(y, cfg.leaky_alpha) * m
            if emu and i < 3:
                h = O.bf16_round(h)
            caches.append((x, y, nc, m))
            outs.append(h)
            x = h
        return outs, caches

    @staticmethod
    def _bwd(cfg, We, caches, d_outs, need_wgrad=True, need_input_grad=False):
        grads = [None] * 16
        g_h = None
        for i in reversed(range(4)):
            k, b, g, be = We[4 * i:4 * i + 4]
            x, y, nc, m = caches[i]
            if d_outs[i] is not None:
                g_h = d_outs[i] if g_h is None else g_h + d_outs[i]
            dy = O.leaky_bwd(y, g_h * m, cfg.leaky_alpha)
            dz, dg, dbe = O.instnorm_bwd(nc, g[0], dy)
            dzq = O._q(cfg, dz)
            dx = O.conv_bwd_input(dzq, O._q(cfg, k), 2, x.shape[1:3]) if (i > 0 or need_input_grad) else None
            if dx is not None and i > 0:
                dx = O._q(cfg, dx)
            if need_wgrad:
                grads[4 * i] = O.conv_bwd_filter(x, dzq, 2, k.shape[0])
                grads[4 * i + 1] = dz.sum(axis=(0, 1, 2))
                grads[4 * i + 2] = np.array([dg])
                grads[4 * i + 3] = np.array([dbe])
            g_h = dx
        return grads, g_h

    def __enter__(self):
        self.saved = (O.encoder_fwd, O.encoder_bwd)
        self.todo = list(self.specs)
        O.encoder_fwd, O.encoder_bwd = self._fwd, self._bwd
        return self

    def __exit__(self, *exc):
        O.encoder_fwd, O.encoder_bwd = self.saved


@pytest.mark.parametrize("b", [4, 5, 11], ids=["full", "partition", "adjuster"])
@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_step_matches_the_masked_oracle(mfma, b):
    """Whole step at rate 0.5 against the float64 oracle with the restated masks.  Without the feature the key is ignored and the
    losses are those of the mask-free oracle: this test fails there."""
    tol = TOLS[mfma]
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 1)
    rate = 0.5
    seed, koff = key_of(0, 0, 3)
    inp = f32_round(O.make_inputs(cfg, cfg.batch_size, seed=50 + b))
    ref = drop_step_gradients(DropNet(cfg, W, seed, koff, rate), b, {k: torch.tensor(v, dtype=torch.float64) for k, v in inp.items()})
    plain = O.step_gradients(cfg, W, b, inp)
    tr = build_drop(cfg, W, mfma, rate=rate)
    fake, adj, lg, ld, la = tr.train_step_from_inputs(b, dict(dev_inputs(inp), dropout_key=dev_key(0, 0, 3)))
    torch.cuda.synchronize()
    print(f"{mfma} b={b}: gen {lg.item():.6f} / masked oracle {ref['gen_loss']:.6f} / mask-free {plain['gen_loss']:.6f};"
          f" disc {ld.item():.6f} / {ref['disc_loss']:.6f} / {plain['disc_loss']:.6f}")
    # the masks matter at this bound: some loss of the mask-free oracle is at least five tolerances away
    keys = ("gen_loss", "disc_loss") + (("adj_loss",) if b > 10 else ())
    assert max(abs(plain[k] - ref[k]) / abs(ref[k]) for k in keys) > 5 * tol["loss"]
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
    check_grads(tr, ref, sets, tol, tag=f"drop {mfma} b={b}", only=only)
    # the two float64 restatements of the masked step agree (torch autograd against the numpy oracle's hand-written backward)
    with masked_np_oracle(seed, koff, rate, cfg.batch_size):
        ref_np = O.step_gradients(cfg, W, b, inp)
    assert abs(ref_np["disc_loss"] - ref["disc_loss"]) < 1e-10 and abs(ref_np["gen_loss"] - ref["gen_loss"]) < 1e-10
    for key in [k for _, k in sets]:
        for i, (u, v) in enumerate(zip(ref_np[key], ref[key])):
            assert np.abs(np.asarray(u).ravel() - np.asarray(v).ravel()).max() <= 1e-9 * (1 + np.abs(v).max()), (key, i)
    if mfma == "bf16":   # the tight whole-step check of the bf16 path: the bf16-emulating oracle under the same masks
        with masked_np_oracle(seed, koff, rate, cfg.batch_size):
            check_emu(tr, cfg, W, b, inp, fake, adj, lg, ld, la, only=only)


def test_masked_step_at_the_c3_geometry_leaves_the_fused_routes():
    """Reference channel widths, 128 x 128 images, bf16, Adjuster branch on, rate 0.5.  At this geometry the feature-off step takes
    the normalising conv (D's pass on the Adjuster output) and the producer-fused first-pass sums (every encoder backward); the
    masked step must take neither, and must match the bf16-emulating oracle under the same masks at TOLS["bf16_emu"]."""
    from littlegan_amd import ops
    cfg = O.Cfg(init_dim=8, cond_dim=40, batch_size=2)
    W = perturbed(cfg, 7)
    inp = f32_round(O.make_inputs(cfg, 2, seed=9))
    seed, koff = key_of(0, 0, 2)
    calls = {"zn": 0, "fuse": 0, "partials": 0}
    real_zn, real_dg, real_bwd = ops.conv2d_s2_fwd_stats_zn, ops.conv2d_s2_dgrad, ops.instnorm_bwd

    def zn(*a, **k):
        calls["zn"] += 1
        return real_zn(*a, **k)

    def dg(*a, **k):
        r = real_dg(*a, **k)
        if k.get("fuse") is not None and r[1] is not None:
            calls["fuse"] += 1
        return r

    def bwd(*a, **k):
        if k.get("partials") is not None and k.get("drop") is not None:
            calls["partials"] += 1
        return real_bwd(*a, **k)
    ops.conv2d_s2_fwd_stats_zn, ops.conv2d_s2_dgrad, ops.instnorm_bwd = zn, dg, bwd
    try:
        off = build_drop(cfg, W, "bf16", dropout_train=False)
        off.train_step_from_inputs(11, dev_inputs(inp))
        torch.cuda.synchronize()
        assert calls["zn"] >= 1 and calls["fuse"] >= 3, calls        # the routes are in use at this geometry
        calls.update(zn=0, fuse=0)
        tr = build_drop(cfg, W, "bf16", rate=0.5)
        fake, adj, lg, ld, la = tr.train_step_from_inputs(11, dict(dev_inputs(inp), dropout_key=dev_key(0, 0, 2)))
        torch.cuda.synchronize()
        assert calls == {"zn": 0, "fuse": 0, "partials": 0}, calls   # ... and the masked encoder leaves them
    finally:
        ops.conv2d_s2_fwd_stats_zn, ops.conv2d_s2_dgrad, ops.instnorm_bwd = real_zn, real_dg, real_bwd
    with masked_np_oracle(seed, koff, 0.5, cfg.batch_size):
        check_emu(tr, cfg, W, 11, inp, fake, adj, lg, ld, la)
    plain = O.step_gradients(cfg, W, 11, inp)
    print(f"C3 geometry: disc {ld.item():.5f} (mask-free oracle {plain['disc_loss']:.5f}), adj {la.item():.5f} ({plain['adj_loss']:.5f})")


# ---- 10: reproducibility
def test_graph_replay_is_bit_exact_with_dropout():
    """graph_step against the eager path at rate 0.5, a fresh key every step: every step kind eager, captured and replayed."""
    cfg = O.Cfg(init_dim=2, conv_filter=(64, 32, 32, 64, 32), cond_dim=5, noise_dim=11, batch_size=3)
    W = perturbed(cfg, 5)
    tr_e, tr_g = build_drop(cfg, W, "bf16"), build_drop(cfg, W, "bf16")
    steps = [8, 9, 10, 11, 12, 13, 15, 16, 20, 21, 25, 26, 30, 31, 35, 40, 45, 50, 55]
    for n, b in enumerate(steps):
        inp = dict(dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=400 + b))), dropout_key=dev_key(0, 0, n + 1))
        fe, ae, lge, lde, lae = tr_e.train_step_from_inputs(b, inp)
        fg, ag, lgg, ldg, lag = tr_g.graph_step(b, inp)
        torch.cuda.synchronize()
        assert torch.equal(fe, fg) and torch.equal(lge, lgg) and torch.equal(lde, ldg), b
        assert (ae is None) == (ag is None) and (ae is None or (torch.equal(ae, ag) and torch.equal(lae, lag))), b
        assert _same_state(tr_e, tr_g), b
    assert len(tr_g._graphs) == 5


def test_replays_of_one_graph_draw_new_masks():
    """lr = 0 freezes the weights, so a step's losses depend on its inputs and masks alone: replays of ONE captured graph with the
    same inputs give the same losses under the same key and other losses under another."""
    cfg = O.Cfg(**{**SMALL, "lr": 0.0})
    tr = build_drop(cfg, perturbed(cfg, 2), "bf16")
    base = dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=77)))
    w0 = tr.store.flat.clone()
    seen = []
    for k in (1, 1, 1, 2, 1, 3):     # eager, capture + replay, replay, ...
        _, _, lg, ld, la = tr.graph_step(11, dict(base, dropout_key=dev_key(0, 0, k)))
        torch.cuda.synchronize()
        seen.append((k, lg.item(), ld.item(), la.item()))
    assert len(tr._graphs) == 1 and torch.equal(tr.store.flat, w0)
    print(seen)
    assert seen[0][1:] == seen[1][1:] == seen[2][1:] == seen[4][1:]          # key 1: eager == replays, bit for bit
    assert seen[3][2] != seen[2][2] and seen[5][2] != seen[3][2] and seen[5][2] != seen[2][2]   # disc loss under keys 2 and 3
    assert seen[3][3] != seen[2][3]                                            # adj loss (call slot 2) too


def test_checkpoint_resume_continues_the_mask_stream(tmp_path):
    """input_step is part of the checkpoint: a restored trainer draws the inputs AND the dropout key of the next step as the
    uninterrupted run does, and lands on the same bits."""
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    cfg = O.Cfg(init_dim=2, conv_filter=(32, 32, 32, 32, 32), cond_dim=3, noise_dim=5, batch_size=2)

    def mk(restore):
        args = make_args(cfg, "f32")
        args.no_io, args.result_dir, args.restore, args.exp_name, args.epoch = False, str(tmp_path), restore, "t", 1
        args.dropout_train = True
        dec, enc = Decoder(args), Encoder(args)
        g = Generator(args, dec)
        d = Discriminator(args, enc)
        return EagerTrainer(args, g, d, Adjuster(args, d, g), None)

    data = [dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=70 + b))) for b in range(4)]

    def step(tr, b, d):
        noise, new_image = tr.draw_step_inputs(d["real_image_1"])
        inp = dict(d, noise=noise, new_image=new_image, dropout_key=tr.draw_dropout_key())
        tr.train_step_from_inputs(b, inp)
        return inp["dropout_key"].tolist()

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


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from littlegan_amd import ops
        cfg = O.Cfg(**{**SMALL, "batch_size": 2})
        tr = build_drop(cfg, perturbed(cfg, 21), "bf16")
        assert tr.sync.enabled and tr.rank == rank
        B = cfg.batch_size
        full = f32_round(O.make_inputs(cfg, B * world, seed=311))
        shard = dev_inputs({k: v[rank * B:(rank + 1) * B] for k, v in full.items()})
        tr._input_step = 1
        key = tr.draw_dropout_key()
        _, _, lg, ld, la = tr.train_step_from_inputs(11, dict(shard, dropout_key=key))
        torch.cuda.synchronize()
        np.save(os.path.join(outdir, f"key_{rank}.npy"), key.cpu().numpy())
        np.save(os.path.join(outdir, f"mask_{rank}.npy"), ops.dropout_mask(key, 0, 1, 0, 2 * B, 16 * 16 * 32, 0.5).cpu().numpy())
        np.save(os.path.join(outdir, f"flat_{rank}.npy"), tr.store.flat.cpu().numpy())
        np.save(os.path.join(outdir, f"loss_{rank}.npy"), np.array([lg.item(), ld.item(), la.item()]))
    finally:
        dist.destroy_process_group()


def test_two_ranks_draw_different_masks_and_finish_a_step(tmp_path):
    world = 2
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
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
                if p.is_alive():
                    p.kill()
    key = [np.load(tmp_path / f"key_{r}.npy") for r in range(world)]
    mask = [np.load(tmp_path / f"mask_{r}.npy") for r in range(world)]
    flat = [np.load(tmp_path / f"flat_{r}.npy") for r in range(world)]
    loss = [np.load(tmp_path / f"loss_{r}.npy") for r in range(world)]
    assert key[0].tolist() == list(key_of(0, 0, 1)) and key[1].tolist() == list(key_of(0, 1, 1))
    assert 0.45 < (mask[0] == mask[1]).mean() < 0.55                     # independent masks
    for r in range(world):
        seed, koff = key[r].tolist()
        assert np.array_equal(mask[r].astype(bool), keep_mask(seed, koff, 0, 1, 0, mask[r].shape[0], mask[r].shape[1], 0.5))
    assert np.array_equal(flat[0], flat[1]) and np.isfinite(flat[0]).all()   # all-reduced gradients: the same weights on both ranks
    assert np.isfinite(loss[0]).all() and np.isfinite(loss[1]).all()
