"""The losses, the optimizer and the element-wise / column-sum kernels at the sizes where their launch shapes change
(loss_optim.hip; colsum_kernel of wgrad_igemm.hip): one element, one block, the first size past a block, and the size that crosses
each launcher's block cap so that the grid-stride loop makes a ragged second trip.

Where the arithmetic can be restated exactly the comparison is bit for bit:
  l1_tanh_loss  t, img multiples of 2^-6 in [-1, 1]: d = t - img and every partial sum of |d| (a block sums about 1028 of them,
                < 2^18 in units of 2^-6; the block partials are merged in fp64) are exact in any order, so
                loss = float32(float64(sum |d|) * float64(gscale)), gscale = float32(lam) / float32(n), and dpre is the kernel's
                documented fp32 expression evaluated by numpy in float32 (the library is built with -ffp-contract=off).
  axpby         numpy float32 a * x + b * y.
  bias_grad     integer data: column sums below 2^24 are exact.
Elsewhere the tolerances are those the ops already have in tests/test_ops_gpu.py; the observed maxima are printed."""
import zlib

import numpy as np
import pytest
import torch

from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def ops():
    from littlegan_amd import ops as _ops
    return _ops


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda")


def f64(t):
    return t.detach().cpu().double().numpy()


def rel(got, exp):
    got = f64(got) if torch.is_tensor(got) else np.asarray(got)
    return float(np.abs(got - exp).max() / (np.abs(exp).max() + 1e-30))


def seed(case):
    return zlib.crc32(repr(case).encode())


# ---------------------------------------------------------------------------------------------------------------- l1_tanh_loss
L1_BIG = 4 * (262144 + 773)   # 1024 blocks x 256 threads x 4 floats, plus a ragged second grid-stride trip


@pytest.mark.parametrize("with_gin", [True, False])
@pytest.mark.parametrize("n", [4, 1024, 1028, L1_BIG])
def test_l1_tanh_loss_bit_exact(ops, n, with_gin):
    rng = np.random.default_rng(seed((n, with_gin)))
    t = (rng.integers(-64, 65, n) / 64.0).astype(F32)
    img = (rng.integers(-64, 65, n) / 64.0).astype(F32)
    gin = (rng.integers(-128, 129, n) / 1024.0).astype(F32) if with_gin else None
    lam = 0.02
    gscale = F32(lam) / F32(n)
    d = t - img
    sg = np.sign(d).astype(F32)
    dpre_e = ((gin if with_gin else F32(0.0)) - gscale * sg) * (F32(1.0) - img * img)   # float32 operations throughout
    assert dpre_e.dtype == F32 and gscale.dtype == F32
    term = F32(np.float64(np.abs(d.astype(np.float64)).sum()) * np.float64(gscale))
    td, imgd, gd = dev(t), dev(img), (dev(gin) if with_gin else None)
    dpre = torch.full((n,), 9.0, device="cuda")
    loss = torch.full((1,), 5.0, device="cuda")
    ops.l1_tanh_loss(td, imgd, gd, dpre, loss, lam, False)
    assert np.array_equal(dpre.cpu().numpy(), dpre_e), int((dpre.cpu().numpy() != dpre_e).sum())
    assert loss.cpu().numpy()[0] == term, (loss.item(), float(term))
    prior = F32(0.375)
    loss.fill_(float(prior))
    ops.l1_tanh_loss(td, imgd, gd, dpre, loss, lam, True)                                   # accumulate: fp32 add onto what is there
    assert loss.cpu().numpy()[0] == prior + term, (loss.item(), float(prior + term))
    assert np.array_equal(dpre.cpu().numpy(), dpre_e)
    loss.fill_(5.0)
    ops.l1_tanh_loss(td, imgd, gd, None, loss, lam, False)                                  # loss only
    assert loss.cpu().numpy()[0] == term, (loss.item(), float(term))


def test_l1_tanh_loss_random_large(ops):
    """random operands past the block cap against the fp64 oracle, tolerances of test_ops_gpu.py::test_l1_tanh_loss"""
    n = L1_BIG
    rng = np.random.default_rng(seed(("l1", n)))
    t = rng.uniform(-1, 1, n).astype(F32).astype(np.float64)
    img = np.tanh(rng.standard_normal(n)).astype(F32).astype(np.float64)
    gin = (rng.standard_normal(n) * 1e-3).astype(F32).astype(np.float64)
    loss, dpre = torch.zeros(1, device="cuda"), torch.empty(n, device="cuda")
    ops.l1_tanh_loss(dev(t), dev(img), dev(gin), dpre, loss, 0.02, False)
    e_loss = abs(loss.item() - 0.02 * O.l1_mean(t, img))
    e_dpre = rel(dpre, (gin + 0.02 * O.l1_mean_bwd_b(t, img)) * (1 - img * img))
    print(f"l1_tanh_loss n={n} rand: |loss err| {e_loss:.2e} dpre {e_dpre:.2e}")
    assert e_loss < 1e-6 and e_dpre < 1e-5


# ---------------------------------------------------------------------------------------------------------------- bce_heads_loss
@pytest.mark.parametrize("B,c", [(1, 1), (512, 40), (1024, 40)])   # one thread busy; 21 and 41 trips of the single 1024-thread block
def test_bce_heads_loss_sizes(ops, B, c):
    rng = np.random.default_rng(seed((B, c)))
    p = rng.uniform(0.02, 0.98, (B, 1 + c)).astype(F32).astype(np.float64)
    p[B - 1, c] = 1.0                      # saturated: clipped, zero gradient
    if B > 1:
        p[0, 0], p[1, 2], p[B - 1, 0], p[B // 2, c] = 0.0, 1.0, 1.0, 0.0
    t_c = O.soft(2.0 * rng.integers(0, 2, (B, c)) - 1.0).astype(F32).astype(np.float64)
    loss = torch.full((1,), 3.0, device="cuda")
    dz = torch.full((B, 1 + c), 9.0, device="cuda")
    ops.bce_heads_loss(dev(p), dev(t_c), O.soft(1.0), 1.0, 2.0, loss, dz, False)
    exp = O.bce_mean(O.soft(1.0), p[:, :1]) + 2.0 * O.bce_mean(t_c, p[:, 1:])
    dp = np.concatenate([O.bce_mean_bwd(O.soft(1.0), p[:, :1]), 2.0 * O.bce_mean_bwd(t_c, p[:, 1:])], 1)
    e1, ez = abs(loss.item() - exp), rel(dz, dp * p * (1 - p))
    assert e1 < 2e-6 * abs(exp) + 1e-6, (loss.item(), exp)
    assert ez < 1e-5
    sat = (p == 0.0) | (p == 1.0)
    assert sat.any() and float(np.abs(f64(dz)[sat]).max()) == 0.0
    ops.bce_heads_loss(dev(p), None, O.soft(0.0), 1.0, 0.0, loss, dz, True)   # no condition targets, weight 0; accumulate
    exp2 = exp + O.bce_mean(O.soft(0.0), p[:, :1])
    e2 = abs(loss.item() - exp2)
    print(f"bce_heads_loss B={B} c={c}: |loss err| {e1:.2e} / {e2:.2e} (loss {exp:.4f} / {exp2:.4f}) dz {ez:.2e}")
    assert e2 < 2e-6 * abs(exp2) + 1e-6, (loss.item(), exp2)
    assert float(dz[:, 1:].abs().max()) == 0.0
    assert rel(dz[:, :1], O.bce_mean_bwd(O.soft(0.0), p[:, :1]) * p[:, :1] * (1 - p[:, :1])) < 1e-5


# ---------------------------------------------------------------------------------------------------------------- clip_adam_update
@pytest.mark.parametrize("clip,gscale", [(0.0, 1.0), (0.5, 0.5)])
@pytest.mark.parametrize("n", [1, 255, 257, 4096 * 256 + 259])   # the last: past the 4096-block cap, ragged second trip
def test_clip_adam_sizes(ops, n, clip, gscale):
    """3 steps against the fp64 oracle: w at the 1e-6 (absolute) of test_ops_gpu.py::test_clip_adam, m and v at 1e-6 relative to their
    largest element (the oracle keeps them: AdamState.m / .v)."""
    rng = np.random.default_rng(seed((n, clip)))
    w0 = rng.standard_normal(n).astype(F32).astype(np.float64)
    lr, b1, b2 = 5e-5, 0.5, 0.9
    st = O.AdamState(lr, b1, b2, 1)
    ws = [w0.copy()]
    w, m, v = dev(w0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    state = dev(np.array([b1, b2]))
    for step in range(3):
        g = rng.standard_normal(n).astype(F32).astype(np.float64)   # gscale * g ~ N(0, 0.25): a third is clipped at 0.5
        gv = gscale * g
        st.apply(ws, [0], [np.clip(gv, -clip, clip) if clip > 0 else gv])
        ops.clip_adam_update(w, dev(g), m, v, state, lr, b1, b2, 1e-8, clip, gscale=gscale)
        ops.adam_advance(state, b1, b2)
    ew, em, ev = float(np.abs(f64(w) - ws[0]).max()), rel(m, st.m[0]), rel(v, st.v[0])
    print(f"clip_adam n={n} clip={clip} gscale={gscale}: |w err| {ew:.2e} m {em:.2e} v {ev:.2e}")
    assert ew < 1e-6 and em < 1e-6 and ev < 1e-6
    assert not np.array_equal(f64(w), w0)
    assert abs(state[0].item() - b1 ** 4) < 1e-7


# ---------------------------------------------------------------------------------------------------------------- axpby
@pytest.mark.parametrize("n", [1, 257, 4096 * 256 + 3])
def test_axpby_bit_exact(ops, n):
    from littlegan_amd import _lib
    rng = np.random.default_rng(seed(("axpby", n)))
    x, y = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    a, b = F32(0.3), F32(-1.7)
    xd, yd = dev(x), dev(y)
    _lib.check(_lib.load().lg_axpby(yd.data_ptr(), xd.data_ptr(), float(a), float(b), n, torch.cuda.current_stream().cuda_stream),
               "lg_axpby")
    exp = a * x + b * y
    assert exp.dtype == F32
    assert np.array_equal(yd.cpu().numpy(), exp), int((yd.cpu().numpy() != exp).sum())
    assert np.array_equal(xd.cpu().numpy(), x)


# ---------------------------------------------------------------------------------------------------------------- bias_grad
# (M, C): one row; C / 4 = 3 does not divide 256; 96 column quads; past the 512-block cap (131149 rows -> 511 blocks of 257);
# C / 4 = 257 (a second column pass for one quad); four full column passes
BIAS_CASES = [(1, 4), (300, 12), (1000, 384), (131072 + 77, 64), (70, 1028), (5, 4096)]


@pytest.mark.parametrize("src", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ["int", "rand"])
@pytest.mark.parametrize("case", BIAS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bias_grad_shapes(ops, case, mode, src):
    M, C = case
    rng = np.random.default_rng(seed(case) + (mode == "rand"))
    if mode == "int":
        dy = rng.integers(-4, 5, (M, C)).astype(F32)       # |column sum| <= 4 * 131149 < 2^24; exact in bf16 too
        prior = rng.integers(-4, 5, C).astype(np.float64)
    else:
        dy = rng.standard_normal((M, C)).astype(F32)
        prior = rng.standard_normal(C).astype(F32).astype(np.float64)
    dyd = dev(dy)
    if src == "bf16":
        dy16 = dyd.to(torch.bfloat16)
        exp = dy16.cpu().double().numpy().sum(0)             # the kernel reads the rounded values
        call = lambda db, acc: ops.bias_grad(None, db, acc, dy16=dy16)
    else:
        exp = dy.astype(np.float64).sum(0)
        call = lambda db, acc: ops.bias_grad(dyd, db, acc)
    db = torch.full((C,), 7.0, device="cuda")
    call(db, False)
    db2 = dev(prior)
    call(db2, True)
    if mode == "int":
        assert np.array_equal(f64(db), exp) and np.array_equal(f64(db2), prior + exp)
    else:
        e1, e2 = rel(db, exp), rel(db2, prior + exp)
        print(f"bias_grad {case} {src} rand: {e1:.2e} accumulate {e2:.2e}")
        assert e1 < 3e-5 and e2 < 3e-5
