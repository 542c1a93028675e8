"""The dense / head GEMMs (dense.hip, heads.hip, skinny_mfma.hip) at their routing edges: every case asserts WHICH kernel each entry
point launched (lg_last_kernel; the route table of DESIGN.md 17 is the specification, restated per case below) and runs two ways:

  "int"   every operand (prior dw / db contents of accumulate=True included) is an integer in [-4, 4].  Every product and every
          partial sum, in any order, is then an integer of magnitude <= 16 * 24576 < 2^24: any correct fp32 kernel returns exactly
          the fp64 result, so the comparison is np.array_equal — a dropped, doubled or misplaced term cannot hide in a tolerance.
          heads_fwd: weights and biases scaled by 2^-10 (logits exact and moderate); p against the sigmoid at 1e-5, and rows
          0..B-2 of an MFMA-routed call bit-equal to the same rows computed as a batch of B-1 (VALU route: the logits are exact on
          both routes and both end in heads_final_kernel).
  "rand"  random fp32 operands at the tolerances of tests/test_ops_gpu.py (1e-5 forward and weight gradients, 3e-5 dense_dgrad,
          max-abs error relative to the max-abs of the fp64 result): what notices reduced-precision products, which small integers
          would not.  The observed maximum of every case is printed.

accumulate runs both ways in every case.  One test runs the same checks in a fresh child process under LG_NO_SKINNY_MFMA=1."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import np_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, V = "mfma", "valu"

# (B, K, N, dense_fwd route, dense_wgrad route: V or the MFMA template's MT = ceil(K / 32))
#   dense_fwd   MFMA iff B % 32 == 0 and N % 128 == 0 and K <= 144
#   dense_wgrad MFMA iff B % 32 == 0 and N % 32 == 0 and K <= 160
DENSE_CASES = [
    (32, 133, 128, M, 5),      # the reference batch
    (32, 1, 128, M, 1),        # K = 1
    (64, 144, 256, M, 5),      # K at the forward limit
    (32, 96, 128, M, 3),       # MT = 3 exact
    (32, 97, 128, M, 4),       # MT = 4 ragged
    (32, 128, 128, M, 4),      # MT = 4 exact
    (96, 65, 384, M, 3),       # MT = 3, 1.5 trips of the 16-sample loop (24 samples per wave)
    (32, 160, 128, V, 5),      # weight gradient at its limit, forward VALU
    (32, 145, 128, V, 5),      # mixed: K > 144
    (32, 40, 96, V, 2),        # mixed: N % 128 != 0
    (32, 161, 128, V, V),      # both VALU; exactly one unrolled 8-sample trip per wave
    (31, 133, 128, V, V),      # B just under a tile
    (33, 133, 132, V, V),      # B just over a tile
    (100, 133, 1028, V, V),    # three unrolled trips plus a tail; ragged column block
    (250, 168, 1024, V, V),    # K > 160 at a production-like batch
    (9, 1024, 260, V, V),      # the K limit of dense_fwd
    (1, 1, 4, V, V),           # smallest shape
]
DGRAD_CASES = [(32, 133, 1024), (250, 7, 260)]

# (B, K, c, heads_fwd, heads_wgrad, heads_dgrad)
#   heads_fwd   MFMA iff B % 32 == 0 and K % 512 == 0
#   heads_wgrad MFMA iff B % 64 == 0 and K % 32 == 0
#   heads_dgrad MFMA iff B % 32 == 0 and K % 128 == 0 and ceil((B / 32) / gy) * 32 * ((c + 1) | 1) * 4 <= 48 KiB, gy = 4 / 2 / 1 for B / 32 >= 8 / >= 2 / else
HEADS_CASES = [
    (32, 512, 40, M, V, M),    # the reference batch: dgrad with gy = 1
    (96, 512, 40, M, V, M),    # dgrad sample tiles 2 + 1
    (160, 512, 40, M, V, M),   # 3 + 2
    (192, 512, 40, M, M, M),   # 3 + 3; wgrad 1.5 trips of the 32-sample loop
    (288, 512, 40, M, V, M),   # 3 + 2 + 2 + 2
    (320, 512, 40, M, M, M),   # 3 + 3 + 2 + 2; wgrad 2.5 trips
    (64, 512, 1, M, M, M),     # one real column beside column 0
    (64, 512, 31, M, M, M),    # last value with one column tile
    (64, 512, 32, M, M, M),    # first value with two
    (64, 512, 33, M, M, M),
    (64, 128, 5, V, M, M),     # mixed routes per entry point
    (64, 96, 5, V, M, V),
    (64, 640, 40, V, M, M),
    (64, 1536, 40, M, M, M),   # three k-blocks in heads_fwd
    (64, 36, 3, V, V, V),      # all VALU at B = 64
    (63, 1024, 40, V, V, V),   # VALU at ragged large B: full 8-sample trips of heads_wgrad_kernel
    (65, 1024, 40, V, V, V),
    (250, 1028, 7, V, V, V),   # last k-chunk 4 wide
    (1152, 128, 40, V, M, M),  # the largest batch whose dgrad tiles fit the 48 KiB (9 tiles per block)
    (1184, 128, 40, V, V, V),  # one tile more: 10 per block
    (2048, 128, 40, V, M, V),  # 16 tiles per block = 84 KiB
    (32, 24576, 40, M, V, M),  # the reference batch at full width
]

DENSE_FWD = {M: "dense_fwd_mfma_kernel", V: "dense_fwd_kernel"}
HEADS_FWD = {M: "heads_fwd_mfma_kernel", V: "heads_fwd_kernel"}
HEADS_WGRAD = {M: "heads_wgrad_mfma_kernel", V: "heads_wgrad_kernel"}
HEADS_DGRAD = {M: "heads_dgrad_mfma_kernel", V: "heads_dgrad_kernel"}


def dense_wgrad_name(route):
    return "dense_wgrad_kernel" if route == V else f"dense_wgrad_mfma_kernel<{route}>"


@pytest.fixture(scope="module")
def ops():
    from littlegan_amd import ops as _ops
    return _ops


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda")


def f64(t):
    return t.detach().cpu().double().numpy()


def draw(rng, mode, *shape, scale=1.0, unit=1.0):
    """"int": integers in [-4, 4] times `unit` (a power of two); "rand": normal values times `scale`, exactly representable in fp32"""
    if mode == "int":
        return rng.integers(-4, 5, shape).astype(np.float64) * unit
    return (rng.standard_normal(shape) * scale).astype(np.float32).astype(np.float64)


def launched(ops, want, fn):
    """fn() with the sticky kernel name cleared in front of it; asserts the kernel it launched"""
    from littlegan_amd import _lib
    _lib.load().lg_clear_kernel()
    out = fn()
    assert ops.last_kernel() == want, (ops.last_kernel(), want)
    return out


class Check:
    """exact equality in the integer form; max-abs error relative to max-abs of the fp64 result, recorded, in the random form"""
    def __init__(self, mode):
        self.mode, self.seen = mode, {}

    def __call__(self, what, got, exp, tol, exact=None):
        got, exp = f64(got), np.asarray(exp, np.float64)
        assert got.shape == exp.shape, (what, got.shape, exp.shape)
        if self.mode == "int" if exact is None else exact:
            assert np.array_equal(got, exp), (what, int((got != exp).sum()), float(np.abs(got - exp).max()))
            return
        err = float(np.abs(got - exp).max() / (np.abs(exp).max() + 1e-30))
        self.seen[what] = max(self.seen.get(what, 0.0), err)
        assert err < tol, (what, err, tol)

    def report(self, head):
        if self.seen:
            print(head + " " + " ".join(f"{k} {v:.2e}" for k, v in self.seen.items()))


def check_dense(ops, case, mode):
    B, K, N, fwd, wg = case
    rng = np.random.default_rng(zlib.crc32(repr(case).encode()) + (mode == "rand"))
    x, w, b, dy = draw(rng, mode, B, K), draw(rng, mode, K, N, scale=0.1), draw(rng, mode, N), draw(rng, mode, B, N)
    dw0, db0 = draw(rng, mode, K, N), draw(rng, mode, N)
    chk = Check(mode)
    xd, wd, dyd = dev(x), dev(w), dev(dy)
    y = launched(ops, DENSE_FWD[fwd], lambda: ops.dense_fwd(xd, wd, dev(b)))
    chk("fwd", y, x @ w + b, 1e-5)
    y = launched(ops, DENSE_FWD[fwd], lambda: ops.dense_fwd(xd, wd, None))
    chk("fwd", y, x @ w, 1e-5)
    dw_e, db_e = x.T @ dy, dy.sum(0)
    dw, db = torch.full((K, N), 7.0, device="cuda"), torch.full((N,), -3.0, device="cuda")   # overwrite: what is there must not show
    launched(ops, dense_wgrad_name(wg), lambda: ops.dense_wgrad(xd, dyd, dw, db, accumulate=False))
    chk("dw", dw, dw_e, 1e-5), chk("db", db, db_e, 1e-5)
    dw, db = dev(dw0), dev(db0)
    launched(ops, dense_wgrad_name(wg), lambda: ops.dense_wgrad(xd, dyd, dw, db, accumulate=True))
    chk("dw", dw, dw0 + dw_e, 1e-5), chk("db", db, db0 + db_e, 1e-5)
    dw = dev(dw0)
    launched(ops, dense_wgrad_name(wg), lambda: ops.dense_wgrad(xd, dyd, dw, None, accumulate=True))   # no bias gradient asked for
    chk("dw", dw, dw0 + dw_e, 1e-5)
    chk.report(f"dense {case[:3]} {mode}:")


def check_heads(ops, case, mode):
    B, K, c, fwd, wg, dg = case
    rng = np.random.default_rng(zlib.crc32(repr(case).encode()) + (mode == "rand"))
    x = draw(rng, mode, B, K)
    u = 2.0 ** -10   # integer form: weights and biases are multiples of 2^-10, the logits stay exact (|z| < 2^9) and moderate
    wpr, wc = draw(rng, mode, K, 1, scale=0.02, unit=u), draw(rng, mode, K, c, scale=0.02, unit=u)
    bpr, bc = draw(rng, mode, 1, unit=u), draw(rng, mode, c, unit=u)
    dz = draw(rng, mode, B, 1 + c)
    chk = Check(mode)
    xd, dzd = dev(x), dev(dz)
    wprd, wcd, bprd, bcd = dev(wpr), dev(wc), dev(bpr), dev(bc)
    # forward: the sigmoid is not exact, so 1e-5 in both forms; the integer form adds the bit comparison across the two routes
    p = launched(ops, HEADS_FWD[fwd], lambda: ops.heads_fwd(xd, wprd, bprd, wcd, bcd))
    p_e = np.concatenate([O.sigmoid(x @ wpr + bpr), O.sigmoid(x @ wc + bc)], 1)
    chk("p", p, p_e, 1e-5, exact=False)
    if mode == "int" and fwd == M:
        p1 = launched(ops, HEADS_FWD[V], lambda: ops.heads_fwd(xd[:B - 1].contiguous(), wprd, bprd, wcd, bcd))
        assert torch.equal(p[:B - 1], p1), int((p[:B - 1] != p1).sum())
    # data gradient
    dx = launched(ops, HEADS_DGRAD[dg], lambda: ops.heads_dgrad(dzd, wprd, wcd))
    chk("dx", dx, dz[:, :1] @ wpr.T + dz[:, 1:] @ wc.T, 1e-5)
    # weight gradients, overwrite and accumulate
    # (the bias gradients are the 1 + c column sums of dz: compared as that one vector, so that the relative measure of the random
    #  form is not taken against a single sum that may cancel to nothing)
    e = (x.T @ dz[:, :1], dz[:, 0].sum(0, keepdims=True), x.T @ dz[:, 1:], dz[:, 1:].sum(0))

    def compare(outs, prior):
        chk("dwpr", outs[0], prior[0] + e[0], 1e-5), chk("dwc", outs[2], prior[2] + e[2], 1e-5)
        chk("db", torch.cat([outs[1], outs[3]]), np.concatenate([prior[1] + e[1], prior[3] + e[3]]), 1e-5)
    outs = (torch.full((K, 1), 7.0, device="cuda"), torch.full((1,), -3.0, device="cuda"),
            torch.full((K, c), 5.0, device="cuda"), torch.full((c,), 2.0, device="cuda"))
    launched(ops, HEADS_WGRAD[wg], lambda: ops.heads_wgrad(xd, dzd, *outs, accumulate=False))
    compare(outs, (0.0, 0.0, 0.0, 0.0))
    prior = (draw(rng, mode, K, 1), draw(rng, mode, 1), draw(rng, mode, K, c), draw(rng, mode, c))
    outs = tuple(dev(a) for a in prior)
    launched(ops, HEADS_WGRAD[wg], lambda: ops.heads_wgrad(xd, dzd, *outs, accumulate=True))
    compare(outs, prior)
    chk.report(f"heads {case[:3]} {mode}:")


@pytest.mark.parametrize("mode", ["int", "rand"])
@pytest.mark.parametrize("case", DENSE_CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_dense_fwd_wgrad_routes(ops, case, mode):
    check_dense(ops, case, mode)


@pytest.mark.parametrize("mode", ["int", "rand"])
@pytest.mark.parametrize("case", DGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dense_dgrad(ops, case, mode):
    B, K, N = case
    rng = np.random.default_rng(zlib.crc32(repr(case).encode()) + (mode == "rand"))
    dy, w = draw(rng, mode, B, N), draw(rng, mode, K, N, scale=0.1)
    chk = Check(mode)
    dx = launched(ops, "dense_dgrad_kernel", lambda: ops.dense_dgrad(dev(dy), dev(w)))
    chk("dx", dx, dy @ w.T, 3e-5)
    chk.report(f"dense_dgrad {case} {mode}:")


@pytest.mark.parametrize("mode", ["int", "rand"])
@pytest.mark.parametrize("case", HEADS_CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_heads_fwd_dgrad_wgrad_routes(ops, case, mode):
    check_heads(ops, case, mode)


def test_heads_dgrad_changes_kernel_at_the_lds_threshold(ops):
    """c = 40: 32 * 41 * 4 = 5248 B per sample tile, 9 tiles = 47232 B fit the 48 KiB, 10 do not; gy = 4 blocks share the tiles, so
    B = 1152 (36 tiles) is the last MFMA batch and B = 1184 (37 tiles) the first that falls back."""
    rng = np.random.default_rng(1152)
    K, c = 128, 40
    wpr, wc = draw(rng, "int", K, 1), draw(rng, "int", K, c)
    names = []
    for B in (1152, 1184):
        dz = draw(rng, "int", B, 1 + c)
        from littlegan_amd import _lib
        _lib.load().lg_clear_kernel()
        dx = ops.heads_dgrad(dev(dz), dev(wpr), dev(wc))
        names.append(ops.last_kernel())
        assert np.array_equal(f64(dx), dz[:, :1] @ wpr.T + dz[:, 1:] @ wc.T)
    assert names == ["heads_dgrad_mfma_kernel", "heads_dgrad_kernel"], names


def test_input_forming_kernels_are_named(ops):
    """the two non-GEMM launchers of dense.hip (values: tests/test_ops_gpu.py::test_step_input_forming_kernels)"""
    a, c = torch.zeros(3, 5, device="cuda"), torch.ones(3, 2, device="cuda")
    launched(ops, "concat_cols_kernel", lambda: ops.concat_cols(a, c))
    launched(ops, "adj_conditions_kernel", lambda: ops.adj_conditions(c, c))


def test_every_gemm_kernel_is_the_route_of_some_case():
    seen = {DENSE_FWD[c[3]] for c in DENSE_CASES} | {dense_wgrad_name(c[4]) for c in DENSE_CASES} | {"dense_dgrad_kernel"}
    seen |= {HEADS_FWD[c[3]] for c in HEADS_CASES} | {HEADS_WGRAD[c[4]] for c in HEADS_CASES} | {HEADS_DGRAD[c[5]] for c in HEADS_CASES}
    want = {"dense_fwd_mfma_kernel", "dense_fwd_kernel", "dense_wgrad_kernel", "dense_dgrad_kernel", "heads_fwd_mfma_kernel",
            "heads_fwd_kernel", "heads_wgrad_mfma_kernel", "heads_wgrad_kernel", "heads_dgrad_mfma_kernel", "heads_dgrad_kernel"}
    want |= {f"dense_wgrad_mfma_kernel<{m}>" for m in range(1, 6)}
    assert seen == want, seen ^ want


# ---------------------------------------------------------------------------------------------------------------- the kill switch
KILL_DENSE = (64, 133, 256, V, V)      # MFMA shapes (forward and MT = 5 weight gradient) that the switch sends to the VALU kernels
KILL_HEADS = (64, 512, 40, V, V, V)


def kill_switch_child():
    """body of the child process of test_kill_switch_routes_everything_to_the_valu_kernels (LG_NO_SKINNY_MFMA=1 in its environment)"""
    from littlegan_amd import ops as _ops
    assert os.environ.get("LG_NO_SKINNY_MFMA") == "1"
    check_dense(_ops, KILL_DENSE, "int")
    check_heads(_ops, KILL_HEADS, "int")
    torch.cuda.synchronize()


def test_kill_switch_routes_everything_to_the_valu_kernels():
    """LG_NO_SKINNY_MFMA is read once per process, so a fresh child: shapes that take the MFMA kernels run on the VALU kernels,
    named so, with exactly the integer results.  One child, no retry."""
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_skinny_gpu as T; T.kill_switch_child(); print('child ok')"
            % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "LG_NO_SKINNY_MFMA": "1"}, timeout=120,
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
