"""The memory contract of every kernel entry point, checked with guard bands (tests/guards.py).

The op tests compare values with the fp64 oracle; none of them looks at WHERE a kernel reads and writes.  Every row of CASES below
is a small function run(ops, alloc) that calls one op wrapper, or a short producer-to-consumer chain, at the smallest shape that
still reaches the kernel it names.  `alloc` hands it every device buffer.  The test body runs the row four times:

  plain, plain2   plain tensors, torch.empty outputs, the pooled workspace (never below 1 MiB)
  A               every buffer inside 0xFF red zones, outputs pre-filled with 0xFF, every workspace of EXACTLY the advertised
                  size, 0xFF-filled, inside red zones
  B               the same with 0x00
  C               the same with 0x3F (a finite, non-zero value in every floating type)

and asserts  1. control: plain == plain2 bit for bit;  2. same route: the advertised workspace size selects the kernel the pool
selects (lg_last_kernel after every call of the chain);  3. same bits: every result of A, B and C equals plain — the result does not
depend on bytes outside the inputs, nor on what the workspace or the outputs held before;  4. nothing else touched: every red zone
intact, every input bit-identical to what went in (and, for a row with exact_sizing, the workspaces handed over are exactly its sizing
entries);  5. everything written: no output element of A still holds 0xFF..FF where the
plain result is finite;  6. oracle: plain against oracle/np_oracle.py (or the op's bit-exact restatement) at the tolerances the op
has in its own test module — imported from there, none is introduced here.

Each row names the entry points it covers; tests/test_guards_cpu.py checks that every pointer-taking function of the C ABI (every
include/littlegan_*.h) is named by a row or listed in EXEMPT with its reason, so a new entry point fails there until it gets a row."""
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import input_oracle as I  # noqa: E402
from oracle import np_oracle as O  # noqa: E402
from guards import Guarded, called, describe, exact_workspaces  # noqa: E402
from test_ops_gpu import TOL, rel  # noqa: E402
from test_launch_shapes_gpu import _norm_ref, _rms  # noqa: E402
from test_tail_ops_gpu import BIAS_CASES  # noqa: E402
from test_skinny_gpu import (DENSE_CASES, DENSE_FWD, DGRAD_CASES, HEADS_CASES, HEADS_DGRAD, HEADS_FWD, HEADS_WGRAD,  # noqa: E402
                             dense_wgrad_name)
from test_dropout_cpu import drop_mult, keep_mask  # noqa: E402
from test_diffaug_cpu import diffaug_adjoint_np, diffaug_np, draw_params, extreme_records  # noqa: E402
from test_diffaug_gpu import SHAPES as DIFFAUG_SHAPES, coef_sum  # noqa: E402
from test_ema_cpu import ema_update  # noqa: E402
from test_ema_gpu import ADAM, BOUND, DECAY  # noqa: E402
from test_metrics_cpu import CASES as PAIR_CASES, MARGIN, ball_margin, dot_eps, make_sets, oracle_d2, oracle_poly  # noqa: E402
from test_fid_stream import check_stats, eigh_reference, fixture  # noqa: E402
from test_r1_cpu import EXACT_LOSS0 as R1_LOSS0, EXACT_WEIGHT, exact_colsum_case, exact_seed_case, heads_seed_wpr  # noqa: E402
from test_r1_gpu import _bits as i32, _np_bits as np_i32  # noqa: E402
from test_ada_cpu import ada_accumulate_np, ada_adjust_np, draw_params_gated  # noqa: E402
from test_ada_gpu import FULL, PER_ROW, heads_mix, u32, words  # noqa: E402
from test_gan_loss_cpu import (EXACT_LOSS0 as GAN_LOSS0, EXACT_W_PR, KIND_NO, ROLE_D_FAKE, ROLE_D_REAL, ROLE_G,  # noqa: E402
                               exact_case)
from test_gan_loss_gpu import HEADS_CASES as LOGIT_HEADS_CASES, _heads_data, _heads_operands  # noqa: E402
from test_geom_cpu import FULL as GEOM_FULL, extreme_records as geom_extreme_records, geom_adjoint_np, geom_np, geom_records, key_of, usable  # noqa: E402
from test_rel_cpu import EXACT_LOSS0 as PAIR_LOSS0, EXACT_W_PR as PAIR_W_PR, KIND_NO as PAIR_KIND_NO, SIDE_OTHER, SIDE_SELF, exact_pair_case  # noqa: E402
from test_rel_gpu import W_FAKE, _seed_halves  # noqa: E402
from test_lr_schedule_cpu import settings as sched_settings  # noqa: E402
from test_lr_schedule_gpu import B1, B2, EPS, RATES, _t as as_i32  # noqa: E402
from test_adj_fused_gpu import hand_moments  # noqa: E402
from test_grad_guard_cpu import CH  # noqa: E402
from test_grad_guard_gpu import _c_from, _data as guard_data, _rec_np, _ulps  # noqa: E402
from test_blur_cpu import blur_np  # noqa: E402
from test_blur_gpu import bound as blur_bound, images as blur_images, state_words as blur_state_words  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16, F64, U8, I32, I64 = torch.float32, torch.bfloat16, torch.float64, torch.uint8, torch.int32, torch.int64
ALPHA = 0.3   # test_launch_shapes_gpu.ALPHA, which _norm_ref is written for

# Public functions with a pointer parameter that no row runs, each with its reason.  (lg_last_error, lg_last_kernel and the pure
# queries take no pointer: the ledger does not ask for them.)
EXEMPT = {
    "lg_contention_probe": "run-time probe of bench.py (CU footprint rehearsal), not part of the training or evaluation path",
    "lg_set_clock_census": "run-time probe: registers a counter buffer that instrumented kernels add clock ticks to",
    "lg_clock_sample": "run-time probe: spins for a given time and adds clock ticks; its result is a timing, never reproducible",
}


# ------------------------------------------------------------------------------------------------------------------ the harness
def arr(seed, *shape, scale=1.0, shift=0.0):
    """seeded fp32 values (numpy), the same in every run of a row and in its oracle"""
    return (np.random.default_rng(seed).standard_normal(shape) * scale + shift).astype(np.float32)


def bf(a):
    """the bf16 mirror (RNE, as the device kernels round) of an fp32 numpy array, as a CPU tensor"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(BF16)


def q(a):
    """the values that mirror holds, fp64"""
    return O.bf16_round(np.asarray(a, np.float64))


def f64(t):
    return t.detach().double().cpu().numpy()


def crc(*x):
    import zlib
    return zlib.crc32(repr(x).encode())


class Alloc:
    """How a row obtains its device buffers.  mode "plain": ordinary tensors, outputs torch.empty.  mode "guard": every buffer
    inside red zones holding `byte`, outputs pre-filled with `byte`."""

    def __init__(self, mode, byte=0xFF):
        self.mode, self.byte = mode, byte
        self.bufs = []   # (name, kind, Guarded, snapshot of the payload bytes | None)

    def _cpu(self, a, dtype):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        return (t if dtype is None else t.to(dtype)).contiguous()

    def _put(self, name, kind, t):
        if self.mode == "plain":
            return t.cuda()
        g = Guarded(t.shape, t.dtype, "cuda", fill=t.cuda(), zone=self.byte)
        self.bufs.append((name, kind, g, g.payload.clone() if kind == "input" else None))
        return g.t

    def inp(self, name, a, dtype=None):
        """an input: its red zones AND its payload must come back unchanged"""
        return self._put(name, "input", self._cpu(a, dtype))

    def state(self, name, a, dtype=None):
        """a buffer the op updates in place (accumulate=True outputs, optimizer state): seeded values, red zones checked"""
        return self._put(name, "state", self._cpu(a, dtype))

    def out(self, name, shape, dtype=F32):
        if self.mode == "plain":
            return torch.empty(shape, dtype=dtype, device="cuda")
        g = Guarded(shape, dtype, "cuda", fill=self.byte, zone=self.byte)
        self.bufs.append((name, "output", g, None))
        return g.t

    def problems(self):
        out = []
        for name, kind, g, snap in self.bufs:
            bad = g.intact()
            if bad:
                out.append(f"{kind} '{name}' ({g.nbytes} bytes): written outside the tensor: {describe(bad)}")
            if snap is not None and not torch.equal(g.payload, snap):
                d = (g.payload != snap).nonzero().flatten()
                out.append(f"input '{name}' ({g.nbytes} bytes): the op changed it: {describe([int(i) for i in d[:8].tolist()])}")
        return out


class Trace:
    """the kernel name after every call of a chain: "label=kernel;label=kernel" (lg_last_kernel is sticky: cleared in between)"""

    def __init__(self, ops):
        self.ops, self.parts = ops, []
        ops._lib.load().lg_clear_kernel()

    def __call__(self, label):
        self.parts.append(f"{label}={self.ops.last_kernel()}")
        self.ops._lib.load().lg_clear_kernel()

    def __str__(self):
        return ";".join(self.parts)


class Row:
    """id; covers: the entry points the row runs; run(ops, alloc) -> dict of results (tensors, or plain Python values; "_route":
    the Trace); check(res): the oracle comparison of the plain results; route: substrings the plain route must contain; sizing:
    [(*_workspace_bytes name, args)] of the workspaces the row uses; wgrad: (B, Hs, Ws, cb, cs, dtype) of a conv weight gradient;
    exact_sizing: the guarded runs are handed exactly one workspace per sizing entry, of that size (an older row may list a size once
    and take it several times, or take the heads' workspace without an entry)."""

    def __init__(self, id, covers, run, check=None, route=(), sizing=(), wgrad=None, exact_sizing=False):
        self.id, self.covers, self.run, self.check, self.exact_sizing = id, tuple(covers), run, check, exact_sizing
        self.route = (route,) if isinstance(route, str) else tuple(route)
        self.sizing, self.wgrad = list(sizing), wgrad
        if wgrad is not None:
            self.sizing.append(("lg_wgrad_workspace_bytes", tuple(wgrad)))

    def __repr__(self):
        return self.id


CASES = []


def row(*a, **k):
    CASES.append(Row(*a, **k))


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(U8)


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))
    return a == b


def _diff(what, plain, got):
    bad = [k for k in plain if k not in got or not _same(plain[k], got[k])] + [k for k in got if k not in plain]
    msgs = []
    for k in bad:
        if k in plain and k in got and torch.is_tensor(plain[k]) and torch.is_tensor(got[k]) and plain[k].shape == got[k].shape:
            ne = (_bits(plain[k]) != _bits(got[k])).nonzero().flatten()
            msgs.append(f"'{k}': {ne.numel()} byte(s) differ, first at byte {int(ne[0])} of {_bits(plain[k]).numel()}")
        else:
            msgs.append(f"'{k}': {plain.get(k, '<absent>')!r} / {got.get(k, '<absent>')!r}")
    return f"{what}: " + "; ".join(msgs) if msgs else ""


def _stale(plain, got):
    """names of results of the 0xFF run with an element that still is 0xFF..FF where the plain result is a finite value (an integer: not -1)"""
    out = []
    for k, t in got.items():
        if not torch.is_tensor(t) or k not in plain or not torch.is_tensor(plain[k]) or plain[k].shape != t.shape or t.numel() == 0:
            continue
        item = t.element_size()
        ff = (_bits(t).reshape(-1, item) == 0xFF).all(1)
        p = plain[k].reshape(-1)
        real = torch.isfinite(p) if p.is_floating_point() else (p != -1)
        n = int((ff & real).sum())
        if n:
            out.append(f"'{k}': {n} of {t.numel()} elements never written, first at element {int((ff & real).nonzero()[0])}")
    return out


def _once(row_, ops, monkeypatch, mode, byte=0xFF):
    alloc = Alloc(mode, byte)
    with monkeypatch.context() as mp:
        ws = exact_workspaces(mp, ops, fill=byte) if mode == "guard" else None
        names = called(mp, ops)
        ops._lib.load().lg_clear_kernel()
        res = dict(row_.run(ops, alloc))
        route = str(res.pop("_route")) if "_route" in res else ops.last_kernel()
        torch.cuda.synchronize()
    return res, route, alloc, ws, set(names)


@pytest.fixture(scope="module")
def ops():
    from littlegan_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("case", CASES, ids=lambda r: r.id)
def test_memory_contract(case, ops, monkeypatch):
    plain, route, _, _, names = _once(case, ops, monkeypatch, "plain")
    missing = set(case.covers) - names
    assert not missing, f"the row claims entry points it never fetched: {sorted(missing)} (fetched {sorted(names)})"
    plain2, route2, _, _, _ = _once(case, ops, monkeypatch, "plain")
    # 1. control
    d = _diff("two plain runs differ (the op is not reproducible; nothing below can be read)", plain, plain2)
    assert not d and route == route2, d or (route, route2)
    print(f"{case.id}: route {route}")
    for want in case.route:
        assert want in route, f"route {route!r} does not contain {want!r}"
    # C: 0x3F3F3F3F is 0.747 as fp32 (0x3F3F = 0.746 as bf16): an overrun that READS what it then rewrites (y[n] = a x[n] + b y[n])
    # returns NaN for NaN and 0 for 0 and so leaves the zones of A and B as they were; it does not return 0.747 for 0.747
    for tag, byte in (("A (0xFF)", 0xFF), ("B (0x00)", 0x00), ("C (0x3F)", 0x3F)):
        got, route_g, alloc, ws, _ = _once(case, ops, monkeypatch, "guard", byte)
        # 2. same route
        assert route_g == route, f"run {tag}: workspaces of the advertised size take another route: {route_g!r}, the pool {route!r}"
        # 4. nothing else touched
        bad = alloc.problems() + [f"{what}: written outside its advertised size: {describe(offs)}" for what, offs in ws.damaged()]
        assert not bad, f"run {tag}: " + " | ".join(bad)
        if case.exact_sizing:   # the workspaces handed over are the row's sizing entries, no more and no fewer (none for a row without one)
            handed = sorted(nb for _, nb, _ in ws.handed)
            sized = sorted(int(getattr(ops._lib.load(), fn)(*args)) for fn, args in case.sizing)
            assert handed == sized, f"run {tag}: workspaces of {handed} bytes handed over, the sizing entries give {sized}"
        # 5. everything written
        if byte == 0xFF:
            stale = _stale(plain, got)
            assert not stale, f"run {tag}: " + " | ".join(stale)
        # 3. same bits
        d = _diff(f"run {tag} differs from the plain run (foreign bytes, stale workspace or stale output contents show in the result)",
                  plain, got)
        assert not d, d
    # 6. oracle
    if case.check is not None:
        case.check(plain)


# ------------------------------------------------------------------------------------------------------------------ shared pieces
def _pack(ops, alloc, w, cb, cs, dtype):
    return ops.conv_pack(alloc.inp("w", w), cb, cs, dtype, out=alloc.out("pack", (ops.conv_pack_bytes(cb, cs, dtype),), U8))


def _gb(alloc, gamma=1.2, beta=0.1, tag=""):
    return alloc.inp("gamma" + tag, np.array([gamma], np.float32)), alloc.inp("beta" + tag, np.array([beta], np.float32))


def _moments_ok(st, z, tol):
    """statistics records against the moments of the fp64 oracle result z"""
    B = z.shape[0]
    ef = z.reshape(B, -1)
    assert rel(st[:, 0].double() + st[:, 4].double(), ef.mean(1)) < tol and rel(st[:, 1], ef.std(1)) < tol


def _stats_bytes(up, B, Hs, Ws, N):
    return ("lg_conv_stats_workspace_bytes", (int(up), B, Hs, Ws, N))


# ------------------------------------------------------------------------------------------------------------------ conv forward / data gradient / forward with moments
def conv_rows(kind, case, dtype, route=()):
    """kind "down": Conv2D(cs, 5, 2, same) on x [B,2Hs,2Ws,cb]; "up": Conv2DTranspose(cb, 5, 2, same) on x [B,Hs,Ws,cs].  Forward,
    data gradient and forward-with-moments through the fp32 entry points, as tests/test_ops_gpu.py calls them."""
    B, Hs, Ws, cb, cs = case
    down = kind == "down"
    big, small = (B, 2 * Hs, 2 * Ws, cb), (B, Hs, Ws, cs)

    @functools.lru_cache(maxsize=None)
    def data():
        s = crc(kind, case)
        return (arr(s, *(big if down else small)), arr(s + 1, 5, 5, cb, cs, scale=0.1), arr(s + 2, cs if down else cb),
                arr(s + 3, *(small if down else big)))

    def run(ops, alloc):
        x, w, b, dy = data()
        tr = Trace(ops)
        xd, bd, dyd = alloc.inp("x", x), alloc.inp("bias", b), alloc.inp("dy", dy)
        pack = _pack(ops, alloc, w, cb, cs, dtype)
        gm, bt = _gb(alloc)
        if down:
            y = ops.conv2d_s2_fwd(xd, pack, bd, cs, dtype, out=alloc.out("y", small))
            tr("fwd")
            dx = ops.conv2d_s2_dgrad(dyd, pack, cb, dtype, out=alloc.out("dx", big))
            tr("dgrad")
            z, st = ops.conv2d_s2_fwd_stats(xd, pack, bd, cs, dtype, gm, bt)
        else:
            y = ops.convT_s2_fwd(xd, pack, bd, cb, dtype, out=alloc.out("y", big))
            tr("fwd")
            dx = ops.convT_s2_dgrad(dyd, pack, cs, dtype, out=alloc.out("dx", small))
            tr("dgrad")
            z, st = ops.convT_s2_fwd_stats(xd, pack, bd, cb, dtype, gm, bt)
        tr("stats")
        res = dict(pack=pack, y=y, dx=dx, z=z, fused=st is not None, _route=tr)
        if st is not None:
            res["stats"] = st
        return res

    def check(res):
        x, w, b, dy = (a.astype(np.float64) for a in data())
        if down:
            y_e, dx_e = O.conv2d(x, w, b, 2), O.conv2d_bwd(x, w, dy, 2)[0]
        else:
            y_e, dx_e = O.conv2d_transpose(x, w, b, 2), O.conv2d_transpose_bwd(x, w, dy, 2)[0]
        assert rel(res["y"], y_e) < TOL[dtype] and rel(res["dx"], dx_e) < TOL[dtype] and rel(res["z"], y_e) < TOL[dtype]
        if res["fused"]:   # fused moments == moments of the produced tensor (test_bf16_mirror_operands_are_bit_identical)
            zf = res["z"].double().reshape(B, -1)
            st = res["stats"]
            assert rel(st[:, 0], zf.mean(1).cpu().numpy()) < 1e-6 and rel(st[:, 1], zf.std(1, unbiased=False).cpu().numpy()) < 1e-6

    fwd = ("lg_conv2d_s2_fwd", "lg_conv2d_s2_dgrad_m16", "lg_conv2d_s2_fwd_stats") if down else \
          ("lg_convT_s2_fwd", "lg_convT_s2_dgrad_m16", "lg_convT_s2_fwd_stats")
    row(f"conv-{kind}-{'x'.join(map(str, case))}-{'bf16' if dtype else 'f32'}", ("lg_conv_pack",) + fwd, run, check, route,
        sizing=[_stats_bytes(not down, B, Hs, Ws, cs if down else cb)])


def _r3(fwd, dgrad, stats=None):
    """the whole route of a conv row.  An empty name: the launch path names no kernel (the VALU kernels of n3_kernels.hip)."""
    return f"fwd={fwd};dgrad={dgrad};stats={fwd if stats is None else stats}"


IG, HALO = "conv_igemm_kernel", "conv_halo_kernel"
for _dt, _t in ((0, "f32"), (1, "bf16")):
    conv_rows("down", (3, 5, 6, 32, 64), _dt, _r3(IG + "<DOWN>", IG + "<UP>"))                 # gather kernel
    conv_rows("up", (3, 5, 6, 32, 64), _dt, _r3(IG + "<UP>", IG + "<DOWN>"))
    conv_rows("down", (3, 7, 5, 3, 64), _dt, _r3(IG + "<PATCH>", IG + "<UP>"))                  # 3-channel patch, odd map
    conv_rows("down", (1, 16, 16, 3, 32), _dt, _r3(IG + "<PATCH>", ""))                          # its data gradient: the n3 kernel
    conv_rows("down", (3, 8, 8, 32, 64), _dt, _r3(f"{HALO}<{_t},DOWN>", f"{HALO}<{_t},UP,K-sliced>"))    # HALO_CASES ("down", 3, 8, 8, 32, 64)
    conv_rows("up", (2, 4, 4, 32, 32), _dt, _r3(f"{HALO}<{_t},UP,K-sliced>", f"{HALO}<{_t},DOWN>"))      # ("up", 2, 4, 4, 32, 32)
    # ("up", 2, 16, 16, 64, 3): the conv1 data-gradient form; bf16: the forward with moments is the bf16-source patch kernel
    conv_rows("down", (2, 16, 16, 3, 64), _dt, _r3(IG + "<PATCH>", "", "patch_p16_kernel<2,64>" if _dt else None))
    # ("up", 5, 2, 2, 64, 64): several samples per tile; the data gradient (a 1 x 1 result map) is the gather kernel's
    conv_rows("up", (5, 2, 2, 64, 64), _dt, _r3(f"{HALO}<{_t},UP,K-sliced>", IG + "<DOWN>"))
    conv_rows("up", (2, 8, 9, 64, 128), _dt, _r3(IG + "<UP>", IG + "<DOWN>"))                   # transposed conv, odd width
    conv_rows("up", (2, 3, 3, 256, 384), _dt, _r3(IG + "<UP>", IG + "<DOWN>"))


# ------------------------------------------------------------------------------------------------------------------ persistent bf16 kernels
def persistent_rows(kind, case, route):
    """The bf16 activation path as the step runs it: conv with deferred moments -> instnorm_apply finishing them in its own launch
    (the Moments come from an exact-size buffer) -> the matching fused data gradient -> instnorm_bwd from its NormPartials.
    kind "down": case = (B, Hm, Wm, Cs, N) of test_bf16_path_down_kernels_small_shapes; "up": (B, Hs, Ws, Cs, N) of ..._up_..."""
    B, Hm, Wm, Cs, N = case
    down = kind == "down"
    src = (B, 2 * Hm, 2 * Wm, Cs) if down else (B, Hm, Wm, Cs)
    dst = (B, Hm, Wm, N) if down else (B, 2 * Hm, 2 * Wm, N)
    wshape = (5, 5, Cs, N) if down else (5, 5, N, Cs)
    cb, cs = (Cs, N) if down else (N, Cs)

    @functools.lru_cache(maxsize=None)
    def data():
        s = crc("persistent", kind, case)
        return arr(s, *src), arr(s + 1, *wshape, scale=0.1), arr(s + 2, N, scale=0.2)

    def run(ops, alloc):
        x, w, b = data()
        tr = Trace(ops)
        x16, bd = alloc.inp("x16", bf(x)), alloc.inp("bias", b)
        pack = _pack(ops, alloc, w, cb, cs, 1)
        gm, bt = _gb(alloc, 1.0, 0.0)
        fwd = ops.conv2d_s2_fwd_stats if down else ops.convT_s2_fwd_stats
        z16, mom = fwd(None, pack, bd, N, 1, gm, bt, x16=x16, z16=True, alpha=ALPHA, defer_stats=True)
        tr("fwd")
        deferred = isinstance(mom, ops.Moments)
        h16 = alloc.out("h16", dst, BF16)
        ops.instnorm_apply(z16, mom, None, 0, 1, ALPHA, out16=h16, want_f32=False)
        st = ops.stats_tensor(mom)
        dgrad = ops.convT_s2_dgrad if down else ops.conv2d_s2_dgrad   # the same contraction, no bias
        g16, parts = dgrad(None, pack, N, 1, dy16=x16, out_bf16=True, fuse=(z16, st, ALPHA))
        tr("dgrad")
        dgm, dbt = alloc.out("dgamma", (1,)), alloc.out("dbeta", (1,))
        dz16 = alloc.out("dz16", dst, BF16)
        ops.instnorm_bwd(z16, st, g16, dgm, dbt, 0, 1, ALPHA, out16=dz16, want_f32=False, partials=parts)
        return dict(z16=z16, stats=st, h16=h16, g16=g16, dz16=dz16, dgamma=dgm, dbeta=dbt, deferred=deferred,
                    nparts=None if parts is None else parts.nparts, _route=tr)

    def check(res):
        x, w, b = (a.astype(np.float64) for a in data())
        exp = O.conv2d(q(x), q(w), b, 2) if down else O.conv2d_transpose(q(x), q(w), b, 2)
        assert rel(res["z16"].float(), exp) < TOL[1]
        _moments_ok(res["stats"], exp, 2e-5)
        gexp = O.conv2d(q(x), q(w), np.zeros(N), 2) if down else O.conv2d_transpose(q(x), q(w), np.zeros(N), 2)
        assert rel(res["g16"].float(), gexp) < TOL[1]
        _norm_chain_ok(res["z16"], res["stats"], res["g16"], res["dz16"], res["dgamma"], res["dbeta"], res["h16"])

    halo = "conv_halo" in route
    covers = ["lg_conv_pack", "lg_conv2d_s2_fwd_stats" if down else "lg_convT_s2_fwd_stats", "lg_instnorm_leaky_apply_z16_p",
              "lg_convT_s2_dgrad_nf" if down else "lg_conv2d_s2_dgrad_nf", "lg_instnorm_leaky_bwd_z16" if halo else "lg_instnorm_leaky_bwd_z16_p"]
    row(f"persistent-{kind}-{'x'.join(map(str, case))}", covers, run, check, ("fwd=" + route, "dgrad=" + route),
        sizing=[_stats_bytes(not down, B, Hm, Wm, N), _stats_bytes(down, B, Hm, Wm, N), ("lg_instnorm_bwd_db_workspace_bytes", (B, int(np.prod(dst[1:])), 0))])


def _affine_ref(zs, gs, ss):
    """fp64 (dgamma, dbeta) = (sum g' c / (sigma + 1e-3), sum g') of the norm backward from the kernel's own inputs and statistics
    records, the LeakyReLU mask in the kernels' fp32 order (as _norm_ref)"""
    s32 = ss.astype(np.float32)
    y32 = (s32[:, 2:3] * ((zs.astype(np.float32) - s32[:, 0:1]) - s32[:, 4:5])).astype(np.float32) + s32[:, 3:4]
    gp = np.where(y32 > 0, gs, ALPHA * gs)
    c = zs - (ss[:, 0] + ss[:, 4])[:, None]
    return float((gp * c / (ss[:, 1][:, None] + 1e-3)).sum()), float(gp.sum())


def _affine_ok(dgm, dbt, zs, gs, ss):
    """the bound of test_instnorm_stats_apply_bwd"""
    dg_e, db_e = _affine_ref(zs, gs, ss)
    assert abs(float(dgm) - dg_e) < 2e-5 * max(1.0, abs(dg_e)) * 10, (float(dgm), dg_e)
    assert abs(float(dbt) - db_e) < 2e-5 * max(1.0, abs(db_e)) * 10, (float(dbt), db_e)


def _colsum_ok(db, dx):
    """db against the column sums of the dx written in the same pass: test_instnorm_bwd_fused_bias_column_sums"""
    C = dx.shape[-1]
    exp = dx.double().reshape(-1, C).sum(0).cpu().numpy()
    scale = np.abs(f64(dx)).reshape(-1, C).sum(0).max()   # the sums cancel to ~0: compare to the mass
    assert np.abs(f64(db) - exp).max() < 2e-6 * scale


def _norm_chain_ok(z16, st, g16, dz16, dgm, dbt, h16=None):
    """dz of the norm backward against _norm_ref (tests/test_launch_shapes_gpu.py: fp64 from the kernel's own inputs and statistics
    records, 6e-4 rms against the bf16-rounded reference); dgamma / dbeta against the fp64 sums of the same quantities at the bound
    of test_instnorm_stats_apply_bwd; the activated map against the same records."""
    B = z16.shape[0]
    zs, gs, ss = f64(z16).reshape(B, -1), f64(g16).reshape(B, -1), f64(st)
    assert _rms(f64(dz16).reshape(B, -1), O.bf16_round(_norm_ref(zs, gs, ss))) < 6e-4
    _affine_ok(dgm, dbt, zs, gs, ss)
    if h16 is not None:
        s32 = ss.astype(np.float32)
        y32 = (s32[:, 2:3] * ((zs.astype(np.float32) - s32[:, 0:1]) - s32[:, 4:5])).astype(np.float32) + s32[:, 3:4]
        h = np.where(y32 > 0, y32, np.float32(ALPHA) * y32)
        assert rel(h16.float(), h.astype(np.float64).reshape(z16.shape)) < TOL[1]


persistent_rows("down", (2, 8, 8, 32, 128), "conv_down3_kernel<PAIR>")
persistent_rows("down", (1, 8, 16, 32, 64), "conv_down3_kernel<NW=64>")
persistent_rows("down", (1, 8, 16, 32, 128), "conv_down3_kernel<NW=128>")
persistent_rows("down", (3, 8, 8, 32, 128), "conv_halo_kernel")                     # odd batch on the 8 x 8 level
persistent_rows("up", (2, 8, 16, 64, 128), "conv_up4_kernel")
persistent_rows("up", (2, 8, 8, 64, 128), "conv_up4_kernel<PAIR>")
persistent_rows("up", (2, 8, 16, 128, 64), "conv_up3_kernel<128,64>")
persistent_rows("up", (2, 8, 16, 64, 32), "conv_up3_kernel<64,32,4w>")


def zn_row(case):
    """NORM form of conv_down3.hip: test_down_conv_normalises_while_staging"""
    B, Hm, Wm, Cs, N = case

    @functools.lru_cache(maxsize=None)
    def data():
        s = crc("zn", case)
        zin = arr(s, B, 2 * Hm, 2 * Wm, Cs) * (0.5 + 2.0 * np.random.default_rng(s + 9).random((B, 1, 1, 1), dtype=np.float32)) \
            + arr(s + 8, B, 1, 1, 1)
        return zin.astype(np.float32), arr(s + 1, 5, 5, Cs, N, scale=0.05), arr(s + 2, N, scale=0.1)

    def run(ops, alloc):
        zin, w, b = data()
        tr = Trace(ops)
        gm, bt = _gb(alloc, 0.9, 0.2)
        gm2, bt2 = _gb(alloc, 1.2, -0.1, "2")
        zin16 = alloc.out("zin16", zin.shape, BF16)
        st_in = ops.instnorm_stats(alloc.inp("zin", zin), gm, bt, 0, ALPHA, stats=alloc.out("st_in", (B, 8)), x16_out=zin16)
        h16 = alloc.out("h16", zin.shape, BF16)
        ops.instnorm_apply(zin16, st_in, None, 0, 1, ALPHA, out16=h16, want_f32=False)
        pack = _pack(ops, alloc, w, Cs, N, 1)
        assert ops.conv2d_s2_fwd_stats_zn_supported(B, 2 * Hm, 2 * Wm, Cs, N, 1)
        z, st = ops.conv2d_s2_fwd_stats_zn(zin16, st_in, ALPHA, pack, alloc.inp("bias", b), N, 1, gm2, bt2)
        tr("zn")
        return dict(zin16=zin16, st_in=st_in, h16=h16, z=z, stats=st, _route=tr)

    def check(res):
        _, w, b = data()
        exp = O.conv2d(f64(res["h16"]), q(w), b.astype(np.float64), 2)
        assert rel(res["z"].float(), exp) < TOL[1]
        _moments_ok(res["stats"], exp, 2e-5)

    row(f"persistent-down-NORM-{'x'.join(map(str, case))}",
        ("lg_conv2d_s2_fwd_stats_zn", "lg_instnorm_leaky_stats_z16", "lg_instnorm_leaky_apply_z16",
         "lg_instnorm_stats_finalize"), run, check, "zn=conv_down3_kernel<NW=128,NORM>",
        sizing=[_stats_bytes(0, B, Hm, Wm, N), ("lg_instnorm_workspace_bytes", (B, 4 * Hm * Wm * Cs))])


zn_row((2, 8, 16, 32, 128))


def bwdnorm_row(B, s_h, s_w, cb, cs):
    """BWDNORM form of conv_down3.hip through convT_s2_dgrad_bn with instnorm_bwd_coef, at the smallest shape
    convT_s2_dgrad_bn_supported accepts (one 8 x 16 tile of 64 columns): the final layer's fused data gradient produces the
    level's NormPartials, the coefficients are formed from them, and the result is compared with the two-pass chain
    (instnorm_bwd writing dz16, then convT_s2_dgrad with the sums of the level below), which must agree bit for bit."""
    shape = (B, 2 * s_h, 2 * s_w, cb)

    @functools.lru_cache(maxsize=None)
    def data():
        s = crc("bn", B, s_h, s_w, cb, cs)
        z = arr(s, *shape) * (0.5 + 2.0 * np.random.default_rng(s + 9).random((B, 1, 1, 1), dtype=np.float32)) + arr(s + 8, B, 1, 1, 1)
        return (z.astype(np.float32), arr(s + 1, *shape), arr(s + 2, 5, 5, cb, cs, scale=0.05), arr(s + 3, B, s_h, s_w, cs, scale=1.3, shift=0.2))

    def sums(z16, st, g16):
        """{sum g', sum g' c} per (sample, part) as a producer would leave them ([B][4][2] doubles), from a torch reduction
        (test_backward_normalising_data_gradient_at_the_adjuster_batch)"""
        zz, gg = z16.double().reshape(B, 4, -1), g16.double().reshape(B, 4, -1)
        mu, a_, b_ = (st[:, 0].double() + st[:, 4].double()).view(B, 1, 1), st[:, 2].view(B, 1, 1), st[:, 3].view(B, 1, 1)
        c32 = (z16.float().reshape(B, 4, -1) - st[:, 0].view(B, 1, 1)) - st[:, 4].view(B, 1, 1)
        gp = torch.where(a_ * c32 + b_ > 0, gg, ALPHA * gg)
        return torch.stack([gp.sum(-1), (gp * (zz - mu)).sum(-1)], -1).contiguous()

    def run(ops, alloc):
        z, g, w, zl = data()
        tr = Trace(ops)
        gm, bt = _gb(alloc, 0.9, 0.15)
        gml, btl = _gb(alloc, 1.1, -0.05, "_l")
        z16, g16, zl16 = alloc.inp("z16", bf(z)), alloc.inp("g16", bf(g)), alloc.inp("zl16", bf(zl))
        st = ops.instnorm_stats(alloc.inp("z", q(z).astype(np.float32)), gm, bt, 0, ALPHA, stats=alloc.out("st", (B, 8)))
        stl = ops.instnorm_stats(alloc.inp("zl", q(zl).astype(np.float32)), gml, btl, 0, ALPHA, stats=alloc.out("stl", (B, 8)))
        pack = _pack(ops, alloc, w, cb, cs, 1)
        assert ops.convT_s2_dgrad_bn_supported(B, s_h, s_w, cb, cs, 1)
        sm = alloc.inp("sums", sums(z16, st, g16).cpu().view(U8).reshape(-1))
        P = ops.NormPartials(sm, 4, ALPHA, shape)
        coef = ops.instnorm_bwd_coef(z16, st, P)
        g_bn, p_bn = ops.convT_s2_dgrad_bn(z16, g16, coef, ALPHA, pack, cs, fuse=(zl16, stl, ALPHA))
        tr("bn")
        sums_bn = p_bn.buf[:B * p_bn.nparts * 16].clone().view(F64)
        dz16 = alloc.out("dz16", shape, BF16)
        ops.instnorm_bwd(z16, st, g16, None, None, 0, 1, ALPHA, out16=dz16, want_f32=False, partials=P)
        g_ref, p_ref = ops.convT_s2_dgrad(None, pack, cs, 1, dy16=dz16, out_bf16=True, fuse=(zl16, stl, ALPHA))
        tr("ref")
        sums_ref = p_ref.buf[:B * p_ref.nparts * 16].clone().view(F64)
        return dict(coef=coef, g_bn=g_bn, sums_bn=sums_bn, dz16=dz16, g_ref=g_ref, sums_ref=sums_ref, st=st, _route=tr)

    def check(res):
        z, g, w, _ = data()
        assert torch.equal(res["g_bn"], res["g_ref"]) and torch.equal(res["sums_bn"], res["sums_ref"])
        dref = _norm_ref(q(z).reshape(B, -1), q(g).reshape(B, -1), f64(res["st"]))
        assert _rms(f64(res["dz16"]).reshape(B, -1), O.bf16_round(dref)) < 6e-4
        assert _rms(f64(res["g_bn"]), O.bf16_round(O.conv_fwd(f64(res["dz16"]), q(w), 2))) < 6e-4

    row(f"persistent-down-BWDNORM-{B}x{s_h}x{s_w}x{cb}x{cs}",
        ("lg_convT_s2_dgrad_bn", "lg_convT_s2_dgrad_bn_supported", "lg_instnorm_bwd_coef", "lg_instnorm_leaky_bwd_z16_p", "lg_convT_s2_dgrad_nf"),
        run, check, ("bn=conv_down3_kernel<NW=64,BWDNORM>", "ref=conv_down3_kernel<NW=64>"), sizing=[_stats_bytes(0, B, s_h, s_w, cs)])


bwdnorm_row(2, 8, 16, 32, 64)


# ------------------------------------------------------------------------------------------------------------------ weight gradients
def wgrad_rows(case, dtype, mirrors, route, accumulate, form="conv"):
    """conv: dw (+)= wgrad(big = x, small = dy); "convT": the operands swapped at the call.  mirrors: "none" fp32 operands only,
    "both" bf16 mirrors only (the all-taps kernels read nothing else), "with" fp32 operands and their mirrors."""
    B, Hm, Wm, cb, cs = case

    @functools.lru_cache(maxsize=None)
    def data():
        s = crc("wgrad", case)
        return arr(s, B, 2 * Hm, 2 * Wm, cb), arr(s + 1, B, Hm, Wm, cs), arr(s + 2, 5, 5, cb, cs)

    def run(ops, alloc):
        big, small, prior = data()
        tr = Trace(ops)
        b32 = alloc.inp("big", big) if mirrors != "both" else None
        s32 = alloc.inp("small", small) if mirrors != "both" else None
        b16 = alloc.inp("big16", bf(big)) if mirrors != "none" else None
        s16 = alloc.inp("small16", bf(small)) if mirrors != "none" else None
        dw = alloc.state("dw", prior) if accumulate else alloc.out("dw", (5, 5, cb, cs))
        if form == "conv":
            ops.conv2d_s2_wgrad(b32, s32, dw, accumulate, dtype, x16=b16, dy16=s16)
        else:
            ops.convT_s2_wgrad(s32, b32, dw, accumulate, dtype, x16=s16, dy16=b16)
        tr("wgrad")
        return dict(dw=dw, _route=tr)

    def check(res):
        big, small, prior = (a.astype(np.float64) for a in data())
        rounded = dtype == 1 and mirrors == "both"   # against the oracle on the rounded operands: fp32 accumulation only (3e-5)
        exp = O.conv2d_bwd(q(big) if rounded else big, np.zeros((5, 5, cb, cs)), q(small) if rounded else small, 2)[1]
        assert rel(res["dw"], exp + (prior if accumulate else 0.0)) < (3e-5 if rounded else TOL[dtype])

    row(f"wgrad-{form}-{'x'.join(map(str, case))}-{'bf16' if dtype else 'f32'}-mirrors-{mirrors}-{'acc' if accumulate else 'ovw'}",
        ("lg_conv2d_s2_wgrad_m16" if form == "conv" else "lg_convT_s2_wgrad_m16",), run, check, "wgrad=" + route,
        wgrad=(B, Hm, Wm, cb, cs, dtype))


for _acc in (False, True):
    wgrad_rows((3, 5, 6, 32, 64), 0, "none", "wgrad_kernel<f32,per-tap>", _acc)
    wgrad_rows((3, 5, 6, 32, 64), 1, "none", "wgrad_kernel<bf16,per-tap>", _acc)
    wgrad_rows((3, 5, 6, 32, 64), 1, "with", "wgrad_kernel<bf16,per-tap>", _acc)
    wgrad_rows((2, 8, 8, 32, 64), 0, "none", "wgrad_at32_kernel", _acc)
    wgrad_rows((2, 12, 16, 32, 192), 0, "none", "wgrad_at32_kernel", _acc)          # height a multiple of 4, not of 8
    wgrad_rows((2, 16, 16, 32, 64), 1, "both", "wgrad_at_kernel<16,8>", _acc)
    wgrad_rows((2, 4, 32, 32, 64), 1, "both", "wgrad_at_kernel<32,4>", _acc)
    wgrad_rows((2, 8, 8, 64, 128), 1, "both", "wgrad_at_kernel<8,8>", _acc)
    wgrad_rows((3, 8, 8, 64, 128), 1, "both", "wgrad_kernel<bf16,per-tap>", _acc)   # odd batch: back to the per-tap kernel
wgrad_rows((2, 8, 8, 32, 64), 0, "none", "wgrad_at32_kernel", False, form="convT")
wgrad_rows((2, 16, 16, 32, 64), 1, "both", "wgrad_at_kernel<16,8>", False, form="convT")


def n3_wgrad_row(case, dtype, accumulate):
    """3-channel all-taps weight gradient in conv1 form (stride 2, pad 1): image x3 [B,2H,2W,3] fp32, dz [B,H,W,C] (bf16 path: its
    mirror alone)"""
    B, H, W, C = case

    @functools.lru_cache(maxsize=None)
    def data():
        s = crc("n3wgrad", case)
        return arr(s, B, 2 * H, 2 * W, 3), arr(s + 1, B, H, W, C), arr(s + 2, 5, 5, 3, C)

    def run(ops, alloc):
        x3, dz, prior = data()
        tr = Trace(ops)
        dw = alloc.state("dw", prior) if accumulate else alloc.out("dw", (5, 5, 3, C))
        if dtype:
            ops.conv2d_s2_wgrad(alloc.inp("x3", x3), None, dw, accumulate, 1, dy16=alloc.inp("dz16", bf(dz)))
        else:
            ops.conv2d_s2_wgrad(alloc.inp("x3", x3), alloc.inp("dz", dz), dw, accumulate, 0)
        tr("wgrad")
        return dict(dw=dw, _route=tr)

    def check(res):
        x3, dz, prior = (a.astype(np.float64) for a in data())
        exp = O.conv2d_bwd(q(x3), np.zeros((5, 5, 3, C)), q(dz), 2)[1] if dtype else O.conv2d_bwd(x3, np.zeros((5, 5, 3, C)), dz, 2)[1]
        assert rel(res["dw"], exp + (prior if accumulate else 0.0)) < 3e-5   # test_n3_tap_product_kernels_from_bf16_mirror / exact f32

    row(f"wgrad-n3-conv1-{'x'.join(map(str, case))}-{'bf16' if dtype else 'f32'}-{'acc' if accumulate else 'ovw'}",
        ("lg_conv2d_s2_wgrad_m16",), run, check, "wgrad=n3_wgrad", wgrad=(B, H, W, 3, C, dtype))


for _acc in (False, True):
    n3_wgrad_row((2, 16, 16, 32), 0, _acc)
    n3_wgrad_row((2, 16, 16, 32), 1, _acc)


def bias_grad_row(case, src, accumulate):
    M, C = case

    @functools.lru_cache(maxsize=None)
    def data():
        return arr(crc("bias", case), M, C), arr(crc("bias", case) + 1, C)

    def run(ops, alloc):
        dy, prior = data()
        db = alloc.state("db", prior) if accumulate else alloc.out("db", (C,))
        if src == "bf16":
            ops.bias_grad(None, db, accumulate, dy16=alloc.inp("dy16", bf(dy)))
        else:
            ops.bias_grad(alloc.inp("dy", dy), db, accumulate)
        return dict(db=db)

    def check(res):
        dy, prior = data()
        exp = (q(dy) if src == "bf16" else dy.astype(np.float64)).sum(0) + (prior.astype(np.float64) if accumulate else 0.0)
        assert rel(res["db"], exp) < 3e-5   # test_bias_grad_shapes

    row(f"bias_grad-{M}x{C}-{src}-{'acc' if accumulate else 'ovw'}", ("lg_bias_grad_m16",), run, check,
        sizing=[("lg_bias_grad_workspace_bytes", (M, C))])


assert (70, 1028) in BIAS_CASES
for _src in ("f32", "bf16"):
    for _acc in (False, True):
        bias_grad_row((70, 1028), _src, _acc)   # C / 4 = 257: a second column pass for one quad


# ------------------------------------------------------------------------------------------------------------------ final layer
def final_rows(case, dtype, route):
    """tanh(Conv2DTranspose(3, 5, 1, same)) forward and backward (data, weight and bias gradients; overwrite, then accumulate on
    seeded values) through the fp32 operands: test_convT_s1_tanh_fwd_bwd"""
    B, H, W, cs = case

    @functools.lru_cache(maxsize=None)
    def data():
        s = crc("final", case)
        return (arr(s, B, H, W, cs), arr(s + 1, 5, 5, 3, cs, scale=0.05), arr(s + 2, 3, scale=0.1), arr(s + 3, B, H, W, 3),
                arr(s + 4, 5, 5, 3, cs), arr(s + 5, 3))

    def run(ops, alloc):
        x, w, b, dpre, pw, pb = data()
        tr = Trace(ops)
        xd, dp = alloc.inp("x", x), alloc.inp("dpre", dpre)
        pack = _pack(ops, alloc, w, 3, cs, dtype)
        y = ops.convT_s1_tanh_fwd(xd, pack, alloc.inp("bias", b), 3, dtype, out=alloc.out("y", (B, H, W, 3)))
        tr("fwd")
        dx, dw, db = alloc.out("dx", (B, H, W, cs)), alloc.out("dw", (5, 5, 3, cs)), alloc.out("db", (3,))
        ops.convT_s1_tanh_bwd(xd, dp, pack, cs, dtype, dx=dx, dw=dw, db=db)
        tr("bwd")
        dw2, db2 = alloc.state("dw2", pw), alloc.state("db2", pb)
        ops.convT_s1_tanh_bwd(xd, dp, pack, cs, dtype, dw=dw2, db=db2, accumulate=True)
        tr("bwd_acc")
        return dict(y=y, dx=dx, dw=dw, db=db, dw2=dw2, db2=db2, _route=tr)

    def check(res):
        x, w, b, dpre, pw, pb = (a.astype(np.float64) for a in data())
        assert rel(res["y"], np.tanh(O.conv2d_transpose(x, w, b, 1))) < TOL[dtype]
        dx_e, dw_e, db_e = O.conv2d_transpose_bwd(x, w, dpre, 1)
        assert rel(res["dx"], dx_e) < TOL[dtype]
        assert rel(res["dw"], dw_e) < 3e-5 and rel(res["db"], db_e) < 3e-5   # the patch weight gradient runs on the exact f32 MFMA
        assert rel(res["dw2"], pw + dw_e) < 3e-5 and rel(res["db2"], pb + db_e) < 3e-5

    row(f"final-{'x'.join(map(str, case))}-{'bf16' if dtype else 'f32'}", ("lg_conv_pack", "lg_convT_s1_tanh_fwd_m16", "lg_convT_s1_tanh_bwd_m16"),
        run, check, route, sizing=[("lg_convT_s1_bwd_workspace_bytes", (B, H, W, 3, cs, dtype))], wgrad=(B, H, W, 3, cs, dtype))


for _dt in (0, 1):
    final_rows((2, 6, 10, 32), _dt, "fwd=conv_igemm_kernel<S1T>;bwd=wgrad_kernel<PATCH>;bwd_acc=wgrad_kernel<PATCH>")
    final_rows((1, 4, 4, 64), _dt, "fwd=conv_halo_kernel<S1T>;bwd=wgrad_kernel<PATCH>;bwd_acc=wgrad_kernel<PATCH>")
    # the forward of this shape is the unnamed n3 kernel; the backward must end in the all-taps 3-channel weight gradient
    final_rows((2, 16, 16, 32), _dt, "fwd=;bwd=n3_wgrad_kernel<f32>;bwd_acc=n3_wgrad_kernel<f32>")   # HALO_CASES ("s1t", 2, 16, 16, 32, 3); the all-taps 3-channel weight gradient in final-layer form


def final_m16_row(case):
    """bf16 path of the final layer from the mirror alone (n3_pgemm.hip, n3_kernels.hip): forward, backward with the weight gradient
    from the mirror and the data gradient written as bf16 together with the norm-backward sums of the level below (_bwd_nf), consumed
    by instnorm_bwd: test_n3_tap_product_kernels_from_bf16_mirror, test_final_layer_fused_data_gradient"""
    B, H, W, C = case

    @functools.lru_cache(maxsize=None)
    def data():
        s = crc("final16", case)
        return (arr(s, B, H, W, C), arr(s + 1, 5, 5, 3, C, scale=0.05), arr(s + 2, 3, scale=0.1), arr(s + 3, B, H, W, 3),
                arr(s + 4, B, H, W, C, scale=1.7, shift=0.4))

    def run(ops, alloc):
        x, w, b, dpre, z = data()
        tr = Trace(ops)
        assert ops.n3_m16_supported(H, W, 3, C, 1)
        x16, dp = alloc.inp("x16", bf(x)), alloc.inp("dpre", dpre)
        pack = _pack(ops, alloc, w, 3, C, 1)
        y = ops.convT_s1_tanh_fwd(None, pack, alloc.inp("bias", b), 3, 1, out=alloc.out("y", (B, H, W, 3)), x16=x16)
        tr("fwd")
        gm, bt = _gb(alloc, 0.9, 0.15)
        z16 = alloc.inp("z16", bf(z))
        st = ops.instnorm_stats(alloc.inp("z", q(z).astype(np.float32)), gm, bt, 0, ALPHA, stats=alloc.out("st", (B, 8)))
        dx16, dw, db = alloc.out("dx16", (B, H, W, C), BF16), alloc.out("dw", (5, 5, 3, C)), alloc.out("db", (3,))
        _, parts = ops.convT_s1_tanh_bwd(None, dp, pack, C, 1, dx16=dx16, dw=dw, db=db, x16=x16, fuse=(z16, st, ALPHA))
        tr("bwd_nf")
        dgm, dbt = alloc.out("dgamma", (1,)), alloc.out("dbeta", (1,))
        dz16 = alloc.out("dz16", (B, H, W, C), BF16)
        ops.instnorm_bwd(z16, st, dx16, dgm, dbt, 0, 1, ALPHA, out16=dz16, want_f32=False, partials=parts)
        dx16b = alloc.out("dx16b", (B, H, W, C), BF16)
        ops.convT_s1_tanh_bwd(None, dp, pack, C, 1, dx16=dx16b)   # the plain _m16 entry point: data gradient alone
        tr("bwd")
        return dict(y=y, dx16=dx16, dw=dw, db=db, dz16=dz16, dgamma=dgm, dbeta=dbt, st=st, dx16b=dx16b,
                    nparts=None if parts is None else parts.nparts, _route=tr)

    def check(res):
        x, w, b, dpre, z = (a.astype(np.float64) for a in data())
        assert res["nparts"] is not None and torch.equal(res["dx16"], res["dx16b"])
        assert rel(res["y"], np.tanh(O.conv2d_transpose(q(x), q(w), b, 1))) < 3e-5
        dx_e, _, db_e = O.conv2d_transpose_bwd(q(x), w, dpre, 1)
        dw_e = O.conv2d_transpose_bwd(q(x), w, q(dpre), 1)[1]
        assert rel(res["dw"], dw_e) < 3e-5 and rel(res["db"], db_e) < 3e-5 and rel(res["dx16"].float(), dx_e) < TOL[1]
        _norm_chain_ok(torch.from_numpy(q(z)), res["st"], res["dx16"], res["dz16"], res["dgamma"], res["dbeta"])

    row(f"final-m16-{'x'.join(map(str, case))}", ("lg_convT_s1_tanh_fwd_m16", "lg_convT_s1_tanh_bwd_nf", "lg_convT_s1_tanh_bwd_m16", "lg_n3_m16_supported",
                                                    "lg_instnorm_leaky_bwd_z16_p", "lg_instnorm_leaky_stats_z16"), run, check,
        "fwd=s1t_fwd_rows_kernel<32>;bwd_nf=n3_wgrad16_kernel<1,16>;bwd=patch_p16_kernel<1,32>",
        sizing=[("lg_convT_s1_bwd_workspace_bytes", (B, H, W, 3, C, 1)), _stats_bytes(0, B, H, W, C)], wgrad=(B, H, W, 3, C, 1))


final_m16_row((2, 16, 16, 32))


def final_z16_row(case):
    """lg_convT_s1_tanh_fwd_z16 (n3_rows.hip): test_final_layer_normalises_while_staging"""
    B, H, W, C = case

    @functools.lru_cache(maxsize=None)
    def data():
        s = crc("finalz16", case)
        return arr(s, B, H, W, C, scale=1.3, shift=0.2), arr(s + 1, 5, 5, 3, C, scale=0.05), arr(s + 2, 3, scale=0.1)

    def run(ops, alloc):
        z, w, b = data()
        tr = Trace(ops)
        gm, bt = _gb(alloc, 1.1, -0.15)
        z16 = alloc.out("z16", (B, H, W, C), BF16)
        st = ops.instnorm_stats(alloc.inp("z", z), gm, bt, 0, ALPHA, stats=alloc.out("st", (B, 8)), x16_out=z16)
        h16 = alloc.out("h16", (B, H, W, C), BF16)
        ops.instnorm_apply(z16, st, None, 0, 1, ALPHA, out16=h16, want_f32=False)
        pack = _pack(ops, alloc, w, 3, C, 1)
        assert ops.convT_s1_tanh_fwd_z16_supported(H, W, 3, C, 1)
        y = ops.convT_s1_tanh_fwd_z16(z16, st, ALPHA, pack, alloc.inp("bias", b), 3, 1, out=alloc.out("y", (B, H, W, 3)))
        tr("z16")
        return dict(z16=z16, st=st, h16=h16, y=y, _route=tr)

    def check(res):
        _, w, b = data()
        assert rel(res["y"], np.tanh(O.conv2d_transpose(f64(res["h16"]), q(w), b.astype(np.float64), 1))) < 3e-5

    row(f"final-z16-{'x'.join(map(str, case))}", ("lg_convT_s1_tanh_fwd_z16", "lg_convT_s1_tanh_fwd_z16_supported", "lg_instnorm_leaky_stats_z16",
                                                    "lg_instnorm_leaky_apply_z16"), run, check, "z16=s1t_fwd_rows_kernel<32,NORM>",
        sizing=[("lg_instnorm_workspace_bytes", (B, H * W * C))])


final_z16_row((2, 16, 16, 32))
final_z16_row((1, 80, 48, 32))   # a ragged last row block


# ------------------------------------------------------------------------------------------------------------------ norm
def norm_row(shape, pre, post, skip):
    """stats, apply (fp32 result + bf16 mirror) and backward (dx + mirror, dgamma / dbeta accumulated onto seeded values) from fp32
    tensors: test_instnorm_stats_apply_bwd"""
    B = shape[0]
    L = int(np.prod(shape[1:]))
    gamma, beta = 1.3, -0.2

    @functools.lru_cache(maxsize=None)
    def data():
        s = crc("norm", shape)
        return arr(s, *shape, scale=1.5, shift=0.7), arr(s + 1, *shape), arr(s + 2, *shape)

    def run(ops, alloc):
        x, g, sk = data()
        gm, bt = _gb(alloc, gamma, beta)
        xd = alloc.inp("x", x)
        st = ops.instnorm_stats(xd, gm, bt, pre, ALPHA, stats=alloc.out("stats", (B, 8)))
        y16 = alloc.out("y16", shape, BF16)
        y = ops.instnorm_apply(xd, st, alloc.inp("skip", sk) if skip else None, pre, post, ALPHA, out=alloc.out("y", shape), out16=y16)
        dg, db = alloc.state("dgamma", np.array([0.25], np.float32)), alloc.state("dbeta", np.array([-0.5], np.float32))
        dx16 = alloc.out("dx16", shape, BF16)
        dx = ops.instnorm_bwd(xd, st, alloc.inp("g", g), dg, db, pre, post, ALPHA, accumulate=True, out=alloc.out("dx", shape), out16=dx16)
        return dict(stats=st, y=y, y16=y16, dx=dx, dx16=dx16, dgamma=dg, dbeta=db)

    def check(res):
        x, g, sk = (a.astype(np.float64) for a in data())
        xx = O.leaky(x, ALPHA) if pre else x
        y_e, cache = O.instnorm(xx, gamma, beta)
        out_e = (O.leaky(y_e, ALPHA) if post else y_e) + (sk if skip else 0.0)
        st = res["stats"]
        assert rel(st[:, 0], xx.reshape(B, -1).mean(1)) < 1e-5 and rel(st[:, 1], xx.reshape(B, -1).std(1)) < 1e-5
        assert rel(res["y"], out_e) < 1e-5 and torch.equal(res["y16"], res["y"].to(BF16))
        dxx_e, dg_e, db_e = O.instnorm_bwd(cache, gamma, O.leaky_bwd(y_e, g, ALPHA) if post else g)
        dx_e = O.leaky_bwd(x, dxx_e, ALPHA) if pre else dxx_e
        assert rel(res["dx"], dx_e) < 2e-5 and torch.equal(res["dx16"], res["dx"].to(BF16))
        assert abs(float(res["dgamma"]) - 0.25 - dg_e) < 2e-5 * max(1.0, abs(dg_e)) * 10
        assert abs(float(res["dbeta"]) + 0.5 - db_e) < 2e-5 * max(1.0, abs(db_e)) * 10

    row(f"norm-{'x'.join(map(str, shape))}-pre{pre}-post{post}-{'skip' if skip else 'noskip'}",
        ("lg_instnorm_leaky_stats_z16", "lg_instnorm_leaky_apply", "lg_instnorm_leaky_bwd_db"), run, check,
        sizing=[("lg_instnorm_workspace_bytes", (B, L)), ("lg_instnorm_bwd_db_workspace_bytes", (B, L, 0))])


for _shape in ((3, 4, 4, 32), (2, 8, 8, 96), (5, 24576)):
    norm_row(_shape, 0, 1, False)
    norm_row(_shape, 1, 0, True)


def norm_db_row(shape, g16, z16):
    """the backward that also writes the conv bias gradient db (column sums of dx), from an fp32 or bf16 z and an fp32 or bf16
    gradient: test_instnorm_bwd_fused_bias_column_sums"""
    B, C = shape[0], shape[-1]
    L = int(np.prod(shape[1:]))

    @functools.lru_cache(maxsize=None)
    def data():
        s = crc("normdb", shape)
        return arr(s, *shape, scale=1.3, shift=0.2), arr(s + 1, *shape)

    def run(ops, alloc):
        x, g = data()
        gm, bt = _gb(alloc)
        st = ops.instnorm_stats(alloc.inp("x", x), gm, bt, 0, ALPHA, stats=alloc.out("stats", (B, 8)))
        xd = alloc.inp("x16", bf(x)) if z16 else alloc.inp("x_", x)
        gd = alloc.inp("g16", bf(g)) if g16 else alloc.inp("g", g)
        db, d16 = alloc.out("db", (C,)), alloc.out("dx16", shape, BF16)
        dx = ops.instnorm_bwd(xd, st, gd, None, None, 0, 1, ALPHA, out=alloc.out("dx", shape), out16=d16, db=db)
        y16 = alloc.out("y16", shape, BF16)
        ops.instnorm_apply(xd, st, None, 0, 1, ALPHA, out16=y16, want_f32=False)
        return dict(stats=st, dx=dx, dx16=d16, db=db, y16=y16)

    def check(res):
        dx = res["dx"]
        assert torch.equal(res["dx16"], dx.to(BF16))
        _colsum_ok(res["db"], dx)
        x, g = data()
        xs, gs = (q(x) if z16 else x.astype(np.float64)), (q(g) if g16 else g.astype(np.float64))
        # fp32 dx against fp64 from the kernel's own operands and statistics records: the fp32 bound of test_instnorm_stats_apply_bwd
        assert rel(dx.reshape(B, -1), _norm_ref(xs.reshape(B, -1), gs.reshape(B, -1), f64(res["stats"]))) < 2e-5

    row(f"norm-db-{'x'.join(map(str, shape))}-{'z16' if z16 else 'z32'}-{'g16' if g16 else 'g32'}",
        ("lg_instnorm_leaky_bwd_z16", "lg_instnorm_leaky_apply_z16") if z16 else ("lg_instnorm_leaky_bwd_db", "lg_instnorm_leaky_apply"), run, check,
        sizing=[("lg_instnorm_bwd_db_workspace_bytes", (B, L, C))])


norm_db_row((2, 6, 10, 128), False, False)
norm_db_row((2, 6, 10, 128), True, False)
norm_db_row((2, 6, 10, 128), True, True)


def dropout_row(shape, path):
    """dropout_key, dropout_mask and the *_drop twins of apply and backward (rate 0.5): the dropped apply is the plain apply times
    keep * scale bit for bit, the mask is the restatement of tests/test_dropout_cpu.py (test_dropout_gpu.py)"""
    B = shape[0]
    L = int(np.prod(shape[1:]))
    C = shape[-1]
    rate, call, level, r0 = 0.5, 2, 3, 1
    seed, koff = 0x1234567, (5 << 40) + 77

    @functools.lru_cache(maxsize=None)
    def data():
        s = crc("drop", shape)
        return arr(s, *shape, scale=1.5, shift=0.7), arr(s + 1, *shape)

    def synthetic(ops, alloc, x16, gm, bt, nparts=4):
        zz = x16.double().reshape(B, nparts, -1)
        mean = zz.mean(2)
        rec = torch.stack([torch.full_like(mean, zz.shape[2]), mean, ((zz - mean[..., None]) ** 2).sum(2)], dim=-1).contiguous()
        return ops.Moments(alloc.inp("moments", rec.cpu().view(U8).reshape(-1)), nparts, gm, bt, B)

    def run(ops, alloc):
        x, g = data()
        gm, bt = _gb(alloc, 1.3, -0.2)
        key = ops.dropout_key(seed, koff, out=alloc.out("key", (2,), I64))
        keep = ops.dropout_mask(key, call, level, r0, B, L, rate)
        d = ops.Drop(key, call, level, r0, rate)
        st = ops.instnorm_stats(alloc.inp("x", q(x).astype(np.float32) if path != "f32" else x), gm, bt, 0, ALPHA, stats=alloc.out("stats", (B, 8)))
        xd = alloc.inp("x_", x) if path == "f32" else alloc.inp("x16", bf(x))
        y16, yd16 = alloc.out("y16", shape, BF16), alloc.out("yd16", shape, BF16)
        res = dict(key=key, keep=keep)
        if path == "p":
            m0, m1 = synthetic(ops, alloc, xd, gm, bt), synthetic(ops, alloc, xd, gm, bt)
            y = ops.instnorm_apply(xd, m0, None, 0, 1, ALPHA, out=alloc.out("y", shape), out16=y16)
            yd = ops.instnorm_apply(xd, m1, None, 0, 1, ALPHA, out=alloc.out("yd", shape), out16=yd16, drop=d)
            res.update(st0=m0.stats, st1=m1.stats)
            st = m1.stats
        else:
            y = ops.instnorm_apply(xd, st, None, 0, 1, ALPHA, out=alloc.out("y", shape), out16=y16)
            yd = ops.instnorm_apply(xd, st, None, 0, 1, ALPHA, out=alloc.out("yd", shape), out16=yd16, drop=d)
        dg, dbt = alloc.out("dgamma", (1,)), alloc.out("dbeta", (1,))
        db, dx16 = alloc.out("db", (C,)), alloc.out("dx16", shape, BF16)
        dx = ops.instnorm_bwd(xd, st, alloc.inp("g", g), dg, dbt, 0, 1, ALPHA, out=alloc.out("dx", shape), out16=dx16, db=db, drop=d)
        res.update(stats=st, y=y, yd=yd, y16=y16, yd16=yd16, dx=dx, dx16=dx16, dgamma=dg, dbeta=dbt, db=db)
        return res

    def check(res):
        x, g = data()
        assert res["key"].tolist() == [seed, koff]
        assert np.array_equal(res["keep"].cpu().numpy().astype(bool), keep_mask(seed, koff, call, level, r0, B, L, rate))
        m = torch.tensor(drop_mult(seed, koff, call, level, r0, B, L, rate), device="cuda").view(shape)
        want = res["y"] * m
        assert torch.equal(res["yd"], want) and torch.equal(res["yd16"], want.to(BF16)) and torch.equal(res["y16"], res["y"].to(BF16))
        if path == "p":
            assert torch.equal(res["st0"], res["st1"])
        xs = (x.astype(np.float64) if path == "f32" else q(x)).reshape(B, -1)
        gpre = (g.astype(np.float64) * f64(m)).reshape(B, -1)   # the masked gradient is what flows
        ss = f64(res["stats"])
        assert rel(res["dx"].reshape(B, -1), _norm_ref(xs, gpre, ss)) < 2e-5   # fp32 dx: test_dropped_backward_is_plain_backward_of_the_masked_gradient
        assert torch.equal(res["dx16"], res["dx"].to(BF16))
        _affine_ok(res["dgamma"], res["dbeta"], xs, gpre, ss)
        _colsum_ok(res["db"], res["dx"])

    covers = {"f32": ("lg_instnorm_leaky_apply_drop", "lg_instnorm_leaky_bwd_drop"),
              "bf16": ("lg_instnorm_leaky_apply_z16_drop", "lg_instnorm_leaky_bwd_z16_drop"),
              "p": ("lg_instnorm_leaky_apply_z16_p_drop", "lg_instnorm_leaky_apply_z16_p", "lg_instnorm_leaky_bwd_z16_drop")}[path]
    row(f"dropout-{'x'.join(map(str, shape))}-{path}", ("lg_dropout_key", "lg_dropout_mask") + covers, run, check,
        sizing=[("lg_instnorm_bwd_db_workspace_bytes", (B, L, C))])


for _path in ("f32", "bf16", "p"):
    dropout_row((3, 8, 8, 32), _path)


def gp_norm_row(B, H, C, bf16):
    """gp_norm_bwd and gp_norm_dd at the smallest LEVELS entry of tests/test_gp_gpu.py, against its fp64 formulas"""
    shape = (B, H, H, C)
    L = H * H * C

    @functools.lru_cache(maxsize=None)
    def data():
        s = crc("gpnorm", shape)
        return arr(s, *shape, scale=0.7, shift=0.1), arr(s + 1, *shape), arr(s + 2, *shape), arr(s + 3, *shape)

    def run(ops, alloc):
        z, g, u, add = data()
        gm, bt = _gb(alloc, 1.2, 0.1)
        st = ops.instnorm_stats(alloc.inp("z", z), gm, bt, 0, ALPHA, stats=alloc.out("stats", (B, 8)))
        zd = alloc.inp("z16", bf(z)) if bf16 else alloc.inp("z_", z)
        gd, ud, ad = alloc.inp("g", g), alloc.inp("u", u), alloc.inp("add", add)
        dgm, dbt, dgm2 = (alloc.state(n, np.zeros(1, np.float32)) for n in ("dgamma", "dbeta", "dgamma2"))
        dz16 = alloc.out("dz16", shape, BF16)
        dz = ops.gp_norm_bwd(zd, st, gm, gd, ALPHA, add=ad, dgamma=dgm, dbeta=dbt, out16=dz16)
        uh, uz2 = ops.gp_norm_dd(zd, st, gm, gd, ud, ALPHA, dgamma=dgm2)
        return dict(stats=st, dz=dz, dz16=dz16, uh=uh, uz2=uz2, dgamma=dgm, dbeta=dbt, dgamma2=dgm2)

    def check(res):
        from test_gp_gpu import _ref_level, _rel_rms
        z, g, u, add = (torch.from_numpy(a).cuda() for a in data())
        if bf16:
            z = z.to(BF16)
        gamma = torch.tensor([1.2], device="cuda")
        c, sigma, s, m = _ref_level(z, res["stats"], gamma, ALPHA)
        N, gmf = c.shape[1], 1.2
        gn, ud = g.double().reshape(B, -1) * m, u.double().reshape(B, -1)
        A, M = gn.mean(1, keepdim=True), (gn * c).mean(1, keepdim=True)
        dz_ref = (gmf / s) * (gn - A - c * M / (s * sigma)) + add.double().reshape(B, -1)
        U, P = ud.sum(1, keepdim=True), (ud * c).sum(1, keepdim=True)
        T1 = (ud * gn).sum(1, keepdim=True) - A * U
        uh_ref = m * (gmf / s) * (ud - U / N - c * (P / N) / (s * sigma))
        uz_ref = (-gmf * T1 * c / (N * s ** 2 * sigma) - gmf / (s ** 2 * sigma) * (P * (gn - A) / N + M * (ud - U / N))
                  + gmf * M * P * (2 / s + 1 / sigma) * c / (N * s ** 2 * sigma ** 2))
        for got, ref in ((res["dz"], dz_ref), (res["uh"], uh_ref), (res["uz2"], uz_ref)):
            assert _rel_rms(got.double().reshape(B, -1).cpu(), ref.cpu()) < 1e-5
        for got, exp, l2 in ((res["dgamma"], (gn * c / s).sum(), (gn * c / s).norm()), (res["dbeta"], gn.sum(), gn.norm()),
                             (res["dgamma2"], ((T1 - M * P / (s * sigma)) / s).sum(), ((ud * gn) / s).norm() + (ud * c * M / (s * s * sigma)).norm())):
            assert abs(float(got) - float(exp)) <= 1e-5 * abs(float(exp)) + 1e-6 * float(l2), (float(got), float(exp))
        assert torch.equal(res["dz16"], res["dz"].to(BF16))

    row(f"gp-norm-{B}x{H}x{C}-{'bf16' if bf16 else 'f32'}", ("lg_gp_norm_bwd", "lg_gp_norm_dd"), run, check,
        sizing=[("lg_gp_workspace_bytes", (B, L))])


gp_norm_row(3, 4, 32, False)
gp_norm_row(3, 4, 32, True)


def gp_small_row(B, H):
    """gp_draw_eps, gp_interp, gp_seed, gp_heads_seed, gp_heads_2nd at (3, 32): test_interp_seed_and_heads_kernels_against_fp64"""
    K, c = 8 * 8 * 384, 40
    L = H * H * 3
    seed, off = 0x51, (3 << 40) + 9

    @functools.lru_cache(maxsize=None)
    def data():
        r = np.random.default_rng(crc("gp", B, H))
        g = (r.standard_normal((B, H, H, 3)) * 0.02).astype(np.float32)
        g[0] = 0.0   # r = 0: the seed factor is 0, not NaN
        return dict(real=(r.random((B, H, H, 3)) * 2 - 1).astype(np.float32), fake=(r.random((B, H, H, 3)) * 2 - 1).astype(np.float32),
                    eps=r.random(B).astype(np.float32), g=g, p=(r.random((B, 1 + c)) * 0.9 + 0.05).astype(np.float32),
                    wpr=(r.standard_normal((K, 1)) * 0.01).astype(np.float32), x=r.standard_normal((B, K)).astype(np.float32),
                    u=r.standard_normal((B, K)).astype(np.float32))

    def run(ops, alloc):
        d = data()
        t = {k: alloc.inp(k, v) for k, v in d.items()}
        drawn = alloc.out("eps_drawn", (B,))   # the wrapper allocates its own output: the entry point with a guarded one
        ops._lib.check(ops._lib.load().lg_gp_draw_eps(drawn.data_ptr(), B, ops._i64(seed), ops._i64(off), torch.cuda.current_stream().cuda_stream),
                       "lg_gp_draw_eps")
        xh = ops.gp_interp(t["real"], t["fake"], t["eps"], out=alloc.out("xhat", (B, H, H, 3)))
        loss, gp_loss = alloc.state("loss", np.array([0.5], np.float32)), alloc.out("gp_loss", (1,))
        u0, r = ops.gp_seed(t["g"], 5.0, loss, gp_loss)
        gs = ops.gp_heads_seed(t["p"], t["wpr"])
        dw, db = alloc.state("dwpr", np.full((K, 1), 0.25, np.float32)), alloc.state("dbpr", np.array([-0.5], np.float32))
        tt, g2 = ops.gp_heads_2nd(t["p"], t["wpr"], t["x"], t["u"], dwpr=dw, dbpr=db)
        return dict(drawn=drawn, xhat=xh, loss=loss, gp_loss=gp_loss, u0=u0, r=r, gs=gs, t=tt, g2=g2, dwpr=dw, dbpr=db)

    def check(res):
        from test_gp_gpu import _rel_rms
        d = {k: torch.from_numpy(v).double() for k, v in data().items()}
        bits = I.philox_blocks((B + 3) // 4, seed, off).reshape(-1)[:B]
        assert np.array_equal(res["drawn"].cpu().numpy(), ((bits >> 8).astype(np.float64) / 2 ** 24).astype(np.float32))
        e = d["eps"].view(B, 1, 1, 1)
        assert (res["xhat"].double().cpu() - (e * d["real"] + (1 - e) * d["fake"])).abs().max() < 1e-6
        rd = d["g"].reshape(B, -1).norm(dim=1)
        term = 5.0 * ((rd - 1) ** 2).mean()
        assert (res["r"].double().cpu() - rd).abs().max() < 1e-6 * rd.max()
        assert abs(float(res["gp_loss"]) - float(term)) < 1e-6 * float(term) and abs(float(res["loss"]) - 0.5 - float(term)) < 1e-6 * float(term)
        k = (2 * 5.0 / B) * (rd - 1) / rd.clamp(min=1e-12)
        assert torch.isfinite(res["u0"]).all() and _rel_rms(res["u0"].double().cpu(), k.view(B, 1, 1, 1) * d["g"]) < 1e-6
        pd = d["p"][:, 0]
        sp, spp = pd * (1 - pd), pd * (1 - pd) * (1 - 2 * pd)
        assert _rel_rms(res["gs"].double().cpu(), sp[:, None] * d["wpr"].view(1, K)) < 1e-6
        td = spp * (d["u"] @ d["wpr"].view(K))
        assert _rel_rms(res["t"].double().cpu(), td) < 1e-6 and _rel_rms(res["g2"].double().cpu(), td[:, None] * d["wpr"].view(1, K)) < 1e-6
        assert _rel_rms(res["dwpr"].double().view(K).cpu(), 0.25 + (sp[:, None] * d["u"]).sum(0) + d["x"].T @ td) < 1e-6
        assert abs(float(res["dbpr"]) - (-0.5 + float(td.sum()))) < 1e-5 * float(td.abs().sum())

    row(f"gp-small-{B}x{H}", ("lg_gp_draw_eps", "lg_gp_interp", "lg_gp_seed", "lg_gp_heads_seed", "lg_gp_heads_2nd"), run, check,
        sizing=[("lg_gp_workspace_bytes", (B, L))])


gp_small_row(3, 32)


# ------------------------------------------------------------------------------------------------------------------ top of the network
def dense_row(case):
    B, K, N, fwd, wg = case

    @functools.lru_cache(maxsize=None)
    def data():
        s = crc("dense", case)
        return arr(s, B, K), arr(s + 1, K, N, scale=0.1), arr(s + 2, N), arr(s + 3, B, N), arr(s + 4, K, N), arr(s + 5, N)

    def run(ops, alloc):
        x, w, b, dy, dw0, db0 = data()
        tr = Trace(ops)
        xd, dyd = alloc.inp("x", x), alloc.inp("dy", dy)
        y = ops.dense_fwd(xd, alloc.inp("w", w), alloc.inp("bias", b), out=alloc.out("y", (B, N)))
        tr("fwd")
        dw, db = alloc.out("dw", (K, N)), alloc.out("db", (N,))
        ops.dense_wgrad(xd, dyd, dw, db, accumulate=False)
        tr("wgrad")
        dw2, db2 = alloc.state("dw2", dw0), alloc.state("db2", db0)
        ops.dense_wgrad(xd, dyd, dw2, db2, accumulate=True)
        tr("wgrad_acc")
        return dict(y=y, dw=dw, db=db, dw2=dw2, db2=db2, _route=tr)

    def check(res):
        x, w, b, dy, dw0, db0 = (a.astype(np.float64) for a in data())
        assert rel(res["y"], x @ w + b) < 1e-5 and rel(res["dw"], x.T @ dy) < 1e-5 and rel(res["db"], dy.sum(0)) < 1e-5
        assert rel(res["dw2"], dw0 + x.T @ dy) < 1e-5 and rel(res["db2"], db0 + dy.sum(0)) < 1e-5

    row(f"dense-{B}x{K}x{N}", ("lg_dense_fwd", "lg_dense_wgrad"), run, check,
        (f"fwd={DENSE_FWD[fwd]};", f"wgrad={dense_wgrad_name(wg)};", f"wgrad_acc={dense_wgrad_name(wg)}"))


def _smallest(cases, key):
    """the smallest case (by the product of its three sizes) of every distinct value of key(case)"""
    best = {}
    for c in cases:
        k = key(c)
        if k not in best or np.prod(c[:3]) < np.prod(best[k][:3]):
            best[k] = c
    return sorted(set(best.values()))


for _c in sorted(set(_smallest(DENSE_CASES, lambda c: c[3]) + _smallest(DENSE_CASES, lambda c: c[4]))):
    dense_row(_c)


def dense_dgrad_row(case):
    B, K, N = case

    @functools.lru_cache(maxsize=None)
    def data():
        return arr(crc("ddgrad", case), B, N), arr(crc("ddgrad", case) + 1, K, N, scale=0.1)

    def run(ops, alloc):
        dy, w = data()
        tr = Trace(ops)
        dx = ops.dense_dgrad(alloc.inp("dy", dy), alloc.inp("w", w), out=alloc.out("dx", (B, K)))
        tr("dgrad")
        return dict(dx=dx, _route=tr)

    def check(res):
        dy, w = (a.astype(np.float64) for a in data())
        assert rel(res["dx"], dy @ w.T) < 3e-5

    row(f"dense-dgrad-{B}x{K}x{N}", ("lg_dense_dgrad",), run, check, "dgrad=dense_dgrad_kernel")


dense_dgrad_row(min(DGRAD_CASES, key=lambda c: np.prod(c)))


def heads_row(case):
    B, K, c, fwd, wg, dg = case

    @functools.lru_cache(maxsize=None)
    def data():
        s = crc("heads", case)
        return dict(x=arr(s, B, K), wpr=arr(s + 1, K, 1, scale=0.02), wc=arr(s + 2, K, c, scale=0.02), bpr=arr(s + 3, 1), bc=arr(s + 4, c),
                    dz=arr(s + 5, B, 1 + c), p0=arr(s + 6, K, 1), p1=arr(s + 7, 1), p2=arr(s + 8, K, c), p3=arr(s + 9, c))

    def run(ops, alloc):
        d = data()
        tr = Trace(ops)
        t = {k: alloc.inp(k, d[k]) for k in ("x", "wpr", "wc", "bpr", "bc", "dz")}
        p = ops.heads_fwd(t["x"], t["wpr"], t["bpr"], t["wc"], t["bc"], out=alloc.out("p", (B, 1 + c)))
        tr("fwd")
        dx = ops.heads_dgrad(t["dz"], t["wpr"], t["wc"], out=alloc.out("dx", (B, K)))
        tr("dgrad")
        outs = (alloc.out("dwpr", (K, 1)), alloc.out("dbpr", (1,)), alloc.out("dwc", (K, c)), alloc.out("dbc", (c,)))
        ops.heads_wgrad(t["x"], t["dz"], *outs, accumulate=False)
        tr("wgrad")
        acc = tuple(alloc.state(f"acc{i}", d[f"p{i}"]) for i in range(4))
        ops.heads_wgrad(t["x"], t["dz"], *acc, accumulate=True)
        tr("wgrad_acc")
        return dict(p=p, dx=dx, dwpr=outs[0], dbpr=outs[1], dwc=outs[2], dbc=outs[3], a0=acc[0], a1=acc[1], a2=acc[2], a3=acc[3], _route=tr)

    def check(res):
        d = {k: v.astype(np.float64) for k, v in data().items()}
        x, dz = d["x"], d["dz"]
        assert rel(res["p"], np.concatenate([O.sigmoid(x @ d["wpr"] + d["bpr"]), O.sigmoid(x @ d["wc"] + d["bc"])], 1)) < 1e-5
        assert rel(res["dx"], dz[:, :1] @ d["wpr"].T + dz[:, 1:] @ d["wc"].T) < 1e-5
        e = (x.T @ dz[:, :1], dz[:, 0].sum(0, keepdims=True), x.T @ dz[:, 1:], dz[:, 1:].sum(0))
        for outs, prior in (((res["dwpr"], res["dbpr"], res["dwc"], res["dbc"]), (0.0, 0.0, 0.0, 0.0)),
                            ((res["a0"], res["a1"], res["a2"], res["a3"]), (d["p0"], d["p1"], d["p2"], d["p3"]))):
            assert rel(outs[0], prior[0] + e[0]) < 1e-5 and rel(outs[2], prior[2] + e[2]) < 1e-5
            assert rel(torch.cat([outs[1], outs[3]]), np.concatenate([prior[1] + e[1], prior[3] + e[3]])) < 1e-5

    row(f"heads-{B}x{K}x{c}", ("lg_heads_fwd", "lg_heads_dgrad", "lg_heads_wgrad"), run, check,
        (f"fwd={HEADS_FWD[fwd]};", f"dgrad={HEADS_DGRAD[dg]};", f"wgrad={HEADS_WGRAD[wg]};", f"wgrad_acc={HEADS_WGRAD[wg]}"),
        sizing=[("lg_heads_fwd_workspace_bytes", (B, K, c))])


for _c in sorted(set(_smallest(HEADS_CASES, lambda c: c[3]) + _smallest(HEADS_CASES, lambda c: c[4]) + _smallest(HEADS_CASES, lambda c: c[5]))):
    heads_row(_c)


def step_inputs_row(B, ka, kc):
    @functools.lru_cache(maxsize=None)
    def data():
        s = crc("stepin", B, ka, kc)
        return arr(s, B, ka), arr(s + 1, B, kc), arr(s + 2, B, kc)

    def run(ops, alloc):
        a, c, c1 = data()
        tr = Trace(ops)
        cd = alloc.inp("c", c)
        out = ops.concat_cols(alloc.inp("a", a), cd, out=alloc.out("cat", (B, ka + kc)))
        tr("concat")
        t, u = ops.adj_conditions(cd, alloc.inp("c1", c1))
        tr("adj")
        return dict(cat=out, t=t, u=u, _route=tr)

    def check(res):
        a, c, c1 = data()
        assert np.array_equal(res["cat"].cpu().numpy(), np.concatenate([a, c], -1))
        t_ref = np.concatenate([c, c1], 0)
        assert np.array_equal(res["t"].cpu().numpy(), t_ref)
        assert np.array_equal(res["u"].cpu().numpy(), (t_ref + np.float32(1.0)) * np.float32(0.5))

    row(f"step-inputs-{B}x{ka}x{kc}", ("lg_concat_cols", "lg_adj_conditions"), run, check, ("concat=concat_cols_kernel", "adj=adj_conditions_kernel"))


step_inputs_row(7, 93, 40)


# ------------------------------------------------------------------------------------------------------------------ tail
def l1_row(n):
    """bit-exact restatement of test_l1_tanh_loss_bit_exact (multiples of 2^-6: every partial sum is exact)"""
    lam = 0.02

    @functools.lru_cache(maxsize=None)
    def data():
        r = np.random.default_rng(crc("l1", n))
        return ((r.integers(-64, 65, n) / 64.0).astype(np.float32), (r.integers(-64, 65, n) / 64.0).astype(np.float32),
                (r.integers(-128, 129, n) / 1024.0).astype(np.float32))

    def run(ops, alloc):
        t, img, gin = data()
        loss, dpre = alloc.state("loss", np.array([0.375], np.float32)), alloc.out("dpre", (n,))
        ops.l1_tanh_loss(alloc.inp("t", t), alloc.inp("img", img), alloc.inp("g_in", gin), dpre, loss, lam, True)
        loss2 = alloc.out("loss2", (1,))
        ops.l1_tanh_loss(alloc.inp("t2", t), alloc.inp("img2", img), None, None, loss2, lam, False)   # loss only, overwritten
        return dict(loss=loss, dpre=dpre, loss2=loss2)

    def check(res):
        t, img, gin = data()
        gscale = np.float32(lam) / np.float32(n)
        d = t - img
        dpre_e = (gin - gscale * np.sign(d).astype(np.float32)) * (np.float32(1.0) - img * img)
        term = np.float32(np.float64(np.abs(d.astype(np.float64)).sum()) * np.float64(gscale))
        assert np.array_equal(res["dpre"].cpu().numpy(), dpre_e)
        assert res["loss"].cpu().numpy()[0] == np.float32(0.375) + term and res["loss2"].cpu().numpy()[0] == term

    row(f"l1_tanh_loss-{n}", ("lg_l1_tanh_loss_fwd_bwd",), run, check, sizing=[("lg_l1_workspace_bytes", ())])


l1_row(1028)


def bce_row(B, c):
    @functools.lru_cache(maxsize=None)
    def data():
        r = np.random.default_rng(crc("bce", B, c))
        p = r.uniform(0.02, 0.98, (B, 1 + c)).astype(np.float32)
        p[B - 1, c] = 1.0
        if B > 1:
            p[0, 0], p[1, 2], p[B - 1, 0], p[B // 2, c] = 0.0, 1.0, 1.0, 0.0
        return p, O.soft(2.0 * r.integers(0, 2, (B, c)) - 1.0).astype(np.float32)

    def run(ops, alloc):
        p, t_c = data()
        pd = alloc.inp("p", p)
        loss, dz = alloc.out("loss", (1,)), alloc.out("dz", (B, 1 + c))
        ops.bce_heads_loss(pd, alloc.inp("t_c", t_c), O.soft(1.0), 1.0, 2.0, loss, dz, False)
        loss2, dz2 = alloc.state("loss2", np.array([3.0], np.float32)), alloc.out("dz2", (B, 1 + c))
        ops.bce_heads_loss(pd, None, O.soft(0.0), 1.0, 0.0, loss2, dz2, True)
        return dict(loss=loss, dz=dz, loss2=loss2, dz2=dz2)

    def check(res):
        p, t_c = (a.astype(np.float64) for a in data())
        exp = O.bce_mean(O.soft(1.0), p[:, :1]) + 2.0 * O.bce_mean(t_c, p[:, 1:])
        dp = np.concatenate([O.bce_mean_bwd(O.soft(1.0), p[:, :1]), 2.0 * O.bce_mean_bwd(t_c, p[:, 1:])], 1)
        assert abs(res["loss"].item() - exp) < 2e-6 * abs(exp) + 1e-6 and rel(res["dz"], dp * p * (1 - p)) < 1e-5
        sat = (p == 0.0) | (p == 1.0)
        assert float(np.abs(f64(res["dz"])[sat]).max()) == 0.0
        exp2 = 3.0 + O.bce_mean(O.soft(0.0), p[:, :1])
        assert abs(res["loss2"].item() - exp2) < 2e-6 * abs(exp2) + 1e-6 and float(res["dz2"][:, 1:].abs().max()) == 0.0
        assert rel(res["dz2"][:, :1], O.bce_mean_bwd(O.soft(0.0), p[:, :1]) * p[:, :1] * (1 - p[:, :1])) < 1e-5

    row(f"bce_heads_loss-{B}x{c}", ("lg_bce_heads_loss_fwd_bwd",), run, check)


bce_row(1, 1)
bce_row(512, 40)


def adam_row(n):
    """one clipped Adam step from zero moments, then the state advance: test_clip_adam_sizes"""
    lr, b1, b2, clip, gscale = 5e-5, 0.5, 0.9, 0.5, 0.5

    @functools.lru_cache(maxsize=None)
    def data():
        return arr(crc("adam", n), n), arr(crc("adam", n) + 1, n)

    def run(ops, alloc):
        w0, g = data()
        w, m, v = alloc.state("w", w0), alloc.state("m", np.zeros(n, np.float32)), alloc.state("v", np.zeros(n, np.float32))
        state = alloc.state("state", np.array([b1, b2], np.float32))
        ops.clip_adam_update(w, alloc.inp("g", g), m, v, state, lr, b1, b2, 1e-8, clip, gscale=gscale)
        ops.adam_advance(state, b1, b2)
        return dict(w=w, m=m, v=v, state=state)

    def check(res):
        w0, g = (a.astype(np.float64) for a in data())
        st = O.AdamState(lr, b1, b2, 1)
        ws = [w0.copy()]
        st.apply(ws, [0], [np.clip(gscale * g, -clip, clip)])
        assert float(np.abs(f64(res["w"]) - ws[0]).max()) < 1e-6 and rel(res["m"], st.m[0]) < 1e-6 and rel(res["v"], st.v[0]) < 1e-6
        assert abs(res["state"][0].item() - b1 ** 2) < 1e-7 and abs(res["state"][1].item() - b2 ** 2) < 1e-7

    row(f"clip_adam-{n}", ("lg_clip_adam_update", "lg_adam_advance"), run, check)


adam_row(257)


def ema_adam_row(n, lo, hi, k):
    """clip + Adam on the inner range [lo, hi) with the weight average over everything, then the counter advance:
    test_kernel_against_the_restatement (g, m, v outside the range are NaN: whatever is read there poisons the result)"""
    sc = (ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["clip"], ADAM["gscale"])

    @functools.lru_cache(maxsize=None)
    def data():
        r = np.random.default_rng(crc("ema", n))
        w, g, m, e = (r.standard_normal(n).astype(np.float32) for _ in range(4))
        v = (r.random(n) * 0.1).astype(np.float32)
        g, m = 2.0 * g, 0.1 * m
        for t in (g, m, v):
            t[:lo], t[hi:] = np.nan, np.nan
        return w, g.astype(np.float32), m.astype(np.float32), v, e

    def run(ops, alloc):
        w0, g0, m0, v0, e0 = data()
        w, m, v, ema = alloc.state("w", w0), alloc.state("m", m0), alloc.state("v", v0), alloc.state("ema", e0)
        state = alloc.inp("adam_state", np.array([0.5 ** 3, 0.9 ** 3], np.float32))
        counter = alloc.state("counter", torch.tensor([k], dtype=I32))
        ops.clip_adam_ema_update(w, alloc.inp("g", g0), m, v, ema, lo, hi, state, counter, *sc, DECAY)
        wr, mr, vr = alloc.state("w_ref", w0[lo:hi]), alloc.state("m_ref", m0[lo:hi]), alloc.state("v_ref", v0[lo:hi])
        ops.clip_adam_update(wr, alloc.inp("g_ref", g0[lo:hi]), mr, vr, state, *sc)
        ops.ema_advance(counter)
        return dict(w=w, m=m, v=v, ema=ema, counter=counter, wr=wr, mr=mr, vr=vr)

    def check(res):
        w0, g0, m0, v0, e0 = data()
        w, m, v = res["w"], res["m"], res["v"]
        assert int(res["counter"]) == k + 1
        assert torch.equal(w[lo:hi], res["wr"]) and torch.equal(m[lo:hi], res["mr"]) and torch.equal(v[lo:hi], res["vr"])
        out = np.ones(n, bool)
        out[lo:hi] = False
        assert np.array_equal(w.cpu().numpy()[out], w0[out]) and np.isnan(m.cpu().numpy()[out]).all() and np.isnan(v.cpu().numpy()[out]).all()
        ref = ema_update(e0.astype(np.float64), f64(w), DECAY, k)
        err = np.abs(f64(res["ema"]) - ref)
        assert (err <= BOUND * np.maximum(np.abs(e0.astype(np.float64)), np.abs(f64(w)))).all()

    row(f"clip_adam_ema-{n}-{lo}-{hi}", ("lg_clip_adam_ema_update", "lg_clip_adam_update", "lg_ema_advance"), run, check)


ema_adam_row(1028, 4, 1024, 5)


def swap_axpby_row(n_swap, n):
    """swap_f32 moves bits (NaN and -inf included); axpby is numpy float32 a * x + b * y (test_swap, test_axpby_bit_exact).  lg_swap_f32
    takes multiples of 4 only: 1028 floats are 257 vectors, the first size past one block, as 257 elements are for axpby."""
    a_, b_ = np.float32(0.3), np.float32(-1.7)

    @functools.lru_cache(maxsize=None)
    def data():
        s = crc("swap", n)
        a0, b0 = arr(s, n_swap), arr(s + 1, n_swap)
        a0[0], b0[n_swap - 1] = np.nan, -np.inf
        return a0, b0, arr(s + 2, n), arr(s + 3, n)

    def run(ops, alloc):
        a0, b0, x, y = data()
        a, b = alloc.state("a", a0), alloc.state("b", b0)
        ops.swap_f32(a, b)
        xd, yd = alloc.inp("x", x), alloc.state("y", y)
        lib = ops._lib.load()
        ops._lib.check(lib.lg_axpby(yd.data_ptr(), xd.data_ptr(), float(a_), float(b_), n, torch.cuda.current_stream().cuda_stream), "lg_axpby")
        return dict(a=a, b=b, y=yd)

    def check(res):
        a0, b0, x, y = data()
        assert np.array_equal(res["a"].cpu().numpy().view(np.uint32), b0.view(np.uint32))
        assert np.array_equal(res["b"].cpu().numpy().view(np.uint32), a0.view(np.uint32))
        assert np.array_equal(res["y"].cpu().numpy(), a_ * x + b_ * y)

    row(f"swap-{n_swap}-axpby-{n}", ("lg_swap_f32", "lg_axpby"), run, check)


swap_axpby_row(1028, 257)


# ------------------------------------------------------------------------------------------------------------------ inputs
def rng_row(nblocks, n):
    seed, off = 0x0123456789ABCDEF, (7 << 40) + 5

    def run(ops, alloc):
        # the wrappers allocate their own outputs and take no tensor: the entry points are called with guarded outputs
        lib, chk, st_ = ops._lib.load(), ops._lib.check, torch.cuda.current_stream().cuda_stream
        bits, z = alloc.out("bits", (nblocks * 4,), I32), alloc.out("z", (n,))
        chk(lib.lg_philox4x32(bits.data_ptr(), nblocks, ops._i64(seed), ops._i64(off), st_), "lg_philox4x32")
        chk(lib.lg_randn(z.data_ptr(), n, 0.5, 2.0, ops._i64(seed), ops._i64(off), st_), "lg_randn")
        return dict(bits=bits, z=z, bits_w=ops.philox4x32(nblocks, seed, off), z_w=ops.randn((n,), seed, off, mean=0.5, std=2.0))

    def check(res):
        assert np.array_equal(res["bits"].cpu().numpy().view(np.uint32).reshape(nblocks, 4), I.philox_blocks(nblocks, seed, off))
        exp = 0.5 + 2.0 * I.normals((n + 3) // 4, seed, off).reshape(-1)[:n]
        assert np.abs(res["z"].cpu().numpy() - exp).max() < 2e-5
        assert torch.equal(res["bits"], res["bits_w"]) and torch.equal(res["z"], res["z_w"])   # the wrappers give the same bits

    row(f"philox-{nblocks}-randn-{n}", ("lg_philox4x32", "lg_randn"), run, check)


rng_row(300, 1001)


def augment_row(B, H, W):
    """augment with the caller's draws and augment_drawn with the device's: test_device_augmentation_matches_the_oracle,
    test_device_side_draws_match_the_oracle"""
    db, cf, dh = 0.013, 0.81, -0.021
    seed, off = 99, 3 << 38
    dseed, doff, noff = (5 << 20) ^ 1, (9 << 40) + (1 << 39), (9 << 40) + (1 << 38)

    @functools.lru_cache(maxsize=None)
    def data():
        r = np.random.default_rng(crc("aug", B, H, W))
        img = r.uniform(-1, 1, (B, H, W, 3)).astype(np.float32)
        img[0, 0, 0] = 0.25
        return img, r.random(B) < 0.5

    def run(ops, alloc):
        img, flip = data()
        x, f = alloc.inp("img", img), alloc.inp("flip", flip.astype(np.uint8))
        out = ops.augment(x, f, db, cf, dh, 0.0, 1, 0, out=alloc.out("out", img.shape))
        outn = ops.augment(x, f, db, cf, dh, 0.02, seed, off, out=alloc.out("outn", img.shape))
        drawn = ops.augment_drawn(x, 0.02, 0.75, 1.003, 0.03, 0.02, dseed, doff, noff, out=alloc.out("drawn", img.shape))
        return dict(out=out, outn=outn, drawn=drawn)

    def check(res):
        img, flip = data()
        exp = I.augment(img.astype(np.float64), flip, db, cf, dh)
        assert np.abs(res["out"].cpu().numpy() - exp).max() < 3e-6
        nz = I.normals(B * H * W, seed, off)[:, :3].reshape(B, H, W, 3)
        assert np.abs(res["outn"].cpu().numpy() - (exp + 0.02 * nz)).max() < 5e-6
        ddb, dcf, ddh, dflip = I.step_draws(B, dseed, doff)
        nz = I.normals(B * H * W, dseed, noff)[:, :3].reshape(B, H, W, 3)
        assert np.abs(res["drawn"].cpu().numpy() - (I.augment(img.astype(np.float64), dflip, ddb, dcf, ddh) + 0.02 * nz)).max() < 8e-6

    row(f"augment-{B}x{H}x{W}", ("lg_augment", "lg_augment_drawn"), run, check,
        sizing=[("lg_augment_workspace_bytes", (B,)), ("lg_augment_drawn_workspace_bytes", (B,))])


augment_row(3, 8, 12)


def u8_row(N, B, H, W, A, cols):
    """the packed uint8 input side, bit for bit the host expressions: tests/test_packed_input_gpu.py"""
    seed, doff, noff = (3 << 20) ^ 1, (7 << 40) + (1 << 39), (7 << 40) + (1 << 38)

    @functools.lru_cache(maxsize=None)
    def data():
        g = torch.Generator().manual_seed(crc("u8", N, B, H, W) % (1 << 31))
        src = torch.randint(0, 256, (N, H, W, 3), dtype=U8, generator=g)
        src.view(-1)[:256] = torch.arange(256, dtype=U8)
        idx = torch.randint(0, N, (B,), generator=g).to(I64)
        idx[B // 2] = idx[0]
        attr = torch.randint(-1, 2, (N, A), generator=g).float()
        attr[0, 0] = 0.3
        return src, idx, attr

    def run(ops, alloc):
        src, idx, attr = data()
        s, i = alloc.inp("src", src), alloc.inp("idx", idx)
        resc = ops.rescale_u8(s, i, out=alloc.out("rescaled", (B, H, W, 3)))
        lab = ops.soft_labels(alloc.inp("attr", attr), i, alloc.inp("cols", torch.tensor(cols, dtype=I32)), out=alloc.out("labels", (B, len(cols))))
        ref = ops.augment_drawn(resc, 0.02, 0.75, 1.003, 0.03, 0.02, seed, doff, noff, out=alloc.out("ref", (B, H, W, 3)))
        aug, resc2 = ops.augment_drawn_u8(s, i, 0.02, 0.75, 1.003, 0.03, 0.02, seed, doff, noff, out=alloc.out("aug", (B, H, W, 3)),
                                          out_rescaled=alloc.out("rescaled2", (B, H, W, 3)))
        return dict(rescaled=resc, labels=lab, ref=ref, aug=aug, rescaled2=resc2)

    def check(res):
        from littlegan_amd.utils import data_rescale, soft
        src, idx, attr = data()
        assert torch.equal(res["rescaled"].cpu(), data_rescale(src[idx].float())) and torch.equal(res["rescaled2"], res["rescaled"])
        assert torch.equal(res["labels"].cpu(), soft(attr[idx][:, cols])) and torch.equal(res["aug"], res["ref"])

    row(f"u8-inputs-{B}x{H}x{W}", ("lg_rescale_u8", "lg_soft_labels", "lg_augment_drawn_u8", "lg_augment_drawn"), run, check,
        sizing=[("lg_augment_drawn_u8_workspace_bytes", (B,)), ("lg_augment_drawn_workspace_bytes", (B,))])


u8_row(5, 3, 8, 12, 4, [3, 3, 0])


def diffaug_row(B, S):
    """diffaug_draw against its restatement bit for bit; T and its adjoint under the first B extreme records against the definition:
    tests/test_diffaug_gpu.py"""
    seed, koff = 0x7654321, (9 << 40) + 3

    @functools.lru_cache(maxsize=None)
    def data():
        r = np.random.default_rng(crc("diffaug", B, S))
        ext = extreme_records(S)
        return (r.uniform(-1, 1, (B, S, S, 3)).astype(np.float32), r.uniform(-1, 1, (B, S, S, 3)).astype(np.float32),
                np.asarray(ext[np.arange(B) % len(ext)], np.float32))

    def run(ops, alloc):
        x, g, recs = data()
        key = alloc.inp("key", torch.tensor([seed, koff], dtype=I64))
        drawn = ops.diffaug_draw(key, 1, 2, B, S, "color,translation,cutout", out=alloc.out("params", (B, 8)))
        p = alloc.inp("records", recs)
        out = ops.diffaug_fwd(alloc.inp("x", x), p, out=alloc.out("out", x.shape))
        gx = ops.diffaug_bwd(alloc.inp("g", g), p, out=alloc.out("gx", x.shape))
        out2 = ops.diffaug_fwd(alloc.inp("x2", x), drawn, out=alloc.out("out2", x.shape))
        return dict(drawn=drawn, out=out, gx=gx, out2=out2)

    def check(res):
        x, g, recs = data()
        want = draw_params(seed, koff, 1, 2, B, S, "color,translation,cutout")
        assert np.array_equal(res["drawn"].cpu().numpy().view(np.uint32), want.view(np.uint32))
        for got, ref, rr, scale in ((res["out"], diffaug_np(x, recs), recs, 1.0), (res["out2"], diffaug_np(x, want), want, 1.0),
                                    (res["gx"], diffaug_adjoint_np(g, recs), recs, np.abs(g).reshape(B, -1).max(axis=1))):
            err = np.abs(f64(got) - ref).reshape(B, -1).max(axis=1)
            assert (err <= 5e-6 * coef_sum(rr) * scale).all(), (err, coef_sum(rr))

    row(f"diffaug-{B}x{S}", ("lg_diffaug_draw", "lg_diffaug_fwd", "lg_diffaug_bwd"), run, check,
        sizing=[("lg_diffaug_workspace_bytes", (B, S))])


diffaug_row(*min(DIFFAUG_SHAPES, key=lambda s: s[0] * s[1] * s[1]))


# ------------------------------------------------------------------------------------------------------------------ metrics
def fid_row(N, D):
    """fid_stats, and fid_accum in two batches + fid_finalize, against numpy (check_stats of tests/test_fid_stream.py) and each other:
    test_accum_finalize_match_numpy_and_fid_stats"""
    @functools.lru_cache(maxsize=None)
    def data():
        return (torch.randn(N, D, generator=torch.Generator().manual_seed(N)) * 3.0 + 1.5).numpy()

    def run(ops, alloc):
        a = data()
        mu, sigma = ops.fid_stats(alloc.inp("act", a))
        shift = alloc.inp("shift", 1.4 + np.arange(D) * 1e-3)
        sm, gram = alloc.state("sum", np.zeros(D)), alloc.state("gram", np.zeros(ops.fid_gram_elems(D)))
        h = N // 2 + 1
        ops.fid_accum(alloc.inp("act_a", a[:h]), sm, gram, shift)
        ops.fid_accum(alloc.inp("act_b", a[h:]), sm, gram, shift)
        mu2, sigma2 = ops.fid_finalize(sm, gram, N, shift)
        return dict(mu=mu, sigma=sigma, sum=sm, gram=gram, mu2=mu2, sigma2=sigma2)

    def check(res):
        an = data().astype(np.float64)
        check_stats(res["mu"].cpu().numpy(), res["sigma"].cpu().numpy(), an)
        check_stats(res["mu2"].cpu().numpy(), res["sigma2"].cpu().numpy(), an)
        assert torch.equal(res["sigma2"], res["sigma2"].t()) and (res["mu2"] - res["mu"]).abs().max().item() < 1e-12
        assert (res["sigma2"] - res["sigma"]).abs().max().item() < 1e-10 * max(1.0, res["sigma"].abs().max().item())

    row(f"fid-stats-{N}x{D}", ("lg_fid_stats", "lg_fid_accum", "lg_fid_finalize"), run, check,
        sizing=[("lg_fid_stats_workspace_bytes", (N, D))])


fid_row(33, 70)


def fid_gemm_row(D):
    """test_fp64_gemm_matches_torch: asymmetric operands, the alpha / beta epilogue"""
    alpha, beta = -0.5, 1.5

    @functools.lru_cache(maxsize=None)
    def data():
        g = torch.Generator().manual_seed(D)
        a = torch.randn(D, D, generator=g, dtype=F64) + torch.arange(D, dtype=F64)[:, None] * 0.01
        b = torch.randn(D, D, generator=g, dtype=F64) - torch.arange(D, dtype=F64)[None, :] * 0.02
        return a, b

    def run(ops, alloc):
        a, b = data()
        ad, bd, c = alloc.inp("a", a), alloc.inp("b", b), alloc.out("c", (D, D), F64)   # the wrapper allocates c itself
        ab = (ctypes.c_double * 2)(alpha, beta)
        ops._lib.check(ops._lib.load().lg_fid_gemm(ad.data_ptr(), bd.data_ptr(), c.data_ptr(), D, ctypes.addressof(ab),
                                                   torch.cuda.current_stream().cuda_stream), "lg_fid_gemm")
        return dict(c=c, c_w=ops.fid_gemm(ad, bd, alpha, beta))

    def check(res):
        a, b = data()
        ref = alpha * torch.matmul(a, b) + beta * torch.eye(D, dtype=F64)
        assert (res["c"].cpu() - ref).abs().max().item() <= 1e-13 * D * a.abs().max().item() * b.abs().max().item()
        assert torch.equal(res["c"], res["c_w"])

    row(f"fid-gemm-{D}", ("lg_fid_gemm",), run, check)


fid_gemm_row(70)
fid_gemm_row(193)


def fid_distance_row(D, N, seed):
    """the Frechet distance with its device operands guarded (result_host is host memory): test_distance_full_rank_against_eigh"""
    def run(ops, alloc):
        m1, s1, m2, s2 = fixture(D, N, seed)
        d2, tr_sqrt, it, status = ops.fid_distance(alloc.inp("mu1", m1), alloc.inp("s1", s1), alloc.inp("mu2", m2), alloc.inp("s2", s2))
        return dict(d2=d2, tr_sqrt=tr_sqrt, iterations=it, status=status)

    def check(res):
        m1, s1, m2, s2 = fixture(D, N, seed)
        ref, _ = eigh_reference(m1, s1, m2, s2)
        assert res["status"] == 0 and abs(res["d2"] - ref) <= 1e-9 * (np.trace(s1) + np.trace(s2))

    row(f"fid-distance-{D}", ("lg_fid_distance",), run, check, sizing=[("lg_fid_distance_workspace_bytes", (D,))])


fid_distance_row(70, 600, 4)


def pairs_row(case):
    """pairs_poly_sum (added onto seeded sums, and its diagonal form), pairs_knn (merged into +inf lists) and pairs_ball_count (added
    onto seeded counters): against the brute-force fp64 oracle of tests/test_metrics_cpu.py with its bounds (tests/test_metrics_gpu.py)"""
    kk = 3

    @functools.lru_cache(maxsize=None)
    def data():
        real, fake = make_sets(*case)
        d2 = oracle_d2(real, fake)
        if real.shape[0] > 3:   # fakes inside the real balls of k = 3
            return real, fake, d2, np.sort(oracle_d2(real, real), axis=1)[:, 3], fake, real, d2.T
        return real, fake, d2, np.full(fake.shape[0], d2.mean()), real, fake, d2

    def run(ops, alloc):
        real, fake, d2, r2, qs, ref, _ = data()
        n, m = real.shape[0], fake.shape[0]
        x, y = alloc.inp("x", real), alloc.inp("y", fake)
        sums = ops.pairs_poly_sum(x, y, alloc.state("sums", np.array([1.5, -2.0])))
        diag = ops.pairs_poly_sum(x, alloc.inp("x_again", real), alloc.state("diag", np.zeros(2)), diag=True)
        best = ops.pairs_knn(x, y, alloc.state("best", np.full((n, min(kk, m)), np.inf)))
        count = ops.pairs_ball_count(alloc.inp("q", qs), alloc.inp("ref", ref), alloc.inp("radius2", r2),
                                     alloc.state("count", torch.full((qs.shape[0],), 7, dtype=I32)))
        return dict(sums=sums, diag=diag, best=best, count=count)

    def check(res):
        real, fake, d2, r2, _, _, dq = data()
        s, _, bound, _ = oracle_poly(real, fake)
        assert abs(res["sums"][0].item() - 1.5 - s) <= bound and res["sums"][1].item() == -2.0
        s, tr, bound, tbound = oracle_poly(real, real)
        assert abs(res["diag"][0].item() - s) <= bound and abs(res["diag"][1].item() - tr) <= tbound
        k = res["best"].shape[1]
        assert np.abs(res["best"].cpu().numpy() - np.sort(d2, axis=1)[:, :k]).max() <= 4 * dot_eps(real, fake)
        assert ball_margin(dq, r2) >= MARGIN             # the oracle excludes no pair: exactness may be asked
        want = (dq <= r2[None, :]).sum(1)
        assert 0 < want.sum() < dq.size and np.array_equal(res["count"].cpu().numpy(), 7 + want)

    n, m, D = case[1:]
    row(f"pairs-{'x'.join(map(str, case))}", ("lg_pairs_poly_sum", "lg_pairs_knn", "lg_pairs_ball_count"), run, check,
        sizing=[("lg_pairs_workspace_bytes", (n, m, D)), ("lg_pairs_workspace_bytes", (n, n, D)), ("lg_pairs_workspace_bytes", (m, n, D))])


pairs_row((6, 1, 3, 5))
pairs_row(min(PAIR_CASES, key=lambda c: c[1] * c[2] * c[3]))


# ------------------------------------------------------------------------------------------------------------------ the entry points without a mirror operand
def legacy_row():
    """The entry points of the first ABI generation, which the wrappers no longer call (they forward to the *_m16 / *_z16 / *_db
    forms with null mirrors): called through ctypes at the gather / per-tap shape, results bit-equal to the wrappers' route."""
    B, Hs, Ws, cb, cs = 3, 5, 6, 32, 64
    shape = (3, 4, 4, 32)
    L = 4 * 4 * 32

    @functools.lru_cache(maxsize=None)
    def data():
        s = crc("legacy")
        return dict(x=arr(s, B, 2 * Hs, 2 * Ws, cb), w=arr(s + 1, 5, 5, cb, cs, scale=0.1), dy=arr(s + 2, B, Hs, Ws, cs),
                    xs=arr(s + 3, B, 6, 10, 32), w3=arr(s + 4, 5, 5, 3, 32, scale=0.05), b3=arr(s + 5, 3, scale=0.1), dpre=arr(s + 6, B, 6, 10, 3),
                    z=arr(s + 7, *shape, scale=1.5, shift=0.7), g=arr(s + 8, *shape))

    def run(ops, alloc):
        d = data()
        lib, chk, st_ = ops._lib.load(), ops._lib.check, torch.cuda.current_stream().cuda_stream
        t = {k: alloc.inp(k, v) for k, v in d.items()}
        pack = ops.conv_pack(t["w"], cb, cs, 0, out=alloc.out("pack", (ops.conv_pack_bytes(cb, cs, 0),), U8))
        pack3 = ops.conv_pack(t["w3"], 3, 32, 0, out=alloc.out("pack3", (ops.conv_pack_bytes(3, 32, 0),), U8))
        P = lambda v: 0 if v is None else v.data_ptr()   # noqa: E731
        o = dict(dx=alloc.out("dx", d["x"].shape), dxT=alloc.out("dxT", d["dy"].shape), dw=alloc.out("dw", (5, 5, cb, cs)),
                 dwT=alloc.out("dwT", (5, 5, cb, cs)), db=alloc.out("db", (cs,)), y3=alloc.out("y3", (B, 6, 10, 3)),
                 dx3=alloc.out("dx3", (B, 6, 10, 32)), dw3=alloc.out("dw3", (5, 5, 3, 32)), db3=alloc.out("db3", (3,)),
                 stats=alloc.out("stats", (3, 8)), dz=alloc.out("dz", shape))
        dgm, dbt = alloc.out("dgamma", (1,)), alloc.out("dbeta", (1,))
        gm, bt = _gb(alloc)
        chk(lib.lg_conv2d_s2_dgrad(P(t["dy"]), P(pack), P(o["dx"]), B, Hs, Ws, cb, cs, 0, st_), "lg_conv2d_s2_dgrad")
        chk(lib.lg_convT_s2_dgrad(P(t["x"]), P(pack), P(o["dxT"]), B, Hs, Ws, cb, cs, 0, st_), "lg_convT_s2_dgrad")
        ws = ops.workspace(int(lib.lg_wgrad_workspace_bytes(B, Hs, Ws, cb, cs, 0)), "cuda", "wgrad")
        chk(lib.lg_conv2d_s2_wgrad(P(t["x"]), P(t["dy"]), P(o["dw"]), P(ws), ws.numel(), B, Hs, Ws, cb, cs, 0, 0, st_), "lg_conv2d_s2_wgrad")
        ws = ops.workspace(int(lib.lg_wgrad_workspace_bytes(B, Hs, Ws, cb, cs, 0)), "cuda", "wgrad")
        chk(lib.lg_convT_s2_wgrad(P(t["dy"]), P(t["x"]), P(o["dwT"]), P(ws), ws.numel(), B, Hs, Ws, cb, cs, 0, 0, st_), "lg_convT_s2_wgrad")
        ws = ops.workspace(int(lib.lg_bias_grad_workspace_bytes(B * Hs * Ws, cs)), "cuda", "small")
        chk(lib.lg_bias_grad(P(t["dy"]), P(o["db"]), P(ws), ws.numel(), B * Hs * Ws, cs, 0, st_), "lg_bias_grad")
        chk(lib.lg_convT_s1_tanh_fwd(P(t["xs"]), P(pack3), P(t["b3"]), P(o["y3"]), B, 6, 10, 3, 32, 0, st_), "lg_convT_s1_tanh_fwd")
        ws = ops.workspace(int(lib.lg_convT_s1_bwd_workspace_bytes(B, 6, 10, 3, 32, 0)), "cuda", "wgrad")
        chk(lib.lg_convT_s1_tanh_bwd(P(t["xs"]), P(t["dpre"]), P(pack3), P(o["dx3"]), P(o["dw3"]), P(o["db3"]), P(ws), ws.numel(), B, 6, 10, 3, 32,
                                     0, 0, st_), "lg_convT_s1_tanh_bwd")
        ws = ops.workspace(int(lib.lg_instnorm_workspace_bytes(3, L)), "cuda", "small")
        chk(lib.lg_instnorm_leaky_stats(P(t["z"]), P(o["stats"]), P(gm), P(bt), P(ws), ws.numel(), 3, L, 0, ALPHA, st_), "lg_instnorm_leaky_stats")
        ws = ops.workspace(int(lib.lg_instnorm_bwd_db_workspace_bytes(3, L, 0)), "cuda", "small")
        chk(lib.lg_instnorm_leaky_bwd(P(t["z"]), P(o["stats"]), P(t["g"]), 0, P(o["dz"]), 0, P(dgm), P(dbt), P(ws), ws.numel(), 3, L, 0, 1, ALPHA,
                                      0, st_), "lg_instnorm_leaky_bwd")
        o.update(dgamma=dgm, dbeta=dbt)
        return o

    def check(res):
        d = {k: v.astype(np.float64) for k, v in data().items()}
        zero = np.zeros((5, 5, cb, cs))
        dx_e, dw_e, db_e = O.conv2d_bwd(d["x"], d["w"], d["dy"], 2)
        assert rel(res["dx"], dx_e) < TOL[0] and rel(res["dw"], dw_e) < TOL[0] and rel(res["db"], db_e) < 3e-5
        assert rel(res["dxT"], O.conv2d_transpose_bwd(d["dy"], d["w"], d["x"], 2)[0]) < TOL[0]
        assert rel(res["dwT"], O.conv2d_transpose_bwd(d["dy"], zero, d["x"], 2)[1]) < TOL[0]
        assert rel(res["y3"], np.tanh(O.conv2d_transpose(d["xs"], d["w3"], d["b3"], 1))) < TOL[0]
        dx3, dw3, db3 = O.conv2d_transpose_bwd(d["xs"], d["w3"], d["dpre"], 1)
        assert rel(res["dx3"], dx3) < TOL[0] and rel(res["dw3"], dw3) < 3e-5 and rel(res["db3"], db3) < 3e-5
        y_e, cache = O.instnorm(d["z"], 1.2, 0.1)
        dz_e, dg_e, db_e = O.instnorm_bwd(cache, 1.2, O.leaky_bwd(y_e, d["g"], ALPHA))
        assert rel(res["stats"][:, 0], d["z"].reshape(3, -1).mean(1)) < 1e-5 and rel(res["dz"], dz_e) < 2e-5
        assert abs(float(res["dgamma"]) - dg_e) < 2e-5 * max(1.0, abs(dg_e)) * 10 and abs(float(res["dbeta"]) - db_e) < 2e-5 * max(1.0, abs(db_e)) * 10

    row("legacy-entry-points", ("lg_conv2d_s2_dgrad", "lg_convT_s2_dgrad", "lg_conv2d_s2_wgrad", "lg_convT_s2_wgrad", "lg_bias_grad",
                                "lg_convT_s1_tanh_fwd", "lg_convT_s1_tanh_bwd", "lg_instnorm_leaky_stats", "lg_instnorm_leaky_bwd"), run, check,
        sizing=[("lg_bias_grad_workspace_bytes", (B * Hs * Ws, cs)), ("lg_convT_s1_bwd_workspace_bytes", (B, 6, 10, 3, 32, 0)),
                ("lg_instnorm_workspace_bytes", (3, L))], wgrad=(B, Hs, Ws, cb, cs, 0))


legacy_row()


# ------------------------------------------------------------------------------------------------------------------ adaptive augmentation probability
def ada_draw_row(rows, S):
    """the gated draw against its restatement bit for bit: tests/test_ada_gpu.py"""
    seed, koff = 0x7654321, (9 << 40) + 3

    def run(ops, alloc):
        key = alloc.inp("key", torch.tensor([seed, koff], dtype=torch.int64))
        state = alloc.inp("state", torch.from_numpy(words(0.5, 7, 9, 1))).view(torch.float32)
        return dict(drawn=ops.diffaug_draw_gated(key, 1, 2, rows, S, FULL, state, out=alloc.out("params", (rows, 8))))

    def check(res):
        assert np.array_equal(u32(res["drawn"].cpu().numpy()), u32(draw_params_gated(seed, koff, 1, 2, rows, S, FULL, 0.5)))

    row(f"ada-draw-{rows}x{S}", ("lgx_diffaug_draw_gated",), run, check)


def ada_accumulate_row(B, ld):
    st = (0.375, -3, 11, 1)

    def run(ops, alloc):
        state = alloc.state("state", torch.from_numpy(words(*st)))
        ops.ada_accumulate(state.view(torch.float32), alloc.inp("heads", heads_mix(B, ld, 3)), B)
        return dict(state=state)

    def check(res):
        want = ada_accumulate_np((np.float32(st[0]),) + st[1:], heads_mix(B, ld, 3), B)
        assert res["state"].cpu().numpy().tolist() == words(*want).tolist()

    row(f"ada-accumulate-{B}x{ld}", ("lgx_ada_accumulate",), run, check)


def ada_adjust_row(tag, st):
    def run(ops, alloc):
        state = alloc.state("state", torch.from_numpy(words(*st)))
        ops.ada_adjust(state.view(torch.float32), 2, 0.6, PER_ROW)
        return dict(state=state)

    def check(res):
        want = ada_adjust_np((np.float32(st[0]),) + st[1:], 2, 0.6, PER_ROW)
        assert res["state"].cpu().numpy().tolist() == words(*want).tolist()
        assert (want[1:] == (0, 0, 0)) == (tag == "due")

    row(f"ada-adjust-{tag}", ("lgx_ada_adjust",), run, check)


def ada_init_row():
    def run(ops, alloc):
        return dict(state=ops.ada_init(0.625, out=alloc.out("state", (4,))).view(torch.int32))

    def check(res):
        assert res["state"].cpu().numpy().tolist() == words(0.625).tolist()

    row("ada-init", ("lgx_ada_init",), run, check)


ada_draw_row(3, 8)
ada_accumulate_row(65, 6)
ada_adjust_row("due", (0.5, 5, 6, 2))
ada_adjust_row("not-due", (0.5, 5, 6, 1))
ada_init_row()


# ------------------------------------------------------------------------------------------------------------------ R1 gradient penalty
def r1_seed_row(B, L):
    """the three R1 kernels bit for bit in exact arithmetic: tests/test_r1_gpu.py (data: tests/test_r1_cpu.py)"""
    def run(ops, alloc):
        g = alloc.inp("g", exact_seed_case(B, L)[0])
        loss, r1l = alloc.state("loss", np.array([R1_LOSS0], np.float32)), alloc.out("r1_loss", (1,))
        u0, r2 = alloc.out("u0", (B, L)), alloc.out("r2", (B,))
        lib = ops._lib.load()
        ws = ops.workspace(int(lib.lgr_r1_workspace_bytes(B, L)), g.device, "r1")   # (the wrapper allocates its outputs: guarded ones here)
        ops._lib.check(lib.lgr_r1_seed(g.data_ptr(), u0.data_ptr(), r2.data_ptr(), loss.data_ptr(), r1l.data_ptr(), EXACT_WEIGHT,
                                       ws.data_ptr(), ws.numel(), B, L, torch.cuda.current_stream().cuda_stream), "lgr_r1_seed")
        return dict(u0=u0, r2=r2, loss=loss, r1_loss=r1l)

    def check(res):
        _, u0, r2, term, loss = exact_seed_case(B, L)
        assert np.array_equal(i32(res["u0"]), np_i32(u0)) and np.array_equal(i32(res["r2"]), np_i32(r2))
        assert np.array_equal(i32(res["r1_loss"]), np_i32([term])) and np.array_equal(i32(res["loss"]), np_i32([loss]))

    row(f"r1-seed-{B}x{L}", ("lgr_r1_seed",), run, check, sizing=[("lgr_r1_workspace_bytes", (B, L))])


def r1_colsum_row(B, K):
    def run(ops, alloc):
        u, d0, _ = exact_colsum_case(B, K)
        dw = alloc.state("dwpr", d0)
        ops.r1_heads_colsum(alloc.inp("u", u), dw)
        return dict(dwpr=dw)

    def check(res):
        assert np.array_equal(i32(res["dwpr"]), np_i32(exact_colsum_case(B, K)[2]))

    row(f"r1-colsum-{B}x{K}", ("lgr_r1_heads_colsum",), run, check, sizing=[("lgr_r1_colsum_workspace_bytes", (B, K))])


def r1_heads_seed_row(B, K):
    def run(ops, alloc):
        wpr = alloc.inp("wpr", heads_seed_wpr(K).reshape(K, 1))
        g = alloc.out("g", (B, K))
        ops._lib.check(ops._lib.load().lgr_r1_heads_seed(wpr.data_ptr(), g.data_ptr(), B, K, torch.cuda.current_stream().cuda_stream),
                       "lgr_r1_heads_seed")
        return dict(g=g.view(torch.int32))   # compared as words: a NaN is equal to itself

    def check(res):
        assert np.array_equal(res["g"].cpu().numpy(), np.broadcast_to(heads_seed_wpr(K).view(np.int32), (B, K)))

    row(f"r1-heads-seed-{B}x{K}", ("lgr_r1_heads_seed",), run, check)


r1_seed_row(1, 4)
r1_seed_row(4, 4100)
r1_colsum_row(1, 4)
r1_colsum_row(33, 5)
r1_heads_seed_row(1, 1)
r1_heads_seed_row(3, 8)


# ------------------------------------------------------------------------------------------------------------------ logit-side objectives
def heads_logit_row(case):
    """the heads forward that keeps the logit, on both GEMM routes, and the loss on it: tests/test_gan_loss_gpu.py"""
    B, K, c, route = case

    def run(ops, alloc):
        x, wpr, bpr, wc, bc = _heads_operands(case, "int")
        ins = [alloc.inp(n, a.astype(np.float32)) for n, a in (("x", x), ("wpr", wpr), ("bpr", bpr), ("wc", wc), ("bc", bc))]
        p, z = ops.heads_fwd_logit(*ins, out=alloc.out("p", (B, 1 + c)), z_out=alloc.out("z_pr", (B,)))   # the workspace comes exactly sized
        return dict(p=p, z_pr=z)

    def check(res):
        x, wpr, bpr, wc, bc = _heads_operands(case, "int")
        assert np.array_equal(i32(res["z_pr"]), np_i32((x @ wpr + bpr)[:, 0]))
        assert rel(res["p"], np.concatenate([O.sigmoid(x @ wpr + bpr), O.sigmoid(x @ wc + bc)], 1)) < 1e-5

    row(f"heads-fwd-logit-{B}x{K}x{c}", ("lgo_heads_fwd",), run, check, route=HEADS_FWD[route])


def gan_loss_row(kind, role, B, c):
    def run(ops, alloc):
        p, t_c = _heads_data(B, c, 23 * B + c)
        z = exact_case(kind, role, B)[0]
        loss, dz = alloc.state("loss", np.array([GAN_LOSS0], np.float32)), alloc.out("dz", (B, 1 + c))
        ops.gan_heads_loss(alloc.inp("p", p.astype(np.float32)), alloc.inp("z_pr", z), alloc.inp("t_c", t_c.astype(np.float32)), KIND_NO[kind], role,
                           EXACT_W_PR, 1.0, loss, dz, True)
        return dict(loss=loss, dz=dz)

    def check(res):
        p, t_c = _heads_data(B, c, 23 * B + c)
        _, dz_w, term_w, _ = exact_case(kind, role, B)
        assert np.array_equal(i32(res["dz"][:, 0]), np_i32(dz_w))
        exp = GAN_LOSS0 + float(term_w) + O.bce_mean(t_c, p[:, 1:])
        assert abs(float(res["loss"]) - exp) < 2e-6 * abs(exp) + 1e-6
        assert rel(res["dz"][:, 1:], O.bce_mean_bwd(t_c, p[:, 1:]) * p[:, 1:] * (1 - p[:, 1:])) < 1e-5

    row(f"gan-loss-{kind}-{role}-{B}x{c}", ("lgo_gan_heads_loss_fwd_bwd",), run, check, route="gan_heads_kernel")


heads_logit_row(LOGIT_HEADS_CASES[4])
heads_logit_row(LOGIT_HEADS_CASES[0])
gan_loss_row("hinge", ROLE_D_REAL, 1, 1)
gan_loss_row("lsgan", ROLE_D_FAKE, 4, 3)
gan_loss_row("wgan", ROLE_G, 1024, 40)


# ------------------------------------------------------------------------------------------------------------------ geometric augmentation
def geom_draw_row():
    """the draw, plain and gated, against the restatement of tests/test_geom_cpu.py at the bound of tests/test_geom_gpu.py"""
    rows, S, seed_arg, step = 300, 16, 3, 7        # two blocks of the one-thread-per-row launch, the second partly empty
    seed, koff = key_of(seed_arg, 1, step)

    def run(ops, alloc):
        key = alloc.inp("key", np.array([seed, koff], np.int64))
        state = alloc.inp("state", np.array([0.3, 0, 0, 0], np.float32))
        return {"plain": ops.geom_draw(key, 1, 5, rows, S, GEOM_FULL, out=alloc.out("geo", (rows, 4))),
                "gated": ops.geom_draw(key, 0, 0, rows, S, GEOM_FULL, state=state, out=alloc.out("geo_gated", (rows, 4)))}

    def check(res):
        for name, want in (("plain", geom_records(seed, koff, 1, 5, rows, S, GEOM_FULL)),
                           ("gated", geom_records(seed, koff, 0, 0, rows, S, GEOM_FULL, p=0.3))):
            got = res[name].cpu().numpy()
            assert (np.abs(got.astype(np.float64) - want) <= 2.0 ** -23 * np.maximum(1, np.abs(want))).all(), name
            exact = (np.abs(want) == 1) | (want == 0)        # what a selected identity leaves
            assert np.array_equal(got[exact], want[exact]), name

    row("geom-draw-300", ("lgeo_draw",), run, check, exact_sizing=True)


def geom_map_row(id_, S, recs, seed):
    """Geo and its adjoint: lgeo_fwd within 8 2^-24 max|x| per row of the restatement (one rounding per weight product, per term, per
    add), lgeo_bwd within (n + 3) 2^-24 sum |w g| per source pixel of the scatter restatement; an unusable record gives zeros"""
    B = len(recs)
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (B, S, S, 3)).astype(np.float32)
    g = rng.uniform(-1, 1, (B, S, S, 3)).astype(np.float32)

    def run(ops, alloc):
        geo = alloc.inp("geo", recs)
        return {"out": ops.geom_fwd(alloc.inp("x", x), geo, out=alloc.out("out", x.shape)),
                "gx": ops.geom_bwd(alloc.inp("g", g), geo, out=alloc.out("gx", g.shape))}

    def check(res):
        assert torch.isfinite(res["out"]).all() and torch.isfinite(res["gx"]).all()
        err = np.abs(f64(res["out"]) - geom_np(x, recs)).reshape(B, -1).max(1)
        bound = 8 * 2.0 ** -24 * np.abs(x).reshape(B, -1).max(1)
        assert (err <= bound).all(), (err, bound)
        ref, cnt, mag = geom_adjoint_np(g, recs, stats=True)
        bound = (cnt[..., None] + 3) * 2.0 ** -24 * mag
        assert (np.abs(f64(res["gx"]) - ref) <= bound).all(), float((np.abs(f64(res["gx"]) - ref) - bound).max())
        dead = [n for n, r in enumerate(recs) if not usable(r)]
        assert not res["out"][dead].any() and not res["gx"][dead].any()

    row(id_, ("lgeo_fwd", "lgeo_bwd"), run, check, exact_sizing=True)


def geom_arbitrary_records():
    """Record bits a kernel has to survive: random 32-bit patterns (NaN, infinities, every exponent), entries with random mantissas near
    1, nearly singular matrices at both sides of the 2^-20 bound, huge entries with a finite determinant, denormals and negative zeros.
    The records are device data that the host cannot validate, so the kernels compare every coordinate as a float before it becomes an
    index: the row checks that property (nothing read outside x, nothing written outside out)."""
    rng = np.random.default_rng(2026)
    recs = [rng.integers(0, 1 << 32, 4, dtype=np.uint64).astype(np.uint32).view(np.float32) for _ in range(8)]
    recs += [rng.uniform(-1.5, 1.5, 4).astype(np.float32) for _ in range(4)]
    recs += [np.array(r, np.float32) for r in (
        [1, 1, 1, 1 + 2.0 ** -19], [1, 1, 1, 1 + 2.0 ** -21], [2.0 ** -9, 0, 0, 2.0 ** -9], [1e30, 0, 0, 1e-30], [1e30, -1e30, 1, 0],
        [3e38, 3e38, -3e38, 3e38], [1e-40, 0, 0, 1e-40], [-0.0, 1, -1, -0.0], [np.nan] * 4, [np.inf, 0, 0, -np.inf], [0, 0, 0, 0],
        [1e19, 1, 1e-19, 1], [512, 0, 0, 2.0 ** -9])]
    return np.stack(recs).astype(np.float32)


geom_draw_row()
geom_map_row("geom-extreme-records-16", 16, geom_extreme_records(), 11)
geom_map_row("geom-arbitrary-records-8", 8, geom_arbitrary_records(), 12)
geom_map_row("geom-workload-row-128", 128, geom_extreme_records()[[0, 10]], 13)      # the workload's row length: many blocks, the row stride


# ------------------------------------------------------------------------------------------------------------------ relativistic pairing, R1 + R2
def rel_pair_row(kind, side, n, m, c):
    """the pairing loss in exact arithmetic: tests/test_rel_gpu.py (data: tests/test_rel_cpu.py)"""
    def run(ops, alloc):
        p, t_c = _heads_data(n, c, 23 * n + c)
        z, zr, _, _ = exact_pair_case(kind, side, n, m)
        loss, dz = alloc.state("loss", np.array([PAIR_LOSS0], np.float32)), alloc.out("dz", (n, 1 + c))
        ops.pair_heads_loss(alloc.inp("p", p.astype(np.float32)), alloc.inp("z", z), alloc.inp("z_ref", zr), alloc.inp("t_c", t_c.astype(np.float32)),
                            PAIR_KIND_NO[kind], side, PAIR_W_PR, 1.0, loss, dz, True)
        return dict(loss=loss, dz=dz)

    def check(res):
        p, t_c = _heads_data(n, c, 23 * n + c)
        _, _, dz_w, term_w = exact_pair_case(kind, side, n, m)
        assert torch.equal(res["dz"][:, 0].cpu(), torch.from_numpy(dz_w))
        exp = PAIR_LOSS0 + float(term_w) + O.bce_mean(t_c, p[:, 1:])
        assert abs(float(res["loss"]) - exp) < 2e-6 * abs(exp) + 1e-6
        assert rel(res["dz"][:, 1:], O.bce_mean_bwd(t_c, p[:, 1:]) * p[:, 1:] * (1 - p[:, 1:])) < 1e-5

    row(f"rel-pair-{kind}-{side}-{n}x{m}x{c}", ("lgrel_pair_heads_loss_fwd_bwd",), run, check, exact_sizing=True)


def rel_seed_row(B, L):
    """the joint R1 + R2 seed bit for bit: the exact case of tests/test_r1_cpu.py as the real half, tests/test_rel_gpu.py::_seed_halves"""
    def run(ops, alloc):
        g = alloc.inp("g", _seed_halves(B, L)[0])
        loss = alloc.state("loss", np.array([R1_LOSS0], np.float32))
        r1l, r2l = alloc.out("r1_loss", (1,)), alloc.out("r2_loss", (1,))
        u0, r2 = alloc.out("u0", (2 * B, L)), alloc.out("r2", (2 * B,))
        lib = ops._lib.load()
        ws = ops.workspace(int(lib.lgrel_r12_workspace_bytes(B, L)), g.device, "r1")   # (the wrapper allocates its outputs: guarded ones here)
        ops._lib.check(lib.lgrel_r12_seed(g.data_ptr(), u0.data_ptr(), r2.data_ptr(), loss.data_ptr(), r1l.data_ptr(), r2l.data_ptr(), EXACT_WEIGHT,
                                          W_FAKE, ws.data_ptr(), ws.numel(), B, L, torch.cuda.current_stream().cuda_stream), "lgrel_r12_seed")
        return dict(u0=u0, r2=r2, loss=loss, r1_loss=r1l, r2_loss=r2l)

    def check(res):
        _, u0, r2, t1, t2, loss = _seed_halves(B, L)
        assert np.array_equal(i32(res["u0"]), np_i32(u0)) and np.array_equal(i32(res["r2"]), np_i32(r2))
        assert np.array_equal(i32(res["r1_loss"]), np_i32([t1])) and np.array_equal(i32(res["r2_loss"]), np_i32([t2]))
        assert np.array_equal(i32(res["loss"]), np_i32([loss]))

    row(f"rel-r12-seed-{B}x{L}", ("lgrel_r12_seed",), run, check, sizing=[("lgrel_r12_workspace_bytes", (B, L))], exact_sizing=True)


rel_pair_row("hinge", SIDE_SELF, 1, 1, 1)
rel_pair_row("lsgan", SIDE_OTHER, 6, 3, 3)
rel_seed_row(1, 4)
rel_seed_row(4, 4100)


# ------------------------------------------------------------------------------------------------------------------ learning-rate schedule
def sched_init_row(k0):
    def run(ops, alloc):
        return dict(state=ops.sched_init(k0, out=alloc.out("state", (8,))))

    def check(res):
        assert i32(res["state"]).tolist() == [k0, 0, 0, 0, 0, 0, 0, 0]

    row(f"sched-init-{k0}", ("lgsch_init",), run, check, exact_sizing=True)


def sched_step_row(k):
    """one step of the schedule against config.lr_factor: tests/test_lr_schedule_gpu.py"""
    def run(ops, alloc):
        c = sched_settings("cosine", W=3, N=7, r=0.1, **RATES)
        words_ = np.array([k, 0, 0, 0, 0, 0, 0, 0], np.int32).view(np.float32)
        state = alloc.state("state", words_)
        ops.sched_step(state, c["kind"], c["warmup"], c["decay"], c["final_ratio"], c["lr_g"], c["lr_d"], c["lr_adj"])
        return dict(state=state)

    def check(res):
        from littlegan_amd import config
        c = sched_settings("cosine", W=3, N=7, r=0.1, **RATES)
        got = i32(res["state"])
        assert got[0] == k + 1 and not got[5:].any() and abs(int(got[1]) - int(np_i32([config.lr_factor(k, c)])[0])) <= 1
        s = res["state"].cpu().numpy()[1]
        assert got[2:5].tolist() == np_i32([np.float32(c[m]) * s for m in ("lr_g", "lr_d", "lr_adj")]).tolist()

    row(f"sched-step-{k}", ("lgsch_step",), run, check, exact_sizing=True)


def sched_adam_row(n, ema):
    """the Adam passes that read their rate from device memory, bit for bit against the ones that take it as a scalar"""
    def data():
        rng = np.random.default_rng(900 + n)
        return {k: rng.standard_normal(n).astype(np.float32) * sc for k, sc in (("w", 1.0), ("g", 1.0), ("m", 0.1), ("e", 1.0))}, \
            np.abs(rng.standard_normal(n)).astype(np.float32) * 0.1

    lo, hi = (4 * (n // 12), 4 * (n // 6)) if ema else (0, n)

    def run(ops, alloc):
        d, v0 = data()
        w, m, v = alloc.state("w", d["w"]), alloc.state("m", d["m"]), alloc.state("v", v0)
        g, st, lr = alloc.inp("g", d["g"]), alloc.inp("adam_state", np.array([0.25, 0.81], np.float32)), alloc.inp("lr", np.array([1e-2], np.float32))
        if not ema:
            ops.sched_clip_adam_update(w, g, m, v, st, lr, B1, B2, EPS, 0.5, 0.5)
            return dict(w=w, m=m, v=v)
        e = alloc.state("ema", d["e"])
        count = alloc.inp("ema_state", np.array([7], np.int32))
        ops.sched_clip_adam_ema_update(w, g, m, v, e, lo, hi, st, count, lr, B1, B2, EPS, 0.5, 0.5, 0.99)
        return dict(w=w, m=m, v=v, ema=e)

    def check(res):
        from littlegan_amd import ops
        d, v0 = data()
        dev = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
        w, m, v, g, e = dev(d["w"]), dev(d["m"]), dev(v0), dev(d["g"]), dev(d["e"])
        st = torch.tensor([0.25, 0.81], dtype=torch.float32, device="cuda")
        if ema:
            ops.clip_adam_ema_update(w, g, m, v, e, lo, hi, st, torch.tensor([7], dtype=torch.int32, device="cuda"), 1e-2, B1, B2, EPS, 0.5, 0.5, 0.99)
            assert _same(res["ema"], e) and 0 < lo < hi < n
        else:
            ops.clip_adam_update(w, g, m, v, st, 1e-2, B1, B2, EPS, 0.5, 0.5)
        assert _same(res["w"], w) and _same(res["m"], m) and _same(res["v"], v)

    row(f"sched-adam{'-ema' if ema else ''}-{n}", ("lgsch_clip_adam_ema_update" if ema else "lgsch_clip_adam_update",), run, check,
        exact_sizing=True)


sched_init_row(5)
sched_step_row(6)        # strictly inside the cosine decay
sched_adam_row(257, False)
sched_adam_row(1028, True)


# ------------------------------------------------------------------------------------------------------------------ the Adjuster's fused forward
@functools.lru_cache(maxsize=None)
def _records16(ops, seed, shape, scale, shift, gamma, beta):
    """a bf16 map (seeded) and its finished statistics records, from the library's own statistics pass on its fp32 value -> CPU tensors.
    Cached: the pass runs once, in the row's first run, on the pooled workspace, and never between guard bands."""
    a = bf(arr(seed, *shape, scale=scale, shift=shift))
    gm, bt = (torch.tensor([v], dtype=F32, device="cuda") for v in (gamma, beta))
    return a, ops.instnorm_stats(a.cuda().float(), gm, bt, 0, ALPHA).cpu()


def _stored_map(ops, z, stats):
    """the bf16 map the encoder's apply pass stores for a raw level (z, records)"""
    h = torch.empty_like(z)
    ops.instnorm_apply(z, stats, None, 0, 1, ALPHA, out16=h, want_f32=False)
    return h


def adj_fused_row(cs, cb, Hs, Ws):
    """lgadj_convT_s2_fwd_stats_ns with an uneven split of a raw and a stored skip part, bit for bit against the route through the
    stored maps (instnorm_apply per skip part + convT_s2_fwd_stats): tests/test_adj_fused_gpu.py"""
    B, b1 = 3, 1
    s = crc("adj-fused", cs, cb, Hs, Ws)
    nbytes = _stats_bytes(True, B, Hs, Ws, cb)

    def data(ops):
        z, zst = _records16(ops, s, (B, Hs, Ws, cs), 1.3, 0.2, 0.9, 0.15)
        s0, s0st = _records16(ops, s + 1, (b1, Hs, Ws, cs), 0.8, -0.3, 1.1, -0.2)
        return z, zst, s0, s0st, bf(arr(s + 2, B - b1, Hs, Ws, cs)), arr(s + 3, 5, 5, cb, cs, scale=0.05), arr(s + 4, cb, scale=0.2)

    def run(ops, alloc):
        z, zst, s0, s0st, s1, w, b = data(ops)
        tr = Trace(ops)
        lib, P = ops._lib.load(), lambda v: v.data_ptr()   # noqa: E731
        zd, zstd = alloc.inp("z16", z), alloc.inp("z_stats", zst)
        s0d, s0std, s1d = alloc.inp("skip0", s0), alloc.inp("skip0_stats", s0st), alloc.inp("skip1", s1)
        pack, bd = _pack(ops, alloc, w, cb, cs, 1), alloc.inp("bias", b)
        gm, bt = _gb(alloc, 1.2, -0.1)
        out, stats = alloc.out("out16", (B, 2 * Hs, 2 * Ws, cb), BF16), alloc.out("stats", (B, 8))
        want = int(getattr(lib, nbytes[0])(*nbytes[1]))
        ws = ops.workspace(want, zd.device, "statpart")          # (the wrapper allocates its outputs: guarded ones here)
        nparts, st_ = ctypes.c_int(0), torch.cuda.current_stream().cuda_stream
        ops._lib.check(lib.lgadj_convT_s2_fwd_stats_ns(P(zd), P(zstd), ALPHA, P(s0d), P(s0std), P(s1d), 0, b1, P(pack), P(bd), P(out), B, Hs, Ws,
                                                       cb, cs, 1, P(ws), ws.numel(), ctypes.addressof(nparts), st_), "lgadj_convT_s2_fwd_stats_ns")
        tr("fwd")
        ops._lib.check(lib.lg_instnorm_stats_finalize(P(ws), nparts.value, P(stats), P(gm), P(bt), B, st_), "lg_instnorm_stats_finalize")
        return dict(pack=pack, out16=out, stats=stats, nparts=nparts.value, ws_bytes=want, _route=tr)

    def check(res):
        from littlegan_amd import ops
        z, zst, s0, s0st, s1, _, b = (t.cuda() if torch.is_tensor(t) else t for t in data(ops))
        assert 0 < res["nparts"] * B * 24 <= res["ws_bytes"]
        h = torch.empty_like(z)
        ops.instnorm_apply(z[:b1], zst[:b1], _stored_map(ops, s0, s0st), 0, 1, ALPHA, out16=h[:b1], want_f32=False)
        ops.instnorm_apply(z[b1:], zst[b1:], s1, 0, 1, ALPHA, out16=h[b1:], want_f32=False)
        gm, bt = (torch.tensor([v], dtype=F32, device="cuda") for v in (1.2, -0.1))
        out, st = ops.convT_s2_fwd_stats(None, res["pack"], torch.from_numpy(b).cuda(), cb, 1, gm, bt, x16=h, z16=True, alpha=ALPHA)
        assert _same(res["out16"], out) and _same(res["stats"], st)
        assert torch.isfinite(out.float()).all() and out.float().abs().max() > 0.1

    row(f"adj-fused-fwd-{B}x{Hs}x{Ws}x{cs}-{cb}", ("lgadj_convT_s2_fwd_stats_ns",), run, check, route="fwd=conv_up3_kernel",
        sizing=[nbytes], exact_sizing=True)


def adj_apply_row(B, L, nparts):
    """the apply pass whose skip is raw, bit for bit against normalise-then-apply; nparts 0: finished records (lgadj_instnorm_apply_rs,
    through the wrapper), else the finalize of nparts partial records per sample folded in (lgadj_instnorm_apply_p_rs)"""
    s = crc("adj-apply", B, L, nparts)

    def data(ops):
        z, zst = _records16(ops, s, (B, L), 1.0, 0.0, 1.1, 0.05)
        sk, skst = _records16(ops, s + 1, (B, L), 1.0, 0.4, 1.1, 0.05)
        return z, zst, sk, skst

    @functools.lru_cache(maxsize=None)
    def partials(ops):
        gm, bt = (torch.tensor([v], dtype=F32, device="cuda") for v in (1.1, 0.05))
        return hand_moments(ops, data(ops)[0].cuda(), nparts, gm, bt).ws.cpu()

    def run(ops, alloc):
        z, zst, sk, skst = data(ops)
        tr = Trace(ops)
        zd, skd, skstd = alloc.inp("z16", z), alloc.inp("skip", sk), alloc.inp("skip_stats", skst)
        y16 = alloc.out("y16", (B, L), BF16)
        if not nparts:
            y = ops.instnorm_apply(zd, alloc.inp("z_stats", zst), ops.Raw(skd, skstd), 0, 1, ALPHA, out=alloc.out("y", (B, L)), out16=y16)
            tr("apply")
            return dict(y=y, y16=y16, _route=tr)
        part, stats = alloc.inp("partials", partials(ops)), alloc.out("stats", (B, 8))   # (ops.Moments allocates the records: guarded ones here)
        gm, bt = _gb(alloc, 1.1, 0.05)
        lib, P = ops._lib.load(), lambda v: v.data_ptr()   # noqa: E731
        ops._lib.check(lib.lgadj_instnorm_apply_p_rs(P(zd), P(part), nparts, P(gm), P(bt), P(stats), P(skd), P(skstd), 0, P(y16), B, L, 1, ALPHA,
                                                     torch.cuda.current_stream().cuda_stream), "lgadj_instnorm_apply_p_rs")
        tr("apply")
        return dict(stats=stats, y16=y16, _route=tr)

    def check(res):
        from littlegan_amd import ops
        z, zst, sk, skst = (t.cuda() for t in data(ops))
        smap, want16 = _stored_map(ops, sk, skst), torch.empty_like(z)
        if not nparts:
            want = ops.instnorm_apply(z, zst, smap, 0, 1, ALPHA, out16=want16)
            assert _same(res["y"], want)
        else:
            gm, bt = (torch.tensor([v], dtype=F32, device="cuda") for v in (1.1, 0.05))
            want_st = ops.stats_tensor(ops.Moments(partials(ops).cuda(), nparts, gm, bt, B))
            ops.instnorm_apply(z, want_st, smap, 0, 1, ALPHA, out16=want16, want_f32=False)
            assert _same(res["stats"], want_st)
        assert _same(res["y16"], want16)

    if nparts:
        row(f"adj-apply-p-rs-{B}x{L}-{nparts}", ("lgadj_instnorm_apply_p_rs",), run, check, route="apply=apply16p_rs_kernel", exact_sizing=True)
    else:
        row(f"adj-apply-rs-{B}x{L}", ("lgadj_instnorm_apply_rs",), run, check, route="apply=apply16_rs_kernel", exact_sizing=True)


adj_fused_row(128, 64, 8, 16)       # both tilings of conv_up3's normalising form
adj_fused_row(64, 32, 8, 32)
adj_apply_row(2, 8 * 1029, 0)       # a sample length that is no multiple of the block's unroll
adj_apply_row(2, 8 * 1029, 5)


# ------------------------------------------------------------------------------------------------------------------ gradient guard
def guard_init_row():
    def run(ops, alloc):
        return dict(rec=ops.guard_init(3, 7, out=alloc.out("rec", (8,))))

    def check(res):
        assert res["rec"].cpu().view(I32).tolist() == [0, 0, 0, 3, 7, 0, 0, 0]

    row("guard-init", ("lgg_init",), run, check, exact_sizing=True)


def guard_sumsq_row(n, poison):
    """partials of exactly P(n) doubles, the record from them, and ops.grad_sumsq through a workspace of exactly lgg_workspace_bytes(n)"""
    def data():
        g = guard_data(n, 100 + n)[0]
        if poison:
            g[n - 1] = np.nan
        return g

    def run(ops, alloc):
        g = alloc.inp("g", data())
        part = alloc.out("partial", (ops.guard_partials_count(n),), F64)
        ops.guard_sumsq_partial(g, part)
        route = ops.last_kernel()
        rec = alloc.state("rec", _rec_np(skipped=2, nonfinite=4))
        ops.guard_finalise(part, n, rec, 0.5, 1e-2, 1)
        S = ops.grad_sumsq(g)
        return dict(partial=part, rec=rec, S=repr(S), _route=route + ";" + ops.last_kernel())

    def check(res):
        from littlegan_amd import config
        want = config.grad_guard_restate(data(), 0.5, float(np.float32(1e-2)), True)
        words_ = res["rec"].cpu().view(I32).tolist()
        assert _ulps(res["rec"][0].item(), want["N"]) <= 1 or poison
        assert words_[2:5] == ([1, 3, 5] if poison else [0, 2, 4]) and words_[6:] == [0, 0]
        assert res["rec"][5].item() == (1.0 if poison else float(_c_from(res["rec"][0].item(), np.float32(1e-2), False)))
        S = float(res["S"])
        assert (math.isnan(S) if poison else abs(S - float(want["S"])) <= n * 2.0 ** -52 * float(want["S"]))

    row(f"guard-sumsq-{n}{'-nan' if poison else ''}", ("lgg_sumsq_partial", "lgg_finalise", "lgg_workspace_bytes", "lgg_partials_count"),
        run, check, sizing=[("lgg_workspace_bytes", (n,))], exact_sizing=True)


def guard_adam_row(n, skip_now):
    eff = float(np.float32(0.5) * np.float32(0.3713))

    def run(ops, alloc):
        w0, g0, m0, _, v0 = guard_data(n, 200 + n)
        w, m, v = alloc.state("w", w0), alloc.state("m", 0.1 * m0), alloc.state("v", v0)
        state = alloc.state("adam_state", np.array([B1 ** 3, B2 ** 3], np.float32))
        rec, lr = alloc.inp("rec", _rec_np(eff, skip_now)), alloc.inp("lr", np.array([1e-2], np.float32))
        ops.guard_clip_adam_update(w, alloc.inp("g", g0), m, v, state, lr, rec, B1, B2, EPS, 0.5)
        ops.guard_adam_advance(state, rec, B1, B2)
        wr, mr, vr = alloc.state("w_ref", w0), alloc.state("m_ref", 0.1 * m0), alloc.state("v_ref", v0)
        sr = alloc.state("state_ref", np.array([B1 ** 3, B2 ** 3], np.float32))
        if not skip_now:
            ops.clip_adam_update(wr, alloc.inp("g_ref", g0), mr, vr, sr, 1e-2, B1, B2, EPS, 0.5, eff)
            ops.adam_advance(sr, B1, B2)
        return dict(w=w, m=m, v=v, state=state, wr=wr, mr=mr, vr=vr, sr=sr)

    def check(res):
        for a, b in (("w", "wr"), ("m", "mr"), ("v", "vr"), ("state", "sr")):
            assert torch.equal(as_i32(res[a]), as_i32(res[b])), a
        assert (res["state"].tolist() == [float(np.float32(B1 ** 3)), float(np.float32(B2 ** 3))]) == bool(skip_now)

    row(f"guard-adam-{n}{'-skip' if skip_now else ''}", ("lgg_clip_adam_update", "lgg_adam_advance"), run, check, exact_sizing=True)


def guard_ema_adam_row(n, lo, hi, skip_now):
    eff = float(np.float32(0.5) * np.float32(0.3713))

    def data():
        w, g, m, e, v = guard_data(n, 300 + n)
        for t in (g, m, v):       # outside the range: whatever is read there poisons the result
            t[:lo], t[hi:] = np.nan, np.nan
        return w, g, 0.1 * m, v, e

    def run(ops, alloc):
        w0, g0, m0, v0, e0 = data()
        w, m, v, ema = alloc.state("w", w0), alloc.state("m", m0), alloc.state("v", v0), alloc.state("ema", e0)
        state = alloc.inp("adam_state", np.array([B1 ** 3, B2 ** 3], np.float32))
        count = alloc.inp("counter", torch.tensor([5], dtype=I32))
        rec, lr = alloc.inp("rec", _rec_np(eff, skip_now)), alloc.inp("lr", np.array([1e-2], np.float32))
        ops.guard_clip_adam_ema_update(w, alloc.inp("g", g0), m, v, ema, lo, hi, state, count, lr, rec, B1, B2, EPS, 0.5, 0.99)
        wr, mr, vr, er = alloc.state("w_ref", w0), alloc.state("m_ref", m0), alloc.state("v_ref", v0), alloc.state("ema_ref", e0)
        ops.clip_adam_ema_update(wr, alloc.inp("g_ref", g0), mr, vr, er, lo, lo if skip_now else hi, state, count, 1e-2, B1, B2, EPS, 0.5,
                                 eff, 0.99)
        return dict(w=w, m=m, v=v, ema=ema, wr=wr, mr=mr, vr=vr, er=er)

    def check(res):
        for a, b in (("w", "wr"), ("m", "mr"), ("v", "vr"), ("ema", "er")):
            assert torch.equal(as_i32(res[a]), as_i32(res[b])), a
        assert torch.isfinite(res["ema"]).all() and torch.isfinite(res["w"]).all()
        assert torch.equal(res["w"].cpu(), torch.from_numpy(data()[0])) == bool(skip_now)

    row(f"guard-adam-ema-{n}{'-skip' if skip_now else ''}", ("lgg_clip_adam_ema_update",), run, check, exact_sizing=True)


guard_init_row()
for _n in (5, CH + 1):      # one group of four and a tail; one element past a chunk: two workgroups
    guard_sumsq_row(_n, False)
    guard_adam_row(_n, 0)
guard_sumsq_row(5, True)
guard_adam_row(5, 1)
guard_ema_adam_row(1028, 4, 1024, 0)
guard_ema_adam_row(1028, 4, 1024, 1)


# ------------------------------------------------------------------------------------------------------------------ faded blur of D's inputs
def blur_apply_row(S):
    """2 images under sigma = 10 (R = 30; at S = 8 most taps lie outside the image, S = 40 takes two tiles a side), the state's k and
    reserved words holding junk: sigma is the only word the kernel may read.  Against blur_np at the bound of tests/test_blur_gpu.py"""
    def run(ops, alloc):
        x = alloc.inp("x", blur_images(2, S))
        state = alloc.inp("state", blur_state_words(10.0, 0x12345678, 0x7FC00001, -7).view(np.float32))
        return dict(out=ops.blur_apply(x, state, out=alloc.out("out", (2, S, S, 3))))

    def check(res):
        assert np.abs(f64(res["out"]) - blur_np(blur_images(2, S), 10.0)).max() <= blur_bound(30, 1.0)

    row(f"blur-apply-2x{S}", ("lgblur_apply",), run, check, route="dblur_apply_kernel", exact_sizing=True)


def blur_init_step_row():
    """init(5) into a state that holds junk, then one step: k = 6, the reserved words zero"""
    def run(ops, alloc):
        tr = Trace(ops)
        state = ops.blur_init(5, out=alloc.out("state", (4,)))
        tr("init")
        ops.blur_step(state, 10.0, 3, 100)
        tr("step")
        return dict(state=state, _route=tr)

    def check(res):
        got = i32(res["state"]).tolist()
        assert got[0] == 6 and got[2:] == [0, 0]      # (sigma against the restatement: tests/test_blur_gpu.py)

    row("blur-init-step", ("lgblur_init", "lgblur_step"), run, check, route=("init=dblur_init_kernel", "step=dblur_step_kernel"),
        exact_sizing=True)


blur_apply_row(8)
blur_apply_row(40)
blur_init_step_row()
