"""Global-norm gradient clipping and the non-finite step guard on the device: the fp64 sum of squares at every edge of
its launch geometry (one group, one wave, one chunk, many chunks, the stride over chunks), exact on integer inputs and within the bound
of any fp64 summation on random ones, independent of the address; the record against the host restatement (config.grad_guard_restate);
the two Adam passes that read their scale and skip flag from the record against the existing ones, bit for bit (the memory contract
of every pointer-taking lgg_* entry point: the guard-* rows of tests/test_memory_contract_gpu.py, on this module's data); and whole
training steps: with a threshold nothing reaches, against a trainer whose gradients the test scales itself, with a
NaN planted in one gradient, through replayed graphs, across a checkpoint, with the weight average, under a schedule, on two ranks."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import np_oracle as O  # noqa: E402
from guards import called  # noqa: E402
from test_dp_gpu import CFG as DP_CFG, _free_port, _join_all  # noqa: E402
from test_grad_guard_cpu import CH, PMAX  # noqa: E402
from test_lr_schedule_gpu import B1, B2, EPS, SCHED_KW, SMALL, STEPS, _build, _same, _snapshot, _step_inputs, _t  # noqa: E402
from test_step_gpu import dev_inputs, f32_round, perturbed  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
I_MAX = 2 ** 31 - 1
NS = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, CH - 1, CH, CH + 1, 2 * CH + 7, 1024 * CH + 5]   # the last: blocks stride over chunks


@pytest.fixture(scope="module")
def ops():
    from littlegan_amd import ops as _ops
    return _ops


def _guard_names(fetched):
    """the lgg_ names among the ABI names guards.called recorded, in order"""
    return [n for n in fetched if n.startswith("lgg_")]


def _ulps(a, b):
    return abs(int(F32(a).view(np.int32)) - int(F32(b).view(np.int32)))


def _partials(ops, g):
    """the device's partials of g, as a fresh fp64 tensor of exactly P(n) elements"""
    p = torch.full((ops.guard_partials_count(g.numel()),), float("nan"), dtype=torch.float64, device="cuda")
    ops.guard_sumsq_partial(g, p)
    return p


def _index_sum(p):
    s = 0.0
    for x in p.cpu().tolist():
        s += x
    return s


def _record(ops, g, gscale, clip, skip, skipped0=0, nonfinite0=0):
    rec = ops.guard_init(skipped0, nonfinite0)
    assert ops.last_kernel() == "gg_init_kernel"
    assert rec.cpu().view(torch.int32).tolist() == [0, 0, 0, skipped0, nonfinite0, 0, 0, 0]
    ops.guard_finalise(_partials(ops, g), g.numel(), rec, gscale, clip, skip)
    assert ops.last_kernel() == "gg_finalise_kernel"
    return rec


def _misaligned(g, k):
    """the same values at an address 4 k bytes past a 16-byte boundary"""
    base = torch.empty(g.numel() + 4, dtype=torch.float32, device="cuda")
    view = base[k:k + g.numel()]
    view.copy_(g)
    assert view.data_ptr() % 16 == 4 * k and view.is_contiguous()
    return view


# ---------------------------------------------------------------------------------------------------------------- the reduction
@pytest.mark.parametrize("n", NS)
def test_sum_of_squares_is_exact_on_integers(ops, n):
    """integer values in [-8, 8]: every partial sum is an integer below 2^53, so S is the integer sum exactly, whatever the order; two
    launches give equal bits; a view of the same data misaligned by 4, 8 and 12 bytes gives the bits of the aligned one"""
    gen = torch.Generator(device="cuda").manual_seed(1000 + n % 991)
    g = torch.randint(-8, 9, (n,), generator=gen, device="cuda").to(torch.float32)
    want = int((g.to(torch.int64) ** 2).sum())
    assert g.data_ptr() % 16 == 0
    p1 = _partials(ops, g)
    assert ops.last_kernel() == "gg_sumsq_partial_kernel<vec>"
    p2 = _partials(ops, g)
    P = min(PMAX, -(-n // CH))
    assert p1.numel() == P == ops.guard_workspace_bytes(n) // 8 and torch.equal(p1.view(torch.int64), p2.view(torch.int64))
    S = ops.grad_sumsq(g)
    assert S == _index_sum(p1) == float(want) and float(p1.sum()) == float(want), (n, S, want)
    for k in (1, 2, 3):
        pk = _partials(ops, _misaligned(g, k))
        assert ops.last_kernel() == "gg_sumsq_partial_kernel<scalar>"
        assert torch.equal(pk.view(torch.int64), p1.view(torch.int64)), (n, k)


@pytest.mark.parametrize("scale", [1e-20, 1.0, 1e18])
@pytest.mark.parametrize("n", NS)
def test_sum_of_squares_against_fsum(ops, n, scale):
    """random normal inputs against math.fsum of the fp64 squares (each square is exact in fp64); 1e18 would overflow an fp32
    accumulation.  |S - S_ref| <= n 2^-52 S_ref: the bound of any fp64 summation of n positive terms, nothing measured in it.
    The same bits from a misaligned view."""
    gen = torch.Generator(device="cuda").manual_seed(2000 + n % 983)
    g = (torch.randn(n, generator=gen, device="cuda") * scale).contiguous()
    x = g.cpu().double()
    ref = math.fsum((x * x).tolist())
    S = ops.grad_sumsq(g)
    print(f"n={n} scale={scale:g}: S {S!r} fsum {ref!r} rel {abs(S - ref) / ref:.3e} bound {n * 2.0 ** -52:.3e}")
    assert math.isfinite(S) and ref > 0 and abs(S - ref) <= n * 2.0 ** -52 * ref, (n, scale, S, ref)
    assert torch.equal(_partials(ops, _misaligned(g, 1 + n % 3)).view(torch.int64), _partials(ops, g).view(torch.int64))


def _c_from(N, clip, bad):
    """c of the definition from a given fp32 N"""
    if clip == 0 or bad:
        return F32(1.0)
    with np.errstate(over="ignore"):
        q = F32(clip) / (F32(N) + F32(1e-6))
    return q if q < F32(1.0) else F32(1.0)


@pytest.mark.parametrize("n", [1, 5, 257, CH + 1, 2 * CH + 7])
def test_record_against_the_restatement(ops, n):
    from littlegan_amd import config
    gen = torch.Generator(device="cuda").manual_seed(3000 + n)
    g = torch.randn(n, generator=gen, device="cuda")
    host = g.cpu().numpy()
    norm = float(np.sqrt(np.sum(host.astype(np.float64) ** 2)))
    seen = set()
    for gscale in (1.0, 0.5, 0.125):
        for clip in (0.0, 1e30, 0.5 * norm * gscale, 2.0 * norm * gscale, 1e-3):
            for skip in (0, 1):
                clip32 = float(F32(clip))
                rec = _record(ops, g, gscale, clip32, skip, 3, 7)
                r = ops.guard_read(rec)
                want = config.grad_guard_restate(host, gscale, clip32, skip)
                assert _ulps(r["N"], want["N"]) <= 1, (n, gscale, r["N"], want["N"])           # N: 1 fp32 ulp (the order of the additions)
                from_S = config.grad_guard_restate(None, gscale, clip32, skip, sumsq=ops.grad_sumsq(g))
                assert F32(r["N"]).view(np.int32) == from_S["N"].view(np.int32)               # ... and bit for bit from the device's own S
                c = _c_from(r["N"], clip32, False)                                             # c, eff, counters: from the device's own N
                words = rec.cpu().view(torch.int32).tolist()
                assert words[5] == int(c.view(np.int32)) and words[1] == int((F32(gscale) * c).view(np.int32)), (n, gscale, clip)
                assert words[2:5] == [0, 3, 7] and words[6:] == [0, 0]
                seen.add(bool(c < 1))
    assert seen == {True, False}


POISON = (float("nan"), float("inf"), float("-inf"))


def test_a_non_finite_element_is_found_wherever_it_is(ops):
    n = 2 * CH + 7
    gen = torch.Generator(device="cuda").manual_seed(41)
    clean = torch.randn(n, generator=gen, device="cuda")
    for at in (0, n - 1, CH - 1, CH, 2 * CH - 1, 2 * CH):        # the ends, both sides of both chunk edges
        for poison in POISON:
            g = clean.clone()
            g[at] = poison
            for skip in (0, 1):
                for gscale in (1.0, 0.25):
                    rec = _record(ops, g, gscale, 1e-3, skip, 3, 7)
                    r = ops.guard_read(rec)
                    assert not math.isfinite(r["N"]) and r["c"] == 1.0 and F32(r["eff"]).view(np.int32) == F32(gscale).view(np.int32)
                    assert (r["skip_now"], r["skipped"], r["nonfinite"]) == (skip, 3 + skip, 8), (at, poison, skip, r)
    # a second bad step on the same record counts again; a clean one counts nothing and clears skip_now
    g = clean.clone()
    g[5] = float("nan")
    rec = ops.guard_init(0, 0)
    for k in range(3):
        ops.guard_finalise(_partials(ops, g), n, rec, 1.0, 1.0, 1)
    assert ops.guard_read(rec)["skipped"] == 3 and ops.guard_read(rec)["nonfinite"] == 3 and ops.guard_read(rec)["skip_now"] == 1
    ops.guard_finalise(_partials(ops, clean), n, rec, 1.0, 1.0, 1)
    r = ops.guard_read(rec)
    assert (r["skip_now"], r["skipped"], r["nonfinite"]) == (0, 3, 3) and math.isfinite(r["N"]) and r["c"] < 1
    # +Inf and -Inf together, and the largest finite value everywhere (its squares stay far below the fp64 range: not bad)
    g = clean.clone()
    g[0], g[n - 1] = float("inf"), float("-inf")
    assert ops.guard_read(_record(ops, g, 1.0, 1.0, 1))["skip_now"] == 1
    big = torch.full((n,), float(np.finfo(F32).max), device="cuda")
    r = ops.guard_read(_record(ops, big, 1.0, 1.0, 1))
    assert (r["skip_now"], r["nonfinite"]) == (0, 0) and math.isinf(r["N"]) and r["c"] == 0.0 and r["eff"] == 0.0


def test_counters_saturate(ops):
    g = torch.ones(5, device="cuda")
    g[2] = float("nan")
    for skip, want in ((1, (I_MAX, I_MAX)), (0, (I_MAX - 1, I_MAX))):
        rec = _record(ops, g, 1.0, 1.0, skip, I_MAX if skip else I_MAX - 1, I_MAX)
        r = ops.guard_read(rec)
        assert (r["skipped"], r["nonfinite"]) == want and r["skip_now"] == skip
    rec = _record(ops, g, 1.0, 1.0, 1, I_MAX - 1, I_MAX - 1)
    assert (ops.guard_read(rec)["skipped"], ops.guard_read(rec)["nonfinite"]) == (I_MAX, I_MAX)


# ---------------------------------------------------------------------------------------------------------------- the Adam variants
STEP_RATES = (1e-2, 3.3333334e-3, 7.7e-4)      # a different rate on each of the three steps
_BETAS = [float(F32(B1)), float(F32(B2))]         # the beta powers before any advance, as fp32 holds them


def _rec_of(eff, skip_now):
    """a record {0, eff, skip_now, 0, 0, 1, 0, 0} the test writes itself"""
    w = np.zeros(8, np.float32)
    w[1], w[5] = eff, 1.0
    w.view(np.int32)[2] = skip_now
    return torch.from_numpy(w).cuda()


def _adam_data(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda scale: torch.randn(n, generator=g, device="cuda") * scale
    return dict(w=rnd(1.0), g=[rnd(1.0) for _ in STEP_RATES], m=rnd(0.1), v=rnd(0.1).abs(), ema=rnd(1.0))


def _lr(lr):
    return torch.tensor([lr], dtype=torch.float32, device="cuda")


def _plain_runs(ops, d, clip, gscale, eff, skip_now=0):
    """three steps with the advance between them: the existing function at `gscale`, the variant with a record holding `eff`"""
    runs = []
    for variant in (False, True):
        w, m, v = d["w"].clone(), d["m"].clone(), d["v"].clone()
        state = torch.tensor([B1, B2], dtype=torch.float32, device="cuda")
        rec = _rec_of(eff, skip_now)
        for lr, g in zip(STEP_RATES, d["g"]):
            if variant:
                ops.guard_clip_adam_update(w, g, m, v, state, _lr(lr), rec, B1, B2, EPS, clip)
                assert ops.last_kernel() == "clip_adam_gg_kernel"
                ops.guard_adam_advance(state, rec, B1, B2)
                assert ops.last_kernel() == "adam_advance_gg_kernel"
            else:
                ops.clip_adam_update(w, g, m, v, state, lr, B1, B2, EPS, clip, gscale)
                ops.adam_advance(state, B1, B2)
        runs.append((w, m, v, state))
    return runs


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1048577])
def test_plain_adam_variant_is_bit_identical(ops, n):
    d = _adam_data(n, 11 + n % 97)
    for clip in (0.5, 0.0):
        for gscale in (1.0, 0.5):
            runs = _plain_runs(ops, d, clip, gscale, gscale)                      # eff == gscale
            assert all(torch.equal(_t(a), _t(b)) for a, b in zip(*runs)), (n, clip, gscale)
            assert not torch.equal(runs[0][0], d["w"])
            eff = float(F32(gscale) * F32(0.3713))                               # eff = gscale * c, c < 1: the function at that product
            runs = _plain_runs(ops, d, clip, eff, eff)
            assert all(torch.equal(_t(a), _t(b)) for a, b in zip(*runs)), (n, clip, gscale, "c < 1")
        # skip_now: nothing is touched, the beta powers stay
        runs = _plain_runs(ops, d, clip, 1.0, 1.0, skip_now=1)
        w, m, v, state = runs[1]
        assert torch.equal(_t(w), _t(d["w"])) and torch.equal(_t(m), _t(d["m"])) and torch.equal(_t(v), _t(d["v"]))
        assert state.tolist() == _BETAS and not torch.equal(runs[0][0], d["w"])


@pytest.mark.parametrize("n", [4, 1024, 1028, 4194308])
def test_ema_adam_variant_is_bit_identical(ops, n):
    d = _adam_data(n, 23 + n % 89)
    n4 = n // 4
    lo_i = (n4 // 3) * 4
    ranges = dict(empty=(lo_i, lo_i), interior=(lo_i, min(n, max(lo_i + 4, (2 * n4 // 3) * 4))), whole=(0, n))

    def run(variant, lo, hi, clip, gscale, eff, skip_now=0):
        w, m, v, ema = d["w"].clone(), d["m"].clone(), d["v"].clone(), d["ema"].clone()
        state = torch.tensor([B1, B2], dtype=torch.float32, device="cuda")
        count = torch.tensor([3], dtype=torch.int32, device="cuda")
        rec = _rec_of(eff, skip_now)
        for lr, g in zip(STEP_RATES, d["g"]):
            if variant:
                ops.guard_clip_adam_ema_update(w, g, m, v, ema, lo, hi, state, count, _lr(lr), rec, B1, B2, EPS, clip, 0.99)
                assert ops.last_kernel() == "clip_adam_ema_gg_kernel"
                ops.guard_adam_advance(state, rec, B1, B2)
            else:
                ops.clip_adam_ema_update(w, g, m, v, ema, lo, hi, state, count, lr, B1, B2, EPS, clip, gscale, 0.99)
                if lo != hi or not skip_now:
                    ops.adam_advance(state, B1, B2)
            ops.ema_advance(count)
        return w, m, v, ema, state

    for rng_name, (lo, hi) in ranges.items():
        for clip in (0.5, 0.0):
            for gscale, eff in ((1.0, 1.0), (0.5, 0.5), (None, float(F32(0.5) * F32(0.3713)))):
                a, b = run(False, lo, hi, clip, eff if gscale is None else gscale, eff), run(True, lo, hi, clip, None, eff)
                assert all(torch.equal(_t(x), _t(y)) for x, y in zip(a, b)), (n, rng_name, clip, gscale)
                assert not torch.equal(a[3], d["ema"]) and (lo == hi) == torch.equal(a[0], d["w"])
        # skip_now: w, m, v and the beta powers stay; the average is that of the twin with lo == hi
        got = run(True, lo, hi, 0.5, None, 1.0, skip_now=1)
        twin = run(False, lo, lo, 0.5, 1.0, 1.0, skip_now=1)
        assert all(torch.equal(_t(x), _t(y)) for x, y in zip(got, twin)), (n, rng_name, "skip")
        assert torch.equal(_t(got[0]), _t(d["w"])) and torch.equal(_t(got[1]), _t(d["m"])) and torch.equal(_t(got[2]), _t(d["v"]))
        assert got[4].tolist() == _BETAS and not torch.equal(got[3], d["ema"])


@pytest.mark.parametrize("n", [257, 1028])
def test_a_bad_gradient_without_skip_is_the_step_as_it_is(ops, n):
    """bad and skip = 0: the record the device itself writes (eff == gscale, skip_now = 0) and the existing function's bits, NaNs included.
    Without the element-wise clip the NaN and the Inf reach the weights; with it clip_adam_element's fminf(fmaxf(g, -clip), clip) turns
    a NaN into -clip and an Inf into +clip, as it always did: the weights stay finite (and wrong), which only the counter shows."""
    d = _adam_data(n, 5 + n)
    g = d["g"][0].clone()
    g[n // 2] = float("nan")
    g[1] = float("inf")
    for clip, poisoned in ((0.0, 2), (0.5, 0)):
        for gscale in (1.0, 0.5):
            rec = _record(ops, g, gscale, 1e-3, 0)
            r = ops.guard_read(rec)
            assert (r["skip_now"], r["skipped"], r["nonfinite"], r["c"]) == (0, 0, 1, 1.0)
            a = [d[k].clone() for k in ("w", "m", "v")] + [torch.tensor([B1, B2], dtype=torch.float32, device="cuda")]
            b = [t.clone() for t in a]
            ops.clip_adam_update(a[0], g, a[1], a[2], a[3], 1e-2, B1, B2, EPS, clip, gscale)
            ops.adam_advance(a[3], B1, B2)
            ops.guard_clip_adam_update(b[0], g, b[1], b[2], b[3], _lr(1e-2), rec, B1, B2, EPS, clip)
            ops.guard_adam_advance(b[3], rec, B1, B2)
            assert all(torch.equal(_t(x), _t(y)) for x, y in zip(a, b)) and a[3].tolist() != _BETAS
            assert int(torch.isnan(b[0]).sum()) == poisoned, (clip, gscale)
            if n % 4 == 0:
                ea, eb = d["ema"].clone(), d["ema"].clone()
                count = torch.tensor([2], dtype=torch.int32, device="cuda")
                a = [d[k].clone() for k in ("w", "m", "v")]
                b = [t.clone() for t in a]
                st = torch.tensor([B1, B2], dtype=torch.float32, device="cuda")
                ops.clip_adam_ema_update(a[0], g, a[1], a[2], ea, 0, n, st, count, 1e-2, B1, B2, EPS, clip, gscale, 0.99)
                ops.guard_clip_adam_ema_update(b[0], g, b[1], b[2], eb, 0, n, st, count, _lr(1e-2), rec, B1, B2, EPS, clip, 0.99)
                assert all(torch.equal(_t(x), _t(y)) for x, y in zip(a + [ea], b + [eb])) and int(torch.isnan(eb).sum()) == poisoned


# ---------------------------------------------------------------------------------------------------------------- memory contract
# (the guard-* rows of tests/test_memory_contract_gpu.py, which imports these two and _ulps, _c_from above)
def _rec_np(eff=0.0, skip_now=0, skipped=0, nonfinite=0):
    w = np.zeros(8, np.float32)
    w[1] = eff
    w.view(np.int32)[2:5] = (skip_now, skipped, nonfinite)
    return w


def _data(n, seed):
    r = np.random.default_rng(seed)
    return [r.standard_normal(n).astype(np.float32) for _ in range(4)] + [(r.random(n) * 0.1).astype(np.float32)]


# ---------------------------------------------------------------------------------------------------------------- whole steps
IDX = {"G": 3, "D": 4, "A": 5}      # the beta powers in a _snapshot


def _records(tr):
    return tr.guard_state.detach().cpu().numpy().copy().reshape(3, 8)      # rows G, D, A


def _run(tr, cfg, steps=STEPS, step=None):
    """-> (snapshots, records) after each step"""
    snaps, recs = [], []
    for b in steps:
        (step or tr.train_step_from_inputs)(b, dev_inputs(_step_inputs(cfg, b)))
        snaps.append(_snapshot(tr))
        if tr.guard is not None:
            recs.append(_records(tr))
    torch.cuda.synchronize()
    return snaps, recs


def _trained(tr, batch_no):
    from littlegan_amd.eager_trainer import train_weight_range
    run_adj = bool(tr.args.train_adj and batch_no > 10)
    return [(m, tr.store.model_range(m, *train_weight_range(tr.args, m, batch_no))) for m in tr.adam_order if m != "A" or run_adj]


def _wrap_scaling(tr, ops, clip, log):
    """the default path made to clip: before the optimizers run, the gradient range of each trained network is multiplied by the fp32 c
    that the restatement gives from the device's own S of that range (world 1: gscale = 1, eff = c, g * c is the kernel's product)"""
    from littlegan_amd import config
    orig = tr._apply_optimizers

    def wrapped(batch_no, run_adj):
        for m, (s, e) in _trained(tr, batch_no):
            r = config.grad_guard_restate(None, 1.0, clip, False, sumsq=ops.grad_sumsq(tr.store.grad[s:e]))
            tr.store.grad[s:e].mul_(float(r["c"]))
            log.append((batch_no, m, r))
        return orig(batch_no, run_adj)

    tr._apply_optimizers = wrapped
    return tr


def _wrap_nan(tr, at_step=9):
    """a NaN written into one element of D's gradient on one step, before the optimizers run: ordinary arithmetic, not a fault"""
    orig = tr._apply_optimizers

    def wrapped(batch_no, run_adj):
        if batch_no == at_step:
            s, e = dict(_trained(tr, batch_no))["D"]
            tr.store.grad[s + (e - s) // 3] = float("nan")
        return orig(batch_no, run_adj)

    tr._apply_optimizers = wrapped
    return tr


_CACHE = {}


def _base():
    """(cfg, W, the default trainer's snapshots, the records of the run that clips nothing): once per module"""
    if "base" not in _CACHE:
        cfg = O.Cfg(**SMALL)
        W = perturbed(cfg, 6)
        default_snaps, _ = _run(_build(cfg, W), cfg)
        tr = _build(cfg, W, clip_norm=1e30, skip_nonfinite=True)
        snaps, recs = _run(tr, cfg)
        _CACHE["base"] = (cfg, W, default_snaps, snaps, recs, tr)
    return _CACHE["base"]


def _clip():
    """a threshold between D's and G's norm of the first step"""
    recs = _base()[4]
    nG, nD = float(recs[0][0, 0]), float(recs[0][1, 0])
    assert nG > 0 and nD > 0 and nG != nD
    return float(F32(math.sqrt(nG * nD)))


def _clipped(ema=False):
    """the eight steps under clip_norm = _clip() with skip_nonfinite, eager: (snapshots, records, trainer), once per module"""
    key = ("clipped", ema)
    if key not in _CACHE:
        cfg, W = _base()[:2]
        tr = _build(cfg, W, clip_norm=_clip(), skip_nonfinite=True, **(dict(ema_decay=0.99) if ema else {}))
        _CACHE[key] = _run(tr, cfg) + (tr,)
    return _CACHE[key]


def test_a_threshold_nothing_reaches_is_the_default_step(ops, monkeypatch):
    """(a) clip_norm = 1e30 with skip_nonfinite: every weight, Adam slot and beta power of eight steps as with the keys at their defaults"""
    with monkeypatch.context() as mp_:
        fetched = called(mp_, ops)
        cfg, W, default_snaps, snaps, recs, tr = _base()
        names = _guard_names(fetched)
    assert tr.guard == {"clip_norm": float(F32(1e30)), "skip": True} and tr.grad_norm_now().shape == (3,)
    assert cfg.partition_interval == 4 and tr.step_kind(10)[0] >= 0 and not tr.step_kind(10)[1] and tr.step_kind(11) == (-1, True, False)
    for k, b in enumerate(STEPS):
        assert _same(snaps[k], default_snaps[k]), (b, k)
        rows = recs[k].view(np.int32)
        for i, m in enumerate("GDA"):
            if m == "A" and b <= 10:
                assert not rows[i].any()                                  # the Adjuster has not trained yet: the record as lgg_init left it
                continue
            N, eff, c = recs[k][i, 0], recs[k][i, 1], recs[k][i, 5]
            assert np.isfinite(N) and N > 0 and c == 1.0 and eff == 1.0 and rows[i, 2:5].tolist() == [0, 0, 0], (b, m)
    assert tr.guard_counts() == {m: (0, 0) for m in "GDA"}
    assert torch.equal(tr.grad_norm_now().cpu(), torch.from_numpy(recs[-1][:, 0].copy()))
    assert len({float(r[1, 0]) for r in recs}) == len(STEPS)              # D's norm: another one on every step
    if names:       # (empty when another test of this module ran the shared steps first)
        per_net = 2 * 4 + 3 * 4                                           # D and G on 7..10, all three from 11 on
        assert names.count("lgg_init") == 3
        for fn in ("lgg_sumsq_partial", "lgg_finalise", "lgg_clip_adam_update", "lgg_adam_advance"):
            assert names.count(fn) == per_net, (fn, names.count(fn))
        names = [x for x in names if x != "lgg_workspace_bytes"]           # (the wrapper of lgg_finalise asks it for the size it checks)
        at = names.index("lgg_sumsq_partial")
        assert names[at:at + 4] == ["lgg_sumsq_partial", "lgg_finalise", "lgg_clip_adam_update", "lgg_adam_advance"]


def test_clipping_equals_gradients_scaled_by_the_test(ops):
    """(b) a threshold between D's and G's first norm: bit-identical to a default-path trainer whose gradients the test multiplies by c"""
    cfg, W = _base()[:2]
    snaps, recs, tr = _clipped()
    log = []
    ref = _wrap_scaling(_build(cfg, W), ops, _clip(), log)
    assert ref.guard is None
    for k, b in enumerate(STEPS):
        ref.train_step_from_inputs(b, dev_inputs(_step_inputs(cfg, b)))
        assert _same(_snapshot(ref), snaps[k]), (b, k)
    cs = [float(r["c"]) for _, _, r in log]
    assert any(c < 1 for c in cs) and any(c == 1 for c in cs), cs       # both sides of the threshold occur
    for b, m, r in log:      # the device's record of that step holds the same N, c and eff
        row = recs[STEPS.index(b)]["GDA".index(m)]
        assert row[0] == r["N"] and row[5] == r["c"] and row[1] == r["eff"], (b, m, row, r)
    assert tr.guard_counts() == {m: (0, 0) for m in "GDA"}


def _nan_run(skip, **kw):
    key = ("nan", skip, tuple(sorted(kw.items())))
    if key not in _CACHE:
        cfg, W = _base()[:2]
        tr = _wrap_nan(_build(cfg, W, clip_norm=_clip(), skip_nonfinite=skip, **kw))
        _CACHE[key] = _run(tr, cfg) + (tr,)
    return _CACHE[key]


def _part(snap, tr, m):
    s, e = tr.store.model_range(m)
    return [snap[0][s:e], snap[1][s:e], snap[2][s:e], snap[IDX[m]]]


def test_a_nan_gradient_skips_that_network_alone(ops):
    """(c) a NaN in D's gradient on step 9: D is left exactly as it was, G's update is the one of the run without the NaN, the event is
    counted, and the run goes on finite.  Without skip_nonfinite the step is today's, shown once for each of its two forms: with D's
    element-wise clip off (use_clip false) D's weights hold NaN from then on; with it on, as in this configuration, clip_adam_element's
    fminf(fmaxf(g, -clip), clip) has always turned a NaN into -clip_range, so D's weights stay finite and take a wrong step, which the
    non-finite counter alone shows."""
    clean = _clipped()[0]
    snaps, recs, tr = _nan_run(True)
    k = STEPS.index(9)
    assert _same(snaps[k - 1], clean[k - 1])
    assert _same(_part(snaps[k], tr, "D"), _part(snaps[k - 1], tr, "D"))                 # w, m, v, beta powers: untouched
    assert _same(_part(snaps[k], tr, "G"), _part(clean[k], tr, "G")) and not _same(_part(snaps[k], tr, "G"), _part(snaps[k - 1], tr, "G"))
    rows = recs[k].view(np.int32)
    assert rows[1, 2:5].tolist() == [1, 1, 1] and rows[0, 2:5].tolist() == [0, 0, 0] and not np.isfinite(recs[k][1, 0])
    for j in range(k + 1, len(STEPS)):
        rows = recs[j].view(np.int32)
        assert rows[:, 2].tolist() == [0, 0, 0] and rows[1, 3:5].tolist() == [1, 1] and np.isfinite(recs[j][:, 0]).all(), STEPS[j]
        assert all(torch.isfinite(t).all() for t in snaps[j][:3]) and not _same(_part(snaps[j], tr, "D"), _part(snaps[j - 1], tr, "D"))
    assert tr.guard_counts() == {"G": (0, 0), "D": (1, 1), "A": (0, 0)}
    # skip_nonfinite off, no element-wise clip on D: the NaN reaches m, v and the weight, for good
    snaps0, recs0, tr0 = _nan_run(False, use_clip=False)
    s, e = tr0.store.model_range("D")
    assert not torch.isnan(snaps0[k - 1][0]).any() and torch.isnan(snaps0[k][0][s:e]).any() and torch.isnan(snaps0[-1][0][s:e]).any()
    assert tr0.guard_counts()["D"][0] == 0 and tr0.guard_counts()["D"][1] >= 1 and tr0.guard_counts()["G"][0] == 0
    # skip_nonfinite off, D's element-wise clip on: the poisoned element moved as under a gradient of -clip_range; counted, not skipped
    snaps1, recs1, tr1 = _nan_run(False)
    assert all(torch.isfinite(t).all() for snap in snaps1 for t in snap[:3])
    assert _same(snaps1[k - 1], clean[k - 1]) and not _same(_part(snaps1[k], tr1, "D"), _part(clean[k], tr1, "D"))
    assert not _same(_part(snaps1[k], tr1, "D"), _part(snaps1[k - 1], tr1, "D")) and _same(_part(snaps1[k], tr1, "G"), _part(clean[k], tr1, "G"))
    assert recs1[k].view(np.int32)[1, 2:5].tolist() == [0, 0, 1] and recs1[k][1, 1] == 1.0 and recs1[k][1, 5] == 1.0
    assert tr1.guard_counts() == {"G": (0, 0), "D": (0, 1), "A": (0, 0)}


def test_graph_replay_clips_by_its_own_gradient(ops, monkeypatch):
    """(d) the clipped steps through graph_step: bit-identical to eager; the norms differ from step to step, so the record is live"""
    cfg, W = _base()[:2]
    snaps, recs, _ = _clipped()
    tg = _build(cfg, W, clip_norm=_clip(), skip_nonfinite=True)
    kinds = [tg.step_kind(b) for b in STEPS]
    replayed = []
    for k, b in enumerate(STEPS):
        with monkeypatch.context() as mp_:
            fetched = called(mp_, ops)
            tg.graph_step(b, dev_inputs(_step_inputs(cfg, b)))
            torch.cuda.synchronize()
        names = _guard_names(fetched)
        assert bool(names) == (kinds.index(kinds[k]) == k or kinds[:k].count(kinds[k]) == 1), (b, len(names))   # a replay fetches nothing
        if not names:
            replayed.append(k)
        assert _same(_snapshot(tg), snaps[k]), (b, k)
        assert np.array_equal(_records(tg).view(np.int32), recs[k].view(np.int32)), (b, k)
    assert len(tg._graphs) == 2 and len(replayed) >= 2
    assert len({float(recs[k][1, 0]) for k in replayed}) == len(replayed)      # D's norm of every replayed step is its own


def test_resume_restores_the_counters(ops, tmp_path):
    """(e) save after four steps (a skip planted on the third), load into a fresh trainer, four more: the uninterrupted run's bits"""
    cfg, W = _base()[:2]
    snaps, recs, _ = _nan_run(True)
    kw = dict(clip_norm=_clip(), skip_nonfinite=True, result_dir=str(tmp_path))
    first = _wrap_nan(_build(cfg, W, **kw))
    _run(first, cfg, STEPS[:4])
    assert first.checkpoint_state()["grad_guard_state"] == [0, 0, 1, 1, 0, 0]
    path = first.save_checkpoint("4")
    fresh = _build(cfg, None, **kw)
    assert fresh.guard_counts() == {m: (0, 0) for m in "GDA"}
    fresh.load_checkpoint(path)
    assert fresh.guard_counts() == {"G": (0, 0), "D": (1, 1), "A": (0, 0)}
    for k, b in list(enumerate(STEPS))[4:]:
        fresh.train_step_from_inputs(b, dev_inputs(_step_inputs(cfg, b)))
        assert _same(_snapshot(fresh), snaps[k]), (b, k)
    assert np.array_equal(_records(fresh).view(np.int32), recs[-1].view(np.int32))
    # a field that is not six counters is refused before anything is loaded; a checkpoint without it starts at zero
    ck = torch.load(path, map_location="cpu", weights_only=True)
    before, counts = _snapshot(fresh), fresh.guard_counts()
    for bad in ([0, 0, 1, 1, 0], [0, 0, 2, 1, 0, 0], [0, 0, -1, 1, 0, 0], [0, 0, 1, 2 ** 31, 0, 0], [0, 0, 1.0, 1, 0, 0], [True, 1, 0, 0, 0, 0], 3):
        torch.save({**ck, "grad_guard_state": bad}, tmp_path / "bad.pt")
        with pytest.raises(ValueError, match="grad_guard_state"):
            fresh.load_checkpoint(str(tmp_path / "bad.pt"))
        assert _same(_snapshot(fresh), before) and fresh.guard_counts() == counts
    torch.save({k: v for k, v in ck.items() if k != "grad_guard_state"}, tmp_path / "old.pt")
    fresh.load_checkpoint(str(tmp_path / "old.pt"))
    assert fresh.guard_counts() == {m: (0, 0) for m in "GDA"} and _same(_snapshot(fresh), snaps[3])
    # a trainer that guards nothing ignores the field
    plain = _build(cfg, None)
    plain.load_checkpoint(path)
    assert plain.guard is None and "grad_guard_state" not in plain.checkpoint_state()


def test_clipping_with_the_weight_average(ops, monkeypatch):
    """(f) with ema_decay the fused variant is taken, and (b) holds for the weights, the slots and the average"""
    cfg, W = _base()[:2]
    with monkeypatch.context() as mp_:
        fetched = called(mp_, ops)
        snaps, recs, tr = _clipped(ema=True)
        names = _guard_names(fetched)
    assert names.count("lgg_clip_adam_ema_update") == 2 * 4 + 3 * 4 and "lgg_clip_adam_update" not in names
    assert tr.store.ema is not None and len(snaps[0]) == 7
    ref = _wrap_scaling(_build(cfg, W, ema_decay=0.99), ops, _clip(), [])
    for k, b in enumerate(STEPS):
        ref.train_step_from_inputs(b, dev_inputs(_step_inputs(cfg, b)))
        assert _same(_snapshot(ref), snaps[k]), (b, k)
    # a skipped network under the average: its weights stay, its average still moves towards them
    skipped = _wrap_nan(_build(cfg, W, clip_norm=_clip(), skip_nonfinite=True, ema_decay=0.99))
    s_snaps, _ = _run(skipped, cfg, STEPS[:3])
    s, e = skipped.store.model_range("D")
    assert _same(_part(s_snaps[2], skipped, "D"), _part(s_snaps[1], skipped, "D")) and not torch.equal(s_snaps[2][6][s:e], s_snaps[1][6][s:e])
    assert skipped.guard_counts()["D"] == (1, 1) and int(skipped.store.ema_updates) == 3


def test_clipping_under_a_schedule(ops):
    """(f) with lr_schedule linear the rate pointer is the schedule's, and (b) holds against host-set rates"""
    from littlegan_amd import config
    cfg, W = _base()[:2]
    tr = _build(cfg, W, clip_norm=_clip(), skip_nonfinite=True, **SCHED_KW)
    assert tr.lr_state is not None and tr._guard_lr is None
    snaps, _ = _run(tr, cfg)
    host = _wrap_scaling(_build(cfg, W), ops, _clip(), [])
    for k, b in enumerate(STEPS):
        host.opt_cfg = {m: (float(r),) + host.opt_cfg[m][1:] for m, r in zip("GDA", config.lr_rates(k, tr.lr_sched))}
        host.train_step_from_inputs(b, dev_inputs(_step_inputs(cfg, b)))
        assert _same(_snapshot(host), snaps[k]), (b, k)


# ---------------------------------------------------------------------------------------------------------------- data parallel
DP_STEPS = (9, 10, 11)


def _dp_worker(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = O.Cfg(**DP_CFG)
        tr = _build(cfg, perturbed(cfg, 21), clip_norm=0.05, skip_nonfinite=True)
        assert tr.sync.enabled and tr.sync.world_size == world
        B = cfg.batch_size
        for b in DP_STEPS:
            full = f32_round(O.make_inputs(cfg, B * world, seed=300 + b))
            tr.train_step_from_inputs(b, dev_inputs({k: v[rank * B:(rank + 1) * B] for k, v in full.items()}))
        torch.cuda.synchronize()
        np.save(os.path.join(outdir, f"flat_{rank}.npy"), tr.store.flat.cpu().numpy())
        np.save(os.path.join(outdir, f"rec_{rank}.npy"), tr.guard_state.cpu().view(torch.int32).numpy())
    finally:
        dist.destroy_process_group()


def test_two_ranks_compute_the_same_record(tmp_path):
    """(g) the norm is that of the all-reduced gradient: every rank computes the same record from the same bits, without a collective"""
    world = 2
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    _join_all(procs, 600)
    flat = [np.load(tmp_path / f"flat_{r}.npy") for r in range(world)]
    rec = [np.load(tmp_path / f"rec_{r}.npy") for r in range(world)]
    assert np.array_equal(flat[0], flat[1]) and np.array_equal(rec[0], rec[1]) and np.isfinite(flat[0]).all()
    words = rec[0].reshape(3, 8)
    f = words.view(np.float32)
    assert (f[:, 0] > 0).all() and not words[:, 2:5].any()                              # three finite norms, nothing skipped
    assert all(f[i, 1] == F32(0.5) * f[i, 5] for i in range(3)) and (f[:, 5] <= 1).all()   # eff = gscale * c with gscale = 1 / 2
