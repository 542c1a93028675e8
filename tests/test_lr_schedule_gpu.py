"""Per-network learning rates and the device-side schedule on the device: lgsch_step against the host restatement
(config.lr_factor) at every edge of warm-up, decay and the counter's saturation; the two Adam passes that read their rate from device
memory against the existing ones, bit for bit, at the one-block, block-edge and grid-stride edges of a 4096 x 256 grid; (their memory
contract: the sched-* rows of tests/test_memory_contract_gpu.py); and
whole training steps: against a trainer whose rates are set on the host before every step, through replayed graphs, across a checkpoint,
with the keys at their defaults, with rates per network alone, with the weight average, and on two data-parallel ranks."""
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
from test_lr_schedule_cpu import KINDS, NS, RS, WS, settings  # noqa: E402
from test_step_gpu import dev_inputs, f32_round, load_weights, make_args, perturbed  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = dict(init_dim=2, conv_filter=(64, 32, 32, 32, 32), cond_dim=5, noise_dim=11, batch_size=3)
F32 = np.float32
RATES = dict(lr_g=2e-4, lr_d=5e-5, lr_adj=1.25e-3)      # distinct base rates
K_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def ops():
    from littlegan_amd import ops as _ops
    return _ops


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _np_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------- lgsch_step
def _counters(W, N):
    ks = [0, W - 1, W, W + 1, W + N - 1, W + N, W + N + 5, K_MAX - 1, K_MAX]
    return sorted({k for k in ks if k >= 0})


def _schedule_cases(kind):
    """[(settings, k)]: W in {0, 1, 3}, N in {1, 7}, r in {0, 0.1, 1}, the counter planted at every edge (constant has no N)"""
    out = []
    for W in WS:
        for N in ((None,) if kind == "constant" else NS):
            for r in RS:
                c = settings(kind, W=W, N=N, r=r, **RATES)
                out += [(c, k) for k in _counters(W, N or 1)]
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_schedule_step_against_the_host_restatement(ops, kind):
    from littlegan_amd import config
    cases = _schedule_cases(kind)
    assert len(cases) >= 6 * (9 if kind == "constant" else 18)
    states = torch.empty(len(cases), 8, dtype=torch.float32, device="cuda")       # rows are 32 bytes apart: each a state of its own
    for row, (c, k) in zip(states, cases):
        ops.sched_init(k, out=row)
    planted = states.cpu().view(torch.int32).numpy().copy()
    for row, (c, k) in zip(states, cases):
        ops.sched_step(row, c["kind"], c["warmup"], c["decay"], c["final_ratio"], c["lr_g"], c["lr_d"], c["lr_adj"])
    assert ops.last_kernel() == "sched_step_kernel"
    got_f = states.cpu().numpy()
    got = got_f.view(np.int32)
    inside = 0
    for i, (c, k) in enumerate(cases):
        tag = (kind, c["warmup"], c["decay"], c["final_ratio"], k)
        assert planted[i].tolist() == [k, 0, 0, 0, 0, 0, 0, 0], tag                # lgsch_init: the counter and seven zero words
        assert got[i, 0] == min(k + 1, K_MAX) and not got[i, 5:].any(), tag        # k + 1, saturating; the reserved words stay zero
        want = config.lr_factor(k, c)
        s = got_f[i, 1]
        W, N = c["warmup"], c["decay"]
        if kind == "cosine" and W < k < W + N:        # strictly inside the decay: the two fp64 cosines may differ in their last place
            inside += 1
            print(f"cosine W={W} N={N} r={c['final_ratio']:.3g} k={k}: device {s!r} host {want!r} ({int(got[i, 1]) - int(_np_bits([want])[0])} ulp)")
            assert abs(int(got[i, 1]) - int(_np_bits([want])[0])) <= 1, tag
        else:
            assert got[i, 1] == _np_bits([want])[0], (tag, s, want)
        rates = [F32(c[m]) * s for m in ("lr_g", "lr_d", "lr_adj")]                 # one fp32 multiply of the device's own s
        assert got[i, 2:5].tolist() == _np_bits(rates).tolist(), tag
    assert inside == (0 if kind != "cosine" else 3 * 3 * len([k for k in _counters(0, 7) if 0 < k < 7]))
    assert ops.sched_read(states[0]) == (int(got[0, 0]),) + tuple(float(x) for x in got_f[0, 1:5])


def test_consecutive_steps_walk_the_schedule(ops):
    """one state, advanced step by step (what a replayed graph does), with the settings of the whole-step tests"""
    from littlegan_amd import config
    c = settings("linear", W=2, N=6, r=0.0, **RATES)
    st = ops.sched_init(0)
    for k in range(12):
        ops.sched_step(st, c["kind"], c["warmup"], c["decay"], c["final_ratio"], c["lr_g"], c["lr_d"], c["lr_adj"])
        kk, s, g, d, a = ops.sched_read(st)
        assert kk == k + 1 and F32(s) == config.lr_factor(k, c) and (F32(g), F32(d), F32(a)) == config.lr_rates(k, c), k
    assert s == 0.0 and g == 0.0      # r = 0: the rates end at zero


# ---------------------------------------------------------------------------------------------------------------- the Adam variants
B1, B2, EPS = 0.5, 0.9, 1e-8
STEP_RATES = (1e-2, 3.3333334e-3, 7.7e-4)      # a different rate on each of the three steps


def _adam_data(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda scale: torch.randn(n, generator=g, device="cuda") * scale
    return dict(w=rnd(1.0), g=[rnd(1.0) for _ in STEP_RATES], m=rnd(0.1), v=rnd(0.1).abs(), ema=rnd(1.0))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1048576, 1048577])
def test_plain_adam_variant_is_bit_identical(ops, n):
    d = _adam_data(n, 11 + n % 97)
    for clip, gscale in ((0.5, 1.0), (0.0, 0.5)):
        runs = []
        for variant in (False, True):
            w, m, v = d["w"].clone(), d["m"].clone(), d["v"].clone()
            state = torch.tensor([B1, B2], dtype=torch.float32, device="cuda")
            for lr, g in zip(STEP_RATES, d["g"]):
                if variant:
                    ops.sched_clip_adam_update(w, g, m, v, state, torch.tensor([lr], dtype=torch.float32, device="cuda"), B1, B2, EPS, clip, gscale)
                    assert ops.last_kernel() == "clip_adam_lrp_kernel"
                else:
                    ops.clip_adam_update(w, g, m, v, state, lr, B1, B2, EPS, clip, gscale)
                ops.adam_advance(state, B1, B2)
            runs.append((w, m, v, state))
        assert all(torch.equal(_t(a), _t(b)) for a, b in zip(*runs)), (n, clip, gscale)
        assert not torch.equal(runs[0][0], d["w"])


def _t(x):
    return x.view(torch.int32)


@pytest.mark.parametrize("n", [4, 1024, 1028, 4194304, 4194308])
def test_ema_adam_variant_is_bit_identical(ops, n):
    d = _adam_data(n, 23 + n % 89)
    n4 = n // 4
    lo_i = (n4 // 3) * 4
    ranges = dict(empty=(lo_i, lo_i), interior=(lo_i, min(n, max(lo_i + 4, (2 * n4 // 3) * 4))), whole=(0, n))
    for rng_name, (lo, hi) in ranges.items():
        for clip in (0.5, 0.0):
            for gscale in (1.0, 0.5):
                runs = []
                for variant in (False, True):
                    w, m, v, ema = d["w"].clone(), d["m"].clone(), d["v"].clone(), d["ema"].clone()
                    state = torch.tensor([B1, B2], dtype=torch.float32, device="cuda")
                    count = torch.tensor([3], dtype=torch.int32, device="cuda")
                    for lr, g in zip(STEP_RATES, d["g"]):
                        if variant:
                            ops.sched_clip_adam_ema_update(w, g, m, v, ema, lo, hi, state, count, torch.tensor([lr], dtype=torch.float32, device="cuda"),
                                                           B1, B2, EPS, clip, gscale, 0.99)
                            assert ops.last_kernel() == "clip_adam_ema_lrp_kernel"
                        else:
                            ops.clip_adam_ema_update(w, g, m, v, ema, lo, hi, state, count, lr, B1, B2, EPS, clip, gscale, 0.99)
                        ops.adam_advance(state, B1, B2)
                        ops.ema_advance(count)
                    runs.append((w, m, v, ema, state))
                assert all(torch.equal(_t(a), _t(b)) for a, b in zip(*runs)), (n, rng_name, clip, gscale)
                assert not torch.equal(runs[0][3], d["ema"]) and (lo == hi) == torch.equal(runs[0][0], d["w"])


# ---------------------------------------------------------------------------------------------------------------- whole steps
SCHED_KW = dict(lr_schedule="linear", lr_warmup_steps=2, lr_decay_steps=6, **RATES)
STEPS = tuple(range(7, 15))      # 10 is a partition step; from 11 on the Adjuster trains


def _build(cfg, W, **kw):
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    args = make_args(cfg, "f32")
    for k, v in kw.items():
        setattr(args, k, v)
    decoder, encoder = Decoder(args), Encoder(args)
    g = Generator(args, decoder)
    d = Discriminator(args, encoder)
    tr = EagerTrainer(args, g, d, Adjuster(args, d, g), None)
    if W is not None:
        load_weights(tr, W)
    return tr


def _step_inputs(cfg, b):
    return f32_round(O.make_inputs(cfg, cfg.batch_size, seed=70 + b))


def _snapshot(tr):
    st = tr.store
    out = [st.flat.clone(), st.m.clone(), st.v.clone()] + [tr.opt_state[m].clone() for m in "GDA"]
    return out + ([st.ema.clone()] if st.ema is not None else [])


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(_t(x), _t(y)) for x, y in zip(a, b))


_EAGER = {}


def _eager_run(ema=False):
    """the eight scheduled steps on the eager path, once per module: -> (cfg, W, snapshots after each step, the trainer)"""
    if ema not in _EAGER:
        cfg = O.Cfg(**SMALL)
        W = perturbed(cfg, 6)
        tr = _build(cfg, W, **SCHED_KW, **(dict(ema_decay=0.99) if ema else {}))
        snaps = []
        for b in STEPS:
            tr.train_step_from_inputs(b, dev_inputs(_step_inputs(cfg, b)))
            snaps.append(_snapshot(tr))
        torch.cuda.synchronize()
        _EAGER[ema] = (cfg, W, snaps, tr)
    return _EAGER[ema]


def _against_host_set_rates(ops, monkeypatch, ema):
    from littlegan_amd import config
    with monkeypatch.context() as mp_:
        names = called(mp_, ops)
        cfg, W, snaps, tr = _eager_run(ema)
        names = list(names)
    assert tr.lr_state is not None and tr.lr_sched["device"] and tr.lr_now().shape == (3,)
    assert cfg.partition_interval == 4 and tr.step_kind(10)[0] >= 0 and not tr.step_kind(10)[1] and tr.step_kind(11) == (-1, True, False)
    host = _build(cfg, W, **(dict(ema_decay=0.99) if ema else {}))
    assert host.lr_state is None
    c = tr.lr_sched
    seen = []
    for k, b in enumerate(STEPS):
        rates = config.lr_rates(k, c)
        seen.append(float(config.lr_factor(k, c)))
        host.opt_cfg = {m: (float(r),) + host.opt_cfg[m][1:] for m, r in zip("GDA", rates)}
        host.train_step_from_inputs(b, dev_inputs(_step_inputs(cfg, b)))
        assert _same(_snapshot(host), snaps[k]), (b, k)
    assert seen == [0.5, 1.0] + [float(F32(1.0 - t / 6.0)) for t in range(6)]       # warm-up, then down the line: every step another rate
    k, s, g, d, a = ops.sched_read(tr.lr_state)
    assert k == len(STEPS) and (F32(s),) + (F32(g), F32(d), F32(a)) == (config.lr_factor(7, c),) + config.lr_rates(7, c)
    assert torch.equal(tr.lr_now().cpu(), torch.tensor([g, d, a], dtype=torch.float32))
    return names


def test_scheduled_steps_equal_host_set_rates(ops, monkeypatch):
    """(a) eight eager steps under the device-side schedule against a trainer on the scalar path whose rates the host sets before each
    step from config.lr_rates: every weight, Adam slot and beta power bit for bit."""
    names = _against_host_set_rates(ops, monkeypatch, ema=False)
    if names:       # (empty when another test of this module ran the shared steps first)
        assert names.count("lgsch_init") == 1 and names.count("lgsch_step") == len(STEPS) and "lg_clip_adam_update" not in names
        assert names.count("lgsch_clip_adam_update") == 2 * 4 + 3 * 4      # D and G on 7..10, all three from 11 on


def test_scheduled_steps_with_the_weight_average(ops, monkeypatch):
    """(f) with ema_decay the fused variant is taken, and (a) holds for the weights, the slots and the average"""
    names = _against_host_set_rates(ops, monkeypatch, ema=True)
    if names:
        assert names.count("lgsch_clip_adam_ema_update") == 3 * len(STEPS) and names.count("lgsch_step") == len(STEPS)
        assert "lg_clip_adam_ema_update" not in names and "lg_clip_adam_update" not in names and "lgsch_clip_adam_update" not in names


def test_graph_replay_walks_the_schedule(ops, monkeypatch):
    """(b) the same steps through graph_step: replays of a captured graph read the rates the replayed lgsch_step writes"""
    cfg, W, snaps, _ = _eager_run()
    tg = _build(cfg, W, **SCHED_KW)
    kinds = [tg.step_kind(b) for b in STEPS]
    for k, b in enumerate(STEPS):
        with monkeypatch.context() as mp_:
            names = called(mp_, ops)
            tg.graph_step(b, dev_inputs(_step_inputs(cfg, b)))
            torch.cuda.synchronize()
        assert not names or names[0] == "lgsch_step", (b, names[:3])      # the step's first launch (a replay fetches nothing)
        assert bool(names) == (kinds.index(kinds[k]) == k or kinds[:k].count(kinds[k]) == 1), (b, len(names))
        assert _same(_snapshot(tg), snaps[k]), (b, k)
    assert len(tg._graphs) == 2 and max(kinds.count(k) for k in set(kinds)) >= 3      # both repeated kinds were replayed
    assert ops.sched_read(tg.lr_state)[0] == len(STEPS)


def test_resume_continues_the_schedule(ops, tmp_path):
    """(c) save after four steps, load into a fresh trainer, four more: the bits of the uninterrupted run"""
    cfg, W, snaps, _ = _eager_run()
    first = _build(cfg, W, **SCHED_KW, result_dir=str(tmp_path))
    for b in STEPS[:4]:
        first.train_step_from_inputs(b, dev_inputs(_step_inputs(cfg, b)))
    assert first.checkpoint_state()["lr_sched_state"] == 4
    path = first.save_checkpoint("4")
    fresh = _build(cfg, None, **SCHED_KW, result_dir=str(tmp_path))
    assert ops.sched_read(fresh.lr_state) == (0, 0.0, 0.0, 0.0, 0.0)
    fresh.load_checkpoint(path)
    assert ops.sched_read(fresh.lr_state)[0] == 4
    for k, b in list(enumerate(STEPS))[4:]:
        fresh.train_step_from_inputs(b, dev_inputs(_step_inputs(cfg, b)))
        assert _same(_snapshot(fresh), snaps[k]), (b, k)
    # a counter that is no counter is refused before anything is loaded; a checkpoint without one starts at k = 0
    ck = torch.load(path, map_location="cpu", weights_only=True)
    before = _snapshot(fresh)
    for bad in (-1, 2 ** 31, 1.5, True, [4]):
        torch.save({**ck, "lr_sched_state": bad}, tmp_path / "bad.pt")
        with pytest.raises(ValueError, match="lr_sched_state"):
            fresh.load_checkpoint(str(tmp_path / "bad.pt"))
        assert _same(_snapshot(fresh), before) and ops.sched_read(fresh.lr_state)[0] == len(STEPS)
    torch.save({k: v for k, v in ck.items() if k != "lr_sched_state"}, tmp_path / "old.pt")
    fresh.load_checkpoint(str(tmp_path / "old.pt"))
    assert ops.sched_read(fresh.lr_state)[0] == 0 and _same(_snapshot(fresh), snaps[3])
    # a trainer that schedules nothing ignores the field
    plain = _build(cfg, None)
    plain.load_checkpoint(path)
    assert plain.lr_state is None and "lr_sched_state" not in plain.checkpoint_state()


def test_defaults_have_no_state_and_the_parents_bits(ops, monkeypatch):
    """(d) with the keys at their defaults: no state, no lgsch_* function, the step of a trainer that never heard of the keys"""
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 2)
    absent = _build(cfg, W)
    off = _build(cfg, W, lr_g=None, lr_d=None, lr_adj=None, lr_schedule="constant", lr_warmup_steps=0, lr_decay_steps=None, lr_final_ratio=0.0)
    assert not hasattr(absent.args, "lr_schedule") and absent.lr_state is None and off.lr_state is None and off.lr_now() is None
    seen = []
    for tr in (absent, off):
        with monkeypatch.context() as mp_:
            names = called(mp_, ops)
            for b in (1, 5, 12):
                tr.train_step_from_inputs(b, dev_inputs(_step_inputs(cfg, b)))
            torch.cuda.synchronize()
        seen.append(list(names))
    assert seen[0] == seen[1] and seen[0] and not [n for n in seen[0] if n.startswith("lgsch_")]
    assert _same(_snapshot(absent), _snapshot(off)) and torch.equal(absent.store.grad, off.store.grad)


def test_rates_per_network_alone(ops, monkeypatch):
    """(e) another lr_d moves D's weights and leaves G's first-step update bit for bit; the scalar path: no state, no lgsch_* function"""
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 2)
    base, other = _build(cfg, W), _build(cfg, W, lr_d=4 * cfg.lr)
    assert other.lr_state is None and other.opt_cfg["D"][0] == float(F32(4 * cfg.lr)) and other.opt_cfg["G"] == base.opt_cfg["G"]
    names = called(monkeypatch, ops)
    inp = dev_inputs(_step_inputs(cfg, 12))
    before = base.store.flat.clone()
    base.train_step_from_inputs(12, inp)
    other.train_step_from_inputs(12, inp)
    torch.cuda.synchronize()
    assert names and not [n for n in names if n.startswith("lgsch_")]
    for m, same in (("G", True), ("A", True), ("D", False)):
        s, e = base.store.model_range(m)
        assert torch.equal(base.store.flat[s:e], other.store.flat[s:e]) == same, m
        assert not torch.equal(base.store.flat[s:e], before[s:e]), m
    s, e = base.store.model_range("D")
    moved = (other.store.flat[s:e] - before[s:e]).abs().sum() / (base.store.flat[s:e] - before[s:e]).abs().sum()
    assert 3.5 < float(moved) < 4.5      # Adam's step is proportional to its rate


# ---------------------------------------------------------------------------------------------------------------- data parallel
DP_STEPS = (9, 10, 11)


def _dp_worker(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = O.Cfg(**DP_CFG)
        tr = _build(cfg, perturbed(cfg, 21), **SCHED_KW)
        assert tr.sync.enabled and tr.sync.world_size == world
        B = cfg.batch_size
        for b in DP_STEPS:
            full = f32_round(O.make_inputs(cfg, B * world, seed=300 + b))
            tr.train_step_from_inputs(b, dev_inputs({k: v[rank * B:(rank + 1) * B] for k, v in full.items()}))
        torch.cuda.synchronize()
        np.save(os.path.join(outdir, f"flat_{rank}.npy"), tr.store.flat.cpu().numpy())
        np.save(os.path.join(outdir, f"state_{rank}.npy"), tr.lr_state.cpu().view(torch.int32).numpy())
    finally:
        dist.destroy_process_group()


def test_two_ranks_walk_the_same_schedule(tmp_path):
    """every rank advances its own counter by the same launches: equal weights and equal states, without a collective"""
    from littlegan_amd import config
    world = 2
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    _join_all(procs, 600)
    flat = [np.load(tmp_path / f"flat_{r}.npy") for r in range(world)]
    state = [np.load(tmp_path / f"state_{r}.npy") for r in range(world)]
    assert np.array_equal(flat[0], flat[1]) and np.array_equal(state[0], state[1])
    c = settings("linear", W=2, N=6, r=0.0, **RATES)
    assert state[0][0] == len(DP_STEPS) and state[0][1] == _np_bits([config.lr_factor(len(DP_STEPS) - 1, c)])[0]
