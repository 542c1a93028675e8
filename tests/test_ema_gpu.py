"""Weight average for sampling on the GPU: the fused Adam + average kernel against the existing Adam kernel (bit for
bit) and the float64 restatement of tests/test_ema_cpu.py, the in-place swap, whole training steps with the average on and off,
graph replay, sampling through `ema_weights()`, checkpoints and two data-parallel ranks.

Tolerance of one average (not a measurement): the kernel forms ema - w, multiplies by 1 - d_t and subtracts from ema; each of those
roundings, and that of 1 - d_t, is at most half an ulp of a term no larger than 2 max(|ema|, |w|):
  |ema_kernel - ema_f64| <= 8 * 2^-24 * max(|ema_prev|, |w|)   elementwise,
the reference being the restatement applied to the previous average and the DEVICE's weights after the step.  Iterated over t steps
from the device's weights the bound is t times that (an average contracts earlier errors: d_t <= 1), against the running maximum of
the magnitudes seen."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # the spawned ranks import this module by name too
from oracle import np_oracle as O  # noqa: E402
from test_dropout_gpu import SMALL  # noqa: E402
from test_ema_cpu import ema_decay_at, ema_update  # noqa: E402
from test_step_gpu import dev_inputs, f32_round, load_weights, make_args, perturbed  # noqa: E402

pytestmark = pytest.mark.gpu

BOUND = 8 * 2.0 ** -24
DECAY = 0.9
BATCHES = [1, 5, 10, 11, 15, 12]   # a full step without the Adjuster, the partition groups 1, 2, (with the Adjuster) 0, full steps with it
ADAM = dict(lr=1e-2, b1=0.5, b2=0.9, eps=1e-8, clip=0.5, gscale=0.5)


@pytest.fixture(scope="module")
def ops():
    from littlegan_amd import ops as _ops
    return _ops


def _f64(t):
    return t.detach().cpu().double().numpy()


# ---------------------------------------------------------------------------------------------------------------- 1: the kernel
_CASE_DATA = {}


def _case_data(n):
    """The random arrays of size n, drawn once per size and left unchanged (every case clones what it writes to)."""
    if n not in _CASE_DATA:
        gen = torch.Generator().manual_seed(n)
        w, g, m, ema = (torch.randn(n, generator=gen) for _ in range(4))
        v = torch.rand(n, generator=gen) * 0.1
        _CASE_DATA.clear()   # one size resident at a time (the large one is 5 x 16 MiB)
        _CASE_DATA[n] = tuple(t.cuda() for t in (w, 2.0 * g, 0.1 * m, v, ema))   # g * gscale ~ N(0, 1): a third is clipped at 0.5
    return _CASE_DATA[n]


def _sub_range(kind, n):
    if kind == "all":
        return 0, n
    if kind == "none":                       # lo == hi: the average alone
        h = (n // 8) * 4
        return h, h
    return 4, n - 4                          # "inner"


@pytest.mark.parametrize("k", [0, 5, 10 ** 6])
@pytest.mark.parametrize("kind", ["all", "none", "inner"])
@pytest.mark.parametrize("n", [4, 1028, 4096 * 256 * 4 + 4])   # one vector; several blocks; one group more than the capped grid covers
def test_kernel_against_the_restatement(ops, n, kind, k):
    from littlegan_amd import _lib
    lo, hi = _sub_range(kind, n)
    w0, g0, m0, v0, e0 = _case_data(n)
    w, g, m, v, ema = (t.clone() for t in (w0, g0, m0, v0, e0))
    state = torch.tensor([0.5 ** 3, 0.9 ** 3], dtype=torch.float32, device="cuda")
    counter = torch.tensor([k], dtype=torch.int32, device="cuda")
    sc = (ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["clip"], ADAM["gscale"])
    if lo > hi:   # n = 4 has no inner range (4, 0): the entry point refuses it, nothing is launched
        with pytest.raises(_lib.LittleGanHipError, match="lo <= hi"):
            ops.clip_adam_ema_update(w, g, m, v, ema, lo, hi, state, counter, *sc, DECAY)
        torch.cuda.synchronize()
        assert torch.equal(w, w0) and torch.equal(ema, e0)
        return
    outside = torch.ones(n, dtype=torch.bool, device="cuda")
    outside[lo:hi] = False
    for t in (g, m, v):   # stale-range sentinel: whatever is read out there poisons the result
        t[outside] = float("nan")
    # the existing kernel on the trained slice
    wr, mr, vr = w0[lo:hi].clone(), m0[lo:hi].clone(), v0[lo:hi].clone()
    if hi > lo:
        ops.clip_adam_update(wr, g0[lo:hi].clone(), mr, vr, state, *sc)
    ops.clip_adam_ema_update(w, g, m, v, ema, lo, hi, state, counter, *sc, DECAY)
    torch.cuda.synchronize()
    assert int(counter) == k                                              # the update reads the counter, lg_ema_advance moves it
    assert torch.equal(w[lo:hi], wr) and torch.equal(m[lo:hi], mr) and torch.equal(v[lo:hi], vr)
    if hi > lo:
        assert not torch.equal(wr, w0[lo:hi])
    assert torch.equal(w[outside], w0[outside])                           # bit-unchanged
    assert bool(torch.isnan(m[outside]).all()) and bool(torch.isnan(v[outside]).all()) and bool(torch.isnan(g[outside]).all())
    assert bool(torch.isfinite(ema).all())
    ref = ema_update(_f64(e0), _f64(w), DECAY, k)
    err = np.abs(_f64(ema) - ref)
    bound = BOUND * np.maximum(np.abs(_f64(e0)), np.abs(_f64(w)))
    print(f"n={n} [{lo},{hi}) k={k}: d_t={ema_decay_at(DECAY, k):.7f} max err/bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), float((err / bound).max())
    assert not torch.equal(ema, e0)


def test_counter_advances_and_saturates(ops):
    c = torch.tensor([0], dtype=torch.int32, device="cuda")
    for want in (1, 2, 3):
        ops.ema_advance(c)
        assert int(c) == want
    c.fill_(2 ** 31 - 2)
    ops.ema_advance(c)
    assert int(c) == 2 ** 31 - 1
    ops.ema_advance(c)
    assert int(c) == 2 ** 31 - 1    # saturates, does not wrap


# ---------------------------------------------------------------------------------------------------------------- 2: the swap
@pytest.mark.parametrize("n", [4, 1028])
def test_swap(ops, n):
    gen = torch.Generator().manual_seed(7 + n)
    a0, b0 = torch.randn(n, generator=gen).cuda(), torch.randn(n, generator=gen).cuda()
    a0[0], b0[n - 1] = float("nan"), float("-inf")    # bits, not values, are moved
    a, b = a0.clone(), b0.clone()
    ops.swap_f32(a, b)
    assert torch.equal(a.view(torch.int32), b0.view(torch.int32)) and torch.equal(b.view(torch.int32), a0.view(torch.int32))
    ops.swap_f32(a, b)
    assert torch.equal(a.view(torch.int32), a0.view(torch.int32)) and torch.equal(b.view(torch.int32), b0.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- whole steps
def build_ema(cfg, W, mfma, ema_decay, **kw):
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    args = make_args(cfg, mfma)
    args.ema_decay = ema_decay
    for k, v in kw.items():
        setattr(args, k, v)
    decoder, encoder = Decoder(args), Encoder(args)
    g = Generator(args, decoder)
    d = Discriminator(args, encoder)
    tr = EagerTrainer(args, g, d, Adjuster(args, d, g), None)
    load_weights(tr, W)
    tr.reset_ema()   # the average starts from the weights just loaded
    return tr


_INPUTS = {}


def _inputs(cfg, b):
    """The step inputs of batch number b at the SMALL geometry: computed once, shared, never written to."""
    key = (cfg.batch_size, b)
    if key not in _INPUTS:
        _INPUTS[key] = f32_round(O.make_inputs(cfg, cfg.batch_size, seed=900 + b))
    return dev_inputs(_INPUTS[key])


def _same(a, b, what=("flat", "m", "v")):
    return all(torch.equal(getattr(a.store, k), getattr(b.store, k)) for k in what)


@pytest.mark.parametrize("mfma", ["f32", "bf16"])
def test_steps_with_the_average_leave_training_unchanged(mfma):
    """ema_decay = 0.9 against 0 on the same inputs: weights, Adam slots, beta powers and losses bit-identical after every step; the
    average follows the restatement iterated from the device's weights; the device counter is the step count."""
    cfg = O.Cfg(**SMALL)
    assert cfg.use_partition and cfg.partition_interval == 4 and cfg.train_adj
    W = perturbed(cfg, 1)
    on, off = build_ema(cfg, W, mfma, DECAY), build_ema(cfg, W, mfma, 0.0)
    assert off.store.ema is None and torch.equal(on.store.ema, on.store.flat) and int(on.store.ema_updates) == 0
    ref = _f64(on.store.ema)
    scale = np.abs(ref)
    for t, b in enumerate(BATCHES):
        inp = _inputs(cfg, b)
        r_on = on.train_step_from_inputs(b, inp)
        r_off = off.train_step_from_inputs(b, inp)
        torch.cuda.synchronize()
        assert _same(on, off), b
        assert all(torch.equal(on.opt_state[m], off.opt_state[m]) for m in "GDA"), b
        assert all(torch.equal(on.losses[k], off.losses[k]) for k in ("gen", "disc", "adj")), b
        for x, y in zip(r_on, r_off):
            assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), b
        w = _f64(on.store.flat)
        ref = ema_update(ref, w, DECAY, t)
        scale = np.maximum(scale, np.abs(w))
        err = np.abs(_f64(on.store.ema) - ref)
        bound = (t + 1) * BOUND * scale
        print(f"{mfma} b={b}: max err/bound {float((err[bound > 0] / bound[bound > 0]).max()):.3f}")
        assert (err <= bound).all(), (b, float(err.max()))
        assert int(on.store.ema_updates) == t + 1
    assert not torch.equal(on.store.ema, on.store.flat)


# ---------------------------------------------------------------------------------------------------------------- 4: graph replay
def test_graph_replay_with_the_average_is_bit_exact():
    """The sequence three times over, so every step kind runs eagerly, is captured and is replayed: the ramp of d_t continues through
    the replays because the kernel reads the counter on the device."""
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 2)
    eager, graph = build_ema(cfg, W, "bf16", DECAY), build_ema(cfg, W, "bf16", DECAY)
    for n, b in enumerate(BATCHES * 3):
        inp = _inputs(cfg, b)
        eager.train_step_from_inputs(b, inp)
        graph.graph_step(b, inp)
        torch.cuda.synchronize()
        assert _same(eager, graph, ("flat", "ema", "m", "v")), (n, b)
        assert int(eager.store.ema_updates) == int(graph.store.ema_updates) == n + 1
    assert len(graph._graphs) == 5   # (-1, F), (1, F), (2, F), (-1, T), (0, T)


# ---------------------------------------------------------------------------------------------------------------- 5: sampling
def test_sampling_through_the_average():
    cfg = O.Cfg(**SMALL)
    W = perturbed(cfg, 3)
    tr, twin = build_ema(cfg, W, "f32", DECAY), build_ema(cfg, W, "f32", DECAY)   # twin never samples
    for b in (1, 11, 12):
        tr.train_step_from_inputs(b, _inputs(cfg, b))
        twin.train_step_from_inputs(b, _inputs(cfg, b))
    d = _inputs(cfg, 1)
    noise, cond, image = d["noise"], d["real_cond_2"], d["real_image_1"]
    flat0, ema0 = tr.store.flat.clone(), tr.store.ema.clone()
    assert not torch.equal(flat0, ema0)
    other = build_ema(cfg, W, "f32", 0.0)
    other.store.flat.copy_(ema0)
    other.store.bump()
    want = other.generator([noise, cond])
    with tr.ema_weights():
        got = tr.generator([noise, cond])
        assert torch.equal(tr.store.flat, ema0) and torch.equal(tr.store.ema, flat0)
        with tr.ema_weights():     # nested: a no-op
            assert torch.equal(tr.store.flat, ema0)
        assert torch.equal(tr.store.flat, ema0)     # ... that leaves the outer block in place
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.train_step_from_inputs(13, _inputs(cfg, 13))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(tr.store.flat, flat0) and torch.equal(tr.store.ema, ema0)    # bit-restored
    raw = tr.generator([noise, cond])
    assert not torch.equal(raw, got)
    # predict: the default reads the average, ema=False the raw weights
    p_def = tr.predict(noise, cond, image)
    p_raw = tr.predict(noise, cond, image, ema=False)
    p_ema = tr.predict(noise, cond, image, ema=True)
    assert torch.equal(p_def[0], got) and torch.equal(p_ema[0], got) and torch.equal(p_raw[0], raw)
    assert not torch.equal(p_def[0], p_raw[0])
    assert not torch.equal(p_def[2], p_raw[2])      # the Adjuster's output too: the whole store is averaged
    assert torch.equal(tr.store.flat, flat0) and torch.equal(tr.store.ema, ema0)
    tr.sample_ema = False
    assert torch.equal(tr.predict(noise, cond, image)[0], raw)
    tr.sample_ema = True
    # an EMA-off trainer: ema_weights() and predict(ema=True) are the raw weights
    with other.ema_weights():
        assert torch.equal(other.store.flat, ema0)
    assert torch.equal(other.predict(noise, cond, image, ema=True)[0], want)
    # one more training step: the same bits as the run that never sampled
    tr.train_step_from_inputs(13, _inputs(cfg, 13))
    twin.train_step_from_inputs(13, _inputs(cfg, 13))
    torch.cuda.synchronize()
    assert _same(tr, twin, ("flat", "ema", "m", "v")) and int(tr.store.ema_updates) == int(twin.store.ema_updates) == 4


# ---------------------------------------------------------------------------------------------------------------- 6: checkpoints
def test_checkpoint_round_trip_continues_the_average(tmp_path):
    from littlegan_amd.eager_trainer import EagerTrainer
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    cfg = O.Cfg(init_dim=2, conv_filter=(32, 32, 32, 32, 32), cond_dim=3, noise_dim=5, batch_size=2)

    def mk(restore, ema_decay, sub):
        args = make_args(cfg, "f32")
        args.no_io, args.result_dir, args.restore, args.exp_name, args.epoch = False, str(tmp_path / sub), restore, "t", 1
        args.ema_decay = ema_decay
        dec, enc = Decoder(args), Encoder(args)
        g = Generator(args, dec)
        d = Discriminator(args, enc)
        return EagerTrainer(args, g, d, Adjuster(args, d, g), None)

    inps = [dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=70 + b))) for b in range(4)]
    tr = mk(False, DECAY, "on")
    load_weights(tr, perturbed(cfg, 3))
    tr.reset_ema()
    for b in range(3):
        tr.train_step_from_inputs(9 + b, inps[b])
    path = tr.save_checkpoint("7")
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["format"] == "littlegan_amd-ckpt-1" and ck["ema_updates"] == 3 and torch.equal(ck["ema"], tr.store.ema.cpu())
    saved_ema = tr.store.ema.clone()
    tr.train_step_from_inputs(12, inps[3])
    tr2 = mk(True, DECAY, "on")   # restores in the constructor
    assert torch.equal(tr2.store.ema, saved_ema) and int(tr2.store.ema_updates) == 3
    tr2.train_step_from_inputs(12, inps[3])
    torch.cuda.synchronize()
    assert _same(tr, tr2, ("flat", "ema", "m", "v")) and int(tr2.store.ema_updates) == int(tr.store.ema_updates) == 4
    # a checkpoint with the average loads into a trainer that keeps none: the keys are ignored
    tr_off = mk(True, 0.0, "on")
    assert tr_off.store.ema is None and torch.equal(tr_off.store.flat.cpu(), ck["flat"])
    assert "ema" not in tr_off.checkpoint_state()
    # a checkpoint written without the average loads into a trainer that keeps one: it restarts from the loaded weights
    off = mk(False, 0.0, "off")
    load_weights(off, perturbed(cfg, 4))
    off.train_step_from_inputs(11, inps[0])
    p_off = off.save_checkpoint("1")
    assert "ema" not in torch.load(p_off, map_location="cpu", weights_only=True)
    tr3 = mk(True, DECAY, "off")
    assert torch.equal(tr3.store.flat, off.store.flat) and torch.equal(tr3.store.ema, tr3.store.flat) and int(tr3.store.ema_updates) == 0
    # export-model: the average beside the raw weights
    exp = torch.load(tr2.export_model_checkpoint(), map_location="cpu", weights_only=True)
    assert torch.equal(exp["ema_flat"], tr2.store.ema.cpu()) and torch.equal(exp["flat"], tr2.store.flat.cpu())
    assert "ema_flat" not in torch.load(off.export_model_checkpoint(), map_location="cpu", weights_only=True)


# ---------------------------------------------------------------------------------------------------------------- 7: two ranks
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
        cfg = O.Cfg(**{**SMALL, "batch_size": 2})
        tr = build_ema(cfg, perturbed(cfg, 21), "bf16", DECAY)
        assert tr.sync.enabled and tr.rank == rank
        B = cfg.batch_size
        for b in (10, 11, 12):   # a partition step without the Adjuster, two full steps with it
            full = f32_round(O.make_inputs(cfg, B * world, seed=300 + b))
            tr.train_step_from_inputs(b, dev_inputs({k: v[rank * B:(rank + 1) * B] for k, v in full.items()}))
        torch.cuda.synchronize()
        np.save(os.path.join(outdir, f"ema_{rank}.npy"), tr.store.ema.cpu().numpy())
        np.save(os.path.join(outdir, f"flat_{rank}.npy"), tr.store.flat.cpu().numpy())
        with open(os.path.join(outdir, f"count_{rank}.json"), "w") as f:
            json.dump(int(tr.store.ema_updates), f)
    finally:
        dist.destroy_process_group()


def test_two_ranks_hold_the_same_average(tmp_path):
    """No communication is added for the average: the weights are identical on every rank after the all-reduced step, so are the averages."""
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
    ema = [np.load(tmp_path / f"ema_{r}.npy") for r in range(world)]
    flat = [np.load(tmp_path / f"flat_{r}.npy") for r in range(world)]
    assert np.array_equal(ema[0].view(np.int32), ema[1].view(np.int32)) and np.isfinite(ema[0]).all()
    assert np.array_equal(flat[0], flat[1]) and not np.array_equal(ema[0], flat[0])
    assert [json.load(open(tmp_path / f"count_{r}.json")) for r in range(world)] == [3, 3]
