"""The Adjuster's forward without its single-reader normalised maps (include/littlegan_adj.h), on the GPU.

Every fused form is bit-identical to the route through the stored maps by construction, so every comparison here is torch.equal:

  * lgadj_convT_s2_fwd_stats_ns (conv_up3's NSK form: norm + LeakyReLU + skip formed between the halo's buffer load and its LDS store)
    against instnorm_apply per skip part + convT_s2_fwd_stats, on the output z16, the moment partials and the finished records, for
    both tilings, at a single tile (every halo side is padding), interior + edge tiles, an odd tile count per wave rotation, B = 1..3
    with an empty first / empty second / odd split of the skip, every combination of raw and normalised skip parts, and one batch
    that gives the persistent grid more than one item per block (computed from the launcher's grid rule);
  * lgadj_instnorm_apply_rs / _p_rs (the apply pass whose skip is raw) against normalise-then-apply, at a sample length that is no
    multiple of the block's unroll and for one sample;
  * the same fused launch twice: equal outputs;
  * (every new entry point between guard bands, operands included: the adj-* rows of tests/test_memory_contract_gpu.py);
  * the whole Adjuster forward + backward_own at the smallest configuration that reaches every new route, against the same run with
    the predicates forced off: image, loss and the four gradients."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ALPHA = 0.3
BF16 = 1          # _lib.DT_BF16
TH, TW = 8, 16    # conv_up3's source tile


@pytest.fixture(scope="module")
def ops():
    from littlegan_amd import ops as _ops
    return _ops


def bf16(rng, *shape, scale=1.0, shift=0.0):
    return (torch.tensor(rng.standard_normal(shape) * scale + shift, dtype=torch.float32, device="cuda")).to(torch.bfloat16)


def f32(a):
    return torch.tensor(np.asarray(a, dtype=np.float32), device="cuda")


def records(ops, z16, gamma, beta):
    """finished statistics records of a raw bf16 map (the library's own statistics pass on its fp32 value)"""
    return ops.instnorm_stats(z16.float().contiguous(), gamma, beta, 0, ALPHA)


def stored_map(ops, raw):
    """the bf16 map the encoder's apply pass stores for a raw level"""
    h = torch.empty_like(raw.z)
    ops.instnorm_apply(raw.z, raw.stats, None, 0, 1, ALPHA, out16=h, want_f32=False)
    return h


def multi_item_batch(ops, hs, ws, n):
    """the smallest B at which conv_up3's persistent grid runs more than one item per block: grid = min(steps, blocks), steps = B * tiles
    per sample (one tile per step in both forward tilings), blocks = one 8-wave workgroup per CU (N = 64) or two 4-wave ones (N = 32)"""
    blocks = (1 if n == 64 else 2) * int(ops._lib.load().lg_grid_cus())
    tiles = (hs // TH) * (ws // TW)
    return blocks // tiles + 1


class Layer:
    """one transposed conv cs -> cb with its norm parameters, and the level below it (raw z + records + skip parts)"""

    def __init__(self, ops, cs, cb, seed):
        rng = np.random.default_rng(seed)
        self.cs, self.cb, self.rng = cs, cb, rng
        w = torch.tensor(rng.standard_normal((5, 5, cb, cs)) * 0.05, dtype=torch.float32, device="cuda")
        self.pack = ops.conv_pack(w, cb, cs, BF16)
        self.bias = f32(rng.standard_normal(cb) * 0.2)
        self.gm, self.bt = f32([1.2]), f32([-0.1])          # of the produced map
        self.gz, self.bz = f32([0.9]), f32([0.15])          # of the level below
        self.gs, self.bs = f32([1.1]), f32([-0.2])          # of a raw skip

    def operands(self, ops, B, hs, ws, b1, kinds):
        z = bf16(self.rng, B, hs, ws, self.cs, scale=1.3, shift=0.2)
        zst = records(ops, z, self.gz, self.bz)
        parts = []
        for rows, kind in zip((b1, B - b1), kinds):
            if rows == 0:
                parts.append(None)
            elif kind == "raw":
                s = bf16(self.rng, rows, hs, ws, self.cs, scale=0.8, shift=-0.3)
                parts.append(ops.Raw(s, records(ops, s, self.gs, self.bs)))
            else:
                parts.append(bf16(self.rng, rows, hs, ws, self.cs))
        return z, zst, parts

    def two_pass(self, ops, z, zst, parts, b1):
        """instnorm_apply per skip part (a raw part through its stored map) + the plain forward -> (z16, partials, records)"""
        B = z.shape[0]
        h = torch.empty_like(z)
        for (lo, hi), part in zip(((0, b1), (b1, B)), parts):
            if hi > lo:
                sk = stored_map(ops, part) if isinstance(part, ops.Raw) else part
                ops.instnorm_apply(z[lo:hi], zst[lo:hi], sk, 0, 1, ALPHA, out16=h[lo:hi], want_f32=False)
        out, mom = ops.convT_s2_fwd_stats(None, self.pack, self.bias, self.cb, BF16, self.gm, self.bt, x16=h, z16=True, defer_stats=True)
        assert ops.last_kernel().startswith("conv_up3_kernel"), ops.last_kernel()
        part = mom.ws[:B * mom.nparts * 24].clone()
        return out, part, ops.stats_tensor(mom).clone()

    def fused(self, ops, z, zst, parts, b1):
        B = z.shape[0]
        skip = (parts[0] if parts[0] is not None else z[:0], parts[1]) if b1 < B else (parts[0], None)
        out, mom = ops.convT_s2_fwd_stats_ns(z, zst, ALPHA, skip, self.pack, self.bias, self.cb, BF16, self.gm, self.bt, defer_stats=True)
        assert ops.last_kernel().startswith("conv_up3_kernel"), ops.last_kernel()
        part = mom.ws[:B * mom.nparts * 24].clone()
        return out, part, ops.stats_tensor(mom).clone()


FORMS = [(128, 64, 8, 16), (128, 64, 16, 32), (64, 32, 8, 16), (64, 32, 16, 32), (64, 32, 8, 32)]


@pytest.mark.parametrize("cs,cb,hs,ws", FORMS)
def test_fused_conv_up3_equals_apply_then_conv(ops, cs, cb, hs, ws):
    lay = Layer(ops, cs, cb, seed=cs + hs * ws)
    seen = 0
    for B in (1, 2, 3):
        assert ops.convT_s2_fwd_ns_supported(B, hs, ws, cb, cs, BF16)
        for b1 in sorted({0, 1, B}):
            for kinds in itertools.product(("raw", "map"), repeat=2):
                z, zst, parts = lay.operands(ops, B, hs, ws, b1, kinds)
                want, got = lay.two_pass(ops, z, zst, parts, b1), lay.fused(ops, z, zst, parts, b1)
                for name, w, g in zip(("z16", "moment partials", "records"), want, got):
                    assert torch.equal(w, g), (name, B, b1, kinds)
                assert torch.isfinite(got[0].float()).all() and got[0].float().abs().max() > 0.1
                seen += 1
    assert seen == (2 + 3 + 3) * 4


@pytest.mark.parametrize("cs,cb,hs,ws", [(128, 64, 16, 32), (64, 32, 16, 32)])
def test_fused_conv_up3_with_more_than_one_item_per_block(ops, cs, cb, hs, ws):
    """a batch one tile beyond the persistent grid, split unevenly between a raw and a stored skip part; launched twice: the two
    launches agree with each other (determinism) and with the two-pass route"""
    B = multi_item_batch(ops, hs, ws, cb)
    assert B * (hs // TH) * (ws // TW) > (1 if cb == 64 else 2) * int(ops._lib.load().lg_grid_cus())
    lay = Layer(ops, cs, cb, seed=7 + cs)
    b1 = B // 3
    z, zst, parts = lay.operands(ops, B, hs, ws, b1, ("raw", "map"))
    want = lay.two_pass(ops, z, zst, parts, b1)
    first, second = lay.fused(ops, z, zst, parts, b1), lay.fused(ops, z, zst, parts, b1)
    for name, w, a, b in zip(("z16", "moment partials", "records"), want, first, second):
        assert torch.equal(a, b), f"{name}: two launches differ"
        assert torch.equal(w, a), name


def hand_moments(ops, z16, nparts, gamma, beta):
    """ops.Moments over exact {count, mean, M2} records of nparts chunks per sample, as a conv epilogue would have left them"""
    B = z16.shape[0]
    x = z16.double().reshape(B, -1)
    rec = torch.empty(B, nparts, 3, dtype=torch.float64, device="cuda")
    for i, c in enumerate(torch.tensor_split(x, nparts, dim=1)):
        m = c.mean(1)
        rec[:, i, 0], rec[:, i, 1], rec[:, i, 2] = c.shape[1], m, ((c - m[:, None]) ** 2).sum(1)
    return ops.Moments(rec.view(torch.uint8).reshape(-1), nparts, gamma, beta, B)


@pytest.mark.parametrize("B,L8", [(1, 1029), (3, 2049), (2, 5), (3, 4096)])
@pytest.mark.parametrize("post_leaky", [1, 0])
def test_apply_with_a_raw_skip_equals_normalise_then_apply(ops, B, L8, post_leaky):
    """both forms (records finished / finalize folded into the launch, over two row ranges as the decoder calls it); 512 sixteen-byte
    pieces per block trip: L8 = 1029 and 2049 end in a ragged trip, 5 is less than one wave, B = 1 is one sample"""
    rng = np.random.default_rng(B * 10000 + L8)
    L = 8 * L8
    gm, bt, gs, bs = f32([1.2]), f32([-0.1]), f32([0.8]), f32([0.25])
    z = bf16(rng, B, L, scale=1.4, shift=0.3)
    s = bf16(rng, B, L, scale=0.7, shift=-0.2)
    raw = ops.Raw(s, records(ops, s, gs, bs))
    smap = stored_map(ops, raw)
    st = ops.stats_tensor(hand_moments(ops, z, 3, gm, bt)).clone()
    # records finished
    want16, got16 = torch.empty_like(z), torch.empty_like(z)
    want = ops.instnorm_apply(z, st, smap, 0, post_leaky, ALPHA, out16=want16)
    got = ops.instnorm_apply(z, st, raw, 0, post_leaky, ALPHA, out16=got16)
    assert ops.last_kernel() == "apply16_rs_kernel"
    assert torch.equal(want, got) and torch.equal(want16, got16)
    # finalize folded in, rows [0, b1) with the raw skip and the rest with the stored map
    b1 = (B + 1) // 2
    outs = []
    for use_raw in (False, True):
        mom = hand_moments(ops, z, 3, gm, bt)
        y16 = torch.empty_like(z)
        for lo, hi in ((0, b1), (b1, B)):
            if hi > lo:
                sk = ops.Raw(raw.z[lo:hi], raw.stats[lo:hi]) if (use_raw and lo == 0) else smap[lo:hi]
                ops.instnorm_apply(z[lo:hi], mom[lo:hi], sk, 0, post_leaky, ALPHA, out16=y16[lo:hi], want_f32=False)
                if use_raw and lo == 0:
                    assert ops.last_kernel() == "apply16p_rs_kernel"
        assert mom.covered == B
        outs.append((y16, mom.stats.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[1][0], want16) and torch.equal(outs[1][1], st)


def test_refusals_without_a_launch(ops):
    lib = ops._lib.load()
    one = torch.zeros(64, device="cuda")
    p = one.data_ptr()
    n = ctypes.c_int(0)
    assert lib.lgadj_instnorm_apply_rs(p, p, p, p, 0, 0, 1, 8, 1, ALPHA, 0) != 0 and b"null pointer" in lib.lg_last_error()
    assert lib.lgadj_instnorm_apply_rs(p, p, p, p, p, 0, 1, 12, 1, ALPHA, 0) != 0 and b"bad shape" in lib.lg_last_error()
    assert lib.lgadj_instnorm_apply_p_rs(p, p, 0, p, p, p, p, p, p, 0, 1, 8, 1, ALPHA, 0) != 0 and b"bad shape" in lib.lg_last_error()
    assert not lib.lgadj_convT_s2_fwd_ns_supported(2, 8, 16, 64, 128, 0)        # f32 operands
    assert not lib.lgadj_convT_s2_fwd_ns_supported(2, 8, 8, 64, 128, BF16)      # no whole tile
    assert not lib.lgadj_convT_s2_fwd_ns_supported(2, 8, 16, 128, 256, BF16)    # conv_up4's layer
    assert lib.lgadj_convT_s2_fwd_stats_ns(p, p, ALPHA, p, 0, p, 0, 3, p, p, p, 2, 8, 16, 64, 128, BF16, p, 1 << 20, ctypes.addressof(n), 0) != 0
    assert b"first skip range" in lib.lg_last_error()
    assert lib.lgadj_convT_s2_fwd_stats_ns(p, p, ALPHA, 0, 0, p, 0, 1, p, p, p, 2, 8, 16, 64, 128, BF16, p, 1 << 20, ctypes.addressof(n), 0) != 0
    assert lib.lgadj_convT_s2_fwd_stats_ns(p, p, ALPHA, p, 0, p, 0, 1, p, p, p, 2, 8, 8, 64, 128, BF16, p, 1 << 20, ctypes.addressof(n), 0) == -3
    assert lib.lgadj_convT_s2_fwd_stats_ns(p, p, ALPHA, p, 0, p, 0, 1, p, p, p, 2, 8, 16, 64, 128, BF16, p, 16, ctypes.addressof(n), 0) != 0
    assert b"workspace too small" in lib.lg_last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# the whole Adjuster forward + backward_own.  init_dim = 4 (a 64 x 64 image) has the smallest maps that reach every new route: the
# encoder's level 1 -> 2 (32 x 32 x 64 into conv2; its 16 x 16 output is the smallest map of the normalising conv, level 2 -> 3 is an
# 8 x 8 output and stays on the apply route), the decoder's levels 2 -> 3 (16 x 16 x 128 into convT3) and 3 -> 4 (32 x 32 x 64 into
# convT4, with the RAW level-1 skip), the smallest whole tiles of both fused forward tilings, and — with the fused conv off — the
# raw-skip apply.  The smallest batch is read off the adoption rule (ops.enc_raw_skip_adopted, ops.convT_s2_fwd_ns_adopted): the
# consuming conv must have a tile for every CU, and conv2's 16 x 16 output is two tiles per sample.  The predicates are asserted below.
def adopted_batch(ops):
    return -(-int(ops._lib.load().lg_grid_cus()) // 2)


def _adjuster_run(ops, monkeypatch, off, batch=None):
    from types import SimpleNamespace
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator, ParamStore
    args = SimpleNamespace(batch_size=batch or adopted_batch(ops), image_channel=3, noise_dim=16, init_dim=4, conv_filter=(512, 256, 128, 64, 32), kernel_size=5,
                           leaky_alpha=ALPHA, cond_dim=5, mfma_dtype="bf16", device="cuda", seed=3)
    for name in off:
        monkeypatch.setattr(ops, name, lambda *a, **k: False)
    g = Generator(args, Decoder(args))
    d = Discriminator(args, Encoder(args))
    adj = Adjuster(args, d, g)
    store = ParamStore(g, d, adj)
    store.bump()
    B, S = args.batch_size, args.init_dim * 16
    rng = np.random.default_rng(11)
    img1, fake, target = (f32(np.tanh(rng.standard_normal((n, S, S, 3)))) for n in (B, B, 2 * B))
    cond = f32(rng.uniform(0, 1, (2 * B, args.cond_dim)))
    # which routes the forward takes: calls of the three wrappers only the new routing reaches
    calls = {"zn": 0, "ns": 0, "raw_apply": 0}
    real_zn, real_ns, real_apply = ops.conv2d_s2_fwd_stats_zn, ops.convT_s2_fwd_stats_ns, ops.instnorm_apply

    def zn(*a, **k):
        calls["zn"] += 1
        return real_zn(*a, **k)

    def ns(*a, **k):
        calls["ns"] += 1
        return real_ns(*a, **k)

    def apply(x, stats, skip, *a, **k):
        calls["raw_apply"] += isinstance(skip, ops.Raw)
        return real_apply(x, stats, skip, *a, **k)

    monkeypatch.setattr(ops, "conv2d_s2_fwd_stats_zn", zn)
    monkeypatch.setattr(ops, "convT_s2_fwd_stats_ns", ns)
    monkeypatch.setattr(ops, "instnorm_apply", apply)
    tails = adj.encoder(fake)
    ctx = {}
    img = adj([img1, cond], ctx, enc_tails=tails)
    loss = torch.zeros(1, device="cuda")
    g_in = f32(rng.standard_normal(img.shape) * 0.01)
    dpre = torch.empty_like(img)
    ops.l1_tanh_loss(target, img, g_in, dpre, loss, 10.0, True)
    store.grad.zero_()
    adj.backward_own(ctx, dpre)
    torch.cuda.synchronize()
    lo, hi = store.model_range("A")
    grads = [adj._dn._g[n].clone() for n in ("dense.kernel", "dense.bias", "norm.gamma", "norm.beta")]
    assert store.grad[lo:hi].abs().max() > 0
    return img.clone(), loss.clone(), grads, calls, ctx


PREDICATES = ("enc_raw_skip_adopted", "convT_s2_fwd_ns_adopted")
_REF = {}   # the run with both predicates off, computed once


@pytest.mark.parametrize("off", [(), PREDICATES, PREDICATES[:1], PREDICATES[1:]], ids=["routed", "all-off", "encoder-off", "decoder-off"])
def test_adjuster_forward_and_backward_own_do_not_depend_on_the_route(ops, monkeypatch, off):
    if not off:
        B = adopted_batch(ops)
        assert ops.enc_raw_skip_adopted(B, 32, 32, 64, 128, BF16) and not ops.enc_raw_skip_adopted(B - 1, 32, 32, 64, 128, BF16)
        assert not ops.enc_raw_skip_adopted(B, 16, 16, 128, 256, BF16) and not ops.enc_raw_skip_adopted(B + 1, 16, 16, 128, 256, BF16)
        assert ops.convT_s2_fwd_ns_adopted(2 * B, 16, 16, 64, 128, BF16) and ops.convT_s2_fwd_ns_adopted(2 * B, 32, 32, 32, 64, BF16)
        assert not ops.convT_s2_fwd_ns_adopted(2 * B, 8, 8, 128, 256, BF16)
    if "ref" not in _REF:
        with monkeypatch.context() as mp:
            _REF["ref"] = _adjuster_run(ops, mp, PREDICATES)
    ref = _REF["ref"]
    assert ref[3] == {"zn": 0, "ns": 0, "raw_apply": 0}
    with monkeypatch.context() as mp:
        got = _adjuster_run(ops, mp, off)
    enc_on, dec_on = PREDICATES[0] not in off, PREDICATES[1] not in off
    # level 1 -> 2 of the encoder; both conv_up3 levels of the decoder; the raw level-1 skip goes through the raw-skip apply exactly
    # where the fused conv does not take it
    assert got[3] == {"zn": int(enc_on), "ns": 2 * int(dec_on), "raw_apply": int(enc_on and not dec_on)}, got[3]
    if dec_on:   # the levels above a fused level keep no input; backward_own worked from z and the records alone
        assert [got[4]["dec"][i][0] is None and got[4]["dec"][i][3] is None for i in range(4)] == [False, False, True, True]
    assert torch.equal(ref[0], got[0]), "image"
    assert torch.equal(ref[1], got[1]), "loss"
    for name, a, b in zip(("dense.kernel", "dense.bias", "norm.gamma", "norm.beta"), ref[2], got[2]):
        assert torch.equal(a, b), name


def test_a_batch_below_the_adoption_rule_stays_on_the_apply_route(ops, monkeypatch):
    """B = 2: the kernels would run (the *_supported predicates say so) but no CU's workgroup would get a whole round of tiles — every
    level keeps its apply pass, launch for launch the parent's forward"""
    assert ops.conv2d_s2_fwd_stats_zn_supported(2, 32, 32, 64, 128, BF16) and ops.convT_s2_fwd_ns_supported(4, 32, 32, 32, 64, BF16)
    assert not ops.enc_raw_skip_adopted(2, 32, 32, 64, 128, BF16) and not ops.convT_s2_fwd_ns_adopted(4, 32, 32, 32, 64, BF16)
    with monkeypatch.context() as mp:
        got = _adjuster_run(ops, mp, (), batch=2)
    assert got[3] == {"zn": 0, "ns": 0, "raw_apply": 0}
    assert all(got[4]["dec"][i][3] is not None for i in range(4))
