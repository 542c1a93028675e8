"""The Adjuster's forward without its single-reader normalised maps, without a GPU: the names of the header
include/littlegan_adj.h, its host-side refusals, and the ROUTING decisions of Encoder,
Decoder and Adjuster for every combination of predicate results — model.py run on CPU tensors against a stand-in for littlegan_amd.ops
that records each call and computes nothing (the arithmetic is tests/test_adj_fused_gpu.py's business)."""
import ctypes as C
import itertools
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_abi import ROOT, _protos  # noqa: E402

ADJ_HEADER = os.path.join(ROOT, "include", "littlegan_adj.h")
ENTRY_POINTS = ("lgadj_instnorm_apply_rs", "lgadj_instnorm_apply_p_rs", "lgadj_convT_s2_fwd_ns_supported", "lgadj_convT_s2_fwd_stats_ns")


# ---------------------------------------------------------------------------------------------------------------------
# the header
@pytest.fixture(scope="module")
def lib():
    from littlegan_amd.csrc.build import build
    build(verbose=False)
    from littlegan_amd import _lib
    return _lib


def test_adj_header_declares_the_entry_points(lib):
    assert set(_protos(ADJ_HEADER)) == set(ENTRY_POINTS) == {n for n in lib.SIGNATURES if n.startswith("lgadj_")}


def test_the_sources_include_the_header_and_are_built():
    from littlegan_amd.csrc import build as B
    for name in ("norm_rs.hip", "conv_up3.hip"):
        assert "littlegan_adj.h" in open(os.path.join(ROOT, "littlegan_amd", "csrc", name)).read() and name in B.SOURCES


def test_host_side_refusals(lib):
    h = lib.load()
    n = C.c_int(7)
    assert h.lgadj_instnorm_apply_rs(None, None, None, None, None, None, 1, 8, 1, 0.3, None) == -1 and b"null pointer" in h.lg_last_error()
    assert h.lgadj_instnorm_apply_p_rs(None, None, 1, None, None, None, None, None, None, None, 1, 8, 1, 0.3, None) == -1
    assert h.lgadj_convT_s2_fwd_stats_ns(None, None, 0.3, None, None, None, None, 0, None, None, None, 1, 8, 16, 64, 128, 1, None, 0,
                                         C.addressof(n), None) == -1
    assert n.value == 0 and b"null pointer" in h.lg_last_error()
    for shape in ((2, 8, 16, 64, 128, 0), (2, 8, 8, 64, 128, 1), (2, 12, 16, 64, 128, 1), (2, 8, 16, 128, 256, 1), (0, 8, 16, 64, 128, 1)):
        assert h.lgadj_convT_s2_fwd_ns_supported(*shape) == 0, shape


# ---------------------------------------------------------------------------------------------------------------------
# the routing: model.py on a stand-in for ops
class FakeRaw:
    def __init__(self, z, stats):
        self.z, self.stats = z, stats

    @property
    def shape(self):
        return self.z.shape


class FakeDrop:
    def __init__(self, active):
        self.active = active

    def at(self, level=None, r0=None):
        return self


class FakeOps:
    """records (name, note) per call; zn_ok(level below) / ns_ok(level below) decide the two predicates by the channel count of the
    map the asking conv reads, which names the level in the configuration below"""
    Raw = FakeRaw

    def __init__(self, zn_ok=(), ns_ok=(), raw_ok=None):
        """raw_ok: the levels the Adjuster's encoder route is adopted for (default: wherever the normalising conv runs)"""
        self.zn_ok, self.ns_ok, self.log, self.asked = set(zn_ok), set(ns_ok), [], []
        self.raw_ok = self.zn_ok if raw_ok is None else set(raw_ok)

    def names(self):
        return [n for n, _ in self.log]

    # -- predicates
    def conv2d_s2_fwd_stats_zn_supported(self, B, H, W, cb, cs, dtype):
        return ENC_LEVEL_OF[cb] in self.zn_ok

    def enc_raw_skip_adopted(self, B, H, W, cb, cs, dtype):
        self.asked.append(("raw", ENC_LEVEL_OF[cb]))
        return ENC_LEVEL_OF[cb] in self.raw_ok

    def convT_s2_fwd_ns_adopted(self, B, Hs, Ws, cb, cs, dtype):
        return DEC_LEVEL_OF[cs] in self.ns_ok

    def conv_halo_supported(self, *a):
        return True

    def n3_m16_supported(self, *a):
        return True

    def convT_s1_tanh_fwd_z16_supported(self, *a):
        return True

    # -- ops
    def conv_pack(self, w, cb, cs, dtype, out=None):
        return torch.zeros(1)

    def stats_tensor(self, st):
        return st

    def instnorm_stats(self, x, *a, **k):
        return torch.zeros(x.shape[0], 8)

    def conv2d_s2_fwd_stats(self, x, pack, bias, cs, dtype, gamma, beta, x16=None, z16=False, alpha=0.3, defer_stats=False):
        src = x if x is not None else x16
        B, H, W, _ = src.shape
        self.log.append(("conv", cs))
        return torch.zeros(B, H // 2, W // 2, cs, dtype=torch.bfloat16 if z16 else torch.float32), torch.zeros(B, 8)

    def conv2d_s2_fwd_stats_zn(self, z, st, alpha, pack, bias, cs, dtype, gamma, beta):
        B, H, W, _ = z.shape
        self.log.append(("conv_zn", cs))
        return torch.zeros(B, H // 2, W // 2, cs, dtype=torch.bfloat16), torch.zeros(B, 8)

    def convT_s2_fwd_stats(self, x, pack, bias, cb, dtype, gamma, beta, x16=None, z16=False, alpha=0.3, defer_stats=False):
        src = x if x is not None else x16
        B, H, W, _ = src.shape
        self.log.append(("convT", cb))
        return torch.zeros(B, 2 * H, 2 * W, cb, dtype=torch.bfloat16 if z16 else torch.float32), torch.zeros(B, 8)

    def convT_s2_fwd_stats_ns(self, z, st, alpha, skip, pack, bias, cb, dtype, gamma, beta, defer_stats=False):
        B, H, W, _ = z.shape
        parts = skip if isinstance(skip, tuple) else (skip,)
        self.log.append(("convT_ns", (cb, tuple("raw" if isinstance(p, FakeRaw) else "map" for p in parts))))
        return torch.zeros(B, 2 * H, 2 * W, cb, dtype=torch.bfloat16), torch.zeros(B, 8)

    def instnorm_apply(self, x, stats, skip, pre_leaky, post_leaky, alpha, out=None, out16=None, want_f32=True, drop=None):
        kind = "none" if skip is None else "raw" if isinstance(skip, FakeRaw) else "map"
        self.log.append(("apply", (x.shape[-1], kind, drop is not None and drop.active)))
        return None if not want_f32 else (out if out is not None else torch.zeros(x.shape))

    def dense_fwd(self, x, w, b):
        return torch.zeros(x.shape[0], w.shape[1])

    def convT_s1_tanh_fwd_z16(self, z, st, alpha, pack, bias, cb, dtype, out=None):
        self.log.append(("final_raw", cb))
        return torch.zeros(*z.shape[:3], cb)

    def convT_s1_tanh_fwd(self, x, pack, bias, cb, dtype, out=None, x16=None):
        self.log.append(("final", cb))
        src = x if x is not None else x16
        return torch.zeros(*src.shape[:3], cb)


CF = (80, 64, 48, 32, 16)                       # conv_filter: every level has its own channel count
ENC_LEVEL_OF = {3: 0, 32: 1, 48: 2, 64: 3}      # channels of the map a conv reads -> the encoder level that wrote it
DEC_LEVEL_OF = {80: 0, 64: 1, 48: 2, 32: 3}     # channels of the map a transposed conv reads -> the decoder level that wrote it
SIDE, OWN, TAIL = 32, 2, 3


def args_of(dtype="bf16"):
    return SimpleNamespace(image_channel=3, conv_filter=CF, init_dim=SIDE // 16, leaky_alpha=0.3, cond_dim=4, noise_dim=5,
                           mfma_dtype=dtype, device="cpu", seed=1)


@pytest.fixture
def fake(monkeypatch):
    from littlegan_amd import model

    def install(**kw):
        f = FakeOps(**kw)
        monkeypatch.setattr(model, "ops", f)
        return f
    return install


def tails_of(rows=TAIL):
    """what D's pass over the handed-over rows left: bf16 maps 1-3, the fp32 top map"""
    out, side = [], SIDE
    for i in range(1, 5):
        side //= 2
        out.append(torch.zeros(rows, side, side, CF[4 - i], dtype=torch.float32 if i == 4 else torch.bfloat16))
    return out


@pytest.mark.parametrize("zn_ok", [(), (1,), (2,), (1, 2), (1, 2, 3)])
@pytest.mark.parametrize("raw_skips,with_tails,drop", [(True, True, None), (True, True, "inactive"), (True, True, "active"),
                                                       (True, False, None), (False, True, None)])
def test_encoder_routing(fake, zn_ok, raw_skips, with_tails, drop):
    from littlegan_amd.model import Encoder
    f = fake(zn_ok=zn_ok)
    enc = Encoder(args_of())
    tails = tails_of() if with_tails else None
    d = None if drop is None else FakeDrop(drop == "active")
    outs = enc(torch.zeros(OWN, SIDE, SIDE, 3), None, tails=tails, drop=d, raw_skips=raw_skips)
    on = raw_skips and with_tails and drop != "active"
    raw_levels = [i for i in (1, 2) if on and i in zn_ok]          # level 3 keeps its apply whatever the predicate says
    for i in range(1, 5):
        own = outs[i - 1][0] if with_tails else outs[i - 1]
        assert isinstance(own, FakeRaw) == (i in raw_levels), (i, raw_levels)
        if with_tails:
            assert outs[i - 1][1] is tails[i - 1]
    convs = [n for n in f.log if n[0] in ("conv", "conv_zn")]
    assert convs == [("conv_zn" if (i - 1) in raw_levels else "conv", CF[4 - i]) for i in range(1, 5)]
    applies = [n[1][0] for n in f.log if n[0] == "apply"]
    assert applies == [CF[4 - i] for i in range(1, 5) if i not in raw_levels]
    assert all(n[1][2] == (drop == "active") for n in f.log if n[0] == "apply")


def test_encoder_top_only_is_unchanged_and_f32_never_goes_raw(fake):
    from littlegan_amd.model import Encoder
    f = fake(zn_ok=(1, 2, 3), raw_ok=())            # top_only asks the kernel's predicate, never the Adjuster's adoption rule
    outs = Encoder(args_of())(torch.zeros(OWN, SIDE, SIDE, 3), None, top_only=True)
    assert outs[:3] == [None, None, None] and f.names().count("conv_zn") == 3 and f.names().count("apply") == 1 and not f.asked
    f = fake(zn_ok=(1, 2, 3), raw_ok=())            # ... and a batch the rule does not adopt stays on the apply route
    outs = Encoder(args_of())(torch.zeros(OWN, SIDE, SIDE, 3), None, tails=tails_of(), raw_skips=True)
    assert "conv_zn" not in f.names() and f.names().count("apply") == 4 and f.asked == [("raw", 1), ("raw", 2)]
    f = fake(zn_ok=(1, 2, 3))
    outs = Encoder(args_of("f32"))(torch.zeros(OWN, SIDE, SIDE, 3), None, tails=tails_of(), raw_skips=True)
    assert "conv_zn" not in f.names() and not any(isinstance(o[0], FakeRaw) for o in outs)


def decoder_inputs(kinds):
    """level-1 input pair + the skips of levels 1..3 as (own part, handed-over part) pairs; kinds: 'raw' / 'map' of each own part"""
    B, side = OWN + TAIL, SIDE // 16
    x = (torch.zeros(B, side, side, CF[0]), torch.zeros(B, side, side, CF[0], dtype=torch.bfloat16))
    add = [None]
    for i, kind in zip((1, 2, 3), kinds):
        side *= 2
        own = torch.zeros(OWN, side, side, CF[i], dtype=torch.bfloat16)
        add.append((FakeRaw(own, torch.zeros(OWN, 8)) if kind == "raw" else own, torch.zeros(TAIL, side, side, CF[i], dtype=torch.bfloat16)))
    return [x, add]


@pytest.mark.parametrize("ns_ok", [(), (1,), (2,), (3,), (2, 3), (1, 2, 3)])
@pytest.mark.parametrize("kinds", [("map", "map", "map"), ("map", "raw", "raw"), ("raw", "raw", "raw")])
@pytest.mark.parametrize("no_wgrad", [True, False])
def test_decoder_routing(fake, ns_ok, kinds, no_wgrad):
    from littlegan_amd.model import Decoder
    f = fake(ns_ok=ns_ok)
    dec = Decoder(args_of())
    ctx = {}
    x, x16 = dec(decoder_inputs(kinds), ctx, no_wgrad=no_wgrad)
    fused = [i for i in (1, 2, 3) if no_wgrad and i in ns_ok]       # levels whose norm + skip pass is left to the next conv
    convs = [n for n in f.log if n[0] in ("convT", "convT_ns")]
    want = []
    for i in range(1, 5):
        if (i - 1) in fused:
            want.append(("convT_ns", (CF[i], (kinds[i - 2], "map"))))
        else:
            want.append(("convT", CF[i]))
    assert convs == want
    # a level that is not fused applies its skip part by part, a raw part through the raw-skip form; level 4 has no skip
    applies = [n[1][:2] for n in f.log if n[0] == "apply"]
    want_applies = []
    for i in range(1, 5):
        if i not in fused:
            want_applies += [(CF[i], kinds[i - 1]), (CF[i], "map")] if i < 4 else [(CF[4], "none")]
    assert applies == want_applies
    for i in range(1, 5):   # the level above a fused level keeps no input; every level keeps z and its statistics
        xin, z, st, xin16 = ctx["dec"][i - 1]
        assert (xin is None and xin16 is None) == ((i - 1) in fused) and z is not None and st is not None
    assert x16 is not None


def test_decoder_f32_path_and_skipless_levels_are_never_fused(fake):
    from littlegan_amd.model import Decoder
    f = fake(ns_ok=(1, 2, 3))
    B, side = 2, SIDE // 16
    Decoder(args_of())([(torch.zeros(B, side, side, CF[0]), torch.zeros(B, side, side, CF[0], dtype=torch.bfloat16)), [None] * 4], {},
                       no_wgrad=True)
    assert "convT_ns" not in f.names()          # the Generator's call shape: no skip, nothing to fuse
    f = fake(ns_ok=(1, 2, 3))
    inp = decoder_inputs(("map", "map", "map"))
    inp[0] = (inp[0][0], None)
    inp[1] = [None] + [tuple(p.float() for p in pair) for pair in inp[1][1:]]
    Decoder(args_of("f32"))(inp, {}, no_wgrad=True)
    assert "convT_ns" not in f.names()


@pytest.mark.parametrize("zn_ok,ns_ok", list(itertools.product([(), (1, 2)], [(), (2, 3)])))
@pytest.mark.parametrize("drop", [None, "active"])
def test_adjuster_asks_for_both(fake, zn_ok, ns_ok, drop):
    """Adjuster.__call__ with handed-over encoder maps: its own encoder pass may hand levels 1 and 2 over raw, its decoder may leave
    levels 2 and 3 to the next conv; an active dropout mask puts the encoder back on the apply route (the decoder is not affected)"""
    from littlegan_amd.model import Adjuster, Decoder, Discriminator, Encoder, Generator
    f = fake(zn_ok=zn_ok, ns_ok=ns_ok)
    a = args_of()
    adj = Adjuster(a, Discriminator(a, Encoder(a)), Generator(a, Decoder(a)))
    ctx = {}
    d = None if drop is None else FakeDrop(True)
    adj([torch.zeros(OWN, SIDE, SIDE, 3), torch.zeros(OWN + TAIL, a.cond_dim)], ctx, enc_tails=tails_of(), drop=d)
    raw_levels = [i for i in (1, 2) if i in zn_ok and drop is None]
    assert [n for n in f.log if n[0] == "conv_zn"] == [("conv_zn", CF[4 - i - 1]) for i in raw_levels]
    kind = lambda enc_level: "raw" if enc_level in raw_levels else "map"   # decoder level i adds encoder level 4 - i
    fused = [n[1] for n in f.log if n[0] == "convT_ns"]
    assert fused == [(CF[i + 1], (kind(4 - i), "map")) for i in (2, 3) if i in ns_ok]
    raw_applies = [n[1][0] for n in f.log if n[0] == "apply" and n[1][1] == "raw"]
    assert raw_applies == [CF[i] for i in (2, 3) if kind(4 - i) == "raw" and i not in ns_ok]
    assert f.names()[-1] == "final_raw"
    assert ctx["dec"][3][1] is not None and ctx["dec"][3][2] is not None   # what backward_own starts from
    # without handed-over maps the encoder pass is the plain one
    f = fake(zn_ok=zn_ok, ns_ok=ns_ok)
    adj([torch.zeros(OWN, SIDE, SIDE, 3), torch.zeros(OWN, a.cond_dim)], {})
    assert "conv_zn" not in f.names()
