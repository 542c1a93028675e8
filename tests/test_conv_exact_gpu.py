"""The convolution kernels in exact integer arithmetic, on every route.

Every operand (x, w, bias, dy, the prior contents of dw / db) is an integer in [-4, 4] times a power-of-two unit, drawn iid per
element from a seeded generator.  An integer that small is exact in bf16 and in fp32, every product is exact, and every partial sum
in ANY order stays below 2^24 units (tests/test_conv_exact_cpu.py checks that on the oracle alone), so

  * an fp32 result (y, dx, dw, db) must be np.array_equal to the fp64 oracle, at dtype 0 and at dtype 1;
  * a bf16 result (z16, g16, dx16) must be bit-equal to O.bf16_round(exact) — and because integer sums DO land half-way between two
    bf16 values (several per cent of the outputs, in both directions), the round-to-nearest-even rule of every bf16 store is checked;
  * the final layer's image is tanh of an exact, moderate pre-activation (|pre| <= 2): 1e-5 absolute against fp64 tanh.

Every case names the kernel it must reach (lg_clear_kernel before the call, ops.last_kernel() after it).  The persistent kernels are
run twice, as launched and under a one-CU budget (lg_set_reserved_cus(lg_device_cus() - 1)): there the grid is one or two blocks and a
block walks many items (ring phase, LDS reuse, prefetch of the next item, per-item record slot), both runs must be exact and equal
bit for bit, moment and NormPartials records included.

The case tables below are plain data; tests/test_conv_exact_cpu.py imports them and checks the conditions of the form on the CPU.

The test bodies are helpers that take the routes to assert (run_conv32, run_persistent, run_zn, run_wgrad, run_final, run_final_z16,
run_p16) and return their problems: the tests here call them with the routes of the tables, tests/test_kill_switch_gpu.py calls them in
a process with a kill switch set, with the routes that take over there."""
import functools
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import np_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16, F64, U8 = torch.float32, torch.bfloat16, torch.float64, torch.uint8
ALPHA = 0.25        # LeakyReLU slope of the hand-made norm records: a power of two, so the activated map stays a multiple of 1/8
R = 4               # operands are integers in [-R, R] (times a unit)
W_FINAL = 2.0 ** -10   # unit of the final layer's weights and bias: the tanh pre-activation is exact and moderate
TANH_TOL = 1e-5     # absolute, image against fp64 tanh of the exact pre-activation (the figure of the integer form of heads_fwd)
MOM_TOL = 2e-5      # fused moments against the moments of the exact map (tests/test_memory_contract_gpu.py, _moments_ok)

IG, HALO, D3, U3, U4 = "conv_igemm_kernel", "conv_halo_kernel", "conv_down3_kernel", "conv_up3_kernel", "conv_up4_kernel"


# ------------------------------------------------------------------------------------------------------------------ the form
def crc(*x):
    return zlib.crc32(repr(x).encode())


def ints(seed, *shape, unit=1.0, r=R):
    """iid integers in [-r, r] times `unit` (fp64)"""
    return np.random.default_rng(seed).integers(-r, r + 1, shape).astype(np.float64) * unit


def records(seed, B):
    """hand-made statistics records [B, 8] = {mu_hi, sigma, a, beta, mu_lo, 0, 0, 0}, different per sample: mu_hi and beta integers,
    a in {0.5, 1, 2}, mu_lo = 0"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((B, 8), np.float64)
    rec[:, 0] = rng.integers(-2, 3, B)
    rec[:, 1] = 1.0
    rec[:, 2] = np.array([0.5, 1.0, 2.0])[(rng.integers(0, 3) + np.arange(B)) % 3]
    rec[:, 3] = rng.integers(-2, 3, B)
    return rec


def activated(z, rec):
    """leaky(a((z - mu_hi) - mu_lo) + beta) of an integer map under hand-made records: every intermediate is a multiple of 1/8 below
    32, exact in fp32 and in bf16"""
    s = (slice(None),) + (None,) * (z.ndim - 1)
    y = rec[:, 2][s] * ((z - rec[:, 0][s]) - rec[:, 4][s]) + rec[:, 3][s]
    return np.where(y > 0, y, ALPHA * y)


class Exact:
    """operands, exact results and the conditions of one case: want[name] the fp64 oracle result, bound[name] the oracle on the
    absolute operands (the largest partial sum any order can meet), unit[name] the unit the result is a multiple of, bf16: names of
    the results a kernel stores as bf16, pre: the tanh pre-activation (final layer)"""

    def __init__(self):
        self.op, self.want, self.bound, self.unit, self.bf16, self.pre = {}, {}, {}, {}, [], None

    def add(self, name, want, bound, unit=1.0, bf16=False):
        self.want[name], self.bound[name], self.unit[name] = want, float(np.abs(bound).max()), unit
        if bf16:
            self.bf16.append(name)


def _down(x, w, b):
    return O.conv2d(x, w, b, 2)


def _up(x, w, b):
    return O.conv2d_transpose(x, w, b, 2)


# ---- gather, halo and patch kernels through the fp32 entry points: forward, data gradient, forward with moments
CONV32 = []   # (kind, (B, Hs, Ws, cb, cs), dtype, {call: route})


def conv32(kind, case, routes):
    for dt, r in enumerate(routes):
        if r is not None:
            CONV32.append((kind, case, dt, r))


def _r(fwd, dgrad, stats=None, stats16=None, dgrad16=None):
    """routes of a CONV32 case: forward, data gradient, forward with moments (default: the forward's kernel); bf16 dtype also the two
    calls with the bf16 mirror of the source beside the fp32 operand (None: not run)"""
    return dict(fwd=fwd, dgrad=dgrad, stats=fwd if stats is None else stats, stats16=stats16, dgrad16=dgrad16)


def _hn(dt, mode):
    return f"{HALO}<{'bf16' if dt else 'f32'},{mode}>"


KS = "UP,K-sliced"
conv32("down", (3, 5, 6, 32, 64), [_r(IG + "<DOWN>", IG + "<UP>")] * 2)                               # gather kernel, odd map
conv32("up", (3, 5, 6, 32, 64), [_r(IG + "<UP>", IG + "<DOWN>")] * 2)
conv32("down", (3, 7, 5, 3, 64), [_r(IG + "<PATCH>", IG + "<UP>")] * 2)                               # 3-channel patch, odd map
conv32("down", (2, 16, 16, 3, 64), [_r(IG + "<PATCH>", ""), _r(IG + "<PATCH>", "", "patch_p16_kernel<2,64>", dgrad16="up_p16_kernel")])
conv32("down", (3, 8, 8, 32, 64), [_r(_hn(0, "DOWN"), _hn(0, KS)), _r(_hn(1, "DOWN"), _hn(1, KS), stats16=_hn(1, "DOWN"), dgrad16=HALO + "<UP,resident>")])
conv32("down", (2, 8, 8, 128, 64), [_r(_hn(0, "DOWN"), _hn(0, KS)), None])   # f32, four channel chunks: the contraction split over two blocks adding into the zeroed result
conv32("up", (2, 4, 4, 32, 32), [_r(_hn(0, KS), _hn(0, "DOWN")), _r(_hn(1, KS), _hn(1, "DOWN"))])
conv32("up", (5, 2, 2, 64, 64), [_r(_hn(0, KS), IG + "<DOWN>"), _r(_hn(1, KS), IG + "<DOWN>")])       # 1 x 1 result map of the data gradient
conv32("up", (2, 8, 9, 64, 128), [_r(IG + "<UP>", IG + "<DOWN>")] * 2)                                # transposed conv, odd width
conv32("up", (2, 3, 3, 256, 384), [_r(IG + "<UP>", IG + "<DOWN>")] * 2)                               # the deepest contraction
conv32("up", (1, 8, 16, 32, 64), [_r(HALO + "<f32,UP,resident>", _hn(0, "DOWN")),                     # resident forms: f32 at 32 columns,
                                  _r(_hn(1, KS), _hn(1, "DOWN"), stats16=HALO + "<UP,resident>")])    # bf16 from the mirror at 64 channels
conv32("up", (2, 16, 16, 64, 32), [None, _r(_hn(1, KS), _hn(1, "DOWN"), stats16=_hn(1, KS), dgrad16=_hn(1, "DOWN"))])   # K-sliced from the mirror (32 channels)


@functools.lru_cache(maxsize=None)
def exact_conv32(kind, case):
    B, Hs, Ws, cb, cs = case
    s = crc("conv32", kind, case)
    big, small = (B, 2 * Hs, 2 * Ws, cb), (B, Hs, Ws, cs)
    down = kind == "down"
    e = Exact()
    x, w, b, dy = ints(s, *(big if down else small)), ints(s + 1, 5, 5, cb, cs), ints(s + 2, cs if down else cb), ints(s + 3, *(small if down else big))
    e.op = dict(x=x, w=w, b=b, dy=dy)
    ax, aw, ab, ady = np.abs(x), np.abs(w), np.abs(b), np.abs(dy)
    if down:
        e.add("y", _down(x, w, b), _down(ax, aw, ab))
        e.add("dx", O.conv2d_bwd(x, w, dy, 2)[0], O.conv2d_bwd(ax, aw, ady, 2)[0])
    else:
        e.add("y", _up(x, w, b), _up(ax, aw, ab))
        e.add("dx", O.conv2d_transpose_bwd(x, w, dy, 2)[0], O.conv2d_transpose_bwd(ax, aw, ady, 2)[0])
    return e


# ---- bf16 activation path: the persistent kernels (and the halo kernel's bf16 stores), as launched and under a one-CU budget
PERSISTENT = [  # (kind, (B, Hm, Wm, Cs, N), route); down: x [B,2Hm,2Wm,Cs] -> [B,Hm,Wm,N]; up: x [B,Hm,Wm,Cs] -> [B,2Hm,2Wm,N]
    ("down", (2, 8, 8, 32, 128), D3 + "<PAIR>"),
    ("down", (10, 8, 8, 32, 128), D3 + "<PAIR>"),          # 5 items
    ("down", (2, 8, 8, 32, 256), D3 + "<PAIR>"),           # two column tiles
    ("down", (1, 8, 16, 32, 64), D3 + "<NW=64>"),          # one tile holding all four borders
    ("down", (1, 24, 48, 32, 64), D3 + "<NW=64>"),         # 3 x 3 tile map, one border-free tile: 9 items
    ("down", (3, 8, 16, 32, 192), D3 + "<NW=64>"),         # three column tiles, odd batch: 9 items
    ("down", (1, 8, 16, 32, 128), D3 + "<NW=128>"),
    ("down", (1, 24, 48, 32, 128), D3 + "<NW=128>"),       # 9 items
    ("down", (3, 8, 16, 64, 256), D3 + "<NW=128>"),        # two column tiles, odd batch, four 16-channel slices: 6 items
    ("down", (3, 8, 8, 32, 128), HALO + "<bf16,DOWN>"),    # odd batch on the 8 x 8 level: the halo kernel's bf16 stores
    ("up", (1, 8, 16, 64, 128), U4),
    ("up", (1, 24, 48, 64, 128), U4),                      # 9 items per class
    ("up", (3, 8, 16, 128, 256), U4),                      # two 64-channel slices, two column tiles, odd batch: 6 items per class
    ("up", (2, 8, 8, 64, 128), U4 + "<PAIR>"),
    ("up", (10, 8, 8, 64, 128), U4 + "<PAIR>"),            # 5 items per class
    ("up", (2, 8, 8, 128, 256), U4 + "<PAIR>"),
    ("up", (1, 8, 16, 128, 64), U3 + "<128,64>"),
    ("up", (1, 24, 48, 128, 64), U3 + "<128,64>"),         # 9 items
    ("up", (3, 8, 16, 128, 64), U3 + "<128,64>"),          # odd batch
    ("up", (1, 8, 16, 64, 32), U3 + "<64,32,4w>"),
    ("up", (1, 24, 48, 64, 32), U3 + "<64,32,4w>"),        # 9 items
    ("up", (3, 8, 16, 64, 32), U3 + "<64,32,4w>"),         # odd batch
]


@functools.lru_cache(maxsize=None)
def exact_persistent(kind, case):
    B, Hm, Wm, Cs, N = case
    s = crc("persistent", kind, case)
    down = kind == "down"
    src = (B, 2 * Hm, 2 * Wm, Cs) if down else (B, Hm, Wm, Cs)
    dst = (B, Hm, Wm, N) if down else (B, 2 * Hm, 2 * Wm, N)
    e = Exact()
    x, w, b = ints(s, *src), ints(s + 1, *((5, 5, Cs, N) if down else (5, 5, N, Cs))), ints(s + 2, N)
    e.op = dict(x=x, w=w, b=b, zl=ints(s + 3, *dst), rec=records(s + 4, B))
    f = _down if down else _up
    g, ag = f(x, w, np.zeros(N)), f(np.abs(x), np.abs(w), np.zeros(N))
    e.add("z16", g + b, ag + np.abs(b), bf16=True)
    e.add("g16", g, ag, bf16=True)   # the matching data gradient: the same contraction without bias
    return e


# ---- NORM forms: the operand is normalised while it is staged, from hand-made records
ZN = [(2, 8, 16, 32, 128), (1, 24, 48, 32, 128), (3, 8, 16, 32, 256)]   # conv2d_s2_fwd_stats_zn: (B, Hm, Wm, Cs, N)
ZN_ROUTE = D3 + "<NW=128,NORM>"


@functools.lru_cache(maxsize=None)
def exact_zn(case):
    B, Hm, Wm, Cs, N = case
    s = crc("zn", case)
    e = Exact()
    z, w, b, rec = ints(s, B, 2 * Hm, 2 * Wm, Cs), ints(s + 1, 5, 5, Cs, N), ints(s + 2, N), records(s + 3, B)
    h = activated(z, rec)
    e.op = dict(z=z, w=w, b=b, rec=rec, h=h)
    e.add("z16", _down(h, w, b), _down(np.abs(h), np.abs(w), np.abs(b)), unit=0.125, bf16=True)
    return e


# ---- weight gradients
WGRAD = [  # (form, (B, Hm, Wm, cb, cs), dtype, mirrors, route); mirrors: "none" fp32 operands, "both" bf16 mirrors alone, "with" both
    ("conv", (3, 5, 6, 32, 64), 0, "none", "wgrad_kernel<f32,per-tap>"),
    ("conv", (3, 5, 6, 32, 64), 1, "none", "wgrad_kernel<bf16,per-tap>"),
    ("conv", (3, 5, 6, 32, 64), 1, "with", "wgrad_kernel<bf16,per-tap>"),
    ("convT", (3, 5, 6, 32, 64), 0, "none", "wgrad_kernel<f32,per-tap>"),
    ("convT", (3, 5, 6, 32, 64), 1, "with", "wgrad_kernel<bf16,per-tap>"),
    ("conv", (3, 8, 8, 64, 128), 1, "both", "wgrad_kernel<bf16,per-tap>"),     # odd batch on the 8 x 8 level: back to the per-tap kernel
    ("conv", (2, 3, 3, 256, 384), 0, "none", "wgrad_kernel<f32,per-tap>"),     # 128 x 128 tiles
    ("conv", (2, 3, 3, 256, 384), 1, "none", "wgrad_kernel<bf16,per-tap>"),
    ("conv", (3, 7, 5, 3, 64), 0, "none", "wgrad_kernel<PATCH>"),              # 3-channel, odd map
    ("conv", (3, 7, 5, 3, 64), 1, "none", "wgrad_kernel<PATCH>"),
    ("conv", (2, 12, 16, 32, 192), 0, "none", "wgrad_at32_kernel<16,4>"),      # height a multiple of 4, not of 8
    ("convT", (2, 12, 16, 32, 192), 0, "none", "wgrad_at32_kernel<16,4>"),
    ("conv", (2, 8, 8, 32, 64), 0, "none", "wgrad_at32_kernel<8,8>"),
    ("conv", (3, 8, 8, 64, 128), 0, "none", "wgrad_at32_kernel<8,8>"),         # odd batch, four units
    ("conv", (9, 8, 16, 256, 512), 0, "none", "wgrad_at32_kernel<16,4>"),      # 64 units: 18 items over 4 splits, the last one ragged
    ("conv", (2, 4, 32, 32, 64), 1, "both", "wgrad_at_kernel<32,4>"),
    ("convT", (2, 4, 32, 32, 64), 1, "both", "wgrad_at_kernel<32,4>"),
    ("conv", (2, 16, 16, 32, 64), 1, "both", "wgrad_at_kernel<16,8>"),
    ("convT", (3, 8, 16, 64, 128), 1, "both", "wgrad_at_kernel<16,8>"),
    ("conv", (2, 8, 8, 64, 128), 1, "both", "wgrad_at_kernel<8,8>"),
    ("conv", (9, 8, 16, 256, 512), 1, "both", "wgrad_at_kernel<16,8>"),        # 64 units: 9 items over 3 splits, three items per block
    ("conv", (9, 4, 32, 256, 512), 1, "both", "wgrad_at_kernel<32,4>"),
    ("conv", (26, 8, 8, 256, 512), 1, "both", "wgrad_at_kernel<8,8>"),         # 13 sample pairs over 4 splits, the last one ragged
    ("conv", (2, 16, 16, 3, 32), 0, "none", "n3_wgrad_kernel<f32>"),           # 3-channel all-taps kernels, conv1 form
    ("conv", (2, 16, 16, 3, 64), 0, "none", "n3_wgrad_kernel<f32>"),
    ("conv", (2, 16, 16, 3, 32), 1, "n3", "n3_wgrad16_kernel<1>"),             # "n3": fp32 image + the mirror of the wide operand alone
    ("conv", (3, 8, 32, 3, 64), 1, "n3", "n3_wgrad16_kernel<2>"),
]


@functools.lru_cache(maxsize=None)
def exact_wgrad(case):
    B, Hm, Wm, cb, cs = case
    s = crc("wgrad", case)
    e = Exact()
    big, small, prior = ints(s, B, 2 * Hm, 2 * Wm, cb), ints(s + 1, B, Hm, Wm, cs), ints(s + 2, 5, 5, cb, cs)
    e.op = dict(big=big, small=small, prior=prior)
    dw = O.conv_bwd_filter(big, small, 2, 5)   # (what O.conv2d_bwd(...)[1] is, without its data gradient against zero weights)
    adw = O.conv_bwd_filter(np.abs(big), np.abs(small), 2, 5)
    e.add("dw", dw, adw)
    e.add("dw_acc", prior + dw, np.abs(prior) + adw)
    return e


# ---- final layer tanh(Conv2DTranspose(3, 5, 1, same)) and its backward; the bf16-source 3-channel kernels of n3_pgemm.hip
FINAL = [  # ((B, H, W, cs), dtype, src, {call: route}); src "f32": fp32 operands; "m16": the bf16 mirror of x alone (bf16 path)
    ((2, 6, 10, 32), 0, "f32", dict(fwd=IG + "<S1T>", dx=IG + "<PATCH>", dw="wgrad_kernel<PATCH>")),
    ((2, 6, 10, 32), 1, "f32", dict(fwd=IG + "<S1T>", dx=IG + "<PATCH>", dw="wgrad_kernel<PATCH>")),
    ((1, 4, 4, 64), 0, "f32", dict(fwd=HALO + "<S1T>", dx=IG + "<PATCH>", dw="wgrad_kernel<PATCH>")),
    ((1, 4, 4, 64), 1, "f32", dict(fwd=HALO + "<S1T>", dx=IG + "<PATCH>", dw="wgrad_kernel<PATCH>")),
    ((2, 16, 16, 32), 0, "f32", dict(fwd="", dx=IG + "<PATCH>", dw="n3_wgrad_kernel<f32>")),      # forward: the unnamed VALU kernel
    ((2, 16, 16, 32), 1, "f32", dict(fwd="", dx="patch_p16_kernel<1,32>", dw="n3_wgrad_kernel<f32>")),
    ((2, 16, 16, 32), 1, "m16", dict(fwd="s1t_fwd_rows_kernel<32>", dx="patch_p16_kernel<1,32>", nf="patch_p16_kernel<1,32,nf>", dw="n3_wgrad16_kernel<1,16>")),
    ((1, 48, 48, 32), 1, "m16", dict(fwd="s1t_fwd_rows_kernel<32>", dx="patch_p16_kernel<1,32>", nf="patch_p16_kernel<1,32,nf>", dw="n3_wgrad16_kernel<1,16>")),   # 3 x 3 tiles: 9 items
    ((1, 80, 16, 32), 1, "m16", dict(fwd="s1t_fwd_rows_kernel<32>", dx="patch_p16_kernel<1,32>", dw="n3_wgrad16_kernel<1,16>")),   # a ragged last row block (64 + 16 rows)
    ((2, 16, 16, 64), 1, "m16", dict(fwd="s1t_fwd_p16_kernel", dw="n3_wgrad16_kernel<2>")),
    ((1, 48, 48, 64), 1, "m16", dict(fwd="s1t_fwd_p16_kernel", dw="n3_wgrad16_kernel<2>")),
]
FINAL_Z16 = [(2, 16, 16, 32), (1, 80, 48, 32), (3, 8, 32, 32)]   # convT_s1_tanh_fwd_z16: (B, H, W, C), NORM form of the row kernel
FINAL_Z16_ROUTE = "s1t_fwd_rows_kernel<32,NORM>"


@functools.lru_cache(maxsize=None)
def exact_final(case):
    B, H, W, cs = case
    s = crc("final", case)
    e = Exact()
    x, w, b, dpre = ints(s, B, H, W, cs), ints(s + 1, 5, 5, 3, cs, unit=W_FINAL), ints(s + 2, 3, unit=W_FINAL), ints(s + 3, B, H, W, 3)
    pw, pb = ints(s + 4, 5, 5, 3, cs), ints(s + 5, 3)
    e.op = dict(x=x, w=w, b=b, dpre=dpre, pw=pw, pb=pb, zl=ints(s + 6, B, H, W, cs), rec=records(s + 7, B))
    e.pre = O.conv2d_transpose(x, w, b, 1)
    e.add("pre", e.pre, O.conv2d_transpose(np.abs(x), np.abs(w), np.abs(b), 1), unit=W_FINAL)
    dx, dw, db = O.conv2d_transpose_bwd(x, w, dpre, 1)
    adx, adw, adb = O.conv2d_transpose_bwd(np.abs(x), np.abs(w), np.abs(dpre), 1)
    e.add("dx", dx, adx, unit=W_FINAL)
    e.add("dx16", dx, adx, unit=W_FINAL, bf16=True)
    e.add("dw", dw, adw)
    e.add("db", db, adb)
    e.add("dw_acc", pw + dw, np.abs(pw) + adw)
    e.add("db_acc", pb + db, np.abs(pb) + adb)
    return e


@functools.lru_cache(maxsize=None)
def exact_final_z16(case):
    B, H, W, C = case
    s = crc("finalz16", case)
    e = Exact()
    z, w, b, rec = ints(s, B, H, W, C), ints(s + 1, 5, 5, 3, C, unit=W_FINAL), ints(s + 2, 3, unit=W_FINAL), records(s + 3, B)
    h = activated(z, rec)
    e.op = dict(z=z, w=w, b=b, rec=rec, h=h)
    e.pre = O.conv2d_transpose(h, w, b, 1)
    e.add("pre", e.pre, O.conv2d_transpose(np.abs(h), np.abs(w), np.abs(b), 1), unit=W_FINAL / 8)
    return e


# ---- conv1 from the fp32 image on the bf16 MFMA, and its data gradient from the mirror (n3_pgemm.hip; persistent grids)
P16 = [(2, 16, 16, 64), (1, 48, 48, 64), (5, 16, 16, 64)]   # (B, Hs, Ws, N): image [B,2Hs,2Ws,3]; 3 x 3 tile map; odd batch
P16_FWD, P16_UP = "patch_p16_kernel<2,64>", "up_p16_kernel"


@functools.lru_cache(maxsize=None)
def exact_p16(case):
    B, Hs, Ws, N = case
    s = crc("p16", case)
    e = Exact()
    # the contraction is only 75 products deep (|sum| rarely reaches 256, where bf16 starts to round): a bias unit of 64 moves a third of
    # the outputs into [256, 512), where every odd integer is a tie
    x, w, b, dy = ints(s, B, 2 * Hs, 2 * Ws, 3), ints(s + 1, 5, 5, 3, N), ints(s + 2, N, unit=64.0), ints(s + 3, B, Hs, Ws, N)
    e.op = dict(x=x, w=w, b=b, dy=dy)
    z, az = _down(x, w, b), _down(np.abs(x), np.abs(w), np.abs(b))
    e.add("z", z, az)
    e.add("z16", z, az, bf16=True)
    e.add("dx", O.conv2d_bwd(x, w, dy, 2)[0], O.conv2d_bwd(np.abs(x), np.abs(w), np.abs(dy), 2)[0])
    return e


# BWDNORM: (B, s_h, s_w, cb, cs) of convT_s2_dgrad_bn; the second shape has 6 tiles
BWDNORM = [(2, 8, 16, 32, 64), (3, 16, 32, 32, 64)]
BWDNORM_ROUTE = (D3 + "<NW=64,BWDNORM>", D3 + "<NW=64>")

# Kernel names of the ledger files that no exact case asserts, each with its reason (tests/test_conv_exact_cpu.py)
NOT_EXACT = {
    D3 + "<NW=64,BWDNORM>": "its per-sample coefficients come from a device function (lg_instnorm_bwd_coef), so no operand set makes dz exact; "
                            "pinned bit for bit to instnorm_bwd + conv_down3_kernel<NW=64> in test_bwdnorm_equals_two_pass_chain, "
                            "and that two-pass kernel is exact here",
}


def all_cases():
    """(id, routes asserted, Exact factory) of every exact case: what tests/test_conv_exact_cpu.py walks"""
    out = []
    for kind, case, dt, r in CONV32:
        out.append((f"conv32-{kind}-{_cid(case)}-{_dn(dt)}", [v for v in r.values() if v], functools.partial(exact_conv32, kind, case)))
    for kind, case, route in PERSISTENT:
        out.append((f"persistent-{kind}-{_cid(case)}", [route], functools.partial(exact_persistent, kind, case)))
    for case in ZN:
        out.append((f"zn-{_cid(case)}", [ZN_ROUTE], functools.partial(exact_zn, case)))
    for form, case, dt, mirrors, route in WGRAD:
        out.append((f"wgrad-{form}-{_cid(case)}-{_dn(dt)}-{mirrors}", [route], functools.partial(exact_wgrad, case)))
    for case, dt, src, r in FINAL:
        out.append((f"final-{_cid(case)}-{_dn(dt)}-{src}", [v for v in r.values() if v], functools.partial(exact_final, case)))
    for case in FINAL_Z16:
        out.append((f"final-z16-{_cid(case)}", [FINAL_Z16_ROUTE], functools.partial(exact_final_z16, case)))
    for case in P16:
        out.append((f"p16-{_cid(case)}", [P16_FWD, P16_UP], functools.partial(exact_p16, case)))
    return out


def _cid(case):
    return "x".join(map(str, case))


def _dn(dt):
    return "bf16" if dt else "f32"


# ------------------------------------------------------------------------------------------------------------------ the harness
@pytest.fixture(scope="module")
def ops():
    from littlegan_amd import ops as _ops
    return _ops


def dev(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def f64(t):
    return t.detach().double().cpu().numpy()


def bits(t):
    return t.detach().contiguous().reshape(-1).view(U8).cpu()


def explain(name, got, want):
    """'' if got == want element for element, else: how many differ, the first index (b, i, j, n), got and want there, and the
    8 x 16 pixel tile and the column tiles it lies in"""
    got = f64(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
    if got.shape != want.shape:
        return f"{name}: shape {got.shape}, want {want.shape}"
    ne = got != want
    if not ne.any():
        return ""
    idx = tuple(int(v) for v in np.argwhere(ne)[0])
    msg = f"{name}: {int(ne.sum())} of {ne.size} elements differ; first at {idx}: got {float(got[idx])!r}, want {float(want[idx])!r}"
    if got.ndim == 4 and not name.startswith(("dw", "db")):
        b, i, j, n = idx
        msg += f" (8 x 16 tile ({i // 8}, {j // 16}) of sample {b}, column tile {n // 128} of 128 / {n // 64} of 64)"
    return msg


class Route:
    """lg_clear_kernel before a call, ops.last_kernel() after it (launched() of tests/test_skinny_gpu.py)"""

    def __init__(self, ops, problems):
        self.ops, self.problems = ops, problems
        ops._lib.load().lg_clear_kernel()

    def __call__(self, label, want):
        got = self.ops.last_kernel()
        if got != want:
            self.problems.append(f"route of {label}: {got!r}, want {want!r}")
        self.ops._lib.load().lg_clear_kernel()


class one_cu:
    """the persistent grids sized to ONE CU (1-2 blocks of conv_down3 / conv_up3 / conv_up4, 2-4 of the n3_pgemm kernels)"""

    def __init__(self, ops, on):
        self.lib, self.on = ops._lib.load(), on

    def __enter__(self):
        if self.on:
            assert self.lib.lg_set_reserved_cus(self.lib.lg_device_cus() - 1) == 0

    def __exit__(self, *a):
        assert self.lib.lg_set_reserved_cus(0) == 0


def moments_problem(name, st, exact):
    """fused moments against the moments of the exact map; the mean is measured against the spread it is subtracted from"""
    B = exact.shape[0]
    ef = exact.reshape(B, -1)
    mu, sg = ef.mean(1), ef.std(1)
    s = f64(st)
    em, es = np.abs(s[:, 0] + s[:, 4] - mu).max() / max(np.abs(mu).max(), sg.max()), np.abs(s[:, 1] - sg).max() / sg.max()
    return "" if em < MOM_TOL and es < MOM_TOL else f"{name}: moments off by {em:.2e} (mean) / {es:.2e} (sigma), bound {MOM_TOL}"


def finish(problems):
    problems = [p for p in problems if p]
    if problems:
        pytest.fail("\n".join(problems), pytrace=False)


def same_bits(name, runs):
    """the results of the run as launched and of the run under the one-CU budget, bit for bit"""
    out = []
    a, b = runs
    for k in a:
        if not torch.equal(a[k], b[k]):
            out.append(f"{name}: '{k}' differs between the grid as launched and the one-CU grid ({int((a[k] != b[k]).sum())} bytes)")
    return out


# ------------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("kind,case,dtype,routes", CONV32, ids=[f"{k}-{_cid(c)}-{_dn(d)}" for k, c, d, _ in CONV32])
def test_gather_halo_patch_exact(ops, kind, case, dtype, routes):
    finish(run_conv32(ops, kind, case, dtype, routes))


def run_conv32(ops, kind, case, dtype, routes):
    """body of test_gather_halo_patch_exact: the problems of one CONV32 case whose calls must reach `routes`"""
    B, Hs, Ws, cb, cs = case
    e = exact_conv32(kind, case)
    down = kind == "down"
    P = []
    x, b, dy = dev(e.op["x"]), dev(e.op["b"]), dev(e.op["dy"])
    pack = ops.conv_pack(dev(e.op["w"]), cb, cs, dtype)
    gm, bt = torch.ones(1, device="cuda"), torch.zeros(1, device="cuda")
    fwd, dgrad, fstats = (ops.conv2d_s2_fwd, ops.conv2d_s2_dgrad, ops.conv2d_s2_fwd_stats) if down else \
                         (ops.convT_s2_fwd, ops.convT_s2_dgrad, ops.convT_s2_fwd_stats)
    nin, nout = (cs, cb) if down else (cb, cs)   # channel argument of the forward / of the data gradient
    rt = Route(ops, P)
    y = fwd(x, pack, b, nin, dtype)
    rt("fwd", routes["fwd"])
    dx = dgrad(dy, pack, nout, dtype)
    rt("dgrad", routes["dgrad"])
    z, st = fstats(x, pack, b, nin, dtype, gm, bt)
    rt("stats", routes["stats"])
    P += [explain("y", y, e.want["y"]), explain("dx", dx, e.want["dx"]), explain("z (forward with moments)", z, e.want["y"])]
    if st is not None:
        P.append(moments_problem("stats", ops.stats_tensor(st), e.want["y"]))
    if routes["stats16"]:   # the bf16 mirror beside the fp32 source: an integer's mirror is the integer
        z, st = fstats(x, pack, b, nin, dtype, gm, bt, x16=x.to(BF16))
        rt("stats16", routes["stats16"])
        P.append(explain("z (forward with moments, from the mirror)", z, e.want["y"]))
        if st is not None:
            P.append(moments_problem("stats16", ops.stats_tensor(st), e.want["y"]))
    if routes["dgrad16"]:
        dx = dgrad(dy, pack, nout, dtype, dy16=dy.to(BF16))
        rt("dgrad16", routes["dgrad16"])
        P.append(explain("dx (from the mirror)", dx, e.want["dx"]))
    return P


@pytest.mark.parametrize("kind,case,route", PERSISTENT, ids=[f"{k}-{_cid(c)}" for k, c, _ in PERSISTENT])
def test_persistent_exact_as_launched_and_on_one_cu(ops, kind, case, route):
    """forward with deferred moments (z16), the matching data gradient without and with the fused norm-backward sums (g16), each
    bit-equal to bf16_round(exact) — on the grid as launched and on the one-CU grid, and the two runs equal bit for bit with their
    moment and NormPartials records"""
    finish(run_persistent(ops, kind, case, route))


def run_persistent(ops, kind, case, route, with32=False, records=None):
    """body of test_persistent_exact_as_launched_and_on_one_cu: the problems of one PERSISTENT case whose three calls must reach `route`.
    with32: the fp32 operand is handed over beside its mirror, and the data gradient with fused sums (a mirror-only form) is not asked
    for — what a caller does where conv_halo_supported says 0.  records: the record kinds the route must fuse, (moments, NormPartials);
    None: both for the persistent kernels, not asserted for the halo kernel (the rule of the primary routes)."""
    B, Hm, Wm, Cs, N = case
    e = exact_persistent(kind, case)
    down = kind == "down"
    P, runs = [], []
    x16, b, zl16, stl = dev(e.op["x"], BF16), dev(e.op["b"]), dev(e.op["zl"], BF16), dev(e.op["rec"])
    x32 = dev(e.op["x"]) if with32 else None
    cb, cs = (Cs, N) if down else (N, Cs)
    pack = ops.conv_pack(dev(e.op["w"]), cb, cs, 1)
    gm, bt = torch.ones(1, device="cuda"), torch.zeros(1, device="cuda")
    fwd = ops.conv2d_s2_fwd_stats if down else ops.convT_s2_fwd_stats
    dgrad = ops.convT_s2_dgrad if down else ops.conv2d_s2_dgrad
    z_want, g_want = O.bf16_round(e.want["z16"]), O.bf16_round(e.want["g16"])
    for budget in (False, True):
        tag = "one CU" if budget else "as launched"
        with one_cu(ops, budget):
            rt = Route(ops, P)
            z16, mom = fwd(x32, pack, b, N, 1, gm, bt, x16=x16, z16=True, alpha=ALPHA, defer_stats=True)
            rt(f"fwd ({tag})", route)
            res = dict(z16=bits(z16))
            if isinstance(mom, ops.Moments):
                res["moment records"] = bits(mom.ws[:B * mom.nparts * 24])
            st = ops.stats_tensor(mom)
            g16 = dgrad(x32, pack, N, 1, dy16=x16, out_bf16=True)
            rt(f"dgrad ({tag})", route)
            g16f, parts = g16, None
            if not with32:
                g16f, parts = dgrad(None, pack, N, 1, dy16=x16, out_bf16=True, fuse=(zl16, stl, ALPHA))
                rt(f"dgrad + sums ({tag})", route)
            res.update(g16=bits(g16), g16f=bits(g16f), stats=bits(st))
            if parts is not None:
                res["NormPartials"] = bits(parts.buf[:B * parts.nparts * 16])
            torch.cuda.synchronize()
        assert z16.dtype == BF16 and g16.dtype == BF16 and g16f.dtype == BF16
        if records is None and "conv_halo" not in route:
            assert isinstance(mom, ops.Moments) and parts is not None, "the persistent kernels fuse both record kinds"
        if records is not None:
            assert (isinstance(mom, ops.Moments), parts is not None) == tuple(records), (route, type(mom).__name__, parts is not None, records)
        P += [explain(f"z16 ({tag})", z16, z_want), explain(f"g16 ({tag})", g16, g_want), explain(f"g16 with sums ({tag})", g16f, g_want),
              moments_problem(f"moments ({tag})", st, e.want["z16"])]
        runs.append(res)
    return P + same_bits("persistent", runs)


@pytest.mark.parametrize("case", ZN, ids=_cid)
def test_normalising_down_conv_exact(ops, case):
    """conv2d_s2_fwd_stats_zn from hand-made records: z16 == bf16_round(conv(h_exact, w) + b), h_exact computed in numpy from the same
    records; as launched and on the one-CU grid"""
    finish(run_zn(ops, case, ZN_ROUTE))


def run_zn(ops, case, route, two_pass=False, with32=False):
    """body of test_normalising_down_conv_exact.  two_pass: the chain that replaces the form where conv2d_s2_fwd_stats_zn_supported says
    0 — instnorm_apply from the same hand-made records to a bf16 map (h is a multiple of 1/8 below 32: the map is exact), then
    conv2d_s2_fwd_stats from that mirror (with32: and from the fp32 map beside it); the same `want` holds, `route` is the conv's"""
    B, Hm, Wm, Cs, N = case
    e = exact_zn(case)
    P, runs = [], []
    zin16, rec, b = dev(e.op["z"], BF16), dev(e.op["rec"]), dev(e.op["b"])
    pack = ops.conv_pack(dev(e.op["w"]), Cs, N, 1)
    gm, bt = torch.ones(1, device="cuda"), torch.zeros(1, device="cuda")
    assert bool(ops.conv2d_s2_fwd_stats_zn_supported(B, 2 * Hm, 2 * Wm, Cs, N, 1)) == (not two_pass)
    want = O.bf16_round(e.want["z16"])
    for budget in (False, True):
        tag = "one CU" if budget else "as launched"
        with one_cu(ops, budget):
            rt = Route(ops, P)
            if two_pass:
                h16 = torch.empty_like(zin16)
                h32 = ops.instnorm_apply(zin16, rec, None, 0, 1, ALPHA, out16=h16, want_f32=with32)
                P.append(explain(f"h16 of the apply pass ({tag})", h16, e.op["h"]))
                ops._lib.load().lg_clear_kernel()
                z16, st = ops.conv2d_s2_fwd_stats(h32 if with32 else None, pack, b, N, 1, gm, bt, x16=h16, z16=True, alpha=ALPHA)
                st = ops.stats_tensor(st)
            else:
                z16, st = ops.conv2d_s2_fwd_stats_zn(zin16, rec, ALPHA, pack, b, N, 1, gm, bt)
            rt(f"zn ({tag})", route)
            torch.cuda.synchronize()
        assert z16.dtype == BF16
        P += [explain(f"z16 ({tag})", z16, want), moments_problem(f"moments ({tag})", st, e.want["z16"])]
        runs.append(dict(z16=bits(z16), stats=bits(st)))
    return P + same_bits("zn", runs)


@pytest.mark.parametrize("form,case,dtype,mirrors,route", WGRAD, ids=[f"{f}-{_cid(c)}-{_dn(d)}-{m}" for f, c, d, m, _ in WGRAD])
def test_weight_gradient_exact(ops, form, case, dtype, mirrors, route):
    finish(run_wgrad(ops, form, case, dtype, mirrors, route))


def run_wgrad(ops, form, case, dtype, mirrors, route):
    """body of test_weight_gradient_exact: the problems of one WGRAD case, overwrite and accumulate, whose calls must reach `route`"""
    B, Hm, Wm, cb, cs = case
    e = exact_wgrad(case)
    P = []
    big, small = e.op["big"], e.op["small"]
    b32 = dev(big) if mirrors != "both" else None
    s32 = dev(small) if mirrors in ("none", "with") else None
    b16 = dev(big, BF16) if mirrors in ("both", "with") else None
    s16 = dev(small, BF16) if mirrors != "none" else None
    for acc in (False, True):
        dw = dev(e.op["prior"]) if acc else torch.full((5, 5, cb, cs), float("nan"), device="cuda")
        rt = Route(ops, P)
        if form == "conv":
            ops.conv2d_s2_wgrad(b32, s32, dw, acc, dtype, x16=b16, dy16=s16)
        else:
            ops.convT_s2_wgrad(s32, b32, dw, acc, dtype, x16=s16, dy16=b16)
        rt("accumulate" if acc else "overwrite", route)
        P.append(explain("dw (accumulate)" if acc else "dw", dw, e.want["dw_acc" if acc else "dw"]))
    return P


@pytest.mark.parametrize("case,dtype,src,routes", FINAL, ids=[f"{_cid(c)}-{_dn(d)}-{s}" for c, d, s, _ in FINAL])
def test_final_layer_exact(ops, case, dtype, src, routes):
    """image: fp64 tanh of the exact pre-activation at 1e-5 absolute; backward with integer dpre: dx (fp32, or bf16 with and without
    the fused sums), dw and db exact, overwrite and accumulate; the persistent patch kernels also on the one-CU grid"""
    finish(run_final(ops, case, dtype, src, routes))


def run_final(ops, case, dtype, src, routes, with32=False, sums=True):
    """body of test_final_layer_exact.  with32 (an "m16" case where n3_m16_supported says 0): the same calls of the bf16 path with the
    fp32 operand handed over beside its mirror.  sums: the route of the "nf" call fuses the norm-backward sums (NormPartials)."""
    B, H, W, cs = case
    e = exact_final(case)
    P, runs = [], []
    m16 = src == "m16"
    x = None if (m16 and not with32) else dev(e.op["x"])
    x16 = dev(e.op["x"], BF16) if m16 else None
    b, dpre, zl16, stl = dev(e.op["b"]), dev(e.op["dpre"]), dev(e.op["zl"], BF16), dev(e.op["rec"])
    pack = ops.conv_pack(dev(e.op["w"]), 3, cs, dtype)
    if m16:
        assert bool(ops.n3_m16_supported(H, W, 3, cs, 1)) == (not with32)
    want_y = np.tanh(e.pre)
    for budget in (False, True):
        tag = "one CU" if budget else "as launched"
        res = {}
        with one_cu(ops, budget):
            rt = Route(ops, P)
            y = ops.convT_s1_tanh_fwd(x, pack, b, 3, dtype, x16=x16)
            rt(f"fwd ({tag})", routes["fwd"])
            dev_y = float(np.abs(f64(y) - want_y).max())
            print(f"final {_cid(case)} {_dn(dtype)} {src} ({tag}): max |y - tanh(pre)| = {dev_y:.3e}, max |pre| = {np.abs(e.pre).max():.3f}")
            if not dev_y <= TANH_TOL:
                P.append(f"y ({tag}): max |y - tanh(exact pre)| = {dev_y:.3e} > {TANH_TOL}")
            res["y"] = bits(y)
            if "dx" in routes and not m16:
                dx = torch.full((B, H, W, cs), float("nan"), device="cuda")
                ops.convT_s1_tanh_bwd(x, dpre, pack, cs, dtype, dx=dx)
                rt(f"dx ({tag})", routes["dx"])
                P.append(explain(f"dx ({tag})", dx, e.want["dx"]))
                res["dx"] = bits(dx)
            if "dx" in routes and (m16 or dtype == 1):
                dx16 = torch.zeros((B, H, W, cs), dtype=BF16, device="cuda")
                ops.convT_s1_tanh_bwd(None, dpre, pack, cs, dtype, dx16=dx16)
                rt(f"dx16 ({tag})", routes["dx"])
                P.append(explain(f"dx16 ({tag})", dx16, O.bf16_round(e.want["dx16"])))
                res["dx16"] = bits(dx16)
            if "nf" in routes:
                dx16 = torch.zeros((B, H, W, cs), dtype=BF16, device="cuda")
                _, parts = ops.convT_s1_tanh_bwd(None, dpre, pack, cs, dtype, dx16=dx16, fuse=(zl16, stl, ALPHA))
                rt(f"dx16 + sums ({tag})", routes["nf"])
                assert (parts is not None) == sums, (routes["nf"], parts is not None, sums)
                P.append(explain(f"dx16 with sums ({tag})", dx16, O.bf16_round(e.want["dx16"])))
                res["dx16f"] = bits(dx16)
                if parts is not None:
                    res["NormPartials"] = bits(parts.buf[:B * parts.nparts * 16])
            for acc in (False, True):
                dw = dev(e.op["pw"]) if acc else torch.full((5, 5, 3, cs), float("nan"), device="cuda")
                db = dev(e.op["pb"]) if acc else torch.full((3,), float("nan"), device="cuda")
                ops.convT_s1_tanh_bwd(x, dpre, pack, cs, dtype, dw=dw, db=db, accumulate=acc, x16=x16)
                rt(f"dw {'accumulate' if acc else 'overwrite'} ({tag})", routes["dw"])
                sfx = "_acc" if acc else ""
                P += [explain(f"dw{sfx} ({tag})", dw, e.want["dw" + sfx]), explain(f"db{sfx} ({tag})", db, e.want["db" + sfx])]
                res["dw" + sfx] = bits(dw)
            torch.cuda.synchronize()
        runs.append(res)
    return P + same_bits("final", runs)


@pytest.mark.parametrize("case", FINAL_Z16, ids=_cid)
def test_normalising_final_layer_exact(ops, case):
    finish(run_final_z16(ops, case, FINAL_Z16_ROUTE))


def run_final_z16(ops, case, route, two_pass=False):
    """body of test_normalising_final_layer_exact.  two_pass: the chain that replaces the form where convT_s1_tanh_fwd_z16_supported says
    0 — instnorm_apply from the same records (h is exact), then convT_s1_tanh_fwd from the mirror alone where n3_m16_supported, else
    from the fp32 map beside it (the Decoder's own rule); `route` is the final layer's"""
    B, H, W, C = case
    e = exact_final_z16(case)
    P = []
    assert bool(ops.convT_s1_tanh_fwd_z16_supported(H, W, 3, C, 1)) == (not two_pass)
    pack = ops.conv_pack(dev(e.op["w"]), 3, C, 1)
    z16, rec = dev(e.op["z"], BF16), dev(e.op["rec"])
    rt = Route(ops, P)
    if two_pass:
        m16 = bool(ops.n3_m16_supported(H, W, 3, C, 1))
        h16 = torch.empty_like(z16)
        h32 = ops.instnorm_apply(z16, rec, None, 0, 1, ALPHA, out16=h16, want_f32=not m16)
        P.append(explain("h16 of the apply pass", h16, e.op["h"]))
        ops._lib.load().lg_clear_kernel()
        y = ops.convT_s1_tanh_fwd(h32, pack, dev(e.op["b"]), 3, 1, x16=h16)
    else:
        y = ops.convT_s1_tanh_fwd_z16(z16, rec, ALPHA, pack, dev(e.op["b"]), 3, 1)
    rt("z16", route)
    d = float(np.abs(f64(y) - np.tanh(e.pre)).max())
    print(f"final-z16 {_cid(case)}: max |y - tanh(pre)| = {d:.3e}, max |pre| = {np.abs(e.pre).max():.3f}")
    if not d <= TANH_TOL:
        P.append(f"y: max |y - tanh(exact pre)| = {d:.3e} > {TANH_TOL}")
    return P


@pytest.mark.parametrize("case", P16, ids=_cid)
def test_three_channel_bf16_source_kernels_exact(ops, case):
    """conv1 forward from the fp32 image on the bf16 MFMA with fused moments (fp32 and bf16 result) and conv1's data gradient from the
    mirror: persistent grids, as launched and on one CU"""
    finish(run_p16(ops, case, P16_FWD, P16_UP))


def run_p16(ops, case, fwd_route, up_route, fused=True):
    """body of test_three_channel_bf16_source_kernels_exact.  fused=False (the routes that take over where n3_m16_supported says 0): the
    forward returns no statistics with its fp32 result (ops: "stats or None") and the bf16 result's come from the instnorm_stats pass of
    ops._fwd_stats_z16 — still the moments of the exact map; the data gradient gets the fp32 gradient beside its mirror"""
    B, Hs, Ws, N = case
    e = exact_p16(case)
    P, runs = [], []
    x, b, dy = dev(e.op["x"]), dev(e.op["b"]), dev(e.op["dy"])
    pack = ops.conv_pack(dev(e.op["w"]), 3, N, 1)
    gm, bt = torch.ones(1, device="cuda"), torch.zeros(1, device="cuda")
    assert bool(ops.n3_m16_supported(Hs, Ws, 3, N, 1)) == fused
    for budget in (False, True):
        tag = "one CU" if budget else "as launched"
        with one_cu(ops, budget):
            rt = Route(ops, P)
            z, st = ops.conv2d_s2_fwd_stats(x, pack, b, N, 1, gm, bt)
            rt(f"fwd ({tag})", fwd_route)
            z16, st16 = ops.conv2d_s2_fwd_stats(x, pack, b, N, 1, gm, bt, z16=True, alpha=ALPHA)
            rt(f"fwd z16 ({tag})", fwd_route)   # (unfused: the statistics pass that follows the conv names no kernel)
            dx = ops.conv2d_s2_dgrad(None if fused else dy, pack, 3, 1, dy16=dy.to(BF16))
            rt(f"dgrad ({tag})", up_route)
            torch.cuda.synchronize()
        assert (st is not None) == fused and z16.dtype == BF16 and st16 is not None
        st16 = ops.stats_tensor(st16)
        P += [explain(f"z ({tag})", z, e.want["z"]), explain(f"z16 ({tag})", z16, O.bf16_round(e.want["z16"])),
              explain(f"dx ({tag})", dx, e.want["dx"]), moments_problem(f"moments z16 ({tag})", st16, e.want["z"])]
        if st is not None:
            P.append(moments_problem(f"moments ({tag})", st, e.want["z"]))
        runs.append(dict(z=bits(z), z16=bits(z16), dx=bits(dx), stats16=bits(st16), **({"stats": bits(st)} if st is not None else {})))
    return P + same_bits("p16", runs)


@pytest.mark.parametrize("case", BWDNORM, ids=_cid)
def test_bwdnorm_equals_two_pass_chain(ops, case):
    """convT_s2_dgrad_bn == instnorm_bwd + convT_s2_dgrad bit for bit (gradient and NormPartials), beyond one tile per sample and on
    the one-CU grid (the row of tests/test_memory_contract_gpu.py, whose inputs these are)"""
    B, s_h, s_w, cb, cs = case
    s = crc("bn", case)
    shape = (B, 2 * s_h, 2 * s_w, cb)
    alpha = 0.3

    def arr(seed, *sh, scale=1.0, shift=0.0):
        return (np.random.default_rng(seed).standard_normal(sh) * scale + shift).astype(np.float32)

    z = arr(s, *shape) * (0.5 + 2.0 * np.random.default_rng(s + 9).random((B, 1, 1, 1), dtype=np.float32)) + arr(s + 8, B, 1, 1, 1)
    g, w, zl = arr(s + 1, *shape), arr(s + 2, 5, 5, cb, cs, scale=0.05), arr(s + 3, B, s_h, s_w, cs, scale=1.3, shift=0.2)
    z16, g16, zl16 = dev(z, BF16), dev(g, BF16), dev(zl, BF16)
    gm, bt = torch.tensor([0.9], device="cuda"), torch.tensor([0.15], device="cuda")
    gml, btl = torch.tensor([1.1], device="cuda"), torch.tensor([-0.05], device="cuda")
    st = ops.instnorm_stats(z16.float(), gm, bt, 0, alpha)
    stl = ops.instnorm_stats(zl16.float(), gml, btl, 0, alpha)
    pack = ops.conv_pack(dev(w), cb, cs, 1)
    assert ops.convT_s2_dgrad_bn_supported(B, s_h, s_w, cb, cs, 1)
    # {sum g', sum g' c} per (sample, part) as a producer would leave them
    zz, gg = z16.double().reshape(B, 4, -1), g16.double().reshape(B, 4, -1)
    mu, a_, b_ = (st[:, 0].double() + st[:, 4].double()).view(B, 1, 1), st[:, 2].view(B, 1, 1), st[:, 3].view(B, 1, 1)
    c32 = (z16.float().reshape(B, 4, -1) - st[:, 0].view(B, 1, 1)) - st[:, 4].view(B, 1, 1)
    gp = torch.where(a_ * c32 + b_ > 0, gg, alpha * gg)
    sums = torch.stack([gp.sum(-1), (gp * (zz - mu)).sum(-1)], -1).contiguous().view(U8).reshape(-1)
    Pn = ops.NormPartials(sums, 4, alpha, shape)
    coef = ops.instnorm_bwd_coef(z16, st, Pn)
    dz16 = torch.empty(shape, dtype=BF16, device="cuda")
    ops.instnorm_bwd(z16, st, g16, None, None, 0, 1, alpha, out16=dz16, want_f32=False, partials=Pn)
    P, runs = [], []
    for budget in (False, True):
        tag = "one CU" if budget else "as launched"
        with one_cu(ops, budget):
            rt = Route(ops, P)
            g_bn, p_bn = ops.convT_s2_dgrad_bn(z16, g16, coef, alpha, pack, cs, fuse=(zl16, stl, alpha))
            rt(f"bn ({tag})", BWDNORM_ROUTE[0])
            sums_bn = bits(p_bn.buf[:B * p_bn.nparts * 16])
            g_ref, p_ref = ops.convT_s2_dgrad(None, pack, cs, 1, dy16=dz16, out_bf16=True, fuse=(zl16, stl, alpha))
            rt(f"two-pass ({tag})", BWDNORM_ROUTE[1])
            sums_ref = bits(p_ref.buf[:B * p_ref.nparts * 16])
            torch.cuda.synchronize()
        P.append(explain(f"g_bn against the two-pass chain ({tag})", g_bn, f64(g_ref)))
        if not torch.equal(sums_bn, sums_ref):
            P.append(f"NormPartials of the BWDNORM form differ from the two-pass chain ({tag})")
        runs.append(dict(g_bn=bits(g_bn), sums_bn=sums_bn, g_ref=bits(g_ref), sums_ref=sums_ref))
    finish(P + same_bits("bwdnorm", runs))
