"""The route behind every run-time kill switch, as plain data, checked on the CPU.

A kill switch makes one kernel family decline; "the next product kernel takes the shape".  TABLE says, per switch, which family that
is (kernel-name prefixes in the spelling of ops.last_kernel()), which kernel takes over for every call of every exact case of
tests/test_conv_exact_gpu.py whose asserted route lies in the family, and which API forms disappear altogether (their *_supported query
turns 0 and a two-pass chain replaces them).  The fallback routes are read off the dispatch chains of capi.hip, conv_igemm.hip,
wgrad_igemm.hip and conv_halo.hip; tests/test_kill_switch_gpu.py reruns every selected case under its switch in a fresh process and
asserts exactly these routes, with the same exact comparisons.

The cases are selected from the case tables by the route string, so a case added there is picked up here (and fails here until its
fallback route is written down).  This file checks what can be checked without a GPU: the table covers exactly the switches of
tests/test_switches.py, every switch selects cases, no fallback lies in the family it replaces, every fallback is a kernel name some
source notes, and every (switch, case) pair meets the conditions of the exact form (the bound walk of tests/test_conv_exact_cpu.py on
the same Exact objects)."""
import functools
import glob
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_conv_exact_gpu as X  # noqa: E402
import test_skinny_gpu as S  # noqa: E402
from test_conv_exact_cpu import test_conditions_of_the_exact_form as conditions_of_the_exact_form  # noqa: E402
from test_kernel_names import CASES as NAME_CASES  # noqa: E402
from test_switches import KILL_SWITCHES  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IG, HALO, D3, U3, U4 = X.IG, X.HALO, X.D3, X.U3, X.U4
H16D, H16K, HRES, HS1T = HALO + "<bf16,DOWN>", HALO + "<bf16,UP,K-sliced>", HALO + "<UP,resident>", HALO + "<S1T>"
WG32, WG16, WGP = "wgrad_kernel<f32,per-tap>", "wgrad_kernel<bf16,per-tap>", "wgrad_kernel<PATCH>"

# API forms that exist only while a kernel family does: name -> (the ops query that turns False, the chain that replaces the form)
FORMS = {
    "zn": ("conv2d_s2_fwd_stats_zn_supported", "instnorm_apply to a bf16 map, then conv2d_s2_fwd_stats from that mirror"),
    "bn": ("convT_s2_dgrad_bn_supported", "instnorm_bwd to a bf16 gradient, then convT_s2_dgrad from that mirror"),
    "z16": ("convT_s1_tanh_fwd_z16_supported", "instnorm_apply, then convT_s1_tanh_fwd (from the mirror alone where n3_m16_supported)"),
    "ns": ("convT_s2_fwd_ns_supported", "instnorm_apply with the skip, then convT_s2_fwd_stats"),
    "mirror": ("conv_halo_supported", "the same call with the fp32 operand beside its bf16 mirror; no fused norm-backward sums"),
    "m16": ("n3_m16_supported", "the same call with the fp32 operand beside its bf16 mirror"),
    "fused": ("lg_conv_fwd_stats_fused", "the conv writes fp32, instnorm_stats gives the moments and the bf16 copy (ops._fwd_stats_z16)"),
}

# One whole training step per switch (tests/test_kill_switch_gpu.py): the smallest O.Cfg whose default step reaches the family.
# 64 x 64 images (init_dim 4: the smallest side at which a level has an 8 x 16 tile), batch 2, and the narrowest widths the shape
# predicates allow: conv_up3 takes exactly 128 -> 64 and 64 -> 32 channels (conv_filter[2:5]), the PAIR tilings of conv_down3 / conv_up4
# and the NW=128 tiling need 128 columns on the 8 x 8 and 16 x 16 levels (conv_filter[1:3]), wgrad_at / wgrad_at32 need 64 columns; the
# top width is free.  One configuration reaches every conv family, so the parent records the default step once per dtype.
STEP_CONV = dict(init_dim=4, conv_filter=(64, 128, 128, 64, 32), cond_dim=40, batch_size=2)
# the skinny GEMMs take batches that are multiples of 32 (the heads see [real; fake] = 2 x batch_size) and K % 512 == 0 (16 x width)
STEP_SKINNY = dict(init_dim=4, conv_filter=(32, 32, 32, 32, 32), cond_dim=40, batch_size=16)

# switch -> family: kernel-name prefixes the switch turns off
#           fallback: asserted route of an exact case -> the route that takes over (a route outside the family stays)
#           where: (table, case key, call or None) -> route, where the shape decides (reason beside it)
#           forms: the API forms that disappear (FORMS)
#           records: (moments, NormPartials) the fallback of a PERSISTENT case still fuses; None in second place: the form is gone
#           steps: dtypes of the whole-step run; cfg: its configuration
TABLE = {
    "LG_NO_HALO": dict(
        family=(HALO, D3, U3, U4),   # through lg_halo_enabled(): the halo-tile kernel and the three persistent kernels, NORM / BWDNORM / ns forms included
        fallback={HALO + "<f32,DOWN>": IG + "<DOWN>", H16D: IG + "<DOWN>", HALO + "<f32,UP,K-sliced>": IG + "<UP>", H16K: IG + "<UP>",
                  HRES: IG + "<UP>", HALO + "<f32,UP,resident>": IG + "<UP>", HS1T: IG + "<S1T>",
                  D3 + "<PAIR>": IG + "<DOWN>", D3 + "<NW=64>": IG + "<DOWN>", D3 + "<NW=128>": IG + "<DOWN>",
                  D3 + "<NW=128,NORM>": IG + "<DOWN>", D3 + "<NW=64,BWDNORM>": IG + "<DOWN>",
                  U3 + "<128,64>": IG + "<UP>", U3 + "<64,32,4w>": IG + "<UP>", U4: IG + "<UP>", U4 + "<PAIR>": IG + "<UP>"},
        where={}, forms=("mirror", "fused", "zn", "bn", "ns"), records=(False, None), steps=("bf16", "f32"), cfg=STEP_CONV),
    "LG_NO_DOWN3": dict(
        family=(D3,),
        fallback={D3 + "<PAIR>": H16D, D3 + "<NW=64>": H16D, D3 + "<NW=128>": H16D, D3 + "<NW=128,NORM>": H16D, D3 + "<NW=64,BWDNORM>": H16D},
        where={}, forms=("zn", "bn"), records=(True, False), steps=("bf16",), cfg=STEP_CONV),
    "LG_NO_D3_NORM": dict(
        family=(D3 + "<NW=128,NORM>",), fallback={D3 + "<NW=128,NORM>": D3 + "<NW=128>"},
        where={}, forms=("zn",), records=None, steps=("bf16",), cfg=STEP_CONV),
    "LG_NO_D3_BWDNORM": dict(
        family=(D3 + "<NW=64,BWDNORM>",), fallback={D3 + "<NW=64,BWDNORM>": D3 + "<NW=64>"},
        where={}, forms=("bn",), records=None, steps=("bf16",), cfg=STEP_CONV),
    "LG_NO_UP3": dict(
        family=(U3,),   # conv_up4 wants N % 128 == 0, so both shapes go on to the halo kernel: 64 / 128 channels of bf16 fit its resident form
        fallback={U3 + "<128,64>": HRES, U3 + "<64,32,4w>": HRES},
        where={}, forms=("ns",), records=(True, False), steps=("bf16",), cfg=STEP_CONV),
    "LG_NO_UP4": dict(
        family=(U4,),
        fallback={U4: HRES, U4 + "<PAIR>": HRES},
        # two 8 x 8 samples per tile: 200 halo rows x (128 channels x 2 B + 16) = 54400 B is over the resident form's 52 KiB
        where={("PERSISTENT", ("up", (2, 8, 8, 128, 256)), None): H16K},
        forms=(), records=(True, False), steps=("bf16",), cfg=STEP_CONV),
    "LG_NO_WGAT": dict(
        family=("wgrad_at_kernel",),
        fallback={"wgrad_at_kernel<32,4>": WG16, "wgrad_at_kernel<16,8>": WG16, "wgrad_at_kernel<8,8>": WG16},
        where={}, forms=(), records=None, steps=("bf16",), cfg=STEP_CONV),
    "LG_NO_WGAT32": dict(
        family=("wgrad_at32_kernel",),
        fallback={"wgrad_at32_kernel<16,4>": WG32, "wgrad_at32_kernel<8,8>": WG32},
        where={}, forms=(), records=None, steps=("bf16", "f32"), cfg=STEP_CONV),
    "LG_NO_ROWS": dict(
        family=("s1t_fwd_rows_kernel",),
        fallback={"s1t_fwd_rows_kernel<32>": "s1t_fwd_p16_kernel", "s1t_fwd_rows_kernel<32,NORM>": "s1t_fwd_p16_kernel"},
        # 8 rows are no multiple of the 16 x 16 tiles of n3_pgemm.hip and n3_kernels.hip: n3_m16_supported says 0, the fp32 map goes to the gather chain
        where={("FINAL_Z16", ((3, 8, 32, 32),), None): HS1T},
        forms=("z16",), records=None, steps=("bf16",), cfg=STEP_CONV),
    "LG_NO_N3": dict(
        family=("n3_", "patch_p16_kernel", "up_p16_kernel", "s1t_fwd_"),
        fallback={"patch_p16_kernel<2,64>": IG + "<PATCH>", "patch_p16_kernel<1,32>": IG + "<PATCH>", "patch_p16_kernel<1,32,nf>": IG + "<PATCH>",
                  "up_p16_kernel": H16K, "n3_wgrad_kernel<f32>": WGP, "n3_wgrad16_kernel<1>": WGP, "n3_wgrad16_kernel<2>": WGP,
                  "n3_wgrad16_kernel<1,16>": WGP, "s1t_fwd_rows_kernel<32>": HS1T, "s1t_fwd_p16_kernel": HS1T,
                  "s1t_fwd_rows_kernel<32,NORM>": HS1T},
        # the VALU kernels of n3_kernels.hip note no name (route ""): what replaces them depends on the call
        where={("CONV32", ("down", (2, 16, 16, 3, 64), 1), "dgrad"): H16K,
               ("FINAL", ((2, 16, 16, 32), 0, "f32"), "fwd"): HS1T, ("FINAL", ((2, 16, 16, 32), 1, "f32"), "fwd"): HS1T},
        forms=("m16", "z16", "fused"), records=None, steps=("bf16", "f32"), cfg=STEP_CONV),
    "LG_NO_SKINNY_MFMA": dict(
        family=("dense_fwd_mfma_kernel", "dense_wgrad_mfma_kernel", "heads_fwd_mfma_kernel", "heads_wgrad_mfma_kernel", "heads_dgrad_mfma_kernel"),
        fallback={"dense_fwd_mfma_kernel": "dense_fwd_kernel", "dense_wgrad_mfma_kernel<5>": "dense_wgrad_kernel",
                  "heads_fwd_mfma_kernel": "heads_fwd_kernel", "heads_wgrad_mfma_kernel": "heads_wgrad_kernel",
                  "heads_dgrad_mfma_kernel": "heads_dgrad_kernel"},
        where={}, forms=(), records=None, steps=("bf16", "f32"), cfg=STEP_SKINNY),
}


def in_family(route, family):
    return bool(route) and any(route.startswith(p) for p in family)


def exact_cases():
    """(table, key, {call: asserted route}, case id of test_conv_exact_cpu or None) of every exact case, calls that are not run left out"""
    out = []
    for kind, case, dt, r in X.CONV32:
        out.append(("CONV32", (kind, case, dt), {k: v for k, v in r.items() if v is not None}, f"conv32-{kind}-{X._cid(case)}-{X._dn(dt)}"))
    for kind, case, route in X.PERSISTENT:
        out.append(("PERSISTENT", (kind, case), {"fwd": route, "dgrad": route, "dgrad + sums": route}, f"persistent-{kind}-{X._cid(case)}"))
    for case in X.ZN:
        out.append(("ZN", (case,), {"zn": X.ZN_ROUTE}, f"zn-{X._cid(case)}"))
    for form, case, dt, mirrors, route in X.WGRAD:
        out.append(("WGRAD", (form, case, dt, mirrors), {"dw": route}, f"wgrad-{form}-{X._cid(case)}-{X._dn(dt)}-{mirrors}"))
    for case, dt, src, r in X.FINAL:
        out.append(("FINAL", (case, dt, src), dict(r), f"final-{X._cid(case)}-{X._dn(dt)}-{src}"))
    for case in X.FINAL_Z16:
        out.append(("FINAL_Z16", (case,), {"z16": X.FINAL_Z16_ROUTE}, f"final-z16-{X._cid(case)}"))
    for case in X.P16:
        out.append(("P16", (case,), {"fwd": X.P16_FWD, "dgrad": X.P16_UP}, f"p16-{X._cid(case)}"))
    for case in X.BWDNORM:   # its Exact: the plain data gradient at the BWDNORM shape, a PERSISTENT case of the same layout
        out.append(("BWDNORM", (case,), {"bn": X.BWDNORM_ROUTE[0], "two-pass": X.BWDNORM_ROUTE[1]}, None))
    # the op-level part of LG_NO_SKINNY_MFMA: the two shapes of tests/test_skinny_gpu.py's own child test, with the routes they take by
    # the rules stated there (dense: B % 32 == 0, N % 128 == 0, K <= 144, MT = ceil(133 / 32) = 5; heads: B % 64 == 0, K % 512 == 0)
    out.append(("SKINNY_DENSE", (S.KILL_DENSE[:3],), {"fwd": S.DENSE_FWD[S.M], "wgrad": S.dense_wgrad_name(5)}, None))
    out.append(("SKINNY_HEADS", (S.KILL_HEADS[:3],), {"fwd": S.HEADS_FWD[S.M], "wgrad": S.HEADS_WGRAD[S.M], "dgrad": S.HEADS_DGRAD[S.M]}, None))
    return out


def selected(switch):
    """the exact cases with a route in the switch's family: (table, key, {call: asserted route}, case id)"""
    fam = TABLE[switch]["family"]
    return [c for c in exact_cases() if any(in_family(r, fam) for r in c[2].values())]


def fallback_routes(switch, table, key, calls):
    """{call: the route that must take over under the switch} of one selected case"""
    ent = TABLE[switch]
    out = {}
    for call, route in calls.items():
        for k in ((table, key, call), (table, key, None)):
            if k in ent["where"]:
                out[call] = ent["where"][k]
                break
        else:
            out[call] = ent["fallback"][route] if in_family(route, ent["family"]) else route
    return out


@functools.lru_cache(maxsize=None)
def ledger():
    """every kernel name some source passes to lg_note_kernel, and the short names of tests/test_kernel_names.py"""
    names = {want for _, want in NAME_CASES}
    for path in glob.glob(os.path.join(ROOT, "littlegan_amd", "csrc", "*.hip")):
        for call in re.finditer(r"lg_note_kernel\((.*?)\);", open(path).read(), re.S):
            names |= set(re.findall(r'"([^"]*)"', call.group(1)))
    return names


def exact_factory(table, key, cid):
    """the Exact object the (switch, case) pair compares with under the switch: the case's own"""
    if table == "BWDNORM":
        return functools.partial(X.exact_persistent, "down", key[0])
    return {c[0]: c[2] for c in X.all_cases()}[cid]


def test_the_table_has_exactly_the_kill_switches():
    assert set(TABLE) == KILL_SWITCHES, set(TABLE) ^ KILL_SWITCHES
    for sw, ent in TABLE.items():
        assert set(ent) == {"family", "fallback", "where", "forms", "records", "steps", "cfg"}, sw
        assert ent["family"] and all(ent["family"]) and set(ent["forms"]) <= set(FORMS) and "bf16" in ent["steps"], sw
    assert {sw for sw, e in TABLE.items() if "f32" in e["steps"]} == {"LG_NO_HALO", "LG_NO_N3", "LG_NO_WGAT32", "LG_NO_SKINNY_MFMA"}


@pytest.mark.parametrize("switch", sorted(TABLE))
def test_every_switch_selects_cases_and_names_their_fallbacks(switch):
    ent = TABLE[switch]
    cases = selected(switch)
    assert cases, f"{switch}: no exact case asserts a route of {ent['family']}"
    used_fb, used_where = set(), set()
    for table, key, calls, _ in cases:
        fb = fallback_routes(switch, table, key, calls)   # (KeyError: a selected route without a fallback in the table)
        assert set(fb) == set(calls)
        for call, route in fb.items():
            assert not in_family(route, ent["family"]), f"{switch} {table} {key} {call}: the fallback {route!r} lies in the family it replaces"
            assert route in ledger(), f"{switch} {table} {key} {call}: no source notes a kernel {route!r}"
            if in_family(calls[call], ent["family"]):
                assert route != calls[call]
        used_fb |= {r for r in calls.values() if in_family(r, ent["family"])}
        used_where |= {k for k in ent["where"] if k[:2] == (table, key)}
    assert set(ent["fallback"]) <= ledger() and all(in_family(r, ent["family"]) for r in ent["fallback"]), switch
    assert used_fb == set(ent["fallback"]), f"{switch}: fallback entries no selected case uses: {set(ent['fallback']) - used_fb}"
    assert used_where == set(ent["where"]), f"{switch}: 'where' entries that match no selected case: {set(ent['where']) - used_where}"


def test_the_family_prefixes_are_kernel_names():
    for sw, ent in TABLE.items():
        for p in ent["family"]:
            assert any(n.startswith(p) for n in ledger()), (sw, p)


PAIRS = [(sw, c) for sw in sorted(TABLE) for c in selected(sw)]


@pytest.mark.parametrize("switch,case", PAIRS, ids=[f"{sw}-{c[0]}-{c[3] or X._cid(c[1][0])}" for sw, c in PAIRS])
def test_every_switch_case_pair_keeps_the_conditions_of_the_exact_form(switch, case):
    table, key, calls, cid = case
    if table.startswith("SKINNY"):
        B, K, N = key[0]   # integers in [-4, 4]: every partial sum of the forward, the weight gradient (and its prior) stays below 2^24
        assert 16 * max(B, K) + 4 < 2 ** 24
        return
    conditions_of_the_exact_form(cid or f"bwdnorm-plain-{X._cid(key[0])}", list(fallback_routes(switch, table, key, calls).values()),
                                 exact_factory(table, key, cid))
