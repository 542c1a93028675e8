"""Every run-time kill switch, set in a fresh process: the route that takes over is the one tests/test_kill_switch_cpu.py names, and
it is exact.

A switch is read once per process, so one test = one child (subprocess.run of a fresh interpreter, the parent's environment plus the
one switch; the pattern of tests/test_skinny_gpu.py), one child at a time.  The child

  1. walks the exact cases of tests/test_conv_exact_gpu.py whose asserted route lies in the switched-off family, through the bodies of
     those tests (run_conv32, run_persistent, ...) with the fallback routes of the table: every call must reach exactly that route, fp32
     results np.array_equal to the fp64 oracle, bf16 results bit-equal to bf16_round(exact), images within TANH_TOL, moments within
     MOM_TOL.  The default run is exact on the same operands, so this says the fallback and the primary kernel agree bit for bit.  Where
     the API form itself disappears, the *_supported query must say so and the two-pass chain that replaces the form must be exact;
  2. runs one training step (batch_no 11, the Adjuster branch on) at the table's configuration under tests/replay.py: the step ends
     without an error, every recorded call passes check_call at replay.py's tolerances, and no recorded kernel name lies in the family.

The parent records the same step once with no switch set and asserts that the family IS reached there (else the step says nothing).
LG_NO_SKINNY_MFMA keeps tests/test_skinny_gpu.py's own child as its op-level part.  A child that dies (signal, abort, time limit) ends
the module: the remaining switches skip and start nothing more on the GPU."""
import functools
import os
import subprocess
import sys
import time
import traceback

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import np_oracle as O  # noqa: E402
import test_conv_exact_gpu as X  # noqa: E402
from replay import OpRecorder, check_call  # noqa: E402
from test_kill_switch_cpu import TABLE, fallback_routes, in_family, selected  # noqa: E402
from test_switches import KILL_SWITCHES  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_NO = 11
# wgrad_at32 is a kernel of the exact-f32 path alone: the bf16 step under LG_NO_WGAT32 only shows that the switch disturbs nothing there
BF16_NOT_REACHED = {"LG_NO_WGAT32"}
_DIED = []   # reason, once a child has died: the remaining tests of the module skip


# ------------------------------------------------------------------------------------------------------------------ the step
def record_step(cfg_kw, mfma):
    from test_step_gpu import build, dev_inputs, f32_round, perturbed
    cfg = O.Cfg(**cfg_kw)
    tr = build(cfg, perturbed(cfg, 7), mfma)
    inp = dev_inputs(f32_round(O.make_inputs(cfg, cfg.batch_size, seed=9)))
    with OpRecorder() as r:
        tr.train_step_from_inputs(BATCH_NO, inp)
        torch.cuda.synchronize()
    return r


@functools.lru_cache(maxsize=None)
def default_step_kernels(cfg_items, mfma):
    """kernel names of the step with no switch set (recorded once per configuration and dtype, in the parent)"""
    assert not [s for s in KILL_SWITCHES if os.environ.get(s)], "the parent process runs with no kill switch set"
    return tuple(sorted({rec["kernel"] for rec in record_step(dict(cfg_items), mfma).calls}))


def step_part(switch, mfma):
    ent = TABLE[switch]
    r = record_step(ent["cfg"], mfma)
    for i, rec in enumerate(r.calls):
        try:
            check_call(rec, r.packs)
        except AssertionError as e:
            raise AssertionError(f"call {i} {rec['name']} (kernel {rec['kernel']!r}) of the {mfma} step: {e}") from e
    bad = sorted({rec["kernel"] for rec in r.calls if in_family(rec["kernel"], ent["family"])})
    assert not bad, f"{mfma} step under {switch}: kernels of the switched-off family ran: {bad}"
    return len(r.calls), sorted({rec["kernel"] for rec in r.calls})


# ------------------------------------------------------------------------------------------------------------------ the exact cases
def exact_part(ops, switch):
    ent = TABLE[switch]
    forms = ent["forms"]
    with32 = "mirror" in forms
    rec = None if ent["records"] is None else (bool(ent["records"][0]), bool(ent["records"][1]))
    problems, done = [], 0
    for table, key, calls, cid in selected(switch):
        if table.startswith("SKINNY"):
            continue   # tests/test_skinny_gpu.py::test_kill_switch_routes_everything_to_the_valu_kernels
        fb = fallback_routes(switch, table, key, calls)
        if table == "CONV32":
            kind, case, dt = key
            p = X.run_conv32(ops, kind, case, dt, {k: fb.get(k) for k in ("fwd", "dgrad", "stats", "stats16", "dgrad16")})
        elif table == "PERSISTENT":
            kind, case = key
            B, Hm, Wm, Cs, N = case
            assert len(set(fb.values())) == 1
            if with32:
                assert not ops.conv_halo_supported(0 if kind == "down" else 1, 1, *case), (switch, key)
            if "fused" in forms:
                up = kind == "up"
                assert not ops._lib.load().lg_conv_fwd_stats_fused(int(up), 1, B, Hm, Wm, N if up else Cs, Cs if up else N), (switch, key)
            if "ns" in forms and calls["fwd"].startswith(X.U3):   # the normalising forward exists on conv_up3's tilings alone
                assert not ops.convT_s2_fwd_ns_supported(B, Hm, Wm, N, Cs, 1), (switch, key)
            p = X.run_persistent(ops, kind, case, fb["fwd"], with32=with32, records=rec)
        elif table == "ZN":
            p = X.run_zn(ops, key[0], fb["zn"], two_pass=True, with32=with32)
        elif table == "WGRAD":
            form, case, dt, mirrors = key
            if mirrors == "n3" and "m16" in forms:   # the mirror of the wide operand alone is no form any more
                assert not ops.n3_m16_supported(case[1], case[2], 3, case[4], 1), (switch, key)
                mirrors = "with"
            p = X.run_wgrad(ops, form, case, dt, mirrors, fb["dw"])
        elif table == "FINAL":
            case, dt, src = key
            p = X.run_final(ops, case, dt, src, fb, with32=src == "m16" and "m16" in forms,
                            sums=fb.get("nf") == calls.get("nf"))   # only the patch_p16 kernel fuses the norm-backward sums
        elif table == "FINAL_Z16":
            p = X.run_final_z16(ops, key[0], fb["z16"], two_pass=True)
        elif table == "P16":
            B, Hs, Ws, N = key[0]
            assert "fused" in forms and not ops._lib.load().lg_conv_fwd_stats_fused(0, 1, B, Hs, Ws, 3, N), (switch, key)
            p = X.run_p16(ops, key[0], fb["fwd"], fb["dgrad"], fused=False)
        elif table == "BWDNORM":
            B, s_h, s_w, cb, cs = key[0]
            assert not ops.convT_s2_dgrad_bn_supported(B, s_h, s_w, cb, cs, 1), (switch, key)
            assert fb["bn"] == fb["two-pass"]   # what is left of the form is the plain data gradient: exact, and on this route
            p = X.run_persistent(ops, "down", key[0], fb["two-pass"], with32=with32, records=rec)
        else:
            raise KeyError(table)
        problems += [f"{table} {key}: {q}" for q in p if q]
        done += 1
    print(f"{switch}: {done} exact cases rerun")
    return problems


# ------------------------------------------------------------------------------------------------------------------ the child
def _goes_on(exc):
    """a failed check or a refused argument leaves the GPU as it was; anything else (a launch error, an error torch reports) ends the child"""
    from littlegan_amd._lib import LittleGanHipError
    if isinstance(exc, (AssertionError, ValueError, KeyError)):
        return True
    return isinstance(exc, LittleGanHipError) and ("(rc=-1)" in str(exc) or "(rc=-3)" in str(exc))


def child(switch):
    """body of the child process: both parts, every failure reported; exit status 0 and 'child ok' only if there was none"""
    assert os.environ.get(switch) == "1" and switch in TABLE
    from littlegan_amd import ops
    failures = []
    parts = [("exact cases", lambda: exact_part(ops, switch))] + [(f"{m} step", functools.partial(step_part, switch, m)) for m in TABLE[switch]["steps"]]
    for name, fn in parts:
        t0 = time.perf_counter()
        try:
            out = fn()
            if name == "exact cases" and out:
                failures.append(f"{name}:\n" + "\n".join(out))
            elif name != "exact cases":
                print(f"{switch} {name}: {out[0]} calls checked; kernels {out[1]}")
        except Exception as e:  # noqa: BLE001
            failures.append(f"{name}: {traceback.format_exc()}")
            if not _goes_on(e):
                print("\n".join(failures))
                print(f"{switch}: stopped after the {name} (not a failed check: nothing more is started on the GPU)")
                sys.exit(3)
        print(f"{switch} {name}: {time.perf_counter() - t0:.1f} s", flush=True)
    torch.cuda.synchronize()
    if failures:
        print("\n".join(failures))
        sys.exit(1)
    print("child ok")


@pytest.mark.parametrize("switch", sorted(KILL_SWITCHES))
def test_the_route_behind_the_switch_is_the_table_s_and_exact(switch):
    if _DIED:
        pytest.skip(f"a child died earlier in this module ({_DIED[0]}): nothing more is started on the GPU")
    ent = TABLE[switch]
    for mfma in ent["steps"]:   # without this the step under the switch would be vacuous
        names = default_step_kernels(tuple(sorted(ent["cfg"].items())), mfma)
        reached = [n for n in names if in_family(n, ent["family"])]
        print(f"{switch}: the default {mfma} step reaches {reached}")
        assert reached or (mfma == "bf16" and switch in BF16_NOT_REACHED), (switch, mfma, names)
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_kill_switch_gpu as T; T.child(%r)" % (ROOT, os.path.join(ROOT, "tests"), switch))
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, "-c", code], env={**os.environ, switch: "1"}, timeout=120, capture_output=True, text=True, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        _DIED.append(f"{switch}: time limit")
        pytest.fail(f"{switch}: the child ran into its time limit\n{str(e.stdout)[-4000:]}\n{str(e.stderr)[-4000:]}", pytrace=False)
    print(f"{switch}: child wall time {time.perf_counter() - t0:.1f} s\n{r.stdout[-3000:]}")
    if r.returncode < 0 or r.returncode in (134, 139, 3):
        _DIED.append(f"{switch}: exit status {r.returncode}")
    assert r.returncode == 0 and "child ok" in r.stdout, (r.returncode, r.stdout[-6000:], r.stderr[-4000:])
