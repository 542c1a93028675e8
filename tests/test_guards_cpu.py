"""CPU side of the memory-contract tests: the guard-band helper (tests/guards.py) is shown to bite on CPU tensors; the ledger — every
pointer-taking function of the C ABI (every include/littlegan_*.h) is named by a row of tests/test_memory_contract_gpu.py or exempted with a reason;
and the host-only sizing functions at every row's shape (no kernel runs here)."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guards  # noqa: E402
import test_memory_contract_gpu as MC  # noqa: E402
from guards import ALIGN, ZONE_MIN, Guarded, called, exact_workspaces, guard  # noqa: E402
from test_abi import _protos  # noqa: E402
from test_launch_shapes_gpu import LAYERS  # noqa: E402

DTYPES = [torch.float32, torch.bfloat16, torch.float64, torch.uint8, torch.int64]


# ------------------------------------------------------------------------------------------------------------------ the helper
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("shape", [(3, 5, 7), (70000,)])   # a payload below the 64 KiB floor of a zone, and one above it
def test_layout_and_fill(dtype, shape):
    g = Guarded(shape, dtype, "cpu", fill=0xFF)
    item = torch.empty((), dtype=dtype).element_size()
    assert tuple(g.t.shape) == shape and g.t.dtype == dtype and g.t.is_contiguous() and g.t.data_ptr() % ALIGN == 0
    assert g.nbytes == g.t.numel() * item
    assert g.zone_bytes == (max(g.nbytes, ZONE_MIN) + ALIGN - 1) // ALIGN * ALIGN and g.zone_bytes % ALIGN == 0
    assert g.front.numel() == g.back.numel() == g.zone_bytes
    assert g.front.data_ptr() + g.zone_bytes == g.t.data_ptr() and g.t.data_ptr() + g.nbytes == g.back.data_ptr()   # adjacent
    assert g.intact() == []
    # 0xFF reads as NaN in every floating type, as -1 in a signed integer, as 255 in a byte
    if dtype.is_floating_point:
        assert bool(torch.isnan(g.t).all())
        assert bool(torch.isnan(g.front[:g.zone_bytes // item * item].view(dtype)).all())
    elif dtype == torch.int64:
        assert bool((g.t == -1).all())
    else:
        assert bool((g.t == 255).all())
    z = Guarded(shape, dtype, "cpu", fill=0x00)
    assert bool((z.t == 0).all()) and z.intact() == []


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_a_single_changed_byte_is_reported_with_its_offset(dtype):
    g = Guarded((5, 9), dtype, "cpu", fill=0x00)
    assert g.intact() == []
    g.t.fill_(3)                                   # writing the payload is what an op does: not reported
    assert g.intact() == []
    for zone, index, want in ((g.front, g.zone_bytes - 1, -1),            # the byte just before the payload
                              (g.back, 0, g.nbytes),                     # the byte just after it
                              (g.front, 0, -g.zone_bytes),               # the far end of the front zone
                              (g.back, g.zone_bytes - 1, g.nbytes + g.zone_bytes - 1)):
        zone[index] = 0x7E
        assert g.intact() == [want], (index, want, g.intact()[:4])
        zone[index] = 0xFF
        assert g.intact() == []
    g.front[10], g.back[20] = 0, 1
    assert g.intact() == [10 - g.zone_bytes, g.nbytes + 20]
    assert "2 byte(s) changed" in guards.describe(g.intact()) and f"{g.nbytes + 20:+d}" in guards.describe(g.intact())
    g.refill_zones(0x00)                           # run B of the contract test: zero zones
    assert g.intact() == []
    g.back[0] = 0xFF
    assert g.intact() == [g.nbytes]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_guard_copies_a_tensor_and_a_tensor_fill_is_checked(dtype):
    src = (torch.arange(24).reshape(2, 3, 4) % 7).to(dtype)
    g = guard(src)
    assert torch.equal(g.t, src) and g.t.data_ptr() != src.data_ptr() and g.intact() == []
    g2 = guard(src.transpose(0, 2))                # not contiguous: copied by value
    assert torch.equal(g2.t, src.transpose(0, 2)) and g2.t.is_contiguous()
    with pytest.raises(ValueError):
        Guarded((2, 3), dtype, "cpu", fill=src)


def test_exact_workspaces_hand_out_what_was_asked_for(monkeypatch):
    ops = types.SimpleNamespace(workspace=lambda nbytes, device, tag="default": torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8))
    pool = ops.workspace
    with monkeypatch.context() as mp:
        ws = exact_workspaces(mp, ops, fill=0xFF)
        a, b = ops.workspace(24, "cpu", "small"), ops.workspace(100000, "cpu", tag="wgrad")
        assert a.numel() == 24 and b.numel() == 100000 and a.dtype == torch.uint8 and a.data_ptr() % ALIGN == 0
        assert bool((a == 0xFF).all()) and a.data_ptr() != ops.workspace(24, "cpu", "small").data_ptr()   # a fresh buffer per call
        assert len(ws.handed) == 3 and [h[0] for h in ws.handed] == ["small", "wgrad", "small"]
        ws.assert_intact()
        a.fill_(1)                                  # inside the advertised size
        ws.assert_intact()
        ws.handed[1][2].back[3] = 0                 # a kernel that writes one record too many
        with pytest.raises(AssertionError, match=r"workspace #1 'wgrad' of 100000 bytes.*\+100003"):
            ws.assert_intact()
        zero = exact_workspaces(mp, ops, fill=0x00)
        z = ops.workspace(64, "cpu")
        assert bool((z == 0).all()) and zero.handed[0][2].zone_byte == 0 and zero.damaged() == []
    assert ops.workspace is pool


def test_called_records_the_entry_points_fetched(monkeypatch):
    real = types.SimpleNamespace(lg_a=lambda: 1, lg_b=lambda: 2, other=3)
    ops = types.SimpleNamespace(_lib=types.SimpleNamespace(load=lambda: real))
    with monkeypatch.context() as mp:
        names = called(mp, ops)
        h = ops._lib.load()
        assert h.lg_a() == 1 and h.other == 3 and h.lg_b() == 2 and h.lg_a() == 1
        assert names == ["lg_a", "lg_b", "lg_a"]
        with pytest.raises(AttributeError):
            h.lg_missing
    assert ops._lib.load() is real


# ------------------------------------------------------------------------------------------------------------------ the ledger
def _pointer_functions():
    return {name for name, (ret, plist) in _protos().items() if any("*" in p for p in plist)}


def test_every_pointer_taking_entry_point_has_a_row_or_a_reason():
    protos = _protos()
    want = _pointer_functions()
    assert len(want) >= 100, len(want)
    covered = {n for r in MC.CASES for n in r.covers}
    unknown = covered - set(protos)
    assert not unknown, f"rows name functions no header declares: {sorted(unknown)}"
    assert set(MC.EXEMPT) == {"lg_contention_probe", "lg_set_clock_census", "lg_clock_sample"}      # the run-time probes, nothing else
    for name, reason in MC.EXEMPT.items():
        assert name in want, f"EXEMPT lists {name}, which takes no pointer or is not declared"
        assert isinstance(reason, str) and len(reason.split()) >= 4, f"EXEMPT[{name}] needs its reason"
        assert name not in covered, f"{name} is exempt AND covered: drop the exemption"
    missing = want - covered - set(MC.EXEMPT)
    assert not missing, ("entry points without a row in tests/test_memory_contract_gpu.py (add one, or an EXEMPT entry with its reason): "
                         f"{sorted(missing)}")


def test_rows_are_well_formed():
    ids = [r.id for r in MC.CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    for r in MC.CASES:
        assert r.covers and callable(r.run) and callable(r.check), r.id
        for fn, args in r.sizing:
            assert fn.endswith("_workspace_bytes") and fn in _protos(), (r.id, fn)


# ------------------------------------------------------------------------------------------------------------------ the sizing functions
@pytest.fixture(scope="module")
def lib():
    from littlegan_amd.csrc.build import build
    build(verbose=False)
    from littlegan_amd import _lib
    return _lib.load()


def test_sizing_functions_are_positive_and_repeatable(lib):
    seen, fns = 0, set()
    for r in MC.CASES:
        for fn, args in r.sizing:
            first, second = int(getattr(lib, fn)(*args)), int(getattr(lib, fn)(*args))
            assert first > 0 and first == second, (r.id, fn, args, first, second)
            seen += 1
            fns.add(fn)
    assert seen >= 60 and "lgrel_r12_workspace_bytes" in fns, (seen, sorted(fns))


def _internal(lib, name, argtypes):
    import ctypes as C
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = C.c_size_t, argtypes
    return fn


def _wgrad_shapes():
    shapes = {r.wgrad for r in MC.CASES if r.wgrad is not None}
    for _, _, cb, cs, s in LAYERS:          # the launch shapes: Hs = Ws = s, both operand types, B = 256 and 512
        for B in (256, 512):
            for dtype in (0, 1):
                shapes.add((B, s, s, cb, cs, dtype))
    return sorted(shapes)


def test_wgrad_workspace_covers_every_route(lib):
    """lg_wgrad_workspace_bytes is a max over routes: it must not be below what any of the launchers it may dispatch to checks for
    itself (a short value is invisible behind the 1 MiB pool until the launch batch, where the buffer is exact for the first time).
    Compared per route: the 3-channel kernel for cb == 3, wgrad_at in bf16, wgrad_at32 in f32, as lg_conv_wgrad_m16 dispatches; taken
    over all three a bf16 call would be measured against the slabs of an f32 kernel it never runs (2 x 16 x 16 x 32 x 64: 819200 bytes
    for bf16, 1638400 for wgrad_at32).
    What this can and cannot show: it restates the max that lg_wgrad_workspace_bytes takes, so it catches a route dropped from that
    max, and a sizing function that stops being repeatable.  It cannot see a launcher whose own ws_bytes check disagrees with its
    sizing function: that is what the weight-gradient rows of tests/test_memory_contract_gpu.py test, by running each route with a
    workspace of exactly this size and asserting the kernel name."""
    import ctypes as C
    i5 = [C.c_int] * 5
    at = _internal(lib, "lg_wgrad_at_workspace_bytes", i5)
    at32 = _internal(lib, "lg_wgrad_at32_workspace_bytes", i5)
    n3 = _internal(lib, "lg_n3_wgrad_workspace_bytes", [C.c_int] * 4)
    shapes = _wgrad_shapes()
    assert len(shapes) >= 30 and any(s[0] == 512 for s in shapes)
    for B, Hs, Ws, cb, cs, dtype in shapes:
        total = int(lib.lg_wgrad_workspace_bytes(B, Hs, Ws, cb, cs, dtype))
        assert total > 0 and total == int(lib.lg_wgrad_workspace_bytes(B, Hs, Ws, cb, cs, dtype))
        if cb == 3:
            need = {"lg_n3_wgrad_workspace_bytes": int(n3(B, Hs, Ws, cs))}
        elif dtype == 1:
            need = {"lg_wgrad_at_workspace_bytes": int(at(B, Hs, Ws, cb, cs))}
        else:
            need = {"lg_wgrad_at32_workspace_bytes": int(at32(B, Hs, Ws, cb, cs))}
        for name, n in need.items():
            assert total >= n, f"B={B} {Hs}x{Ws} cb={cb} cs={cs} dtype={dtype}: lg_wgrad_workspace_bytes {total} < {name} {n}"
        # the final layer's backward (stride 1) shares the function through lg_convT_s1_bwd_workspace_bytes
        if cb == 3:
            assert int(lib.lg_convT_s1_bwd_workspace_bytes(B, Hs, Ws, 3, cs, dtype)) >= total
