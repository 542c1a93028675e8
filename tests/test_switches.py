"""The switch lists of DESIGN.md 4, as a text scan of the sources (no GPU, no library): an experiment's switch lives in the commit
that measured it — the product tree carries the adopted form and its kill switch only, so these lists do not grow silently."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "littlegan_amd")

# run-time: per-kernel kill switches (each makes one specialised kernel decline; the next product kernel takes the shape) ...
KILL_SWITCHES = {"LG_NO_HALO", "LG_NO_N3", "LG_NO_ROWS", "LG_NO_SKINNY_MFMA", "LG_NO_DOWN3", "LG_NO_D3_NORM", "LG_NO_D3_BWDNORM",
                 "LG_NO_UP3", "LG_NO_UP4", "LG_NO_WGAT", "LG_NO_WGAT32"}
# ... and what the Python side reads: the variant-build mechanism (build.py, _lib.py) and the CUs left to communication kernels
PY_ENV = {"LG_EXTRA_FLAGS", "LG_VARIANT_SOURCES", "LG_LIB_VARIANT", "LG_RESERVED_CUS"}
# compile-time: the timing-ablation masks of the variant builds (they cannot enter the product library)
MACROS = {"LG_D3_DBG", "LG_WGAT_DBG", "LG_N3W_DBG", "LG_P16_DBG"}


def _sources():
    out = []
    for ext in ("hip", "h", "py"):
        out += glob.glob(os.path.join(PKG, "**", "*." + ext), recursive=True)
    assert len(out) > 30, out
    return {p: open(p).read() for p in sorted(out)}


def test_environment_switches_are_the_keep_list():
    flags, raw, pyenv = [], set(), set()
    for path, text in _sources().items():
        flags += re.findall(r'lg_env_flag\(\s*"(\w+)"', text)
        raw |= set(re.findall(r'getenv\(\s*"(\w+)"', text))
        if path.endswith(".py"):
            pyenv |= set(re.findall(r'environ(?:\.get\(|\[)\s*["\'](LG_\w+)', text))
    assert set(flags) == KILL_SWITCHES, set(flags) ^ KILL_SWITCHES
    assert sorted(flags) == sorted(KILL_SWITCHES), "each kill switch is read in exactly one place: " + str(sorted(flags))
    assert not raw, raw
    assert pyenv == PY_ENV, pyenv ^ PY_ENV


def test_compile_time_macros_are_the_keep_list():
    seen = set()
    for text in _sources().values():
        for line in re.findall(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", text, flags=re.M):
            seen |= set(re.findall(r"\bLG_\w+", line))
    assert seen == MACROS, seen ^ MACROS


def test_getenv_only_inside_lg_env_flag():
    hits = []
    for path in sorted(glob.glob(os.path.join(PKG, "csrc", "*"))):
        if not path.endswith((".hip", ".h")):
            continue
        text = open(path).read()
        for m in re.finditer(r"\bgetenv\s*\(", text):
            hits.append((os.path.basename(path), text[:m.start()].count("\n") + 1))
    assert len(hits) == 1 and hits[0][0] == "runtime.hip", hits
    text = open(os.path.join(PKG, "csrc", "runtime.hip")).read()
    body = text[text.index('extern "C" int lg_env_flag(const char* name) {'):]
    body = body[:body.index("\n}\n")]
    assert "getenv(name)" in body
