"""CPU: the shade-math mode's public interface (include/rspt.h rspt_set_shade_math / rspt_get_shade_math): host-only state that needs no device,
the constants in the header, rs_pbrt_amd/abi.py and rust_shim/ffi.rs, and an ABI version that stays 27 (the interface is additive)."""
import os
import re
import subprocess
import sys

import pytest

from rs_pbrt_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rspt.h")).read()
FFI = open(os.path.join(ROOT, "rust_shim", "ffi.rs")).read()


@pytest.fixture(autouse=True)
def exact_afterwards():
    yield
    lib.lib().rspt_set_shade_math(abi.SHADE_MATH_EXACT)


def test_default_is_exact_and_needs_no_device():
    """a fresh process (this one may have set the mode before): no rspt_init, no scene, and the mode reads exact"""
    code = ("from rs_pbrt_amd import abi, lib\n"
            "assert lib.lib().rspt_get_shade_math() == abi.SHADE_MATH_EXACT == 0\n"
            "assert lib.get_shade_math() == 'exact'\n"
            "lib.set_shade_math('fast'); assert lib.get_shade_math() == 'fast' and lib.lib().rspt_get_shade_math() == abi.SHADE_MATH_FAST == 1\n")
    env = {k: v for k, v in os.environ.items() if k != "RSPT_SHADE_MATH"}
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, check=True)


def test_set_get_round_trip():
    L = lib.lib()
    for name, value in (("fast", 1), ("exact", 0), ("fast", 1)):
        lib.set_shade_math(name)
        assert lib.get_shade_math() == name and L.rspt_get_shade_math() == value
    assert L.rspt_set_shade_math(abi.SHADE_MATH_EXACT) == 0 and L.rspt_get_shade_math() == 0


def test_a_value_above_one_is_invalid_and_changes_nothing():
    lib.set_shade_math("fast")
    with pytest.raises(lib.RsptError) as e:
        lib.set_shade_math(2)
    assert e.value.code == abi.E_INVALID and "shade_math" in str(e.value)
    assert lib.get_shade_math() == "fast"
    with pytest.raises(KeyError):
        lib.set_shade_math("quick")


def test_the_environment_does_not_reach_the_getter(monkeypatch):
    """RSPT_SHADE_MATH is read per render (tests/test_gpu_shade_math.py); the getter answers what the call set"""
    monkeypatch.setenv("RSPT_SHADE_MATH", "fast")
    assert lib.get_shade_math() == "exact"


def test_header_abi_py_and_ffi_rs_agree_on_the_constants():
    m = re.search(r"enum\s*\{\s*RSPT_SHADE_MATH_EXACT\s*=\s*(\d+)\s*,\s*RSPT_SHADE_MATH_FAST\s*=\s*(\d+)\s*\}", HEADER)
    assert m, "the enum is not in include/rspt.h"
    header = (int(m.group(1)), int(m.group(2)))
    rust = tuple(int(re.search(r"pub const RSPT_SHADE_MATH_%s: u32 = (\d+);" % n, FFI).group(1)) for n in ("EXACT", "FAST"))
    assert header == rust == (abi.SHADE_MATH_EXACT, abi.SHADE_MATH_FAST) == (0, 1)
    assert lib.SHADE_MATH == {"exact": 0, "fast": 1}


def test_both_symbols_are_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"\bint\s+rspt_set_shade_math\s*\(\s*uint32_t\s+mode\s*\)\s*;", src)
    assert re.search(r"\buint32_t\s+rspt_get_shade_math\s*\(\s*void\s*\)\s*;", src)
    assert re.search(r"pub fn rspt_set_shade_math\(mode: u32\) -> c_int;", FFI) and re.search(r"pub fn rspt_get_shade_math\(\) -> u32;", FFI)
    dyn = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("rspt_set_shade_math", "rspt_get_shade_math"):
        assert re.search(r"\bT %s$" % sym, dyn, re.M), sym
        assert sym in lib.EXPORTS


def test_the_abi_version_stays_27():
    assert lib.lib().rspt_abi_version() == 27 == abi.ABI_VERSION
    assert FFI.splitlines()[0].count("ABI version 27") == 1
    assert re.search(r"#define RSPT_ABI_VERSION 27\b", HEADER)


def test_python_mirror_keyword_is_validated():
    from rs_pbrt_amd import integrator
    with pytest.raises(ValueError):
        integrator.PathIntegrator(camera=object(), shade_math="quick")
    assert integrator.PathIntegrator(camera=object(), shade_math="fast").shade_math == "fast"
    assert integrator.PathIntegrator(camera=object()).shade_math is None
