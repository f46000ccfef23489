"""No GPU: pcore_evaluate_states is declared, listed and exported, its LDS limit is the same in the header and in the
binding, the ABI version stays 9, and the argument checks that need no context hold."""
import ctypes
import os
import re

from perception_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "pcore.h")).read()


def test_evaluate_states_is_declared_listed_and_exported():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+pcore_evaluate_states\s*\(", src)
    assert "pcore_evaluate_states" in _native.EXPORTED_SYMBOLS
    lib = _native.load()
    assert isinstance(lib.pcore_evaluate_states, ctypes._CFuncPtr)
    assert len(lib.pcore_evaluate_states.argtypes) == 16
    assert lib.pcore_abi_version() == 9 and "#define PCORE_ABI_VERSION 9" in _header()


def test_lds_limit_matches_the_header_and_fits_the_workgroup():
    m = re.search(r"#define\s+PCORE_STATE_LDS_OBS\s+(\d+)", _header())
    assert m and int(m.group(1)) == _native.PCORE_STATE_LDS_OBS
    # one bit per observed point beside about 8 KB of queues and counters: within the 64 KB a workgroup gets as it is
    assert _native.PCORE_STATE_LDS_OBS // 8 + 8704 <= 65536


def test_null_context_and_parameters_are_refused():
    lib = _native.load()
    p = _native.EvalParams(2, 1, 8, 100.0, 0.01, 1.0, 15.0)
    args = [None] * 6 + [0, None, ctypes.byref(p)] + [None] * 5 + [0, None]
    args[2] = 0
    assert lib.pcore_evaluate_states(*args) == _native.PCORE_E_INVALID_ARG
