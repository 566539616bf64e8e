"""Limit sets without a GPU: the new entry points are exported and bound, refuse a null handle, the header compiles as C and C++,
the status bit is free, the drop-in overloads compile, and the Python wrapper rejects wrong shapes before touching a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ltp_set_limit_sets", "ltp_get_limit_sets", "ltp_bind_limit_sets", "ltp_plan_batch_sets_host")


@pytest.fixture(scope="module")
def abi():
    from longtermplanner_amd import _abi
    _abi.build()
    return _abi


def test_new_symbols_are_exported_and_bound(abi):
    lib = C.CDLL(abi.LIB_PATH)
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in abi.exported_symbols(), n


def test_null_handle_is_refused(abi):
    lib = abi.lib()
    d = (C.c_double * 7)()
    INVALID = 1
    assert lib.ltp_set_limit_sets(None, 1, d, d, d, d, d) == INVALID
    assert lib.ltp_set_limit_sets(None, 0, None, None, None, None, None) == INVALID
    assert lib.ltp_get_limit_sets(None) == -1
    assert lib.ltp_bind_limit_sets(None, None) == INVALID
    assert lib.ltp_plan_batch_sets_host(None, 0, None, None, None, None, None, None, None, None) == INVALID


def _header_defines():
    text = open(os.path.join(ROOT, "include", "ltp_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (LTP_STATUS_\w+)\s+(\d+)", text)}


def test_bad_limit_set_status_is_a_bit_of_its_own(abi):
    st = _header_defines()
    assert st["LTP_STATUS_BAD_LIMIT_SET"] == 512 == abi.STATUS_BAD_LIMIT_SET
    others = [v for k, v in st.items() if k != "LTP_STATUS_BAD_LIMIT_SET"]
    assert all(v & 512 == 0 for v in others)
    assert (512 & (512 - 1)) == 0


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles(tmp_path, lang):
    src = tmp_path / ("t.c" if lang == "c" else "t.cc")
    src.write_text('#include "ltp_hip.h"\n'
                   "int f(ltp_planner* p, const int* ix, const double* l, long long n, const double* q, unsigned long long* o,\n"
                   "      double** packed) {\n"
                   "    int s = LTP_STATUS_BAD_LIMIT_SET;\n"
                   "    if (ltp_set_limit_sets(p, 2, l, l, l, l, l) || ltp_bind_limit_sets(p, ix)) return -1;\n"
                   "    return s + ltp_get_limit_sets(p) + ltp_plan_batch_sets_host(p, n, q, q, q, q, ix, 0, o, packed);\n"
                   "}\n")
    cc = "gcc" if lang == "c" else "g++"
    subprocess.run([cc, "-std=c11" if lang == "c" else "-std=c++17", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(tmp_path / "t.o")], check=True)


def test_dropin_overloads_compile(tmp_path):
    src = tmp_path / "d.cc"
    src.write_text("#include <long_term_planner/long_term_planner.h>\n"
                   "bool g(long_term_planner::LongTermPlanner& p, const double* l, const double* q, const int* ix) {\n"
                   "    long_term_planner::BatchTrajectory out;\n"
                   "    if (!p.setLimitSets(2, l, l, l, l, l)) return false;\n"
                   "    return p.planTrajectoryBatch(3, q, q, q, q, ix, out) && p.planTrajectoryBatch(3, q, q, q, q, ix, out, false)\n"
                   "           && p.limitSets() == 2;\n"
                   "}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "d.o")],
                   check=True)


class _NoDevice:
    """Stands in for the library: any call but the dof query fails the test (nothing may reach a device)."""
    def ltp_get_dof(self, h):
        return 7

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


@pytest.mark.parametrize("shapes", [
    [(2, 7)] * 4 + [(2, 6)],            # one array with the wrong dof
    [(2, 7)] * 4 + [(3, 7)],            # different numbers of sets
    [(7,)] * 5,                         # not [K, dof]
    [(0, 7)] * 5,                       # no set at all: use None to clear
])
def test_set_limit_sets_rejects_wrong_shapes_before_any_device_call(abi, shapes):
    from longtermplanner_amd import LongTermPlanner
    p = LongTermPlanner.__new__(LongTermPlanner)
    p._lib, p._h = _NoDevice(), None
    with pytest.raises(ValueError):
        p.setLimitSets(*[np.ones(s) for s in shapes])
    with pytest.raises(ValueError):
        p.setLimitSets(None, np.ones((2, 7)), None, None, None)
