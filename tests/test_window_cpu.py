"""Horizon windows (ltp_sample_window_batch, include/ltp_hip.h) without a device: the symbols, the size rule, the validation that runs
before anything is launched, and the drop-in header's new method under plain g++."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NAMES = ("ltp_window_elements", "ltp_sample_window_batch", "ltp_plan_window_host")


@pytest.fixture(scope="module")
def abi():
    from longtermplanner_amd import _abi
    _abi.build()
    return _abi


def test_window_symbols_are_declared_and_exported(abi):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltp_hip.h")).read(), flags=re.S)
    lib = C.CDLL(abi.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} is not declared in include/ltp_hip.h"
        assert n in abi.exported_symbols(), f"{n} is not declared in _abi._SIGNATURES"
        assert hasattr(lib, n), f"{n} is not exported"
    # the Python structure is the C struct, field for field
    fields = re.search(r"typedef struct \{([^}]*)\} ltp_window_opts;", open(os.path.join(ROOT, "include", "ltp_hip.h")).read(), flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"(\w+);", fields) == [f[0] for f in abi.WindowOpts._fields_]
    assert C.sizeof(abi.WindowOpts) == 40 and C.sizeof(abi.WindowOpts) % 8 == 0


@pytest.mark.parametrize("N", [1, 31, 32, 33, 64, 100])
def test_window_elements_without_a_handle_and_row_stride_factor(abi, N):
    """NOT the product rule itself: ltp_window_elements reads dof from a handle, and a handle needs a device. Checked here is what
    exists without one — the factor R = ltp_row_stride(N) and the null-handle result 0 (ltp_run_tables_bytes' convention). The rule
    count * 4 * dof * R is asserted by tests/test_gpu_window.py::test_window_elements for the same N."""
    lib = abi.lib()
    R = lib.ltp_row_stride(N)
    assert R % 32 == 0 and R >= N and R - N < 32
    assert lib.ltp_window_elements(None, 10, N) == 0


def test_window_calls_are_refused_without_a_handle(abi):
    """Without a device there is no handle, and a call without a handle is LTP_ERR_INVALID_ARGUMENT whatever its opts hold: nothing
    is dereferenced, nothing launched, no crash on any of the malformed structs below. WHICH check refuses a malformed struct on a
    live handle, and with what text, is asserted by tests/test_gpu_window.py::test_refusals; this test cannot tell the checks apart
    (a null handle has nowhere to keep an error text) and does not claim to."""
    lib = abi.lib()
    O = abi.WindowOpts
    q, r = abi.Queries(), abi.Records()

    def call(o):
        return lib.ltp_sample_window_batch(None, 0, 0, C.byref(q), C.byref(r), C.addressof(o) if o is not None else None, None, 0, None)
    good = dict(size=C.sizeof(O), format=0, n_samples=32)
    assert call(O(**good)) == INVALID                               # null handle
    assert call(None) == INVALID
    for bad in (dict(size=0), dict(size=C.sizeof(O) - 8), dict(size=C.sizeof(O) + 4), dict(format=2), dict(format=-1), dict(n_samples=0),
                dict(n_samples=-5)):
        assert call(O(**dict(good, **bad))) == INVALID, bad
    assert lib.ltp_plan_window_host(None, 0, None, None, None, None, None, 0, 32, None, None, None) == INVALID


DROPIN = r'''
#include "long_term_planner/long_term_planner.h"
#include <cstdio>
int main() {
  using namespace long_term_planner;
  std::vector<double> lo = {-1.0}, hi = {1.0}, one = {1.0};
  try {
    LongTermPlanner ltp(1, 0.001, lo, hi, one, one, one);
    std::vector<double> rows;
    std::vector<int> valid;
    const double qg = 0.5, z = 0.0;
    const int k = 3;
    const long long ok = ltp.planWindowBatch(1, &qg, &z, &z, &z, &k, 0, 32, rows, &valid);
    std::printf("%lld %zu %zu\n", ok, rows.size(), valid.size());
    return rows.size() == 4u * 32u && valid.size() == 1u ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 2;
  }
}
'''


def test_dropin_header_with_plan_window_batch_compiles_with_plain_gxx(abi, tmp_path):
    src = tmp_path / "window.cc"
    src.write_text(DROPIN)
    exe = tmp_path / "window"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "longtermplanner_amd"), "-lltp_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "longtermplanner_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)
