"""Strided horizon windows (ltp_sample_horizon_batch, include/ltp_hip.h) without a device: the symbols, the options struct, the
validation that runs before anything is launched, the drop-in header's new method under plain g++, and the yardstick of the GPU
tests (tests/horizon_checker.py) against a plain loop over the CPU oracle's trajectories."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import horizon_checker as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NAMES = ("ltp_sample_horizon_batch", "ltp_plan_horizon_host")


@pytest.fixture(scope="module")
def abi():
    from longtermplanner_amd import _abi
    _abi.build()
    return _abi


def test_horizon_symbols_are_declared_and_exported(abi):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltp_hip.h")).read(), flags=re.S)
    lib = C.CDLL(abi.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} is not declared in include/ltp_hip.h"
        assert n in abi.exported_symbols(), f"{n} is not declared in _abi._SIGNATURES"
        assert hasattr(lib, n), f"{n} is not exported"


def test_horizon_opts_is_the_c_struct(abi):
    fields = re.search(r"typedef struct \{([^}]*)\} ltp_horizon_opts;", open(os.path.join(ROOT, "include", "ltp_hip.h")).read(), flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"(\w+);", fields) == [f[0] for f in abi.HorizonOpts._fields_]
    assert C.sizeof(abi.HorizonOpts) == 40
    # the window struct is what it was
    assert C.sizeof(abi.WindowOpts) == 40 and "stride" not in [f[0] for f in abi.WindowOpts._fields_]


def test_horizon_calls_are_refused_without_a_handle(abi):
    """A call without a handle is LTP_ERR_INVALID_ARGUMENT whatever its opts hold: nothing is dereferenced, nothing launched, no
    crash on the malformed structs. Which check refuses what on a live handle is tests/test_gpu_horizon.py::test_refusals."""
    lib = abi.lib()
    O = abi.HorizonOpts
    q, r = abi.Queries(), abi.Records()

    def call(o):
        return lib.ltp_sample_horizon_batch(None, 0, 0, C.byref(q), C.byref(r), C.addressof(o) if o is not None else None, None, 0, None)
    good = dict(size=C.sizeof(O), format=0, n_samples=32, stride=10)
    assert call(O(**good)) == INVALID
    assert call(None) == INVALID
    for bad in (dict(size=0), dict(size=C.sizeof(O) - 8), dict(size=C.sizeof(O) + 4), dict(format=2), dict(n_samples=0), dict(stride=0),
                dict(stride=-1)):
        assert call(O(**dict(good, **bad))) == INVALID, bad
    assert lib.ltp_plan_horizon_host(None, 0, None, None, None, None, None, 0, 32, 10, None, None, None) == INVALID


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
    const long long ok = ltp.planHorizonBatch(1, &qg, &z, &z, &z, &k, 0, 32, 10, rows, &valid);
    std::printf("%lld %zu %zu\n", ok, rows.size(), valid.size());
    return rows.size() == 4u * 32u && valid.size() == 1u ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 2;
  }
}
'''


def test_dropin_header_with_plan_horizon_batch_compiles_with_plain_gxx(abi, tmp_path):
    src = tmp_path / "horizon.cc"
    src.write_text(DROPIN)
    exe = tmp_path / "horizon"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "longtermplanner_amd"), "-lltp_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "longtermplanner_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.fixture(scope="module")
def oracle_plans(oracle_mod):
    """50 panda plans of the CPU oracle with their trajectories, packed into the full-row layout (computed once, not modified)."""
    from longtermplanner_amd import generate_queries, limit_set
    dof, lim = limit_set("panda")
    n = 50
    qs = [np.ascontiguousarray(x) for x in generate_queries(n, lim, seed=4242)]
    orc = oracle_mod.Oracle(dof, hc.TS, **lim)
    o = orc.plan_batch(*qs, sample=True)
    trajs = []
    for p in range(n):
        if o["status"][p] == 0:
            trajs.append((0, *[np.zeros((dof, 0))] * 4))
        else:
            trajs.append(orc.get_trajectory(o["t_scaled"][p], o["dir"][p], o["mod"][p], qs[1][p], qs[2][p], qs[3][p], o["v_drive"][p]))
    full, offsets, lens = hc.pack_full_rows(trajs, dof)
    assert np.mean(lens > 0) > 0.9
    return dof, trajs, full, offsets, lens, np.asarray(o["t_scaled"]).reshape(n, dof, 7)


@pytest.mark.parametrize("N,s", [(32, 10), (33, 3), (1, 7)])
def test_checker_against_a_plain_loop(oracle_plans, N, s):
    """The checker's gather, hold rule and `valid` on the grid s * arange(N) are what a loop over (plan, w) reads from the oracle's
    own trajectories; `valid` is also the closed form min(N, ceil(max(0, traj_len - k) / s))."""
    import torch
    dof, trajs, full, offsets, lens, t_scaled = oracle_plans
    n = len(trajs)
    k = hc.draw_starts(np.random.default_rng(99), lens, t_scaled, N, s)
    assert np.any(k < 0) and np.any(k >= lens) and np.any((k > 0) & (k < lens))
    first, count = 3, n - 5
    exp, valid, planned = hc.expected(torch.from_numpy(full), torch.from_numpy(offsets), torch.from_numpy(lens), torch.from_numpy(k[first:first + count]),
                                      hc.stride_grid(N, s), dof, first, count)
    # the closed form the header documents for the strided `valid` is the count form on these cases
    closed = hc.strided_valid(torch.from_numpy(lens[first:first + count]).long(), torch.from_numpy(k[first:first + count]).long().clamp(min=0), N, s)
    assert torch.equal(valid, closed)
    exp = exp.numpy().view(np.float64)
    held = 0
    for i in range(count):
        L, *arrs = trajs[first + i]
        assert bool(planned[i]) == (L > 0)
        if L == 0:
            assert int(valid[i]) == 0
            continue
        k0 = max(int(k[first + i]), 0)
        n_real = 0
        for w in range(N):
            t = k0 + w * s
            n_real += t < L
            held += t >= L
            for x, arr in enumerate(arrs):
                for j in range(dof):
                    want = arr[j][t] if t < L else (arr[j][L - 1] if x == 0 else 0.0)
                    assert exp[i, x, j, w].tobytes() == np.float64(want).tobytes(), (i, x, j, w)
        assert int(valid[i]) == n_real == min(N, -(-max(0, L - k0) // s))
    assert held > 0
