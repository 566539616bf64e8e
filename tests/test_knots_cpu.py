"""Knot-grid horizons (ltp_sample_knots_batch, include/ltp_hip.h) without a device: the symbols, the options struct, the validation
that runs before anything is launched, the drop-in header's new method under plain g++, the host arithmetic of the kernel's search
and clamp (tests/cpp/knots_ranges_test.cc, also under the address and undefined-behaviour sanitizers), and the yardstick of the GPU
tests (tests/horizon_checker.py on the grids of tests/knots_checker.py, and the latter's stretch logic) against a plain loop over the
CPU oracle's trajectories."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import horizon_checker as hc
import knots_checker as kc
from horizon_checker import TS, draw_starts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NAMES = ("ltp_sample_knots_batch", "ltp_plan_knots_host")


@pytest.fixture(scope="module")
def abi():
    from longtermplanner_amd import _abi
    _abi.build()
    return _abi


def test_knots_symbols_are_declared_and_exported(abi):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltp_hip.h")).read(), flags=re.S)
    lib = C.CDLL(abi.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} is not declared in include/ltp_hip.h"
        assert n in abi.exported_symbols(), f"{n} is not declared in _abi._SIGNATURES"
        assert hasattr(lib, n), f"{n} is not exported"
    assert re.search(r"#define\s+LTP_MAX_KNOTS\s+512\b", text) and abi.MAX_KNOTS == kc.MAX_KNOTS == 512


def test_knots_opts_is_the_c_struct(abi):
    fields = re.search(r"typedef struct \{([^}]*)\} ltp_knots_opts;", open(os.path.join(ROOT, "include", "ltp_hip.h")).read(), flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"(\w+);", fields) == [f[0] for f in abi.KnotsOpts._fields_]
    assert C.sizeof(abi.KnotsOpts) == 40
    assert abi.KnotsOpts.knot_offsets.offset == 16 and abi.KnotsOpts.first_sample.offset == 24 and abi.KnotsOpts.valid.offset == 32
    # the two structs this one stands next to are what they were
    assert C.sizeof(abi.HorizonOpts) == 40 and C.sizeof(abi.WindowOpts) == 40
    assert "knot_offsets" not in [f[0] for f in abi.HorizonOpts._fields_]


def test_knots_calls_are_refused_without_a_handle(abi):
    """A call without a handle is LTP_ERR_INVALID_ARGUMENT whatever its opts hold: nothing is dereferenced, nothing launched, no
    crash on the malformed structs. Which check refuses what on a live handle is tests/test_gpu_knots.py::test_refusals."""
    lib = abi.lib()
    O = abi.KnotsOpts
    q, r = abi.Queries(), abi.Records()

    def call(o):
        return lib.ltp_sample_knots_batch(None, 0, 0, C.byref(q), C.byref(r), C.addressof(o) if o is not None else None, None, 0, None)
    good = dict(size=C.sizeof(O), format=0, n_knots=40, knot_offsets=64)     # a pointer nobody follows
    assert call(O(**good)) == INVALID
    assert call(None) == INVALID
    for bad in (dict(size=0), dict(size=C.sizeof(O) - 8), dict(size=C.sizeof(O) + 4), dict(format=2), dict(n_knots=0), dict(n_knots=-1),
                dict(n_knots=kc.MAX_KNOTS + 1), dict(knot_offsets=None)):
        assert call(O(**dict(good, **bad))) == INVALID, bad
    g = (C.c_int * 3)(0, 4, 9)
    assert lib.ltp_plan_knots_host(None, 0, None, None, None, None, None, 0, 3, g, None, None, None) == INVALID
    assert lib.ltp_plan_knots_host(None, 0, None, None, None, None, None, 0, 3, None, None, None, None) == INVALID


def test_host_grids_are_checked_by_the_python_wrapper(abi):
    """sampleKnots validates a host grid before it touches a device: the rule of ltp_plan_knots_host."""
    from longtermplanner_amd import LongTermPlanner
    check = LongTermPlanner._checked_knots
    for name, g in kc.GRIDS.items():
        assert np.array_equal(check(g), g) and check(list(map(int, g))).dtype == np.int32, name
    for bad in ([], [3, 2], [0, 5, 4, 9], [-1, 0], [0, (1 << 30) + 1], list(range(kc.MAX_KNOTS + 1)), [0.5, 1.5], [[0, 1], [2, 3]]):
        with pytest.raises(ValueError):
            check(bad)
    assert int(check([0, 1 << 30])[-1]) == 1 << 30


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
    const std::vector<int> knots = {0, 1, 2, 3, 8, 8, 16, 64, 240};
    const double qg = 0.5, z = 0.0;
    const int k = 3;
    const long long ok = ltp.planKnotsBatch(1, &qg, &z, &z, &z, &k, 0, knots, rows, &valid);
    std::printf("%lld %zu %zu\n", ok, rows.size(), valid.size());
    return rows.size() == 4u * 32u && valid.size() == 1u ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 2;
  }
}
'''


def test_dropin_header_with_plan_knots_batch_compiles_with_plain_gxx(abi, tmp_path):
    src = tmp_path / "knots.cc"
    src.write_text(DROPIN)
    exe = tmp_path / "knots"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "longtermplanner_amd"), "-lltp_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "longtermplanner_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_knots_ranges_on_the_host(tmp_path, flags):
    """knots_below against a linear count on valid grids; on contract-breaking grids every count in [0, N], every staged offset in
    [0, 2^30], no index outside the grid. A stand-alone host program, compiled here, once more with the sanitizers."""
    exe = tmp_path / "knots_ranges_test"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "longtermplanner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "knots_ranges_test.cc"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]


@pytest.fixture(scope="module")
def oracle_plans(oracle_mod):
    """50 panda plans of the CPU oracle with their trajectories, packed into the full-row layout (computed once, not modified)."""
    from longtermplanner_amd import generate_queries, limit_set
    dof, lim = limit_set("panda")
    n = 50
    qs = [np.ascontiguousarray(x) for x in generate_queries(n, lim, seed=4242)]
    orc = oracle_mod.Oracle(dof, TS, **lim)
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


@pytest.mark.parametrize("grid", ["mpc", "duplicates", "from37", "one"])
def test_checker_against_a_plain_loop(oracle_plans, grid):
    """The checker's gather, hold rule and `valid` are what a loop over (plan, w) reads from the oracle's own trajectories; its
    stretch count is what a loop over the samples counts."""
    import torch
    dof, trajs, full, offsets, lens, t_scaled = oracle_plans
    g = kc.GRIDS[grid]
    N = len(g)
    n = len(trajs)
    k = draw_starts(np.random.default_rng(99), lens, t_scaled, int(g[-1]) + 1, 1)
    assert np.any(k < 0) and np.any(k >= lens) and np.any((k > 0) & (k < lens))
    first, count = 3, n - 5
    exp, valid, planned = hc.expected(torch.from_numpy(full), torch.from_numpy(offsets), torch.from_numpy(lens), torch.from_numpy(k[first:first + count]),
                                      g, dof, first, count)
    exp = exp.numpy().view(np.float64)
    assert exp.shape == (count, 4, dof, N)
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
            t = k0 + int(g[w])
            n_real += t < L
            held += t >= L
            for x, arr in enumerate(arrs):
                for j in range(dof):
                    want = arr[j][t] if t < L else (arr[j][L - 1] if x == 0 else 0.0)
                    assert exp[i, x, j, w].tobytes() == np.float64(want).tobytes(), (i, x, j, w)
        assert int(valid[i]) == n_real
    assert held > 0
    # stretches and skipped: per joint, label every sample of the trajectory with its stretch, then look at the knots' labels
    sw = kc.switch_indices(t_scaled)
    got, got_skipped = kc.stretches(k, g, lens, t_scaled), kc.skipped(k, g, lens, t_scaled)
    for p in range(n):
        L = int(lens[p])
        most, skip = 0, False
        for j in range(dof if L > 0 else 0):
            label = np.zeros(L, dtype=np.int64)
            for s in sw[p, j]:
                if 0 < s < L:
                    label[int(s):] += 1                          # equal switch indices add equal steps: the labels stay ordered
            label = np.unique(label, return_inverse=True)[1]     # consecutive numbers
            ts = [max(int(k[p]), 0) + int(x) for x in g]
            mine = sorted({int(label[t]) for t in ts if t < L})
            most = max(most, len(mine))
            skip |= bool(mine) and mine[-1] - mine[0] + 1 > len(mine)
        assert got[p] == most and bool(got_skipped[p]) == skip, (p, got[p], most, got_skipped[p], skip)


@pytest.mark.parametrize("grid", ["mpc", "geometric"])
def test_aimed_starts_put_a_stretch_between_two_knots(oracle_plans, grid):
    """Every start kc.aimed_starts changes is >= 0 and gives its plan a skipped stretch with a real knot before and after it (by
    the plain-loop-pinned kc.skipped); plans it leaves alone keep their start; most plans of the oracle's batch are changed."""
    dof, trajs, full, offsets, lens, t_scaled = oracle_plans
    g = kc.GRIDS[grid]
    k = draw_starts(np.random.default_rng(7), lens, t_scaled, int(g[-1]) + 1, 1)
    ka = kc.aimed_starts(k, g, lens, t_scaled)
    changed = ka != k
    assert ka.dtype == np.int32 and np.all(ka[changed] >= 0) and np.all(lens[changed] > 0)
    assert np.all(kc.skipped(ka, g, lens, t_scaled)[changed]) and np.mean(changed) > 0.5
