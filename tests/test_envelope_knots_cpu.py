"""Horizon envelopes (ltp_envelope_knots_batch, include/ltp_hip.h) without a device: the symbols, the options struct, the validation
that runs before anything is launched, the drop-in header's new method under plain g++, the host arithmetic of the kernel's interval
walk (tests/cpp/envelope_knots_ranges_test.cc, also under the address and undefined-behaviour sanitizers), and the yardstick of the
GPU tests (tests/envelope_knots_checker.py) against a plain loop over the CPU oracle's trajectories."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import envelope_knots_checker as ec
from horizon_checker import TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NAMES = ("ltp_envelope_knots_elements", "ltp_envelope_knots_batch", "ltp_plan_envelope_knots_host")


@pytest.fixture(scope="module")
def abi():
    from longtermplanner_amd import _abi
    _abi.build()
    return _abi


def test_envelope_knots_symbols_are_declared_and_exported(abi):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltp_hip.h")).read(), flags=re.S)
    lib = C.CDLL(abi.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} is not declared in include/ltp_hip.h"
        assert n in abi.exported_symbols(), f"{n} is not declared in _abi._SIGNATURES"
        assert hasattr(lib, n), f"{n} is not exported"
    assert ec.MAX_INTERVALS == abi.MAX_KNOTS - 1 == 511
    from longtermplanner_amd import LongTermPlanner
    assert hasattr(LongTermPlanner, "envelopeKnots") and hasattr(LongTermPlanner, "planEnvelopeKnotsHost")
    # the header says which rule does not apply and which form the values have
    doc = open(os.path.join(ROOT, "include", "ltp_hip.h")).read()
    at = doc.index("HORIZON ENVELOPES")
    assert "ltp_set_envelope_mode" in doc[at:doc.index("} ltp_envelope_knots_opts;")]


def test_envelope_knots_opts_is_the_c_struct(abi):
    fields = re.search(r"typedef struct \{([^}]*)\} ltp_envelope_knots_opts;", open(os.path.join(ROOT, "include", "ltp_hip.h")).read(), flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    O = abi.EnvelopeKnotsOpts
    assert re.findall(r"(\w+);", fields) == [f[0] for f in O._fields_] == ["size", "n_intervals", "closed", "uniform_first", "edge_offsets",
                                                                         "first_sample", "valid"]
    assert C.sizeof(O) == 40
    assert O.edge_offsets.offset == 16 and O.first_sample.offset == 24 and O.valid.offset == 32
    assert C.sizeof(abi.KnotsOpts) == 40                         # the struct this one stands next to is what it was
    # the header's prototypes and _abi's agree in the number of arguments
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltp_hip.h")).read(), flags=re.S)
    for n in NAMES:
        args = re.search(r"\b%s\s*\(([^;]*)\);" % n, text, flags=re.S).group(1)
        assert len(args.split(",")) == len(abi._SIGNATURES[n][1]), n


def test_envelope_knots_calls_are_refused_without_a_handle(abi):
    """A call without a handle is LTP_ERR_INVALID_ARGUMENT whatever its opts hold: nothing is dereferenced, nothing launched, no
    crash on the malformed structs. Which check refuses what on a live handle is tests/test_gpu_envelope_knots.py::test_refusals."""
    lib = abi.lib()
    O = abi.EnvelopeKnotsOpts
    q, r = abi.Queries(), abi.Records()

    def call(o):
        return lib.ltp_envelope_knots_batch(None, 0, 0, C.byref(q), C.byref(r), C.addressof(o) if o is not None else None, None, 0, None)
    good = dict(size=C.sizeof(O), n_intervals=39, closed=0, edge_offsets=64)     # a pointer nobody follows
    assert call(O(**good)) == INVALID
    assert call(None) == INVALID
    for bad in (dict(size=0), dict(size=C.sizeof(O) - 8), dict(size=C.sizeof(O) + 4), dict(closed=2), dict(closed=-1), dict(n_intervals=0),
                dict(n_intervals=-1), dict(n_intervals=ec.MAX_INTERVALS + 1), dict(edge_offsets=None)):
        assert call(O(**dict(good, **bad))) == INVALID, bad
    assert lib.ltp_envelope_knots_elements(None, 10, 4) == 0
    g = (C.c_int * 3)(0, 4, 9)
    host = lib.ltp_plan_envelope_knots_host
    assert host(None, 0, None, None, None, None, None, 0, 2, g, 0, None, None, None) == INVALID
    assert host(None, 0, None, None, None, None, None, 0, 2, None, 0, None, None, None) == INVALID


def test_host_edges_are_checked_by_the_python_wrapper(abi):
    """envelopeKnots validates a host edge list through the knots rule (plus: at least two edges) before it touches a device; a
    call with a bad list never reaches the batch it is given."""
    from longtermplanner_amd import LongTermPlanner
    check = LongTermPlanner._checked_knots
    for name, g in ec.EDGE_GRIDS.items():
        assert np.array_equal(check(g), g), name
    assert "one" not in ec.EDGE_GRIDS and len(ec.GRIDS["one"]) == 1
    ltp = LongTermPlanner.__new__(LongTermPlanner)              # no handle, no device: the refusals below come first

    class NoBatch:
        class offsets:
            device = "cpu"
    for bad in ([], [11], ec.GRIDS["one"], [3, 2], [0, 5, 4, 9], [-1, 0], [0, (1 << 30) + 1], list(range(ec.MAX_INTERVALS + 2)), [0.5, 1.5],
                [[0, 1], [2, 3]]):
        with pytest.raises(ValueError):
            ltp.envelopeKnots(NoBatch, 0, 1, 0, bad)


DROPIN = r'''
#include "long_term_planner/long_term_planner.h"
#include <cstdio>
int main() {
  using namespace long_term_planner;
  std::vector<double> lo = {-1.0}, hi = {1.0}, one = {1.0};
  try {
    LongTermPlanner ltp(1, 0.001, lo, hi, one, one, one);
    std::vector<double> env;
    std::vector<int> valid;
    const std::vector<int> edges = {0, 1, 2, 3, 8, 8, 16, 64, 240};
    const double qg = 0.5, z = 0.0;
    const int k = 3;
    const long long ok = ltp.planEnvelopeKnotsBatch(1, &qg, &z, &z, &z, &k, 0, edges, true, env, &valid);
    std::printf("%lld %zu %zu\n", ok, env.size(), valid.size());
    return env.size() == 8u * 2u && valid.size() == 1u ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 2;
  }
}
'''


def test_dropin_header_with_plan_envelope_knots_batch_compiles_with_plain_gxx(abi, tmp_path):
    src = tmp_path / "envelope_knots.cc"
    src.write_text(DROPIN)
    exe = tmp_path / "envelope_knots"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "longtermplanner_amd"), "-lltp_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "longtermplanner_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_envelope_knots_ranges_on_the_host(tmp_path, flags):
    """The kernel's interval walk (ltp_intervals.hpp) over random cut lists. Valid grids: the stretches of interval w unite to
    exactly [a_w, min(b_w, len - 1)], in order, each inside one run; at most one interval is carried across a cut. All grids, the
    contract-breaking ones included: every index in [0, M), each pair written once, at most M + runs steps. A stand-alone host
    program, compiled here, once more with the sanitizers."""
    exe = tmp_path / "envelope_knots_ranges_test"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "longtermplanner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "envelope_knots_ranges_test.cc"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]


@pytest.fixture(scope="module")
def oracle_plans(oracle_mod):
    """60 panda plans of the CPU oracle with their trajectories, packed into the full-row layout (computed once, not modified)."""
    from longtermplanner_amd import generate_queries, limit_set
    dof, lim = limit_set("panda")
    n = 60
    qs = [np.ascontiguousarray(x) for x in generate_queries(n, lim, seed=4242)]
    orc = oracle_mod.Oracle(dof, TS, **lim)
    o = orc.plan_batch(*qs, sample=True)
    trajs = []
    for p in range(n):
        if o["status"][p] == 0:
            trajs.append((0, *[np.zeros((dof, 0))] * 4))
        else:
            trajs.append(orc.get_trajectory(o["t_scaled"][p], o["dir"][p], o["mod"][p], qs[1][p], qs[2][p], qs[3][p], o["v_drive"][p]))
    full, offsets, lens = ec.pack_full_rows(trajs, dof)
    assert np.mean(lens > 0) > 0.9
    return dof, trajs, full, offsets, lens


@pytest.mark.parametrize("closed", [0, 1])
@pytest.mark.parametrize("grid", ["duplicates", "from37", "n33"])
def test_checker_against_a_plain_loop(oracle_plans, grid, closed):
    """The checker's gather, clamp, per-interval reduction and `valid` are what a loop over (plan, joint, w, t) reads from the
    oracle's own trajectories: starts below 0, inside and at or past the end."""
    import torch
    dof, trajs, full, offsets, lens = oracle_plans
    g = ec.GRIDS[grid]
    M = len(g) - 1
    n = len(trajs)
    rng = np.random.default_rng(31 + closed)
    k = rng.integers(-5, lens.astype(np.int64) + 41).astype(np.int32)
    k[0::9] = -3
    k[1::9] = lens[1::9]
    k[2::9] = lens[2::9] - 1
    assert np.any(k < 0) and np.any(k >= lens) and np.any((k > 0) & (k < lens))
    first, count = 3, n - 5
    env, valid, planned = ec.expected(torch.from_numpy(full), torch.from_numpy(offsets), torch.from_numpy(lens), torch.from_numpy(k[first:first + count]),
                                      g, closed, dof, first, count, chunk=16)
    env = env.numpy()
    assert env.shape == (count, dof, M, 2)
    held = ended_in = singles = 0
    for i in range(count):
        L, q = trajs[first + i][0], trajs[first + i][1]
        assert bool(planned[i]) == (L > 0)
        if L == 0:
            assert int(valid[i]) == 0 and np.isnan(env[i]).all()
            continue
        k0 = max(int(k[first + i]), 0)
        n_real = 0
        for w in range(M):
            a = k0 + int(g[w])
            b = max(a, k0 + int(g[w + 1]) - 1 + closed)
            n_real += a < L
            held += a >= L
            ended_in += a < L <= b
            singles += a == b
            for j in range(dof):
                samples = [q[j][min(t, L - 1)] for t in range(a, b + 1)]
                assert env[i, j, w, 0].tobytes() == np.float64(min(samples)).tobytes(), (i, j, w)
                assert env[i, j, w, 1].tobytes() == np.float64(max(samples)).tobytes(), (i, j, w)
        assert int(valid[i]) == n_real
    assert held > 0 and ended_in > 0 and (singles > 0 or grid != "duplicates")
    # the acceptance rule accepts the yardstick itself, and refuses a value outside the samples, a far value and a NaN
    red = torch.from_numpy(env)
    bad, worst, share = ec.compare(red.clone(), red, planned)
    assert not bad.any() and worst == 0.0 and share == 1.0
    pi = int(np.nonzero(planned.numpy())[0][0])
    for change in (lambda x: x[pi, 0, 0, 0].sub_(1e-15), lambda x: x[pi, 0, 0, 1].add_(1e-15), lambda x: x[pi, 0, 0, 0].add_(1e-11),
                   lambda x: x[pi, 0, 0, 0].fill_(float("nan"))):
        other = red.clone()
        change(other)
        assert bool(ec.compare(other, red, planned)[0][pi])
