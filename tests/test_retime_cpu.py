"""CPU-side checks of the retime feature (ltp_retime_batch / ltp_plan_retimed_host, include/ltp_hip.h): the symbols, the struct
layout the Python binding assumes, the drop-in overloads, and the checker (tests/retime_checker.py) against the CPU oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import retime_checker as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def abi():
    from longtermplanner_amd import _abi
    _abi.build()
    return _abi


def test_retime_entry_points_are_exported_and_refuse_a_null_handle(abi):
    lib = C.CDLL(abi.LIB_PATH)
    assert hasattr(lib, "ltp_retime_batch") and hasattr(lib, "ltp_plan_retimed_host")
    L = abi.lib()
    o = abi.RetimeOpts(C.sizeof(abi.RetimeOpts), None, 1.0, None, 0, None)
    assert L.ltp_retime_batch(None, 0, None, None, C.addressof(o), None, None) == 1          # LTP_ERR_INVALID_ARGUMENT
    assert L.ltp_plan_retimed_host(None, 0, None, None, None, None, None, 0.0, None, None, None) == 1


def test_retime_opts_layout_matches_the_header(abi, tmp_path):
    src = tmp_path / "offsets.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ltp_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ltp_retime_opts), offsetof(ltp_retime_opts, size), '
                   'offsetof(ltp_retime_opts, t_target), offsetof(ltp_retime_opts, t_uniform), offsetof(ltp_retime_opts, group), '
                   'offsetof(ltp_retime_opts, n_groups), offsetof(ltp_retime_opts, group_time)); return 0; }\n')
    exe = tmp_path / "offsets"
    subprocess.check_call(["g++", "-x", "c++", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    R = abi.RetimeOpts
    want = [C.sizeof(R)] + [getattr(R, f).offset for f in ("size", "t_target", "t_uniform", "group", "n_groups", "group_time")]
    assert got == want
    assert got[0] % 8 == 0


def test_dropin_timed_overloads_compile(tmp_path):
    src = tmp_path / "timed.cc"
    src.write_text('#include "long_term_planner/long_term_planner.h"\n'
                   'using long_term_planner::LongTermPlanner; using long_term_planner::Trajectory; using long_term_planner::BatchTrajectory;\n'
                   'bool f(LongTermPlanner& p, const std::vector<double>& g, const std::vector<double>& q, Trajectory& t) {\n'
                   '  bool (LongTermPlanner::*ref)(const std::vector<double>&, const std::vector<double>&, const std::vector<double>&,\n'
                   '                               const std::vector<double>&, Trajectory&) = &LongTermPlanner::planTrajectory;\n'
                   '  (void)ref; BatchTrajectory b; const double d[1] = {2.0};\n'
                   '  p.planTrajectoryBatchTimed(1, g.data(), q.data(), q.data(), q.data(), d, b);\n'
                   '  return p.planTrajectory(g, q, q, q, 1.5, t); }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)])


@pytest.mark.parametrize("name", ["panda", "ref"])
def test_checker_at_the_optimum_reproduces_plan_batch(oracle_mod, name):
    """T_q = T*: the checker's timeScaling of every non-slowest joint is planTrajectory's, bit for bit."""
    from longtermplanner_amd import generate_queries, limit_set
    dof, lim = limit_set(name)
    orc = oracle_mod.Oracle(dof, 0.001, **lim)
    qg, q0, v0, a0 = generate_queries(2000, lim, seed=4242)
    orec = orc.plan_batch(qg, q0, v0, a0)
    elig = rc.oracle_eligible(orec)
    assert elig.sum() > 1500
    T = rc.t_star(orec)
    checked = 0
    for q in np.nonzero(elig)[0]:
        for j in range(dof):
            if j == orec["slowest"][q]:
                continue
            ok, t, vd, mod, case = orc.time_scaling(j, qg[q, j], q0[q, j], v0[q, j], a0[q, j], orec["dir"][q, j], T[q])
            if rc.needs_fallback(t):
                t = orec["t_opt"][q, j]
            assert np.array_equal(t.view(np.int64), orec["t_scaled"][q, j].view(np.int64)), (q, j)
            assert np.float64(vd).view(np.int64) == orec["v_drive"][q, j].view(np.int64), (q, j)
            assert mod == orec["mod"][q, j], (q, j)
            checked += 1
    assert checked > 1500 * (dof - 1)


@pytest.mark.parametrize("k", [1.5, 3.0, 10.0])
def test_retimed_plans_reach_the_goal_in_the_requested_time(oracle_mod, k):
    """The retime rule gives usable trajectories: end within 5e-3 of the goal, v = a = 0 at the end, and the achieved duration in
    the reference's accept window [T - 0.1, T + 0.01 + Ts] (cc:398-405)."""
    from longtermplanner_amd import generate_queries, limit_set
    dof, lim = limit_set("panda")
    Ts = 0.001
    orc = oracle_mod.Oracle(dof, Ts, **lim)
    qg, q0, v0, a0 = generate_queries(300, lim, seed=777)
    orec = orc.plan_batch(qg, q0, v0, a0)
    elig = rc.oracle_eligible(orec)
    T = k * rc.t_star(orec)
    rec, retimed, cases = rc.retime(orc, orec, qg, q0, v0, a0, T)
    assert retimed.sum() == elig.sum() > 250
    for q in np.nonzero(retimed)[0]:
        n, qq, vv, aa, jj = rc.trajectory(orc, rec, q, q0, v0, a0)
        assert n == rec["traj_len"][q] > 0
        assert np.max(np.abs(qq[:, -1] - qg[q])) < 5e-3, q
        assert np.all(vv[:, -1] == 0.0) and np.all(aa[:, -1] == 0.0), q
        dur = (n - 1) * Ts
        assert T[q] - 0.1 <= dur <= T[q] + 0.01 + Ts, (q, dur, T[q])
    # most joints take a closed form (c1 / c2); a handful of tiny motions fall back
    assert cases[:, 0].sum() < 0.01 * cases.sum()
    assert (cases[:, 1].sum() + cases[:, 2].sum()) > 0.9 * cases.sum()
