"""Stop plans (ltp_plan_stop_batch), the part that needs no GPU: the checker tests/stop_checker.py against an independent path
through the oracle, the class census of the batches the GPU tests plan, the check modes, and the options struct."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import stop_checker as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _random_states(lim, n, seed):
    """Start states of the project's generator plus states inside planned trajectories' reach: all pass checkInputs or are dropped."""
    from longtermplanner_amd.synthetic import generate_queries
    _, q0, v0, a0 = generate_queries(n, lim, seed=seed)
    return q0, v0, a0


@pytest.mark.parametrize("limits", ["panda", "ref"])
def test_checker_equals_one_joint_plans_towards_the_standstill(oracle_mod, limits):
    """A stop plan's records are what planTrajectory holds for a joint whose goal is its standstill position (the early exit of
    optSwitchTimes, cc:100-107, then cc:50-55): for every joint, a 1-DoF planner with that joint's limits, planning towards
    fl(q_0 + q_stop), gives the checker's t_opt, t_scaled, dir and mod bit for bit, and its rows are the composed 7-joint rows over
    its own length; behind it the composed rows rest: the last position, and +0.0 in v, a and j."""
    from longtermplanner_amd.synthetic import limit_set
    dof, lim = limit_set(limits)
    orc = oracle_mod.Oracle(dof, sc.TS, **lim)
    q0, v0, a0 = _random_states(lim, 300, seed=4242)
    E = sc.expected_stop(orc, q0, v0, a0, "inputs")
    n_ok = 0
    for p in np.nonzero(E["accepted"])[0]:
        assert E["status"][p] == 0
        rows = E["rows"][p]
        L = int(E["traj_len"][p])
        assert rows.shape == (4, dof, L)
        n_ok += 1
        for j in range(dof):
            one = oracle_mod.Oracle(1, sc.TS, *[[lim[k][j]] for k in ("q_min", "q_max", "v_max", "a_max", "j_max")])
            tr = one.plan_trajectory([E["q_stop"][p, j]], [q0[p, j]], [v0[p, j]], [a0[p, j]])
            assert tr["status"] != 0
            assert _bits(tr["t_opt"][0], E["t_opt"][p, j]) and _bits(tr["t_scaled"][0], E["t_scaled"][p, j])
            assert _bits(tr["dir"][0], E["dir"][p, j]) and int(tr["mod"][0]) == 0 == int(E["mod"][p, j])
            assert _bits(tr["v_drive"][0], E["v_drive"][p, j])
            Lj = tr["length"]
            assert 1 <= Lj <= L and (j != E["slowest"][p] or Lj == L)
            for arr, name in enumerate("qvaj"):
                assert _bits(tr[name][0], rows[arr, j, :Lj]), (p, j, name)
            assert _bits(rows[0, j, Lj:], np.full(L - Lj, rows[0, j, Lj - 1]))
            assert _bits(rows[1:, j, Lj:], np.zeros((3, L - Lj)))
    assert n_ok >= 250


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_gpu_batches_reach_every_class(oracle_mod, name):
    S = sc.states(oracle_mod, name)
    totals = sc.census_totals(sc.census(S["orc"], S["v0"], S["a0"]))
    print(name, totals)
    for k in sc.CLASSES:
        assert totals[k] >= sc.MIN_LANES, (name, k, totals)
    lanes = S["v0"].size
    assert sum(totals[k] for k in sc.DIR_CLASSES) == lanes == sum(totals[k] for k in sc.PHASE_CLASSES)


def test_check_mode_truth_table(oracle_mod):
    """"inputs" is checkInputs; "braking" admits what fails only on q, v or the third rule and rejects |a_0| > a_max; NaN passes both."""
    lim = dict(q_min=[-3.14], q_max=[3.14], v_max=[1.0], a_max=[2.0], j_max=[15.0])
    orc = oracle_mod.Oracle(1, sc.TS, **lim)
    table = [  # q_0, v_0, a_0, inputs, braking
        (0.0, 0.0, 0.0, True, True),
        (3.5, 0.0, 0.0, False, True),          # q outside
        (0.0, 1.5, 0.0, False, True),          # |v| > v_max
        (0.0, 0.95, 2.0, False, True),         # the third rule alone: 0.95 + 0.5 * 4 / 15 > 1
        (0.0, 0.0, 2.0, True, True),           # |a| == a_max is admitted
        (0.0, 0.0, np.nextafter(2.0, 3.0), False, False),
        (0.0, 0.0, -2.5, False, False),
        (np.nan, 0.0, 0.0, True, True),
        (0.0, np.nan, np.nan, True, True),
    ]
    q0, v0, a0 = (np.array([[row[k]] for row in table]) for k in range(3))
    assert list(sc.accepted(orc, q0, v0, a0, "inputs")) == [row[3] for row in table]
    assert list(sc.accepted(orc, q0, v0, a0, "braking")) == [row[4] for row in table]
    E = sc.expected_stop(orc, q0, v0, a0, "braking")
    assert list(E["status"][:5]) == [0] * 5 and list(E["status"][5:7]) == [sc.INVALID_INPUT] * 2
    assert E["status"][7] == 0                                   # a NaN position does not reach the times
    assert E["status"][8] == sc.NONFINITE | sc.NO_SLOWEST and E["traj_len"][8] == 0
    assert E["traj_len"][0] == 1 and E["slowest"][0] == 0 and E["t_required"][0] == 0.0     # a robot at rest
    assert np.all(np.isnan(E["q_stop"][5:7])) and np.all(E["t_scaled"][5:7] == 0.0)


def test_stop_opts_are_validated_before_anything_runs():
    """ltp_stop_opts is 16 bytes, the binding declares the header's fields, and a missing struct, a bad size or an unknown check is
    LTP_ERR_INVALID_ARGUMENT before any device work (checked here without a device and without a handle)."""
    from longtermplanner_amd import _abi as abi
    lib = abi.lib()
    O = abi.StopOpts
    assert C.sizeof(O) == 16
    text = open(os.path.join(ROOT, "include", "ltp_hip.h")).read()
    fields = re.search(r"typedef struct \{([^}]*)\} ltp_stop_opts;", text, flags=re.S).group(1)
    assert re.findall(r"^\s*(?:unsigned|int|double\*) (\w+);", fields, flags=re.M) == [f[0] for f in O._fields_]
    assert re.search(r"#define LTP_STOP_CHECK_INPUTS\s+0\b", text) and re.search(r"#define LTP_STOP_CHECK_BRAKING\s+1\b", text)
    assert abi.STOP_CHECKS == {"inputs": 0, "braking": 1}

    def call(o):
        return lib.ltp_plan_stop_batch(None, 0, None, None, C.addressof(o) if o is not None else None, None, None)
    INVALID = 1
    assert call(None) == INVALID
    for bad in (O(0, 0, None), O(8, 0, None), O(20, 0, None), O(16, 2, None), O(16, -1, None)):
        assert call(bad) == INVALID
    assert call(O(16, 1, None)) == INVALID      # well-formed: refused for the null handle instead (same code, later check)
    assert lib.ltp_plan_stop_host(None, 0, None, None, None, 0, None, None, None, None) == INVALID
