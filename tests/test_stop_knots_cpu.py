"""Stop horizons (ltp_stop_knots_batch), the part that needs no GPU: the checker tests/stop_knots_checker.py against an independent
path through tests/stop_checker.py, the strict mode's NaN mask, and the options struct."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import stop_checker as sc
import stop_knots_checker as skc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PLANS = 40
SEED = 4242


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


_ROWS = {}


def _oracle_rows(oracle_mod):
    """The oracle's trajectories of N_PLANS panda queries, one of them made invalid (|a_0| > a_max: no trajectory). Once per process:
    (orc, list of None | [3][dof][L] arrays of q, v, a)."""
    if not _ROWS:
        from longtermplanner_amd.synthetic import generate_queries, limit_set
        dof, lim = limit_set("panda")
        orc = oracle_mod.Oracle(dof, sc.TS, **lim)
        qg, q0, v0, a0 = generate_queries(N_PLANS, lim, seed=SEED)
        a0[5, 0] = 2.0 * lim["a_max"][0]
        trajs = []
        for p in range(N_PLANS):
            tr = orc.plan_trajectory(qg[p], q0[p], v0[p], a0[p])
            trajs.append(None if tr["length"] == 0 else np.stack([tr["q"], tr["v"], tr["a"]]))
        _ROWS.update(orc=orc, trajs=trajs)
    return _ROWS["orc"], _ROWS["trajs"]


def _knot_states(trajs, dof, k, g):
    """What ltp_sample_knots_batch stores in planes q, v, a: sample max(k, 0) + g[w]; past the end (q_last, +0.0, +0.0); NaN for a
    plan without a trajectory. [n][3][dof][N]."""
    n, N = len(trajs), len(g)
    out = np.full((n, 3, dof, N), np.nan)
    for p, tr in enumerate(trajs):
        if tr is None:
            continue
        L = tr.shape[2]
        t = max(int(k[p]), 0) + np.asarray(g, dtype=np.int64)
        real = t < L
        out[p][:, :, real] = tr[:, :, t[real]]
        out[p, 0][:, ~real] = tr[0, :, L - 1][:, None]
        out[p, 1:][:, :, ~real] = 0.0
    return out


def _starts(trajs, g, seed):
    """A start per plan, by plan index mod 4: uniform inside the trajectory, -3, traj_len + 5, ten samples before the end."""
    rng = np.random.default_rng(seed)
    lens = [0 if tr is None else tr.shape[2] for tr in trajs]
    return np.array([(int(rng.integers(0, max(L, 1))), -3, L + 5, L - 10)[p % 4] for p, L in enumerate(lens)], dtype=np.int32)


@pytest.mark.parametrize("grid", ["mpc", "duplicates"])
def test_checker_equals_the_stop_checker_on_the_clamped_states(oracle_mod, grid):
    """The helper's q_stop / t_stop are stop_checker.expected_stop(..., check="braking")'s q_closed / t_opt[..., 6] on the knot
    states with the acceleration clamped, bit for bit; knots past the end and a plan without a trajectory occur."""
    orc, trajs = _oracle_rows(oracle_mod)
    dof = orc.dof
    g = skc.GRIDS[grid]
    N = len(g)
    k = _starts(trajs, g, 7)
    rows = _knot_states(trajs, dof, k, g)
    lens = np.array([0 if tr is None else tr.shape[2] for tr in trajs])
    assert np.count_nonzero(lens == 0) >= 1 and np.isnan(rows[lens == 0]).all()
    past = (np.maximum(k, 0)[:, None] + g[None, :].astype(np.int64) >= lens[:, None]) & (lens > 0)[:, None]
    assert past.any() and (~past & (lens > 0)[:, None]).any() and np.count_nonzero(k < 0) > 0 and np.count_nonzero(k >= lens) > 0
    got = skc.expected(orc, rows, orc.a_max, skc.CLAMP)
    # the independent path: count * N states [dof], clamped, through the stop plans' checker
    states = np.ascontiguousarray(rows.transpose(0, 3, 1, 2).reshape(-1, 3, dof))
    a_cl = np.clip(states[:, 2], -orc.a_max, orc.a_max)
    with np.errstate(invalid="ignore"):
        E = sc.expected_stop(orc, states[:, 0], states[:, 1], a_cl, check="braking", rows=False)
    q_ref = E["q_closed"].reshape(len(trajs), N, dof).transpose(0, 2, 1)
    t_ref = E["t_opt"][..., 6].reshape(len(trajs), N, dof).transpose(0, 2, 1)
    assert _bits(got[:, 0], q_ref) and _bits(got[:, 1], t_ref)
    # a resting robot stops where it is, in no time
    rest = np.broadcast_to(past[:, None, :], got[:, 0].shape)
    assert _bits(got[:, 0][rest], np.broadcast_to(rows[:, 0], got[:, 0].shape)[rest]) and np.all(got[:, 1][rest] == 0.0)
    assert np.isnan(got[lens == 0]).all()


def test_strict_mode_is_nan_exactly_where_the_acceleration_is_beyond_a_max(oracle_mod):
    """STRICT: NaN in both planes exactly where |a| > a_max (a NaN state is NaN as well, but by arithmetic), the CLAMP values' bits
    elsewhere — where the clamp is the identity. Sampled accelerations exceed a_max by rounding: at least 8 such elements occur."""
    orc, trajs = _oracle_rows(oracle_mod)
    g = np.arange(0, 400, 1, dtype=np.int32)
    rows = _knot_states(trajs, orc.dof, np.zeros(len(trajs), dtype=np.int32), g)
    mask = skc.beyond(rows[:, 2], orc.a_max)
    print("elements with |a| > a_max:", int(mask.sum()), "of", mask.size, "in", int(mask.any(axis=(1, 2)).sum()), "plans")
    assert int(mask.sum()) >= 8
    strict = skc.expected(orc, rows, orc.a_max, skc.STRICT)
    clamp = skc.expected(orc, rows, orc.a_max, skc.CLAMP)
    planned = ~np.isnan(rows[:, 0])
    for plane in (0, 1):
        assert np.array_equal(np.isnan(strict[:, plane]) & planned, mask)
        assert _bits(strict[:, plane][~mask], clamp[:, plane][~mask])
    assert not np.isnan(clamp[:, :][np.broadcast_to(planned[:, None], clamp.shape)]).any()


def test_stop_knots_opts_are_validated_before_anything_runs():
    """ltp_stop_knots_opts is 40 bytes, the binding declares the header's fields, and a missing struct, a bad size, a bad n_knots or an
    unknown accel is LTP_ERR_INVALID_ARGUMENT before any device work (checked here without a device and without a handle)."""
    from longtermplanner_amd import _abi as abi
    O = abi.StopKnotsOpts
    assert C.sizeof(O) == 40
    text = open(os.path.join(ROOT, "include", "ltp_hip.h")).read()
    fields = re.search(r"typedef struct \{([^}]*)\} ltp_stop_knots_opts;", text, flags=re.S).group(1)
    assert re.findall(r"^\s*(?:unsigned|int|const int\*|int\*) (\w+);", fields, flags=re.M) == [f[0] for f in O._fields_]
    assert re.search(r"#define LTP_STOP_ACCEL_CLAMP\s+0\b", text) and re.search(r"#define LTP_STOP_ACCEL_STRICT\s+1\b", text)
    assert (abi.STOP_ACCEL_CLAMP, abi.STOP_ACCEL_STRICT) == (skc.CLAMP, skc.STRICT) == (0, 1)
    lib = abi.lib()
    INVALID = 1
    grid = (C.c_int * 4)(0, 1, 2, 3)
    gp = C.cast(grid, C.c_void_p).value

    def call(o):
        return lib.ltp_stop_knots_batch(None, 0, 0, None, None, C.addressof(o) if o is not None else None, None, 0, None)
    assert call(None) == INVALID
    for bad in (O(0, 4, 0, 0, gp), O(32, 4, 0, 0, gp), O(44, 4, 0, 0, gp), O(40, 0, 0, 0, gp), O(40, 513, 0, 0, gp), O(40, 4, 2, 0, gp),
                O(40, 4, -1, 0, gp), O(40, 4, 0, 0, None)):
        assert call(bad) == INVALID
    assert call(O(40, 4, 1, 0, gp)) == INVALID      # well-formed: refused for the null handle instead (same code, later check)
    assert lib.ltp_stop_knots_elements(None, 10, 40) == 0
    assert lib.ltp_plan_stop_knots_host(None, 0, None, None, None, None, None, 0, 4, grid, 0, None, None, None) == INVALID
