"""Stop states of the census batches (test infrastructure, not a test module, like stop_checker.py, which it builds on).

The stop entries (ltp_plan_stop_batch, ltp_stop_knots_batch) were pinned on panda / S-ref / 30-DoF states at 1 ms. Here the states
come from the three families that pin the planner and the samplers class by class: every batch of run_census.BATCHES (coarse and
dyadic: sample times of the order of the phases, switching times on exact multiples of the sample time) and the soft dense batch of
branch_census (jerk-dominated limits). knot_states takes states (q, v, a) at seeded random samples of the ORACLE's rows, with the
acceleration clamped to +-a_max as planStopFrom does; expected is stop_checker.expected_stop of those states, once per process;
stop_runs is the run census of the resulting stop records; wide_states is the one batch with more joints than joint slots, built so
that the slowest joint ties inside a slot. The totals, the floors and what a batch does not reach are pinned in
tests/test_stop_census_cpu.py; tests/test_gpu_stop_runs.py compares the device with the checker class by class.
"""
import numpy as np

import branch_census as bc
import run_census as rc
import stop_checker as sc

SOFT_DENSE = "soft_dense"
ROWS_N = 600                                   # plans of bc.DENSE_BATCH whose rows are taken (tests/test_gpu_branches.py's ROWS_N)
BATCHES = tuple(rc.BATCHES) + (SOFT_DENSE,)
SEED = 31
MAX_STATES = 1500
# batch -> samples per plan: two, and three of the soft dense batch, whose rows are long against its plan count. ref_0.05 takes
# four of EVERY plan (4000 states; its stop rows have at most 19 samples): a stop plan of at most four samples starts within the
# last few samples of a 20-150 sample row, 3 % of a uniform draw, and the floor of tests/test_stop_census_cpu.py asks for 100.
PER_PLAN = {name: 2 for name in rc.BATCHES}
PER_PLAN[SOFT_DENSE] = 3
PER_PLAN["ref_0.05"] = 4
MAX_OF = {"ref_0.05": 4000}
FLOOR = bc.FLOOR


def source(oracle_mod, name):
    """(oracle, limits, Ts, queries, records, rows [(length, q, v, a, j) or None], census, describe) of the batch the states are
    drawn from; `describe` is rc.describe or bc.describe, to be given that census."""
    if name == SOFT_DENSE:
        dof, n, ts = bc.DENSE_BATCH
        orc, lim, qs, rec, cen = bc.soft_batch(oracle_mod, dof, n, ts)
        return orc, lim, ts, qs, rec, _soft_rows(oracle_mod), cen, bc.describe
    orc, lim, ts, qs, rec, cen = rc.batch(oracle_mod, name)
    return orc, lim, ts, qs, rec, rc.all_rows(oracle_mod, name), cen, rc.describe


def _soft_rows(oracle_mod, cache={}):
    if not cache:
        dof, n, ts = bc.DENSE_BATCH
        orc, lim, qs, rec, cen = bc.soft_batch(oracle_mod, dof, n, ts)
        cache["rows"] = [rc.oracle_rows(orc, rec, qs, p) if rec["status"][p] != 0 else None for p in range(ROWS_N)]
    return cache["rows"]


def knot_states(oracle_mod, name, per_plan=None, seed=SEED, max_states=None, cache={}):
    """States at seeded random samples of the oracle's rows of a batch: dict orc, lim, ts, dof, q0, v0, a0 ([n][dof], a0 clamped to
    +-a_max), a_raw (the sampled acceleration before the clamp), plan and sample ([n]: the source plan in the batch and the sample
    of its rows). per_plan samples (with replacement) of each of at most max_states // per_plan planned plans, the plans drawn
    without replacement. Once per process and left unchanged."""
    per_plan = PER_PLAN[name] if per_plan is None else per_plan
    max_states = MAX_OF.get(name, MAX_STATES) if max_states is None else max_states
    key = (name, per_plan, seed, max_states)
    if key not in cache:
        orc, lim, ts, qs, rec, rows, cen, _ = source(oracle_mod, name)
        rng = np.random.default_rng(seed)
        planned = np.array([p for p, r in enumerate(rows) if r is not None and r[0] > 0], dtype=np.int64)
        take = min(len(planned), max_states // per_plan)
        plans = np.sort(rng.choice(planned, take, replace=False))
        plan, sample, q, v, a = [], [], [], [], []
        for p in plans:
            L, rq, rv, ra, _ = rows[p]
            for k in rng.integers(0, L, per_plan):
                plan.append(p); sample.append(int(k))
                q.append(rq[:, k]); v.append(rv[:, k]); a.append(ra[:, k])
        a_raw = np.ascontiguousarray(np.array(a))
        cache[key] = dict(name=name, orc=orc, lim={k: list(x) for k, x in lim.items()}, ts=ts, dof=orc.dof,
                          q0=np.ascontiguousarray(np.array(q)), v0=np.ascontiguousarray(np.array(v)),
                          a0=np.ascontiguousarray(np.clip(a_raw, -orc.a_max, orc.a_max)), a_raw=a_raw,
                          plan=np.array(plan, dtype=np.int64), sample=np.array(sample, dtype=np.int64))
    return cache[key]


def census(oracle_mod, name, cache={}):
    """stop_checker.census of the (clamped) states of a batch: dict class -> bool [n][dof]."""
    if name not in cache:
        S = knot_states(oracle_mod, name)
        cache[name] = sc.census(S["orc"], S["v0"], S["a0"])
    return cache[name]


def expected(oracle_mod, name, check="braking", exact_pow=False, rows=False, cache={}):
    """stop_checker.expected_stop of the states of a batch under the batch's own sample time, once per process (exact_pow: by the
    oracle's exact-pow twin)."""
    key = (name, check, exact_pow)
    if key not in cache or (rows and cache[key]["rows"] is None):
        S = knot_states(oracle_mod, name)
        orc = oracle_mod.Oracle(S["dof"], S["ts"], exact_pow=True, **S["lim"]) if exact_pow else S["orc"]
        cache[key] = sc.expected_stop(orc, S["q0"], S["v0"], S["a0"], check, rows=rows)
    return cache[key]


def stop_runs(oracle_mod, name, cache={}):
    """The run census (run_census.census) of the stop records of a batch, expected(check="braking")."""
    if name not in cache:
        E = expected(oracle_mod, name)
        cache[name] = rc.census(E["t_scaled"], E["traj_len"], knot_states(oracle_mod, name)["ts"])
    return cache[name]


# the batches in which the standstill time of the slowest joint is shared by a second joint in at least FLOOR states: joints with the
# same limits that rest at a coarse sample time (t_stop = a_max / j_max each), the two dyadic joints. There the strict comparison of
# the slowest-joint scan (cc:31-39: the first joint wins) decides `slowest`.
TIED = ("panda_0.1", "ref_1", "ref_0.05", "soft_1", "dyadic_two")


def tied(E):
    """[n]: the largest t_opt[..][6] of the state is held by two joints or more."""
    t6 = E["t_opt"][:, :, 6]
    return (t6 == t6.max(axis=1, keepdims=True)).sum(axis=1) >= 2


WIDE_DOF, WIDE_SLOTS, WIDE_N = 24, 8, 600


def wide_states(oracle_mod, cache={}):
    """More joints than joint slots at a coarse sample time, with ties INSIDE a slot: the first WIDE_N states of soft_1 (Ts 1) spread
    over 24 joints, joint j a copy — limits and state — of source joint (j % 8) % 7. The stop kernel deals joints j, j + 8, j + 16 to
    one wave (kMaxJointSlots = 8), so in every state the slowest joint ties with its two copies in its own wave (and joint 7 with
    joint 0 across waves): the scan's strict comparison inside a wave decides `slowest`, which no batch of at most 8 joints can
    show. Dict like knot_states, without a_raw, plan and sample; the source state of row i is row i of knot_states("soft_1")."""
    if not cache:
        S = knot_states(oracle_mod, "soft_1")
        jm = (np.arange(WIDE_DOF) % WIDE_SLOTS) % S["dof"]
        lim = {k: [v[i] for i in jm] for k, v in S["lim"].items()}
        cache.update(name="soft_1_wide", orc=oracle_mod.Oracle(WIDE_DOF, S["ts"], **lim), lim=lim, ts=S["ts"], dof=WIDE_DOF, source=jm,
                     **{k: np.ascontiguousarray(S[k][:WIDE_N][:, jm]) for k in ("q0", "v0", "a0")})
    return cache


def describe(cen, lanes):
    """The stop_checker.CLASSES of the lanes in `lanes` (a bool mask [n][dof], or [n] for whole states) of a census (`census`), for
    assertion messages."""
    shape = cen[sc.CLASSES[0]].shape
    lanes = np.asarray(lanes, dtype=bool)
    if lanes.ndim == 1:
        lanes = np.broadcast_to(lanes[:, None], shape)
    where = np.argwhere(lanes)
    if where.size == 0:
        return "no lanes"
    hit = {k: int((cen[k] & lanes).sum()) for k in sc.CLASSES}
    first = ", ".join(f"(state {p}, joint {j}: " + " ".join(k for k in sc.CLASSES if cen[k][p, j]) + ")" for p, j in where[:3])
    return f"{len(where)} lanes; classes {{" + ", ".join(f"{k}: {c}" for k, c in hit.items() if c) + "}; first " + first


def describe_source(oracle_mod, name, states):
    """describe of the SOURCE lanes of the states in `states` (a bool mask [n]): the run-census classes (branch-census classes for
    the soft dense batch) of the plans they were sampled from, and the first samples."""
    S = knot_states(oracle_mod, name)
    *_, cen, desc = source(oracle_mod, name)
    states = np.asarray(states, dtype=bool)
    n_src = len(cen["case"] if name == SOFT_DENSE else cen["traj_len"])
    plans = np.zeros(n_src, dtype=bool)
    plans[S["plan"][states]] = True
    at = ", ".join(f"plan {p} sample {k}" for p, k in zip(S["plan"][states][:3], S["sample"][states][:3]))
    return f"sampled at {at}: {desc(cen, plans)}"


def present(oracle_mod, name):
    """The stop_checker.CLASSES a batch holds at all: each must be present in every GPU comparison of that batch."""
    t = sc.census_totals(census(oracle_mod, name))
    return tuple(k for k in sc.CLASSES if t[k] > 0)
