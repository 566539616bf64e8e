"""Which planner branches the test batches reach, from the CPU oracle alone (tests/branch_census.py): the exact census of the
7-joint soft batch, the floors every batch of tests/test_gpu_branches.py has to meet, and what the named limit sets do NOT reach.

The floors are conditions on the batches, not measurements: every timeScaling case 0-8 and every optSwitchTimes site in at least
20 lanes, at least 10 plans whose optSwitchTimes is false, at least 5 end-limit plans where rows are taken, at least half of the
scaled lanes outside c1 / c2. A batch that misses one gets more queries, never a lower floor."""
import numpy as np
import pytest

import branch_census as bc

from branch_census import DENSE_BATCH, FLOOR, RECORD_BATCHES, RETIME_BATCHES, RETIME_FACTORS, SEED, assert_floors, soft_batch


def test_soft_limits_are_jerk_dominated():
    lim = bc.soft_limits(7)
    v, a, j = (np.asarray(lim[k]) for k in ("v_max", "a_max", "j_max"))
    assert np.all(a * a / (2.0 * j) <= v), "generate_queries' premise: every query then passes checkInputs"
    assert np.count_nonzero(v <= a * a / j) >= 4, "most joints cannot reach a_max and v_max in one profile"
    assert (v[3], a[3], j[3]) == (1.0, 2.0, 15.0), "joint 3 is the reference's stiff joint"
    lim30 = bc.soft_limits(30)
    assert lim30["j_max"][7:14] == lim["j_max"] and len(lim30["q_min"]) == 30 and lim30["v_max"][29] == lim["v_max"][1]


def test_exact_census_of_the_seven_joint_batch(oracle_mod):
    """seed 5, 3000 queries, Ts 0.004. If one figure moves, the batch is no longer the one the GPU tests were sized for."""
    orc, lim, qs, rec, cen = soft_batch(oracle_mod, 7, 3000)
    t = cen["totals"]
    assert t["invalid"] == 0
    assert (t["planned"], t["end_limit"], t["not_planned"]) == (2952, 18, 30)
    assert t["opt_false"] == 30 and np.array_equal(~cen["opt_ok"].all(axis=1), rec["status"] == 0)
    assert t["cases"] == {0: 3902, 1: 4428, 2: 1896, 3: 904, 4: 170, 5: 3474, 6: 73, 7: 280, 8: 2693}
    assert t["sites"] == {1: 17916, 4: 12373, 8: 11981, 16: 9756, 32: 9348, 64: 2307, 128: 91, 256: 31}
    assert sum(t["cases"].values()) == 6 * (2952 + 18)                  # every joint but the slowest of every planned query
    assert abs(t["beyond_c2"] - 0.645) < 1e-3 and abs(t["cases"][0] / 17820 - 0.219) < 1e-3
    assert np.all(np.isfinite(rec["t_scaled"])) and np.all(np.isfinite(rec["t_opt"]))
    assert_floors(t)
    # the exact-pow twin (the reference of the "exact" pow rule) takes the same branches on this batch
    twin = soft_batch(oracle_mod, 7, 3000, exact_pow=True)[4]
    assert twin["totals"] == t and np.array_equal(twin["case"], cen["case"]) and np.array_equal(twin["site_bits"], cen["site_bits"])


@pytest.mark.parametrize("dof", sorted(RECORD_BATCHES))
def test_record_batches_meet_the_floors(oracle_mod, dof):
    t = soft_batch(oracle_mod, dof, RECORD_BATCHES[dof])[4]["totals"]
    print(f"soft dof {dof} n {RECORD_BATCHES[dof]}: {t}")
    assert_floors(t, dof)


def test_dense_batch_meets_the_floors(oracle_mod):
    dof, n, ts = DENSE_BATCH
    for exact_pow in (False, True):
        t = soft_batch(oracle_mod, dof, n, ts, exact_pow=exact_pow)[4]["totals"]
        print(f"soft dof {dof} n {n} Ts {ts} exact_pow {exact_pow}: {t}")
        assert_floors(t, dof)


def test_matlab_semantics_batch_meets_the_floors(oracle_mod):
    t = soft_batch(oracle_mod, 7, 3000, semantics="matlab", sample=False)[4]["totals"]
    print(f"soft dof 7 n 3000 matlab: {t}")
    assert_floors(t, matlab=True)
    assert t["opt_false"] == 0 and t["not_planned"] == 0


@pytest.mark.parametrize("dof", RETIME_BATCHES)
def test_retimed_batches_meet_the_floors(oracle_mod, dof):
    """A retime scales ALL joints of a query; the census with per-query targets counts what retime_checker.retime counts."""
    import retime_checker as rc
    orc, lim, qs, rec, _ = soft_batch(oracle_mod, dof, RECORD_BATCHES[dof], sample=False)
    ts = rc.t_star(rec)
    for k in RETIME_FACTORS:
        cen = bc.census(orc, lim, qs, rec, t_required=k * ts)
        print(f"soft dof {dof} retimed to {k} T*: {cen['totals']['cases']}")
        bc.assert_reaches(cen["totals"], FLOOR, FLOOR)
        assert cen["totals"]["beyond_c2"] >= 0.5
        assert sum(cen["totals"]["cases"].values()) == dof * np.count_nonzero(rc.oracle_eligible(rec))
    _, retimed, cases = rc.retime(orc, rec, *qs, 1.5 * ts)
    cen = bc.census(orc, lim, qs, rec, t_required=1.5 * ts)
    assert np.array_equal(cases.sum(axis=0), [cen["totals"]["cases"][c] for c in bc.CASES])
    assert np.array_equal(retimed, (cen["case"] >= 0).all(axis=1))


NAMED = {"panda": dict(cases={0: 251, 1: 102563, 2: 17186, 3: 0, 4: 0, 5: 0, 6: 0, 7: 0, 8: 0}, reached={1, 16, 256}),
         "ref": dict(cases={0: 169, 1: 95639, 2: 23758, 3: 191, 4: 14, 5: 3, 6: 226, 7: 0, 8: 0}, reached={1, 4, 16, 32, 64, 128, 256})}


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_sets_reach_c1_and_c2_almost_only(oracle_mod, name):
    """What the named-set parity tests do NOT cover (seed 12345, 20 000 x 7 joints, the batch of test_switch_times_parity): no c7 / c8
    under either set, no c3-c8 and no quartic site under panda, never site 8, never a failed optSwitchTimes. Documented here so
    that nobody takes the named-set bit-identity figures for a statement about those branches; they are pinned under the soft set."""
    from longtermplanner_amd.synthetic import generate_queries, limit_set
    dof, lim = limit_set(name)
    orc = oracle_mod.Oracle(dof, 0.001, **lim)
    qs = generate_queries(20000, lim, seed=12345)
    rec = orc.plan_batch(*qs, sample=False)
    t = bc.census(orc, lim, qs, rec)["totals"]
    print(f"{name}: {t}")
    assert t["invalid"] == 0, "generate_queries' premise a_max^2 / (2 j_max) <= v_max holds for the named sets"
    assert t["cases"] == NAMED[name]["cases"]
    assert {s for s in bc.SITES if t["sites"][s] > 0} == NAMED[name]["reached"]
    assert t["opt_false"] == 0 and t["not_planned"] == 0
    assert t["beyond_c2"] < 0.01


def test_generated_queries_pass_check_inputs_only_under_the_generators_premise(oracle_mod):
    """generate_queries draws a_0 against the sign of v_0 from the whole [-a_max, 0]: v_0 + a_0 |a_0| / (2 j_max) stays within
    +-v_max only if a_max^2 / (2 j_max) <= v_max. True for panda, ref and the soft set; false for a slow-jerk set, where a large
    share of the generated queries fails checkInputs (as under the slow-jerk sets of dense_compare.fuzz_limits(wide=True))."""
    from longtermplanner_amd.synthetic import generate_queries, limit_set
    slow_jerk = dict(q_min=[-3.0] * 7, q_max=[3.0] * 7, v_max=[1.0] * 7, a_max=[2.0] * 7, j_max=[1.0] * 7)   # a^2 / (2 j) = 2 > v
    sets = [(limit_set("panda")[1], True), (limit_set("ref")[1], True), (bc.soft_limits(7), True), (bc.soft_limits(30), True),
            (slow_jerk, False)]
    for lim, premise in sets:
        v, a, j = (np.asarray(lim[k]) for k in ("v_max", "a_max", "j_max"))
        assert bool(np.all(a * a / (2.0 * j) <= v)) == premise
        dof = len(v)
        orc = oracle_mod.Oracle(dof, 0.001, **lim)
        qg, q0, v0, a0 = generate_queries(1000, lim, seed=SEED)
        invalid = sum(not orc.check_inputs(q0[i], v0[i], a0[i]) for i in range(1000))
        assert (invalid == 0) == premise, (lim, invalid)
