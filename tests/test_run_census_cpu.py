"""Which places of the trajectory sampler the test batches reach, from the CPU oracle alone (tests/run_census.py): the checker
pinned bit for bit against Oracle.get_trajectory, its sensitivity shown with three kinds of deliberately wrong rows, what the named
limit sets at their own sample times do NOT reach, and the floors every class has to meet in the batches of tests/test_gpu_runs.py.

The floors are conditions on the batches, not measurements: every class of run_census.CLASSES in at least 20 lanes of at least one
batch, both end-limit verdicts in at least 20 plans. A batch that misses one gets more queries or another sample time. A class no
input can produce is listed in UNREACHABLE with the argument, and asserted empty."""
import numpy as np
import pytest

import branch_census as bc
import run_census as rc

# class -> why no record can be in it. Switching times are cumulative sums of non-negative phase lengths: 0 <= t0 <= ... <= t6,
# so 0 <= s[k] for every k and ceil(t[k] / Ts) >= floor(t[k-1] / Ts) for odd k.
UNREACHABLE = {
    "cc781_not_landed": "s2 < s1 with s1 <= 0 needs s2 < 0",
    "fill1_negative": "s1 = ceil(t1 / Ts) >= floor(t0 / Ts) = s0 since t1 >= t0",
    "fill3_negative": "s3 = ceil(t3 / Ts) >= floor(t2 / Ts) = s2 since t3 >= t2",
    "fill5_negative": "s5 = ceil(t5 / Ts) >= floor(t4 / Ts) = s4 since t5 >= t4",
}


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def _lane(cen, orc, lim, rec, qs, p, j, mutant=None):
    return rc.expected_lane(cen, p, j, rec["t_scaled"][p, j], rec["dir"][p, j], rec["mod"][p, j], lim["j_max"][j], qs[1][p, j], qs[2][p, j],
                            qs[3][p, j], rec["v_drive"][p, j], last_joint=(j == orc.dof - 1), mutant=mutant)


CHECKED = [(b, "cpp") for b in rc.BATCHES] + [(b, "matlab") for b in rc.MATLAB_BATCHES]


@pytest.mark.parametrize("name,semantics", CHECKED)
def test_the_checker_has_the_oracles_bits(oracle_mod, name, semantics):
    """Up to 8 lanes of every class (a few hundred per batch): the rows built from the census' s, pos and stack in a plain loop
    over samples are Oracle.get_trajectory's, bit for bit, all four of them."""
    orc, lim, ts, qs, rec, cen = rc.batch(oracle_mod, name, semantics)
    lanes = rc.pick_lanes(cen, 8, np.random.default_rng(1))
    assert len(lanes) >= 100, len(lanes)
    rows = {}
    for p, j in lanes:
        if p not in rows:
            rows[p] = rc.oracle_rows(orc, rec, qs, p)
        L = rows[p][0]
        assert L == cen["traj_len"][p]
        *exp, most = _lane(cen, orc, lim, rec, qs, p, j)
        one = np.zeros(cen["live"].shape, dtype=bool)
        one[p, j] = True
        for x, (e, o) in zip("qvaj", zip(exp, rows[p][1:])):
            assert _bits(e, o[j]), f"{name} {semantics}: the checker's {x} row differs from the oracle's: {rc.describe(cen, one)}"
        assert most == cen["stack"][p, j], f"{name} {semantics}: {most} terms on one sample, the census says {cen['stack'][p, j]}: {rc.describe(cen, one)}"


MUTANTS = [("drop", k) for k in range(rc.N_TERMS)] + ["vs0", "o1"]


def test_wrong_rows_fail_the_checker(oracle_mod):
    """Sensitivity, on the CPU: a dropped correction term (each of the ten), constant-velocity samples that start one sample late and
    s2 == s1 taken as the else branch of cc:768 each give rows that are NOT the oracle's; and every reachable class has a lane in
    which some wrong row is caught, so no class is compared only where nothing can show. (A lane all of whose terms are zero cannot
    show a dropped term: the lanes whose seven times are all zero, which is where s1, s3 or s5 are zero, and the one-sample rows are
    exempt, and asserted to be exactly that.)"""
    caught = {m: 0 for m in MUTANTS}
    class_caught = {k: 0 for k in rc.CLASSES}
    for name in rc.BATCHES:
        orc, lim, ts, qs, rec, cen = rc.batch(oracle_mod, name)
        for p, j in rc.pick_lanes(cen, 3, np.random.default_rng(2)):
            o = rc.oracle_rows(orc, rec, qs, p)
            hit = False
            for m in MUTANTS:
                exp = _lane(cen, orc, lim, rec, qs, p, j, mutant=m)[:4]
                if not all(_bits(e, r[j]) for e, r in zip(exp, o[1:])):
                    caught[m] += 1
                    hit = True
            if hit:
                for k, mask in cen["masks"].items():
                    class_caught[k] += bool(mask[p, j])
            else:
                assert not np.any(o[4][j]) or o[0] == 1, (name, p, j, "no wrong row shows in a lane whose jerk row is not zero")
    print("lanes in which each wrong row was caught:", caught)
    print("lanes of each class in which a wrong row was caught:", class_caught)
    assert all(c >= 5 for c in caught.values()), caught
    exempt = set(UNREACHABLE) | {"all_zero_lane", "len1", "s1_zero", "s3_zero", "s5_zero"}
    missed = [k for k, c in class_caught.items() if c == 0 and k not in exempt]
    assert not missed, f"no wrong row was caught in any lane of {missed}"


def test_the_dyadic_grid_census_is_pinned(oracle_mod):
    """9409 one-joint rest-to-rest plans, every input a multiple of 1/16, Ts 0.25. No generator and no random draw is involved: if a
    figure moves, the oracle's planner or the census moved."""
    orc, lim, ts, qs, rec, cen = rc.batch(oracle_mod, "dyadic_grid")
    t = cen["totals"]
    assert (t["exact_any"], t["last_dropped"], t["len1"], t["exact_all7"]) == (6642, 743, 97, 646), t
    assert (t["w_le0"], t["w1"], t["w2"], t["w3"], t["w_ge4"]) == (491, 7278, 584, 456, 600), t
    assert (t["cc781_landed"], t["cc798_landed"], t["cc798_not_landed"], t["stack3"]) == (2670, 2670, 97, 2670), t
    assert int((rec["status"] == 2).sum()) == 840 and int((rec["status"] == 1).sum()) == 8569
    # the last correction index s6 + 1 equals traj_len exactly where t6 is a multiple of Ts: the reference writes out of range there
    t6 = rec["t_scaled"][:, 0, 6] / ts
    assert np.array_equal(cen["masks"]["last_dropped"][:, 0], np.floor(t6) == np.ceil(t6))


def test_every_class_meets_its_floor_in_some_batch(oracle_mod):
    best = {k: (0, None) for k in rc.CLASSES}
    verdicts = {1: 0, 2: 0}
    for name in rc.BATCHES:
        orc, lim, ts, qs, rec, cen = rc.batch(oracle_mod, name)
        n = len(rec["status"])
        assert 300 <= n <= 10000, "a few hundred to a few thousand plans per GPU batch"
        assert rec["traj_len"].max() <= 160, "rows of at most 160 samples: every GPU test stays at a few seconds"
        print(f"{name}: n {n}, Ts {ts}, traj_len {int(rec['traj_len'][rec['status'] != 0].min())}-{int(rec['traj_len'].max())}, planned "
              f"{int((rec['status'] == 1).sum())}, end-limit {int((rec['status'] == 2).sum())}, not planned {int((rec['status'] == 0).sum())}, "
              f"most runs {int((cen['runs'] * cen['live']).max())}: {cen['totals']}")
        for k, c in cen["totals"].items():
            if c > best[k][0]:
                best[k] = (c, name)
        for v in verdicts:
            verdicts[v] = max(verdicts[v], int((rec["status"] == v).sum()))
        for k, why in UNREACHABLE.items():
            assert cen["totals"][k] == 0, f"{name}: {k} was declared unreachable ({why}) and has {cen['totals'][k]} lanes"
        # s1, s3 or s5 == 0 means t1, t3 or t5 == 0: seen only where all seven times are zero (a joint that does not move)
        zero = (rec["t_scaled"] == 0.0).all(axis=2)
        assert not ((cen["masks"]["s1_zero"] | cen["masks"]["s3_zero"] | cen["masks"]["s5_zero"]) & ~zero).any(), name
    short = {k: v for k, v in best.items() if v[0] < rc.FLOOR and k not in UNREACHABLE}
    assert not short, f"no batch reaches {short}"
    assert min(verdicts.values()) >= rc.FLOOR, verdicts
    # every MATLAB batch: one-sample rows, exact multiples and the collided snap in bulk (LTPlanner.m returns zeros where the C++ fails)
    for name in rc.MATLAB_BATCHES:
        t = rc.batch(oracle_mod, name, "matlab")[5]["totals"]
        print(f"{name} matlab: {t}")
        assert t["w1"] >= rc.FLOOR and t["stack3"] >= rc.FLOOR and t["fill2_empty"] >= rc.FLOOR, (name, t)
    for name in ("dyadic_grid", "dyadic_two"):
        t = rc.batch(oracle_mod, name, "matlab")[5]["totals"]
        assert min(t["len1"], t["exact_any"], t["exact_all7"], t["w_le0"], t["s6_zero"]) >= rc.FLOOR, (name, t)


NAMED = (("panda", 0.001), ("ref", 0.004), ("soft", 0.01))


@pytest.mark.parametrize("which,ts", NAMED)
def test_named_sets_at_their_own_sample_times_reach_the_uncollided_structure_almost_only(oracle_mod, which, ts):
    """What the dense-row parity figures of the named sets do NOT cover (seed 5, 2000 plans x 7 joints): at their own sample times
    the phases are hundreds of samples long, so the else branches of cc:781 / cc:798 are taken by at most a few lanes under panda and
    ref, the narrow constant-velocity snaps (s3 - s2 = 2 or 3) by at most 8, no guard s1 > 0, s4 > 0 or s6 == 0 decides anything, no
    switching time is a multiple of the sample time and no trajectory has fewer than 298 samples. Documented here so that nobody
    takes those figures for a statement about collided switch indices; they are pinned on the batches of run_census.BATCHES."""
    from longtermplanner_amd.synthetic import generate_queries, limit_set
    lim = bc.soft_limits(7) if which == "soft" else limit_set(which)[1]
    orc = oracle_mod.Oracle(7, ts, **lim)
    qs = generate_queries(2000, lim, seed=rc.SEED)
    rec = orc.plan_batch(*qs, sample=False)
    cen = rc.census(rec["t_scaled"], np.where(rec["status"] != 0, rec["traj_len"], 0), ts)
    t = cen["totals"]
    print(f"{which} Ts {ts}: traj_len {int(rec['traj_len'][rec['status'] != 0].min())}-{int(rec['traj_len'].max())}: {t}")
    if which != "soft":
        assert t["cc781_landed"] <= 5 and t["cc798_landed"] + t["cc798_not_landed"] <= 5, t
    assert t["w2"] <= 6 and t["w3"] <= 8, t
    assert t["s1_zero"] == t["s4_zero"] == t["s6_zero"] == t["all_zero_lane"] == 0, t
    assert t["exact_any"] == t["last_dropped"] == t["len_le32"] == 0, t
    assert rec["traj_len"][rec["status"] != 0].min() >= 298
    assert t["stack_ge5"] <= 24 and t["w_le0"] == 0, t
