"""Stop states of the census batches (tests/stop_census.py), the part that needs no GPU: which classes of optBraking the states of
every batch reach and which run structure their stop plans have, from the CPU oracle alone. Every total is pinned — the draw is
seeded, so a figure moves only if the oracle, a generator or a census moved —, the floors the GPU comparisons of
tests/test_gpu_stop_runs.py rely on are asserted (conditions, not measurements: a batch that misses one gets more samples per plan),
what a batch does not reach is listed with the reason and asserted empty, a joint at rest is followed through both forms of
optBraking, and the checker is held against the independent one-joint path of tests/test_stop_cpu.py at coarse sample times."""
import numpy as np
import pytest

import knots_checker as kc
import run_census as rc
import stop_census as sn
import stop_checker as sc

# batch -> lanes per class, in the order of stop_checker.CLASSES:
#            dir_from_va, dir_from_v, dir_from_a, at_rest, phase2_present, phase2_small_negative, sqrt_branch
STOP_TOTALS = {
    "panda_0.1": (4036, 5718, 36, 710, 9715, 785, 0),
    "ref_1": (4629, 3363, 350, 2158, 7007, 3493, 0),
    "ref_0.05": (12829, 13827, 578, 766, 17707, 2993, 7300),
    "soft_0.25": (2838, 5280, 462, 1920, 667, 2144, 7689),
    "soft_1": (3194, 3493, 296, 3517, 1686, 7392, 1422),
    "dyadic_grid": (780, 472, 86, 162, 715, 158, 627),
    "dyadic_two": (1027, 1309, 171, 493, 466, 612, 1922),
    "dyadic_moving": (618, 574, 170, 138, 695, 215, 590),
    "dyadic_moving_1": (810, 237, 39, 414, 601, 899, 0),
    "soft_dense": (4082, 4395, 660, 1363, 591, 114, 9795),
}
# batch -> lanes per class of the run census of the stop records, in the order of run_census.CLASSES
RUN_TOTALS = {
    "panda_0.1": (9687, 0, 0, 6599, 10500, 712, 0, 6599, 0, 6599, 0, 0, 10500, 0, 0, 0, 712, 813, 0, 0, 0, 0, 0, 9687, 0, 10500, 0, 10500, 0, 0, 0, 10500, 0, 0, 0, 0, 749, 3969, 3640, 9002, 0),
    "ref_1": (7867, 0, 0, 8036, 10500, 2212, 0, 8036, 0, 8036, 0, 0, 10500, 0, 0, 0, 2212, 2633, 0, 0, 0, 0, 0, 7867, 0, 10500, 0, 10500, 0, 0, 0, 10500, 0, 0, 0, 0, 5537, 1463, 182, 10220, 0),
    "ref_0.05": (570, 0, 112, 1224, 4185, 781, 766, 1224, 766, 1224, 514, 766, 27234, 0, 0, 0, 1796, 4060, 766, 766, 766, 766, 0, 570, 0, 27234, 0, 27234, 0, 514, 0, 27234, 2373, 0, 252, 252, 21, 119, 392, 28000, 0),
    "soft_0.25": (1808, 0, 179, 3473, 5918, 1952, 1763, 3473, 1763, 3473, 1763, 2684, 7816, 0, 0, 0, 2446, 5522, 2684, 2684, 2684, 2684, 702, 1808, 0, 7816, 0, 7816, 114, 2570, 0, 7816, 978, 729, 313, 0, 329, 91, 2366, 10500, 0),
    "soft_1": (4036, 0, 2214, 5943, 7180, 3654, 304, 5943, 304, 5943, 304, 1568, 8932, 0, 0, 0, 3400, 5096, 1568, 1568, 1568, 1568, 1231, 4036, 0, 8932, 0, 8932, 6, 327, 4, 10163, 2131, 1252, 609, 0, 2058, 3360, 1953, 10458, 0),
    "dyadic_grid": (56, 0, 49, 172, 513, 171, 162, 172, 162, 172, 0, 191, 1309, 0, 0, 0, 301, 518, 191, 191, 191, 191, 6, 56, 0, 1309, 0, 1309, 19, 6, 1, 1312, 508, 18, 191, 162, 10, 174, 228, 1500, 0),
    "dyadic_two": (117, 0, 66, 550, 1028, 506, 493, 550, 493, 550, 307, 523, 2477, 0, 0, 0, 1007, 1246, 523, 523, 523, 523, 2, 117, 0, 2477, 0, 2477, 19, 311, 1, 2483, 757, 23, 211, 186, 16, 126, 204, 3000, 0),
    "dyadic_moving": (85, 0, 27, 199, 603, 151, 138, 199, 138, 199, 0, 242, 1258, 0, 0, 0, 293, 478, 242, 242, 242, 242, 7, 85, 0, 1258, 0, 1258, 90, 11, 0, 1261, 295, 104, 242, 138, 63, 180, 246, 1500, 0),
    "dyadic_moving_1": (603, 0, 28, 801, 1311, 444, 0, 801, 0, 801, 0, 19, 1481, 0, 0, 0, 454, 897, 19, 19, 19, 19, 0, 603, 0, 1481, 0, 1481, 0, 4, 15, 1481, 215, 0, 19, 0, 816, 495, 59, 1500, 0),
    "soft_dense": (18, 0, 6, 1375, 1536, 1363, 1363, 1375, 1363, 1375, 1363, 1381, 9119, 0, 0, 0, 1411, 1453, 1381, 1381, 1381, 1381, 0, 18, 0, 9119, 0, 9119, 17, 1364, 0, 9119, 33, 2, 17, 0, 14, 28, 14, 434, 0),
}
# (batch, class) -> why no state of the batch is in it. With x = a / a_max in [-1, 1] after the direction rule, phase 2 is
# r1 = -v / a_max - (a_max / j_max) (1 - x^2 / 2), and the rule leaves -v >= -a^2 / (2 j_max), so r1 >= -a_max / j_max: the
# square-root branch (r1 < -Ts) needs a joint with a_max / j_max > Ts.
ABSENT = {
    ("panda_0.1", "sqrt_branch"): "cannot occur: a_max / j_max is 0.002 on every panda joint, Ts 0.1",
    ("ref_1", "sqrt_branch"): "cannot occur: a_max / j_max is 2 / 15 on every joint of the reference's limits, Ts 1",
    ("dyadic_moving_1", "sqrt_branch"): "cannot occur: a_max / j_max is 2 / 4 on the one joint, Ts 1",
}
COARSE = tuple(rc.COARSE)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("name", sn.BATCHES)
def test_totals_are_pinned(oracle_mod, name):
    """The classes of optBraking over the states of the batch and the run census of their stop records (check = "braking")."""
    S = sn.knot_states(oracle_mod, name)
    n, dof = S["q0"].shape
    assert n == len(S["plan"]) == len(S["sample"]) and n <= sn.MAX_OF.get(name, sn.MAX_STATES) and S["a_raw"].shape == (n, dof)
    assert np.all(np.abs(S["a0"]) <= S["orc"].a_max[None, :]) and _bits(S["a0"], np.clip(S["a_raw"], -S["orc"].a_max, S["orc"].a_max))
    # the states are the oracle's rows at (plan, sample)
    rows = sn.source(oracle_mod, name)[5]
    for i in range(0, n, 97):
        L, q, v, a, _ = rows[S["plan"][i]]
        k = S["sample"][i]
        assert 0 <= k < L and _bits(S["q0"][i], q[:, k]) and _bits(S["v0"][i], v[:, k]) and _bits(S["a_raw"][i], a[:, k])
    t = sc.census_totals(sn.census(oracle_mod, name))
    print(name, n, "states:", t)
    assert tuple(t[k] for k in sc.CLASSES) == STOP_TOTALS[name], (name, t)
    assert sum(t[k] for k in sc.DIR_CLASSES) == n * dof == sum(t[k] for k in sc.PHASE_CLASSES)
    E = sn.expected(oracle_mod, name)
    assert not E["status"].any() and np.all(E["traj_len"] > 0), "every clamped state is admitted and planned"
    r = sn.stop_runs(oracle_mod, name)["totals"]
    print(name, "stop records:", {k: v for k, v in r.items() if v})
    assert tuple(r[k] for k in rc.CLASSES) == RUN_TOTALS[name], (name, r)


@pytest.mark.parametrize("name", sn.BATCHES)
def test_floors(oracle_mod, name):
    S = sn.knot_states(oracle_mod, name)
    lanes = S["q0"].size
    t = sc.census_totals(sn.census(oracle_mod, name))
    for k in sc.CLASSES:
        if (name, k) in ABSENT:
            assert t[k] == 0, f"{name}: {k} was declared absent ({ABSENT[(name, k)]}) and has {t[k]} lanes"
        else:
            assert t[k] >= sn.FLOOR, f"{name}: {k} in {t[k]} lanes: enlarge stop_census.PER_PLAN or list it in ABSENT with the reason"
    assert set(sn.present(oracle_mod, name)) == {k for k in sc.CLASSES if (name, k) not in ABSENT}
    if name == sn.SOFT_DENSE:
        assert t["sqrt_branch"] >= 0.8 * lanes, t
    if name in ("ref_1", "soft_1"):
        assert t["phase2_small_negative"] >= 0.25 * lanes, t
    E = sn.expected(oracle_mod, name, rows=True)
    r = sn.stop_runs(oracle_mod, name)["totals"]
    if name in COARSE:
        short = int(np.count_nonzero((E["traj_len"] >= 1) & (E["traj_len"] <= 4)))
        over = int(np.count_nonzero(np.any(np.abs(S["a_raw"]) > S["orc"].a_max[None, :], axis=1)))
        print(name, "stop plans of at most 4 samples:", short, "states with |a| > a_max before the clamp:", over, "of", len(S["q0"]))
        assert short >= 100 and over >= 100, (name, short, over)
    if name in ("soft_0.25", "soft_1"):
        assert min(r["cc798_landed"], r["exact_any"], r["fill2_negative"]) >= sn.FLOOR, r
    if name == sn.SOFT_DENSE:
        end = int(np.count_nonzero(E["status_end"] & sc.END_LIMIT))
        print(name, "stop plans that end outside [q_min, q_max]:", end)
        assert end >= 100
    ties = sn.tied(E)
    assert np.all(E["slowest"][ties] == np.argmax(E["t_opt"][ties][:, :, 6], axis=1)), "the first of the tied joints is the slowest"
    assert (ties.sum() >= sn.FLOOR) == (name in sn.TIED), (name, int(ties.sum()))
    # switch indices 3..6 of a stop plan are one number: almost every lane that moves at all stacks five terms or more
    moving = E["t_scaled"][:, :, 6] > 0.0
    assert r["stack_ge5"] >= 0.8 * moving.sum(), (name, r["stack_ge5"], int(moving.sum()))
    assert E["traj_len"].max() <= 500, "rows of a few hundred samples at the most: every GPU test stays at a few seconds"


def test_absent_classes_are_named():
    assert all(b in sn.BATCHES and k in sc.CLASSES and ("cannot occur" in why or "not reached" in why) for (b, k), why in ABSENT.items())
    assert {b for b in sn.BATCHES if STOP_TOTALS[b][sc.CLASSES.index("sqrt_branch")] == 0} == {b for b, _ in ABSENT}


def test_at_rest_under_a_coarse_sample_time(oracle_mod):
    """A joint at rest (v == 0 and a == 0) stops where it is: q_stop has the bits of q_0. Its standstill time follows the reference:
    +0.0 through the square-root branch, and a_max / j_max where a_max / j_max <= Ts keeps phase 2 at -a_max / j_max (cc:679-689).
    Both outcomes occur, the second in bulk on ref_1 and soft_1."""
    seen = {"zero": 0, "kept": 0}
    for name in sn.BATCHES:
        S = sn.knot_states(oracle_mod, name)
        cen = sn.census(oracle_mod, name)
        E = sn.expected(oracle_mod, name)
        rest = cen["at_rest"]
        assert rest.any(), name
        assert _bits(E["q_stop"][rest], S["q0"][rest]), f"{name}: a joint at rest does not stop at q_0: {sn.describe(cen, rest & (E['q_stop'] != S['q0']))}"
        t6 = E["t_opt"][:, :, 6]
        tj = np.broadcast_to((S["orc"].a_max / S["orc"].j_max)[None, :], t6.shape)
        root, kept = rest & cen["sqrt_branch"], rest & ~cen["sqrt_branch"]
        assert np.array_equal(root, rest & (tj > S["ts"])), name
        assert not t6[root].view(np.uint64).any(), f"{name}: at rest through the square-root branch: t_stop is not +0.0"
        assert _bits(t6[kept], tj[kept]) and np.all(t6[kept] > 0.0), f"{name}: at rest with phase 2 kept: t_stop is not a_max / j_max"
        assert not cen["phase2_present"][rest].any()
        print(name, "at rest:", int(root.sum()), "with t_stop +0.0,", int(kept.sum()), "with t_stop a_max / j_max")
        seen["zero"] += int(root.sum())
        if name in ("ref_1", "soft_1"):
            assert kept.sum() >= 100 * sn.FLOOR // 20, (name, int(kept.sum()))
            seen["kept"] += int(kept.sum())
    assert seen["zero"] >= sn.FLOOR and seen["kept"] >= sn.FLOOR, seen


@pytest.mark.parametrize("name", ["soft_1", "ref_0.05", sn.SOFT_DENSE])
def test_checker_equals_one_joint_plans_towards_the_standstill(oracle_mod, name):
    """The independent path of tests/test_stop_cpu.py at the batch's own sample time: a ONE-joint oracle planner with the joint's
    limits, planning towards fl(q_0 + q_stop), gives the checker's t_opt, t_scaled, dir, mod and v_drive bit for bit, on the first
    100 states of the batch and every joint whose one-joint checkInputs admits it (at a coarse sample time the sampled states of
    other joints overshoot v_max: of 1500 states of soft_1 checkInputs admits 41 as a whole); the planner refuses exactly the other
    joints. The identity holds at every sample time tried, the negative phase 2 and the non-zero standstill time of a joint at rest
    included: nothing about the early exit of optSwitchTimes (cc:100-107) depends on Ts beyond optBraking itself."""
    S = sn.knot_states(oracle_mod, name)
    E = sn.expected(oracle_mod, name)
    cen = sn.census(oracle_mod, name)
    lim = S["lim"]
    ones = [oracle_mod.Oracle(1, S["ts"], *[[lim[k][j]] for k in ("q_min", "q_max", "v_max", "a_max", "j_max")]) for j in range(S["dof"])]
    compared = np.zeros(S["q0"].shape, dtype=bool)
    for p in range(100):
        for j, one in enumerate(ones):
            q0, v0, a0 = S["q0"][p, j], S["v0"][p, j], S["a0"][p, j]
            tr = one.plan_batch([E["q_stop"][p, j]], [q0], [v0], [a0])
            lane = np.zeros(S["q0"].shape, dtype=bool)
            lane[p, j] = True
            if not one.check_inputs([q0], [v0], [a0]):
                assert tr["status"][0] == 0
                continue
            compared[p, j] = True
            what = f"{name}: {sn.describe(cen, lane)}; {sn.describe_source(oracle_mod, name, lane.any(axis=1))}"
            assert tr["status"][0] != 0, what
            assert _bits(tr["t_opt"][0, 0], E["t_opt"][p, j]) and _bits(tr["t_scaled"][0, 0], E["t_scaled"][p, j]), what
            assert _bits(tr["dir"][0, 0], E["dir"][p, j]) and int(tr["mod"][0, 0]) == 0 == int(E["mod"][p, j]), what
            assert _bits(tr["v_drive"][0, 0], E["v_drive"][p, j]), what
            assert tr["traj_len"][0] <= E["traj_len"][p] and (j != E["slowest"][p] or tr["traj_len"][0] == E["traj_len"][p]), what
    print(name, "lanes compared:", int(compared.sum()), {k: int((cen[k] & compared).sum()) for k in sc.CLASSES})
    assert compared.sum() >= 300
    for k in sn.present(oracle_mod, name):
        assert (cen[k] & compared).any(), f"{name}: no compared lane of class {k}"


def test_what_the_grid_readers_must_find(oracle_mod):
    """The conditions under which a comparison of sampleKnots or stopKnots on the run-census batches says something about the lanes
    with kMaxSegments runs, about more passes than one and about rows of 1 to 4 samples (run_census.assert_reader_shapes), on the
    oracle's records: the GPU tests assert the same on the device's."""
    held = {}
    for name in rc.BATCHES:
        orc, lim, ts, qs, rec, cen = rc.batch(oracle_mod, name)
        lens = np.where(rec["status"] != 0, rec["traj_len"], 0)
        held[name] = rc.assert_reader_shapes(name, cen, lens, rec["t_scaled"], ts, kc.SMALL_GRIDS["unit"])
        print(name, held[name])
    assert "runs_max" in held[rc.RUNS_MAX_BATCH] and all("multi_pass" in held[b] for b in rc.MULTI_PASS)
    assert {k for h in held.values() for k in h} >= {"runs_max", "multi_pass", "len1", "len2", "len3", "len4"}
    assert np.array_equal(kc.SMALL_GRIDS["unit"], np.arange(25)) and np.any(np.diff(kc.SMALL_GRIDS["duplicates"]) == 0)
    assert all(len(g) == 25 and g.dtype == np.int32 and np.all(np.diff(g) >= 0) for g in kc.SMALL_GRIDS.values())


def test_the_wide_batch_ties_inside_a_joint_slot(oracle_mod):
    """stop_census.wide_states: 24 joints in 8 joint slots at Ts 1. In every state the largest standstill time is held by a joint
    below 8 and by its copies 8 and 16 joints on, and the checker's `slowest` is the first of them (cc:31-39); every class of
    soft_1 is present and the lanes of a copy have the bits of their source lane."""
    W = sn.wide_states(oracle_mod)
    S = sn.knot_states(oracle_mod, "soft_1")
    n = sn.WIDE_N
    assert W["q0"].shape == (n, sn.WIDE_DOF) and sn.WIDE_DOF > sn.WIDE_SLOTS and W["ts"] == 1.0
    E = sc.expected_stop(W["orc"], W["q0"], W["v0"], W["a0"], "braking", rows=False)
    src = sn.expected(oracle_mod, "soft_1")
    assert _bits(E["t_opt"], src["t_opt"][:n][:, W["source"]]) and _bits(E["q_stop"], src["q_stop"][:n][:, W["source"]])
    t6 = E["t_opt"][:, :, 6]
    top = t6 == t6.max(axis=1, keepdims=True)
    assert not E["status"].any() and np.all(E["slowest"] < sn.WIDE_SLOTS) and np.all(E["slowest"] == np.argmax(top, axis=1))
    s = E["slowest"]
    assert np.all(top[np.arange(n), s + sn.WIDE_SLOTS] & top[np.arange(n), s + 2 * sn.WIDE_SLOTS]), "the copies in the same slot tie"
    assert np.all(t6.max(axis=1) > 0.0)
    t = sc.census_totals(sc.census(W["orc"], W["v0"], W["a0"]))
    print("wide:", t)
    assert all(t[k] >= sn.FLOOR for k in sn.present(oracle_mod, "soft_1")) and S["dof"] == 7
