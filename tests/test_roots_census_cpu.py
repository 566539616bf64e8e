"""Which places of the real-Schur root finder the test polynomials reach, from the CPU oracle alone (tests/roots_census.py): the
exact census of every (type, degree), the floor of every class, what no search reached (UNREACHED) and what cannot occur
(UNREACHABLE, CANNOT), the oracle's selection against an independent one, and its roots against numpy.roots where the choice is
well conditioned.

The floors are conditions on the batches, not measurements: every class a degree can have in at least 20 polynomials of every
(type, degree), "not converged" in at least 2 per degree in double. A census that misses one gets more polynomials
(`python tests/roots_census.py --search` and the committed tests/golden/roots_census_rare.npz), never a lower floor."""
import numpy as np
import pytest

import roots_census as rc

F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
TYPES = [F64, F32]
IDS = ["f64", "f32"]

# (type, degree) -> (polynomials, those with status 0 / 1 / 2, the classes' totals in the order of oracle.SCHUR_FLAGS)
PINNED = {
    ('float64', 1): (10650, (10536, 0, 114), (9378, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 114, 0, 0, 1158, 0, 0, 0)),
    ('float64', 2): (10674, (10563, 0, 111), (1201, 3845, 3667, 1850, 0, 90, 4632, 2790, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 111, 0, 24, 0, 0, 0, 0)),
    ('float64', 3): (10751, (10637, 0, 114), (10637, 1762, 1796, 5075, 0, 26, 3291, 241, 0, 3106, 24, 24, 0, 0, 1071, 893, 0, 0, 0, 114, 0, 24, 0, 0, 0, 0)),
    ('float64', 4): (12266, (12117, 24, 125), (5442, 3345, 3346, 7394, 0, 135, 4993, 1065, 3159, 810, 116, 24, 1386, 0, 1245, 212, 10773, 0, 24, 125, 0, 24, 0, 135, 0, 24)),
    ('float64', 5): (11072, (10922, 24, 126), (10922, 2517, 2414, 6912, 0, 24, 4330, 172, 614, 3815, 96, 24, 1780, 0, 598, 449, 4424, 9561, 24, 126, 0, 24, 0, 29, 0, 24)),
    ('float64', 6): (10937, (10770, 24, 143), (7759, 3261, 3143, 7113, 0, 112, 5188, 354, 819, 3766, 118, 65, 2448, 0, 1422, 319, 6129, 9406, 24, 143, 0, 24, 0, 132, 0, 24)),
    ('float64', 7): (10858, (10678, 24, 156), (10685, 3048, 2940, 7061, 0, 26, 5120, 164, 233, 4380, 94, 28, 2849, 0, 460, 316, 4887, 9306, 24, 156, 0, 24, 0, 28, 0, 24)),
    ('float64', 8): (10839, (10653, 14, 172), (8699, 3419, 3299, 7110, 0, 90, 5336, 289, 201, 4564, 105, 31, 3175, 0, 1525, 251, 5579, 9265, 14, 172, 0, 24, 0, 31, 0, 24)),
    ('float32', 1): (10650, (10533, 0, 117), (9277, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 117, 0, 0, 1256, 0, 0, 0)),
    ('float32', 2): (10665, (10547, 0, 118), (1058, 3706, 3505, 2278, 0, 102, 4497, 2612, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 118, 0, 45, 0, 0, 0, 0)),
    ('float32', 3): (10701, (10579, 0, 122), (10579, 1841, 1776, 5109, 0, 39, 3273, 305, 0, 1541, 0, 0, 0, 0, 1233, 956, 0, 0, 0, 122, 0, 24, 0, 0, 0, 0)),
    ('float32', 4): (12255, (12123, 0, 132), (5537, 3418, 3400, 7392, 0, 139, 5123, 1157, 2439, 202, 30, 24, 1944, 24, 1712, 317, 10857, 0, 0, 132, 0, 24, 0, 50, 0, 6)),
    ('float32', 5): (11033, (10873, 25, 135), (10897, 2532, 2433, 7000, 0, 24, 4387, 268, 178, 2509, 30, 35, 2311, 35, 868, 482, 4348, 9589, 25, 135, 0, 24, 0, 47, 24, 1)),
    ('float32', 6): (10961, (10775, 32, 154), (7717, 3311, 3073, 7205, 0, 112, 5095, 468, 454, 2182, 39, 38, 3212, 51, 1930, 419, 6118, 9517, 32, 154, 0, 24, 0, 25, 24, 1)),
    ('float32', 7): (10847, (10650, 30, 167), (10676, 3120, 2873, 7167, 0, 31, 5080, 216, 61, 2412, 35, 33, 3625, 54, 1011, 417, 4816, 9346, 30, 167, 0, 24, 0, 28, 24, 0)),
    ('float32', 8): (10855, (10645, 26, 184), (8679, 3491, 3331, 7255, 0, 100, 5305, 386, 82, 2397, 41, 38, 4050, 42, 2134, 340, 5525, 9321, 26, 184, 0, 24, 0, 24, 24, 0)),
}


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


@pytest.mark.parametrize("degree", rc.DEGREES)
@pytest.mark.parametrize("dt", TYPES, ids=IDS)
def test_the_census_is_pinned(oracle_mod, dt, degree):
    """No figure here is a measurement of the device: if one moves, a generator, the committed bit patterns or the oracle moved."""
    cen = rc.census(degree, dt)
    got = (len(cen["coef"]), tuple(np.bincount(cen["status"], minlength=3).tolist()), tuple(cen["totals"][c] for c in oracle_mod.SCHUR_FLAGS))
    print(f"({dt.name!r}, {degree}): {got},")
    assert got == PINNED[(dt.name, degree)], (dt.name, degree, dict(cen["totals"]))


@pytest.mark.parametrize("degree", rc.DEGREES)
@pytest.mark.parametrize("dt", TYPES, ids=IDS)
def test_every_class_meets_its_floor(oracle_mod, dt, degree):
    cen = rc.census(degree, dt)
    assert set(cen["totals"]) == set(oracle_mod.SCHUR_FLAGS)
    short = {c: (n, rc.floor(c, degree, dt)) for c, n in cen["totals"].items() if n < rc.floor(c, degree, dt)}
    assert not short, f"{dt.name} degree {degree}: classes below their floor (have, floor): {short}"
    assert rc.FLOOR == 20 and rc.floor("not_converged", degree, F64) in (0, 2)
    assert 5000 <= len(cen["coef"]) <= 20000, "a GPU batch of a class is a few thousand solves at the most"
    assert int(cen["iterations"].max()) <= 40 * degree + 1, "the longest solve is the cap"


def test_unreached_and_unreachable_classes_are_empty(oracle_mod):
    """UNREACHABLE / CANNOT: the argument is in roots_census. UNREACHED: no polynomial in the searched budget (roots_census.SEARCHED);
    a class that turns up later fails here and gets its floor and its GPU case."""
    hits = {}
    for dt in TYPES:
        for d in rc.DEGREES:
            cen = rc.census(d, dt)
            for c, n in cen["totals"].items():
                if rc.is_empty(c, d, dt) and n:
                    hits[(c, d, dt.name)] = n
    assert not hits, hits
    assert all(k[0] in oracle_mod.SCHUR_FLAGS and k[1] in rc.DEGREES for k in rc.UNREACHED)
    assert set(rc.UNREACHABLE) <= set(oracle_mod.SCHUR_FLAGS)
    # the classes expected to stay out of reach, and the one that did not: float non-convergence exists from degree 5 on
    assert ("not_converged", 4, "float32") in rc.UNREACHED and all(("nonfinite_eigenvalue", d, t.name) in rc.UNREACHED for d in range(2, 9) for t in TYPES)
    assert all(rc.census(d, F32)["totals"]["not_converged"] >= rc.FLOOR for d in range(5, 9))
    assert "considered_zero" in rc.CANNOT[2] and rc.census(1, F64)["totals"]["considered_zero"] >= rc.FLOOR


def test_the_committed_bit_patterns(oracle_mod):
    """tests/golden/roots_census_rare.npz: found by the search whose budget it records; finite-or-not, they are this project's data.
    The non-converging double polynomials of degrees 4, 5 and 6 are among them."""
    z = np.load(rc.RARE)
    assert "chunks 1..40 of 20000 draws" in str(z["budget"]), str(z["budget"])
    for d in rc.PROBE_DEGREES:
        cen = rc.census(d, F64)
        held = cen["masks"]["not_converged"] & (cen["family"] == rc.FAMILIES.index("rare"))
        assert held.sum() >= 2, (d, int(held.sum()))
        assert (cen["status"][held] == 1).all() and (cen["iterations"][held] == 40 * d + 1).all()
        assert np.isnan(cen["re"][held]).all() and np.isnan(cen["im"][held]).all() and np.isinf(cen["smallest"][held]).all()


@pytest.mark.parametrize("degree", rc.DEGREES)
@pytest.mark.parametrize("dt", TYPES, ids=IDS)
def test_flags_status_and_steps_are_consistent(oracle_mod, dt, degree):
    cen = rc.census(degree, dt)
    m = cen["masks"]
    assert np.array_equal(cen["status"] == 1, m["not_converged"])
    assert np.array_equal(cen["status"] == 2, m["nonfinite_matrix"] | m["nonfinite_eigenvalue"])
    assert np.array_equal(cen["iu_steps"].sum(axis=1), cen["iterations"])
    assert (cen["iterations"][m["shift30_positive"] | m["shift30_not_positive"]] >= 31).all() and (cen["iterations"][m["shift10_window03"] | m["shift10_other"]] >= 11).all()
    assert not (m["shift30_zero"] & ~m["shift30_not_positive"]).any() and not (m["iter30_window03"] & ~(m["shift30_positive"] | m["shift30_not_positive"])).any()
    assert np.array_equal(m["converged_late"], (cen["iterations"] > 30 * degree) & (cen["status"] != 1))
    assert (cen["iterations"][m["not_converged"]] == 40 * degree + 1).all()
    nan = np.isnan(cen["re"]).all(axis=1) & np.isnan(cen["im"]).all(axis=1)
    assert nan[m["not_converged"] | m["nonfinite_matrix"]].all() and not np.isnan(cen["re"][cen["status"] == 0]).any()
    assert np.array_equal(np.isnan(cen["re"]), np.isnan(cen["im"]))


@pytest.mark.parametrize("degree", rc.DEGREES)
def test_smallest_root_is_the_selection_over_the_roots(oracle_mod, degree):
    """ltpo_smallest_root against roots.h:43-50 applied independently (numpy, over roots_f64's output) on every census polynomial,
    and the one-polynomial entry points against the batch entry on the picked ones."""
    cen = rc.census(degree, F64)
    want = rc.select_smallest(cen["re"], cen["im"])
    assert np.array_equal(_u(cen["smallest"]), _u(want))
    assert np.isinf(want).sum() >= rc.FLOOR and np.isfinite(want).sum() >= rc.FLOOR
    if degree >= 2:
        # a pair read out with z == 0 is (er, +0), (er, -0): both count as real, which is what the device's z == 0 && er > 1e-7 says
        z0 = np.flatnonzero(cen["masks"]["pair_z_zero"] & (cen["status"] == 0))
        assert z0.size >= rc.FLOOR and all((np.signbit(cen["im"][i]) & (cen["im"][i] == 0)).any() for i in z0)
    for i in rc.picked(degree, F64):
        p = cen["coef"][i]
        s = oracle_mod.smallest_root(p)
        assert np.float64(s).view(np.uint64) == cen["smallest"][i:i + 1].view(np.uint64)[0], (i, p)
        re, im, st = oracle_mod.roots_f64(p)
        assert st == cen["status"][i] and np.array_equal(np.isnan(re), np.isnan(cen["re"][i]))
        ok = ~np.isnan(re)
        assert np.array_equal(_u(re)[ok], _u(cen["re"][i])[ok]) and np.array_equal(_u(im)[ok], _u(cen["im"][i])[ok])
        assert tuple(c for c in oracle_mod.SCHUR_FLAGS if cen["masks"][c][i]) == oracle_mod.last_schur_flags()


@pytest.mark.parametrize("degree", rc.PROBE_DEGREES)
def test_selected_roots_agree_with_lapack_on_the_well_conditioned_families(oracle_mod, degree):
    """The rule of test_golden_vectors.test_selected_roots_agree_with_lapack (numpy.roots = LAPACK on the same companion matrix; a
    nearly-double real root that could be the answer is counted, not compared) on the families random, real_roots and planner."""
    cen = rc.census(degree, F64)
    rows = np.flatnonzero(np.isin(cen["family"], [rc.FAMILIES.index(f) for f in rc.WELL_CONDITIONED]))
    ambiguous = compared = 0
    worst = 0.0
    for i in rows:
        p, got = cen["coef"][i], cen["smallest"][i]
        if not np.all(np.isfinite(p)) or p[0] == 0.0:
            continue
        z = np.roots(p)
        scale = np.maximum(1.0, np.abs(z))
        real = np.abs(z.imag) <= 1e-9 * scale
        near = (np.abs(z.imag) <= 1e-4 * scale) & ~real
        cand = z.real[real & (z.real > 1e-7)]
        want = cand.min() if cand.size else np.inf
        if near.any() and (z.real[near] > 1e-7).any() and z.real[near & (z.real > 1e-7)].min() < want * (1 + 1e-6):
            ambiguous += 1
            continue
        compared += 1
        if np.isinf(want) or np.isinf(got):
            assert np.isinf(want) and np.isinf(got), (p, z, got)
        else:
            worst = max(worst, abs(got - want) / max(1.0, abs(want)))
    print(f"degree {degree}: {compared} compared, {ambiguous} ambiguous, worst {worst:.3e}")
    assert compared > 0.95 * len(rows), (compared, ambiguous)
    assert worst < 1e-8, worst


@pytest.mark.parametrize("degree", range(4, 9))
@pytest.mark.parametrize("dt", TYPES, ids=IDS)
def test_the_picked_polynomials_take_the_restated_shifts(oracle_mod, dt, degree):
    """tests/test_gpu_roots.py solves picked() under every wave layout. Replicated through a wave, a polynomial of degree >= 5 whose
    window is rows 0..3 at iteration 10 or 30 takes that shift in the sticky loop's restatement, not in the general loop's: the
    picked ones hold at least FLOOR of each (degree 4 has no second restatement; its figures are pinned all the same)."""
    cen = rc.census(degree, dt)
    idx = rc.picked(degree, dt)
    n10, n30 = int(cen["masks"]["shift10_window03"][idx].sum()), int(cen["masks"]["iter30_window03"][idx].sum())
    n30p = int((cen["masks"]["iter30_window03"] & cen["masks"]["shift30_positive"])[idx].sum())
    print(f"{dt.name} degree {degree}: {len(idx)} picked, {n10} take the iteration-10 shift on rows 0..3, {n30} reach iteration 30 there ({n30p} with s > 0)")
    assert 100 <= len(idx) <= 600
    assert n10 >= rc.FLOOR and n30 >= rc.FLOOR
    both = cen["masks"]["iter30_window03"] & cen["masks"]["shift30_positive"], cen["masks"]["iter30_window03"] & cen["masks"]["shift30_not_positive"]
    assert all(m.any() and m[idx].sum() >= min(rc.FLOOR, m.sum()) for m in both), "both outcomes of the restated test, all the census has up to the floor"
    for c in oracle_mod.SCHUR_FLAGS:
        assert cen["masks"][c][idx].sum() >= min(rc.FLOOR, cen["totals"][c]), c
