"""GPU: the per-lane Francis QR of csrc/ltp_roots.hpp against the CPU oracle, bit for bit, class by class of tests/roots_census.py
and under every wave layout.

The device code restates oracle/companion_roots.inc operation for operation and both sides build without contraction, so the
assertion is bits: re and im of every eigenvalue, and the selected root of the probe. NaN is compared as a pattern (where), not
as a payload. For degree >= 5 the step a lane takes depends on the other lanes of its wave (francis_step_window4 and the sticky
loop run on a ballot), so every picked polynomial is also solved under layouts that put it in uniform, mixed, partial and
long-running company: its bits may not depend on the company.

The polynomials, their classes and the floors are pinned on the CPU in tests/test_roots_census_cpu.py."""
import numpy as np
import pytest

import oracle
import roots_census as rc

pytestmark = pytest.mark.gpu

CLASSES = oracle.SCHUR_FLAGS
F64, F32 = np.dtype(np.float64), np.dtype(np.float32)


@pytest.fixture(scope="module")
def ltp():
    import longtermplanner_amd as amd
    D, lim = amd.limit_set("panda")
    return amd.LongTermPlanner(D, 0.001, device=0, **lim)


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _differs(got, ref):
    """bool [...]: not the same NaN pattern, or not the same bits where neither is NaN."""
    gn, rn = np.isnan(got), np.isnan(ref)
    return (gn != rn) | (~gn & ~rn & (_u(got) != _u(ref)))


def _solve_all(ltp, coef, dt):
    z = ltp.roots(coef, dtype=dt)
    return np.ascontiguousarray(z.real.astype(dt)), np.ascontiguousarray(z.imag.astype(dt))


def _probe(ltp, degree, coef):
    c7 = np.zeros((len(coef), 7))
    c7[:, :degree + 1] = coef
    return ltp.debugRootsProbe(degree, c7)


def _check_roots(ltp, cen, idx, dt, what, coef=None, where=None):
    """Solve coef (default: the census' polynomials idx) and compare the rows `where` (default: all) with the oracle's of idx."""
    coef = cen["coef"][idx] if coef is None else coef
    re, im = _solve_all(ltp, coef, dt)
    if where is not None:
        re, im = re[where], im[where]
    bad = (_differs(re, cen["re"][idx]) | _differs(im, cen["im"][idx])).any(axis=1)
    assert not bad.any(), f"{what}: eigenvalues differ from the oracle's bits: {rc.describe(cen, idx[bad])}; device {re[bad][0]} {im[bad][0]}, oracle {cen['re'][idx[bad][0]]} {cen['im'][idx[bad][0]]}"


def _check_probe(ltp, cen, idx, degree, what, coef=None, where=None):
    coef = cen["coef"][idx] if coef is None else coef
    got = _probe(ltp, degree, coef)
    if where is not None:
        got = got[where]
    bad = _differs(got, cen["smallest"][idx])
    assert not bad.any(), f"{what}: the selected root differs from the oracle's bits: {rc.describe(cen, idx[bad])}; device {got[bad][0]!r}, oracle {cen['smallest'][idx[bad][0]]!r}"


# ---- by class ----
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("degree", rc.PROBE_DEGREES)
def test_probe_has_the_oracles_bits_by_class(ltp, degree, cls):
    cen = rc.census(degree, F64)
    idx = np.flatnonzero(cen["masks"][cls])[:2000]
    assert (idx.size == 0) == rc.is_empty(cls, degree, F64), (cls, degree, idx.size)
    if idx.size:
        _check_probe(ltp, cen, idx, degree, f"class {cls}, degree {degree}")


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("degree", rc.DEGREES)
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_roots_have_the_oracles_bits_by_class(ltp, dt, degree, cls):
    cen = rc.census(degree, dt)
    idx = np.flatnonzero(cen["masks"][cls])[:2000]
    assert (idx.size == 0) == rc.is_empty(cls, degree, dt), (cls, degree, idx.size)
    if idx.size:
        _check_roots(ltp, cen, idx, dt, f"class {cls}, degree {degree}, {dt.name}")


# ---- wave composition ----
def _layouts(cen, idx, degree, dt):
    """name -> (coef [n][degree + 1], rows of coef to compare, the census index of the polynomial in each such row). The kernels run
    64-lane blocks with lane = index % 64, so a layout is a placement in the array."""
    P = len(idx)
    mine = cen["coef"][idx]
    xd = np.zeros(degree + 1, dtype=dt)
    xd[0] = 1                                                                   # x^d: one step (none below degree 3), then out
    slow = np.flatnonzero(cen["masks"]["not_converged"])
    slow = cen["coef"][slow[0] if slow.size else int(np.argmax(cen["iterations"]))]    # stays for 40 N steps (or the longest there is)
    rng = np.random.default_rng(degree)
    out = {"replicated": (np.repeat(mine, 64, axis=0), np.arange(P * 64), np.repeat(idx, 64))}
    for name, lane in (("lane0", 0), ("lane63", 63)):
        c = np.tile(xd, (P * 64, 1))
        c[np.arange(P) * 64 + lane] = mine
        out[name] = (c, np.arange(P) * 64 + lane, idx)
    perm = rng.permutation(P)
    out["shuffled"] = (mine[perm], np.argsort(perm), idx)
    # lane 0 of every wave holds the slow polynomial, the other 63 lanes the picked ones in another order
    perm = rng.permutation(P)
    pad = (-P) % 63
    body = np.concatenate([mine[perm], np.tile(xd, (pad, 1))]).reshape(-1, 63, degree + 1)
    c = np.concatenate([np.tile(slow, (len(body), 1, 1)), body], axis=1).reshape(-1, degree + 1)
    pos = np.arange(P) // 63 * 64 + 1 + np.arange(P) % 63
    out["slow_neighbour"] = (c, pos[np.argsort(perm)], idx)
    c = np.repeat(mine, 64, axis=0)
    c[np.arange(P) * 64 + 63] = slow
    rows = np.flatnonzero(np.arange(P * 64) % 64 != 63)
    out["replicated_slow_neighbour"] = (c, rows, np.repeat(idx, 64)[rows])
    return out, xd


@pytest.mark.parametrize("degree", rc.DEGREES)
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_roots_do_not_depend_on_the_wave(ltp, dt, degree):
    cen = rc.census(degree, dt)
    idx = rc.picked(degree, dt)
    layouts, xd = _layouts(cen, idx, degree, dt)
    for name, (coef, rows, who) in layouts.items():
        _check_roots(ltp, cen, who, dt, f"layout {name}, degree {degree}, {dt.name}", coef, rows)
    # alone in the last, partial wave: n = 64 k + 1. One launch per polynomial, so one polynomial per class
    first = np.array(sorted({int(rc.pick(c, degree, dt, 1)[0]) for c in CLASSES if cen["totals"][c]}))
    for k, i in enumerate(first):
        coef = np.concatenate([np.tile(xd, (64 * (1 + k % 2), 1)), cen["coef"][i:i + 1]])
        _check_roots(ltp, cen, np.array([i]), dt, f"layout partial, degree {degree}, {dt.name}", coef, np.array([len(coef) - 1]))


@pytest.mark.parametrize("degree", rc.PROBE_DEGREES)
def test_probe_does_not_depend_on_the_wave(ltp, degree):
    cen = rc.census(degree, F64)
    idx = rc.picked(degree, F64)
    layouts, xd = _layouts(cen, idx, degree, F64)
    for name, (coef, rows, who) in layouts.items():
        _check_probe(ltp, cen, who, degree, f"layout {name}, degree {degree}", coef, rows)
    first = np.array(sorted({int(rc.pick(c, degree, F64, 1)[0]) for c in CLASSES if cen["totals"][c]}))
    for k, i in enumerate(first):
        coef = np.concatenate([np.tile(xd, (64 * (1 + k % 2), 1)), cen["coef"][i:i + 1]])
        _check_probe(ltp, cen, np.array([i]), degree, f"layout partial, degree {degree}", coef, np.array([len(coef) - 1]))


# ---- the two read-outs of one Schur form agree ----
@pytest.mark.parametrize("degree", rc.PROBE_DEGREES)
def test_probe_is_the_selection_over_roots(ltp, degree):
    """On the device alone: smallest_positive_real_root (folded read-out and selection) against roots.h:43-50 applied to
    companion_eigenvalues' output, on every polynomial of the census: the z == 0 pairs and the non-finite classes included."""
    cen = rc.census(degree, F64)
    re, im = _solve_all(ltp, cen["coef"], F64)
    want = rc.select_smallest(re, im)
    got = _probe(ltp, degree, cen["coef"])
    bad = np.flatnonzero(_differs(got, want))
    assert bad.size == 0, f"degree {degree}: the probe's root is not the selection over roots(): {rc.describe(cen, bad)}; probe {got[bad[0]]!r}, selection {want[bad[0]]!r}"
