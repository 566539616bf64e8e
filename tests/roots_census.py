"""Which places of the real-Schur root finder a batch of polynomials reaches (test infrastructure, not a test module, like
run_census.py and branch_census.py).

The device solver (csrc/ltp_roots.hpp: real_schur_companion, francis_step_window4, smallest_positive_real_root,
companion_eigenvalues) restates oracle/companion_roots.inc operation for operation. The oracle records, per solve, a word of
branch flags (oracle.SCHUR_FLAGS, set where the branches are taken); a CLASS here is one of those flags, and a polynomial is in
every class whose branch its solve took. census() returns, per polynomial, the oracle's roots, status, flags and Francis steps
per window end iu.

The polynomials come from named FAMILIES, each a deterministic numpy generator of (degree, dtype), and from
tests/golden/roots_census_rare.npz: explicit bit patterns of the classes that a generator of a few thousand draws does not reach
(not converged, the iteration-30 test with s <= 0, ...), found on the CPU by `python tests/roots_census.py --search` with the
budget printed in that file's `budget` entry. Held as bits, those classes do not vanish with a change of numpy's streams.

tests/test_roots_census_cpu.py pins the census and its floors; tests/test_gpu_roots.py compares the device with the oracle
class by class, and under five wave layouts, on the batches made by pick() here."""
import os

import numpy as np

SEED = 20261019
FLOOR = 20
DEGREES = tuple(range(1, 9))
PROBE_DEGREES = (4, 5, 6)
PER_FAMILY = 1500                                  # draws of a random family per (degree, dtype)
RARE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roots_census_rare.npz")
POLY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planner_polynomials.npz")


_STEPS = ("shift10_window03", "shift10_other", "shift30_positive", "shift30_not_positive", "start_below_top", "hh3_small_tail",
          "hh2_small_tail", "beta_zero", "step_window03", "step_other_n5", "not_converged", "iter30_window03", "shift30_zero", "converged_late")
_PAIRS = ("deflate_two_real_p_nonneg", "deflate_two_real_p_neg", "deflate_two_complex", "givens_p0", "givens_p_larger", "givens_q_larger",
          "pair_z_zero")
# class -> why no polynomial of any degree or type can be in it
UNREACHABLE = {
    "givens_q0": "makeGivens gets q = T[iu][iu-1] of a window with il == iu - 1: the search went past that entry because it is larger "
                 "than max(eps (|T[iu-1][iu-1]| + |T[iu][iu]|), consider_zero) >= the smallest normal number, so it is not zero",
}
# degree -> class -> why that degree cannot have it (degrees 5..8 share one entry)
CANNOT = {
    1: {**{c: "a 1 x 1 matrix has one root and takes no step" for c in _STEPS + _PAIRS},
        "nonfinite_eigenvalue": "T is +-1 and scale is |p1 / p0|, finite"},
    2: {**{c: "a window of two rows is split off without a Francis step" for c in _STEPS}},
    3: {"shift10_window03": "no row 3", "iter30_window03": "no row 3", "step_window03": "no row 3", "step_other_n5": "degree below 5",
        "start_below_top": "the only window with a step is rows 0..2, whose step starts at im = iu - 2 = il",
        "hh3_small_tail": "its one 3-vector reflector is the first of a step, with v2 = T[2][1] inside the window: |v2| > consider_zero >= "
                          "eps^2 norm >= eps^2, and eps^4 is above the smallest normal number in both types"},
    4: {"step_other_n5": "degree below 5"},
}
for _d in range(2, 9):
    CANNOT.setdefault(_d, {})["considered_zero"] = "the sub-diagonal ones make scale >= 1: only a x + b with |b / a| below the smallest normal number gets there"
CANNOT[1]["givens_q0"] = UNREACHABLE["givens_q0"]
# (class, degree, type) -> the search that did not reach it. Budget of every entry: chunk 0 (PER_FAMILY draws) plus chunks 1..40 of
# 20 000 draws of each of the seven random families (`--search 40 20000`: 800 000 polynomials per family, degree and type).
SEARCHED = "40 chunks of 20 000 draws of each of random, real_roots, double_roots, triple_root, sparse, scaled, subnormal"
UNREACHED = {}
for _d in range(2, 9):
    for _t in ("float64", "float32"):
        UNREACHED[("nonfinite_eigenvalue", _d, _t)] = SEARCHED        # a finite companion matrix whose eigenvalue times scale overflows
for _d in range(4, 9):
    UNREACHED[("hh3_small_tail", _d, "float64")] = SEARCHED            # reached in float from degree 4 on (family scaled), never in double
UNREACHED[("not_converged", 3, "float64")] = SEARCHED
UNREACHED[("not_converged", 3, "float32")] = SEARCHED
UNREACHED[("not_converged", 4, "float32")] = SEARCHED
UNREACHED[("shift30_positive", 3, "float32")] = SEARCHED
UNREACHED[("shift30_not_positive", 3, "float32")] = SEARCHED
for _d in range(3, 9):
    UNREACHED[("shift30_zero", _d, "float64")] = SEARCHED            # s == 0 exactly at iteration 30: float only, from degree 5 on
UNREACHED[("shift30_zero", 3, "float32")] = SEARCHED
UNREACHED[("shift30_zero", 4, "float32")] = SEARCHED
for _d, _t in ((3, "float64"), (3, "float32"), (7, "float32"), (8, "float32")):
    UNREACHED[("converged_late", _d, _t)] = SEARCHED
# (class, degree, type) -> how many the same search found where that is fewer than FLOOR: all of them are held, and that is the floor
LOW = {("converged_late", 4, "float32"): 6, ("converged_late", 5, "float32"): 1, ("converged_late", 6, "float32"): 1}


def is_empty(cls, degree, dtype):
    """True where the census of (degree, dtype) is expected to hold no polynomial of the class: it cannot, or no search reached it."""
    return cls in UNREACHABLE or cls in CANNOT.get(degree, {}) or (cls, degree, np.dtype(dtype).name) in UNREACHED


def floor(cls, degree, dtype):
    """How many polynomials of a class the census of (degree, dtype) has to hold at least."""
    if is_empty(cls, degree, dtype):
        return 0
    if (cls, degree, np.dtype(dtype).name) in LOW:
        return LOW[(cls, degree, np.dtype(dtype).name)]
    return 2 if cls == "not_converged" and np.dtype(dtype) == np.float64 else FLOOR


def classes():
    import oracle
    return oracle.SCHUR_FLAGS


def poly_from_roots(r):
    """Monic coefficients [m][d + 1], highest first, of the polynomials with roots r [m][d]: the plain recurrence c <- c x - r c."""
    r = np.asarray(r, dtype=np.float64)
    m, d = r.shape
    c = np.zeros((m, d + 1))
    c[:, 0] = 1.0
    for k in range(d):
        c[:, 1:k + 2] = c[:, 1:k + 2] - r[:, k:k + 1] * c[:, 0:k + 1]
    return c


def _rng(family, degree, chunk=0):
    """chunk 0 is the committed batch; the search (--search) draws chunks 1, 2, ... of the same generators."""
    return np.random.default_rng([SEED, sum(map(ord, family)), degree, chunk])


# ---- the families: name -> f(degree) -> float64 coefficients [m][degree + 1]; a float batch is the same array rounded to float ----
def fam_random(d, m=PER_FAMILY, chunk=0):
    """The generator of test_device_root_finder_matches_oracle: normal coefficients times 10^[-2, 2]."""
    rng = _rng("random", d, chunk)
    return rng.normal(size=(m, d + 1)) * 10.0 ** rng.integers(-2, 3, size=(m, d + 1))


def fam_real_roots(d, m=PER_FAMILY, chunk=0):
    return poly_from_roots(_rng("real_roots", d, chunk).uniform(-3, 3, size=(m, d)))


def fam_double_roots(d, m=PER_FAMILY, chunk=0):
    """Two double real roots (one from degree 2 on, two from degree 4 on): where the iteration is slowest."""
    r = _rng("double_roots", d, chunk).uniform(-3, 3, size=(m, d))
    if d >= 2:
        r[:, 1] = r[:, 0]
    if d >= 4:
        r[:, 3] = r[:, 2]
    return poly_from_roots(r)


def fam_triple_root(d, m=PER_FAMILY, chunk=0):
    r = _rng("triple_root", d, chunk).uniform(-3, 3, size=(m, d))
    r[:, 1:min(d, 3)] = r[:, 0:1]
    return poly_from_roots(r)


def fam_sparse(d, m=PER_FAMILY, chunk=0):
    """x^d + eps x^k + c: almost a binomial, all roots on nearly one circle (the iteration-10 shift)."""
    rng = _rng("sparse", d, chunk)
    c = np.zeros((m, d + 1))
    c[:, 0] = 1.0
    c[:, d] = rng.normal(size=m) * 10.0 ** rng.integers(-2, 3, size=m)
    if d >= 2:
        k = rng.integers(1, d, size=m)
        c[np.arange(m), k] = rng.normal(size=m) * 10.0 ** rng.integers(-12, -2, size=m)
    return c


def fam_named(d, m=None):
    """a (x^d - 1), a (x^d + 1), a x^d, a (x - 1)^d and a (x^d - x) for 24 leading coefficients a = +-(1 + j / 4) 2^(3 j - 18)."""
    j = np.arange(12)
    a = (1.0 + j / 4.0) * 2.0 ** (3 * j - 18)
    a = np.concatenate([a, -a])
    base = []
    for last in (-1.0, 1.0, 0.0):
        p = np.zeros(d + 1); p[0] = 1.0; p[d] = last
        base.append(p)
    base.append(poly_from_roots(np.ones((1, d)))[0])
    p = np.zeros(d + 1); p[0] = 1.0; p[d - 1] += -1.0
    base.append(p)
    return np.concatenate([a[:, None] * b[None, :] for b in base])


def _scaled(d, dtype, m=PER_FAMILY, chunk=0):
    """Mantissas in [1, 2) times 2^e: in half of the rows the exponent of p[i] / p[0] is spread over the whole range of the type and
    past both ends (quotients that overflow, underflow, or are subnormal); in the other half ONE quotient sits within 2^4 of the
    overflow edge and the others are moderate, which is where an eigenvalue times scale could overflow after a finite matrix."""
    rng = _rng("scaled", d, chunk)
    emax = 127 if np.dtype(dtype) == np.float32 else 1023
    c = rng.uniform(1.0, 2.0, size=(m, d + 1)) * np.where(rng.random((m, d + 1)) < 0.5, -1.0, 1.0)
    e0 = rng.integers(-emax // 2, emax // 2, size=(m, 1))
    wide = rng.integers(-emax - 30, emax + 3, size=(m, d + 1))
    edge = rng.integers(-20, 20, size=(m, d + 1))
    edge[np.arange(m), rng.integers(1, d + 1, size=m)] = rng.integers(emax - 4, emax + 3, size=m)
    q = np.where(rng.random((m, 1)) < 0.5, wide, edge)
    q[:, 0] = 0
    return np.ldexp(c, np.clip(e0 + q, -emax - 25, emax))


def _subnormal(d, dtype, m=PER_FAMILY, chunk=0):
    """Normal coefficients whose last 1..d are subnormal numbers of the batch's type, or zero (three in ten)."""
    rng = _rng("subnormal", d, chunk)
    tiny = float(np.finfo(dtype).tiny)
    c = rng.normal(size=(m, d + 1))
    t = rng.integers(0, 1 << 20, size=(m, d + 1)) * (tiny * 2.0 ** -20) * np.where(rng.random((m, d + 1)) < 0.5, -1.0, 1.0)
    t[rng.random((m, d + 1)) < 0.3] = 0.0
    trailing = np.arange(d + 1)[None, :] >= d + 1 - rng.integers(1, d + 1, size=(m, 1))
    return np.where(trailing, t, c)


def fam_nonfinite(d, m=None):
    """A zero, NaN or inf leading or inner coefficient: every position of every kind, on three base polynomials."""
    rng = _rng("nonfinite", d)
    out = []
    for _ in range(3):
        p = rng.normal(size=d + 1)
        for k in range(d + 1):
            for v in (0.0, -0.0, np.nan, np.inf, -np.inf):
                q = p.copy(); q[k] = v
                out.append(q)
    return np.array(out)


def fam_planner(d, m=None):
    """The committed polynomials the planner solves (tests/golden/planner_polynomials.npz): degrees 4, 5 and 6."""
    rows = np.load(POLY)["rows"]
    return np.ascontiguousarray(rows[rows[:, 0] == d][:, 1:d + 2])


FAMILIES = ("random", "real_roots", "double_roots", "triple_root", "sparse", "named", "scaled", "subnormal", "nonfinite", "planner", "rare")
WELL_CONDITIONED = ("random", "real_roots", "planner")          # compared with numpy.roots in tests/test_roots_census_cpu.py


RANDOM_FAMILIES = ("random", "real_roots", "double_roots", "triple_root", "sparse", "scaled", "subnormal")


def family(name, degree, dtype=np.float64, m=PER_FAMILY, chunk=0):
    """float64 or float32 coefficients [m][degree + 1] of a named family (m may be 0)."""
    dt = np.dtype(dtype)
    if name == "scaled":
        c = _scaled(degree, dt, m, chunk)
    elif name == "subnormal":
        c = _subnormal(degree, dt, m, chunk)
    elif name in RANDOM_FAMILIES:
        c = globals()["fam_" + name](degree, m, chunk)
    elif name == "planner":
        c = fam_planner(degree) if degree in PROBE_DEGREES else np.zeros((0, degree + 1))
    elif name == "rare":
        return rare(degree, dt)
    else:
        c = globals()["fam_" + name](degree)
    with np.errstate(over="ignore", under="ignore"):
        return np.ascontiguousarray(c.astype(dt))


def rare(degree, dtype, cache={}):
    """The committed bit patterns of (degree, dtype): coefficients [m][degree + 1]."""
    if "z" not in cache:
        cache["z"] = dict(np.load(RARE)) if os.path.exists(RARE) else {}
    dt = np.dtype(dtype)
    key = f"d{degree}_{dt.name}"
    if key not in cache["z"]:
        return np.zeros((0, degree + 1), dtype=dt)
    bits = cache["z"][key]
    return np.ascontiguousarray(bits.view(dt).reshape(-1, degree + 1))


def census(degree, dtype=np.float64, cache={}):
    """The census of every family's polynomials of (degree, dtype), computed once per process and left unchanged: dict of
    coef [n][degree + 1], family [n] (index into FAMILIES), re, im [n][degree], status, flags, iterations [n], iu_steps [n][9],
    smallest [n] (float64 only), masks {class: bool [n]}, totals {class: count}."""
    import oracle
    dt = np.dtype(dtype)
    key = (degree, dt.name)
    if key not in cache:
        parts = [family(f, degree, dt) for f in FAMILIES]
        coef = np.ascontiguousarray(np.concatenate(parts))
        fam = np.concatenate([np.full(len(p), i) for i, p in enumerate(parts)])
        c = oracle.roots_census(coef, dt)
        c["coef"], c["family"] = coef, fam
        c["masks"] = {name: (c["flags"] >> b & 1).astype(bool) for b, name in enumerate(oracle.SCHUR_FLAGS)}
        c["totals"] = {k: int(v.sum()) for k, v in c["masks"].items()}
        cache[key] = c
    return cache[key]


def pick(cls, degree, dtype=np.float64, k=FLOOR):
    """The indices (into census(degree, dtype)) of up to k polynomials of a class, dealt round-robin over the families that have any."""
    c = census(degree, dtype)
    m = np.logical_and.reduce([c["masks"][x] for x in cls.split("&")])          # "a&b": in both classes
    per = [np.flatnonzero(m & (c["family"] == f)) for f in range(len(FAMILIES))]
    out, i = [], 0
    while len(out) < k and any(i < len(p) for p in per):
        out.extend(int(p[i]) for p in per if i < len(p))
        i += 1
    return np.array(sorted(out[:k]), dtype=np.int64)


def picked(degree, dtype=np.float64, k=FLOOR):
    """The union of pick() over all classes and over both outcomes of the iteration-30 test on rows 0..3 (the sticky loop restates
    it): the polynomials of the wave-composition tests."""
    idx = set()
    for cls in classes() + ("iter30_window03&shift30_positive", "iter30_window03&shift30_not_positive"):
        idx.update(pick(cls, degree, dtype, k).tolist())
    return np.array(sorted(idx), dtype=np.int64)


def describe(cen, idx):
    """The classes and families of the polynomials idx, for assertion messages."""
    idx = np.atleast_1d(np.asarray(idx))
    if idx.size == 0:
        return "no polynomials"
    hit = {k: int(v[idx].sum()) for k, v in cen["masks"].items()}
    fams = sorted({FAMILIES[f] for f in cen["family"][idx]})
    i = int(idx[0])
    return (f"{idx.size} polynomials of {fams}; classes {{" + ", ".join(f"{k}: {c}" for k, c in hit.items() if c) + f"}}; first: index {i}, "
            f"coefficients {[x.hex() for x in cen['coef'][i].astype(np.float64)]}, status {int(cen['status'][i])}, {int(cen['iterations'][i])} steps")


def select_smallest(re, im):
    """roots.h:43-50 over the rows of re, im [n][d], independent of the oracle's loop: min{re : im == 0 and re > 1e-7}, else +inf
    (NaN entries never qualify)."""
    with np.errstate(invalid="ignore"):
        ok = (im == 0) & (re > 1e-7)
    return np.where(ok, re, np.inf).min(axis=1)


# ---- the search behind tests/golden/roots_census_rare.npz: `python tests/roots_census.py --search [chunks] [draws per chunk]` ----
def search(chunks=15, m=20000, keep=FLOOR + 4, log=print):
    """For every (degree, dtype) and every class that chunk 0 of the families leaves below `keep` polynomials: chunks 1..chunks of
    m draws of each random family, keeping the first polynomials of each such class until it has `keep`. Returns the arrays of the
    .npz: d<degree>_<dtype> = the kept coefficients as unsigned integers of the type's width, budget = what was searched."""
    import oracle
    import sys
    sys.modules.setdefault("roots_census", sys.modules[__name__])
    out = {}
    for dt in (np.dtype(np.float64), np.dtype(np.float32)):
        for d in DEGREES:
            parts = [family(f, d, dt) for f in FAMILIES if f != "rare"]
            base = oracle.roots_census(np.concatenate(parts), dt)["flags"]
            have = {b: int((base >> b & 1).sum()) for b in range(len(oracle.SCHUR_FLAGS))}
            kept = []
            for chunk in range(1, chunks + 1):
                need = [b for b, c in have.items() if c < keep]
                if not need:
                    break
                for f in RANDOM_FAMILIES:
                    coef = family(f, d, dt, m, chunk)
                    flags = oracle.roots_census(coef, dt)["flags"]
                    take = np.zeros(len(coef), dtype=bool)
                    for b in need:
                        short = keep - have[b] - int((flags[take] >> b & 1).sum())
                        take[np.flatnonzero((flags >> b & 1).astype(bool) & ~take)[:max(0, short)]] = True
                    if take.any():
                        kept.append(coef[take])
                        for b in have:
                            have[b] += int((flags[take] >> b & 1).sum())
            if kept:
                out[f"d{d}_{dt.name}"] = np.concatenate(kept).view(np.uint64 if dt == np.float64 else np.uint32).reshape(-1)
            log(f"{dt.name} degree {d}: kept {sum(len(k) for k in kept)}; " + ", ".join(f"{oracle.SCHUR_FLAGS[b]} {c}" for b, c in have.items() if c < keep))
    out["budget"] = np.array(f"chunks 1..{chunks} of {m} draws of each of {', '.join(RANDOM_FAMILIES)}, per degree 1..8 and type")
    return out


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if len(sys.argv) > 1 and sys.argv[1] == "--search":
        z = search(*[int(x) for x in sys.argv[2:4]])
        np.savez_compressed(RARE, **z)
        print("wrote", RARE, os.path.getsize(RARE), "bytes")
