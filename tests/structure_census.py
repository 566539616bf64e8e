"""Structured queries and what they reach (test infrastructure, not a test module, like branch_census.py and run_census.py).

generate_queries draws the four inputs of every joint independently: no joint of a moving query starts at rest, none already sits
at its goal, no two joints ask for the same motion. A controller sends the opposite: the arm stands still, one or two joints are
commanded, dual or symmetric axes get identical or mirrored commands. The generator here starts from generate_queries and overwrites
every (query, joint) lane according to a kind:

  random        untouched
  rest          q_goal = q_0, v_0 = a_0 = 0
  near          v_0 = a_0 = 0, 0 < |q_goal - q_0| < 4e-3: inside the eps of cc:96-107, dir stays 0
  rest_to_rest  v_0 = a_0 = 0, q_goal left random
  stop_only     q_goal = q_0 + q_stop of Oracle.opt_braking: the early exit of cc:100-107 with dir left from braking (site 256)
  twin          the four inputs of the query's source joint s(q)
  mirror        the four inputs of the source joint, negated
                (twin and mirror only where the joints share limits and the q range is symmetric: ref and ref30, not panda)

and every query has a shape: all_rest (every joint rests: under ref t_required == 0 and traj_len == 1; under panda at Ts 0.004
a_max / j_max < Ts, optBraking keeps a phase 2 of -0.002 s and a lane that stands still has an optimum of 0.002 s), one_mover (one
random or rest_to_rest joint, the others rest), all_twins (every joint a twin of the source, sets with twins only) or mixed (kinds
drawn per joint; on a set with twins half of the mixed queries are pair queries: ONE twin or mirror of a moving source, the pair
drawn through pair_groups() so that every tie class has its share). The shapes come in runs of RUN queries, so tied queries stand
side by side in a block of 64 and a cut can begin inside such a run.

Every draw is the counter-based unit_random of longtermplanner_amd/synthetic.py under seeds of its own: the batches are the same on
every host and numpy.

Tie classes: a query is tied when the maximal t_opt[..][6] is shared (bit-equal) by at least two joints and T > 0; j1 < j2 are its
first two tied joints. k_reduce_scale combines per-slot-row maxima over the block's JB joint-slot rows (JB = min(dof, 4) under the
libm pow rule, min(dof, 8) under the exact rule), so per JB: same_row (j1 % JB == j2 % JB), later_row_first (j2 % JB < j1 % JB, the
only class that needs the `bj < slowest` clause) and earlier_row_first; across_rounds (j2 >= 8: the second tied joint is met in a
later round of the 8-slot kernel) and three_or_more.

classes() gives (name, lane mask [n][dof]) like branch_census.classes: per-lane kinds crossed with the accepted timeScaling case,
the query shapes and the tie classes (a query class holds every lane of its queries). The floors are in
tests/test_structure_census_cpu.py; tests/test_gpu_structure.py compares the device class by class."""
import numpy as np

import branch_census as bc

from longtermplanner_amd.synthetic import generate_queries, limit_set, unit_random

KINDS = ("random", "rest", "near", "rest_to_rest", "stop_only", "twin", "mirror")
RANDOM, REST, NEAR, REST_TO_REST, STOP_ONLY, TWIN, MIRROR = range(7)
SHAPES = ("all_rest", "one_mover", "all_twins", "mixed")
ALL_REST, ONE_MOVER, ALL_TWINS, MIXED = range(4)
RUN = 13                                    # queries per run of one shape: no divisor of the 64-query block
CYCLE = (MIXED, ALL_TWINS, MIXED, ONE_MOVER, MIXED, ALL_REST, MIXED, ALL_TWINS)       # shares: mixed 1/2, all_twins 1/4, the others 1/8
EPS = 4e-3                                  # cc:96
SEED = 7
TS = bc.TS
FLOOR = bc.FLOOR
# name -> (limit set, dof, queries): the smallest batches that fill every class (tests/test_structure_census_cpu.py)
BATCHES = {"panda7": ("panda", 7, 2000), "ref7": ("ref", 7, 2000), "ref9": ("ref", 9, 1500), "ref30": ("ref30", 30, 1600),
           "ref2": ("ref", 2, 4000)}
ROWS_N = 600                                # plans whose rows are taken, from the start of a batch
CASES = (-1,) + bc.CASES                    # -1: not scaled (the joint that keeps its optimum)

# mixed queries come in three flavours, drawn per query. P(kind) of a lane that is not the source, in the order of KINDS: a pair query
# (half of them on a set with twins: ONE other joint, the partner, is the source's twin or mirror, and most of the others stand
# still, so that the pair is the slowest: a dual axis), a calm one and a busy one (a quarter each)
_P_PAIR = (0.02, 0.72, 0.14, 0.02, 0.10, 0.0, 0.0)
_P_CALM = (0.06, 0.40, 0.10, 0.06, 0.06, 0.20, 0.12)
_P_BUSY = (0.22, 0.14, 0.08, 0.14, 0.14, 0.16, 0.12)


def _row_relation(a, b, JB):
    return "same" if a % JB == b % JB else ("later" if b % JB < a % JB else "earlier")


def pair_groups(dof):
    """The joint pairs (a < b) grouped by what a tie of exactly these two is to k_reduce_scale: the relation of their slot rows under
    each JB and whether b is met in a later round. A pair query draws its group first, then the pair: every tie class gets a share
    that does not shrink with the number of pairs."""
    groups = {}
    for a in range(dof):
        for b in range(a + 1, dof):
            key = tuple(_row_relation(a, b, JB) for JB in jbs(dof)) + (b >= 8,)
            groups.setdefault(key, []).append((a, b))
    return [groups[k] for k in sorted(groups)]


def has_twins(set_name):
    return set_name in ("ref", "ref30")


def jbs(dof):
    """The joint-slot rows of k_reduce_scale's block: libm rule, exact rule."""
    return (min(dof, 4), min(dof, 8))


def generate(orc, set_name, dof, n, seed=SEED):
    """(limits, (q_goal, q_0, v_0, a_0) row-major [n][dof], kind [n][dof], shape [n], source [n]) of a structured batch; `orc` is an
    Oracle of these limits (opt_braking gives q_stop)."""
    d, lim = limit_set(set_name, dof)
    assert d == dof
    qg, q0, v0, a0 = (np.array(x) for x in generate_queries(n, lim, seed=seed))
    q = np.arange(n, dtype=np.uint64)[:, None]
    j = np.arange(dof, dtype=np.uint64)[None, :]
    u_kind, u_near, u_sign = (unit_random(seed + 1, q, j, f) for f in range(3))
    u_src, u_mover, u_mkind, u_calm = (unit_random(seed + 2, q[:, 0], 0, f) for f in range(4))
    twins = has_twins(set_name)
    shape = np.array([CYCLE[(i // RUN) % len(CYCLE)] for i in range(n)], dtype=np.int8)
    if not twins:
        shape[shape == ALL_TWINS] = MIXED
    source = np.minimum((u_src * dof).astype(np.int64), dof - 1)
    mover = np.minimum((u_mover * dof).astype(np.int64), dof - 1)
    rows = np.arange(n)
    # kinds of a mixed query
    pair = (u_calm < 0.5) & twins & (dof >= 2)
    p = np.where(pair[:, None, None], np.asarray(_P_PAIR), np.where((u_calm < 0.75)[:, None, None], np.asarray(_P_CALM), np.asarray(_P_BUSY)))
    if not twins:                           # the twins' share goes to the kinds that exist
        p = p.copy()
        p[..., :TWIN] *= (1.0 / p[..., :TWIN].sum(axis=-1, keepdims=True))
        p[..., TWIN:] = 0.0
    kind = (u_kind[:, :, None] >= np.cumsum(p, axis=-1)).sum(axis=-1).clip(max=MIRROR).astype(np.int8)
    if twins:
        groups = pair_groups(dof)
        partner = np.zeros(n, dtype=np.int64)
        for i in np.nonzero(pair)[0]:       # the pair of a pair query: its group, then the pair; the source is either of the two
            g = groups[min(int(u_src[i] * len(groups)), len(groups) - 1)]
            a, b = g[min(int(u_mover[i] * len(g)), len(g) - 1)]
            source[i], partner[i] = (a, b) if u_sign[i, 0] < 0.5 else (b, a)
        src_kind = np.array([RANDOM, REST_TO_REST, STOP_ONLY], dtype=np.int8)[np.minimum((u_kind[rows, source] * 3).astype(np.int64), 2)]
        kind[rows, source] = src_kind       # the source of a query moves; without twins there is no source
        kind[rows[pair], partner[pair]] = np.where(u_mkind[pair] < 0.6, TWIN, MIRROR)
    m = shape == ALL_REST
    kind[m] = REST
    m = shape == ONE_MOVER
    kind[m] = REST
    kind[rows[m], mover[m]] = np.where(u_mkind[m] < 0.5, RANDOM, REST_TO_REST)
    m = shape == ALL_TWINS
    kind[m] = TWIN
    kind[rows[m], source[m]] = np.where(u_mkind[m] < 0.5, RANDOM, REST_TO_REST)
    # the lanes that do not copy
    still = np.isin(kind, (REST, NEAR, REST_TO_REST))
    v0[still] = 0.0
    a0[still] = 0.0
    qg = np.where(kind == REST, q0, qg)
    d_near = np.where(u_sign < 0.5, -1.0, 1.0) * (1e-4 + u_near * (EPS - 2e-4))
    qg = np.where(kind == NEAR, q0 + d_near, qg)
    for i, k in np.argwhere(kind == STOP_ONLY):
        qg[i, k] = q0[i, k] + orc.opt_braking(int(k), v0[i, k], a0[i, k])[0]
    # and the lanes that do
    for f in (qg, q0, v0, a0):
        s = f[rows, source][:, None]
        f[...] = np.where(kind == TWIN, s, np.where(kind == MIRROR, -s, f))
    near = kind == NEAR
    assert np.all((np.abs(qg - q0)[near] > 0.0) & (np.abs(qg - q0)[near] < EPS))
    return lim, [np.ascontiguousarray(x) for x in (qg, q0, v0, a0)], kind, shape, source


def ties(rec):
    """Of Oracle.plan_batch records: tied [n] (the maximal t_opt[..][6] is shared bit for bit by at least two joints), count [n] of
    the joints that share it, j1, j2 [n] (the first two of them; j2 = -1 without a tie) and T [n]."""
    t6 = np.asarray(rec["t_opt"])[:, :, 6]
    T = t6.max(axis=1)
    at = t6.view(np.uint64) == np.ascontiguousarray(T).view(np.uint64)[:, None]
    count = at.sum(axis=1)
    j1 = at.argmax(axis=1)
    rest = at.copy()
    rest[np.arange(len(T)), j1] = False
    j2 = np.where(count >= 2, rest.argmax(axis=1), -1)
    return dict(tied=count >= 2, count=count, j1=j1, j2=j2, T=T)


def tie_classes(tie, dof):
    """{name: query mask [n]} of the tie classes (queries tied with T > 0), for both JB of `dof`."""
    t = tie["tied"] & (tie["T"] > 0.0)
    j1, j2 = tie["j1"], tie["j2"]
    out = {}
    for JB in sorted(set(jbs(dof))):
        out[f"same_row_jb{JB}"] = t & (j1 % JB == j2 % JB)
        out[f"later_row_first_jb{JB}"] = t & (j2 % JB < j1 % JB)
        out[f"earlier_row_first_jb{JB}"] = t & (j1 % JB < j2 % JB)
    out["across_rounds"] = t & (j2 >= 8)
    out["three_or_more"] = t & (tie["count"] >= 3)
    return out


def impossible(set_name, dof):
    """The shapes and tie classes that cannot exist in a batch of this set and joint count, by name."""
    out = set()
    names = set(tie_classes(ties(dict(t_opt=np.zeros((1, dof, 7)))), dof))
    if not has_twins(set_name):
        # panda: every joint has limits of its own, so no twin, no mirror, no all_twins query. Two joints share a positive t_opt bit
        # for bit only where both stand still (rest or near: a_max / j_max = 0.002 < Ts on every joint, so optBraking keeps a phase 2
        # of -0.002 s and t_opt[6] is 0.002, not 0): then no joint moves, all seven tie and the first two are joints 0 and 1
        out |= {"all_twins"} | {k for k in names if k.startswith(("same_row", "later_row_first"))}
    for JB in set(jbs(dof)):
        if dof <= JB:                       # j % JB == j: the first tied joint always sits in the earlier row
            out |= {f"same_row_jb{JB}", f"later_row_first_jb{JB}"}
    if dof <= 8:
        out.add("across_rounds")
    if dof == 2:
        out.add("three_or_more")
    return out


def classes(S):
    """(name, lane mask [n][dof]) of every class of the batch S (see batch()): kind x case, shapes, tie classes."""
    kind, case = S["kind"], S["cen"]["case"]
    n, dof = kind.shape
    out = [(f"{KINDS[k]}.c{c}", (kind == k) & (case == c)) for k in range(len(KINDS)) for c in CASES]
    out += [(SHAPES[s], np.repeat((S["shape"] == s)[:, None], dof, axis=1)) for s in range(len(SHAPES))]
    out += [(name, np.repeat(m[:, None], dof, axis=1)) for name, m in tie_classes(S["tie"], dof).items()]
    return out


def counts(S):
    """{class: lanes (kind x case) or queries (shapes, tie classes)}."""
    return {name: int(m.sum()) if "." in name else int(m.any(axis=1).sum()) for name, m in classes(S)}


def present(S):
    """The names of the classes that hold at least FLOOR lanes / queries in S: the FILLED cells of kind x case, and every shape and
    tie class that can exist."""
    no = impossible(S["set"], S["dof"])
    return list(FILLED[(S["name"], S["semantics"])]) + [name for name, _ in classes(S) if "." not in name and name not in no]


def describe(S, lanes):
    """The kinds, cases, shapes and tie classes of the lanes in `lanes` ([n][dof], or [n] for whole queries), for assertion messages."""
    lanes = np.asarray(lanes, dtype=bool)
    if lanes.ndim == 1:
        lanes = np.repeat(lanes[:, None], S["dof"], axis=1)
    where = np.argwhere(lanes)
    if where.size == 0:
        return "no lanes"
    hit = [f"{name}: {int((m & lanes).sum())}" for name, m in classes(S) if (m & lanes).any()]
    first = ", ".join(f"(q {q}, joint {j}: {KINDS[S['kind'][q, j]]}, c{S['cen']['case'][q, j]}, {SHAPES[S['shape'][q]]})" for q, j in where[:4])
    return f"{len(where)} lanes; classes {{" + ", ".join(hit) + "}; first " + first


# (batch, semantics) -> the kind x case cells that hold at least FLOOR lanes. Every other cell holds fewer, most of them none: a lane
# that stands still has a handful of outcomes, and under these acceleration-limited sets a lane that moves ends in c1 / c2 almost always
# (tests/test_branch_census_cpu.py, NAMED: c3-c6 in 434 of 120 000 ref lanes, none under panda, c7 / c8 never), so no batch of a
# size a test can afford fills the rest; the jerk-dominated soft set of branch_census.py pins those cases in bulk. The lanes of an
# unfilled cell are compared like all others, only no floor is claimed for them.
_STILL = ("random.c-1", "random.c1", "random.c2", "rest.c-1", "rest.c0", "rest.c3", "near.c0", "rest_to_rest.c-1", "rest_to_rest.c1",
          "stop_only.c-1", "stop_only.c0")
_COPIES = ("twin.c-1", "twin.c1", "mirror.c-1", "mirror.c1")
FILLED = {
    # panda: a_max / j_max < Ts, a lane that stands still has t_opt[6] = 0.002 and is scaled by c1 / c2 or falls back
    ("panda7", "cpp"): ("random.c-1", "random.c1", "random.c2", "rest.c-1", "rest.c0", "rest.c1", "rest.c2", "near.c-1", "near.c0", "near.c1",
                        "near.c2", "rest_to_rest.c-1", "rest_to_rest.c1", "stop_only.c-1", "stop_only.c0", "stop_only.c1", "stop_only.c4"),
    ("ref7", "cpp"): _STILL + _COPIES + ("stop_only.c4", "twin.c0", "twin.c4", "mirror.c0", "mirror.c4"),
    ("ref7", "matlab"): _STILL + _COPIES + ("twin.c0", "mirror.c0"),
    ("ref9", "cpp"): _STILL + _COPIES + ("stop_only.c4", "twin.c0", "twin.c2", "twin.c4", "mirror.c0"),
    ("ref30", "cpp"): _STILL + _COPIES + ("stop_only.c4", "twin.c0", "twin.c2", "mirror.c0", "mirror.c2"),
    ("ref2", "cpp"): _STILL + _COPIES + ("stop_only.c4", "twin.c4", "mirror.c4"),
}
FILLED[("panda7", "matlab")] = FILLED[("panda7", "cpp")]


def batch(oracle_mod, name, semantics="cpp", exact_pow=False, sample=True, cache={}):
    """The structured batch `name` of BATCHES planned by the oracle; computed once per process and left unchanged. A dict: name, set,
    dof, n, lim, qs, kind, shape, source, orc, rec (Oracle.plan_batch), cen (branch_census.census), tie (ties())."""
    key = (name, semantics, exact_pow, sample)
    if key not in cache:
        set_name, dof, n = BATCHES[name]
        lim = limit_set(set_name, dof)[1]
        orc = oracle_mod.Oracle(dof, TS, semantics=semantics, exact_pow=exact_pow, **lim)
        lim, qs, kind, shape, source = generate(orc, set_name, dof, n)
        rec = orc.plan_batch(*qs, sample=sample)
        S = dict(name=name, set=set_name, dof=dof, n=n, lim=lim, qs=qs, kind=kind, shape=shape, source=source, orc=orc, rec=rec,
                 semantics=semantics, exact_pow=exact_pow, cen=bc.census(orc, lim, qs, rec), tie=ties(rec))
        cache[key] = S
    return cache[key]


def assert_floors(S):
    """Every FILLED cell, every shape and every tie class that can exist holds at least FLOOR lanes (kind x case) or queries; what
    cannot exist is empty; and FILLED is complete: every other kind x case cell holds fewer than FLOOR lanes."""
    c = counts(S)
    no = impossible(S["set"], S["dof"])
    filled = set(FILLED[(S["name"], S["semantics"])])
    assert no <= set(c) and filled <= set(c), (sorted(no - set(c)), sorted(filled - set(c)))
    wrong = [f"{k}: {c[k]} queries of a class that cannot exist" for k in sorted(no) if c[k]]
    wrong += [f"{k}: {c[k]} < {FLOOR}" for k in present(S) if c[k] < FLOOR]
    wrong += [f"{k}: {c[k]} >= {FLOOR} but not listed in FILLED" for k in sorted(c) if "." in k and k not in filled and c[k] >= FLOOR]
    assert not wrong, f"{S['name']} ({S['semantics']}): " + "; ".join(wrong)
