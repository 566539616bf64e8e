"""First exits (ltp_first_exit_batch, include/ltp_hip.h) on the GPU: per plan, selected array of q, v, a, j and joint the smallest
trajectory sample t in [k, k + H) that lies outside a box, compared for EQUALITY with the exhaustive scan of the full-row sampler's
rows for the same batch (tests/first_exit_checker.py, itself pinned to a plain loop by tests/test_first_exit_cpu.py) in every (plan,
array, joint): no case is excused. The boxes sit at seeded fractions of each row's own range, so almost every lane has an exit and
none sits on a sample by construction. The batches and planner helpers are tests/horizon_helpers.py's and tests/gpu_helpers.py's."""
import ctypes as C

import numpy as np
import pytest

import first_exit_checker as fc
import horizon_helpers as H
import run_census as rc
from gpu_helpers import _rows
from horizon_helpers import DEV, INVALID

pytestmark = pytest.mark.gpu

REJECTED = 11                 # the plan every batch of _batch() has rejected: LTP_EXIT_NO_PLAN among planned neighbours
MASKS = ("q", "v", "qv", "aj", "qvaj")
HORIZONS = (1, 2, 64, 240, 1 << 30)
GUARD = -77                   # what a buffer holds before a call that must not write (all of) it
LETTERS = "qvaj"


_CACHE = {}


def _batch(name, n, pow_rule="libm"):
    """H.batch with one rejected plan (a start velocity no limit admits) and the row ranges of every plan; the latest one is kept."""
    import torch
    key = (name, n, pow_rule)
    if _CACHE.get("key") != key:
        _CACHE.clear()
        ltp, dof, lim = H.planner(name, pow_rule)
        qs = H.queries(lim, n)
        qs[2][REJECTED, 0] = 99.0
        batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
        full = H.full_rows(ltp, batch)
        lens = batch.traj_len.cpu().numpy()
        assert lens[REJECTED] == 0 and np.mean(lens > 0) >= 0.95
        mn, mx = fc.row_ranges(full, batch.offsets, batch.traj_len, dof, 0, n)
        torch.cuda.synchronize()
        _CACHE.update(key=key, v=(ltp, dof, lim, qs, batch, full, lens, mn, mx))
    return _CACHE["v"]


def _starts(rng, lens):
    """k per plan, uniform in [-3, traj_len + 3]."""
    return rng.integers(-3, lens.astype(np.int64) + 4).astype(np.int32)


def _sides(mask, box4):
    """The dict by array letter firstExit takes, from a box tensor [count, 4, dof] (None: the default on that side)."""
    if box4 is None:
        return None
    return {LETTERS[x]: box4[:, x].contiguous() for x in fc.selected(mask)}


def _mask_of(arrays):
    from longtermplanner_amd import LongTermPlanner
    return LongTermPlanner._env_arrays(arrays)


def _assert_exits(ltp, batch, full, k_host, horizon, first, count, lo4, hi4, what, masks=MASKS, describe=None):
    """One call per mask over plans [first, first + count) with starts k_host[first:first + count] (an int: uniform) and the boxes
    lo4 / hi4 [count, 4, dof], every int of the table and of first_any EQUAL to the checker's; the buffer is exactly the call's
    elements long between guard words, and those stay. Returns {mask: (table, first_any)}."""
    import torch
    dof = batch.dof
    if isinstance(k_host, (int, np.integer)):
        start = int(k_host)
        k = torch.full((count,), start, dtype=torch.int32, device=DEV)
    else:
        start = k = torch.from_numpy(np.ascontiguousarray(k_host[first:first + count])).to(DEV)
    want_all, _ = fc.expected(full, batch.offsets, batch.traj_len, k, horizon, dof, first, count, lo4, hi4, mask=15)
    got = {}
    for arrays in masks:
        mask = _mask_of(arrays)
        planes = fc.selected(mask)
        need = count * len(planes) * dof
        assert ltp._lib.ltp_first_exit_elements(ltp._h, count, mask) == need
        buf = torch.full((need + 32,), GUARD, dtype=torch.int32, device=DEV)
        any_buf = torch.full((count + 32,), GUARD, dtype=torch.int32, device=DEV)
        table, first_any = ltp.firstExit(batch, first, count, start, horizon, arrays=arrays, lo=_sides(mask, lo4), hi=_sides(mask, hi4),
                                         any=any_buf[16:16 + count], out=buf[16:16 + need])
        torch.cuda.synchronize()
        assert bool((buf[:16] == GUARD).all().item()) and bool((buf[16 + need:] == GUARD).all().item()), f"{what} {arrays}: ints beside the call's were written"
        assert bool((any_buf[:16] == GUARD).all().item()) and bool((any_buf[16 + count:] == GUARD).all().item()), f"{what} {arrays}: first_any beside the call's"
        want = want_all[:, planes].contiguous()
        bad = (table != want).flatten(1).any(dim=1)
        if bool(bad.any().item()):
            i = int(bad.nonzero()[0].item())
            x, j = [int(v) for v in (table[i] != want[i]).nonzero()[0]]
            sel = np.zeros(batch.n, dtype=bool)
            sel[first:first + count] = bad.cpu().numpy()
            where = describe(sel) if describe else ""
            raise AssertionError(f"{what} arrays {arrays} H {horizon}: {int(bad.sum().item())} plans differ from the exhaustive scan; local plan {i} "
                                 f"plane {x} joint {j}: got {int(table[i, x, j])}, the scan {int(want[i, x, j])}, k {int(k[i])}, "
                                 f"traj_len {int(batch.traj_len[first + i])}, box [{float(lo4[i, planes[x], j])!r}, {float(hi4[i, planes[x], j])!r}] {where}")
        assert torch.equal(first_any, fc.fold_any(want).int()), f"{what} {arrays}: first_any differs"
        got[arrays] = (table, first_any)
    return got


@pytest.mark.parametrize("name,n,pow_rule", [("panda", 2000, "libm"), ("panda", 2000, "exact"), ("ref", 500, "libm"), ("ref", 500, "exact"),
                                             ("ref30", 200, "libm"), ("ref30", 200, "exact")])
def test_first_exits_against_the_exhaustive_scan(name, n, pow_rule):
    """Masks q, v, qv, aj and qvaj; uniform k = 0 and k per plan from [-3, traj_len + 3]; horizons 1, 2, 64, 240 and 2^30; the whole
    batch (with its rejected plan) and a slice with first > 0 whose count is no multiple of 64; boxes at seeded fractions of every
    row's own range. EQUALITY with the exhaustive scan in every (plan, array, joint) and in first_any."""
    ltp, dof, lim, qs, batch, full, lens, mn, mx = _batch(name, n, pow_rule)
    rng = np.random.default_rng(99)
    first, count = 5, {2000: 1003, 500: 403, 200: 131}[n]
    assert count % 64 != 0 and (count * dof) % 64 != 0 and first <= REJECTED < first + count
    lo, hi = fc.fraction_boxes(mn, mx, seed=7)
    exits = lanes = 0
    for horizon in HORIZONS:
        for k in (0, _starts(rng, lens)):
            what = f"{name} {pow_rule} k {'per plan' if not isinstance(k, int) else k}"
            got = _assert_exits(ltp, batch, full, k, horizon, 0, n, lo, hi, f"{what} whole batch")
            _assert_exits(ltp, batch, full, k, horizon, first, count, lo[first:first + count], hi[first:first + count], f"{what} plans [{first}, {first + count})")
            table, first_any = got["qvaj"]
            assert bool((table[REJECTED] == fc.EXIT_NO_PLAN).all().item()) and int(first_any[REJECTED]) == fc.EXIT_NO_PLAN
            if horizon == 1 << 30 and isinstance(k, int):
                exits, lanes = int((table >= 0).sum().item()), int((table != fc.EXIT_NO_PLAN).sum().item())
    print(f"{name} {pow_rule}: from k = 0 over the whole plan {exits} of {lanes} lanes leave their box")
    assert exits >= 0.9 * lanes                                  # constant rows (range 0) never leave their degenerate box


def test_the_smallest_shapes():
    """One joint; a robot at rest (traj_len 1) and a rejected plan (LTP_EXIT_NO_PLAN in every plane and in first_any) among moving
    ones; H = 1; k = traj_len - 1, traj_len and traj_len + 5; an exit exactly at k; an exit only past the end (a v, a, j box that
    excludes 0 against a q box that holds the last position)."""
    import torch
    from longtermplanner_amd import LongTermPlanner, generate_queries
    lim = dict(q_min=[-3.0], q_max=[3.0], v_max=[2.0], a_max=[10.0], j_max=[5000.0])
    ltp = LongTermPlanner(1, H.TS, device=0, **lim)
    n = 70
    qs = [np.ascontiguousarray(x) for x in generate_queries(n, lim, seed=3)]
    qs[0][4] = qs[1][4]                                          # at rest at its goal
    qs[2][4] = qs[3][4] = 0.0
    qs[2][9] = 99.0                                              # rejected
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    full = H.full_rows(ltp, batch)
    lens = batch.traj_len.cpu().numpy()
    assert lens[4] == 1 and lens[9] == 0 and (np.delete(lens, [4, 9]) > 2).all(), lens
    L = batch.traj_len
    mn, mx = fc.row_ranges(full, batch.offsets, L, 1, 0, n)
    lo, hi = fc.fraction_boxes(mn, mx, seed=1)
    rng = np.random.default_rng(2)
    for horizon in (1, 2, 5, 1 << 30):
        for k in (0, 1, _starts(rng, lens), (lens - 1).astype(np.int32), lens.astype(np.int32), (lens + 5).astype(np.int32)):
            got = _assert_exits(ltp, batch, full, k, horizon, 0, n, lo, hi, "one joint")
            table, first_any = got["qvaj"]
            assert bool((table[9] == fc.EXIT_NO_PLAN).all().item()) and int(first_any[9]) == fc.EXIT_NO_PLAN
            assert bool((table[4] == fc.EXIT_NONE).all().item()), "the robot at rest left the degenerate box of its constant rows"
    # an exit exactly at k: the box ends just below the sample at k (planned plans, k inside the trajectory)
    k = np.clip(_starts(rng, lens), 0, np.maximum(lens - 1, 0)).astype(np.int32)
    kt = torch.from_numpy(k).to(DEV)
    at_k = fc._gather(full, batch.offsets[:n].long(), L.long(), 1, kt.long()[:, None])[..., 0]        # [n, 4, 1]
    below = at_k - 1e-6
    got = _assert_exits(ltp, batch, full, k, 240, 0, n, torch.full_like(at_k, -float("inf")), below, "an exit at k")
    planned = L > 0
    assert bool((got["qvaj"][0][planned] == kt[planned, None, None]).all().item())
    # an exit only past the end: boxes that hold every sample of v, a and j but not the 0 behind the last one
    wide_lo, wide_hi = torch.nan_to_num(mn - 1.0, nan=0.0), torch.nan_to_num(mx + 1.0, nan=0.0)
    no_zero = wide_lo.clone()
    no_zero[:, 1:] = 1e-9                                        # v, a, j: [1e-9, max + 1] excludes 0; q keeps its wide box
    for k, horizon, reaches in (((lens - 1).astype(np.int32), 1, False), ((lens - 1).astype(np.int32), 2, True), (lens.astype(np.int32), 1, True),
                                ((lens + 5).astype(np.int32), 64, True)):
        got = _assert_exits(ltp, batch, full, k, horizon, 0, n, no_zero, wide_hi, "past the end", masks=("qvaj", "vaj", "q"))
        table = got["qvaj"][0]
        assert bool((table[planned][:, 0] == fc.EXIT_NONE).all().item()), "q left a box that holds its last position"
        if reaches and horizon < 64:
            # (from traj_len - 1 the last real sample may lie below 1e-9 itself: then it is the exit)
            ends = (table[planned][:, 1:] == L[planned, None, None]) | (table[planned][:, 1:] == L[planned, None, None] - 1)
            assert bool(ends.all().item())
        if horizon == 64:
            assert bool((table[planned][:, 1:] == L[planned, None, None]).all().item()), "v, a, j past the end: the exit is sample traj_len"
    # and the q sample past the end is the last position: from k >= traj_len a box below it is left at traj_len
    last = fc._gather(full, batch.offsets[:n].long(), L.long(), 1, (L.long() - 1).clamp(min=0)[:, None])[..., 0]
    got = _assert_exits(ltp, batch, full, (lens + 2).astype(np.int32), 3, 0, n, torch.full_like(last, -float("inf")), last - 1e-6, "q past the end", masks=("q",))
    assert bool((got["q"][0][planned][:, 0] == L[planned, None]).all().item())


def test_exits_on_either_side_of_a_run_boundary():
    """The bound is set to the midpoint between two neighbouring samples around a run boundary taken from the records' switching
    times — b - 1 | b for b = floor(t_x / Ts) + {0, 1, 2}, the cut points of the run walk — where the later sample is a new maximum
    of the row so far: the exit is then exactly the later sample, the last sample of a run for some offsets and the first of the
    next run for the others."""
    import torch
    n = 300
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    L = batch.traj_len.long()
    span = int(L.max().item())
    t = torch.arange(span, device=DEV)[None, :].expand(n, span)
    rows = fc._gather(full, batch.offsets[:n].long(), L, dof, torch.minimum(t, (L - 1).clamp(min=0)[:, None]))   # [n, 4, dof, span]
    so_far = rows.cummax(dim=3).values
    ts = torch.from_numpy(t_scaled).to(DEV)                      # [n, dof, 7]
    hit = total = 0
    for x_switch in (0, 2, 4, 6):
        for offset in (0, 1, 2):
            b = (torch.floor(ts[:, :, x_switch] / H.TS).long() + offset).clamp(min=1)
            b = torch.minimum(b, (L - 1).clamp(min=1)[:, None])[:, None, :, None].expand(n, 4, dof, 1)          # [n, 4, dof, 1]
            here, before = rows.gather(3, b)[..., 0], so_far.gather(3, b - 1)[..., 0]
            rises = (here > before) & (L > 1)[:, None, None]
            hi = torch.where(rises, 0.5 * (here + before), torch.full_like(here, float("inf")))
            rises &= (hi < here) & (hi >= before)                                                                # the midpoint separates the two
            hi = torch.where(rises, hi, torch.full_like(here, float("inf")))
            lo = torch.full_like(hi, -float("inf"))
            got = _assert_exits(ltp, batch, full, 0, 1 << 30, 0, n, lo, hi, f"run boundary switch {x_switch} + {offset}", masks=("qvaj",))
            table = got["qvaj"][0]
            assert bool((table[rises] == b[..., 0][rises]).all().item())
            hit, total = hit + int(rises.sum().item()), total + rises.numel()
    print(f"run boundaries: {hit} of {total} (lane, boundary) pairs rise across their boundary and exit exactly there")
    assert hit > 0.05 * total


@pytest.mark.parametrize("name", rc.BATCHES)
def test_short_runs(oracle_mod, name):
    """The run-census batches (rows of 1-153 samples, runs of 1-3 samples, collided switch indices, switching times on exact
    multiples of the sample time): a uniform k swept over 0 .. 4 and per-plan starts, short horizons and the whole plan."""
    R = _rows(oracle_mod, name)
    ltp, batch, n, cen, dof = R["ltp"], R["batch"], R["n"], R["cen"], R["dof"]
    lens = R["rec"]["traj_len"]
    mn, mx = fc.row_ranges(R["full"], batch.offsets, batch.traj_len, dof, 0, n)
    rng = np.random.default_rng(17)
    describe = lambda plans: rc.describe(cen, plans)
    for seed in (3, 4):
        lo, hi = fc.fraction_boxes(mn, mx, seed=seed)
        for horizon in (1, 3, 1 << 30):
            for k in list(range(5)) + [_starts(rng, lens)]:
                _assert_exits(ltp, batch, R["full"], k, horizon, 0, n, lo, hi, f"{name} k {'per plan' if not isinstance(k, int) else k}", masks=("qvaj",),
                              describe=describe)


def test_jerk_dominated_runs(oracle_mod):
    """The jerk-dominated soft set of tests/branch_census.py (every planner case, modified jerk profiles, fallback records): the
    first 200 plans of the dense batch, from k = 0 and per-plan starts."""
    import torch
    import branch_census as bc
    from gpu_helpers import _planner, _tensors
    dof, n_all, ts = bc.DENSE_BATCH
    orc, lim, qs, orec, cen = bc.soft_batch(oracle_mod, dof, n_all, ts)
    n = 200
    ltp = _planner(dof, lim, ts)
    batch = ltp.planSwitchTimesBatch(*_tensors([x[:n] for x in qs]))
    full = H.full_rows(ltp, batch)
    lens = batch.traj_len.cpu().numpy()
    assert np.mean(lens > 0) > 0.9
    mn, mx = fc.row_ranges(full, batch.offsets, batch.traj_len, dof, 0, n)
    lo, hi = fc.fraction_boxes(mn, mx, seed=11)
    rng = np.random.default_rng(5)
    for horizon in (64, 1 << 30):
        for k in (0, _starts(rng, lens)):
            _assert_exits(ltp, batch, full, k, horizon, 0, n, lo, hi, f"soft dense H {horizon}", masks=("qvaj", "q"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["retimed", "limit_sets", "matlab", "stop"])
def test_other_batch_kinds(kind):
    """A retimed batch, a batch with three bound limit sets, MATLAB semantics (full rows from the walk sampler) and a stop batch: each
    against the exhaustive scan of its own rows, whole and a sub-range. Under limit sets the default boxes equal explicit per-plan
    boxes built from each plan's own set, bit for bit in the ints."""
    import torch
    from longtermplanner_amd import limit_set
    if kind == "stop":
        n = 300
        ltp, dof, lim = H.planner("panda")
        qs = H.tensors(H.queries(lim, n))
        batch = ltp.planStopBatch(qs[1], qs[2], qs[3], check="inputs")
        full = H.full_rows(ltp, batch)
        lens = batch.traj_len.cpu().numpy()
        assert np.mean(lens > 0) > 0.9
    else:
        n = 500
        ltp, dof, batch, full, lens, _ = H.other_batch(kind, n)
    mn, mx = fc.row_ranges(full, batch.offsets, batch.traj_len, dof, 0, n)
    lo, hi = fc.fraction_boxes(mn, mx, seed=13)
    rng = np.random.default_rng(21)
    first, count = H.odd_range(n, dof)
    for horizon in (64, 1 << 30):
        k = _starts(rng, lens)
        _assert_exits(ltp, batch, full, k, horizon, 0, n, lo, hi, f"{kind} H {horizon}", masks=("qvaj",))
        _assert_exits(ltp, batch, full, k, horizon, first, count, lo[first:first + count], hi[first:first + count], f"{kind} H {horizon} sub-range",
                      masks=("qvaj", "va"))
    if kind == "limit_sets":
        _, lim = limit_set("panda")
        sets = {key: np.array([[f * x if key in ("v_max", "a_max", "j_max") else x for x in lim[key]] for f in (1.0, 0.5, 0.25)]) for key in lim}
        d_lo, d_hi = fc.default_boxes(n, sets, DEV, set_index=batch.limit_set)
        assert float((d_hi[0, 1] / d_hi[1, 1]).min()) == 2.0     # plan 0 reads set 0, plan 1 set 1
        for horizon in (240, 1 << 30):
            default = ltp.firstExit(batch, 0, n, 0, horizon, arrays="qvaj")
            explicit = _assert_exits(ltp, batch, full, 0, horizon, 0, n, d_lo, d_hi, "limit sets, explicit per-plan boxes", masks=("qvaj",))["qvaj"][0]
            torch.cuda.synchronize()
            assert torch.equal(default, explicit), "the default boxes are not the plan's own set"
            assert int((default[:, 1:3] >= 0).sum().item()) > 0


def test_identities_and_the_path_limit_verdict():
    """Default boxes equal explicit [dof] boxes holding the handle's limits; one box per joint (stride 0) equals the same box
    broadcast to [count, dof]; a mask's planes equal the single-array calls' planes; status is left alone. With q, k = 0, H = 2^30
    and default boxes, exit == LTP_EXIT_NONE exactly for the plans whose dense q rows stay inside [q_min, q_max] and the right index
    for the others — queries that start near a joint stop with velocity towards it overshoot in the middle while
    LTP_STATUS_END_LIMIT stays clear: the verdict the reference does not form."""
    import torch
    n = 600
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    q_min, q_max, v_max = (np.asarray(lim[key]) for key in ("q_min", "q_max", "v_max"))
    for p in range(0, n, 6):                                     # every sixth plan: joint p % dof starts close to its upper stop, moving towards it
        j = p % dof
        qs[1][p, j] = q_max[j] - 0.002
        qs[2][p, j] = 0.6 * v_max[j]
        qs[3][p, j] = 0.0
        qs[0][p, j] = q_max[j] - 0.4 * (q_max[j] - q_min[j])
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    full = H.full_rows(ltp, batch)                               # (the sampler forms the end-limit verdict)
    status = batch.status.clone()
    lens = batch.traj_len.cpu().numpy()
    d_lo, d_hi = fc.default_boxes(n, lim, DEV)
    got = _assert_exits(ltp, batch, full, 0, 1 << 30, 0, n, d_lo, d_hi, "explicit boxes holding the handle's limits", masks=("q", "qvaj"))
    verdict = ltp.firstExit(batch, 0, n, 0, 1 << 30)             # arrays="q", default boxes
    torch.cuda.synchronize()
    assert verdict.shape == (n, 1, dof) and torch.equal(verdict, got["q"][0])
    mn, mx = fc.row_ranges(full, batch.offsets, batch.traj_len, dof, 0, n)
    inside = (mn[:, 0] >= d_lo[:, 0]) & (mx[:, 0] <= d_hi[:, 0])                                                 # [n, dof], False for NaN
    planned = batch.traj_len > 0
    assert torch.equal((verdict[:, 0] == fc.EXIT_NONE)[planned], inside[planned])
    leaves = (verdict[:, 0] >= 0).any(dim=1)
    clear = (batch.status & 8) == 0
    middle = leaves & clear & planned
    print(f"path-limit verdict: {int(leaves.sum())} of {int(planned.sum())} plans leave [q_min, q_max], {int(middle.sum())} of them with END_LIMIT clear")
    assert int(middle.sum().item()) >= 10, "no plan overshoots in the middle with a legal last position: the test says little"
    # the full default call, and one box per joint against its broadcast
    everything = ltp.firstExit(batch, 0, n, 0, 1 << 30, arrays="qvaj")
    torch.cuda.synchronize()
    assert torch.equal(everything, got["qvaj"][0])
    rng = np.random.default_rng(3)
    k = torch.from_numpy(_starts(rng, lens)).to(DEV)
    first, count = H.odd_range(n, dof)
    one_lo, one_hi = 0.5 * d_lo[0].contiguous(), 0.5 * d_hi[0].contiguous()                                      # [4, dof]
    for f, c in ((0, n), (first, count)):
        kk = k[f:f + c].contiguous()
        shared, shared_any = ltp.firstExit(batch, f, c, kk, 240, arrays="qvaj", lo={a: one_lo[x].contiguous() for x, a in enumerate(LETTERS)},
                                           hi={a: one_hi[x].contiguous() for x, a in enumerate(LETTERS)}, any=True)
        each, each_any = ltp.firstExit(batch, f, c, kk, 240, arrays="qvaj", lo={a: one_lo[x].expand(c, dof).contiguous() for x, a in enumerate(LETTERS)},
                                       hi={a: one_hi[x].expand(c, dof).contiguous() for x, a in enumerate(LETTERS)}, any=True)
        torch.cuda.synchronize()
        assert torch.equal(shared, each) and torch.equal(shared_any, each_any)
        assert int((shared >= 0).sum().item()) > 0
        # a mask's planes are the single-array calls' planes, with one side given and the other the default
        for arrays in ("q", "v", "a", "j", "qv", "aj", "qaj"):
            planes = fc.selected(_mask_of(arrays))
            part = ltp.firstExit(batch, f, c, kk, 240, arrays=arrays, hi={a: one_hi["qvaj".index(a)].contiguous() for a in arrays})
            whole = ltp.firstExit(batch, f, c, kk, 240, arrays="qvaj", hi={a: one_hi[x].contiguous() for x, a in enumerate(LETTERS)})
            torch.cuda.synchronize()
            assert part.shape == (c, len(planes), dof) and torch.equal(part, whole[:, planes].contiguous()), arrays
    by_mask = ltp.firstExit(batch, 0, n, 3, 64, arrays=12)
    by_name = ltp.firstExit(batch, 0, n, 3, 64, arrays="ja")
    torch.cuda.synchronize()
    assert torch.equal(by_mask, by_name)
    assert torch.equal(batch.status, status), "firstExit changed batch.status"


def test_refusals_and_bounds():
    """Each refusal of the device entry is LTP_ERR_INVALID_ARGUMENT, its text names the reason, and the guard-filled buffer it was
    given keeps its pattern; a geometry change after planning is refused in ltp_state_at_batch's words; a call whose buffer is
    exactly ltp_first_exit_elements long writes nothing beside it. The wrappers refuse a bad mask, horizon or box (ValueError) and
    the host entry its own arguments (LtpError) before any launch."""
    import torch
    from longtermplanner_amd import _abi
    from longtermplanner_amd._abi import LtpError
    n = 64
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    lib, O = ltp._lib, _abi.FirstExitOpts
    P = C.c_void_p * 4
    need = n * 4 * dof
    assert lib.ltp_first_exit_elements(ltp._h, n, 15) == need and lib.ltp_first_exit_elements(ltp._h, n, 5) == need // 2
    assert lib.ltp_first_exit_elements(ltp._h, n, 0) == 0 and lib.ltp_first_exit_elements(ltp._h, n, 16) == 0 and lib.ltp_first_exit_elements(ltp._h, 0, 15) == 0
    buf = torch.full((need + 64,), GUARD, dtype=torch.int32, device=DEV)
    out = buf[32:32 + need]
    box = torch.zeros((dof,), dtype=torch.float64, device=DEV) + 0.5
    call = H.reader_call(lib.ltp_first_exit_batch, ltp, batch, n, out, capacity=need)
    good = dict(size=C.sizeof(O), arrays=15, horizon=240, box_joint_stride=1)
    status = batch.status.clone()
    rc_, msg = call(O(**good))
    assert rc_ == 0, msg
    torch.cuda.synchronize()
    want = ltp.firstExit(batch, 0, n, 0, 240, arrays="qvaj")
    torch.cuda.synchronize()
    assert torch.equal(out, want.reshape(-1)), "first_any = NULL changes the table"
    assert bool((buf[:32] == GUARD).all().item()) and bool((buf[32 + need:] == GUARD).all().item()), "ints beside the call's elements were written"
    assert torch.equal(batch.status, status)
    buf.fill_(GUARD)
    refusals = [(dict(q=False), {}, "null"), (dict(r=False), {}, "null"), (dict(out_ptr=0), {}, "null"), (dict(capacity=need - 1), {}, "ltp_first_exit_elements"),
                ({}, dict(size=C.sizeof(O) - 8), "size"), ({}, dict(size=C.sizeof(O) + 4), "multiple of 8"),
                ({}, dict(arrays=0), "arrays"), ({}, dict(arrays=16), "arrays"), ({}, dict(arrays=-1), "arrays"),
                ({}, dict(horizon=0), "horizon"), ({}, dict(horizon=-5), "horizon"), ({}, dict(horizon=(1 << 30) + 1), "horizon"),
                ({}, dict(arrays=1, lo=P(None, box.data_ptr(), None, None)), "not selected"),
                ({}, dict(arrays=14, hi=P(box.data_ptr(), None, None, None)), "not selected"),
                ({}, dict(hi=P(box.data_ptr(), None, None, None), box_joint_stride=0), "box_joint_stride")]
    for kw, bad, text in refusals:
        rc_, msg = call(O(**dict(good, **bad)), **kw)
        assert rc_ == INVALID and text in msg, (kw, bad, rc_, msg)
    rc_, msg = call()
    assert rc_ == INVALID and "NULL" in msg
    # the capacity is held against the mask's own element count
    rc_, msg = call(O(**dict(good, arrays=3)), capacity=need // 2 - 1)
    assert rc_ == INVALID and "ltp_first_exit_elements" in msg
    # a newer caller's struct: zero bytes beyond the known fields pass, non-zero ones are refused
    raw = (C.c_ubyte * (C.sizeof(O) + 8))()
    newer = O(**dict(good, size=C.sizeof(O) + 8))
    C.memmove(raw, C.addressof(newer), C.sizeof(O))
    raw[C.sizeof(O) + 3] = 1
    rc_, msg = call(raw=C.addressof(raw))
    assert rc_ == INVALID and "beyond the fields" in msg
    # the geometry rule, in ltp_state_at_batch's words
    rec = batch.c_records()
    scratch = torch.zeros((n * dof,), dtype=torch.float64, device=DEV)
    for change, undo in ((lambda: ltp.setDoF(6), lambda: ltp.setDoF(dof)), (lambda: ltp.setSampleTime(0.002), lambda: ltp.setSampleTime(H.TS))):
        change()
        rc_, msg = call(O(**good))
        rc2 = lib.ltp_state_at_batch(ltp._h, 0, n, C.byref(batch.queries), C.byref(rec), None, 0, scratch.data_ptr(), scratch.data_ptr(), scratch.data_ptr(),
                                     dof, 1, ltp._stream())
        msg2 = (lib.ltp_last_error(ltp._h) or b"").decode()
        assert rc_ == INVALID and rc2 == INVALID and msg == msg2 and "changed since the batch was planned" in msg
        undo()
    # the wrappers: ValueError before any device work
    view = out.view(n, 4, dof)
    for kw in (dict(arrays="qq"), dict(arrays=0), dict(arrays=16), dict(horizon=0), dict(horizon=(1 << 30) + 1), dict(arrays="q", lo={"v": box}),
               dict(lo={"q": box[:6]}), dict(lo={"q": box}, hi={"q": box.expand(n, dof).contiguous()})):
        args = dict(dict(horizon=240, arrays="qvaj"), **kw)
        with pytest.raises(ValueError):
            ltp.firstExit(batch, 0, n, 0, args.pop("horizon"), out=view, **args)
    host_box = np.full(dof, 0.5)
    for kw in (dict(arrays="x"), dict(horizon=0), dict(arrays="q", hi={"j": host_box}), dict(lo={"q": host_box[:3]})):
        args = dict(dict(horizon=240, arrays="qvaj"), **kw)
        with pytest.raises(ValueError):
            ltp.planFirstExitHost(*qs, 0, args.pop("horizon"), **args)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    host_out = np.full(need, GUARD, dtype=np.int32)
    boxes = (dp * 4)(None, host_box.ctypes.data_as(dp), None, None)
    for arrays, horizon, per_plan, his, text in ((0, 240, 0, None, "arrays"), (16, 240, 0, None, "arrays"), (15, 0, 0, None, "horizon"),
                                                 (15, (1 << 30) + 1, 0, None, "horizon"), (15, 240, 2, None, "box_per_plan"), (1, 240, 0, boxes, "not selected")):
        rc_ = lib.ltp_plan_first_exit_host(ltp._h, n, *[x.ctypes.data_as(dp) for x in qs], None, 0, horizon, arrays, None, his, per_plan, None,
                                           host_out.ctypes.data_as(ip), None)
        assert rc_ == INVALID and text in (lib.ltp_last_error(ltp._h) or b"").decode(), (arrays, horizon, per_plan)
    assert (host_out == GUARD).all()
    with pytest.raises(LtpError):
        ltp._check(lib.ltp_plan_first_exit_host(ltp._h, n, *[x.ctypes.data_as(dp) for x in qs], None, 0, 240, 15, None, None, 0, None, None, None))
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all().item()), "a refused call wrote to the buffer"
    assert call(O(**good))[0] == 0


DROPIN = r'''
#include "long_term_planner/long_term_planner.h"
#include <cstdio>
using namespace long_term_planner;
int main(int argc, char** argv) {
  const int dof = 7, n = 40;
  std::vector<double> q_min = {-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973};
  std::vector<double> q_max = {2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973};
  std::vector<double> v_max = {2.175, 2.175, 2.175, 2.175, 2.61, 2.61, 2.61};
  std::vector<double> a_max = {15.0, 7.5, 10.0, 12.5, 15.0, 20.0, 20.0};
  std::vector<double> j_max = {7500.0, 3750.0, 5000.0, 6250.0, 7500.0, 10000.0, 10000.0};
  LongTermPlanner ltp(dof, 0.001, q_min, q_max, v_max, a_max, j_max);
  std::vector<double> in(4 * n * dof), v_hi(n * dof), a_lo(n * dof);
  std::vector<int> k(n);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size() || std::fread(k.data(), sizeof(int), k.size(), f) != k.size() ||
      std::fread(v_hi.data(), sizeof(double), v_hi.size(), f) != v_hi.size() || std::fread(a_lo.data(), sizeof(double), a_lo.size(), f) != a_lo.size()) return 2;
  std::fclose(f);
  std::vector<int> exits, any;
  BatchTrajectory b;
  const double* los[4] = {nullptr, nullptr, a_lo.data(), nullptr};
  const double* his[4] = {nullptr, v_hi.data(), nullptr, nullptr};
  const long long ok = ltp.planFirstExitBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, 500,
                                              LTP_ENV_Q | LTP_ENV_V | LTP_ENV_A, los, his, true, exits, &any, &b);
  int refused = 0;
  for (int arrays : {0, 16}) {
    try {
      std::vector<int> e2;
      ltp.planFirstExitBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, 500, arrays, nullptr, nullptr, false, e2);
    } catch (const std::exception&) { ++refused; }
  }
  for (int horizon : {0, -1}) {
    try {
      std::vector<int> e2;
      ltp.planFirstExitBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, horizon, LTP_ENV_Q, nullptr, nullptr, false, e2);
    } catch (const std::exception&) { ++refused; }
  }
  try {
    std::vector<int> e2;
    ltp.planFirstExitBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, 500, LTP_ENV_Q, nullptr, his, true, e2);
  } catch (const std::exception&) { ++refused; }
  if (refused != 5) return 3;
  FILE* o = std::fopen(argv[2], "wb");
  std::fwrite(exits.data(), sizeof(int), exits.size(), o);
  std::fwrite(any.data(), sizeof(int), any.size(), o);
  std::fwrite(b.status.data(), sizeof(int), b.status.size(), o);
  std::fclose(o);
  std::printf("%lld ok, %zu ints\n", ok, exits.size());
  return 0;
}
'''


def test_host_and_dropin_paths(tmp_path):
    """planFirstExitHost equals the device call int for int (boxes [dof] and [n, dof], with and without first_any) and its status
    carries END_LIMIT like planBatchHost(sample=False); a small C++ program gives the same bytes through
    LongTermPlanner::planFirstExitBatch."""
    import torch
    n = 40
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    qs[0][3, 1] = 2.5                               # a goal beyond joint 1's range: planned, then END_LIMIT
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    lens = batch.traj_len.cpu().numpy()
    k = _starts(np.random.default_rng(1), lens)
    rng = np.random.default_rng(2)
    v_hi = rng.uniform(0.2, 1.0, (n, dof)) * np.asarray(lim["v_max"])
    a_lo = -rng.uniform(0.2, 1.0, (n, dof)) * np.asarray(lim["a_max"])
    dev, dev_any = ltp.firstExit(batch, 0, n, torch.from_numpy(k).to(DEV), 500, arrays="qva", lo={"a": torch.from_numpy(a_lo).to(DEV)},
                                 hi={"v": torch.from_numpy(v_hi).to(DEV)}, any=True)
    dev, dev_any = dev.cpu().numpy(), dev_any.cpu().numpy()
    assert (dev >= 0).sum() > 0 and (dev == fc.EXIT_NONE).sum() > 0
    assert not (batch.status.cpu().numpy()[3] & 8), "the device call forms no end-limit verdict"
    rec, table, first_any = ltp.planFirstExitHost(*qs, k, 500, arrays=7, lo={"a": a_lo}, hi={"v": v_hi}, any=True)
    assert table.shape == (n, 3, dof) and table.dtype == np.int32
    assert np.array_equal(table, dev) and np.array_equal(first_any, dev_any)
    plain = ltp.planBatchHost(*qs, sample=False)
    assert np.array_equal(rec["status"], plain["status"]) and (rec["status"][3] & 8) and np.array_equal(rec["traj_len"], lens)
    # a uniform k, one box per joint, no first_any
    one = 0.5 * np.asarray(lim["v_max"])
    _, table_u = ltp.planFirstExitHost(*qs, 5, 1 << 30, arrays="v", lo={"v": -one}, hi={"v": one})
    dev_u = ltp.firstExit(batch, 0, n, 5, 1 << 30, arrays="v", lo={"v": torch.from_numpy(-one).to(DEV)}, hi={"v": torch.from_numpy(one).to(DEV)})
    assert table_u.shape == (n, 1, dof) and np.array_equal(table_u, dev_u.cpu().numpy())

    raw = H.run_dropin(tmp_path, "first_exit", DROPIN, np.concatenate([x.reshape(-1) for x in qs]).astype(np.float64).tobytes()
                       + k.astype(np.int32).tobytes() + v_hi.tobytes() + a_lo.tobytes())
    assert raw == table.tobytes() + first_any.tobytes() + rec["status"].astype(np.int32).tobytes()


@pytest.mark.parametrize("with_any", [False, True])
def test_graph_capture_and_replay_with_new_starts_and_new_boxes(with_any):
    """The call allocates nothing: captured on one stream (one kernel node, and one fill-kernel node before it with first_any) and
    replayed after first_sample AND the box arrays were rewritten in place, it gives what a direct call gives for the new starts
    and boxes, and what the exhaustive scan gives — twice."""
    import torch
    n = 1000
    ltp, dof, lim, qs, batch, full, lens, mn, mx = _batch("panda", n)
    rng = np.random.default_rng(77)
    ka, kb, kc = (_starts(rng, lens) for _ in range(3))
    assert np.count_nonzero(ka != kb) > 0.5 * n
    boxes = [fc.fraction_boxes(mn, mx, seed=s) for s in (21, 22, 23)]
    k = torch.from_numpy(ka).to(DEV)
    lo, hi = boxes[0][0].clone(), boxes[0][1].clone()
    mask = 15
    lo_by = {a: lo[:, x].contiguous() for x, a in enumerate(LETTERS)}
    hi_by = {a: hi[:, x].contiguous() for x, a in enumerate(LETTERS)}
    out = torch.zeros((n, 4, dof), dtype=torch.int32, device=DEV)
    first_any = torch.zeros((n,), dtype=torch.int32, device=DEV)
    graph = H.capture(lambda: ltp.firstExit(batch, 0, n, k, 240, arrays=mask, lo=lo_by, hi=hi_by, any=first_any if with_any else False, out=out))
    for k_new, (lo_new, hi_new) in ((kb, boxes[1]), (kc, boxes[2])):
        k.copy_(torch.from_numpy(k_new))
        for x, a in enumerate(LETTERS):
            lo_by[a].copy_(lo_new[:, x])
            hi_by[a].copy_(hi_new[:, x])
        out.zero_()
        first_any.fill_(12345)
        graph.replay()
        torch.cuda.synchronize()
        direct = ltp.firstExit(batch, 0, n, k, 240, arrays=mask, lo=lo_by, hi=hi_by, any=with_any)
        torch.cuda.synchronize()
        want, want_any = fc.expected(full, batch.offsets, batch.traj_len, k, 240, dof, 0, n, lo_new, hi_new)
        assert torch.equal(out, want)
        if with_any:
            assert torch.equal(direct[0], out) and torch.equal(direct[1], first_any) and torch.equal(first_any, want_any)
        else:
            assert torch.equal(direct, out) and bool((first_any == 12345).all().item())
