"""Settling (ltp_settle_batch, include/ltp_hip.h) on the GPU: per plan, selected array of q, v, a, j and joint the trajectory sample
from which the array is inside a box and stays inside for the rest of [k, k + H), compared for EQUALITY with the exhaustive scan of
the full-row sampler's rows for the same batch (tests/settle_checker.py, itself pinned to a plain loop by tests/test_settle_cpu.py)
in every (plan, array, joint): no case is excused. Two families of boxes go to the device: boxes around the value each row comes
to rest at (settle_checker.end_boxes: almost every lane settles at an index inside its plan) and boxes at seeded fractions of each
row's own range (first_exit_checker.fraction_boxes: q mostly rests outside, LTP_SETTLE_NOT_YET). The batches and planner helpers
are tests/horizon_helpers.py's and tests/gpu_helpers.py's."""
import ctypes as C

import numpy as np
import pytest

import horizon_helpers as H
import run_census as rc
import settle_checker as sc
from gpu_helpers import _rows
from horizon_helpers import DEV, INVALID

pytestmark = pytest.mark.gpu

REJECTED = 11                 # the plan every batch of _batch() has rejected: LTP_EXIT_NO_PLAN among planned neighbours
MASKS = ("q", "v", "qv", "aj", "qvaj")
HORIZONS = (1, 2, 64, 240, 1 << 30)
GUARD = -77                   # what a buffer holds before a call that must not write (all of) it
LETTERS = "qvaj"
EXIT_NONE = -1


_CACHE = {}


def _batch(name, n, pow_rule="libm"):
    """H.batch with one rejected plan (a start velocity no limit admits), the row ranges of every plan and the boxes around every
    row's resting value; the latest one is kept."""
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
        mn, mx = sc.row_ranges(full, batch.offsets, batch.traj_len, dof, 0, n)
        ends = sc.end_boxes(full, batch.offsets, batch.traj_len, dof, seed=8)
        torch.cuda.synchronize()
        _CACHE.update(key=key, v=(ltp, dof, lim, qs, batch, full, lens, mn, mx, ends))
    return _CACHE["v"]


def _starts(rng, lens):
    """k per plan, uniform in [-3, traj_len + 3]."""
    return rng.integers(-3, lens.astype(np.int64) + 4).astype(np.int32)


def _sides(mask, box4):
    """The dict by array letter settle takes, from a box tensor [count, 4, dof] (None: the default on that side)."""
    if box4 is None:
        return None
    return {LETTERS[x]: box4[:, x].contiguous() for x in sc.selected(mask)}


def _mask_of(arrays):
    from longtermplanner_amd import LongTermPlanner
    return LongTermPlanner._env_arrays(arrays)


def _samples(full, batch, n, dof, extra=1):
    """S_X(t) of every row for t in [0, max traj_len + extra): [n, 4, dof, span], the columns from traj_len on the resting state."""
    import torch
    L = batch.traj_len[:n].long()
    span = int(L.max().item()) + extra
    t = torch.arange(span, device=DEV)[None, :].expand(n, span)
    return sc._gather(full, batch.offsets[:n].long(), L, dof, t)


def _assert_settle(ltp, batch, full, k_host, horizon, first, count, lo4, hi4, what, masks=MASKS, describe=None):
    """One call per mask over plans [first, first + count) with starts k_host[first:first + count] (an int: uniform) and the boxes
    lo4 / hi4 [count, 4, dof], every int of the table and of settle_all EQUAL to the checker's; the buffer is exactly the call's
    elements long between guard words, and those stay. Returns {mask: (table, settle_all)}."""
    import torch
    dof = batch.dof
    if isinstance(k_host, (int, np.integer)):
        start = int(k_host)
        k = torch.full((count,), start, dtype=torch.int32, device=DEV)
    else:
        start = k = torch.from_numpy(np.ascontiguousarray(k_host[first:first + count])).to(DEV)
    want_all, _ = sc.expected(full, batch.offsets, batch.traj_len, k, horizon, dof, first, count, lo4, hi4, mask=15)
    got = {}
    for arrays in masks:
        mask = _mask_of(arrays)
        planes = sc.selected(mask)
        need = count * len(planes) * dof
        assert ltp._lib.ltp_settle_elements(ltp._h, count, mask) == need
        buf = torch.full((need + 32,), GUARD, dtype=torch.int32, device=DEV)
        all_buf = torch.full((count + 32,), GUARD, dtype=torch.int32, device=DEV)
        table, settle_all = ltp.settle(batch, first, count, start, horizon, arrays=arrays, lo=_sides(mask, lo4), hi=_sides(mask, hi4),
                                       all=all_buf[16:16 + count], out=buf[16:16 + need])
        torch.cuda.synchronize()
        assert bool((buf[:16] == GUARD).all().item()) and bool((buf[16 + need:] == GUARD).all().item()), f"{what} {arrays}: ints beside the call's were written"
        assert bool((all_buf[:16] == GUARD).all().item()) and bool((all_buf[16 + count:] == GUARD).all().item()), f"{what} {arrays}: settle_all beside the call's"
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
        assert torch.equal(settle_all, sc.fold_all(want).int()), f"{what} {arrays}: settle_all differs"
        got[arrays] = (table, settle_all)
    return got


@pytest.mark.parametrize("name,n,pow_rule", [("panda", 2000, "libm"), ("panda", 2000, "exact"), ("ref", 500, "libm"), ("ref", 500, "exact"),
                                             ("ref30", 200, "libm"), ("ref30", 200, "exact")])
def test_settling_against_the_exhaustive_scan(name, n, pow_rule):
    """Masks q, v, qv, aj and qvaj; uniform k = 0 and k per plan from [-3, traj_len + 3]; horizons 1, 2, 64, 240 and 2^30; the whole
    batch (with its rejected plan) and a slice with first > 0 whose count is no multiple of 64; both families of boxes. EQUALITY
    with the exhaustive scan in every (plan, array, joint) and in settle_all."""
    ltp, dof, lim, qs, batch, full, lens, mn, mx, ends = _batch(name, n, pow_rule)
    rng = np.random.default_rng(99)
    first, count = 5, {2000: 1003, 500: 403, 200: 131}[n]
    assert count % 64 != 0 and (count * dof) % 64 != 0 and first <= REJECTED < first + count
    families = dict(ends=ends, fractions=sc.fraction_boxes(mn, mx, seed=7))
    L = batch.traj_len[:, None, None]
    report = {}
    for family, (lo, hi) in families.items():
        for horizon in HORIZONS:
            for k in (0, _starts(rng, lens)):
                what = f"{name} {pow_rule} {family} k {'per plan' if not isinstance(k, int) else k}"
                got = _assert_settle(ltp, batch, full, k, horizon, 0, n, lo, hi, f"{what} whole batch")
                _assert_settle(ltp, batch, full, k, horizon, first, count, lo[first:first + count], hi[first:first + count], f"{what} plans [{first}, {first + count})")
                table, settle_all = got["qvaj"]
                assert bool((table[REJECTED] == sc.EXIT_NO_PLAN).all().item()) and int(settle_all[REJECTED]) == sc.EXIT_NO_PLAN
                if horizon == 1 << 30 and isinstance(k, int):
                    lanes = table != sc.EXIT_NO_PLAN
                    report[family] = (int(((table > 0) & (table <= L)).sum().item()), int((table[:, 0] == sc.SETTLE_NOT_YET).sum().item()),
                                      int(lanes.sum().item()), int(lanes[:, 0].sum().item()))
    print(f"{name} {pow_rule}: from k = 0 over the whole plan (lanes with 0 < s <= traj_len, q lanes NOT_YET, lanes, q lanes): {report}")
    inside, _, lanes, _ = report["ends"]
    assert inside >= 0.9 * lanes                                 # constant rows (range 0) never leave their degenerate box
    _, not_yet, _, q_lanes = report["fractions"]
    assert not_yet > 0.5 * q_lanes                               # the goal is an extreme of most q rows: it lies outside a box inside the range


def test_the_smallest_shapes():
    """One joint; a robot at rest (traj_len 1) and a rejected plan (LTP_EXIT_NO_PLAN in every plane and in settle_all) among moving
    ones; H = 1; k = traj_len - 1, traj_len and traj_len + 5; the last outside sample exactly at k; the last outside sample exactly
    at reach - 1 (LTP_SETTLE_NOT_YET with H, an index with H + 1); a v, a, j box that excludes 0 with reach > traj_len (NOT_YET)
    and with reach <= traj_len (an index); a q box that excludes the last position."""
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
    planned = L > 0
    mn, mx = sc.row_ranges(full, batch.offsets, L, 1, 0, n)
    rng = np.random.default_rng(2)
    for lo, hi in (sc.end_boxes(full, batch.offsets, L, 1, seed=1), sc.fraction_boxes(mn, mx, seed=1)):
        for horizon in (1, 2, 5, 1 << 30):
            for k in (0, 1, _starts(rng, lens), (lens - 1).astype(np.int32), lens.astype(np.int32), (lens + 5).astype(np.int32)):
                got = _assert_settle(ltp, batch, full, k, horizon, 0, n, lo, hi, "one joint")
                table, settle_all = got["qvaj"]
                assert bool((table[9] == sc.EXIT_NO_PLAN).all().item()) and int(settle_all[9]) == sc.EXIT_NO_PLAN
                k4 = min(max(int(k if isinstance(k, int) else k[4]), 0), 1)
                assert bool((table[4] == k4).all().item()) and int(settle_all[4]) == k4, "the robot at rest left the degenerate box of its constant rows"
    # the last outside sample exactly at kq: the bound is the midpoint between sample kq and the extreme of everything after it, the
    # resting value included, where sample kq lies beyond that extreme
    S = _samples(full, batch, n, 1)                              # [n, 4, 1, span]
    after_max = S.flip(3).cummax(dim=3).values.flip(3)[..., 1:]  # [.., t] = max S[t + 1:]
    after_min = S.flip(3).cummin(dim=3).values.flip(3)[..., 1:]
    kq = np.clip(_starts(rng, lens), 0, np.maximum(lens - 2, 0)).astype(np.int32)
    kt = torch.from_numpy(kq).to(DEV)
    at = kt.long()[:, None, None, None].expand(n, 4, 1, 1)
    here, top, bottom = S.gather(3, at)[..., 0], after_max.gather(3, at)[..., 0], after_min.gather(3, at)[..., 0]
    above, below = (here > top) & planned[:, None, None], (here < bottom) & planned[:, None, None]
    inf = torch.full_like(here, float("inf"))
    hi = torch.where(above, 0.5 * (here + top), inf)
    lo = torch.where(below & ~above, 0.5 * (here + bottom), -inf)
    above &= (hi < here) & (hi >= top)                           # the midpoint separates the two
    below &= ~above & (lo > here) & (lo <= bottom)
    hi, lo = torch.where(above, hi, inf), torch.where(below, lo, -inf)
    marked = above | below
    assert int(marked.sum().item()) > 0.1 * int(planned.sum().item()) * 4
    k_of = kt[:, None, None].expand(n, 4, 1)
    for start, horizon, answer in ((kq, 1, "not yet"), (kq, 2, "index"), (kq, 1 << 30, "index"), (np.maximum(kq - 5, 0).astype(np.int32), 1 << 30, "index"),
                                   (0, 1 << 30, "index")):
        table = _assert_settle(ltp, batch, full, start, horizon, 0, n, lo, hi, f"the last outside sample at k, H {horizon}", masks=("qvaj",))["qvaj"][0]
        want = torch.full_like(table, sc.SETTLE_NOT_YET) if answer == "not yet" else k_of + 1
        assert torch.equal(table[marked], want[marked])
    # ... and exactly at reach - 1: from k = kq - 5 the horizon H = 6 ends on it (NOT_YET), H + 1 = 7 reaches the sample behind it
    far = torch.from_numpy(kq >= 5).to(DEV)[:, None, None] & marked
    assert int(far.sum().item()) > 0
    back = (kq - 5).astype(np.int32)
    table = _assert_settle(ltp, batch, full, back, 6, 0, n, lo, hi, "the last outside sample at reach - 1", masks=("qvaj", "q", "aj"))["qvaj"][0]
    assert bool((table[far] == sc.SETTLE_NOT_YET).all().item())
    table = _assert_settle(ltp, batch, full, back, 7, 0, n, lo, hi, "the last outside sample at reach - 2", masks=("qvaj", "q", "aj"))["qvaj"][0]
    assert torch.equal(table[far], (k_of + 1)[far])
    # a v, a, j box that excludes 0: past the end the resting state is outside (NOT_YET); a horizon that ends inside the trajectory
    # gives an index (the box holds every real sample: k). The q box holds everything.
    wide_lo, wide_hi = torch.nan_to_num(mn - 1.0, nan=0.0), torch.nan_to_num(mx + 1.0, nan=0.0)
    some_lo = wide_lo.clone()
    some_lo[:, 1:] = 1e-9                                        # v, a, j: [1e-9, max + 1] excludes 0 from below, holds the positive samples
    moving = torch.from_numpy(lens > 8).to(DEV)
    for k, horizon, reaches in (((lens - 1).astype(np.int32), 1, False), ((lens - 1).astype(np.int32), 2, True), (lens.astype(np.int32), 1, True),
                                ((lens + 5).astype(np.int32), 64, True), (0, 1 << 30, True), (0, 4, False), ((lens - 6).astype(np.int32), 6, False)):
        got = _assert_settle(ltp, batch, full, k, horizon, 0, n, some_lo, wide_hi, "a box that excludes 0", masks=("qvaj", "vaj", "q"))
        table = got["qvaj"][0]
        kk = torch.full((n,), k, device=DEV) if isinstance(k, int) else torch.from_numpy(k).to(DEV)
        kk = torch.minimum(kk.clamp(min=0), L)
        assert torch.equal(table[planned][:, 0, 0], kk[planned]), "q left a box that holds every position"
        if reaches:
            assert bool((table[planned][:, 1:] == sc.SETTLE_NOT_YET).all().item()), "v, a, j rest at 0, outside the box"
            assert bool((got["qvaj"][1][planned] == sc.SETTLE_NOT_YET).all().item())
        else:
            assert bool((table[moving][:, 1:] != sc.SETTLE_NOT_YET).any().item()), "no horizon that ends inside the trajectory ends inside the box"
    # a q box that excludes the last position: never settled, from any start, over any horizon that reaches the end
    last = sc._gather(full, batch.offsets[:n].long(), L.long(), 1, (L.long() - 1).clamp(min=0)[:, None])[..., 0]
    for k, horizon in ((0, 1 << 30), ((lens + 2).astype(np.int32), 3), ((lens - 1).astype(np.int32), 1)):
        got = _assert_settle(ltp, batch, full, k, horizon, 0, n, torch.full_like(last, -float("inf")), last - 1e-6, "a q box below the last position", masks=("q",))
        assert bool((got["q"][0][planned] == sc.SETTLE_NOT_YET).all().item())


def test_settling_on_either_side_of_a_run_boundary():
    """Around a run boundary taken from the records' switching times — b = floor(t_x / Ts) + {0, 1, 2}, the cut points of the run
    walk — in the lanes where sample b - 1 exceeds the maximum of everything after it, the resting value included, the bound is set to
    the midpoint between the two: the answer is exactly b, the first sample of a run for some offsets and one inside it for others."""
    import torch
    n = 300
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    L = batch.traj_len.long()
    S = _samples(full, batch, n, dof)                            # [n, 4, dof, span]
    after_max = S.flip(3).cummax(dim=3).values.flip(3)           # [.., t] = max S[t:]
    ts = torch.from_numpy(t_scaled).to(DEV)                      # [n, dof, 7]
    hit = total = 0
    for x_switch in (0, 2, 4, 6):
        for offset in (0, 1, 2):
            b = (torch.floor(ts[:, :, x_switch] / H.TS).long() + offset).clamp(min=1)
            b = torch.minimum(b, L.clamp(min=1)[:, None])[:, None, :, None].expand(n, 4, dof, 1)               # [n, 4, dof, 1]: b - 1 is a real sample
            before, rest_max = S.gather(3, b - 1)[..., 0], after_max.gather(3, b)[..., 0]
            falls = (before > rest_max) & (L > 0)[:, None, None]
            hi = torch.where(falls, 0.5 * (before + rest_max), torch.full_like(before, float("inf")))
            falls &= (hi < before) & (hi >= rest_max)                                                           # the midpoint separates the two
            hi = torch.where(falls, hi, torch.full_like(before, float("inf")))
            lo = torch.full_like(hi, -float("inf"))
            got = _assert_settle(ltp, batch, full, 0, 1 << 30, 0, n, lo, hi, f"run boundary switch {x_switch} + {offset}", masks=("qvaj",))
            table = got["qvaj"][0]
            assert bool((table[falls] == b[..., 0][falls]).all().item())
            hit, total = hit + int(falls.sum().item()), total + falls.numel()
    print(f"run boundaries: {hit} of {total} (lane, boundary) pairs lie above everything behind their boundary and settle exactly there")
    assert hit > 0.05 * total


@pytest.mark.parametrize("name", rc.BATCHES)
def test_short_runs(oracle_mod, name):
    """The run-census batches (rows of 1-153 samples, runs of 1-3 samples, collided switch indices, switching times on exact
    multiples of the sample time): a uniform k swept over 0 .. 4 and per-plan starts, short horizons and the whole plan, both
    families of boxes."""
    R = _rows(oracle_mod, name)
    ltp, batch, n, cen, dof = R["ltp"], R["batch"], R["n"], R["cen"], R["dof"]
    lens = R["rec"]["traj_len"]
    mn, mx = sc.row_ranges(R["full"], batch.offsets, batch.traj_len, dof, 0, n)
    rng = np.random.default_rng(17)
    describe = lambda plans: rc.describe(cen, plans)
    for lo, hi in (sc.end_boxes(R["full"], batch.offsets, batch.traj_len, dof, seed=3), sc.fraction_boxes(mn, mx, seed=4)):
        for horizon in (1, 3, 1 << 30):
            for k in list(range(5)) + [_starts(rng, lens)]:
                _assert_settle(ltp, batch, R["full"], k, horizon, 0, n, lo, hi, f"{name} k {'per plan' if not isinstance(k, int) else k}", masks=("qvaj",),
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
    mn, mx = sc.row_ranges(full, batch.offsets, batch.traj_len, dof, 0, n)
    rng = np.random.default_rng(5)
    for lo, hi in (sc.end_boxes(full, batch.offsets, batch.traj_len, dof, seed=11), sc.fraction_boxes(mn, mx, seed=11)):
        for horizon in (64, 1 << 30):
            for k in (0, _starts(rng, lens)):
                _assert_settle(ltp, batch, full, k, horizon, 0, n, lo, hi, f"soft dense H {horizon}", masks=("qvaj", "q"))
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
    mn, mx = sc.row_ranges(full, batch.offsets, batch.traj_len, dof, 0, n)
    rng = np.random.default_rng(21)
    first, count = H.odd_range(n, dof)
    for lo, hi in (sc.end_boxes(full, batch.offsets, batch.traj_len, dof, seed=13), sc.fraction_boxes(mn, mx, seed=13)):
        for horizon in (64, 1 << 30):
            k = _starts(rng, lens)
            _assert_settle(ltp, batch, full, k, horizon, 0, n, lo, hi, f"{kind} H {horizon}", masks=("qvaj",))
            _assert_settle(ltp, batch, full, k, horizon, first, count, lo[first:first + count], hi[first:first + count], f"{kind} H {horizon} sub-range",
                           masks=("qvaj", "va"))
    if kind == "limit_sets":
        _, lim = limit_set("panda")
        sets = {key: np.array([[f * x if key in ("v_max", "a_max", "j_max") else x for x in lim[key]] for f in (1.0, 0.5, 0.25)]) for key in lim}
        d_lo, d_hi = sc.default_boxes(n, sets, DEV, set_index=batch.limit_set)
        assert float((d_hi[0, 1] / d_hi[1, 1]).min()) == 2.0     # plan 0 reads set 0, plan 1 set 1
        for horizon in (240, 1 << 30):
            default = ltp.settle(batch, 0, n, 0, horizon, arrays="qvaj")
            explicit = _assert_settle(ltp, batch, full, 0, horizon, 0, n, d_lo, d_hi, "limit sets, explicit per-plan boxes", masks=("qvaj",))["qvaj"][0]
            torch.cuda.synchronize()
            assert torch.equal(default, explicit), "the default boxes are not the plan's own set"
            assert int((default[:, 1:3] > 0).sum().item()) > 0


def test_the_readers_agree():
    """With the same boxes, k, H and mask: settle == k exactly where firstExit == LTP_EXIT_NONE; where firstExit >= 0, settle is
    LTP_SETTLE_NOT_YET or greater than firstExit; a plan without a trajectory is LTP_EXIT_NO_PLAN in both. With H = 1 the two tables
    map onto each other: none <-> k, an exit (at k) <-> not yet."""
    import torch
    n = 1000
    ltp, dof, lim, qs, batch, full, lens, mn, mx, ends = _batch("panda", n)
    rng = np.random.default_rng(41)
    L = batch.traj_len
    seen_none = seen_left = 0
    for lo, hi in (ends, sc.fraction_boxes(mn, mx, seed=9)):
        for horizon in (1, 2, 64, 240, 1 << 30):
            for k in (0, _starts(rng, lens)):
                for arrays in ("qvaj", "qv", "a"):
                    mask = _mask_of(arrays)
                    start = k if isinstance(k, int) else torch.from_numpy(k).to(DEV)
                    kk = torch.full((n,), k, device=DEV) if isinstance(k, int) else start
                    kk = torch.minimum(kk.clamp(min=0), L)[:, None, None]
                    settle = ltp.settle(batch, 0, n, start, horizon, arrays=arrays, lo=_sides(mask, lo), hi=_sides(mask, hi))
                    exits = ltp.firstExit(batch, 0, n, start, horizon, arrays=arrays, lo=_sides(mask, lo), hi=_sides(mask, hi))
                    torch.cuda.synchronize()
                    none, left = exits == EXIT_NONE, exits >= 0
                    assert torch.equal(settle == kk, none), (horizon, arrays)
                    assert bool(((settle == sc.SETTLE_NOT_YET) | (settle > exits))[left].all().item())
                    assert torch.equal(settle == sc.EXIT_NO_PLAN, exits == sc.EXIT_NO_PLAN) and torch.equal(none | left, settle != sc.EXIT_NO_PLAN)
                    seen_none, seen_left = seen_none + int(none.sum().item()), seen_left + int(left.sum().item())
                    if horizon == 1:
                        assert torch.equal(settle == sc.SETTLE_NOT_YET, left) and bool((exits[left] == kk.expand_as(exits)[left]).all().item())
                        mapped = torch.where(left, torch.full_like(exits, sc.SETTLE_NOT_YET), torch.where(none, kk.expand_as(exits).int(), exits))
                        assert torch.equal(settle, mapped)
    assert seen_none > 0 and seen_left > 0


def test_arrival():
    """arrival is the scan's maximum over the joints: for a q tolerance around the goal, and for a q plus a v tolerance; with a
    tolerance per joint; from k = 0 and from per-plan starts."""
    import torch
    n = 1000
    ltp, dof, lim, qs, batch, full, lens, mn, mx, ends = _batch("panda", n)
    goal = torch.from_numpy(qs[0]).to(DEV)
    rng = np.random.default_rng(43)
    per_joint = torch.from_numpy(rng.uniform(1e-4, 5e-2, dof)).to(DEV)
    inf = torch.full((n, 4, dof), float("inf"), dtype=torch.float64, device=DEV)
    for q_tol in (1e-3, per_joint):
        for v_tol in (None, 0.01, 0.5):
            for k in (0, torch.from_numpy(_starts(rng, lens)).to(DEV)):
                got = ltp.arrival(batch, 0, n, k, goal, q_tol, v_tol=v_tol)
                torch.cuda.synchronize()
                lo, hi = -inf.clone(), inf.clone()
                lo[:, 0], hi[:, 0] = goal - q_tol, goal + q_tol
                if v_tol is not None:
                    lo[:, 1], hi[:, 1] = -v_tol, v_tol
                table, want = sc.expected(full, batch.offsets, batch.traj_len, k, sc.WHOLE, dof, 0, n, lo, hi, mask=1 if v_tol is None else 3)
                assert got.shape == (n,) and got.dtype == torch.int32 and torch.equal(got, want)
                # the maximum over the joints, written out
                planned = batch.traj_len > 0
                arrived = planned & (table >= 0).flatten(1).all(dim=1)
                assert torch.equal(got[arrived], table[arrived].flatten(1).max(dim=1).values)
                # (the sampled rows end within the sampler's discretisation of the goal, not on it: a 1 mrad tolerance admits few plans)
                assert int(arrived.sum().item()) > 0 and int(got[REJECTED]) == sc.EXIT_NO_PLAN
    first, count = 5, 403
    part = ltp.arrival(batch, first, count, 0, goal[first:first + count].contiguous(), 1e-3, v_tol=0.01)
    whole = ltp.arrival(batch, 0, n, 0, goal, 1e-3, v_tol=0.01)
    one_goal = ltp.arrival(batch, 0, n, 0, goal[0].contiguous(), 1e-3)
    torch.cuda.synchronize()
    assert torch.equal(part, whole[first:first + count]) and int(one_goal[0]) == int(ltp.arrival(batch, 0, n, 0, goal, 1e-3)[0])


def test_refusals_and_bounds():
    """Each refusal of the device entry is LTP_ERR_INVALID_ARGUMENT, its text names the reason, and the guard-filled buffer and
    settle_all it was given keep their pattern; a geometry change after planning is refused in ltp_state_at_batch's words; a call
    whose buffer is exactly ltp_settle_elements long writes nothing beside it. The wrappers refuse a bad mask, horizon or box
    (ValueError) and the host entry its own arguments (LtpError) before any launch."""
    import torch
    from longtermplanner_amd import _abi
    from longtermplanner_amd._abi import LtpError
    n = 64
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    lib, O = ltp._lib, _abi.SettleOpts
    P = C.c_void_p * 4
    need = n * 4 * dof
    assert lib.ltp_settle_elements(ltp._h, n, 15) == need and lib.ltp_settle_elements(ltp._h, n, 5) == need // 2
    assert lib.ltp_settle_elements(ltp._h, n, 0) == 0 and lib.ltp_settle_elements(ltp._h, n, 16) == 0 and lib.ltp_settle_elements(ltp._h, 0, 15) == 0
    buf = torch.full((need + 64,), GUARD, dtype=torch.int32, device=DEV)
    out = buf[32:32 + need]
    all_buf = torch.full((n,), GUARD, dtype=torch.int32, device=DEV)
    box = torch.zeros((dof,), dtype=torch.float64, device=DEV) + 0.5
    call = H.reader_call(lib.ltp_settle_batch, ltp, batch, n, out, capacity=need)
    good = dict(size=C.sizeof(O), arrays=15, horizon=240, box_joint_stride=1)
    status = batch.status.clone()
    rc_, msg = call(O(**good))
    assert rc_ == 0, msg
    torch.cuda.synchronize()
    want = ltp.settle(batch, 0, n, 0, 240, arrays="qvaj")
    torch.cuda.synchronize()
    assert torch.equal(out, want.reshape(-1)), "settle_all = NULL changes the table"
    assert bool((buf[:32] == GUARD).all().item()) and bool((buf[32 + need:] == GUARD).all().item()), "ints beside the call's elements were written"
    assert torch.equal(batch.status, status)
    buf.fill_(GUARD)
    good = dict(good, settle_all=all_buf.data_ptr())
    refusals = [(dict(q=False), {}, "null"), (dict(r=False), {}, "null"), (dict(out_ptr=0), {}, "null"), (dict(capacity=need - 1), {}, "ltp_settle_elements"),
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
    assert rc_ == INVALID and "ltp_settle_elements" in msg
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
            ltp.settle(batch, 0, n, 0, args.pop("horizon"), out=view, all=all_buf, **args)
    host_box = np.full(dof, 0.5)
    for kw in (dict(arrays="x"), dict(horizon=0), dict(arrays="q", hi={"j": host_box}), dict(lo={"q": host_box[:3]}),
               dict(arrays="a", lo={"a": host_box}, hi={"a": np.zeros((n, dof))})):
        args = dict(dict(horizon=240, arrays="qvaj"), **kw)
        with pytest.raises(ValueError):
            ltp.planSettleHost(*qs, 0, args.pop("horizon"), **args)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    host_out = np.full(need, GUARD, dtype=np.int32)
    boxes = (dp * 4)(None, host_box.ctypes.data_as(dp), None, None)
    for arrays, horizon, per_plan, his, text in ((0, 240, 0, None, "arrays"), (16, 240, 0, None, "arrays"), (15, 0, 0, None, "horizon"),
                                                 (15, (1 << 30) + 1, 0, None, "horizon"), (15, 240, 2, None, "box_per_plan"), (1, 240, 0, boxes, "not selected")):
        rc_ = lib.ltp_plan_settle_host(ltp._h, n, *[x.ctypes.data_as(dp) for x in qs], None, 0, horizon, arrays, None, his, per_plan, None,
                                       host_out.ctypes.data_as(ip), None)
        assert rc_ == INVALID and text in (lib.ltp_last_error(ltp._h) or b"").decode(), (arrays, horizon, per_plan)
    assert (host_out == GUARD).all()
    with pytest.raises(LtpError):
        ltp._check(lib.ltp_plan_settle_host(ltp._h, n, *[x.ctypes.data_as(dp) for x in qs], None, 0, 240, 15, None, None, 0, None, None, None))
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all().item()), "a refused call wrote to the buffer"
    assert bool((all_buf == GUARD).all().item()), "a refused call wrote to settle_all"
    assert call(O(**good))[0] == 0
    torch.cuda.synchronize()
    assert torch.equal(all_buf, sc.fold_all(out.view(n, 4, dof)).int())


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
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size() || std::fread(k.data(), sizeof(int), k.size(), f) != k.size() ||
      std::fread(v_hi.data(), sizeof(double), v_hi.size(), f) != v_hi.size() || std::fread(a_lo.data(), sizeof(double), a_lo.size(), f) != a_lo.size()) return 2;
  std::fclose(f);
  std::vector<int> settle, all;
  BatchTrajectory b;
  const double* los[4] = {nullptr, nullptr, a_lo.data(), nullptr};
  const double* his[4] = {nullptr, v_hi.data(), nullptr, nullptr};
  const long long ok = ltp.planSettleBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, 500,
                                           LTP_ENV_Q | LTP_ENV_V | LTP_ENV_A, los, his, true, settle, &all, &b);
  int refused = 0;
  for (int arrays : {0, 16}) {
    try {
      std::vector<int> e2;
      ltp.planSettleBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, 500, arrays, nullptr, nullptr, false, e2);
    } catch (const std::exception&) { ++refused; }
  }
  for (int horizon : {0, -1}) {
    try {
      std::vector<int> e2;
      ltp.planSettleBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, horizon, LTP_ENV_Q, nullptr, nullptr, false, e2);
    } catch (const std::exception&) { ++refused; }
  }
  try {
    std::vector<int> e2;
    ltp.planSettleBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, 500, LTP_ENV_Q, nullptr, his, true, e2);
  } catch (const std::exception&) { ++refused; }
  if (refused != 5) return 3;
  FILE* o = std::fopen(argv[2], "wb");
  std::fwrite(settle.data(), sizeof(int), settle.size(), o);
  std::fwrite(all.data(), sizeof(int), all.size(), o);
  std::fwrite(b.status.data(), sizeof(int), b.status.size(), o);
  std::fclose(o);
  std::printf("%lld ok, %zu ints\n", ok, settle.size());
  return 0;
}
'''


def test_host_and_dropin_paths(tmp_path):
    """planSettleHost equals the device call int for int (boxes [dof] and [n, dof], with and without settle_all) and its status
    carries END_LIMIT like planBatchHost(sample=False); a small C++ program gives the same bytes through
    LongTermPlanner::planSettleBatch."""
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
    dev, dev_all = ltp.settle(batch, 0, n, torch.from_numpy(k).to(DEV), 500, arrays="qva", lo={"a": torch.from_numpy(a_lo).to(DEV)},
                              hi={"v": torch.from_numpy(v_hi).to(DEV)}, all=True)
    dev, dev_all = dev.cpu().numpy(), dev_all.cpu().numpy()
    kk = np.minimum(np.maximum(k, 0), lens)[:, None, None]
    assert (dev > kk).sum() > 0 and (dev == kk).sum() > 0
    assert not (batch.status.cpu().numpy()[3] & 8), "the device call forms no end-limit verdict"
    rec, table, settle_all = ltp.planSettleHost(*qs, k, 500, arrays=7, lo={"a": a_lo}, hi={"v": v_hi}, all=True)
    assert table.shape == (n, 3, dof) and table.dtype == np.int32
    assert np.array_equal(table, dev) and np.array_equal(settle_all, dev_all)
    plain = ltp.planBatchHost(*qs, sample=False)
    assert np.array_equal(rec["status"], plain["status"]) and (rec["status"][3] & 8) and np.array_equal(rec["traj_len"], lens)
    # a uniform k, one box per joint, no settle_all
    one = 0.5 * np.asarray(lim["v_max"])
    _, table_u = ltp.planSettleHost(*qs, 5, 1 << 30, arrays="v", lo={"v": -one}, hi={"v": one})
    dev_u = ltp.settle(batch, 0, n, 5, 1 << 30, arrays="v", lo={"v": torch.from_numpy(-one).to(DEV)}, hi={"v": torch.from_numpy(one).to(DEV)})
    assert table_u.shape == (n, 1, dof) and np.array_equal(table_u, dev_u.cpu().numpy())

    raw = H.run_dropin(tmp_path, "settle", DROPIN, np.concatenate([x.reshape(-1) for x in qs]).astype(np.float64).tobytes()
                       + k.astype(np.int32).tobytes() + v_hi.tobytes() + a_lo.tobytes())
    assert raw == table.tobytes() + settle_all.tobytes() + rec["status"].astype(np.int32).tobytes()


@pytest.mark.parametrize("with_all", [False, True])
def test_graph_capture_and_replay_with_new_starts_and_new_boxes(with_all):
    """The call allocates nothing: captured on one stream (one kernel node, and one fill-kernel node before it with settle_all) and
    replayed after first_sample AND the box arrays were rewritten in place, it gives what a direct call gives for the new starts
    and boxes, and what the exhaustive scan gives — twice."""
    import torch
    n = 1000
    ltp, dof, lim, qs, batch, full, lens, mn, mx, ends = _batch("panda", n)
    rng = np.random.default_rng(77)
    ka, kb, kc = (_starts(rng, lens) for _ in range(3))
    assert np.count_nonzero(ka != kb) > 0.5 * n
    boxes = [sc.fraction_boxes(mn, mx, seed=21), sc.end_boxes(full, batch.offsets, batch.traj_len, dof, seed=22),
             sc.end_boxes(full, batch.offsets, batch.traj_len, dof, seed=23)]
    k = torch.from_numpy(ka).to(DEV)
    lo, hi = boxes[0][0].clone(), boxes[0][1].clone()
    mask = 15
    lo_by = {a: lo[:, x].contiguous() for x, a in enumerate(LETTERS)}
    hi_by = {a: hi[:, x].contiguous() for x, a in enumerate(LETTERS)}
    out = torch.zeros((n, 4, dof), dtype=torch.int32, device=DEV)
    settle_all = torch.zeros((n,), dtype=torch.int32, device=DEV)
    graph = H.capture(lambda: ltp.settle(batch, 0, n, k, 240, arrays=mask, lo=lo_by, hi=hi_by, all=settle_all if with_all else False, out=out))
    for k_new, (lo_new, hi_new) in ((kb, boxes[1]), (kc, boxes[2])):
        k.copy_(torch.from_numpy(k_new))
        for x, a in enumerate(LETTERS):
            lo_by[a].copy_(lo_new[:, x])
            hi_by[a].copy_(hi_new[:, x])
        out.zero_()
        settle_all.fill_(12345)
        graph.replay()
        torch.cuda.synchronize()
        direct = ltp.settle(batch, 0, n, k, 240, arrays=mask, lo=lo_by, hi=hi_by, all=with_all)
        torch.cuda.synchronize()
        want, want_all = sc.expected(full, batch.offsets, batch.traj_len, k, 240, dof, 0, n, lo_new, hi_new)
        assert torch.equal(out, want)
        if with_all:
            assert torch.equal(direct[0], out) and torch.equal(direct[1], settle_all) and torch.equal(settle_all, want_all)
        else:
            assert torch.equal(direct, out) and bool((settle_all == 12345).all().item())
