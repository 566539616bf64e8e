"""Settling (ltp_settle_batch, include/ltp_hip.h) on the GPU: per plan, selected array of q, v, a, j and joint the trajectory sample
from which the array is inside a box and stays inside for the rest of [k, k + H), compared for EQUALITY with the exhaustive scan of
the full-row sampler's rows for the same batch (tests/box_checker.py, itself pinned to a plain loop by tests/test_settle_cpu.py)
in every (plan, array, joint): no case is excused. Two families of boxes go to the device: boxes around the value each row comes
to rest at (box_checker.end_boxes: almost every lane settles at an index inside its plan) and boxes at seeded fractions of each
row's own range (box_checker.fraction_boxes: q mostly rests outside, LTP_SETTLE_NOT_YET). The batch, the assert against the scan
and the tests first exits share are tests/box_helpers.py's."""
import numpy as np
import pytest

import box_checker as sc
import box_helpers as B
import horizon_helpers as H
import run_census as rc
from box_helpers import HORIZONS, REJECTED, _mask_of, _samples, _sides, _starts
from horizon_helpers import DEV

pytestmark = pytest.mark.gpu


def _batch(name, n, pow_rule="libm"):
    return B._batch(name, n, pow_rule, ends=True)


def _assert_settle(*args, **kw):
    return B.assert_reads(B.SETTLE, *args, **kw)


def _ends_and_fractions(end_seed, fraction_seed):
    """The box families of a shared test: boxes around every row's resting value, and fraction boxes of the rows' own ranges."""
    return lambda full, batch, dof, mn, mx: [sc.end_boxes(full, batch.offsets, batch.traj_len, dof, seed=end_seed),
                                             sc.fraction_boxes(mn, mx, seed=fraction_seed)]


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
    B.short_runs(B.SETTLE, oracle_mod, name, _ends_and_fractions(3, 4))


def test_jerk_dominated_runs(oracle_mod):
    """The jerk-dominated soft set of tests/branch_census.py (every planner case, modified jerk profiles, fallback records): the
    first 200 plans of the dense batch, from k = 0 and per-plan starts."""
    B.jerk_dominated_runs(B.SETTLE, oracle_mod, _ends_and_fractions(11, 11))


@pytest.mark.parametrize("kind", ["retimed", "limit_sets", "matlab", "stop"])
def test_other_batch_kinds(kind):
    """A retimed batch, a batch with three bound limit sets, MATLAB semantics (full rows from the walk sampler) and a stop batch: each
    against the exhaustive scan of its own rows, whole and a sub-range. Under limit sets the default boxes equal explicit per-plan
    boxes built from each plan's own set, bit for bit in the ints, and some v or a lane settles behind sample 0."""
    B.other_batch_kinds(B.SETTLE, kind, _ends_and_fractions(13, 13), moved=lambda table: table > 0)


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
                    none, left = exits == sc.EXIT_NONE, exits >= 0
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
                table, want = sc.expected_settle(full, batch.offsets, batch.traj_len, k, sc.WHOLE, dof, 0, n, lo, hi, mask=1 if v_tol is None else 3)
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
    B.refusals_and_bounds(B.SETTLE, more_host_refusals=lambda n, dof, host_box: (
        dict(arrays="a", lo={"a": host_box}, hi={"a": np.zeros((n, dof))}),))


def _holds_both(dev, k, lens):
    kk = np.minimum(np.maximum(k, 0), lens)[:, None, None]
    return (dev > kk).sum() > 0 and (dev == kk).sum() > 0


def test_host_and_dropin_paths(tmp_path):
    """planSettleHost equals the device call int for int (boxes [dof] and [n, dof], with and without settle_all) and its status
    carries END_LIMIT like planBatchHost(sample=False); a small C++ program gives the same bytes through
    LongTermPlanner::planSettleBatch."""
    B.host_and_dropin_paths(B.SETTLE, tmp_path, both_answers=_holds_both)


@pytest.mark.parametrize("with_all", [False, True])
def test_graph_capture_and_replay_with_new_starts_and_new_boxes(with_all):
    """The call allocates nothing: captured on one stream (one kernel node, and one fill-kernel node before it with settle_all) and
    replayed after first_sample AND the box arrays were rewritten in place, it gives what a direct call gives for the new starts
    and boxes, and what the exhaustive scan gives — twice."""
    B.graph_capture_and_replay(B.SETTLE, with_all, lambda full, batch, dof, mn, mx: [
        sc.fraction_boxes(mn, mx, seed=21), sc.end_boxes(full, batch.offsets, batch.traj_len, dof, seed=22),
        sc.end_boxes(full, batch.offsets, batch.traj_len, dof, seed=23)])
