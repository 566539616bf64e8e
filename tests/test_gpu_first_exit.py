"""First exits (ltp_first_exit_batch, include/ltp_hip.h) on the GPU: per plan, selected array of q, v, a, j and joint the smallest
trajectory sample t in [k, k + H) that lies outside a box, compared for EQUALITY with the exhaustive scan of the full-row sampler's
rows for the same batch (tests/box_checker.py, itself pinned to a plain loop by tests/test_first_exit_cpu.py) in every (plan,
array, joint): no case is excused. The boxes sit at seeded fractions of each row's own range, so almost every lane has an exit and
none sits on a sample by construction. The batch, the assert against the scan and the tests settling shares are
tests/box_helpers.py's."""
import numpy as np
import pytest

import box_checker as fc
import box_helpers as B
import horizon_helpers as H
import run_census as rc
from box_helpers import HORIZONS, LETTERS, REJECTED, _batch, _mask_of, _starts
from envelope_checker import selected
from horizon_helpers import DEV

pytestmark = pytest.mark.gpu


def _assert_exits(*args, **kw):
    return B.assert_reads(B.EXITS, *args, **kw)


def _fractions(*seeds):
    """The box families of a shared test: fraction boxes of the rows' own ranges, one per seed."""
    return lambda full, batch, dof, mn, mx: [fc.fraction_boxes(mn, mx, seed=s) for s in seeds]


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
    B.short_runs(B.EXITS, oracle_mod, name, _fractions(3, 4))


def test_jerk_dominated_runs(oracle_mod):
    """The jerk-dominated soft set of tests/branch_census.py (every planner case, modified jerk profiles, fallback records): the
    first 200 plans of the dense batch, from k = 0 and per-plan starts."""
    B.jerk_dominated_runs(B.EXITS, oracle_mod, _fractions(11))


@pytest.mark.parametrize("kind", ["retimed", "limit_sets", "matlab", "stop"])
def test_other_batch_kinds(kind):
    """A retimed batch, a batch with three bound limit sets, MATLAB semantics (full rows from the walk sampler) and a stop batch: each
    against the exhaustive scan of its own rows, whole and a sub-range. Under limit sets the default boxes equal explicit per-plan
    boxes built from each plan's own set, bit for bit in the ints, and some v or a lane has an exit."""
    B.other_batch_kinds(B.EXITS, kind, _fractions(13), moved=lambda table: table >= 0)


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
            planes = selected(_mask_of(arrays))
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
    """Each refusal of the device entry is LTP_ERR_INVALID_ARGUMENT, its text names the reason, and the guard-filled buffer and
    first_any it was given keep their pattern; a geometry change after planning is refused in ltp_state_at_batch's words; a call
    whose buffer is exactly ltp_first_exit_elements long writes nothing beside it. The wrappers refuse a bad mask, horizon or box
    (ValueError) and the host entry its own arguments (LtpError) before any launch."""
    B.refusals_and_bounds(B.EXITS)


def test_host_and_dropin_paths(tmp_path):
    """planFirstExitHost equals the device call int for int (boxes [dof] and [n, dof], with and without first_any) and its status
    carries END_LIMIT like planBatchHost(sample=False); a small C++ program gives the same bytes through
    LongTermPlanner::planFirstExitBatch."""
    B.host_and_dropin_paths(B.EXITS, tmp_path, both_answers=lambda dev, k, lens: (dev >= 0).sum() > 0 and (dev == fc.EXIT_NONE).sum() > 0)


@pytest.mark.parametrize("with_any", [False, True])
def test_graph_capture_and_replay_with_new_starts_and_new_boxes(with_any):
    """The call allocates nothing: captured on one stream (one kernel node, and one fill-kernel node before it with first_any) and
    replayed after first_sample AND the box arrays were rewritten in place, it gives what a direct call gives for the new starts
    and boxes, and what the exhaustive scan gives — twice."""
    B.graph_capture_and_replay(B.EXITS, with_any, _fractions(21, 22, 23))
