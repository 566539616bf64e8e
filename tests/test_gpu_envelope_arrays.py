"""Horizon envelopes of q, v, a and j (ltp_envelope_knots_arrays_batch, include/ltp_hip.h) on the GPU: per plan, selected array and
joint {min, max} over the trajectory samples between the edges k + g[w] and k + g[w + 1] of a knot grid. Compared with the reduced
rows of the full-row sampler for the same batch (tests/envelope_checker.py, itself pinned to a plain loop by
tests/test_envelope_arrays_cpu.py): q and v under the project's acceptance rule for an analytic envelope form, a and j for equality;
with the q-only call and among the masks bit for bit; with the knots call; at the end of a plan; on the run-census batches, on
other batch kinds, through the host and drop-in paths and under graph capture. The bodies it shares with
tests/test_gpu_envelope_knots.py are tests/envelope_helpers.py's.

Contract-breaking device grids are pinned on the host only (tests/cpp/envelope_knots_ranges_test.cc): no test here feeds one."""
import numpy as np
import pytest

import envelope_checker as ac
import envelope_helpers as E
import horizon_helpers as H
import run_census as rc
from envelope_helpers import ARRAYS, REJECTED, _batch, _starts
from horizon_helpers import DEV
from horizon_helpers import grid_tensor as _grid

pytestmark = pytest.mark.gpu

MASKS = (15, 2, 12, 1)


@pytest.mark.parametrize("name,n,pow_rule", [("panda", 1500, "libm"), ("panda", 1500, "exact"), ("ref", 1000, "libm"), ("ref30", 200, "libm")])
def test_envelopes_against_reduced_rows(name, n, pow_rule):
    """Every pair of every mask against the minimum and maximum of the samples sampleBatch wrote for its interval (past the end: the
    last position for q, 0 for v, a, j): q and v by the acceptance rule of the analytic form (NaN pattern identical, inside the
    samples, |d| <= 1e-12; q at least 0.999 bit-identical, the share of v printed), a and j equal. The whole batch (with its
    rejected plan) and a slice with first > 0 whose count * dof is no multiple of 64; starts per plan from [-5, traj_len + 40];
    both `closed` modes; `valid` against its formula."""
    E.reduced_rows(ARRAYS, name, n, pow_rule, ("mpc", "duplicates", "n65", "max"), masks=MASKS)


@pytest.mark.parametrize("name", rc.BATCHES)
def test_the_smallest_shapes(oracle_mod, name):
    """The run-census batches (rows of 1-153 samples, one-sample runs, collided switch indices, switching times on exact multiples
    of the sample time): unit, two-sample and duplicate-holding grids, both modes, a uniform k swept over 0 .. 8 and per-plan
    starts, all four arrays in one call."""
    E.smallest_shapes(ARRAYS, oracle_mod, name)


def _identity_batch(kind, n):
    """(ltp, dof, batch, traj_len) of test_mask_identities: _batch's for a limit-set name; "ref-dof1": one joint; "panda-matlab":
    MATLAB semantics. One plan is rejected in each."""
    if kind in ("panda", "ref"):
        ltp, dof, lim, qs, batch, full, lens = _batch(kind, n)
        return ltp, dof, batch, lens
    if kind == "ref-dof1":
        from longtermplanner_amd import LongTermPlanner, limit_set
        dof, lim = limit_set("ref", dof=1)
        ltp = LongTermPlanner(dof, H.TS, device=0, **lim)
    else:
        ltp, dof, lim = H.planner("panda", semantics="matlab")
    qs = H.queries(lim, n)
    qs[2][REJECTED, 0] = 99.0
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    lens = batch.traj_len.cpu().numpy()
    assert lens[REJECTED] == 0 and np.mean(lens > 0) >= 0.9
    return ltp, dof, batch, lens


def _edge_starts(rng, lens):
    """_starts with every fourth plan at -3, the next at traj_len and the one after it at traj_len + 7."""
    L = lens.astype(np.int64)
    i = np.arange(len(L)) % 4
    return np.where(i == 0, -3, np.where(i == 1, L, np.where(i == 2, L + 7, _starts(rng, lens)))).astype(np.int32)


def _assert_mask_identities(ltp, batch, f, c, k, g, closed, what):
    """Over plans [f, f + c) from the starts k (a tensor [c], or an int for all): the mask-1 call is envelopeKnots bit for bit, and
    the planes of every mask tried are theirs in the mask-15 call bit for bit; `valid` is the same in all of them."""
    import torch
    dof, M = batch.dof, g.numel() - 1
    old, old_valid = ltp.envelopeKnots(batch, f, c, k, g, closed=closed)
    whole, valid = ltp.envelopeKnotsArrays(batch, f, c, k, g, arrays="qvaj", closed=closed)
    assert whole.shape == (c, 4, dof, M, 2)
    for mask in (1, 2, 4, 8, 3, 6, 12, 9, 7):
        part, v2 = ltp.envelopeKnotsArrays(batch, f, c, k, g, arrays=mask, closed=closed)
        torch.cuda.synchronize()
        planes = ac.selected(mask)
        assert part.shape == (c, len(planes), dof, M, 2)
        assert torch.equal(ac.int_view(part), ac.int_view(whole[:, planes].contiguous())), (what, mask)
        assert torch.equal(v2, valid)
        if mask == 1:
            assert torch.equal(ac.int_view(part[:, 0].contiguous()), ac.int_view(old)), what
            assert torch.equal(v2, old_valid)


@pytest.mark.parametrize("name,n", [("panda", 1500), ("ref", 1000), ("ref-dof1", 700), ("panda-matlab", 600)])
def test_mask_identities(name, n):
    """Mask 1 is envelopeKnots bit for bit; every single-array call is its plane of the mask-15 call bit for bit, and so are the
    planes of masks 3, 6 and 12; batch.status is what it was. The shapes are those at which two kernels that share a walk can part:
    M = 1 and M = LTP_MAX_KNOTS - 1 beside the three grids; one joint and seven; count * dof no multiple of 256 (lanes that return
    behind the barrier) in every call; a rejected plan; starts below 0, at traj_len and past it; both modes; per-plan and uniform
    starts; both semantics; a captured call replayed twice."""
    import torch
    ltp, dof, batch, lens = _identity_batch(name, n)
    rng = np.random.default_rng(5)
    first, count = H.odd_range(n, dof)
    assert (n * dof) % 256 != 0 and (count * dof) % 256 != 0 and n * dof > 256 and first <= REJECTED < first + count
    status = batch.status.clone()
    for gname in ("mpc", "duplicates", "n65"):
        g = _grid(ac.GRIDS[gname])
        for closed in (False, True):
            for f, c in ((0, n), (first, count)):
                k = torch.from_numpy(_starts(rng, lens)[f:f + c]).to(DEV)
                _assert_mask_identities(ltp, batch, f, c, k, g, closed, (gname, closed, f))
    k_edge = _edge_starts(rng, lens)
    assert np.any(k_edge < 0) and np.any((k_edge == lens) & (lens > 0)) and np.any(k_edge > lens)
    one, most = _grid(np.array([0, 7], dtype=np.int32)), _grid(ac.GRIDS["max"])
    assert most.numel() - 1 == ac.MAX_INTERVALS
    for closed in (False, True):
        for grid in (one, most, g):
            f, c = (first, 301) if grid is most else (0, n)      # (the longest grid on fewer plans: its planes are large)
            _assert_mask_identities(ltp, batch, f, c, torch.from_numpy(k_edge[f:f + c]).to(DEV), grid, closed, ("edge starts", closed, f))
            _assert_mask_identities(ltp, batch, f, c, 3, grid, closed, ("uniform start", closed, f))
    # the mask-q call captured, replayed after its starts were rewritten in place, twice: the q-only call's bits each time
    k = torch.from_numpy(k_edge).to(DEV)
    out = torch.zeros((n, 1, dof, g.numel() - 1, 2), dtype=torch.float64, device=DEV)
    valid = torch.zeros((n,), dtype=torch.int32, device=DEV)
    graph = H.capture(lambda: ltp.envelopeKnotsArrays(batch, 0, n, k, g, arrays="q", closed=True, out=out, valid=valid))
    for _ in range(2):
        H.replay(graph, [(k, _starts(rng, lens))], out, valid)
        old, old_valid = ltp.envelopeKnots(batch, 0, n, k, g, closed=True)
        torch.cuda.synchronize()
        assert torch.equal(ac.int_view(out[:, 0].contiguous()), ac.int_view(old)) and torch.equal(valid, old_valid)
    by_name, _ = ltp.envelopeKnotsArrays(batch, 0, n, 3, g, arrays="ja")
    by_mask, _ = ltp.envelopeKnotsArrays(batch, 0, n, 3, g, arrays=12)
    torch.cuda.synchronize()
    assert torch.equal(ac.int_view(by_name), ac.int_view(by_mask))
    assert torch.equal(batch.status, status), "envelopeKnotsArrays changed batch.status"


@pytest.mark.parametrize("gname", ["mpc", "duplicates"])
def test_agreement_with_the_knots_call(gname):
    """lo <= the X sampleKnots stores at k + g[w] <= hi for every array and interval; with closed = 1 also at k + g[w + 1]; a
    duplicate interval (g[w] == g[w + 1]) equals that sample twice."""
    E.agreement_with_the_knots_call(ARRAYS, gname, n=1500)


def test_the_end_of_a_plan():
    """k = traj_len - 2 on the grid [0, 1, 5]. Interval 1 starts at the last sample and reaches past it: v, a and j hold the 0 of
    the resting robot, lo <= 0 <= hi, and q is {q_last, q_last}. Interval 0 is sample traj_len - 2 alone when closed = 0 — every
    array holds that sample twice — and with closed = 1 it also holds the last sample. (Under the interval rule of
    ltp_envelope_knots_batch interval 1 of this grid starts at traj_len - 1 in BOTH modes, so its q pair is the last position
    twice in both; what `closed` changes here is interval 0.) From k >= traj_len every pair is {q_last, q_last} for q and {0, 0}
    for v, a and j."""
    import torch
    n = 1500
    ltp, dof, lim, qs, batch, full, lens = _batch("panda", n)
    planned = batch.traj_len > 1
    assert int(planned.sum().item()) > 0.9 * n
    one = _grid(np.array([0], dtype=np.int32))
    last = ltp.sampleKnots(batch, 0, n, (batch.traj_len - 1).clamp(min=0).int(), one)[0][:, :, :, 0].clone()    # sample traj_len - 1 [n, 4, dof]
    prev = ltp.sampleKnots(batch, 0, n, (batch.traj_len - 2).clamp(min=0).int(), one)[0][:, :, :, 0].clone()    # sample traj_len - 2
    g = _grid(np.array([0, 1, 5], dtype=np.int32))
    k = (batch.traj_len - 2).clamp(min=0).int()
    for closed in (0, 1):
        env, valid = ltp.envelopeKnotsArrays(batch, 0, n, k, g, closed=closed)
        torch.cuda.synchronize()
        e, p1, p2 = env[planned], last[planned], prev[planned]
        assert bool(((e[:, 1:, :, 1, 0] <= 0.0) & (0.0 <= e[:, 1:, :, 1, 1])).all().item()), closed
        # and nothing but the last sample and the 0 behind it
        assert bool((e[:, 1:, :, 1, 0] == torch.minimum(p1[:, 1:], torch.zeros_like(p1[:, 1:]))).all().item()), closed
        assert bool((e[:, 1:, :, 1, 1] == torch.maximum(p1[:, 1:], torch.zeros_like(p1[:, 1:]))).all().item()), closed
        ql = p1[:, 0]
        assert torch.equal(ac.int_view(e[:, 0, :, 1].contiguous()), ac.int_view(torch.stack([ql, ql], dim=2).contiguous())), closed
        if closed == 0:
            assert bool(((e[:, :, :, 0, 0] == p2) & (e[:, :, :, 0, 1] == p2)).all().item())
            assert torch.equal(ac.int_view(e[:, 0, :, 0].contiguous()), ac.int_view(torch.stack([p2[:, 0], p2[:, 0]], dim=2).contiguous()))
        else:
            assert bool(((e[:, :, :, 0, 0] == torch.minimum(p2, p1)) & (e[:, :, :, 0, 1] == torch.maximum(p2, p1))).all().item())
        assert torch.equal(valid[planned], torch.full_like(valid[planned], 2))
    has = batch.traj_len > 0
    for extra in (0, 1, 7):
        env, valid = ltp.envelopeKnotsArrays(batch, 0, n, (batch.traj_len + extra).int(), g, closed=True)
        torch.cuda.synchronize()
        e = env[has]
        ql = last[has][:, 0, :, None, None].expand(-1, -1, 2, 2)
        assert torch.equal(ac.int_view(e[:, 0].contiguous()), ac.int_view(ql.contiguous())), extra
        assert bool((e[:, 1:] == 0.0).all().item()), extra
        assert int(valid.abs().sum().item()) == 0


@pytest.mark.parametrize("kind", ["retimed", "limit_sets", "matlab", "stop"])
def test_other_batch_kinds(kind):
    """A retimed batch, a batch with three bound limit sets, MATLAB semantics (full rows from the walk sampler) and a stop batch:
    each against its own reduced rows on the MPC grid, both modes, all four arrays, whole and a sub-range."""
    E.other_batch_kinds(ARRAYS, kind, ("mpc",), sub_masks=(15, 6))


def test_refusals_and_bounds():
    """Each refusal of the device entry is LTP_ERR_INVALID_ARGUMENT, its text names the reason, and the buffer it was given keeps
    its pattern; a geometry change after planning is refused in ltp_state_at_batch's words; guard words behind the call's elements
    stay intact; valid = NULL is accepted. Host edge lists outside the contract and a bad `arrays` are refused by
    ltp_plan_envelope_knots_arrays_host (LtpError) and by the wrappers (ValueError) before any launch."""
    E.refusals_and_bounds(ARRAYS, more_refusals=((dict(arrays=0), "arrays"), (dict(arrays=16), "arrays"), (dict(arrays=-1), "arrays"),
                                                 (dict(reserved=1), "reserved"), (dict(reserved=-1), "reserved")))


BAD_ARRAYS = r'''for (int arrays : {0, 16}) {
    try {
      std::vector<double> e2;
      ltp.planEnvelopeKnotsArraysBatch(QUERIES, edges, false, arrays, e2);
    } catch (const std::exception&) { ++refused; }
  }'''


def test_host_and_dropin_paths(tmp_path):
    """planEnvelopeKnotsArraysHost equals the device path bitwise and its status carries END_LIMIT like planBatchHost(sample=False);
    a small C++ program gives the same bytes through LongTermPlanner::planEnvelopeKnotsArraysBatch."""
    E.host_and_dropin_paths(ARRAYS, tmp_path, refused=5, more_refusals=BAD_ARRAYS)


def test_graph_capture_and_replay_with_new_starts_and_a_new_grid():
    """The call allocates nothing: captured on one stream (one kernel node) and replayed after first_sample AND the content of
    edge_offsets were rewritten in place, it gives what a direct call gives for the new starts and the new grid — twice."""
    E.graph_capture_and_replay(ARRAYS)
