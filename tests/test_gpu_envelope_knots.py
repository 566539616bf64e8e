"""Horizon envelopes (ltp_envelope_knots_batch, include/ltp_hip.h) on the GPU: per plan and joint {min q, max q} over the trajectory
samples between the edges k + g[w] and k + g[w + 1] of a knot grid. Compared with the reduced rows of the full-row sampler for the
same batch (tests/envelope_checker.py, itself pinned to a plain loop by tests/test_envelope_knots_cpu.py) under the project's
acceptance rule for the analytic envelope form, with ltp_envelope_batch's register walk on uniform grids (bit for bit), with the
knots call, on the run-census batches, on other batch kinds, through the host and drop-in paths and under graph capture. The call
is the arrays call with mask q: the bodies it shares with tests/test_gpu_envelope_arrays.py are tests/envelope_helpers.py's.

Contract-breaking device grids are pinned on the host only (tests/cpp/envelope_knots_ranges_test.cc): no test here feeds one."""
import numpy as np
import pytest

import envelope_checker as ec
import envelope_helpers as E
import horizon_helpers as H
import run_census as rc
from envelope_helpers import QONLY, REJECTED, _batch
from horizon_helpers import grid_tensor as _grid

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,n,pow_rule", [("panda", 3000, "libm"), ("panda", 3000, "exact"), ("ref", 2000, "libm"), ("ref30", 300, "libm")])
def test_envelopes_against_reduced_rows(name, n, pow_rule):
    """Every envelope against the minimum and maximum of the samples sampleBatch wrote for its interval, by the acceptance rule of
    the analytic form: NaN pattern identical, inside the samples, |d| <= 1e-12, at least 0.999 of the values bit-identical. The
    whole batch (with its rejected plan) and a slice with first > 0 whose count * dof is no multiple of 64; starts per plan from
    [-5, traj_len + 40]; both `closed` modes; `valid` against its formula."""
    E.reduced_rows(QONLY, name, n, pow_rule, ("mpc", "duplicates", "from37", "n33", "n65", "geometric", "max"), masks=(1,))


@pytest.mark.parametrize("name", rc.BATCHES)
def test_the_smallest_shapes(oracle_mod, name):
    """The run-census batches (rows of 1-153 samples, collided switch indices, switching times on exact multiples of the sample
    time): unit, two-sample and duplicate-holding grids, both modes, a uniform k swept over 0 .. 8 and per-plan starts."""
    E.smallest_shapes(QONLY, oracle_mod, name)


@pytest.mark.parametrize("name,n", [("panda", 3000), ("ref", 2000)])
def test_uniform_grids_are_the_existing_call(name, n):
    """k = 0, g[w] = w * window, closed = 0: bit-identical to envelopeBatch(window, M) in analytic mode without a table pass
    (k_envelope_walk: same stretches, same candidates). The new call leaves batch.status as it is."""
    import torch
    ltp, dof, lim, qs, batch, full, lens = _batch(name, n)
    ltp.setEnvelopeMode("analytic")
    ltp.setTablePass(0)
    try:
        for window, M in ((1, 40), (5, 36), (64, 32), (700, 4)):
            fresh = ltp.planSwitchTimesBatch(*H.tensors(qs))
            torch.cuda.synchronize()
            status = fresh.status.clone()
            env, valid = ltp.envelopeKnots(fresh, 0, n, 0, _grid(np.arange(M + 1) * window), closed=False)
            torch.cuda.synchronize()
            assert torch.equal(fresh.status, status), "envelopeKnots changed batch.status"
            old = ltp.envelopeBatch(fresh, 0, n, window, M)
            assert "k_envelope_walk" in ltp.lastSamplerKernel(), ltp.lastSamplerKernel()
            torch.cuda.synchronize()
            assert torch.equal(ec.int_view(env), ec.int_view(old)), f"{name}: window {window} x {M} differs from envelopeBatch"
            want = torch.clamp((fresh.traj_len.long() + window - 1) // window, max=M).int()
            assert torch.equal(valid, want)
            assert bool(torch.isnan(env[REJECTED]).all().item()) and int((valid > 0).sum().item()) > 0.9 * n
    finally:
        ltp.setEnvelopeMode("exhaustive")
        ltp.setTablePass(0)


@pytest.mark.parametrize("gname", ["mpc", "duplicates", "geometric"])
def test_agreement_with_the_knots_call(gname):
    """lo <= the q sampleKnots stores at k + g[w] <= hi for every interval; with closed = 1 also at k + g[w + 1]; a duplicate
    interval (g[w] == g[w + 1]) equals that q twice, bit for bit."""
    E.agreement_with_the_knots_call(QONLY, gname, n=3000)


@pytest.mark.parametrize("kind", ["retimed", "limit_sets", "matlab"])
def test_other_batch_kinds(kind):
    """A retimed batch, a batch with three bound limit sets, MATLAB semantics (full rows from the walk sampler): each against its
    own reduced rows, n = 1000, on the MPC and the geometric grid, both modes."""
    E.other_batch_kinds(QONLY, kind, ("mpc", "geometric"), sub_masks=(1,))


def test_refusals_and_bounds():
    """Each refusal of the device entry is LTP_ERR_INVALID_ARGUMENT, its text names the reason, and the buffer it was given keeps
    its pattern; a geometry change after planning is refused in ltp_state_at_batch's words; guard words behind count*dof*M*2 stay
    intact; valid = NULL is accepted. Host edge lists outside the contract are refused by ltp_plan_envelope_knots_host (LtpError)
    and by envelopeKnots given a host list (ValueError) before any launch."""
    E.refusals_and_bounds(QONLY)


def test_host_and_dropin_paths(tmp_path):
    """planEnvelopeKnotsHost equals the device path bitwise and its status carries END_LIMIT like planBatchHost(sample=False); a
    small C++ program gives the same bytes through LongTermPlanner::planEnvelopeKnotsBatch, which refuses three bad edge lists."""
    E.host_and_dropin_paths(QONLY, tmp_path, refused=3)


def test_graph_capture_and_replay_with_new_starts_and_a_new_grid():
    """The call allocates nothing: captured on one stream (one kernel node) and replayed after first_sample AND the content of
    edge_offsets were rewritten in place, it gives what a direct call gives for the new starts and the new grid — twice."""
    E.graph_capture_and_replay(QONLY)
