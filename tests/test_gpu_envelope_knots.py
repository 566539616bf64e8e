"""Horizon envelopes (ltp_envelope_knots_batch, include/ltp_hip.h) on the GPU: per plan and joint {min q, max q} over the trajectory
samples between the edges k + g[w] and k + g[w + 1] of a knot grid. Compared with the reduced rows of the full-row sampler for the
same batch (tests/envelope_knots_checker.py, itself pinned to a plain loop by tests/test_envelope_knots_cpu.py) under the project's
acceptance rule for the analytic envelope form, with ltp_envelope_batch's register walk on uniform grids (bit for bit), with the
knots call, on the run-census batches, on other batch kinds, through the host and drop-in paths and under graph capture. The
batches and planner helpers are tests/horizon_helpers.py's and tests/gpu_helpers.py's.

Contract-breaking device grids are pinned on the host only (tests/cpp/envelope_knots_ranges_test.cc): no test here feeds one."""
import ctypes as C

import numpy as np
import pytest

import envelope_knots_checker as ec
import horizon_helpers as H
import knots_checker as kc
import run_census as rc
from gpu_helpers import _rows
from horizon_helpers import DEV, INVALID
from horizon_helpers import assert_envelopes as _assert_envelopes
from horizon_helpers import grid_tensor as _grid

pytestmark = pytest.mark.gpu

REJECTED = 11                 # the plan every batch of _batch() has rejected: a NaN envelope among planned neighbours


_CACHE = {}


def _batch(name, n, pow_rule="libm"):
    """H.batch with one rejected plan (a start velocity no limit admits); the latest one is kept."""
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
        _CACHE.update(key=key, v=(ltp, dof, lim, qs, batch, full, lens))
    return _CACHE["v"]


def _starts(rng, lens):
    """k per plan, uniform in [-5, traj_len + 40]."""
    return rng.integers(-5, lens.astype(np.int64) + 41).astype(np.int32)


@pytest.mark.parametrize("name,n,pow_rule", [("panda", 3000, "libm"), ("panda", 3000, "exact"), ("ref", 2000, "libm"), ("ref30", 300, "libm")])
def test_envelopes_against_reduced_rows(name, n, pow_rule):
    """Every envelope against the minimum and maximum of the samples sampleBatch wrote for its interval, by the acceptance rule of
    the analytic form: NaN pattern identical, inside the samples, |d| <= 1e-12, at least 0.999 of the values bit-identical. The
    whole batch (with its rejected plan) and a slice with first > 0 whose count * dof is no multiple of 64; starts per plan from
    [-5, traj_len + 40]; both `closed` modes; `valid` against its formula."""
    ltp, dof, lim, qs, batch, full, lens = _batch(name, n, pow_rule)
    rng = np.random.default_rng(99)
    first, count = H.odd_range(n, dof)
    assert first > 0 and (count * dof) % 64 != 0 and first <= REJECTED < first + count
    L = lens.astype(np.int64)
    for gname in ("mpc", "duplicates", "from37", "n33", "n65", "geometric", "max"):
        g = ec.GRIDS[gname]
        assert gname != "max" or len(g) - 1 == ec.MAX_INTERVALS == 511
        for closed in (0, 1):
            k = _starts(rng, lens)
            kk = np.maximum(k.astype(np.int64), 0)
            ends, starts = float(np.mean((L > 0) & (kk + int(g[-1]) >= L))), float(np.mean((L > 0) & (kk + int(g[0]) >= L)))
            what = f"{name} {pow_rule} grid {gname} closed {closed}"
            env, _, worst, share = _assert_envelopes(ltp, batch, full, k, g, closed, 0, n, f"{what} whole batch")
            _, _, worst2, share2 = _assert_envelopes(ltp, batch, full, k, g, closed, first, count, f"{what} plans [{first}, {first + count})")
            print(f"{what}: horizon ends past traj_len {ends:.3f}, starts there {starts:.3f}; worst |d| {max(worst, worst2):.3e}, "
                  f"bit-identical {min(share, share2):.6f}")
            assert ends > 0.0 and min(share, share2) >= 0.999, (what, ends, share, share2)
            assert bool(np.isnan(env[REJECTED].cpu().numpy()).all())


@pytest.mark.parametrize("name", rc.BATCHES)
def test_the_smallest_shapes(oracle_mod, name):
    """The run-census batches (rows of 1-153 samples, collided switch indices, switching times on exact multiples of the sample
    time): unit, two-sample and duplicate-holding grids, both modes, a uniform k swept over 0 .. 8 and per-plan starts."""
    R = _rows(oracle_mod, name)
    ltp, batch, n, cen = R["ltp"], R["batch"], R["n"], R["cen"]
    lens = R["rec"]["traj_len"]
    rng = np.random.default_rng(17)
    M = 24
    grids = kc.SMALL_GRIDS
    assert list(grids) == ["unit", "two", "duplicates"] and np.array_equal(grids["unit"], np.arange(M + 1)) and np.array_equal(grids["two"], 2 * np.arange(M + 1))
    assert np.any(np.diff(grids["duplicates"]) == 0) and len(grids["duplicates"]) == M + 1
    describe = lambda mask: rc.describe(cen, mask)
    worst, least = 0.0, 1.0
    for gname, g in grids.items():
        for closed in (0, 1):
            for k in list(range(9)) + [_starts(rng, lens)]:
                what = f"{name} grid {gname} closed {closed} k {'per plan' if not isinstance(k, int) else k}"
                _, _, w, s = _assert_envelopes(ltp, batch, R["full"], k, g.astype(np.int32), closed, 0, n, what, describe)
                worst, least = max(worst, w), min(least, s)
    print(f"{name}: worst |d| {worst:.3e}, least bit-identical share {least:.6f}")
    assert least >= 0.999, (name, least)


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
    import torch
    n = 3000
    ltp, dof, lim, qs, batch, full, lens = _batch("panda", n)
    g = ec.GRIDS[gname]
    M = len(g) - 1
    k = torch.from_numpy(_starts(np.random.default_rng(8), lens)).to(DEV)
    rows, kv = ltp.sampleKnots(batch, 0, n, k, _grid(g))
    planned = batch.traj_len > 0
    q = rows[:, 0, :, :M + 1][planned]                           # [plans, dof, M + 1]
    dup = torch.from_numpy(np.diff(g) == 0).to(DEV)
    for closed in (0, 1):
        env, valid = ltp.envelopeKnots(batch, 0, n, k, _grid(g), closed=closed)
        torch.cuda.synchronize()
        e = env[planned]
        assert bool(((e[..., 0] <= q[..., :M]) & (q[..., :M] <= e[..., 1])).all().item()), (gname, closed)
        if closed:
            assert bool(((e[..., 0] <= q[..., 1:]) & (q[..., 1:] <= e[..., 1])).all().item()), (gname, closed)
        if bool(dup.any().item()):
            twice = torch.stack([q[..., :M], q[..., :M]], dim=3)[:, :, dup]
            assert torch.equal(ec.int_view(e[:, :, dup].contiguous()), ec.int_view(twice.contiguous())), (gname, closed)
        # both calls count the intervals / knots that start inside the trajectory alike, but for the last edge
        last_real = ((k.long().clamp(min=0) + int(g[-1])) < batch.traj_len.long()).int()
        assert torch.equal(valid, kv - torch.where(planned, last_real, torch.zeros_like(last_real)))
    assert gname != "duplicates" or int(dup.sum().item()) >= 5


@pytest.mark.parametrize("kind", ["retimed", "limit_sets", "matlab"])
def test_other_batch_kinds(kind):
    """A retimed batch, a batch with three bound limit sets, MATLAB semantics (full rows from the walk sampler): each against its
    own reduced rows, n = 1000, on the MPC and the geometric grid, both modes."""
    n = 1000
    ltp, dof, batch, full, lens, _ = H.other_batch(kind, n)
    rng = np.random.default_rng(21)
    first, count = H.odd_range(n, dof)
    for gname in ("mpc", "geometric"):
        g = ec.GRIDS[gname]
        for closed in (0, 1):
            k = _starts(rng, lens)
            _, _, worst, share = _assert_envelopes(ltp, batch, full, k, g, closed, 0, n, f"{kind} {gname} closed {closed}")
            _, _, worst2, share2 = _assert_envelopes(ltp, batch, full, k, g, closed, first, count, f"{kind} {gname} closed {closed} sub-range")
            print(f"{kind} {gname} closed {closed}: worst |d| {max(worst, worst2):.3e}, bit-identical {min(share, share2):.6f}")
            assert min(share, share2) >= 0.999


def test_refusals_and_bounds():
    """Each refusal of the device entry is LTP_ERR_INVALID_ARGUMENT, its text names the reason, and the buffer it was given keeps
    its pattern; a geometry change after planning is refused in ltp_state_at_batch's words; guard words behind count*dof*M*2 stay
    intact; valid = NULL is accepted. Host edge lists outside the contract are refused by ltp_plan_envelope_knots_host (LtpError)
    and by envelopeKnots given a host list (ValueError) before any launch."""
    import torch
    from longtermplanner_amd import _abi
    n = 64
    g = ec.GRIDS["mpc"]
    M = len(g) - 1
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    lib, O = ltp._lib, _abi.EnvelopeKnotsOpts
    need = n * dof * M * 2
    assert lib.ltp_envelope_knots_elements(ltp._h, n, M) == need
    guard = 64
    out = torch.full((need + guard,), H.PATTERN, dtype=torch.float64, device=DEV)
    big = torch.full((n * dof * (ec.MAX_INTERVALS + 1) * 2,), H.PATTERN, dtype=torch.float64, device=DEV)
    grid = _grid(np.concatenate([g, np.zeros(ec.MAX_INTERVALS + 2 - len(g), dtype=np.int32) + int(g[-1])]))     # long enough for every M tried
    call = H.reader_call(lib.ltp_envelope_knots_batch, ltp, batch, n, out, capacity=need)
    good = dict(size=C.sizeof(O), n_intervals=M, closed=1, edge_offsets=grid.data_ptr())          # valid = NULL
    status = batch.status.clone()
    rc_, msg = call(O(**good))
    assert rc_ == 0, msg
    torch.cuda.synchronize()
    want, _ = ltp.envelopeKnots(batch, 0, n, 0, _grid(g), closed=True)
    torch.cuda.synchronize()
    assert torch.equal(ec.int_view(out[:need]), ec.int_view(want.reshape(-1))), "valid = NULL changes the envelopes"
    assert bool((out[need:] == H.PATTERN).all().item()), "the guard words behind count * dof * M * 2 were written"
    assert torch.equal(batch.status, status)
    H.common_refusals(ltp, batch, n, dof, call, O, good, out, need - 1, "ltp_envelope_knots_elements")
    for bad, text in ((dict(edge_offsets=None), "edge_offsets is NULL"), (dict(n_intervals=0), "n_intervals"), (dict(n_intervals=-1), "n_intervals"),
                      (dict(n_intervals=ec.MAX_INTERVALS + 1), "LTP_MAX_KNOTS - 1"), (dict(closed=2), "closed"), (dict(closed=-1), "closed")):
        rc_, msg = call(O(**dict(good, **bad)), buf=big, capacity=big.numel())
        assert rc_ == INVALID and text in msg, (bad, rc_, msg)
    torch.cuda.synchronize()
    assert bool((out == H.PATTERN).all().item()) and bool((big == H.PATTERN).all().item()), "a refused call wrote to the buffer"
    # the largest admitted grid is a call like any other
    rc_, msg = call(O(**dict(good, n_intervals=ec.MAX_INTERVALS)), buf=big, capacity=big.numel())
    assert rc_ == 0, msg
    torch.cuda.synchronize()
    assert bool((big[n * dof * ec.MAX_INTERVALS * 2:] == H.PATTERN).all().item())
    # host edge lists are looked at: the library's host entry and the wrapper refuse what breaks the contract, before any launch
    from longtermplanner_amd._abi import LtpError
    env_out = out[:need].view(n, dof, M, 2)
    for bad, text in (([0, 5, 4, 9], "decreases"), ([-1, 0, 3], "negative"), ([0, (1 << 30) + 1], "beyond 2^30"), ([], "n_intervals"),
                      ([11], "n_intervals"), (list(range(ec.MAX_INTERVALS + 2)), "LTP_MAX_KNOTS")):
        with pytest.raises(LtpError) as e:
            ltp.planEnvelopeKnotsHost(*qs, 0, bad)
        assert e.value.code == INVALID and text in str(e.value), (bad, str(e.value))
        with pytest.raises(ValueError):
            ltp.envelopeKnots(batch, 0, n, 0, bad, out=env_out)
    with pytest.raises(ValueError):
        ltp.planEnvelopeKnotsHost(*qs, 0, [0.5, 1.5])
    torch.cuda.synchronize()
    assert bool((out == H.PATTERN).all().item()), "envelopeKnots wrote to the buffer although it refused its host edges"
    assert call(O(**good))[0] == 0


DROPIN = r'''
#include "long_term_planner/long_term_planner.h"
#include <cstdio>
using namespace long_term_planner;
int main(int argc, char** argv) {
  const int dof = 7, n = 40, E = 40;
  std::vector<double> q_min = {-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973};
  std::vector<double> q_max = {2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973};
  std::vector<double> v_max = {2.175, 2.175, 2.175, 2.175, 2.61, 2.61, 2.61};
  std::vector<double> a_max = {15.0, 7.5, 10.0, 12.5, 15.0, 20.0, 20.0};
  std::vector<double> j_max = {7500.0, 3750.0, 5000.0, 6250.0, 7500.0, 10000.0, 10000.0};
  LongTermPlanner ltp(dof, 0.001, q_min, q_max, v_max, a_max, j_max);
  std::vector<double> in(4 * n * dof);
  std::vector<int> k(n), edges(E);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size() || std::fread(k.data(), sizeof(int), k.size(), f) != k.size() ||
      std::fread(edges.data(), sizeof(int), edges.size(), f) != edges.size()) return 2;
  std::fclose(f);
  std::vector<double> env;
  std::vector<int> valid;
  BatchTrajectory b;
  const long long ok = ltp.planEnvelopeKnotsBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, edges, true,
                                                  env, &valid, &b);
  int refused = 0;
  for (const std::vector<int>& bad : {std::vector<int>{4, 3}, std::vector<int>{7}, std::vector<int>{}}) {
    try {
      std::vector<double> e2;
      ltp.planEnvelopeKnotsBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, bad, false, e2);
    } catch (const std::exception&) { ++refused; }
  }
  if (refused != 3) return 3;
  FILE* o = std::fopen(argv[2], "wb");
  std::fwrite(env.data(), sizeof(double), env.size(), o);
  std::fwrite(valid.data(), sizeof(int), valid.size(), o);
  std::fwrite(b.status.data(), sizeof(int), b.status.size(), o);
  std::fclose(o);
  std::printf("%lld ok, %zu doubles\n", ok, env.size());
  return 0;
}
'''


def test_host_and_dropin_paths(tmp_path):
    """planEnvelopeKnotsHost equals the device path bitwise and its status carries END_LIMIT like planBatchHost(sample=False); a
    small C++ program gives the same bytes through LongTermPlanner::planEnvelopeKnotsBatch."""
    import torch
    n = 40
    g = ec.GRIDS["mpc"]
    M = len(g) - 1
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    qs[0][3, 1] = 2.5                               # a goal beyond joint 1's range: planned, then END_LIMIT
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    lens = batch.traj_len.cpu().numpy()
    k = _starts(np.random.default_rng(1), lens)
    dev_env, dev_valid = ltp.envelopeKnots(batch, 0, n, torch.from_numpy(k).to(DEV), _grid(g), closed=True)
    dev_env, dev_valid = dev_env.cpu().numpy(), dev_valid.cpu().numpy()
    assert 0 < int((dev_valid > 0).sum()) and int((dev_valid < M).sum()) > 0
    assert not (batch.status.cpu().numpy()[3] & 8), "the device call forms no end-limit verdict"
    rec, env, valid = ltp.planEnvelopeKnotsHost(*qs, k, g, closed=True)
    assert env.shape == (n, dof, M, 2)
    assert np.array_equal(env.view(np.uint8), dev_env.view(np.uint8)) and np.array_equal(valid, dev_valid)
    plain = ltp.planBatchHost(*qs, sample=False)
    assert np.array_equal(rec["status"], plain["status"]) and (rec["status"][3] & 8) and np.array_equal(rec["traj_len"], lens)
    _, env_u, valid_u = ltp.planEnvelopeKnotsHost(*qs, 5, [int(x) for x in g])
    du, dv = ltp.envelopeKnots(batch, 0, n, 5, g)                                   # a host grid: uploaded by the wrapper
    assert np.array_equal(env_u.view(np.uint8), du.cpu().numpy().view(np.uint8)) and np.array_equal(valid_u, dv.cpu().numpy())

    raw = H.run_dropin(tmp_path, "envelope_knots", DROPIN, np.concatenate([x.reshape(-1) for x in qs]).astype(np.float64).tobytes()
                       + k.astype(np.int32).tobytes() + g.astype(np.int32).tobytes())
    H.assert_dropin_bytes(raw, env, valid, rec["status"])


def test_graph_capture_and_replay_with_new_starts_and_a_new_grid():
    """The call allocates nothing: captured on one stream (one kernel node) and replayed after first_sample AND the content of
    edge_offsets were rewritten in place, it gives what a direct call gives for the new starts and the new grid — twice."""
    import torch
    n = 1000
    ltp, dof, lim, qs, batch, full, lens = _batch("panda", n)
    rng = np.random.default_rng(77)
    ga = ec.GRIDS["mpc"]
    E = len(ga)
    gb = (np.arange(E) ** 2 // 2 + 3).astype(np.int32)             # another 40 edges: further out, g[0] = 3
    gc = np.sort(rng.integers(0, 2000, E)).astype(np.int32)
    ka, kb, kcs = (_starts(rng, lens) for _ in range(3))
    assert np.count_nonzero(ka != kb) > 0.5 * n
    k, grid = torch.from_numpy(ka).to(DEV), _grid(ga)
    out = torch.zeros((n, dof, E - 1, 2), dtype=torch.float64, device=DEV)
    valid = torch.zeros((n,), dtype=torch.int32, device=DEV)
    graph = H.capture(lambda: ltp.envelopeKnots(batch, 0, n, k, grid, closed=True, out=out, valid=valid))
    for k_new, g_new in ((kb, gb), (kcs, gc)):
        H.replay(graph, [(k, k_new), (grid, g_new)], out, valid)
        direct, direct_valid = ltp.envelopeKnots(batch, 0, n, k, grid, closed=True)
        torch.cuda.synchronize()
        assert torch.equal(ec.int_view(direct), ec.int_view(out)) and torch.equal(direct_valid, valid)
        red, exp_valid, planned = ec.expected(full, batch.offsets, batch.traj_len, k, g_new, 1, dof, 0, n)
        bad, worst, share = ec.compare(out, red, planned)
        assert not bool(bad.any().item()) and torch.equal(valid, exp_valid), (worst, share)
