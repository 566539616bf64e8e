"""Stop horizons (ltp_stop_knots_batch, include/ltp_hip.h) on the GPU: standstill position and time of every joint from every knot
k + g[w] of a planned batch, one kernel. The yardstick is the composition of merged entries on the device, Y: sampleKnots, a permute
to [count * N, dof] states, torch.clamp of the accelerations, ONE planStopBatch(check="braking") with the limit-set index repeated N
times; int64 views are compared. Also: the oracle's optBraking on the device's own knot states, other batch kinds, refusals, graph
capture with rewritten starts and grid, the host entry and the C++ wrapper. Y and the batches are tests/horizon_helpers.py's, the
grids tests/knots_checker.py's.

No test feeds the device a grid that breaks the contract: the clamps that keep such a grid from changing an address are the shared
walk's (ltp_knots.hpp), pinned on the host by tests/cpp/knots_ranges_test.cc, and tests/test_gpu_knots.py feeds none either."""
import ctypes as C

import numpy as np
import pytest

import horizon_checker as hc
import horizon_helpers as H
import knots_checker as kc
import stop_knots_checker as skc
from horizon_helpers import DEV, INVALID
from horizon_helpers import assert_stop_knots as _assert_stop_knots
from horizon_helpers import grid_tensor as _grid
from horizon_helpers import uniform_starts as _uniform_starts

pytestmark = pytest.mark.gpu

CASES = [("panda", 1000, tuple(kc.GRIDS)), ("ref", 65, ("mpc", "n65")), ("ref30", 130, ("mpc", "n33", "n65"))]


@pytest.mark.parametrize("pow_rule", ["libm", "exact"])
@pytest.mark.parametrize("name,n,grids", CASES, ids=[c[0] for c in CASES])
def test_bits_against_the_composition(name, n, grids, pow_rule):
    """Both acceleration modes against Y, on every grid of the case, from k = 0, from a uniform draw (negative and past-the-end
    starts included), from kc.aimed_starts (a stretch between two knots), over the whole batch and over a sub-range whose
    count * dof is no multiple of 64. STRICT: Y where |a| <= a_max, NaN elsewhere; such elements occur (sampled accelerations
    exceed a_max by rounding)."""
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch(name, n, pow_rule)
    rng = np.random.default_rng(99)
    first, count = H.odd_range(n, dof)
    assert (count * dof) % 64 != 0
    refused = 0
    for gname in grids:
        g = kc.GRIDS[gname]
        ku = _uniform_starts(rng, lens)
        assert np.count_nonzero(ku < 0) > 0 and np.count_nonzero(ku >= lens) > 0
        what = f"{name} {pow_rule} grid {gname}"
        refused += _assert_stop_knots(ltp, batch, 0, g, 0, n, f"{what}, k = 0")
        refused += _assert_stop_knots(ltp, batch, ku, g, 0, n, f"{what}, uniform starts")
        _assert_stop_knots(ltp, batch, ku, g, first, count, f"{what}, uniform starts, plans [{first}, {first + count})")
        ka = kc.aimed_starts(ku, g, lens, t_scaled)
        _assert_stop_knots(ltp, batch, ka, g, 0, n, f"{what}, aimed starts")
    print(f"{name} {pow_rule}: {refused} elements with |a| > a_max")
    if name == "panda":
        assert refused >= 8


def test_more_passes_than_one():
    """S-ref limits, k = 0, the wide grid: some plan has a joint whose knots fall into more than 6 stretches, more than a lane
    parks in one pass under either pow rule (5 under libm, 6 under exact), so the second pass runs."""
    n = 500
    g = kc.wide_grid()
    for pow_rule in ("libm", "exact"):
        ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("ref", n, pow_rule)
        k = np.zeros(n, dtype=np.int32)
        assert int(np.count_nonzero(kc.stretches(k, g, lens, t_scaled) > 6)) >= 1
        _assert_stop_knots(ltp, batch, k, g, 0, n, f"wide grid {pow_rule}, k = 0")
        _assert_stop_knots(ltp, batch, k, g, 3, n - 10, f"wide grid {pow_rule}, sub-range")


@pytest.mark.parametrize("kind", ["retimed", "limit_sets"])
def test_other_batch_kinds(kind):
    """A retimed batch and a batch with three bound limit sets (each plan under its own a_max, j_max) against Y, n = 1000."""
    n = 1000
    ltp, dof, batch, full, lens, t_scaled = H.other_batch(kind, n)
    stopper = None
    if kind == "limit_sets":                         # H.other_batch's three sets on a second handle
        stopper, _, lim = H.planner("panda")
        scaled = [dict(lim, v_max=[f * x for x in lim["v_max"]], a_max=[f * x for x in lim["a_max"]], j_max=[f * x for x in lim["j_max"]])
                  for f in (1.0, 0.5, 0.25)]
        stopper.setLimitSets(*[np.array([s[key] for s in scaled], dtype=np.float64) for key in ("q_min", "q_max", "v_max", "a_max", "j_max")])
        assert np.array_equal(stopper._set_a_max, ltp._set_a_max)
    rng = np.random.default_rng(21)
    for gname in ("mpc", "geometric"):
        g = kc.GRIDS[gname]
        k = _uniform_starts(rng, lens)
        _assert_stop_knots(ltp, batch, k, g, 0, n, f"{kind} {gname}", stopper=stopper)
        first, count = H.odd_range(n, dof)
        _assert_stop_knots(ltp, batch, k, g, first, count, f"{kind} {gname} sub-range", stopper=stopper)


def test_a_stop_batch_as_input():
    """A stop batch is a planned batch: its stop horizons against Y."""
    n = 300
    ltp, dof, lim = H.planner("panda")
    qs = H.tensors(H.queries(lim, n))
    stop = ltp.planStopBatch(qs[1], qs[2], qs[3], check="inputs")
    lens = stop.traj_len.cpu().numpy()
    assert np.mean(lens > 0) > 0.9
    g = kc.GRIDS["mpc"]
    _assert_stop_knots(ltp, stop, _uniform_starts(np.random.default_rng(4), lens), g, 0, n, "stop batch")
    _assert_stop_knots(ltp, stop, 0, g, 5, n - 12, "stop batch, k = 0, sub-range")


@pytest.mark.parametrize("pow_rule", ["libm", "exact"])
def test_against_the_oracle(request, oracle_mod, pow_rule):
    """The oracle's optBraking (under LTP_POW_EXACT its exact-pow twin) applied on the host to the device's own knot states gives
    the device's bits, in both modes; a resting robot stops where it is in no time. (The knot states themselves are pinned to the
    oracle by tests/test_gpu_knots.py, so no tolerance enters here.)"""
    import torch
    if pow_rule == "libm":
        request.getfixturevalue("restated_host_libm")
    n = 64
    g = kc.GRIDS["mpc"]
    N = len(g)
    ltp, dof, lim = H.planner("panda", pow_rule)
    orc = oracle_mod.Oracle(dof, H.TS, exact_pow=(pow_rule == "exact"), **lim)
    batch = ltp.planSwitchTimesBatch(*H.tensors(H.queries(lim, n)))
    lens = batch.traj_len.cpu().numpy()
    k = torch.from_numpy(_uniform_starts(np.random.default_rng(8), lens)).to(DEV)
    rows, valid = ltp.sampleKnots(batch, 0, n, k, [int(x) for x in g])
    states = rows[..., :N].cpu().numpy()
    planned = lens > 0
    for clamp, accel in ((True, skc.CLAMP), (False, skc.STRICT)):
        got, v2 = ltp.stopKnots(batch, 0, n, k, [int(x) for x in g], clamp_acceleration=clamp)      # a host grid: uploaded by the wrapper
        got = got[..., :N].cpu().numpy()
        exp = skc.expected(orc, states, orc.a_max, accel)
        assert np.array_equal(np.ascontiguousarray(got[planned]).view(np.uint64), np.ascontiguousarray(exp[planned]).view(np.uint64)), (pow_rule, clamp)
        assert np.isnan(got[~planned]).all() and torch.equal(valid, v2)
    past = (np.maximum(k.cpu().numpy(), 0)[:, None] + g[None, :].astype(np.int64) >= lens[:, None]) & planned[:, None]
    assert past.any()
    rest = np.broadcast_to(past[:, None, :], got[:, 0].shape)
    assert np.array_equal(got[:, 0][rest], states[:, 0][rest]) and np.all(got[:, 1][rest] == 0.0)


def test_refusals():
    """Each refusal of the device entry is LTP_ERR_INVALID_ARGUMENT, its text names the reason, and the buffer keeps its pattern:
    the readers' common refusals, accel = 2, n_knots = 0 and 513, a NULL grid, MATLAB semantics. The host entry and both wrappers
    refuse a decreasing, a negative and a beyond-2^30 host grid before anything is launched."""
    import torch
    from longtermplanner_amd import _abi
    from longtermplanner_amd._abi import LtpError
    n = 64
    g = kc.GRIDS["mpc"]
    N = len(g)
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    O = _abi.StopKnotsOpts
    out = torch.full((n, 2, dof, ltp.windowRowStride(N)), H.PATTERN, dtype=torch.float64, device=DEV)
    big = torch.full((n, 2, dof, ltp.windowRowStride(kc.MAX_KNOTS + 1)), H.PATTERN, dtype=torch.float64, device=DEV)
    grid = _grid(np.concatenate([g, np.zeros(kc.MAX_KNOTS + 1 - N, dtype=np.int32) + int(g[-1])]))     # long enough for every n_knots tried
    call = H.reader_call(ltp._lib.ltp_stop_knots_batch, ltp, batch, n, out)
    good = dict(size=C.sizeof(O), n_knots=N, accel=0, knot_offsets=grid.data_ptr())
    assert ltp._lib.ltp_stop_knots_elements(ltp._h, n, N) == out.numel()
    H.common_refusals(ltp, batch, n, dof, call, O, good, out, out.numel() - 1, "ltp_stop_knots_elements")
    for bad, text in ((dict(knot_offsets=None), "knot_offsets is NULL"), (dict(n_knots=0), "n_knots"), (dict(n_knots=-1), "n_knots"),
                      (dict(n_knots=kc.MAX_KNOTS + 1), "LTP_MAX_KNOTS"), (dict(accel=2), "accel"), (dict(accel=-1), "accel")):
        rc, msg = call(O(**dict(good, **bad)), buf=big)
        assert rc == INVALID and text in msg, (bad, rc, msg)
    ltp.setSemantics("matlab")
    mat = ltp.planSwitchTimesBatch(*H.tensors(qs))
    rc, msg = H.reader_call(ltp._lib.ltp_stop_knots_batch, ltp, mat, n, out)(O(**good))
    assert rc == INVALID and "LTP_SEMANTICS_MATLAB" in msg, (rc, msg)
    with pytest.raises(LtpError) as e:
        ltp.planStopKnotsHost(*qs, 0, g)
    assert e.value.code == INVALID and "LTP_SEMANTICS_MATLAB" in str(e.value)
    ltp.setSemantics("cpp")
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    call = H.reader_call(ltp._lib.ltp_stop_knots_batch, ltp, batch, n, out)
    torch.cuda.synchronize()
    assert bool((out == H.PATTERN).all().item()) and bool((big == H.PATTERN).all().item()), "a refused call wrote to the buffer"
    # the largest admitted grid is a call like any other
    rc, msg = call(O(**dict(good, n_knots=kc.MAX_KNOTS)), buf=big)
    assert rc == 0, msg
    # host grids are looked at: the library's host entry and the wrapper refuse what breaks the contract, before any launch
    for bad, text in (([0, 5, 4, 9], "decreases"), ([-1, 0, 3], "negative"), ([0, (1 << 30) + 1], "beyond 2^30"), ([], ""),
                      (list(range(kc.MAX_KNOTS + 1)), "LTP_MAX_KNOTS")):
        with pytest.raises(LtpError) as e:
            ltp.planStopKnotsHost(*qs, 0, bad)
        assert e.value.code == INVALID and text in str(e.value), (bad, str(e.value))
        with pytest.raises(ValueError):
            ltp.stopKnots(batch, 0, n, 0, bad, out=out)
    with pytest.raises(LtpError) as e:
        ltp._plan_reader_host(ltp._lib.ltp_plan_stop_knots_host, qs, 0, (N, g.ctypes.data_as(C.POINTER(C.c_int)), 2), (2, dof, ltp.windowRowStride(N)))
    assert e.value.code == INVALID and "accel" in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == H.PATTERN).all().item()), "stopKnots wrote to the buffer although it refused its host grid"
    assert call(O(**good))[0] == 0


def test_graph_capture_and_replay_with_new_starts_and_a_new_grid():
    """The call allocates nothing: captured on one stream and replayed after first_sample AND the content of knot_offsets were
    rewritten in place, it gives what an eager call gives for the new starts and the new grid — twice, in both modes."""
    import torch
    n = 1000
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    rng = np.random.default_rng(77)
    ga = kc.GRIDS["mpc"]
    N = len(ga)
    gb = (np.arange(N) ** 2 // 2 + 3).astype(np.int32)             # another 40 knots: further out, g[0] = 3
    gc = np.sort(rng.integers(0, 2000, N)).astype(np.int32)
    ka, kb, kcs = (_uniform_starts(rng, lens) for _ in range(3))
    assert np.count_nonzero(ka != kb) > 0.5 * n
    R = ltp.windowRowStride(N)
    for clamp in (True, False):
        k, grid = torch.from_numpy(ka).to(DEV), _grid(ga)
        out = torch.zeros((n, 2, dof, R), dtype=torch.float64, device=DEV)
        valid = torch.zeros((n,), dtype=torch.int32, device=DEV)
        graph = H.capture(lambda: ltp.stopKnots(batch, 0, n, k, grid, clamp_acceleration=clamp, out=out, valid=valid))
        for k_new, g_new in ((kb, gb), (kcs, gc)):
            H.replay(graph, [(k, k_new), (grid, g_new)], out, valid)
            eager, eager_valid = ltp.stopKnots(batch, 0, n, k, grid, clamp_acceleration=clamp, out=torch.zeros_like(out))
            torch.cuda.synchronize()
            assert torch.equal(hc.int_view(eager), hc.int_view(out)) and torch.equal(eager_valid, valid)
            assert int((valid > 0).sum().item()) > 0.5 * n and bool(torch.isfinite(out[..., :N]).any().item())
    # the replayed result is the composition's
    _assert_stop_knots(ltp, batch, kcs, gc, 0, n, "the last replay's starts and grid")


DROPIN = r'''
#include "long_term_planner/long_term_planner.h"
#include <cstdio>
using namespace long_term_planner;
int main(int argc, char** argv) {
  const int dof = 7, n = 40, N = 40;
  std::vector<double> q_min = {-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973};
  std::vector<double> q_max = {2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973};
  std::vector<double> v_max = {2.175, 2.175, 2.175, 2.175, 2.61, 2.61, 2.61};
  std::vector<double> a_max = {15.0, 7.5, 10.0, 12.5, 15.0, 20.0, 20.0};
  std::vector<double> j_max = {7500.0, 3750.0, 5000.0, 6250.0, 7500.0, 10000.0, 10000.0};
  LongTermPlanner ltp(dof, 0.001, q_min, q_max, v_max, a_max, j_max);
  std::vector<double> in(4 * n * dof);
  std::vector<int> k(n), knots(N);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size() || std::fread(k.data(), sizeof(int), k.size(), f) != k.size() ||
      std::fread(knots.data(), sizeof(int), knots.size(), f) != knots.size()) return 2;
  std::fclose(f);
  std::vector<double> stop;
  std::vector<int> valid;
  BatchTrajectory b;
  const long long ok = ltp.planStopKnotsBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, knots, true, stop, &valid, &b);
  int refused = 0;
  for (const std::vector<int>& bad : {std::vector<int>{4, 3}, std::vector<int>{-1, 2}, std::vector<int>{0, (1 << 30) + 1}}) {
    try {
      std::vector<double> r2;
      ltp.planStopKnotsBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, bad, true, r2);
    } catch (const std::exception&) { ++refused; }
  }
  if (refused != 3) return 3;
  FILE* o = std::fopen(argv[2], "wb");
  std::fwrite(stop.data(), sizeof(double), stop.size(), o);
  std::fwrite(valid.data(), sizeof(int), valid.size(), o);
  std::fwrite(b.status.data(), sizeof(int), b.status.size(), o);
  std::fclose(o);
  std::printf("%lld ok, %zu doubles\n", ok, stop.size());
  return 0;
}
'''


def test_host_and_dropin_paths(tmp_path):
    """planStopKnotsHost equals the device path bitwise in both modes (elements [N, R) are zero there) and its status carries
    END_LIMIT like planBatchHost(sample=False); a small C++ program gives the same bytes through
    LongTermPlanner::planStopKnotsBatch and is refused a decreasing, a negative and a beyond-2^30 grid."""
    import torch
    n = 40
    g = kc.GRIDS["mpc"]
    N = len(g)
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    qs[0][3, 1] = 2.5                               # a goal beyond joint 1's range: planned, then END_LIMIT
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    lens = batch.traj_len.cpu().numpy()
    k = _uniform_starts(np.random.default_rng(1), lens)
    R = ltp.windowRowStride(N)
    assert R > N
    plain = ltp.planBatchHost(*qs, sample=False)
    for clamp in (True, False):
        dev_out, dev_valid = ltp.stopKnots(batch, 0, n, torch.from_numpy(k).to(DEV), _grid(g), clamp_acceleration=clamp,
                                           out=torch.zeros((n, 2, dof, R), dtype=torch.float64, device=DEV))
        dev_out, dev_valid = dev_out.cpu().numpy(), dev_valid.cpu().numpy()
        assert 0 < int((dev_valid > 0).sum()) and int((dev_valid < N).sum()) > 0
        rec, out, valid = ltp.planStopKnotsHost(*qs, k, g, clamp_acceleration=clamp)
        assert np.array_equal(out.view(np.uint8), dev_out.view(np.uint8)) and np.array_equal(valid, dev_valid)
        assert not out[..., N:].any()
        assert np.array_equal(rec["status"], plain["status"]) and (rec["status"][3] & 8) and np.array_equal(rec["traj_len"], lens)
        if clamp:
            host_clamp = (rec, out, valid)
    _, out_u, valid_u = ltp.planStopKnotsHost(*qs, 5, g)
    du, dv = ltp.stopKnots(batch, 0, n, 5, g, out=torch.zeros((n, 2, dof, R), dtype=torch.float64, device=DEV))
    assert np.array_equal(out_u.view(np.uint8), du.cpu().numpy().view(np.uint8)) and np.array_equal(valid_u, dv.cpu().numpy())

    rec, out, valid = host_clamp
    raw = H.run_dropin(tmp_path, "stop_knots", DROPIN, np.concatenate([x.reshape(-1) for x in qs]).astype(np.float64).tobytes()
                       + k.astype(np.int32).tobytes() + g.astype(np.int32).tobytes())
    H.assert_dropin_bytes(raw, out, valid, rec["status"])
