"""Knot-grid horizons (ltp_sample_knots_batch, include/ltp_hip.h) on the GPU: element w of a row is trajectory sample k + g[w].
Compared with the rows the full-row sampler wrote for the same batch (tests/horizon_checker.py, itself pinned to a plain loop by
tests/test_knots_cpu.py), with the strided and the window call on the uniform grids, and with the oracle; grids that need more
passes than one, float32, other batch kinds, refusals, the host and drop-in paths and graph capture with a rewritten grid. The
batches, their sizes and the planner helpers are tests/horizon_helpers.py's."""
import ctypes as C

import numpy as np
import pytest

import horizon_checker as hc
import horizon_helpers as H
import knots_checker as kc
from horizon_helpers import DEV, INVALID
from horizon_helpers import grid_tensor as _grid

pytestmark = pytest.mark.gpu


def _starts(rng, lens, t_scaled, g):
    """hc.draw_starts over the span of the grid, g[N-1] + 1 samples."""
    return hc.draw_starts(rng, lens, t_scaled, int(g[-1]) + 1, 1)


def _assert_knots(ltp, batch, full, k_host, g, first, count, what, dtype=None):
    """One knots call over plans [first, first + count) with starts k_host[first:first + count], compared with the full rows. The
    buffer is pre-filled with a pattern: elements [N, R) of a row must keep it."""
    return H.assert_rows(lambda k, out: ltp.sampleKnots(batch, first, count, k, _grid(g), out=out), ltp, batch, full, k_host, g, first, count,
                         what, dtype)


@pytest.mark.parametrize("name,n,pow_rule", [("panda", 3000, "libm"), ("panda", 3000, "exact"), ("ref", 2000, "libm"), ("ref", 2000, "exact"),
                                             ("ref30", 300, "libm"), ("ref30", 300, "exact")])
def test_bits_against_full_rows(name, n, pow_rule):
    """Every real element of every horizon has the bits of the row sampleBatch wrote at k + g[w], every element past the end follows
    the hold rule, `valid` follows its formula — no plan excepted; at first = 0, count = n and at a sub-range whose count * dof is
    no multiple of 64. The coverage conditions are asserted first, the skipped-stretch share (>= 0.30) for the MPC and the geometric
    grid on every batch. With the uniform draw over the grid's span one combination cannot reach it: the "ref" batch under the MPC
    grid has 0.25, because its stretches are several times longer than that grid's 240 samples (a property of the limits, not of
    the draw's seed). So those two grids are compared a second time on every batch from kc.aimed_starts, which puts a stretch
    between two consecutive knots wherever a plan has one that fits, and the share is asserted there for every batch and both
    grids (the CPU oracle's plans give 0.99 to 1.00); on the uniform draw it is asserted everywhere but for ("ref", MPC)."""
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch(name, n, pow_rule)
    rng = np.random.default_rng(99)
    assert set(kc.GRIDS) == {"mpc", "geometric", "duplicates", "from37", "one", "n33", "n65", "max"}
    assert len(kc.GRIDS["mpc"]) == 40 and 50 <= len(kc.GRIDS["geometric"]) <= 60 and kc.GRIDS["geometric"][-1] == 4096
    assert kc.GRIDS["from37"][0] == 37 and np.any(np.diff(kc.GRIDS["duplicates"]) == 0)
    assert [len(kc.GRIDS[x]) for x in ("one", "n33", "n65", "max")] == [1, 33, 65, kc.MAX_KNOTS] and np.all(np.diff(kc.GRIDS["max"]) == 8)
    for gname, g in kc.GRIDS.items():
        what = f"{name} {pow_rule} grid {gname}"
        k = _starts(rng, lens, t_scaled, g)
        planned, ends, starts, skipped = kc.coverage(k, g, lens, t_scaled)
        print(f"{what}: planned {planned:.3f}, ends {ends:.3f}, starts {starts:.3f}, skipped {skipped:.3f}")
        assert planned >= 0.95 and ends >= 0.10 and starts >= 0.03, (what, planned, ends, starts)
        if gname in ("mpc", "geometric") and (name, gname) != ("ref", "mpc"):
            assert skipped >= 0.30, (what, skipped)
        _assert_knots(ltp, batch, full, k, g, 0, n, f"{what} whole batch")
        first, count = H.odd_range(n, dof)
        assert (count * dof) % 64 != 0
        _assert_knots(ltp, batch, full, k, g, first, count, f"{what} plans [{first}, {first + count})")
        if gname in ("mpc", "geometric"):
            ka = kc.aimed_starts(k, g, lens, t_scaled)
            aimed = kc.coverage(ka, g, lens, t_scaled)[3]
            print(f"{what}, aimed starts: skipped {aimed:.3f}, starts changed {float(np.mean(ka != k)):.3f}")
            assert aimed >= 0.30, (what, aimed)
            _assert_knots(ltp, batch, full, ka, g, 0, n, f"{what} aimed starts, whole batch")
            _assert_knots(ltp, batch, full, ka, g, first, count, f"{what} aimed starts, plans [{first}, {first + count})")


@pytest.mark.parametrize("N,s", [(32, 10), (33, 3), (64, 5), (32, 1), (33, 1), (100, 1)])
def test_uniform_grids_are_the_existing_calls(N, s):
    """g[w] = w * s gives the buffer and `valid` of sampleHorizon(N, s), padding included; g[w] = w those of sampleWindow(N)."""
    import torch
    n = 3000
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    k = torch.from_numpy(hc.draw_starts(np.random.default_rng(12), lens, t_scaled, N, s)).to(DEV)
    R = ltp.windowRowStride(N)
    fresh = lambda: torch.full((n, 4, dof, R), H.PATTERN, dtype=torch.float64, device=DEV)
    if s == 1:
        a, va = ltp.sampleWindow(batch, 0, n, k, N, out=fresh())
    else:
        a, va = ltp.sampleHorizon(batch, 0, n, k, N, s, out=fresh())
    b, vb = ltp.sampleKnots(batch, 0, n, k, _grid(np.arange(N) * s), out=fresh())
    torch.cuda.synchronize()
    assert torch.equal(hc.int_view(a), hc.int_view(b)) and torch.equal(va, vb)
    assert int((va > 0).sum().item()) > 0.5 * n


def test_more_passes_than_one():
    """S-ref limits, k = 0, a geometric grid that reaches over whole trajectories: at least a quarter of the plans have a joint whose
    knots fall into more than 6 stretches, more than a lane parks in one pass."""
    n = 500
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("ref", n)
    g = kc.wide_grid()
    assert 140 <= len(g) <= 160 and g[0] == 0 and g[-1] == 5999
    k = np.zeros(n, dtype=np.int32)
    share = float(np.mean(kc.stretches(k, g, lens, t_scaled) > 6))
    print(f"more than 6 stretches with a knot: {share:.3f} of the plans")
    assert share >= 0.25, share
    _assert_knots(ltp, batch, full, k, g, 0, n, "wide grid, k = 0")
    _assert_knots(ltp, batch, full, k, g, 3, n - 10, "wide grid, sub-range")


@pytest.mark.parametrize("grid", ["mpc", "geometric"])
def test_float32_knots(grid):
    """float32 horizons are the float64 horizons rounded once, and equal the float32 sampler's rows where the sample is real."""
    import torch
    n = 2000
    g = kc.GRIDS[grid]
    N = len(g)
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    k = _starts(np.random.default_rng(5), lens, t_scaled, g)
    r64, v64 = _assert_knots(ltp, batch, full, k, g, 0, n, f"f64 {grid}")
    full32 = H.full_rows(ltp, batch, torch.float32)
    r32, v32 = _assert_knots(ltp, batch, full32, k, g, 0, n, f"f32 {grid}", dtype=torch.float32)
    assert torch.equal(v32, v64)
    planned = batch.traj_len > 0
    a, b = r32[planned][..., :N], r64[planned][..., :N].to(torch.float32)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "float32 horizon is not (float) of the float64 horizon"


def test_knots_against_the_oracle(oracle_mod):
    """q, v, a and j of the real elements against the CPU oracle's own trajectories at k + g[w], 1e-9 (the project's parity bar)."""
    import torch
    n = 200
    g = kc.GRIDS["mpc"]
    N = len(g)
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    orc = oracle_mod.Oracle(dof, H.TS, **lim)
    o = orc.plan_batch(*qs, sample=True)
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    lens = batch.traj_len.cpu().numpy()
    assert np.array_equal(lens, o["traj_len"])
    k = _starts(np.random.default_rng(3), lens, batch.t_scaled.cpu().numpy(), g)
    rows, valid = ltp.sampleKnots(batch, 0, n, torch.from_numpy(k).to(DEV), [int(x) for x in g])      # a host grid: uploaded by the wrapper
    rows, valid = rows.cpu().numpy()[..., :N], valid.cpu().numpy()
    worst, checked, n_real, n_all = 0.0, 0, 0, 0
    for p in range(n):
        if o["status"][p] == 0:
            continue
        L, q, v, a, j = orc.get_trajectory(o["t_scaled"][p], o["dir"][p], o["mod"][p], qs[1][p], qs[2][p], qs[3][p], o["v_drive"][p])
        t = max(int(k[p]), 0) + g.astype(np.int64)
        real = t < L
        assert valid[p] == real.sum()
        for arr, ref in enumerate((q, v, a, j)):
            if real.any():
                worst = max(worst, float(np.max(np.abs(rows[p, arr][:, real] - ref[:, t[real]]))))
        n_real += int(real.sum())
        n_all += N
        checked += 1
    print(f"oracle: {checked} plans, {n_real} of {n_all} elements real, worst {worst:.3e}")
    assert checked > 0.95 * n and 2 * n_real >= n_all and worst <= 1e-9, (checked, n_real, n_all, worst)


@pytest.mark.parametrize("kind", ["retimed", "limit_sets", "matlab"])
def test_other_batch_kinds(kind):
    """A retimed batch, a batch with three bound limit sets, MATLAB semantics (full rows from the walk sampler): the bit comparison
    of test_bits_against_full_rows, n = 1000, on the MPC and the geometric grid."""
    n = 1000
    ltp, dof, batch, full, lens, t_scaled = H.other_batch(kind, n)
    rng = np.random.default_rng(21)
    for gname in ("mpc", "geometric"):
        g = kc.GRIDS[gname]
        k = _starts(rng, lens, t_scaled, g)
        print(kind, gname, "planned / ends / starts / skipped:", kc.coverage(k, g, lens, t_scaled))
        _assert_knots(ltp, batch, full, k, g, 0, n, f"{kind} {gname}")
        first, count = H.odd_range(n, dof)
        _assert_knots(ltp, batch, full, k, g, first, count, f"{kind} {gname} sub-range")


def test_refusals():
    """Each refusal of the device entry is LTP_ERR_INVALID_ARGUMENT, its text names the reason, and the buffer it was given keeps its
    pattern. A host grid outside the contract is refused by ltp_plan_knots_host (LtpError with the grid's fault: the text comes from
    the entry's prologue, which runs before anything is staged or launched; the entry has no caller's device buffer that could show
    more) and by sampleKnots given a host list (ValueError before the library is called: the buffer check below covers that path)."""
    import torch
    from longtermplanner_amd import _abi
    n = 64
    g = kc.GRIDS["mpc"]
    N = len(g)
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    O = _abi.KnotsOpts
    out = torch.full((n, 4, dof, ltp.windowRowStride(N)), H.PATTERN, dtype=torch.float64, device=DEV)
    big = torch.full((n, 4, dof, ltp.windowRowStride(kc.MAX_KNOTS + 1)), H.PATTERN, dtype=torch.float64, device=DEV)
    grid = _grid(np.concatenate([g, np.zeros(kc.MAX_KNOTS + 1 - N, dtype=np.int32) + int(g[-1])]))     # long enough for every n_knots tried
    call = H.reader_call(ltp._lib.ltp_sample_knots_batch, ltp, batch, n, out)
    good = dict(size=C.sizeof(O), format=0, n_knots=N, knot_offsets=grid.data_ptr())
    H.common_refusals(ltp, batch, n, dof, call, O, good, out, out.numel() - 1, "ltp_window_elements")
    for bad, text in ((dict(knot_offsets=None), "knot_offsets is NULL"), (dict(n_knots=0), "n_knots"), (dict(n_knots=-1), "n_knots"),
                      (dict(n_knots=kc.MAX_KNOTS + 1), "LTP_MAX_KNOTS"), (dict(format=2), "format")):
        rc, msg = call(O(**dict(good, **bad)), buf=big)
        assert rc == INVALID and text in msg, (bad, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == H.PATTERN).all().item()) and bool((big == H.PATTERN).all().item()), "a refused call wrote to the buffer"
    # the largest admitted grid is a call like any other
    rc, msg = call(O(**dict(good, n_knots=kc.MAX_KNOTS)), buf=big)
    assert rc == 0, msg
    # host grids are looked at: the library's host entry and the wrapper refuse what breaks the contract, before any launch
    from longtermplanner_amd._abi import LtpError
    for bad, text in (([0, 5, 4, 9], "decreases"), ([-1, 0, 3], "negative"), ([0, (1 << 30) + 1], "beyond 2^30"), ([], ""),
                      (list(range(kc.MAX_KNOTS + 1)), "LTP_MAX_KNOTS")):
        with pytest.raises(LtpError) as e:
            ltp.planKnotsHost(*qs, 0, bad)
        assert e.value.code == INVALID and text in str(e.value), (bad, str(e.value))
        with pytest.raises(ValueError):
            ltp.sampleKnots(batch, 0, n, 0, bad, out=out)
    torch.cuda.synchronize()
    assert bool((out == H.PATTERN).all().item()), "sampleKnots wrote to the buffer although it refused its host grid"
    for bad in ([0.5, 1.5], [[0, 1], [2, 3]], [0, 1 << 40]):            # not integers, not a list, beyond an int: the wrapper's own refusals
        with pytest.raises((ValueError, LtpError)):
            ltp.planKnotsHost(*qs, 0, bad)
    with pytest.raises(ValueError):
        ltp.planKnotsHost(*qs, 0, [0.5, 1.5])
    assert call(O(**good))[0] == 0


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
  std::vector<double> rows;
  std::vector<int> valid;
  BatchTrajectory b;
  const long long ok = ltp.planKnotsBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, knots, rows, &valid, &b);
  int refused = 0;
  try {
    std::vector<double> r2;
    ltp.planKnotsBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, std::vector<int>{4, 3}, r2);
  } catch (const std::exception&) { refused = 1; }
  if (!refused) return 3;
  FILE* o = std::fopen(argv[2], "wb");
  std::fwrite(rows.data(), sizeof(double), rows.size(), o);
  std::fwrite(valid.data(), sizeof(int), valid.size(), o);
  std::fwrite(b.status.data(), sizeof(int), b.status.size(), o);
  std::fclose(o);
  std::printf("%lld ok, %zu doubles\n", ok, rows.size());
  return 0;
}
'''


def test_host_and_dropin_paths(tmp_path):
    """planKnotsHost equals the device path bitwise (elements [N, R) are zero there) and its status carries END_LIMIT like
    planBatchHost(sample=False); a small C++ program gives the same bytes through LongTermPlanner::planKnotsBatch."""
    import torch
    n = 40
    g = kc.GRIDS["mpc"]
    N = len(g)
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    qs[0][3, 1] = 2.5                               # a goal beyond joint 1's range: planned, then END_LIMIT
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    lens = batch.traj_len.cpu().numpy()
    k = _starts(np.random.default_rng(1), lens, batch.t_scaled.cpu().numpy(), g)
    R = ltp.windowRowStride(N)
    assert R > N
    dev_rows, dev_valid = ltp.sampleKnots(batch, 0, n, torch.from_numpy(k).to(DEV), _grid(g), out=torch.zeros((n, 4, dof, R), dtype=torch.float64, device=DEV))
    dev_rows, dev_valid = dev_rows.cpu().numpy(), dev_valid.cpu().numpy()
    assert 0 < int((dev_valid > 0).sum()) and int((dev_valid < N).sum()) > 0
    rec, rows, valid = ltp.planKnotsHost(*qs, k, g)
    assert np.array_equal(rows.view(np.uint8), dev_rows.view(np.uint8)) and np.array_equal(valid, dev_valid)
    assert not rows[..., N:].any()
    plain = ltp.planBatchHost(*qs, sample=False)
    assert np.array_equal(rec["status"], plain["status"]) and (rec["status"][3] & 8) and np.array_equal(rec["traj_len"], lens)
    _, rows_u, valid_u = ltp.planKnotsHost(*qs, 5, g)
    du, dv = ltp.sampleKnots(batch, 0, n, 5, g, out=torch.zeros((n, 4, dof, R), dtype=torch.float64, device=DEV))
    assert np.array_equal(rows_u.view(np.uint8), du.cpu().numpy().view(np.uint8)) and np.array_equal(valid_u, dv.cpu().numpy())

    raw = H.run_dropin(tmp_path, "knots", DROPIN, np.concatenate([x.reshape(-1) for x in qs]).astype(np.float64).tobytes() + k.astype(np.int32).tobytes()
                       + g.astype(np.int32).tobytes())
    H.assert_dropin_bytes(raw, rows, valid, rec["status"])


def test_graph_capture_and_replay_with_new_starts_and_a_new_grid():
    """The call allocates nothing: captured on one stream (one kernel node) and replayed after first_sample AND the content of
    knot_offsets were rewritten in place, it gives what an eager call gives for the new starts and the new grid — twice."""
    import torch
    n = 1000
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    rng = np.random.default_rng(77)
    ga = kc.GRIDS["mpc"]
    N = len(ga)
    gb = (np.arange(N) ** 2 // 2 + 3).astype(np.int32)             # another 40 knots: further out, g[0] = 3
    gc = np.sort(rng.integers(0, 2000, N)).astype(np.int32)
    ka, kb, kcs = (_starts(rng, lens, t_scaled, x) for x in (ga, gb, gc))
    assert np.count_nonzero(ka != kb) > 0.5 * n
    R = ltp.windowRowStride(N)
    k, grid = torch.from_numpy(ka).to(DEV), _grid(ga)
    out = torch.zeros((n, 4, dof, R), dtype=torch.float64, device=DEV)
    valid = torch.zeros((n,), dtype=torch.int32, device=DEV)
    graph = H.capture(lambda: ltp.sampleKnots(batch, 0, n, k, grid, out=out, valid=valid))
    for k_new, g_new in ((kb, gb), (kcs, gc)):
        H.replay(graph, [(k, k_new), (grid, g_new)], out, valid)
        exp, exp_valid, planned = hc.expected(full, batch.offsets, batch.traj_len, k, g_new, dof, 0, n)
        assert torch.equal(out.view(torch.int64)[..., :N][planned], exp[planned]) and torch.equal(valid, exp_valid)
        assert bool(torch.isnan(out[~planned][..., :N]).all().item())
        eager, eager_valid = ltp.sampleKnots(batch, 0, n, k, grid, out=torch.zeros_like(out))
        torch.cuda.synchronize()
        assert torch.equal(hc.int_view(eager), hc.int_view(out)) and torch.equal(eager_valid, valid)
