"""What the GPU tests of the two horizon-envelope calls share — the q-only ltp_envelope_knots_batch (tests/test_gpu_envelope_knots.py)
and ltp_envelope_knots_arrays_batch for q, v, a and j (tests/test_gpu_envelope_arrays.py) — a helper, not a test: the batch with its
rejected plan, the starts, the one assert against the reduced rows (tests/envelope_checker.py) and the tests whose body is the same
for either call. A call is described by a Reader (QONLY, ARRAYS); what differs beyond its names — the grids, the masks, the batch
size — is an argument of the shared test. The q-only call is the arrays call with mask q and no plane axis: its masks are (1,). The
batches and planner helpers are tests/horizon_helpers.py's and tests/gpu_helpers.py's."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

import envelope_checker as ec
import horizon_helpers as H
import knots_checker as kc
import run_census as rc
from gpu_helpers import _rows
from horizon_helpers import DEV, INVALID, PATTERN
from horizon_helpers import grid_tensor as _grid

REJECTED = 11                 # the plan every batch of _batch() has rejected: NaN envelopes among planned neighbours
GUARD = 16                    # the words of PATTERN on either side of a call's elements


class Reader(namedtuple("Reader", "call host_call dropin_call elements batch plan_host opts extra planes")):
    """One envelope call, every name in full: the wrapper's method, the Python host wrapper and the drop-in class's method; the C
    entries (the elements function, the device entry, the host entry); the options struct of longtermplanner_amd._abi and the
    fields a passing call sets beyond the q-only struct's; whether `arrays` is an argument and the results carry a plane axis."""

    def read(self, ltp, *args, **kw):
        return getattr(ltp, self.call)(*args, **kw)

    def read_host(self, ltp, *args, **kw):
        return getattr(ltp, self.host_call)(*args, **kw)

    def count(self, ltp, count, M, mask):
        return getattr(ltp._lib, self.elements)(ltp._h, count, M, *((mask,) if self.planes else ()))

    @property
    def every(self):
        """The mask of every array the call can give."""
        return 15 if self.planes else 1

    def shape(self, count, A, dof, M):
        return (count, A, dof, M, 2) if self.planes else (count, dof, M, 2)

    def by_plane(self, env):
        """env as [count, A, dof, M, 2]."""
        return env if self.planes else env[:, None]


QONLY = Reader(call="envelopeKnots", host_call="planEnvelopeKnotsHost", dropin_call="planEnvelopeKnotsBatch", elements="ltp_envelope_knots_elements",
               batch="ltp_envelope_knots_batch", plan_host="ltp_plan_envelope_knots_host", opts="EnvelopeKnotsOpts", extra={}, planes=False)
ARRAYS = Reader(call="envelopeKnotsArrays", host_call="planEnvelopeKnotsArraysHost", dropin_call="planEnvelopeKnotsArraysBatch",
                elements="ltp_envelope_knots_arrays_elements", batch="ltp_envelope_knots_arrays_batch", plan_host="ltp_plan_envelope_knots_arrays_host",
                opts="EnvelopeArraysOpts", extra=dict(arrays=15, reserved=0), planes=True)


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


def assert_envelopes(reader, ltp, batch, full, k_host, g, closed, first, count, what, masks, describe=None):
    """One call of the reader per mask over plans [first, first + count) with starts k_host[first:first + count] (an int: uniform),
    each plane compared with the reduced rows by its rule (envelope_checker.compare: q and v analytic, a and j equal); `valid`
    against its formula; a plan without a trajectory holds NaN; the buffer is exactly the elements function's count long between
    guard words, and those stay. describe: names the plans that miss their rule, given their mask over the whole batch. Returns
    ({mask: env}, {array: (worst |d|, bit-identical share)} over the masks)."""
    import torch
    M, dof = len(g) - 1, batch.dof
    if isinstance(k_host, (int, np.integer)):
        start = int(k_host)
        k = torch.full((count,), start, dtype=torch.int32, device=DEV)
    else:
        start = k = torch.from_numpy(np.ascontiguousarray(k_host[first:first + count])).to(DEV)
    union = 0
    for mask in masks:
        union |= mask
    red, exp_valid, planned = ec.expected(full, batch.offsets, batch.traj_len, k, g, closed, dof, first, count, mask=union)
    envs, figures = {}, {}
    grid = _grid(g)
    for mask in masks:
        planes = ec.selected(mask)
        need = count * len(planes) * dof * M * 2
        assert reader.count(ltp, count, M, mask) == need
        buf = torch.full((need + 2 * GUARD,), PATTERN, dtype=torch.float64, device=DEV)
        arrays = dict(arrays=mask) if reader.planes else {}          # the q-only call takes no mask: its only one is 1
        _, valid = reader.read(ltp, batch, first, count, start, grid, closed=closed, out=buf[GUARD:GUARD + need], **arrays)
        torch.cuda.synchronize()
        assert bool((buf[:GUARD] == PATTERN).all().item()) and bool((buf[GUARD + need:] == PATTERN).all().item()), \
            f"{what} mask {mask}: elements beside the call's were written"
        env = buf[GUARD:GUARD + need].view(count, len(planes), dof, M, 2)
        bad, fig = ec.compare(env, red[:, [ec.selected(union).index(x) for x in planes]].contiguous(), planned, mask)
        if bool(bad.any().item()):
            sel = np.zeros(batch.n, dtype=bool)
            sel[first:first + count] = bad.cpu().numpy()
            where = describe(sel) if describe else f"first local plan {int(bad.nonzero()[0].item())}"
            raise AssertionError(f"{what} mask {mask}: {int(bad.sum().item())} plans miss their rule ({fig}): {where}")
        assert torch.equal(valid, exp_valid), f"{what} mask {mask}: valid differs"
        assert bool(torch.isnan(env[~planned]).all().item()), f"{what} mask {mask}: a plan without a trajectory is not NaN"
        for name, (worst, share) in fig.items():
            w0, s0 = figures.get(name, (0.0, 1.0))
            figures[name] = (max(w0, worst), min(s0, share))
        envs[mask] = env if reader.planes else env[:, 0]
    return envs, figures


def _merged(reader, fig, fig2, share_word="bit-identical", later_word=None):
    """The printed figures of two asserts merged, per array: worst |d| and the smaller share; the q-only call names no array. The
    texts are the evidence the profiles compare from commit to commit, so they are spelt out here:
      QONLY                              "worst |d| 1.234e-16, bit-identical 0.999900"
      ARRAYS                             "q worst |d| 1.234e-16, bit-identical 0.999900; v worst |d| 0.000e+00, bit-identical 1.000000"
      QONLY,  "least ... share", "share" "worst |d| 1.234e-16, least bit-identical share 0.999900"
      ARRAYS, "least ... share", "share" "q worst |d| 1.234e-16, least bit-identical share 0.999900; v worst |d| 0.000e+00, share 1.000000"
    """
    return "; ".join(f"{x + ' ' if reader.planes else ''}worst |d| {max(fig[x][0], fig2[x][0]):.3e}, "
                     f"{share_word if x == 'q' or later_word is None else later_word} {min(fig[x][1], fig2[x][1]):.6f}" for x in fig)


# ---- the tests that are the same body with another reader

def reduced_rows(reader, name, n, pow_rule, grids, masks):
    """Every pair of every mask against the minimum and maximum of the samples sampleBatch wrote for its interval (past the end: the
    last position for q, 0 for v, a, j): q and v by the acceptance rule of the analytic form (NaN pattern identical, inside the
    samples, |d| <= 1e-12; q at least 0.999 bit-identical, the share of v printed), a and j equal. The whole batch (with its
    rejected plan) and a slice with first > 0 whose count * dof is no multiple of 64; starts per plan from [-5, traj_len + 40];
    both `closed` modes; `valid` against its formula."""
    ltp, dof, lim, qs, batch, full, lens = _batch(name, n, pow_rule)
    rng = np.random.default_rng(99)
    first, count = H.odd_range(n, dof)
    assert first > 0 and (count * dof) % 64 != 0 and first <= REJECTED < first + count
    L = lens.astype(np.int64)
    for gname in grids:
        g = ec.GRIDS[gname]
        assert gname != "max" or len(g) - 1 == ec.MAX_INTERVALS == 511
        for closed in (0, 1):
            k = _starts(rng, lens)
            kk = np.maximum(k.astype(np.int64), 0)
            ends, starts = float(np.mean((L > 0) & (kk + int(g[-1]) >= L))), float(np.mean((L > 0) & (kk + int(g[0]) >= L)))
            what = f"{name} {pow_rule} grid {gname} closed {closed}"
            envs, fig = assert_envelopes(reader, ltp, batch, full, k, g, closed, 0, n, f"{what} whole batch", masks)
            _, fig2 = assert_envelopes(reader, ltp, batch, full, k, g, closed, first, count, f"{what} plans [{first}, {first + count})", masks)
            q_share = min(fig["q"][1], fig2["q"][1])
            print(f"{what}: horizon ends past traj_len {ends:.3f}, starts there {starts:.3f}; {_merged(reader, fig, fig2)}")
            assert ends > 0.0 and q_share >= 0.999, (what, ends, q_share)
            for mask, env in envs.items():
                assert bool(np.isnan(env[REJECTED].cpu().numpy()).all()), (what, mask)


def smallest_shapes(reader, oracle_mod, name):
    """The run-census batches (rows of 1-153 samples, one-sample runs, collided switch indices, switching times on exact multiples
    of the sample time): unit, two-sample and duplicate-holding grids, both modes, a uniform k swept over 0 .. 8 and per-plan
    starts, every array of the reader in one call."""
    R = _rows(oracle_mod, name)
    ltp, batch, n, cen = R["ltp"], R["batch"], R["n"], R["cen"]
    lens = R["rec"]["traj_len"]
    rng = np.random.default_rng(17)
    M = 24
    grids = kc.SMALL_GRIDS
    assert list(grids) == ["unit", "two", "duplicates"] and np.array_equal(grids["unit"], np.arange(M + 1)) and np.array_equal(grids["two"], 2 * np.arange(M + 1))
    assert np.any(np.diff(grids["duplicates"]) == 0) and len(grids["duplicates"]) == M + 1
    describe = lambda mask: rc.describe(cen, mask)
    total = {}
    for gname, g in grids.items():
        for closed in (0, 1):
            for k in list(range(9)) + [_starts(rng, lens)]:
                what = f"{name} grid {gname} closed {closed} k {'per plan' if not isinstance(k, int) else k}"
                _, fig = assert_envelopes(reader, ltp, batch, R["full"], k, g.astype(np.int32), closed, 0, n, what, (reader.every,), describe)
                total = {x: (max(total.get(x, fig[x])[0], fig[x][0]), min(total.get(x, fig[x])[1], fig[x][1])) for x in fig}
    print(f"{name}: {_merged(reader, total, total, 'least bit-identical share', 'share')}")
    assert total["q"][1] >= 0.999, (name, total)


def agreement_with_the_knots_call(reader, gname, n):
    """lo <= the X sampleKnots stores at k + g[w] <= hi for every array and interval; with closed = 1 also at k + g[w + 1]; a
    duplicate interval (g[w] == g[w + 1]) equals that sample twice, q bit for bit."""
    import torch
    ltp, dof, lim, qs, batch, full, lens = _batch("panda", n)
    g = ec.GRIDS[gname]
    M = len(g) - 1
    k = torch.from_numpy(_starts(np.random.default_rng(8), lens)).to(DEV)
    rows, kv = ltp.sampleKnots(batch, 0, n, k, _grid(g))
    planned = batch.traj_len > 0
    x = rows[:, :len(ec.selected(reader.every)), :, :M + 1][planned]     # [plans, A, dof, M + 1]
    dup = torch.from_numpy(np.diff(g) == 0).to(DEV)
    for closed in (0, 1):
        env, valid = reader.read(ltp, batch, 0, n, k, _grid(g), closed=closed)
        torch.cuda.synchronize()
        e = reader.by_plane(env)[planned]
        assert bool(((e[..., 0] <= x[..., :M]) & (x[..., :M] <= e[..., 1])).all().item()), (gname, closed)
        if closed:
            assert bool(((e[..., 0] <= x[..., 1:]) & (x[..., 1:] <= e[..., 1])).all().item()), (gname, closed)
        if bool(dup.any().item()):
            twice = torch.stack([x[..., :M], x[..., :M]], dim=4)[:, :, :, dup]
            assert bool((e[:, :, :, dup] == twice).all().item()), (gname, closed)
            assert torch.equal(ec.int_view(e[:, 0][:, :, dup].contiguous()), ec.int_view(twice[:, 0].contiguous())), (gname, closed)
        # both calls count the intervals / knots that start inside the trajectory alike, but for the last edge
        last_real = ((k.long().clamp(min=0) + int(g[-1])) < batch.traj_len.long()).int()
        assert torch.equal(valid, kv - torch.where(planned, last_real, torch.zeros_like(last_real)))
    assert gname != "duplicates" or int(dup.sum().item()) >= 5


def other_batch_kinds(reader, kind, grids, sub_masks):
    """A retimed batch, a batch with three bound limit sets, MATLAB semantics (full rows from the walk sampler) and a stop batch:
    each against its own reduced rows on `grids`, both modes, every array of the reader, whole and a sub-range (there: sub_masks).
    A printed line names its grid where there is more than one."""
    if kind == "stop":
        n = 300
        ltp, dof, lim = H.planner("panda")
        qs = H.tensors(H.queries(lim, n))
        batch = ltp.planStopBatch(qs[1], qs[2], qs[3], check="inputs")
        full = H.full_rows(ltp, batch)
        lens = batch.traj_len.cpu().numpy()
        assert np.mean(lens > 0) > 0.9
    else:
        n = 1000
        ltp, dof, batch, full, lens, _ = H.other_batch(kind, n)
    rng = np.random.default_rng(21)
    first, count = H.odd_range(n, dof)
    for gname in grids:
        g = ec.GRIDS[gname]
        for closed in (0, 1):
            k = _starts(rng, lens)
            what = f"{kind} {gname + ' ' if len(grids) > 1 else ''}closed {closed}"
            _, fig = assert_envelopes(reader, ltp, batch, full, k, g, closed, 0, n, what, (reader.every,))
            _, fig2 = assert_envelopes(reader, ltp, batch, full, k, g, closed, first, count, f"{what} sub-range", sub_masks)
            print(f"{what}: {fig} {fig2}" if reader.planes else f"{what}: {_merged(reader, fig, fig2)}")
            assert min(fig["q"][1], fig2["q"][1]) >= 0.999


def refusals_and_bounds(reader, more_refusals=()):
    """Each refusal of the device entry is LTP_ERR_INVALID_ARGUMENT, its text names the reason, and the buffer it was given keeps
    its pattern; a geometry change after planning is refused in ltp_state_at_batch's words; guard words behind the call's elements
    stay intact; valid = NULL is accepted. Host edge lists outside the contract (and, where the call takes one, a bad `arrays`) are
    refused by the host entry (LtpError) and by the wrappers (ValueError) before any launch. more_refusals: (fields, text) pairs
    of the reader's own options fields. A reader with planes also has its capacity held against the mask's own element count."""
    import torch
    from longtermplanner_amd import _abi
    from longtermplanner_amd._abi import LtpError
    n = 64
    g = ec.GRIDS["mpc"]
    M = len(g) - 1
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    lib, O = ltp._lib, getattr(_abi, reader.opts)
    A = len(ec.selected(reader.every))
    need = n * A * dof * M * 2
    assert reader.count(ltp, n, M, reader.every) == need
    if reader.planes:
        assert reader.count(ltp, n, M, 5) == need // 2 and reader.count(ltp, n, M, 8) == need // 4
        assert reader.count(ltp, n, M, 0) == 0 and reader.count(ltp, n, M, 16) == 0
    guard = 64
    out = torch.full((need + guard,), PATTERN, dtype=torch.float64, device=DEV)
    big = torch.full((n * A * dof * (ec.MAX_INTERVALS + 1) * 2,), PATTERN, dtype=torch.float64, device=DEV)
    grid = _grid(np.concatenate([g, np.zeros(ec.MAX_INTERVALS + 2 - len(g), dtype=np.int32) + int(g[-1])]))     # long enough for every M tried
    call = H.reader_call(getattr(lib, reader.batch), ltp, batch, n, out, capacity=need)
    good = dict(size=C.sizeof(O), n_intervals=M, closed=1, edge_offsets=grid.data_ptr(), **reader.extra)          # valid = NULL
    status = batch.status.clone()
    rc_, msg = call(O(**good))
    assert rc_ == 0, msg
    torch.cuda.synchronize()
    want, _ = reader.read(ltp, batch, 0, n, 0, _grid(g), closed=True)
    torch.cuda.synchronize()
    assert torch.equal(ec.int_view(out[:need]), ec.int_view(want.reshape(-1))), "valid = NULL changes the envelopes"
    assert bool((out[need:] == PATTERN).all().item()), "the guard words behind the call's elements were written"
    assert torch.equal(batch.status, status)
    H.common_refusals(ltp, batch, n, dof, call, O, good, out, need - 1, reader.elements)
    for bad, text in ((dict(edge_offsets=None), "edge_offsets is NULL"), (dict(n_intervals=0), "n_intervals"), (dict(n_intervals=-1), "n_intervals"),
                      (dict(n_intervals=ec.MAX_INTERVALS + 1), "LTP_MAX_KNOTS - 1"), (dict(closed=2), "closed"), (dict(closed=-1), "closed"),
                      *more_refusals):
        rc_, msg = call(O(**dict(good, **bad)), buf=big, capacity=big.numel())
        assert rc_ == INVALID and text in msg, (bad, rc_, msg)
    if reader.planes:
        # the capacity is held against the mask's own element count
        rc_, msg = call(O(**dict(good, arrays=3)), capacity=need // 2 - 1)
        assert rc_ == INVALID and reader.elements in msg
    torch.cuda.synchronize()
    assert bool((out == PATTERN).all().item()) and bool((big == PATTERN).all().item()), "a refused call wrote to the buffer"
    if reader.planes:
        rc_, msg = call(O(**dict(good, arrays=3)), capacity=need // 2)
        assert rc_ == 0, msg
        torch.cuda.synchronize()
        assert bool((out[need // 2:] == PATTERN).all().item()), "a two-array call wrote beyond its elements"
        out.fill_(PATTERN)
    # the largest admitted grid is a call like any other
    rc_, msg = call(O(**dict(good, n_intervals=ec.MAX_INTERVALS)), buf=big, capacity=big.numel())
    assert rc_ == 0, msg
    torch.cuda.synchronize()
    assert bool((big[n * A * dof * ec.MAX_INTERVALS * 2:] == PATTERN).all().item())
    # host edge lists and `arrays` are looked at: the library's host entry and the wrappers refuse, before any launch
    env_out = out[:need].view(reader.shape(n, A, dof, M))
    for bad, text in (([0, 5, 4, 9], "decreases"), ([-1, 0, 3], "negative"), ([0, (1 << 30) + 1], "beyond 2^30"), ([], "n_intervals"),
                      ([11], "n_intervals"), (list(range(ec.MAX_INTERVALS + 2)), "LTP_MAX_KNOTS")):
        with pytest.raises(LtpError) as e:
            reader.read_host(ltp, *qs, 0, bad)
        assert e.value.code == INVALID and text in str(e.value), (bad, str(e.value))
        with pytest.raises(ValueError):
            reader.read(ltp, batch, 0, n, 0, bad, out=env_out)
    if reader.planes:
        g3 = (C.c_int * 3)(0, 4, 9)
        for arrays in (0, 16, -3):
            rc_ = getattr(lib, reader.plan_host)(ltp._h, n, *[x.ctypes.data_as(C.POINTER(C.c_double)) for x in qs], None, 0, 2, g3, 0, arrays, None,
                                                 np.zeros(8).ctypes.data_as(C.POINTER(C.c_double)), None)
            assert rc_ == INVALID and "arrays" in (lib.ltp_last_error(ltp._h) or b"").decode()
            with pytest.raises(ValueError):
                reader.read(ltp, batch, 0, n, 0, [0, 4, 9], arrays=arrays, out=env_out)
    with pytest.raises(ValueError):
        reader.read_host(ltp, *qs, 0, [0.5, 1.5])
    torch.cuda.synchronize()
    assert bool((out == PATTERN).all().item()), f"{reader.call} wrote to the buffer although it refused its arguments"
    assert call(O(**good))[0] == 0


DROPIN = r'''
#include "long_term_planner/long_term_planner.h"
#include <cstdio>
using namespace long_term_planner;
#define QUERIES n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0
ARRAYS_MACRO
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
  const long long ok = ltp.PLAN_BATCH(QUERIES, edges, true, ARRAYS(LTP_ENV_Q | LTP_ENV_V | LTP_ENV_J) env, &valid, &b);
  int refused = 0;
  MORE_REFUSALS
  for (const std::vector<int>& bad : {std::vector<int>{4, 3}, std::vector<int>{7}, std::vector<int>{}}) {
    try {
      std::vector<double> e2;
      ltp.PLAN_BATCH(QUERIES, bad, false, ARRAYS(LTP_ENV_V) e2);
    } catch (const std::exception&) { ++refused; }
  }
  if (refused != N_REFUSED) return 3;
  FILE* o = std::fopen(argv[2], "wb");
  std::fwrite(env.data(), sizeof(double), env.size(), o);
  std::fwrite(valid.data(), sizeof(int), valid.size(), o);
  std::fwrite(b.status.data(), sizeof(int), b.status.size(), o);
  std::fclose(o);
  std::printf("%lld ok, %zu doubles\n", ok, env.size());
  return 0;
}
'''


def host_and_dropin_paths(reader, tmp_path, refused, more_refusals=""):
    """The host wrapper equals the device path bitwise and its status carries END_LIMIT like planBatchHost(sample=False); a small
    C++ program gives the same bytes through the drop-in class's method (dropin_call). A reader with planes is asked for q, v and j
    (by name on the device, by mask on the host). more_refusals: C++ text of further calls the drop-in method must refuse, each
    adding to `refused`; refused: how many refusals the program counts in all."""
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
    by_name, by_mask, A = (dict(arrays="qvj"), dict(arrays=11), 3) if reader.planes else ({}, {}, 1)
    dev_env, dev_valid = reader.read(ltp, batch, 0, n, torch.from_numpy(k).to(DEV), _grid(g), closed=True, **by_name)
    dev_env, dev_valid = dev_env.cpu().numpy(), dev_valid.cpu().numpy()
    assert 0 < int((dev_valid > 0).sum()) and int((dev_valid < M).sum()) > 0
    assert not (batch.status.cpu().numpy()[3] & 8), "the device call forms no end-limit verdict"
    rec, env, valid = reader.read_host(ltp, *qs, k, g, closed=True, **by_mask)
    assert env.shape == reader.shape(n, A, dof, M)
    assert np.array_equal(env.view(np.uint8), dev_env.view(np.uint8)) and np.array_equal(valid, dev_valid)
    plain = ltp.planBatchHost(*qs, sample=False)
    assert np.array_equal(rec["status"], plain["status"]) and (rec["status"][3] & 8) and np.array_equal(rec["traj_len"], lens)
    _, env_u, valid_u = reader.read_host(ltp, *qs, 5, [int(x) for x in g])
    du, dv = reader.read(ltp, batch, 0, n, 5, g)                                   # a host grid: uploaded by the wrapper
    assert env_u.shape == reader.shape(n, 4, dof, M)
    assert np.array_equal(env_u.view(np.uint8), du.cpu().numpy().view(np.uint8)) and np.array_equal(valid_u, dv.cpu().numpy())

    source = (DROPIN.replace("ARRAYS_MACRO", "#define ARRAYS(mask) mask," if reader.planes else "#define ARRAYS(mask)")
              .replace("PLAN_BATCH", reader.dropin_call).replace("MORE_REFUSALS", more_refusals).replace("N_REFUSED", str(refused)))
    raw = H.run_dropin(tmp_path, reader.call, source, np.concatenate([x.reshape(-1) for x in qs]).astype(np.float64).tobytes()
                       + k.astype(np.int32).tobytes() + g.astype(np.int32).tobytes())
    H.assert_dropin_bytes(raw, env, valid, rec["status"])


def graph_capture_and_replay(reader):
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
    out = torch.zeros(reader.shape(n, 4, dof, E - 1), dtype=torch.float64, device=DEV)
    valid = torch.zeros((n,), dtype=torch.int32, device=DEV)
    graph = H.capture(lambda: reader.read(ltp, batch, 0, n, k, grid, closed=True, out=out, valid=valid))
    for k_new, g_new in ((kb, gb), (kcs, gc)):
        H.replay(graph, [(k, k_new), (grid, g_new)], out, valid)
        direct, direct_valid = reader.read(ltp, batch, 0, n, k, grid, closed=True)
        torch.cuda.synchronize()
        assert torch.equal(ec.int_view(direct), ec.int_view(out)) and torch.equal(direct_valid, valid)
        red, exp_valid, planned = ec.expected(full, batch.offsets, batch.traj_len, k, g_new, 1, dof, 0, n, mask=reader.every)
        bad, fig = ec.compare(reader.by_plane(out), red, planned, reader.every)
        assert not bool(bad.any().item()) and torch.equal(valid, exp_valid), fig
