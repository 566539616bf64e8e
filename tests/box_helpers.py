"""What the GPU tests of the two box readers share — first exits (ltp_first_exit_batch, tests/test_gpu_first_exit.py) and settling
(ltp_settle_batch, tests/test_gpu_settle.py) — a helper, not a test: the batch with its rejected plan, the starts, the one assert
against the exhaustive scan (tests/box_checker.py) and the tests whose body is the same for either reader. A reader is described by a
Reader (EXITS, SETTLE); what differs beyond its names — the families of boxes, an expectation about the answers — is an argument of
the shared test. The batches and planner helpers are tests/horizon_helpers.py's and tests/gpu_helpers.py's."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

import box_checker as bx
import horizon_helpers as H
import run_census as rc
from envelope_checker import selected
from gpu_helpers import _rows
from horizon_helpers import DEV, INVALID

REJECTED = 11                 # the plan every batch of _batch() has rejected: LTP_EXIT_NO_PLAN among planned neighbours
MASKS = ("q", "v", "qv", "aj", "qvaj")
HORIZONS = (1, 2, 64, 240, 1 << 30)
GUARD = -77                   # what a buffer holds before a call that must not write (all of) it
LETTERS = "qvaj"


class Reader(namedtuple("Reader", "call fold_kw elements batch plan_host opts host_call dropin_call expected fold fold_name")):
    """One box reader, every name in full: the wrapper's method and the keyword of its per-plan fold; the C entries (the elements
    function, the device entry, the host entry) and the options struct of longtermplanner_amd._abi; the Python host wrapper and the
    drop-in class's method; the checker's scan and fold; the name of the fold (the options' last field, the noun of messages)."""

    def read(self, ltp, *args, fold=False, **kw):
        return getattr(ltp, self.call)(*args, **{self.fold_kw: fold}, **kw)

    def read_host(self, ltp, *args, fold=False, **kw):
        return getattr(ltp, self.host_call)(*args, **{self.fold_kw: fold}, **kw)

    def count(self, ltp, count, mask):
        return getattr(ltp._lib, self.elements)(ltp._h, count, mask)


EXITS = Reader(call="firstExit", fold_kw="any", elements="ltp_first_exit_elements", batch="ltp_first_exit_batch", plan_host="ltp_plan_first_exit_host",
               opts="FirstExitOpts", host_call="planFirstExitHost", dropin_call="planFirstExitBatch", expected=bx.expected_exits, fold=bx.fold_any,
               fold_name="first_any")
SETTLE = Reader(call="settle", fold_kw="all", elements="ltp_settle_elements", batch="ltp_settle_batch", plan_host="ltp_plan_settle_host",
                opts="SettleOpts", host_call="planSettleHost", dropin_call="planSettleBatch", expected=bx.expected_settle, fold=bx.fold_all,
                fold_name="settle_all")


_CACHE = {}


def _batch(name, n, pow_rule="libm", ends=False):
    """H.batch with one rejected plan (a start velocity no limit admits) and the row ranges of every plan — (ltp, dof, lim, qs,
    batch, full, lens, mn, mx) — and, with ends, the boxes around every row's resting value as a tenth; the latest one is kept."""
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
        mn, mx = bx.row_ranges(full, batch.offsets, batch.traj_len, dof, 0, n)
        torch.cuda.synchronize()
        _CACHE.update(key=key, v=(ltp, dof, lim, qs, batch, full, lens, mn, mx))
    if not ends:
        return _CACHE["v"]
    if "ends" not in _CACHE:
        ltp, dof, lim, qs, batch, full = _CACHE["v"][:6]
        _CACHE["ends"] = bx.end_boxes(full, batch.offsets, batch.traj_len, dof, seed=8)
        torch.cuda.synchronize()
    return _CACHE["v"] + (_CACHE["ends"],)


def _starts(rng, lens):
    """k per plan, uniform in [-3, traj_len + 3]."""
    return rng.integers(-3, lens.astype(np.int64) + 4).astype(np.int32)


def _sides(mask, box4):
    """The dict by array letter the readers take, from a box tensor [count, 4, dof] (None: the default on that side)."""
    if box4 is None:
        return None
    return {LETTERS[x]: box4[:, x].contiguous() for x in selected(mask)}


def _mask_of(arrays):
    from longtermplanner_amd import LongTermPlanner
    return LongTermPlanner._env_arrays(arrays)


def _samples(full, batch, n, dof, extra=1):
    """S_X(t) of every row for t in [0, max traj_len + extra): [n, 4, dof, span], the columns from traj_len on the resting state."""
    import torch
    L = batch.traj_len[:n].long()
    span = int(L.max().item()) + extra
    t = torch.arange(span, device=DEV)[None, :].expand(n, span)
    return bx._gather(full, batch.offsets[:n].long(), L, dof, t)


def assert_reads(reader, ltp, batch, full, k_host, horizon, first, count, lo4, hi4, what, masks=MASKS, describe=None):
    """One call of the reader per mask over plans [first, first + count) with starts k_host[first:first + count] (an int: uniform)
    and the boxes lo4 / hi4 [count, 4, dof], every int of the table and of the fold EQUAL to the checker's; the buffer is exactly the
    call's elements long between guard words, and those stay. Returns {mask: (table, fold)}."""
    import torch
    dof = batch.dof
    if isinstance(k_host, (int, np.integer)):
        start = int(k_host)
        k = torch.full((count,), start, dtype=torch.int32, device=DEV)
    else:
        start = k = torch.from_numpy(np.ascontiguousarray(k_host[first:first + count])).to(DEV)
    want_all, _ = reader.expected(full, batch.offsets, batch.traj_len, k, horizon, dof, first, count, lo4, hi4, mask=15)
    got = {}
    for arrays in masks:
        mask = _mask_of(arrays)
        planes = selected(mask)
        need = count * len(planes) * dof
        assert reader.count(ltp, count, mask) == need
        buf = torch.full((need + 32,), GUARD, dtype=torch.int32, device=DEV)
        fold_buf = torch.full((count + 32,), GUARD, dtype=torch.int32, device=DEV)
        table, folded = reader.read(ltp, batch, first, count, start, horizon, arrays=arrays, lo=_sides(mask, lo4), hi=_sides(mask, hi4),
                                    fold=fold_buf[16:16 + count], out=buf[16:16 + need])
        torch.cuda.synchronize()
        assert bool((buf[:16] == GUARD).all().item()) and bool((buf[16 + need:] == GUARD).all().item()), f"{what} {arrays}: ints beside the call's were written"
        assert bool((fold_buf[:16] == GUARD).all().item()) and bool((fold_buf[16 + count:] == GUARD).all().item()), \
            f"{what} {arrays}: {reader.fold_name} beside the call's"
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
        assert torch.equal(folded, reader.fold(want).int()), f"{what} {arrays}: {reader.fold_name} differs"
        got[arrays] = (table, folded)
    return got


# ---- the tests that are the same body with another reader. `boxes(full, batch, dof, mn, mx)` gives the test's families of boxes, a
# ---- list of (lo, hi) [n, 4, dof], from the batch's full rows and their ranges

def short_runs(reader, oracle_mod, name, boxes):
    """The run-census batches: a uniform k swept over 0 .. 4 and per-plan starts, short horizons and the whole plan."""
    R = _rows(oracle_mod, name)
    ltp, batch, n, cen, dof = R["ltp"], R["batch"], R["n"], R["cen"], R["dof"]
    lens = R["rec"]["traj_len"]
    mn, mx = bx.row_ranges(R["full"], batch.offsets, batch.traj_len, dof, 0, n)
    rng = np.random.default_rng(17)
    describe = lambda plans: rc.describe(cen, plans)
    for lo, hi in boxes(R["full"], batch, dof, mn, mx):
        for horizon in (1, 3, 1 << 30):
            for k in list(range(5)) + [_starts(rng, lens)]:
                assert_reads(reader, ltp, batch, R["full"], k, horizon, 0, n, lo, hi, f"{name} k {'per plan' if not isinstance(k, int) else k}",
                             masks=("qvaj",), describe=describe)


def jerk_dominated_runs(reader, oracle_mod, boxes):
    """The jerk-dominated soft set of tests/branch_census.py: the first 200 plans of the dense batch, from k = 0 and per-plan starts."""
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
    mn, mx = bx.row_ranges(full, batch.offsets, batch.traj_len, dof, 0, n)
    rng = np.random.default_rng(5)
    for lo, hi in boxes(full, batch, dof, mn, mx):
        for horizon in (64, 1 << 30):
            for k in (0, _starts(rng, lens)):
                assert_reads(reader, ltp, batch, full, k, horizon, 0, n, lo, hi, f"soft dense H {horizon}", masks=("qvaj", "q"))
    torch.cuda.synchronize()


def other_batch_kinds(reader, kind, boxes, moved):
    """A retimed batch, a batch with three bound limit sets, MATLAB semantics (full rows from the walk sampler) and a stop batch: each
    against the exhaustive scan of its own rows, whole and a sub-range. Under limit sets the default boxes equal explicit per-plan
    boxes built from each plan's own set, bit for bit in the ints; moved(table): the entries that show a v or a lane left its box."""
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
    mn, mx = bx.row_ranges(full, batch.offsets, batch.traj_len, dof, 0, n)
    rng = np.random.default_rng(21)
    first, count = H.odd_range(n, dof)
    for lo, hi in boxes(full, batch, dof, mn, mx):
        for horizon in (64, 1 << 30):
            k = _starts(rng, lens)
            assert_reads(reader, ltp, batch, full, k, horizon, 0, n, lo, hi, f"{kind} H {horizon}", masks=("qvaj",))
            assert_reads(reader, ltp, batch, full, k, horizon, first, count, lo[first:first + count], hi[first:first + count],
                         f"{kind} H {horizon} sub-range", masks=("qvaj", "va"))
    if kind == "limit_sets":
        _, lim = limit_set("panda")
        sets = {key: np.array([[f * x if key in ("v_max", "a_max", "j_max") else x for x in lim[key]] for f in (1.0, 0.5, 0.25)]) for key in lim}
        d_lo, d_hi = bx.default_boxes(n, sets, DEV, set_index=batch.limit_set)
        assert float((d_hi[0, 1] / d_hi[1, 1]).min()) == 2.0     # plan 0 reads set 0, plan 1 set 1
        for horizon in (240, 1 << 30):
            default = reader.read(ltp, batch, 0, n, 0, horizon, arrays="qvaj")
            explicit = assert_reads(reader, ltp, batch, full, 0, horizon, 0, n, d_lo, d_hi, "limit sets, explicit per-plan boxes", masks=("qvaj",))["qvaj"][0]
            torch.cuda.synchronize()
            assert torch.equal(default, explicit), "the default boxes are not the plan's own set"
            assert int(moved(default[:, 1:3]).sum().item()) > 0


def refusals_and_bounds(reader, more_host_refusals=lambda n, dof, host_box: ()):
    """Each refusal of the device entry is LTP_ERR_INVALID_ARGUMENT, its text names the reason, and the guard-filled buffer and fold
    it was given keep their pattern; a geometry change after planning is refused in ltp_state_at_batch's words; a call whose buffer
    is exactly the elements function's count long writes nothing beside it. The wrappers refuse a bad mask, horizon or box
    (ValueError) and the host entry its own arguments (LtpError) before any launch. more_host_refusals(n, dof, host_box): further
    keyword sets the host wrapper must refuse with ValueError."""
    import torch
    from longtermplanner_amd import _abi
    from longtermplanner_amd._abi import LtpError
    n = 64
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    lib, O = ltp._lib, getattr(_abi, reader.opts)
    elements, plan_host = reader.elements, getattr(lib, reader.plan_host)
    P = C.c_void_p * 4
    need = n * 4 * dof
    assert reader.count(ltp, n, 15) == need and reader.count(ltp, n, 5) == need // 2
    assert reader.count(ltp, n, 0) == 0 and reader.count(ltp, n, 16) == 0 and reader.count(ltp, 0, 15) == 0
    buf = torch.full((need + 64,), GUARD, dtype=torch.int32, device=DEV)
    out = buf[32:32 + need]
    fold_buf = torch.full((n,), GUARD, dtype=torch.int32, device=DEV)
    box = torch.zeros((dof,), dtype=torch.float64, device=DEV) + 0.5
    call = H.reader_call(getattr(lib, reader.batch), ltp, batch, n, out, capacity=need)
    good = dict(size=C.sizeof(O), arrays=15, horizon=240, box_joint_stride=1)
    status = batch.status.clone()
    rc_, msg = call(O(**good))
    assert rc_ == 0, msg
    torch.cuda.synchronize()
    want = reader.read(ltp, batch, 0, n, 0, 240, arrays="qvaj")
    torch.cuda.synchronize()
    assert torch.equal(out, want.reshape(-1)), f"{reader.fold_name} = NULL changes the table"
    assert bool((buf[:32] == GUARD).all().item()) and bool((buf[32 + need:] == GUARD).all().item()), "ints beside the call's elements were written"
    assert torch.equal(batch.status, status)
    buf.fill_(GUARD)
    good = dict(good, **{reader.fold_name: fold_buf.data_ptr()})
    refusals = [(dict(q=False), {}, "null"), (dict(r=False), {}, "null"), (dict(out_ptr=0), {}, "null"), (dict(capacity=need - 1), {}, elements),
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
    assert rc_ == INVALID and elements in msg
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
            reader.read(ltp, batch, 0, n, 0, args.pop("horizon"), out=view, fold=fold_buf, **args)
    host_box = np.full(dof, 0.5)
    for kw in (dict(arrays="x"), dict(horizon=0), dict(arrays="q", hi={"j": host_box}), dict(lo={"q": host_box[:3]}),
               *more_host_refusals(n, dof, host_box)):
        args = dict(dict(horizon=240, arrays="qvaj"), **kw)
        with pytest.raises(ValueError):
            reader.read_host(ltp, *qs, 0, args.pop("horizon"), **args)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    host_out = np.full(need, GUARD, dtype=np.int32)
    boxes = (dp * 4)(None, host_box.ctypes.data_as(dp), None, None)
    for arrays, horizon, per_plan, his, text in ((0, 240, 0, None, "arrays"), (16, 240, 0, None, "arrays"), (15, 0, 0, None, "horizon"),
                                                 (15, (1 << 30) + 1, 0, None, "horizon"), (15, 240, 2, None, "box_per_plan"), (1, 240, 0, boxes, "not selected")):
        rc_ = plan_host(ltp._h, n, *[x.ctypes.data_as(dp) for x in qs], None, 0, horizon, arrays, None, his, per_plan, None, host_out.ctypes.data_as(ip), None)
        assert rc_ == INVALID and text in (lib.ltp_last_error(ltp._h) or b"").decode(), (arrays, horizon, per_plan)
    assert (host_out == GUARD).all()
    with pytest.raises(LtpError):
        ltp._check(plan_host(ltp._h, n, *[x.ctypes.data_as(dp) for x in qs], None, 0, 240, 15, None, None, 0, None, None, None))
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all().item()), "a refused call wrote to the buffer"
    assert bool((fold_buf == GUARD).all().item()), f"a refused call wrote to {reader.fold_name}"
    assert call(O(**good))[0] == 0
    torch.cuda.synchronize()
    assert torch.equal(fold_buf, reader.fold(out.view(n, 4, dof)).int())


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
  std::vector<int> table, folded;
  BatchTrajectory b;
  const double* los[4] = {nullptr, nullptr, a_lo.data(), nullptr};
  const double* his[4] = {nullptr, v_hi.data(), nullptr, nullptr};
  const long long ok = ltp.PLAN_BATCH(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, 500,
                                      LTP_ENV_Q | LTP_ENV_V | LTP_ENV_A, los, his, true, table, &folded, &b);
  int refused = 0;
  for (int arrays : {0, 16}) {
    try {
      std::vector<int> e2;
      ltp.PLAN_BATCH(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, 500, arrays, nullptr, nullptr, false, e2);
    } catch (const std::exception&) { ++refused; }
  }
  for (int horizon : {0, -1}) {
    try {
      std::vector<int> e2;
      ltp.PLAN_BATCH(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, horizon, LTP_ENV_Q, nullptr, nullptr, false, e2);
    } catch (const std::exception&) { ++refused; }
  }
  try {
    std::vector<int> e2;
    ltp.PLAN_BATCH(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, 500, LTP_ENV_Q, nullptr, his, true, e2);
  } catch (const std::exception&) { ++refused; }
  if (refused != 5) return 3;
  FILE* o = std::fopen(argv[2], "wb");
  std::fwrite(table.data(), sizeof(int), table.size(), o);
  std::fwrite(folded.data(), sizeof(int), folded.size(), o);
  std::fwrite(b.status.data(), sizeof(int), b.status.size(), o);
  std::fclose(o);
  std::printf("%lld ok, %zu ints\n", ok, table.size());
  return 0;
}
'''


def host_and_dropin_paths(reader, tmp_path, both_answers):
    """The host wrapper equals the device call int for int (boxes [dof] and [n, dof], with and without the fold) and its status
    carries END_LIMIT like planBatchHost(sample=False); a small C++ program gives the same bytes through the drop-in class's
    method (dropin_call). both_answers(table, k, lens): the device table holds lanes that leave their box and lanes that do not."""
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
    dev, dev_fold = reader.read(ltp, batch, 0, n, torch.from_numpy(k).to(DEV), 500, arrays="qva", lo={"a": torch.from_numpy(a_lo).to(DEV)},
                                hi={"v": torch.from_numpy(v_hi).to(DEV)}, fold=True)
    dev, dev_fold = dev.cpu().numpy(), dev_fold.cpu().numpy()
    assert both_answers(dev, k, lens)
    assert not (batch.status.cpu().numpy()[3] & 8), "the device call forms no end-limit verdict"
    rec, table, folded = reader.read_host(ltp, *qs, k, 500, arrays=7, lo={"a": a_lo}, hi={"v": v_hi}, fold=True)
    assert table.shape == (n, 3, dof) and table.dtype == np.int32
    assert np.array_equal(table, dev) and np.array_equal(folded, dev_fold)
    plain = ltp.planBatchHost(*qs, sample=False)
    assert np.array_equal(rec["status"], plain["status"]) and (rec["status"][3] & 8) and np.array_equal(rec["traj_len"], lens)
    # a uniform k, one box per joint, no fold
    one = 0.5 * np.asarray(lim["v_max"])
    _, table_u = reader.read_host(ltp, *qs, 5, 1 << 30, arrays="v", lo={"v": -one}, hi={"v": one})
    dev_u = reader.read(ltp, batch, 0, n, 5, 1 << 30, arrays="v", lo={"v": torch.from_numpy(-one).to(DEV)}, hi={"v": torch.from_numpy(one).to(DEV)})
    assert table_u.shape == (n, 1, dof) and np.array_equal(table_u, dev_u.cpu().numpy())

    raw = H.run_dropin(tmp_path, reader.call, DROPIN.replace("PLAN_BATCH", reader.dropin_call),
                       np.concatenate([x.reshape(-1) for x in qs]).astype(np.float64).tobytes() + k.astype(np.int32).tobytes() + v_hi.tobytes() + a_lo.tobytes())
    assert raw == table.tobytes() + folded.tobytes() + rec["status"].astype(np.int32).tobytes()


def graph_capture_and_replay(reader, with_fold, boxes):
    """The call allocates nothing: captured on one stream (one kernel node, and one fill-kernel node before it with the fold) and
    replayed after first_sample AND the box arrays were rewritten in place, it gives what a direct call gives for the new starts
    and boxes, and what the exhaustive scan gives — twice. boxes(..): three families, the captured one and the two replayed."""
    import torch
    n = 1000
    ltp, dof, lim, qs, batch, full, lens, mn, mx = _batch("panda", n)
    rng = np.random.default_rng(77)
    ka, kb, kc = (_starts(rng, lens) for _ in range(3))
    assert np.count_nonzero(ka != kb) > 0.5 * n
    boxes = boxes(full, batch, dof, mn, mx)
    k = torch.from_numpy(ka).to(DEV)
    lo, hi = boxes[0][0].clone(), boxes[0][1].clone()
    mask = 15
    lo_by = {a: lo[:, x].contiguous() for x, a in enumerate(LETTERS)}
    hi_by = {a: hi[:, x].contiguous() for x, a in enumerate(LETTERS)}
    out = torch.zeros((n, 4, dof), dtype=torch.int32, device=DEV)
    folded = torch.zeros((n,), dtype=torch.int32, device=DEV)
    graph = H.capture(lambda: reader.read(ltp, batch, 0, n, k, 240, arrays=mask, lo=lo_by, hi=hi_by, fold=folded if with_fold else False, out=out))
    for k_new, (lo_new, hi_new) in ((kb, boxes[1]), (kc, boxes[2])):
        k.copy_(torch.from_numpy(k_new))
        for x, a in enumerate(LETTERS):
            lo_by[a].copy_(lo_new[:, x])
            hi_by[a].copy_(hi_new[:, x])
        out.zero_()
        folded.fill_(12345)
        graph.replay()
        torch.cuda.synchronize()
        direct = reader.read(ltp, batch, 0, n, k, 240, arrays=mask, lo=lo_by, hi=hi_by, fold=with_fold)
        torch.cuda.synchronize()
        want, want_fold = reader.expected(full, batch.offsets, batch.traj_len, k, 240, dof, 0, n, lo_new, hi_new)
        assert torch.equal(out, want)
        if with_fold:
            assert torch.equal(direct[0], out) and torch.equal(direct[1], folded) and torch.equal(folded, want_fold)
        else:
            assert torch.equal(direct, out) and bool((folded == 12345).all().item())
