"""Horizon envelopes of q, v, a and j (ltp_envelope_knots_arrays_batch, include/ltp_hip.h) on the GPU: per plan, selected array and
joint {min, max} over the trajectory samples between the edges k + g[w] and k + g[w + 1] of a knot grid. Compared with the reduced
rows of the full-row sampler for the same batch (tests/envelope_arrays_checker.py, itself pinned to a plain loop by
tests/test_envelope_arrays_cpu.py): q and v under the project's acceptance rule for an analytic envelope form, a and j for equality;
with the q-only call and among the masks bit for bit; with the knots call; at the end of a plan; on the run-census batches, on
other batch kinds, through the host and drop-in paths and under graph capture. The batches and planner helpers are
tests/horizon_helpers.py's and tests/gpu_helpers.py's.

Contract-breaking device grids are pinned on the host only (tests/cpp/envelope_knots_ranges_test.cc): no test here feeds one."""
import ctypes as C

import numpy as np
import pytest

import envelope_arrays_checker as ac
import horizon_helpers as H
import knots_checker as kc
import run_census as rc
from gpu_helpers import _rows
from horizon_helpers import DEV, INVALID
from horizon_helpers import grid_tensor as _grid

pytestmark = pytest.mark.gpu

REJECTED = 11                 # the plan every batch of _batch() has rejected: NaN envelopes among planned neighbours
MASKS = (15, 2, 12, 1)


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


def _assert_arrays(ltp, batch, full, k_host, g, closed, first, count, what, masks=MASKS, describe=None):
    """One call per mask over plans [first, first + count) with starts k_host[first:first + count] (an int: uniform), each plane
    compared with the reduced rows by its rule (envelope_arrays_checker.compare); `valid` against its formula; a buffer with guard
    words behind the call's elements keeps them. Returns ({mask: env}, {array: (worst |d|, bit-identical share)} over the masks)."""
    import torch
    M, dof = len(g) - 1, batch.dof
    if isinstance(k_host, (int, np.integer)):
        start = int(k_host)
        k = torch.full((count,), start, dtype=torch.int32, device=DEV)
    else:
        start = k = torch.from_numpy(np.ascontiguousarray(k_host[first:first + count])).to(DEV)
    red, exp_valid, planned = ac.expected(full, batch.offsets, batch.traj_len, k, g, closed, dof, first, count, mask=15)
    envs, figures = {}, {}
    grid = _grid(g)
    for mask in masks:
        planes = ac.selected(mask)
        need = count * len(planes) * dof * M * 2
        assert ltp._lib.ltp_envelope_knots_arrays_elements(ltp._h, count, M, mask) == need
        buf = torch.full((need + 16,), H.PATTERN, dtype=torch.float64, device=DEV)
        _, valid = ltp.envelopeKnotsArrays(batch, first, count, start, grid, arrays=mask, closed=closed, out=buf[:need])
        torch.cuda.synchronize()
        assert bool((buf[need:] == H.PATTERN).all().item()), f"{what} mask {mask}: elements behind the call's were written"
        env = buf[:need].view(count, len(planes), dof, M, 2)
        bad, fig = ac.compare(env, red[:, planes].contiguous(), planned, mask)
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
        envs[mask] = env
    return envs, figures


@pytest.mark.parametrize("name,n,pow_rule", [("panda", 1500, "libm"), ("panda", 1500, "exact"), ("ref", 1000, "libm"), ("ref30", 200, "libm")])
def test_envelopes_against_reduced_rows(name, n, pow_rule):
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
    for gname in ("mpc", "duplicates", "n65", "max"):
        g = ac.GRIDS[gname]
        assert gname != "max" or len(g) - 1 == ac.MAX_INTERVALS == 511
        for closed in (0, 1):
            k = _starts(rng, lens)
            kk = np.maximum(k.astype(np.int64), 0)
            ends, starts = float(np.mean((L > 0) & (kk + int(g[-1]) >= L))), float(np.mean((L > 0) & (kk + int(g[0]) >= L)))
            what = f"{name} {pow_rule} grid {gname} closed {closed}"
            envs, fig = _assert_arrays(ltp, batch, full, k, g, closed, 0, n, f"{what} whole batch")
            _, fig2 = _assert_arrays(ltp, batch, full, k, g, closed, first, count, f"{what} plans [{first}, {first + count})")
            q_share, v_share = min(fig["q"][1], fig2["q"][1]), min(fig["v"][1], fig2["v"][1])
            print(f"{what}: horizon ends past traj_len {ends:.3f}, starts there {starts:.3f}; q worst |d| {max(fig['q'][0], fig2['q'][0]):.3e}, "
                  f"bit-identical {q_share:.6f}; v worst |d| {max(fig['v'][0], fig2['v'][0]):.3e}, bit-identical {v_share:.6f}")
            assert ends > 0.0 and q_share >= 0.999, (what, ends, q_share)
            for mask, env in envs.items():
                assert bool(np.isnan(env[REJECTED].cpu().numpy()).all()), (what, mask)


@pytest.mark.parametrize("name", rc.BATCHES)
def test_the_smallest_shapes(oracle_mod, name):
    """The run-census batches (rows of 1-153 samples, one-sample runs, collided switch indices, switching times on exact multiples
    of the sample time): unit, two-sample and duplicate-holding grids, both modes, a uniform k swept over 0 .. 8 and per-plan
    starts, all four arrays in one call."""
    R = _rows(oracle_mod, name)
    ltp, batch, n, cen = R["ltp"], R["batch"], R["n"], R["cen"]
    lens = R["rec"]["traj_len"]
    rng = np.random.default_rng(17)
    grids = kc.SMALL_GRIDS
    assert list(grids) == ["unit", "two", "duplicates"]
    describe = lambda mask: rc.describe(cen, mask)
    worst = {"q": 0.0, "v": 0.0}
    least = {"q": 1.0, "v": 1.0}
    for gname, g in grids.items():
        for closed in (0, 1):
            for k in list(range(9)) + [_starts(rng, lens)]:
                what = f"{name} grid {gname} closed {closed} k {'per plan' if not isinstance(k, int) else k}"
                _, fig = _assert_arrays(ltp, batch, R["full"], k, g.astype(np.int32), closed, 0, n, what, masks=(15,), describe=describe)
                for x in "qv":
                    worst[x], least[x] = max(worst[x], fig[x][0]), min(least[x], fig[x][1])
    print(f"{name}: q worst |d| {worst['q']:.3e}, least bit-identical share {least['q']:.6f}; v worst |d| {worst['v']:.3e}, share {least['v']:.6f}")
    assert least["q"] >= 0.999, (name, least)


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
    import torch
    n = 1500
    ltp, dof, lim, qs, batch, full, lens = _batch("panda", n)
    g = ac.GRIDS[gname]
    M = len(g) - 1
    k = torch.from_numpy(_starts(np.random.default_rng(8), lens)).to(DEV)
    rows, kv = ltp.sampleKnots(batch, 0, n, k, _grid(g))
    planned = batch.traj_len > 0
    x = rows[..., :M + 1][planned]                               # [plans, 4, dof, M + 1]
    dup = torch.from_numpy(np.diff(g) == 0).to(DEV)
    for closed in (0, 1):
        env, valid = ltp.envelopeKnotsArrays(batch, 0, n, k, _grid(g), closed=closed)
        torch.cuda.synchronize()
        e = env[planned]
        assert bool(((e[..., 0] <= x[..., :M]) & (x[..., :M] <= e[..., 1])).all().item()), (gname, closed)
        if closed:
            assert bool(((e[..., 0] <= x[..., 1:]) & (x[..., 1:] <= e[..., 1])).all().item()), (gname, closed)
        if bool(dup.any().item()):
            twice = torch.stack([x[..., :M], x[..., :M]], dim=4)[:, :, :, dup]
            assert bool((e[:, :, :, dup] == twice).all().item()), (gname, closed)
            assert torch.equal(ac.int_view(e[:, 0][:, :, dup].contiguous()), ac.int_view(twice[:, 0].contiguous())), (gname, closed)
        last_real = ((k.long().clamp(min=0) + int(g[-1])) < batch.traj_len.long()).int()
        assert torch.equal(valid, kv - torch.where(planned, last_real, torch.zeros_like(last_real)))
    assert gname != "duplicates" or int(dup.sum().item()) >= 5


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
    g = ac.GRIDS["mpc"]
    for closed in (0, 1):
        k = _starts(rng, lens)
        _, fig = _assert_arrays(ltp, batch, full, k, g, closed, 0, n, f"{kind} closed {closed}", masks=(15,))
        _, fig2 = _assert_arrays(ltp, batch, full, k, g, closed, first, count, f"{kind} closed {closed} sub-range", masks=(15, 6))
        print(f"{kind} closed {closed}: {fig} {fig2}")
        assert min(fig["q"][1], fig2["q"][1]) >= 0.999


def test_refusals_and_bounds():
    """Each refusal of the device entry is LTP_ERR_INVALID_ARGUMENT, its text names the reason, and the buffer it was given keeps
    its pattern; a geometry change after planning is refused in ltp_state_at_batch's words; guard words behind the call's elements
    stay intact; valid = NULL is accepted. Host edge lists outside the contract and a bad `arrays` are refused by
    ltp_plan_envelope_knots_arrays_host (LtpError) and by the wrappers (ValueError) before any launch."""
    import torch
    from longtermplanner_amd import _abi
    n = 64
    g = ac.GRIDS["mpc"]
    M = len(g) - 1
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    lib, O = ltp._lib, _abi.EnvelopeArraysOpts
    need = n * 4 * dof * M * 2
    assert lib.ltp_envelope_knots_arrays_elements(ltp._h, n, M, 15) == need
    assert lib.ltp_envelope_knots_arrays_elements(ltp._h, n, M, 5) == need // 2 and lib.ltp_envelope_knots_arrays_elements(ltp._h, n, M, 8) == need // 4
    assert lib.ltp_envelope_knots_arrays_elements(ltp._h, n, M, 0) == 0 and lib.ltp_envelope_knots_arrays_elements(ltp._h, n, M, 16) == 0
    guard = 64
    out = torch.full((need + guard,), H.PATTERN, dtype=torch.float64, device=DEV)
    big = torch.full((n * 4 * dof * (ac.MAX_INTERVALS + 1) * 2,), H.PATTERN, dtype=torch.float64, device=DEV)
    grid = _grid(np.concatenate([g, np.zeros(ac.MAX_INTERVALS + 2 - len(g), dtype=np.int32) + int(g[-1])]))     # long enough for every M tried
    call = H.reader_call(lib.ltp_envelope_knots_arrays_batch, ltp, batch, n, out, capacity=need)
    good = dict(size=C.sizeof(O), n_intervals=M, closed=1, arrays=15, reserved=0, edge_offsets=grid.data_ptr())          # valid = NULL
    status = batch.status.clone()
    rc_, msg = call(O(**good))
    assert rc_ == 0, msg
    torch.cuda.synchronize()
    want, _ = ltp.envelopeKnotsArrays(batch, 0, n, 0, _grid(g), closed=True)
    torch.cuda.synchronize()
    assert torch.equal(ac.int_view(out[:need]), ac.int_view(want.reshape(-1))), "valid = NULL changes the envelopes"
    assert bool((out[need:] == H.PATTERN).all().item()), "the guard words behind the call's elements were written"
    assert torch.equal(batch.status, status)
    H.common_refusals(ltp, batch, n, dof, call, O, good, out, need - 1, "ltp_envelope_knots_arrays_elements")
    for bad, text in ((dict(edge_offsets=None), "edge_offsets is NULL"), (dict(n_intervals=0), "n_intervals"), (dict(n_intervals=-1), "n_intervals"),
                      (dict(n_intervals=ac.MAX_INTERVALS + 1), "LTP_MAX_KNOTS - 1"), (dict(closed=2), "closed"), (dict(closed=-1), "closed"),
                      (dict(arrays=0), "arrays"), (dict(arrays=16), "arrays"), (dict(arrays=-1), "arrays"), (dict(reserved=1), "reserved"),
                      (dict(reserved=-1), "reserved")):
        rc_, msg = call(O(**dict(good, **bad)), buf=big, capacity=big.numel())
        assert rc_ == INVALID and text in msg, (bad, rc_, msg)
    # the capacity is held against the mask's own element count
    rc_, msg = call(O(**dict(good, arrays=3)), capacity=need // 2 - 1)
    assert rc_ == INVALID and "ltp_envelope_knots_arrays_elements" in msg
    torch.cuda.synchronize()
    assert bool((out == H.PATTERN).all().item()) and bool((big == H.PATTERN).all().item()), "a refused call wrote to the buffer"
    rc_, msg = call(O(**dict(good, arrays=3)), capacity=need // 2)
    assert rc_ == 0, msg
    torch.cuda.synchronize()
    assert bool((out[need // 2:] == H.PATTERN).all().item()), "a two-array call wrote beyond its elements"
    out.fill_(H.PATTERN)
    # the largest admitted grid is a call like any other
    rc_, msg = call(O(**dict(good, n_intervals=ac.MAX_INTERVALS)), buf=big, capacity=big.numel())
    assert rc_ == 0, msg
    torch.cuda.synchronize()
    assert bool((big[n * 4 * dof * ac.MAX_INTERVALS * 2:] == H.PATTERN).all().item())
    # host edge lists and `arrays` are looked at: the library's host entry and the wrappers refuse, before any launch
    from longtermplanner_amd._abi import LtpError
    env_out = out[:need].view(n, 4, dof, M, 2)
    for bad, text in (([0, 5, 4, 9], "decreases"), ([-1, 0, 3], "negative"), ([0, (1 << 30) + 1], "beyond 2^30"), ([], "n_intervals"),
                      ([11], "n_intervals"), (list(range(ac.MAX_INTERVALS + 2)), "LTP_MAX_KNOTS")):
        with pytest.raises(LtpError) as e:
            ltp.planEnvelopeKnotsArraysHost(*qs, 0, bad)
        assert e.value.code == INVALID and text in str(e.value), (bad, str(e.value))
        with pytest.raises(ValueError):
            ltp.envelopeKnotsArrays(batch, 0, n, 0, bad, out=env_out)
    g3 = (C.c_int * 3)(0, 4, 9)
    for arrays in (0, 16, -3):
        rc_ = lib.ltp_plan_envelope_knots_arrays_host(ltp._h, n, *[x.ctypes.data_as(C.POINTER(C.c_double)) for x in qs], None, 0, 2, g3, 0, arrays, None,
                                                      np.zeros(8).ctypes.data_as(C.POINTER(C.c_double)), None)
        assert rc_ == INVALID and "arrays" in (lib.ltp_last_error(ltp._h) or b"").decode()
        with pytest.raises(ValueError):
            ltp.envelopeKnotsArrays(batch, 0, n, 0, [0, 4, 9], arrays=arrays, out=env_out)
    with pytest.raises(ValueError):
        ltp.planEnvelopeKnotsArraysHost(*qs, 0, [0.5, 1.5])
    torch.cuda.synchronize()
    assert bool((out == H.PATTERN).all().item()), "envelopeKnotsArrays wrote to the buffer although it refused its arguments"
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
  const long long ok = ltp.planEnvelopeKnotsArraysBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, edges,
                                                        true, LTP_ENV_Q | LTP_ENV_V | LTP_ENV_J, env, &valid, &b);
  int refused = 0;
  for (int arrays : {0, 16}) {
    try {
      std::vector<double> e2;
      ltp.planEnvelopeKnotsArraysBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, edges, false, arrays, e2);
    } catch (const std::exception&) { ++refused; }
  }
  for (const std::vector<int>& bad : {std::vector<int>{4, 3}, std::vector<int>{7}, std::vector<int>{}}) {
    try {
      std::vector<double> e2;
      ltp.planEnvelopeKnotsArraysBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, bad, false, LTP_ENV_V, e2);
    } catch (const std::exception&) { ++refused; }
  }
  if (refused != 5) return 3;
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
    """planEnvelopeKnotsArraysHost equals the device path bitwise and its status carries END_LIMIT like planBatchHost(sample=False);
    a small C++ program gives the same bytes through LongTermPlanner::planEnvelopeKnotsArraysBatch."""
    import torch
    n = 40
    g = ac.GRIDS["mpc"]
    M = len(g) - 1
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    qs[0][3, 1] = 2.5                               # a goal beyond joint 1's range: planned, then END_LIMIT
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    lens = batch.traj_len.cpu().numpy()
    k = _starts(np.random.default_rng(1), lens)
    dev_env, dev_valid = ltp.envelopeKnotsArrays(batch, 0, n, torch.from_numpy(k).to(DEV), _grid(g), arrays="qvj", closed=True)
    dev_env, dev_valid = dev_env.cpu().numpy(), dev_valid.cpu().numpy()
    assert 0 < int((dev_valid > 0).sum()) and int((dev_valid < M).sum()) > 0
    assert not (batch.status.cpu().numpy()[3] & 8), "the device call forms no end-limit verdict"
    rec, env, valid = ltp.planEnvelopeKnotsArraysHost(*qs, k, g, arrays=11, closed=True)
    assert env.shape == (n, 3, dof, M, 2)
    assert np.array_equal(env.view(np.uint8), dev_env.view(np.uint8)) and np.array_equal(valid, dev_valid)
    plain = ltp.planBatchHost(*qs, sample=False)
    assert np.array_equal(rec["status"], plain["status"]) and (rec["status"][3] & 8) and np.array_equal(rec["traj_len"], lens)
    _, env_u, valid_u = ltp.planEnvelopeKnotsArraysHost(*qs, 5, [int(x) for x in g])
    du, dv = ltp.envelopeKnotsArrays(batch, 0, n, 5, g)                                   # a host grid: uploaded by the wrapper
    assert env_u.shape == (n, 4, dof, M, 2)
    assert np.array_equal(env_u.view(np.uint8), du.cpu().numpy().view(np.uint8)) and np.array_equal(valid_u, dv.cpu().numpy())

    raw = H.run_dropin(tmp_path, "envelope_arrays", DROPIN, np.concatenate([x.reshape(-1) for x in qs]).astype(np.float64).tobytes()
                       + k.astype(np.int32).tobytes() + g.astype(np.int32).tobytes())
    H.assert_dropin_bytes(raw, env, valid, rec["status"])


def test_graph_capture_and_replay_with_new_starts_and_a_new_grid():
    """The call allocates nothing: captured on one stream (one kernel node) and replayed after first_sample AND the content of
    edge_offsets were rewritten in place, it gives what a direct call gives for the new starts and the new grid — twice."""
    import torch
    n = 1000
    ltp, dof, lim, qs, batch, full, lens = _batch("panda", n)
    rng = np.random.default_rng(77)
    ga = ac.GRIDS["mpc"]
    E = len(ga)
    gb = (np.arange(E) ** 2 // 2 + 3).astype(np.int32)             # another 40 edges: further out, g[0] = 3
    gc = np.sort(rng.integers(0, 2000, E)).astype(np.int32)
    ka, kb, kcs = (_starts(rng, lens) for _ in range(3))
    assert np.count_nonzero(ka != kb) > 0.5 * n
    k, grid = torch.from_numpy(ka).to(DEV), _grid(ga)
    out = torch.zeros((n, 4, dof, E - 1, 2), dtype=torch.float64, device=DEV)
    valid = torch.zeros((n,), dtype=torch.int32, device=DEV)
    graph = H.capture(lambda: ltp.envelopeKnotsArrays(batch, 0, n, k, grid, closed=True, out=out, valid=valid))
    for k_new, g_new in ((kb, gb), (kcs, gc)):
        H.replay(graph, [(k, k_new), (grid, g_new)], out, valid)
        direct, direct_valid = ltp.envelopeKnotsArrays(batch, 0, n, k, grid, closed=True)
        torch.cuda.synchronize()
        assert torch.equal(ac.int_view(direct), ac.int_view(out)) and torch.equal(direct_valid, valid)
        red, exp_valid, planned = ac.expected(full, batch.offsets, batch.traj_len, k, g_new, 1, dof, 0, n)
        bad, fig = ac.compare(out, red, planned)
        assert not bool(bad.any().item()) and torch.equal(valid, exp_valid), fig
