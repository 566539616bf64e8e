"""Every planner branch on the GPU. The named limit sets (panda, ref, ref30) are acceleration-limited: under them timeScaling ends in
c1 / c2 almost always, c7 / c8 never, optSwitchTimes never fails and the fallback of cc:50-55 is taken by 0.2 % of the lanes of
random queries (tests/test_branch_census_cpu.py; with joints that rest it is a bulk path under those sets too: tests/test_gpu_structure.py). Here every batch is the jerk-dominated soft set of tests/branch_census.py with the project's own
query generator: every case 0-8 and every optSwitchTimes site in bulk, a fifth of the lanes on the fallback, two thirds of the scaled
lanes in queue B, some plans failing stage 1. Records, ragged sizes, dense rows, every sampler, the readers of records (the knot grids and
the horizon envelopes included), retime, limit
sets, MATLAB semantics and the single-call kernel are compared with the CPU oracle (or with each other where the suite claims bits),
class by class: a mismatch names the timeScaling case and the site bits of the lanes concerned.

Tolerances are the suite's own: bit identity under pow_rule "exact" against the oracle's exact-pow twin and under "libm" behind the
restated_host_libm fixture, 1e-9 otherwise."""
import numpy as np
import pytest

import branch_census as bc
import envelope_helpers as E
import horizon_checker as hc
import horizon_helpers as H
import knots_checker as kc
import retime_checker as rc
from gpu_helpers import DEV, REC_KEYS, TOL, _agree, _bits_equal, _host, _plan_rows, _planner, _tensors, _window_expected

pytestmark = pytest.mark.gpu

LANE_KEYS = ("t_opt", "t_scaled", "dir", "mod", "v_drive")
QUERY_KEYS = ("t_required", "slowest", "traj_len")
ROWS_N = 600                      # plans of the dense batch (Ts 0.01) whose rows the sampler / reader tests take: 137 MB of float64 rows


def _disagreements(dev, ref, exact, mask):
    """{key: lane mask [n][dof]} of the record fields in which the queries of `mask` [n] disagree (query fields spread over the joints)."""
    D = dev["dir"].shape[1]
    out = {}
    for k in LANE_KEYS + QUERY_KEYS:
        bad = ~_agree(dev[k], ref[k], exact)
        bad = bad.reshape(bad.shape[0], D, -1).any(axis=2) if k in LANE_KEYS else np.repeat(bad[:, None], D, axis=1)
        bad &= mask[:, None]
        if bad.any():
            out[k] = bad
    return out


def _assert_classes(dev, ref, cen, exact, mask, what, empty_ok=()):
    """dev == ref over the queries of `mask`, census class by census class: each class is non-empty and compared as its own group."""
    bad = _disagreements(dev, ref, exact, mask)
    for name, lanes in bc.classes(cen):
        lanes = lanes & mask[:, None]
        if name in empty_ok:
            continue
        assert lanes.any(), f"{what}: no lane of class {name} in this batch: the comparison would prove nothing about it"
        for k, b in bad.items():
            hit = b & lanes
            assert not hit.any(), f"{what}: class {name}: {k} differs from the oracle ({'bits' if exact else '1e-9'}): {bc.describe(cen, hit)}"
    assert not bad, f"{what}: {sorted(bad)} differ outside every census class: {bc.describe(cen, np.any(list(bad.values()), axis=0))}"


def _empty_ok(dof):
    # one joint: it keeps its optimum, nothing is scaled; joint 0 alone never takes site 8 (branch_census.assert_floors)
    return tuple(f"c{c}" for c in bc.CASES) + ("site8",) if dof == 1 else ()


def _records_case(oracle_mod, dof, layout, pow_rule, exact):
    from longtermplanner_amd import STATUS_END_LIMIT, STATUS_OPT_FAILED
    n = bc.RECORD_BATCHES[dof]
    orc, lim, qs, orec, cen = bc.soft_batch(oracle_mod, dof, n, exact_pow=(pow_rule == "exact"))
    bc.assert_floors(cen["totals"], dof)
    ltp = _planner(dof, lim, pow_rule=pow_rule)
    dev = _host(ltp.planSwitchTimesBatch(*_tensors(qs, layout), layout=layout, end_limit=True))
    what = f"soft dof {dof} n {n} {layout} {pow_rule}"
    planned = orec["status"] != 0
    dev_planned = (dev["status"] & ~STATUS_END_LIMIT) == 0
    assert np.array_equal(dev_planned, planned), f"{what}: planned verdicts differ: {bc.describe(cen, dev_planned != planned)}"
    end = (dev["status"] & STATUS_END_LIMIT) != 0
    assert np.array_equal(end, orec["status"] == 2), f"{what}: end-limit verdicts differ: {bc.describe(cen, end != (orec['status'] == 2))}"
    _assert_classes(dev, orec, cen, exact, planned, what, _empty_ok(dof))
    # stage 1 fails exactly where the oracle's does; such a plan has zero scaled records, no trajectory and no rows
    failed = ~cen["opt_ok"].all(axis=1)
    dev_failed = (dev["status"] & STATUS_OPT_FAILED) != 0
    assert np.array_equal(dev_failed, failed), f"{what}: LTP_STATUS_OPT_FAILED differs from the oracle's stage 1: {bc.describe(cen, dev_failed != failed)}"
    assert failed.sum() >= 10 and np.array_equal(failed, ~planned)
    assert not dev["t_scaled"][failed].any() and not dev["traj_len"][failed].any(), what
    assert not np.diff(dev["offsets"].astype(np.int64))[failed].any(), what
    # and its neighbours in the same 64-query block are what the oracle says
    near = np.zeros(n, dtype=bool)
    for q in np.nonzero(failed)[0]:
        near[q // 64 * 64: q // 64 * 64 + 64] = True
    near &= planned
    bad = _disagreements(dev, orec, exact, near)
    assert not bad, f"{what}: neighbours of a failed plan differ in {sorted(bad)}: {bc.describe(cen, np.any(list(bad.values()), axis=0))}"
    return dev


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
@pytest.mark.parametrize("layout", ["query_major", "joint_major"])
@pytest.mark.parametrize("dof", [7, 2, 30, 1])
def test_records_by_class(oracle_mod, dof, layout, pow_rule):
    """"exact": the bits of the exact-pow twin; "libm": within 1e-9 of the parity oracle on any host (bits: the next test)."""
    _records_case(oracle_mod, dof, layout, pow_rule, exact=(pow_rule == "exact"))


@pytest.mark.parametrize("layout", ["query_major", "joint_major"])
@pytest.mark.parametrize("dof", [7, 2, 30, 1])
def test_records_have_the_libm_oracles_bits_by_class(oracle_mod, dof, layout, restated_host_libm):
    _records_case(oracle_mod, dof, layout, "libm", exact=True)


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
@pytest.mark.parametrize("dof,start", [(7, 0), (7, 1000), (30, 300), (2, 64)])
def test_ragged_sizes_have_the_bits_of_the_whole_batch(oracle_mod, dof, start, pow_rule):
    """1, 63, 64, 65 and 130 queries cut from the batch: with most lanes in queue B the per-block reservation of scale_rounds step (3)
    and the 32-per-block dealing of k_scaling_slow (queues of at most 4096 items) see partial blocks."""
    n = bc.RECORD_BATCHES[dof]
    orc, lim, qs, orec, cen = bc.soft_batch(oracle_mod, dof, n, exact_pow=(pow_rule == "exact"))
    ltp = _planner(dof, lim, pow_rule=pow_rule)
    whole = _host(ltp.planSwitchTimesBatch(*_tensors(qs)))
    for m in (1, 63, 64, 65, 130):
        sl = slice(start, start + m)
        part = _host(ltp.planSwitchTimesBatch(*_tensors([x[sl] for x in qs])))
        sub = {k: v[sl] for k, v in cen.items() if k != "totals"}
        if m >= 63:
            assert ((sub["case"] >= 0) & (sub["case"] != 1) & (sub["case"] != 2)).sum() > (sub["case"] >= 0).sum() // 2, "most scaled lanes of the cut go through queue B"
        for k in REC_KEYS:
            bad = ~_agree(part[k], whole[k][sl], True).reshape(m, -1).all(axis=1)
            assert not bad.any(), f"soft dof {dof} {pow_rule}: {m} queries from {start}: {k} differs from the whole batch: {bc.describe(sub, bad)}"
        assert np.array_equal(np.diff(part["offsets"].astype(np.int64)), np.diff(whole["offsets"].astype(np.int64))[sl])


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
def test_dense_rows(oracle_mod, pow_rule, request):
    """Every q / v / a / j sample of the dense batch: the strict bar of test_dense_trajectories_parity_budget against the exact twin, and
    the bar of test_dense_trajectories_strict_under_the_libm_pow_rule against the parity oracle (where this host's libm is the restated
    one). End-limit verdicts are the oracle's status 2."""
    import torch
    import dense_compare as dc
    if pow_rule == "libm":
        request.getfixturevalue("restated_host_libm")
    dof, n, ts = bc.DENSE_BATCH
    exact = pow_rule == "exact"
    orc, lim, qs, orec, cen = bc.soft_batch(oracle_mod, dof, n, ts, exact_pow=exact)
    bc.assert_floors(cen["totals"], dof)
    L = orec["traj_len"].astype(np.int64)
    need = 4 * dof * int(((L + 31) // 32 * 32).sum())                     # 58 M values, 468 MB: one chunk of the soak, so one host buffer
    assert need * 8 <= dc.CHUNK_BYTES
    pinned = torch.empty(need + 1024, dtype=torch.float64, pin_memory=True)     # this test's alone, released when it returns
    s = dc.soak(f"soft{dof}", dof, lim, ts, n, bc.SEED, [pinned, pinned], quiet=True, exact=exact, pow_rule=pow_rule)
    del pinned
    where = np.zeros(n, dtype=bool)
    where[[o["query"] for o in s["outliers"]]] = True
    lanes = bc.describe(cen, where)
    print(f"dense soft rows {pow_rule}: {s['sampled']} plans, {s['values_compared']} values, max |d| {s['max_abs_d']}")
    assert s["verdict_mismatches"] == 0 and s["length_mismatches"] == 0 and s["end_limit_flag_mismatches"] == 0, (s, lanes)
    assert s["plans_beyond_tolerance"] == 0 and max(s["max_abs_d"].values()) <= TOL, (s["max_abs_d"], s["outliers"], lanes)
    assert s["plans_with_bit_identical_jerk_rows"] == s["sampled"], (s["sampled"] - s["plans_with_bit_identical_jerk_rows"], lanes)
    assert s["sampled"] == cen["totals"]["planned"] + cen["totals"]["end_limit"]
    assert s["end_limit_false"] == cen["totals"]["end_limit"] >= 5


_ROWS = {}


def _rows_batch(oracle_mod):
    """The first ROWS_N plans of the dense batch, planned on the device, with their full float64 rows from the fused sampler: the
    yardstick of the sampler and reader tests (itself compared with the oracle sample by sample in test_dense_rows)."""
    import torch
    if not _ROWS:
        dof, n, ts = bc.DENSE_BATCH
        orc, lim, qs, orec, cen = bc.soft_batch(oracle_mod, dof, n, ts)
        qs = [x[:ROWS_N] for x in qs]
        cen = {k: v[:ROWS_N] for k, v in cen.items() if k != "totals"}
        ltp = _planner(dof, lim, ts)
        batch = ltp.planSwitchTimesBatch(*_tensors(qs))
        rec = _host(batch)
        full = torch.zeros(int(rec["offsets"][-1]) + 32, dtype=torch.float64, device=DEV)
        ltp.sampleBatchEx(batch, 0, ROWS_N, full, sampler="fused")
        torch.cuda.synchronize()
        # what the named sets hardly produce: a fifth of the scaled lanes carry fallback records (t_scaled == t_opt, v_drive == v_max),
        # many lanes the modified jerk profile, and every case is among the sampled plans
        fallback = (rec["t_scaled"] == rec["t_opt"]).all(axis=2) & (rec["v_drive"] == np.asarray(lim["v_max"])) & (cen["case"] == 0)
        assert fallback.sum() >= 0.15 * (cen["case"] >= 0).sum() and rec["mod"].sum() >= 0.15 * rec["mod"].size
        assert all((cen["case"] == c).sum() >= 5 for c in bc.CASES)
        _ROWS.update(dof=dof, ts=ts, lim=lim, qs=qs, cen=cen, ltp=ltp, batch=batch, rec=_host(batch), full=full, host=full.cpu().numpy(),
                     orc=orc, orec={k: v[:ROWS_N] for k, v in orec.items() if isinstance(v, np.ndarray)})
    return _ROWS


def test_every_sampler_has_the_bits_of_the_fused_rows(oracle_mod):
    import torch
    from longtermplanner_amd import unpack_trajectory
    R = _rows_batch(oracle_mod)
    ltp, batch, n, dof, cen = R["ltp"], R["batch"], ROWS_N, R["dof"], R["cen"]
    status = R["rec"]["status"]
    assert (R["rec"]["traj_len"] > 0).sum() >= 0.98 * n and (status & 8).sum() >= 1

    def names(p):
        return bc.describe(cen, np.arange(n) == p)
    # the whole rows through every sampler, and as float32
    for sampler in ("auto", "walk", "walk_streaming", "table"):
        tile = torch.zeros_like(R["full"])
        ltp.sampleBatchEx(batch, 0, n, tile, sampler=sampler)
        torch.cuda.synchronize()
        assert np.array_equal(_host(batch)["status"], status), sampler
        if not torch.equal(tile.view(torch.int64), R["full"].view(torch.int64)):
            got = tile.cpu().numpy()
            off = R["rec"]["offsets"].astype(np.int64)
            bad = [p for p in range(n) if not _bits_equal(got[off[p]:off[p + 1]], R["host"][off[p]:off[p + 1]])]
            raise AssertionError(f"sampler {sampler}: rows of {len(bad)} plans differ from the fused sampler's: {bc.describe(cen, np.isin(np.arange(n), bad))}")
    for sampler in ("auto", "fused", "walk", "table"):
        f32 = torch.zeros(R["full"].numel(), dtype=torch.float32, device=DEV)
        ltp.sampleBatchEx(batch, 0, n, f32, sampler=sampler)
        torch.cuda.synchronize()
        assert torch.equal(f32, R["full"].to(torch.float32)), f"float32 rows ({sampler}) are not the float64 rows rounded once"
    # capped rows and a stride: the same samples
    for cap, stride in ((16, 1), (32, 1), (256, 1), (0, 4), (50, 7)):
        p2 = _planner(dof, R["lim"], R["ts"], max_samples=cap, stride=stride)
        b2 = p2.planSwitchTimesBatch(*_tensors(R["qs"]))
        r2 = _host(b2)
        assert np.array_equal(r2["traj_len"], R["rec"]["traj_len"])
        for sampler in ("auto", "fused", "walk", "table"):
            tile = torch.zeros(int(r2["offsets"][-1]) + 32, dtype=torch.float64, device=DEV)
            p2.sampleBatchEx(b2, 0, n, tile, sampler=sampler)
            torch.cuda.synchronize()
            assert np.array_equal(_host(b2)["status"], status), (cap, stride, sampler, "the end-limit check sees the whole trajectory")
            got = tile.cpu().numpy()
            for p in range(n):
                L = int(r2["traj_len"][p])
                if L <= 0:
                    continue
                stored = p2.storedSamples(L)
                want_cnt = -(-L // stride)
                assert stored == (min(want_cnt, cap) if cap else want_cnt)
                want = _plan_rows(R, p)[:, :, ::stride][:, :, :stored]
                have = np.stack(unpack_trajectory(got, int(r2["offsets"][p]), dof, stored))
                assert _bits_equal(want, have), f"cap {cap} stride {stride} sampler {sampler}: plan {p} differs from the full rows: {names(p)}"


def test_readers_have_the_bits_of_the_full_rows(oracle_mod):
    """stateAt, sampleWindow (k = 0, a uniform k, per-plan k), replanStates, sampleHorizon and sampleKnots (float64 and float32) read
    records whose shapes the named sets hardly produce: no phase 2 or 6, zero cruise, the fallback, c7 / c8, OPT_FAILED neighbours
    in the block."""
    import torch
    R = _rows_batch(oracle_mod)
    ltp, batch, n, dof, cen = R["ltp"], R["batch"], ROWS_N, R["dof"], R["cen"]
    lens = R["rec"]["traj_len"].astype(np.int64)
    rng = np.random.default_rng(17)
    N = 64
    per_plan = rng.integers(0, np.maximum(lens, 1) + 40).astype(np.int32)
    per_plan[::9] = np.maximum(lens[::9] - N // 2, 0)                      # windows that straddle the end
    for what, k in (("k = 0", 0), ("uniform k", 137), ("per-plan k", per_plan)):
        kh = np.full(n, k, dtype=np.int32) if np.ndim(k) == 0 else k
        rows, valid = ltp.sampleWindow(batch, 0, n, k if np.ndim(k) == 0 else torch.from_numpy(k).to(DEV), N)
        torch.cuda.synchronize()
        exp, exp_valid = _window_expected(R, kh, N)
        got = rows.cpu().numpy()[..., :N]
        same = ((got.view(np.uint64) == exp.view(np.uint64)) | (np.isnan(got) & np.isnan(exp))).reshape(n, -1).all(axis=1)
        assert same.all(), f"sampleWindow {what}: {int((~same).sum())} plans differ from the full rows: {bc.describe(cen, ~same)}"
        assert np.array_equal(valid.cpu().numpy(), exp_valid), what
    gen = torch.Generator(device=DEV).manual_seed(5)
    tl = batch.traj_len
    for mode in ("random", "first", "last", "beyond", "uniform"):
        k = {"random": lambda: (torch.rand(n, device=DEV, generator=gen) * tl.clamp(min=1)).to(torch.int32),
             "first": lambda: torch.zeros(n, dtype=torch.int32, device=DEV), "last": lambda: (tl - 1).clamp(min=0).to(torch.int32),
             "beyond": lambda: (tl + 1000).to(torch.int32), "uniform": lambda: 137}[mode]()
        want = ltp.replanStates(batch, 0, n, R["full"], k)
        got = ltp.stateAt(batch, 0, n, k)
        got_jm = ltp.stateAt(batch, 3, n - 5, k if isinstance(k, int) else k[3:n - 2].contiguous(), layout="joint_major")
        torch.cuda.synchronize()
        for w, g, gj in zip(want, got, got_jm):
            bad = (w.view(torch.int64) != g.view(torch.int64)).any(dim=1).cpu().numpy()
            assert not bad.any(), f"stateAt ({mode}) differs from the sampled rows: {bc.describe(cen, bad)}"
            assert torch.equal(w[3:n - 2].t().contiguous(), gj), mode
    # and the state at k from the rows themselves (replanStates is a gather), k = 137
    q, v, a = (x.cpu().numpy() for x in ltp.stateAt(batch, 0, n, 137))
    for p in range(0, n, 3):
        if lens[p] > 0:
            rows = _plan_rows(R, p)
            kk = min(137, int(lens[p]) - 1)
            assert _bits_equal(np.stack([q[p], v[p], a[p]]), rows[:3, :, kk]), bc.describe(cen, np.arange(n) == p)
    # sampleHorizon and sampleKnots (float64, and float32 = the float64 rows rounded once) through the shared yardstick: the three
    # smallest grids and the MPC grid, a uniform k swept over 0 .. 8 and per-plan starts with negative and past-the-end ones
    describe = lambda plans: bc.describe(cen, plans)
    ku = H.uniform_starts(rng, lens)
    assert np.count_nonzero(ku < 0) > 0 and np.count_nonzero(ku >= lens) > 0 and (lens == 0).sum() >= 3
    for Nh, s in ((64, 3), (33, 40)):
        H.assert_rows(lambda k, out: ltp.sampleHorizon(batch, 0, n, k, Nh, s, out=out), ltp, batch, R["full"], ku, hc.stride_grid(Nh, s), 0, n,
                      f"sampleHorizon N {Nh} stride {s}", stride=s, describe=describe)
    full = {torch.float64: R["full"], torch.float32: R["full"].to(torch.float32)}
    first, count = H.odd_range(n, dof)
    for gname, g in dict(kc.SMALL_GRIDS, mpc=kc.GRIDS["mpc"]).items():
        read = lambda lo, m: (lambda k, out: ltp.sampleKnots(batch, lo, m, k, H.grid_tensor(g), out=out))
        for k in list(range(9)) + [ku, per_plan]:
            kh = np.full(n, k, dtype=np.int32) if isinstance(k, int) else k
            for dt, rows in full.items():
                what = f"sampleKnots {dt} grid {gname} k {'per plan' if not isinstance(k, int) else k}"
                H.assert_rows(read(0, n), ltp, batch, rows, kh, g, 0, n, what, dtype=dt, describe=describe)
        H.assert_rows(read(first, count), ltp, batch, R["full"], ku, g, first, count, f"sampleKnots grid {gname}, plans [{first}, {first + count})", describe=describe)
    del full
    # replanStates skips what the sampler skipped: a tile that holds the first 150 plans only
    from longtermplanner_amd import STATUS_OVERFLOW
    off = R["rec"]["offsets"]
    b2 = ltp.planSwitchTimesBatch(*_tensors(R["qs"]))
    big = torch.full((int(off[-1]) + 64,), float("nan"), dtype=torch.float64, device=DEV)
    tile = big[:int(off[150] - off[0]) + 8]
    ltp.sampleBatch(b2, 0, n, tile)
    torch.cuda.synchronize()
    over = (b2.status.cpu().numpy() & STATUS_OVERFLOW) != 0
    assert over[150:][lens[150:] > 0].all() and not over[:150].any()
    q1, v1, a1 = (x.cpu().numpy() for x in ltp.replanStates(b2, 0, n, tile, 50))
    for p in range(n):
        if over[p] or lens[p] <= 0:
            assert _bits_equal(np.stack([q1[p], v1[p], a1[p]]), np.stack([R["qs"][1][p], R["qs"][2][p], R["qs"][3][p]])), p
        else:
            assert _bits_equal(np.stack([q1[p], v1[p], a1[p]]), _plan_rows(R, p)[:3, :, min(50, int(lens[p]) - 1)]), bc.describe(cen, np.arange(n) == p)
    assert not np.isnan(q1).any()


def test_analytic_envelopes_by_class(oracle_mod):
    """envelopeBatch: the exhaustive form has the bits of the reduced full rows, the analytic form (which reasons about profile
    shapes) agrees with it as test_analytic_envelopes_agree_with_the_exhaustive_form requires — NaN pattern and statuses identical, a
    subset of the samples, within 1e-12 — and both are within 1e-9 of the oracle's reduced rows."""
    import torch
    R = _rows_batch(oracle_mod)
    ltp, n, dof, cen = R["ltp"], ROWS_N, R["dof"], R["cen"]
    lens = R["rec"]["traj_len"].astype(np.int64)
    worst, worst_oracle = 0.0, 0.0
    try:
        for window, n_windows, table_pass in ((64, 40, 0), (129, 20, -1), (37, 70, 1), (1, 50, 0), (700, 4, 0)):
            ltp.setTablePass(table_pass)
            red = np.full((n, dof, n_windows, 2), np.nan)
            for p in range(n):
                if lens[p] > 0:
                    q = _plan_rows(R, p)[0]
                    pad = np.concatenate([q, np.repeat(q[:, -1:], max(window * n_windows - int(lens[p]), 0) + window, axis=1)], axis=1)
                    w = pad[:, : window * n_windows].reshape(dof, n_windows, window)
                    red[p, :, :, 0], red[p, :, :, 1] = w.min(axis=2), w.max(axis=2)
            res = {}
            for mode in ("exhaustive", "analytic"):
                ltp.setEnvelopeMode(mode)
                b = ltp.planSwitchTimesBatch(*_tensors(R["qs"]))
                env = ltp.envelopeBatch(b, 0, n, window, n_windows)
                assert ("analytic" in ltp.lastSamplerKernel()) == (mode == "analytic"), ltp.lastSamplerKernel()
                torch.cuda.synchronize()
                res[mode] = (env.cpu().numpy(), b.status.cpu().numpy())
            ex, an = res["exhaustive"][0], res["analytic"][0]
            what = f"window {window} x {n_windows}, table pass {table_pass}"
            bad = ~((ex.view(np.uint64) == red.view(np.uint64)) | (np.isnan(ex) & np.isnan(red))).all(axis=(2, 3))
            assert not bad.any(), f"{what}: exhaustive envelopes differ from the reduced rows: {bc.describe(cen, bad)}"
            assert np.array_equal(np.isnan(ex), np.isnan(an)) and np.array_equal(res["exhaustive"][1], res["analytic"][1]), what
            ok = ~np.isnan(ex)
            d = np.where(ok, np.abs(np.where(ok, ex - an, 0.0)), 0.0)
            assert d.max() <= 1e-12, f"{what}: analytic envelopes differ by {d.max()}: {bc.describe(cen, (d > 1e-12).any(axis=(2, 3)))}"
            worst = max(worst, float(d.max()))
            sub = ok & (np.stack([an[..., 0] < ex[..., 0], an[..., 1] > ex[..., 1]], axis=-1))
            assert not sub.any(), f"{what}: an analytic envelope lies outside the samples: {bc.describe(cen, sub.any(axis=(2, 3)))}"
            if window in (64, 129):
                for p in range(0, n, 29):
                    if lens[p] == 0:
                        continue
                    o = R["orc"].plan_trajectory(*[x[p] for x in R["qs"]])
                    qo, L = o["q"], o["length"]
                    pad = np.concatenate([qo, np.repeat(qo[:, -1:], max(window * n_windows - L, 0) + window, axis=1)], axis=1)
                    wo = pad[:, : window * n_windows].reshape(dof, n_windows, window)
                    d = max(float(np.max(np.abs(an[p, :, :, 0] - wo.min(axis=2)))), float(np.max(np.abs(an[p, :, :, 1] - wo.max(axis=2)))))
                    assert d <= TOL, f"{what}: plan {p} differs from the oracle's reduced rows by {d}: {bc.describe(cen, np.arange(n) == p)}"
                    worst_oracle = max(worst_oracle, d)
    finally:
        ltp.setTablePass(0)
        ltp.setEnvelopeMode("analytic")
    print(f"soft envelopes: analytic vs exhaustive worst |d| {worst:.2e}; vs the oracle's reduced rows {worst_oracle:.2e}")


def test_horizon_envelopes_by_class(oracle_mod):
    """envelopeKnots, the analytic form that reasons about profile shapes, on jerk-dominated records: the MPC, the duplicates and
    the geometric grid, both `closed` modes, per-plan starts from [-10, traj_len + 50) and k = 0, the whole batch and an odd
    sub-range, against the reduced full rows under the acceptance rule of the analytic envelope form; the NaN rows of the
    OPT_FAILED plans are part of the comparison. Every case 0-8 is among the plans compared."""
    R = _rows_batch(oracle_mod)
    ltp, batch, n, dof, cen = R["ltp"], R["batch"], ROWS_N, R["dof"], R["cen"]
    lens = R["rec"]["traj_len"]
    assert (lens == 0).sum() >= 3 and all(((cen["case"] == c) & (lens > 0)[:, None]).any() for c in bc.CASES)
    describe = lambda plans: bc.describe(cen, plans)
    rng = np.random.default_rng(41)
    first, count = H.odd_range(n, dof)
    assert (count * dof) % 64 != 0 and ((lens == 0)[first:first + count]).any()
    worst, least = 0.0, 1.0
    for gname in ("mpc", "duplicates", "geometric"):
        g = kc.GRIDS[gname]
        for closed in (0, 1):
            k = H.uniform_starts(rng, lens)
            for kk, lo, m in ((k, 0, n), (0, 0, n), (k, first, count)):
                what = f"soft dense envelopeKnots grid {gname} closed {closed} k {'per plan' if not isinstance(kk, int) else kk} plans [{lo}, {lo + m})"
                envs, fig = E.assert_envelopes(E.QONLY, ltp, batch, R["full"], kk, g, closed, lo, m, what, (1,), describe)
                worst, least = max(worst, fig["q"][0]), min(least, fig["q"][1])
                assert bool(np.isnan(envs[1].cpu().numpy()[(lens == 0)[lo:lo + m]]).all())
    print(f"soft dense horizon envelopes: worst |d| {worst:.3e}, least bit-identical share {least:.6f}")
    assert least >= 0.999, least


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
@pytest.mark.parametrize("dof", bc.RETIME_BATCHES)
def test_retime_reaches_and_matches_every_case(oracle_mod, dof, pow_rule):
    """ltp_retime_batch scales ALL joints: 1.05 / 1.5 / 3.0 x T* and random per-query targets against retime_checker.retime, the
    accepted cases against the floors; rows of 50 retimed plans against the checker's trajectory."""
    import torch
    from longtermplanner_amd import LongTermPlanner, unpack_trajectory
    n = bc.RECORD_BATCHES[dof]
    orc, lim, qs, orec, _ = bc.soft_batch(oracle_mod, dof, n, exact_pow=(pow_rule == "exact"), sample=False)
    exact = pow_rule == "exact" or LongTermPlanner.powRuleMatchingHostLibm()[0] == "libm"
    ltp = _planner(dof, lim, pow_rule=pow_rule)
    tens = _tensors(qs)
    rng = np.random.default_rng(n)
    for k in bc.RETIME_FACTORS + ("random",):
        batch = ltp.planSwitchTimesBatch(*tens)
        plain = _host(batch)
        assert np.array_equal(rc.oracle_eligible(orec), rc.device_eligible(plain))
        ts = rc.t_star(plain)           # the device's own T*: the oracle's bits where `exact`, within 1e-9 of it otherwise
        if k == "random":
            T = ts * rng.uniform(0.5, 4.0, n)
            T[rng.random(n) < 0.05] = np.nan
        else:
            T = k * ts
        ltp.retimeBatch(batch, t_target=torch.from_numpy(np.ascontiguousarray(T)).to(DEV))
        dev = _host(batch)
        chk, retimed, cases = rc.retime(orc, orec, *qs, T)
        what = f"soft dof {dof} {pow_rule} retime {k}"
        tot = dict(cases={c: int(cases[:, c].sum()) for c in bc.CASES}, sites={})
        print(f"{what}: retimed {int(retimed.sum())}, cases {tot['cases']}")
        bc.assert_reaches(tot, bc.FLOOR, 0, sites=())
        assert sum(tot["cases"].values()) == dof * retimed.sum() and sum(tot["cases"][c] for c in range(3, 9)) >= 0.3 * dof * retimed.sum()
        with np.errstate(invalid="ignore"):
            assert np.array_equal(retimed, rc.device_eligible(plain) & (T > ts))
        assert _agree(dev["t_required"][retimed], T[retimed], True).all(), what
        keys = ("t_scaled", "v_drive", "mod", "traj_len")
        bad = {key: ~_agree(dev[key], chk[key], exact).reshape(n, -1).all(axis=1) & retimed for key in keys}
        bad = {key: b for key, b in bad.items() if b.any()}
        if bad:
            cen = bc.census(orc, lim, qs, orec, t_required=T)
            lanes = {key: (~_agree(dev[key], chk[key], exact)).reshape(n, dof, -1).any(axis=2) & retimed[:, None] if dev[key].ndim > 1
                     else np.repeat(b[:, None], dof, axis=1) for key, b in bad.items()}
            raise AssertionError(f"{what}: " + "; ".join(f"{key} differs: {bc.describe(cen, l)}" for key, l in lanes.items()))
        keep = ~retimed
        for key in REC_KEYS:
            assert _agree(dev[key][keep], plain[key][keep], True).all(), (what, key, "a query that was not retimed changed")
        assert np.all((dev["status"][retimed] & ~16) == 0)
        if k == 1.5:
            first = np.nonzero(retimed)[0][:50]
            lo, hi = int(first[0]), int(first[-1]) + 1
            off = dev["offsets"]
            tile = torch.zeros(int(off[hi] - off[lo]) + 32, dtype=torch.float64, device=DEV)
            ltp.sampleBatchEx(batch, lo, hi - lo, tile)
            torch.cuda.synchronize()
            rows = tile.cpu().numpy()
            for p in first:
                L, q, v, a, j = rc.trajectory(orc, chk, p, qs[1], qs[2], qs[3])
                assert L == dev["traj_len"][p]
                got = unpack_trajectory(rows, int(off[p] - off[lo]), dof, L)
                d = max(float(np.max(np.abs(g - o))) for g, o in zip(got, (q, v, a, j)))
                assert d <= TOL, f"{what}: rows of plan {p} differ from the checker's by {d}"


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
def test_limit_sets_mix_soft_and_named_sets(oracle_mod, pow_rule):
    """One batch whose queries use the soft set, panda or ref: queue B then holds lanes of different sets side by side. Bit for bit
    what the per-set handles give."""
    import torch
    from longtermplanner_amd import generate_queries, limit_set
    n = bc.RECORD_BATCHES[7]
    _, soft, soft_qs, _, cen = bc.soft_batch(oracle_mod, 7, n, exact_pow=(pow_rule == "exact"))
    sets = [soft, limit_set("panda")[1], limit_set("ref")[1]]
    per = [soft_qs] + [generate_queries(n, s, seed=bc.SEED + 10 * k) for k, s in enumerate(sets[1:], 1)]
    idx = np.random.default_rng(3).integers(0, 3, n).astype(np.int32)
    qs = [np.ascontiguousarray(np.choose(idx[:, None], [p[f] for p in per])) for f in range(4)]
    ltp = _planner(7, soft, pow_rule=pow_rule)
    ltp.setLimitSets(*[np.array([s[k] for s in sets], dtype=np.float64) for k in ("q_min", "q_max", "v_max", "a_max", "j_max")])
    b = ltp.planSwitchTimesBatch(*_tensors(qs), limit_set=torch.from_numpy(idx).to(DEV))
    ltp.endLimit(b, 0, n)
    mixed = _host(b)
    for s, lim in enumerate(sets):
        ps = _planner(7, lim, pow_rule=pow_rule)
        bs = ps.planSwitchTimesBatch(*_tensors(qs))
        ps.endLimit(bs, 0, n)
        ref = _host(bs)
        m = idx == s
        for k in REC_KEYS:
            bad = ~_agree(mixed[k], ref[k], True).reshape(n, -1).all(axis=1) & m
            assert not bad.any(), (f"set {s} {pow_rule}: {k} of {int(bad.sum())} queries differs from the per-set handle"
                                   + (f": {bc.describe(cen, bad)}" if s == 0 else ""))
        assert np.array_equal(np.diff(mixed["offsets"].astype(np.int64))[m], np.diff(ref["offsets"].astype(np.int64))[m]), s
    soft_lanes = {c: int(((cen["case"] == c) & (idx == 0)[:, None]).sum()) for c in bc.CASES}
    assert min(soft_lanes.values()) >= 5, soft_lanes


def test_matlab_semantics_by_class(oracle_mod):
    """Records and matlab_flags of the soft batch against Oracle(semantics="matlab"); the floors hold for that oracle too."""
    from longtermplanner_amd import STATUS_END_LIMIT, STATUS_MATLAB_COMPLEX, STATUS_MATLAB_ERROR
    n = bc.RECORD_BATCHES[7]
    orc, lim, qs, orec, cen = bc.soft_batch(oracle_mod, 7, n, semantics="matlab", sample=False)
    bc.assert_floors(cen["totals"], matlab=True)
    ltp = _planner(7, lim, semantics="matlab")
    dev = ltp.planBatchHost(*qs, sample=False)
    planned = orec["status"] != 0
    dev_planned = (dev["status"] & ~STATUS_MATLAB_COMPLEX) == 0
    assert np.array_equal(dev_planned, planned), bc.describe(cen, dev_planned != planned)
    for bit, flag in ((STATUS_MATLAB_ERROR, 2), (STATUS_MATLAB_COMPLEX, 1)):
        diff = ((dev["status"] & bit) != 0) != ((orec["matlab_flags"] & flag) != 0)
        assert not diff.any(), f"matlab flag {flag} differs: {bc.describe(cen, diff)}"
    assert not np.any(dev["status"] & STATUS_END_LIMIT)
    _assert_classes(dev, orec, cen, False, planned, "soft dof 7 matlab")
    print(f"soft matlab: {int(planned.sum())} plans, complex flags {int(np.sum(orec['matlab_flags'] & 1))}, errors {int(np.sum((orec['matlab_flags'] & 2) != 0))}")


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
def test_single_call_time_scaling_has_the_bits_of_the_batch(oracle_mod, pow_rule):
    """ltp.timeScaling (the single-call kernel) on at least 5 lanes of each case 0-8 drawn from the census: the case the oracle
    accepts and the bits the batched records hold (case 0: zeros and v_max, where the batch holds the fallback's optimal times)."""
    n = bc.RECORD_BATCHES[7]
    orc, lim, qs, orec, cen = bc.soft_batch(oracle_mod, 7, n, exact_pow=(pow_rule == "exact"))
    ltp = _planner(7, lim, pow_rule=pow_rule)
    dev = ltp.planBatchHost(*qs, sample=False)
    rng = np.random.default_rng(11)
    for c in bc.CASES:
        lanes = np.argwhere(cen["case"] == c)
        assert len(lanes) >= 5
        for q, j in lanes[rng.choice(len(lanes), 6, replace=False)]:
            ok, t, vd, mod, case = ltp.timeScaling(int(j), qs[0][q, j], qs[1][q, j], qs[2][q, j], qs[3][q, j], dev["dir"][q, j], dev["t_required"][q])
            what = f"{pow_rule}: query {q} joint {j}: c{c}, sites {cen['site_bits'][q, j]}"
            assert case == c and ok == (c != 0), f"{what}: the single call ended in c{case}"
            if c == 0:
                assert not t.any() and vd == lim["v_max"][j] and mod == 0, what
                assert _bits_equal(dev["t_scaled"][q, j], dev["t_opt"][q, j]) and dev["v_drive"][q, j] == lim["v_max"][j] and dev["mod"][q, j] == 0, what
            else:
                assert _bits_equal(t, dev["t_scaled"][q, j]) and _bits_equal(np.float64(vd), dev["v_drive"][q, j]) and mod == dev["mod"][q, j], (
                    f"{what}: the single call differs from the batched record: {t} {vd} {mod} against {dev['t_scaled'][q, j]} {dev['v_drive'][q, j]} {dev['mod'][q, j]}")
