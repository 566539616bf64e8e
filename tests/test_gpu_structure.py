"""Structured queries on the GPU: joints that rest, that sit within eps of their goal, that only have to stop, twins and mirrors of
another joint, whole queries in which nothing moves, one joint moves, or every joint asks for the same motion (tests/structure_census.py).
Every other multi-joint test draws the four inputs of every joint independently; such queries never tie, never stand still and never
reach the `bj < slowest` clause of the slowest-joint reduction, timeScaling at T equal to a joint's own optimum or for a joint with
dir == 0, the fallback as a bulk path under the named limit sets, or records whose v_drive is +inf.

Records, MATLAB semantics, limit sets, ragged cuts, the single-call kernel, dense rows, every sampler, the readers of records, stop
horizons, retime
and the end-limit verdict are compared with the CPU oracle (or with each other where the suite claims bits), class by class: a
mismatch names the kind, the timeScaling case, the query shape and the tie class of the lanes concerned, and a class that the CPU
test (tests/test_structure_census_cpu.py) says exists must be present in the comparison.

Tolerances are the suite's own: bit identity under pow_rule "exact" against the oracle's exact-pow twin and under "libm" behind the
restated_host_libm fixture, 1e-9 otherwise; non-finite values compare as bit patterns."""
import ctypes as C
import os

import numpy as np
import pytest

import envelope_checker as ec
import horizon_checker as hc
import horizon_helpers as H
import knots_checker as kc
import retime_checker as rc
import structure_census as sc
from gpu_helpers import DEV, REC_KEYS, TOL, _agree, _bits_equal, _host, _plan_rows, _planner, _tensors, _window_expected
from structure_census import NEAR, REST, ROWS_N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE_KEYS = ("t_opt", "t_scaled", "dir", "mod", "v_drive")
QUERY_KEYS = ("t_required", "slowest", "traj_len")
ALWAYS_EXACT = ("dir", "mod", "t_required", "slowest", "traj_len")          # whatever the pow rule and the host's libm


def _disagreements(dev, ref, exact, mask, keys=LANE_KEYS + QUERY_KEYS):
    """{key: lane mask [n][dof]} of the record fields in which the queries of `mask` [n] disagree (query fields spread over the joints)."""
    D = dev["dir"].shape[1]
    out = {}
    for k in keys:
        bad = ~_agree(dev[k], ref[k], exact or k in ALWAYS_EXACT)
        bad = bad.reshape(bad.shape[0], D, -1).any(axis=2) if k in LANE_KEYS else np.repeat(bad[:, None], D, axis=1)
        bad &= mask[:, None]
        if bad.any():
            out[k] = bad
    return out


def _assert_classes(dev, ref, S, exact, mask, what, keys=LANE_KEYS + QUERY_KEYS, present=None):
    """dev == ref over the queries of `mask`, class by class: each class that exists in the batch is non-empty in the comparison and
    compared as its own group; every lane belongs to a kind x case cell."""
    bad = _disagreements(dev, ref, exact, mask, keys)
    must = set(sc.present(S) if present is None else present)
    for name, lanes in sc.classes(S):
        lanes = lanes & mask[:, None]
        if name in must:
            assert lanes.any(), f"{what}: no lane of class {name} in this comparison: it would prove nothing about it"
        for k, b in bad.items():
            hit = b & lanes
            assert not hit.any(), (f"{what}: class {name}: {k} differs from the reference ({'bits' if exact or k in ALWAYS_EXACT else '1e-9'}): "
                                   f"{sc.describe(S, hit)}")
    assert not bad, f"{what}: {sorted(bad)} differ outside every class"


def _batch(oracle_mod, name, pow_rule="libm", semantics="cpp"):
    return sc.batch(oracle_mod, name, semantics=semantics, exact_pow=(pow_rule == "exact"), sample=(semantics == "cpp"))


def _records_case(oracle_mod, name, layout, pow_rule, exact):
    from longtermplanner_amd import STATUS_END_LIMIT
    S = _batch(oracle_mod, name, pow_rule)
    sc.assert_floors(S)
    orec = S["rec"]
    ltp = _planner(S["dof"], S["lim"], pow_rule=pow_rule)
    dev = _host(ltp.planSwitchTimesBatch(*_tensors(S["qs"], layout), layout=layout, end_limit=True))
    what = f"{name} {layout} {pow_rule}"
    planned = orec["status"] != 0
    assert planned.all()
    dev_planned = (dev["status"] & ~STATUS_END_LIMIT) == 0
    assert np.array_equal(dev_planned, planned), f"{what}: planned verdicts differ: {sc.describe(S, dev_planned != planned)}"
    end = (dev["status"] & STATUS_END_LIMIT) != 0
    assert np.array_equal(end, orec["status"] == 2), f"{what}: end-limit verdicts differ: {sc.describe(S, end != (orec['status'] == 2))}"
    # the tie rule first, so that a wrong slowest joint is reported as such and under its tie class
    wrong = dev["slowest"] != orec["slowest"]
    by_tie = {cls: f"{int((m & wrong).sum())} of {int(m.sum())}" for cls, m in sc.tie_classes(S["tie"], S["dof"]).items() if (m & wrong).any()}
    assert not wrong.any(), (f"{what}: slowest is not the first maximum of t_opt[..][6] in {int(wrong.sum())} queries; by tie class {by_tie}, "
                             f"{int((wrong & ~S['tie']['tied']).sum())} of them not tied: {sc.describe(S, wrong)}")
    _assert_classes(dev, orec, S, exact, planned, what)
    # nothing non-finite leaks: v_drive is +inf exactly where the oracle's is, everything else is finite
    assert np.array_equal(np.isinf(dev["v_drive"]), np.isinf(orec["v_drive"])) and not np.isnan(dev["v_drive"]).any(), what
    assert all(np.isfinite(dev[k]).all() for k in ("t_opt", "t_scaled", "dir", "t_required")), what
    return dev


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
@pytest.mark.parametrize("layout", ["query_major", "joint_major"])
@pytest.mark.parametrize("name", list(sc.BATCHES))
def test_records_by_class(oracle_mod, name, layout, pow_rule):
    """"exact": the bits of the exact-pow twin; "libm": within 1e-9 of the parity oracle on any host (bits: the next test). slowest,
    t_required, traj_len, status and dir are the oracle's exactly under either rule."""
    _records_case(oracle_mod, name, layout, pow_rule, exact=(pow_rule == "exact"))


@pytest.mark.parametrize("layout", ["query_major", "joint_major"])
@pytest.mark.parametrize("name", list(sc.BATCHES))
def test_records_have_the_libm_oracles_bits_by_class(oracle_mod, name, layout, restated_host_libm):
    _records_case(oracle_mod, name, layout, "libm", exact=True)


@pytest.mark.parametrize("name", ["panda7", "ref7"])
def test_matlab_semantics_by_class(oracle_mod, name):
    """Records and matlab_flags against Oracle(semantics="matlab"), which accepts other candidates for a lane that stands still."""
    from longtermplanner_amd import STATUS_END_LIMIT, STATUS_MATLAB_COMPLEX, STATUS_MATLAB_ERROR
    S = _batch(oracle_mod, name, semantics="matlab")
    sc.assert_floors(S)
    orec = S["rec"]
    ltp = _planner(S["dof"], S["lim"], semantics="matlab")
    dev = ltp.planBatchHost(*S["qs"], sample=False)
    planned = orec["status"] != 0
    dev_planned = (dev["status"] & ~STATUS_MATLAB_COMPLEX) == 0
    assert np.array_equal(dev_planned, planned), sc.describe(S, dev_planned != planned)
    for bit, flag in ((STATUS_MATLAB_ERROR, 2), (STATUS_MATLAB_COMPLEX, 1)):
        diff = ((dev["status"] & bit) != 0) != ((orec["matlab_flags"] & flag) != 0)
        assert not diff.any(), f"{name}: matlab flag {flag} differs: {sc.describe(S, diff)}"
    assert not np.any(dev["status"] & STATUS_END_LIMIT)
    _assert_classes(dev, orec, S, False, planned, f"{name} matlab")
    assert np.array_equal(np.isinf(dev["v_drive"]), np.isinf(orec["v_drive"])) and not np.isnan(dev["v_drive"]).any()


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
def test_limit_sets_merge_panda_and_ref(oracle_mod, pow_rule):
    """The panda and ref batches merged into one mixed batch (ltp_set_limit_sets / ltp_bind_limit_sets): standing and tied queries of
    the two sets side by side in a block. Bit for bit what the per-set handles give."""
    import torch
    per = [_batch(oracle_mod, "panda7", pow_rule), _batch(oracle_mod, "ref7", pow_rule)]
    n = per[0]["n"]
    assert per[1]["n"] == n
    idx = (sc.unit_random(sc.SEED + 3, np.arange(n, dtype=np.uint64), 0, 0) < 0.5).astype(np.int32)
    qs = [np.ascontiguousarray(np.choose(idx[:, None], [p["qs"][f] for p in per])) for f in range(4)]
    sets = [p["lim"] for p in per]
    ltp = _planner(7, sets[0], pow_rule=pow_rule)
    ltp.setLimitSets(*[np.array([s[k] for s in sets], dtype=np.float64) for k in ("q_min", "q_max", "v_max", "a_max", "j_max")])
    b = ltp.planSwitchTimesBatch(*_tensors(qs), limit_set=torch.from_numpy(idx).to(DEV))
    ltp.endLimit(b, 0, n)
    mixed = _host(b)
    for s, S in enumerate(per):
        ps = _planner(7, S["lim"], pow_rule=pow_rule)
        bs = ps.planSwitchTimesBatch(*_tensors(qs))
        ps.endLimit(bs, 0, n)
        ref = _host(bs)
        m = idx == s
        assert np.array_equal(mixed["status"][m], ref["status"][m]), f"set {s}: statuses differ: {sc.describe(S, m & (mixed['status'] != ref['status']))}"
        # (the classes of S describe the queries of set s only: those are the ones compared)
        _assert_classes(mixed, ref, S, True, m, f"limit set {s} {pow_rule} against its own handle")
        assert np.array_equal(np.diff(mixed["offsets"].astype(np.int64))[m], np.diff(ref["offsets"].astype(np.int64))[m]), s
        # and the per-set handle on ITS batch is what the records test compares with the oracle: the merged queries are that batch's
        assert all(np.array_equal(q[m], x[m]) for q, x in zip(qs, S["qs"]))


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
@pytest.mark.parametrize("name", ["ref7", "ref9", "ref30"])
def test_ragged_cuts_have_the_bits_of_the_whole_batch(oracle_mod, name, pow_rule):
    """1, 63, 64, 65 and 130 queries cut from the batch, from the middle of a run of tied queries: partial blocks whose first lanes
    tie. Each cut has the bits of the whole batch."""
    S = _batch(oracle_mod, name, pow_rule)
    tied = S["tie"]["tied"] & (S["tie"]["T"] > 0)
    run = np.nonzero(S["shape"] == sc.ALL_TWINS)[0]
    start = int(run[sc.RUN + 4])                 # inside the second run of all_twins queries
    assert tied[start - 2:start + 5].all() and S["shape"][start - 4] == sc.ALL_TWINS, "the cut starts inside a run of tied queries"
    ltp = _planner(S["dof"], S["lim"], pow_rule=pow_rule)
    whole = _host(ltp.planSwitchTimesBatch(*_tensors(S["qs"])))
    for m in (1, 63, 64, 65, 130):
        sl = slice(start, start + m)
        part = _host(ltp.planSwitchTimesBatch(*_tensors([x[sl] for x in S["qs"]])))
        in_cut = np.zeros(S["n"], dtype=bool)
        in_cut[sl] = True
        full = {k: np.zeros_like(whole[k]) for k in REC_KEYS}
        for k in REC_KEYS:
            full[k][sl] = part[k]
        assert np.array_equal(full["status"][sl], whole["status"][sl]), f"{name} {pow_rule}: {m} queries from {start}: statuses differ"
        if m >= 63:
            for cls in ("later_row_first_jb4", "three_or_more", "one_mover") + (("all_rest",) if m == 130 else ()):
                assert (dict(sc.classes(S))[cls][sl]).any(), f"the cut of {m} holds no query of class {cls}"
        _assert_classes(full, whole, S, True, in_cut, f"{name} {pow_rule}: {m} queries from {start} against the whole batch", present=())
        assert np.array_equal(np.diff(part["offsets"].astype(np.int64)), np.diff(whole["offsets"].astype(np.int64))[sl])


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
@pytest.mark.parametrize("name", ["ref9", "panda7"])
def test_single_calls_have_the_bits_of_the_batch(oracle_mod, name, pow_rule):
    """planTrajectory (k_plan_small, which has its own copy of the tie rule) on 20 plans of every query shape and every tie class:
    the batch's verdict, records and row bits."""
    S = _batch(oracle_mod, name, pow_rule)
    no = sc.impossible(S["set"], S["dof"])
    groups = [(cls, m.any(axis=1)) for cls, m in sc.classes(S) if "." not in cls and cls not in no]
    assert len(groups) == (12 if name == "ref9" else 6)
    chosen = {}
    for cls, m in groups:
        plans = np.nonzero(m)[0]
        assert len(plans) >= 20, cls
        for p in plans[np.linspace(0, len(plans) - 1, 20).astype(np.int64)]:
            chosen.setdefault(int(p), cls)
    plans = np.array(sorted(chosen))
    assert len(plans) * S["dof"] > 128, "the chosen plans together go through the batched kernels"
    ltp = _planner(S["dof"], S["lim"], pow_rule=pow_rule)
    big = ltp.planBatchHost(*[x[plans] for x in S["qs"]], sample=True)
    for i, p in enumerate(plans):
        one = ltp.planBatchHost(*[x[p:p + 1] for x in S["qs"]], sample=True)
        what = f"{name} {pow_rule}: class {chosen[int(p)]}: plan {p}: {sc.describe(S, np.arange(S['n']) == p)}"
        for k in REC_KEYS:
            assert one[k].tobytes() == big[k][i:i + 1].tobytes(), f"{what}: {k} of the single call differs from the batch's: {one[k]} against {big[k][i]}"
        lo, hi = int(big["offsets"][i]), int(big["offsets"][i + 1])
        assert one["packed"].tobytes() == big["packed"][lo:hi].tobytes(), f"{what}: the single call's rows differ from the batch's"
    # and the batch of the chosen plans is the oracle's
    sub = {k: v[plans] for k, v in S["rec"].items() if isinstance(v, np.ndarray)}
    for k in ALWAYS_EXACT:
        assert np.array_equal(big[k], sub[k]), k
    print(f"{name} {pow_rule}: {len(plans)} single calls over {len(groups)} classes")


# ---- rows ----------------------------------------------------------------------------------------------------------------------------
_ROWS = {}


def _rows(oracle_mod, name):
    """The first ROWS_N plans of a batch, planned on the device (libm rule), with their full float64 rows from the fused sampler: the
    yardstick of the sampler and reader tests (itself compared with the oracle sample by sample in test_dense_rows)."""
    import torch
    if name not in _ROWS:
        S = _batch(oracle_mod, name)
        n = ROWS_N
        qs = [np.ascontiguousarray(x[:n]) for x in S["qs"]]
        ltp = _planner(S["dof"], S["lim"])
        batch = ltp.planSwitchTimesBatch(*_tensors(qs), end_limit=True)
        before = _host(batch)
        full = torch.zeros(int(before["offsets"][-1]) + 32, dtype=torch.float64, device=DEV)
        ltp.sampleBatchEx(batch, 0, n, full, sampler="fused")
        rec = _host(batch)
        for cls in sc.present(S):
            assert dict(sc.classes(S))[cls][:n].any(), f"{name}: no lane of class {cls} among the first {n} plans"
        _ROWS[name] = dict(S=S, n=n, dof=S["dof"], lim=S["lim"], qs=qs, ltp=ltp, batch=batch, rec=rec, before=before, full=full,
                           host=full.cpu().numpy(), still=np.isin(S["kind"][:n], (REST, NEAR)))
    return _ROWS[name]


def _names(R, plans):
    """describe() of whole plans of the rows batch (indices or a mask over its n plans)."""
    m = np.zeros(R["S"]["n"], dtype=bool)
    m[:R["n"]][plans] = True
    return sc.describe(R["S"], m)


def _assert_still_lanes(R, rows_of, lens, what):
    """Independent of the oracle: every stored sample of a rest or near lane is (q_0, +0, +0, +0) bit for bit, and nothing stored is
    non-finite. rows_of(p) -> [4][dof][stored]."""
    q0 = R["qs"][1]
    lanes = 0
    for p in range(R["n"]):
        if lens[p] <= 0:
            continue
        rows = rows_of(p)
        assert np.isfinite(rows).all(), f"{what}: plan {p} holds a non-finite sample: {_names(R, [p])}"
        for j in np.nonzero(R["still"][p])[0]:
            lanes += 1
            ok = (rows[0, j].view(np.uint64) == q0[p, j:j + 1].view(np.uint64)).all() and not rows[1:, j].view(np.uint64).any()
            assert ok, f"{what}: plan {p} joint {j} stands still but its rows are not (q_0, +0, +0, +0): {rows[:, j, :3]}: {_names(R, [p])}"
    assert lanes >= 1000, lanes


@pytest.mark.parametrize("name", ["panda7", "ref7"])
def test_dense_rows(oracle_mod, name):
    """Every q / v / a / j sample of ROWS_N plans within 1e-9 of the oracle's, lengths and end-limit verdicts exactly; ltp_end_limit_batch
    gave the verdict the sampler gives; lanes that stand still hold q_0; a query in which nothing moves under ref is one sample."""
    from longtermplanner_amd import STATUS_END_LIMIT
    R = _rows(oracle_mod, name)
    S, n, rec = R["S"], R["n"], R["rec"]
    assert np.array_equal(R["before"]["status"], rec["status"]), f"ltp_end_limit_batch differs from the sampler's verdict: {_names(R, R['before']['status'] != rec['status'])}"
    assert np.array_equal((rec["status"] & STATUS_END_LIMIT) != 0, S["rec"]["status"][:n] == 2) and not (rec["status"] & ~STATUS_END_LIMIT).any()
    assert np.array_equal(rec["traj_len"], S["rec"]["traj_len"][:n]), _names(R, rec["traj_len"] != S["rec"]["traj_len"][:n])
    worst, bad = 0.0, []
    for p in range(n):
        o = S["orc"].plan_trajectory(*[x[p] for x in R["qs"]])
        d = float(np.max(np.abs(_plan_rows(R, p) - np.stack([o["q"], o["v"], o["a"], o["j"]]))))
        worst = max(worst, d)
        if not d <= TOL:
            bad.append(p)
    print(f"{name}: dense rows of {n} plans, max |d| {worst:.3e}")
    assert not bad, f"{name}: rows of {len(bad)} plans differ from the oracle's by more than 1e-9 (worst {worst:.3e}): {_names(R, bad)}"
    _assert_still_lanes(R, lambda p: _plan_rows(R, p), rec["traj_len"], f"{name} fused rows")
    standing = R["still"].all(axis=1)
    assert standing.sum() >= sc.FLOOR
    if sc.has_twins(S["set"]):
        for p in np.nonzero(standing)[0]:
            rows = _plan_rows(R, p)
            assert rows.shape[2] == 1 and _bits_equal(rows[:, :, 0], np.stack([R["qs"][1][p]] + [np.zeros(R["dof"])] * 3)), _names(R, [p])


@pytest.mark.parametrize("name", ["panda7", "ref7"])
def test_every_sampler_has_the_bits_of_the_fused_rows(oracle_mod, name):
    import torch
    from longtermplanner_amd import unpack_trajectory
    R = _rows(oracle_mod, name)
    ltp, batch, n, dof = R["ltp"], R["batch"], R["n"], R["dof"]
    status = R["rec"]["status"]
    off = R["rec"]["offsets"].astype(np.int64)
    for sampler in ("walk", "walk_streaming", "table", "auto"):
        tile = torch.zeros_like(R["full"])
        ltp.sampleBatchEx(batch, 0, n, tile, sampler=sampler)
        torch.cuda.synchronize()
        assert np.array_equal(_host(batch)["status"], status), sampler
        if not torch.equal(tile.view(torch.int64), R["full"].view(torch.int64)):
            got = tile.cpu().numpy()
            bad = [p for p in range(n) if not _bits_equal(got[off[p]:off[p + 1]], R["host"][off[p]:off[p + 1]])]
            raise AssertionError(f"{name}: sampler {sampler}: rows of {len(bad)} plans differ from the fused sampler's: {_names(R, bad)}")
    for sampler in ("auto", "fused", "walk", "table"):
        f32 = torch.zeros(R["full"].numel(), dtype=torch.float32, device=DEV)
        ltp.sampleBatchEx(batch, 0, n, f32, sampler=sampler)
        torch.cuda.synchronize()
        want = R["full"].to(torch.float32)
        if not torch.equal(f32.view(torch.int32), want.view(torch.int32)):
            got, w = f32.cpu().numpy(), want.cpu().numpy()
            bad = [p for p in range(n) if not _bits_equal(got[off[p]:off[p + 1]], w[off[p]:off[p + 1]])]
            raise AssertionError(f"{name}: float32 rows ({sampler}) are not the float64 rows rounded once: {_names(R, bad)}")
    for cap, stride in ((32, 1), (0, 4)):
        p2 = _planner(dof, R["lim"], max_samples=cap, stride=stride)
        b2 = p2.planSwitchTimesBatch(*_tensors(R["qs"]))
        r2 = _host(b2)
        assert np.array_equal(r2["traj_len"], R["rec"]["traj_len"])
        for sampler in ("auto", "fused", "walk", "table"):
            tile = torch.zeros(int(r2["offsets"][-1]) + 32, dtype=torch.float64, device=DEV)
            p2.sampleBatchEx(b2, 0, n, tile, sampler=sampler)
            torch.cuda.synchronize()
            assert np.array_equal(_host(b2)["status"], status), (cap, stride, sampler, "the end-limit check sees the whole trajectory")
            got = tile.cpu().numpy()

            def stored_rows(p):
                L = int(r2["traj_len"][p])
                return np.stack(unpack_trajectory(got, int(r2["offsets"][p]), dof, p2.storedSamples(L)))
            for p in range(n):
                want = _plan_rows(R, p)[:, :, ::stride]
                want = want[:, :, :cap] if cap else want
                assert _bits_equal(want, stored_rows(p)), f"{name}: cap {cap} stride {stride} sampler {sampler}: plan {p} differs from the full rows: {_names(R, [p])}"
            if sampler == "auto":
                _assert_still_lanes(R, stored_rows, r2["traj_len"], f"{name} cap {cap} stride {stride}")


def _starts(R):
    """k per plan by plan index mod 5: 0, traj_len - 1, beyond the end, a sample inside, traj_len itself."""
    L = R["rec"]["traj_len"].astype(np.int64)
    p = np.arange(R["n"])
    inside = (sc.unit_random(sc.SEED + 4, p.astype(np.uint64), 0, 0) * L).astype(np.int64)
    return np.select([p % 5 == 0, p % 5 == 1, p % 5 == 2, p % 5 == 3], [0 * L, L - 1, L + 7, inside], L).astype(np.int32)


@pytest.mark.parametrize("name", ["panda7", "ref7"])
def test_readers_have_the_bits_of_the_full_rows(oracle_mod, name):
    """stateAt, replanStates, sampleWindow, sampleHorizon and sampleKnots with a per-plan start (0, traj_len - 1, beyond the end among
    them) read records with dir == 0, zero switch times and v_drive == +inf: the bits of the full rows by the existing rule."""
    import torch
    R = _rows(oracle_mod, name)
    ltp, batch, n, dof = R["ltp"], R["batch"], R["n"], R["dof"]
    lens = R["rec"]["traj_len"].astype(np.int64)
    kh = _starts(R)
    k = torch.from_numpy(kh).to(DEV)
    assert (kh == 0).sum() >= 100 and (kh == lens - 1).sum() >= 100 and (kh > lens).sum() >= 100
    N = 48
    for what, call, stride in (("sampleWindow", lambda: ltp.sampleWindow(batch, 0, n, k, N), 1),
                               ("sampleHorizon stride 3", lambda: ltp.sampleHorizon(batch, 0, n, k, N, 3), 3)):
        rows, valid = call()
        torch.cuda.synchronize()
        exp, exp_valid = _window_expected(R, kh, N, stride)
        got = rows.cpu().numpy()[..., :N]
        same = ((got.view(np.uint64) == exp.view(np.uint64)) | (np.isnan(got) & np.isnan(exp))).reshape(n, -1).all(axis=1)
        assert same.all(), f"{name}: {what}: {int((~same).sum())} plans differ from the full rows: {_names(R, ~same)}"
        assert np.array_equal(valid.cpu().numpy(), exp_valid), what
        assert np.isfinite(got).all()
        still = R["still"]
        q0 = np.broadcast_to(R["qs"][1][:, :, None], got[:, 0].shape)
        assert (got[:, 0][still].view(np.uint64) == np.ascontiguousarray(q0[still]).view(np.uint64)).all() and not got[:, 1:].transpose(0, 2, 1, 3)[still].view(np.uint64).any(), \
            f"{name}: {what}: a lane that stands still is not (q_0, +0, +0, +0)"
    for gname in ("duplicates", "mpc"):
        g = kc.GRIDS[gname]
        rows, valid = ltp.sampleKnots(batch, 0, n, k, torch.from_numpy(g).to(DEV))
        torch.cuda.synchronize()
        exp, exp_valid, planned = hc.expected(R["full"], batch.offsets, batch.traj_len, k, g, dof, 0, n)
        assert bool(planned.all())
        same = (hc.int_view(rows)[..., :len(g)] == exp).reshape(n, -1).all(dim=1).cpu().numpy()
        assert same.all(), f"{name}: sampleKnots {gname}: {int((~same).sum())} plans differ from the full rows: {_names(R, ~same)}"
        assert torch.equal(valid, exp_valid), gname
    # stateAt from the records, replanStates from the rows, and the rows themselves
    want = ltp.replanStates(batch, 0, n, R["full"], k)
    got = ltp.stateAt(batch, 0, n, k)
    got_jm = ltp.stateAt(batch, 3, n - 5, k[3:n - 2].contiguous(), layout="joint_major")
    torch.cuda.synchronize()
    for w, g, gj in zip(want, got, got_jm):
        bad = (w.view(torch.int64) != g.view(torch.int64)).any(dim=1).cpu().numpy()
        assert not bad.any(), f"{name}: stateAt differs from the sampled rows: {_names(R, bad)}"
        assert torch.equal(w[3:n - 2].t().contiguous().view(torch.int64), gj.view(torch.int64))
    q, v, a = (x.cpu().numpy() for x in got)
    for p in range(n):
        kk = min(int(kh[p]), int(lens[p]) - 1)
        assert _bits_equal(np.stack([q[p], v[p], a[p]]), _plan_rows(R, p)[:3, :, kk]), f"{name}: stateAt at {kh[p]}: {_names(R, [p])}"


def _assert_still_envelopes(R, env, what):
    """On a lane that stands still min == max == the bits of q_0, in every window."""
    q0 = np.ascontiguousarray(np.broadcast_to(R["qs"][1][:, :, None, None], env.shape)[R["still"]])
    bad = (env[R["still"]].view(np.uint64) != q0.view(np.uint64)).reshape(q0.shape[0], -1).any(axis=1)
    lanes = np.zeros_like(R["still"])
    lanes[R["still"]] = bad
    assert not bad.any(), f"{what}: the envelope of a lane that stands still is not [q_0, q_0]: {_names(R, lanes.any(axis=1))}"


@pytest.mark.parametrize("name", ["panda7", "ref7"])
def test_envelopes_by_class(oracle_mod, name):
    """ltp_envelope_batch in both modes against the fold of the full rows (exhaustive: bits; analytic: the acceptance rule of
    test_analytic_envelopes_agree_with_the_exhaustive_form) and ltp_envelope_knots_batch against envelope_checker."""
    import torch
    R = _rows(oracle_mod, name)
    ltp, batch, n, dof = R["ltp"], R["batch"], R["n"], R["dof"]
    lens = R["rec"]["traj_len"].astype(np.int64)
    try:
        for window, n_windows in ((64, 40), (1, 50), (700, 4)):
            red = np.empty((n, dof, n_windows, 2))
            for p in range(n):
                q = _plan_rows(R, p)[0]
                pad = np.concatenate([q, np.repeat(q[:, -1:], max(window * n_windows - int(lens[p]), 0) + window, axis=1)], axis=1)
                w = pad[:, : window * n_windows].reshape(dof, n_windows, window)
                red[p, :, :, 0], red[p, :, :, 1] = w.min(axis=2), w.max(axis=2)
            res = {}
            for mode in ("exhaustive", "analytic"):
                ltp.setEnvelopeMode(mode)
                env = ltp.envelopeBatch(batch, 0, n, window, n_windows)
                torch.cuda.synchronize()
                res[mode] = env.cpu().numpy()
                assert np.array_equal(_host(batch)["status"], R["rec"]["status"]), mode
                _assert_still_envelopes(R, res[mode], f"{name}: {mode} envelopes, window {window} x {n_windows}")
            ex, an = res["exhaustive"], res["analytic"]
            what = f"{name}: window {window} x {n_windows}"
            bad = (ex.view(np.uint64) != red.view(np.uint64)).any(axis=(1, 2, 3))
            assert not bad.any(), f"{what}: exhaustive envelopes differ from the reduced rows: {_names(R, bad)}"
            assert np.isfinite(an).all(), what
            d = np.abs(ex - an)
            assert d.max() <= 1e-12, f"{what}: analytic envelopes differ by {d.max()}: {_names(R, (d > 1e-12).any(axis=(1, 2, 3)))}"
            out = (an[..., 0] < ex[..., 0]) | (an[..., 1] > ex[..., 1])
            assert not out.any(), f"{what}: an analytic envelope lies outside the samples: {_names(R, out.any(axis=(1, 2)))}"
    finally:
        ltp.setEnvelopeMode("analytic")
    kh = _starts(R)
    k = torch.from_numpy(kh).to(DEV)
    for gname in ("mpc", "duplicates"):
        g = ec.GRIDS[gname]
        for closed in (0, 1):
            env, valid = ltp.envelopeKnots(batch, 0, n, k, torch.from_numpy(g).to(DEV), closed=closed)
            torch.cuda.synchronize()
            red, exp_valid, planned = ec.expected_q(R["full"], batch.offsets, batch.traj_len, k, g, closed, dof, 0, n)
            bad, worst, share = ec.compare_analytic(env, red, planned)
            what = f"{name}: envelopeKnots {gname} closed {closed}"
            assert not bool(bad.any().item()), f"{what}: {int(bad.sum().item())} plans miss the acceptance rule (worst |d| {worst:.3e}): {_names(R, bad.cpu().numpy())}"
            assert torch.equal(valid, exp_valid), what
            # a lane that stands still: the last position held, whatever the start
            _assert_still_envelopes(R, env.cpu().numpy(), what)


@pytest.mark.parametrize("name", ["panda7", "ref7"])
def test_stop_horizons_by_class(oracle_mod, name):
    """stopKnots on the MPC grid against the composition Y (tests/horizon_helpers.py), both acceleration modes, per-plan starts (0,
    traj_len - 1, beyond the end among them), the whole batch and an odd sub-range. A rest or near lane stops where it stands:
    q_stop has the bits of q_0 at every knot, and t_stop is what tests/test_stop_census_cpu.py established for a joint at rest —
    a_max / j_max where that is at most the sample time (panda at 4 ms: 2 ms), +0.0 through the square-root branch otherwise (ref)."""
    import torch
    R = _rows(oracle_mod, name)
    ltp, batch, n, dof = R["ltp"], R["batch"], R["n"], R["dof"]
    kh = _starts(R)
    g = kc.GRIDS["mpc"]
    N = len(g)
    describe = lambda plans: _names(R, plans)
    H.assert_stop_knots(ltp, batch, kh, g, 0, n, f"{name}: stopKnots mpc", describe=describe)
    first, count = H.odd_range(n, dof)
    assert (count * dof) % 64 != 0
    H.assert_stop_knots(ltp, batch, kh, g, first, count, f"{name}: stopKnots mpc, plans [{first}, {first + count})", describe=describe)
    H.assert_stop_knots(ltp, batch, 0, g, 0, n, f"{name}: stopKnots mpc, k = 0", describe=describe)
    tj = np.asarray(R["lim"]["a_max"], dtype=np.float64) / np.asarray(R["lim"]["j_max"], dtype=np.float64)
    want_t = np.where(tj > sc.TS, 0.0, tj)
    assert (want_t > 0.0).all() if name == "panda7" else not want_t.any()
    still = R["still"]
    assert still.sum() >= 1000
    for clamp in (True, False):
        got, _ = ltp.stopKnots(batch, 0, n, torch.from_numpy(kh).to(DEV), H.grid_tensor(g), clamp_acceleration=clamp)
        torch.cuda.synchronize()
        got = got[..., :N].cpu().numpy()
        q0 = np.broadcast_to(R["qs"][1][:, :, None], got[:, 0].shape)
        tt = np.broadcast_to(want_t[None, :, None], got[:, 1].shape)
        bad = ((got[:, 0].view(np.uint64) != np.ascontiguousarray(q0).view(np.uint64)) | (got[:, 1].view(np.uint64) != np.ascontiguousarray(tt).view(np.uint64))).any(axis=2) & still
        assert not bad.any(), (f"{name} clamp={clamp}: a lane that stands still does not stop at q_0 in {want_t}: first {got[:, :, :, 0][bad.any(axis=1)][:1]}: "
                               f"{_names(R, bad.any(axis=1))}")


@pytest.mark.parametrize("name", ["panda7", "ref7"])
def test_run_tables_through_the_example_consumer(oracle_mod, name):
    """ltp_build_tables_batch + the user-side consumer of tests/cpp: the peak |v| per lane is the reduced rows', bit for bit, and 0
    at sample 0 for a lane that stands still."""
    import torch
    from longtermplanner_amd import _abi
    R = _rows(oracle_mod, name)
    ltp, batch, n, dof = R["ltp"], R["batch"], R["n"], R["dof"]
    _abi.lib()
    path = os.path.join(ROOT, "tests", "cpp", "libexample_consumer.so")
    assert os.path.exists(path), "tests/cpp/libexample_consumer.so is missing: run __graft_entry__.build()"
    lib = C.CDLL(path)
    lib.example_peak_velocity.restype = C.c_int
    lib.example_peak_velocity.argtypes = [C.c_void_p, C.c_longlong, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    tables = ltp.buildRunTables(batch, 0, n)
    lanes = n * dof
    thr = 0.35 * float(min(R["lim"]["v_max"]))
    mx = torch.full((lanes,), -7.0, dtype=torch.float64, device=DEV)
    at = torch.full((lanes,), -7, dtype=torch.int32, device=DEV)
    above = torch.full((lanes,), -7, dtype=torch.int64, device=DEV)
    assert lib.example_peak_velocity(tables.data_ptr(), lanes, sc.TS, thr, mx.data_ptr(), at.data_ptr(), above.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_host(batch)["status"], R["rec"]["status"])
    mx, at, above = mx.cpu().numpy().reshape(n, dof), at.cpu().numpy().reshape(n, dof), above.cpu().numpy().reshape(n, dof)
    for p in range(n):
        av = np.abs(_plan_rows(R, p)[1])
        ok = _bits_equal(mx[p], av.max(axis=1)) and np.array_equal(at[p], av.argmax(axis=1)) and np.array_equal(above[p], (av > thr).sum(axis=1))
        assert ok, f"{name}: the consumer's peak velocity of plan {p} differs from the reduced rows: {mx[p]} {at[p]} {above[p]}: {_names(R, [p])}"
    assert not mx[R["still"]].view(np.uint64).any() and not at[R["still"]].any() and not above[R["still"]].any()


# ---- retime --------------------------------------------------------------------------------------------------------------------------
UNIFORM = 0.3                       # seconds: a few tenths, above the 0 of a standing query and below most moving queries' optimum
GROUP = 20                          # consecutive queries per group: the runs are 13 long, so groups mix standing and moving queries


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
@pytest.mark.parametrize("name", ["panda7", "ref7"])
def test_retime_by_class(oracle_mod, name, pow_rule):
    """ltp_retime_batch against retime_checker: 1.5 x T* (a query with T* == 0 is left alone), a uniform target (standing queries are
    retimed: every joint with dir == 0 and an all-zero optimum is scaled to T > 0) and groups that mix standing and moving queries.
    Untouched queries keep their bits; the rows of retimed plans keep the lanes that stand still at q_0."""
    import torch
    from longtermplanner_amd import LongTermPlanner, unpack_trajectory
    S = _batch(oracle_mod, name, pow_rule)
    n, dof, qs, orc, orec = S["n"], S["dof"], S["qs"], S["orc"], S["rec"]
    orec = dict(orec, status=np.where(orec["status"] == 2, 1, orec["status"]))        # before sampling: the checker's eligibility
    exact = pow_rule == "exact" or LongTermPlanner.powRuleMatchingHostLibm()[0] == "libm"
    ltp = _planner(dof, S["lim"], pow_rule=pow_rule)
    tens = _tensors(qs)
    group = (np.arange(n) // GROUP).astype(np.int32)
    n_groups = int(group[-1]) + 1
    standing = np.isin(S["kind"], (REST, NEAR)).all(axis=1)
    for kind in ("1.5 T*", "uniform", "groups"):
        batch = ltp.planSwitchTimesBatch(*tens)
        plain = _host(batch)
        elig = rc.device_eligible(plain)
        assert elig.all() and np.array_equal(rc.oracle_eligible(orec), elig)
        ts = rc.t_star(plain)
        if kind == "1.5 T*":
            T = 1.5 * ts
            ltp.retimeBatch(batch, t_target=torch.from_numpy(np.ascontiguousarray(T)).to(DEV))
        elif kind == "uniform":
            T = rc.targets(plain, elig, UNIFORM)[0]
            ltp.retimeBatch(batch, uniform=UNIFORM)
        else:
            T, gt_host = rc.targets(plain, elig, 0.0, None, group, n_groups)
            gt = ltp.retimeBatch(batch, group=torch.from_numpy(group).to(DEV), n_groups=n_groups)
            assert _bits_equal(gt.cpu().numpy(), gt_host)
            mixes = np.array([standing[group == g].any() and not standing[group == g].all() for g in range(n_groups)])
            assert mixes.sum() >= sc.FLOOR, "groups that hold standing and moving queries"
        dev = _host(batch)
        chk, retimed, cases = rc.retime(orc, orec, *qs, T)
        what = f"{name} {pow_rule} retime {kind}"
        print(f"{what}: retimed {int(retimed.sum())} of {n}, {int((retimed & standing).sum())} of them standing; cases {cases.sum(axis=0).tolist()}")
        with np.errstate(invalid="ignore"):
            assert np.array_equal(retimed, elig & (T > ts)), what
        if sc.has_twins(S["set"]):
            assert (retimed & standing).sum() >= (0 if kind == "1.5 T*" else sc.FLOOR), what
            assert kind != "1.5 T*" or not (retimed & standing).any(), "T* == 0 is left alone by a factor"
        assert retimed.sum() >= (10 * sc.FLOOR if kind == "uniform" else n // 4), what
        assert np.isfinite(chk["t_scaled"]).all() and not np.isnan(chk["v_drive"]).any(), what
        assert _agree(dev["t_required"][retimed], T[retimed], True).all(), what
        # by class: every class of the batch that holds a retimed query; a retime scales ALL joints
        held = [cls for cls, m in sc.classes(S) if cls in set(sc.present(S)) and (m & retimed[:, None]).any()]
        _assert_classes(dev, chk, S, exact, retimed, what, keys=("t_scaled", "v_drive", "mod", "traj_len"), present=held)
        # (a factor leaves the standing queries of ref alone; a uniform 0.3 s reaches the standing queries and those that only brake)
        missing = sorted(set(sc.present(S)) - set(held))
        assert "all_rest" in held if kind == "uniform" else len(missing) <= (3 if kind == "1.5 T*" else 0), (what, missing)
        keep = ~retimed
        for key in REC_KEYS:
            same = _agree(dev[key], plain[key], True).reshape(n, -1).all(axis=1)
            assert same[keep].all(), f"{what}: {key} of a query that was not retimed changed: {sc.describe(S, keep & ~same)}"
        assert np.all((dev["status"][retimed] & ~16) == 0)
        if kind == "1.5 T*":
            continue
        # rows of the first retimed plans (every shape is among the first 8 runs): the checker's within 1e-9, still lanes at q_0
        hi = 400
        off = dev["offsets"]
        tile = torch.zeros(int(off[hi] - off[0]) + 32, dtype=torch.float64, device=DEV)
        ltp.sampleBatchEx(batch, 0, hi, tile)
        torch.cuda.synchronize()
        rows = tile.cpu().numpy()
        lens = _host(batch)["traj_len"]
        seen = 0
        for p in np.nonzero(retimed[:hi])[0][:100]:
            L, q, v, a, j = rc.trajectory(orc, chk, p, qs[1], qs[2], qs[3])
            assert L == lens[p], f"{what}: plan {p}: {sc.describe(S, np.arange(n) == p)}"
            got = np.stack(unpack_trajectory(rows, int(off[p] - off[0]), dof, L))
            d = float(np.max(np.abs(got - np.stack([q, v, a, j]))))
            assert d <= TOL, f"{what}: rows of plan {p} differ from the checker's by {d}: {sc.describe(S, np.arange(n) == p)}"
            for jj in np.nonzero(np.isin(S["kind"][p], (REST, NEAR)))[0]:
                seen += 1
                ok = (got[0, jj].view(np.uint64) == qs[1][p, jj:jj + 1].view(np.uint64)).all() and not got[1:, jj].view(np.uint64).any()
                assert ok, f"{what}: plan {p} joint {jj} stands still but its retimed rows are not (q_0, +0, +0, +0): {sc.describe(S, np.arange(n) == p)}"
        assert seen >= 100, seen
