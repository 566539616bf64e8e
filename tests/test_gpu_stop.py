"""Stop plans (ltp_plan_stop_batch, include/ltp_hip.h) on the GPU: every joint brakes to rest by optBraking, one batched call.
Records, q_stop and offsets against tests/stop_checker.py (pinned to an independent oracle path by tests/test_stop_cpu.py), rows and
every reader of a planned batch on a stop batch, the wrappers, limit sets, the refusals, graph replay, the host and C++ paths.
Batches of at most 1000 states: n = 1, 65, 1000 (no multiple of 64), dof 1, 7, 30 (more joints than joint slots), both layouts."""
import ctypes as C
import os

import numpy as np
import pytest

import envelope_checker as ec
import horizon_helpers as H
import stop_checker as sc
from gpu_helpers import DEV, REC_KEYS, _agree, _bits_equal, _host, _planner, _tensors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_LIMIT_SET = 512


def _stop(S, idx, check, layout="query_major", pow_rule="libm", ltp=None, **kw):
    """planStopBatch of the states S[idx]: (planner, batch, host records, host q_stop [n][dof])."""
    import torch
    ltp = ltp or _planner(S["dof"], S["lim"], S["ts"], pow_rule=pow_rule)
    ins = _tensors([S["q0"][idx], S["v0"][idx], S["a0"][idx]], layout)
    batch = ltp.planStopBatch(*ins, layout=layout, check=check, **kw)
    torch.cuda.synchronize()
    qs = batch.q_stop.cpu().numpy()
    return ltp, batch, _host(batch), np.ascontiguousarray(qs if layout == "query_major" else qs.T)


def _assert_records(rec, qs, E, idx, what):
    for k in REC_KEYS:
        same = _agree(rec[k], E[k][idx], True)
        assert np.all(same), f"{what}: {k} differs in {int(np.count_nonzero(~same))} places, first {np.argwhere(~same)[0]}"
    same = _agree(qs, E["q_stop"][idx], True)
    assert np.all(same), f"{what}: q_stop differs in {int(np.count_nonzero(~same))} places, first {np.argwhere(~same)[0]}"


@pytest.mark.parametrize("name,n,layout,check,pow_rule", [
    ("panda", 1000, "query_major", "braking", "libm"), ("panda", 1000, "joint_major", "inputs", "exact"),
    ("panda", 65, "joint_major", "braking", "exact"), ("panda", 1, "query_major", "inputs", "libm"),
    ("ref1", 65, "query_major", "inputs", "libm"), ("ref1", 1, "joint_major", "braking", "exact"),
    ("ref30", 130, "joint_major", "inputs", "libm"), ("ref30", 65, "query_major", "braking", "exact")])
def test_records_q_stop_and_offsets(request, oracle_mod, name, n, layout, check, pow_rule):
    """Records and q_stop bit for bit: under LTP_POW_LIBM against the checker, under LTP_POW_EXACT against the oracle's exact-pow
    twin; the offsets are the scan of the padded row sizes, also under max_samples = 40 and sample_stride = 3."""
    if pow_rule == "libm":
        request.getfixturevalue("restated_host_libm")
    S = sc.states(oracle_mod, name)
    E = sc.expected(oracle_mod, name, check, exact_pow=(pow_rule == "exact"))
    # the smaller batches take every k-th state, so that hand-made, mid-trajectory and generated states all occur
    total = len(S["q0"])
    idx = np.arange(total) if n == total else (np.arange(n) * (total // n)) if n > 1 else np.array([total - 1])
    ltp, batch, rec, qs = _stop(S, idx, check, layout, pow_rule)
    what = f"{name} n={n} {layout} {check} {pow_rule}"
    _assert_records(rec, qs, E, idx, what)
    stride_of = ltp._lib.ltp_row_stride
    assert np.array_equal(rec["offsets"], sc.offsets_of(rec["traj_len"], S["dof"], stride_of)), what
    print(what, "status bits:", np.unique(rec["status"]), "plans with rows:", int(np.count_nonzero(rec["traj_len"])))
    if n > 1:
        assert np.count_nonzero(rec["traj_len"]) > 0.5 * n
    if n == 1000:
        ltp.setMaxSamples(40)
        ltp.setSampleStride(3)
        _, _, rec2, _ = _stop(S, idx, check, layout, pow_rule, ltp=ltp)
        assert np.array_equal(rec2["traj_len"], rec["traj_len"])
        off = sc.offsets_of(rec["traj_len"], S["dof"], stride_of, max_samples=40, stride=3)
        assert np.array_equal(rec2["offsets"], off) and off[-1] < rec["offsets"][-1]


def _invalid_states(oracle_mod):
    """Panda states that fail checkInputs each for ONE reason — |a| > a_max (40), q outside (20), |v| > v_max (20), the third rule
    alone (20) — among 28 that pass: dict like stop_checker.states, plus `why` [n] (0 = passes, 1..4)."""
    S = sc.states(oracle_mod, "panda")
    from longtermplanner_amd.synthetic import generate_queries
    _, q0, v0, a0 = generate_queries(128, S["lim"], seed=909)
    lim = {k: np.asarray(v) for k, v in S["lim"].items()}
    why = np.zeros(128, dtype=np.int32)
    rng = np.random.default_rng(3)
    for p in range(100):
        j = int(rng.integers(0, 7))
        if p < 40:
            a0[p, j] = np.copysign(lim["a_max"][j] * (1.0 + 0.2 * rng.uniform()), v0[p, j] if v0[p, j] != 0 else 1.0)
            why[p] = 1
        elif p < 60:
            q0[p, j] = lim["q_max"][j] + 0.25
            why[p] = 2
        elif p < 80:
            v0[p, j] = -(lim["v_max"][j] + 0.1)
            a0[p, j] = 0.0
            why[p] = 3
        else:
            v0[p, j] = lim["v_max"][j] * (1.0 - 1e-6)
            a0[p, j] = 0.5 * lim["a_max"][j]
            why[p] = 4
    return dict(S, q0=q0, v0=v0, a0=a0, why=why)


def test_rejected_states_hold_what_planning_towards_the_standstill_leaves(oracle_mod):
    """A state that fails checkInputs: LTP_STATUS_INVALID_INPUT, q_stop NaN, and every record field has the bits
    ltp_plan_switch_times_batch leaves for the same state planned towards optBraking's standstill position (the goal in whose place
    a stop plan stands). LTP_STOP_CHECK_BRAKING admits the states that fail only on q, v or the third rule and rejects |a| > a_max."""
    import torch
    S = _invalid_states(oracle_mod)
    n, why = len(S["q0"]), S["why"]
    idx = np.arange(n)
    E = sc.expected_stop(S["orc"], S["q0"], S["v0"], S["a0"], "inputs", rows=False)
    assert np.array_equal(E["accepted"], why == 0) and np.all(np.isfinite(E["q_closed"]))
    for pow_rule in ("libm", "exact"):
        ltp, batch, rec, qs = _stop(S, idx, "inputs", pow_rule=pow_rule)
        rej = why != 0
        assert np.all(rec["status"][rej] == sc.INVALID_INPUT) and np.all(rec["status"][~rej] == 0)
        assert np.all(np.isnan(qs[rej])) and np.all(np.isfinite(qs[~rej])) and np.all(rec["traj_len"][rej] == 0)
        goal = torch.from_numpy(E["q_closed"]).to(DEV)
        plain = _host(ltp.planSwitchTimesBatch(goal, *_tensors([S["q0"], S["v0"], S["a0"]])))
        for k in REC_KEYS:
            same = _agree(rec[k][rej], plain[k][rej], True)
            assert np.all(same), f"{pow_rule}: {k} of a rejected state differs from ltp_plan_switch_times_batch's, first {np.argwhere(~same)[0]}"
        # mode 1
        _, _, rec1, qs1 = _stop(S, idx, "braking", pow_rule=pow_rule, ltp=ltp)
        assert np.all(rec1["status"][why == 1] == sc.INVALID_INPUT) and np.all(np.isnan(qs1[why == 1]))
        assert np.all(rec1["status"][why != 1] == 0) and np.all(rec1["traj_len"][why != 1] > 0) and np.all(np.isfinite(qs1[why != 1]))
    E1 = sc.expected_stop(S["orc"], S["q0"], S["v0"], S["a0"], "braking", rows=False)
    assert np.array_equal(E1["status"], rec1["status"]) and np.array_equal(E1["traj_len"], rec1["traj_len"])


def test_nan_states_end_as_nonfinite(oracle_mod):
    S = sc.states(oracle_mod, "panda")
    q0, v0, a0 = (S[k][200:265].copy() for k in ("q0", "v0", "a0"))
    v0[3, 2] = np.nan
    a0[40, :] = np.nan
    q0[50, 0] = np.nan                    # a NaN position does not reach the times: planned, q_stop NaN in that joint
    T = dict(S, q0=q0, v0=v0, a0=a0)
    for check in ("inputs", "braking"):
        E = sc.expected_stop(S["orc"], q0, v0, a0, check, rows=False)
        _, _, rec, qs = _stop(T, np.arange(65), check, pow_rule="exact")
        assert rec["status"][3] == sc.NONFINITE and rec["traj_len"][3] == 0
        assert rec["status"][40] == sc.NONFINITE | sc.NO_SLOWEST and rec["traj_len"][40] == 0 and rec["slowest"][40] == -1
        assert rec["status"][50] == E["status"][50] and np.isnan(qs[50, 0]) and np.all(np.isfinite(qs[50, 1:]))
        assert np.array_equal(rec["status"], E["status"]) and np.array_equal(rec["traj_len"], E["traj_len"])
        off = rec["offsets"]
        assert off[4] == off[3] and off[41] == off[40]


_ROWS = {}


def _row_batch(oracle_mod):
    """Every 8th state of the panda batch (125 plans) as a stop batch with its full rows from the fused sampler."""
    import torch
    if not _ROWS:
        S = sc.states(oracle_mod, "panda")
        idx = np.arange(0, 1000, 8)
        ltp, batch, rec, qs = _stop(S, idx, "braking")
        full = torch.zeros(int(rec["offsets"][-1]) + 32, dtype=torch.float64, device=DEV)
        ltp.sampleBatchEx(batch, 0, len(idx), full, sampler="fused")
        torch.cuda.synchronize()
        _ROWS.update(S=S, idx=idx, ltp=ltp, batch=batch, rec=_host(batch), full=full, n=len(idx))
    return _ROWS


def test_rows_against_the_checker_and_between_the_samplers(oracle_mod):
    """Rows of a stop batch against getTrajectory on the checker's records by the dense-row rule (1e-9, j bit-identical); the
    fused, walk and table samplers write the same bits."""
    import torch
    from longtermplanner_amd import unpack_trajectory
    R = _row_batch(oracle_mod)
    E = sc.expected(oracle_mod, "panda", "braking", rows=True)
    ltp, batch, n, rec = R["ltp"], R["batch"], R["n"], R["rec"]
    host = R["full"].cpu().numpy()
    assert np.array_equal(rec["status"], E["status_end"][R["idx"]])       # the sampler formed the end-limit verdict
    worst = 0.0
    for i, p in enumerate(R["idx"]):
        L = int(rec["traj_len"][i])
        assert L == E["traj_len"][p]
        if L == 0:
            continue
        got = np.stack(unpack_trajectory(host, int(rec["offsets"][i]), 7, L))
        exp = E["rows"][p]
        worst = max(worst, float(np.max(np.abs(got[:3] - exp[:3]))))
        assert np.all(_agree(got[:3], exp[:3], False)) and np.all(_agree(got[3], exp[3], True)), (i, p)
    print("rows: worst |d| of q, v, a", worst)
    assert np.count_nonzero(rec["traj_len"]) >= 100
    for sampler in ("walk", "table"):
        other = torch.zeros_like(R["full"])
        ltp.sampleBatchEx(batch, 0, n, other, sampler=sampler)
        torch.cuda.synchronize()
        assert _bits_equal(other.cpu().numpy(), host), sampler


def test_readers_take_a_stop_batch(oracle_mod):
    """sampleWindow, sampleKnots, envelopeKnots, envelopeBatch and stateAt on a stop batch against its full rows, each under its
    reader's own rule (bit for bit; the analytic envelope rule for the two envelope calls)."""
    import torch
    R = _row_batch(oracle_mod)
    ltp, batch, n, full = R["ltp"], R["batch"], R["n"], R["full"]
    lens = R["rec"]["traj_len"]
    rng = np.random.default_rng(5)
    k = rng.integers(-5, lens.astype(np.int64) + 41).astype(np.int32)
    first, count = 3, n - 8
    N = 24
    H.assert_rows(lambda kk, out: ltp.sampleWindow(batch, first, count, kk, N, out=out), ltp, batch, full, k, np.arange(N), first, count, "window")
    g = np.array([0, 1, 2, 3, 5, 8, 8, 13, 21, 34, 55, 89, 144, 233, 377], dtype=np.int32)
    H.assert_rows(lambda kk, out: ltp.sampleKnots(batch, first, count, kk, H.grid_tensor(g), out=out), ltp, batch, full, k, g, first, count, "knots")
    kt = torch.from_numpy(np.ascontiguousarray(k[first:first + count])).to(DEV)
    for closed in (0, 1):
        env, valid = ltp.envelopeKnots(batch, first, count, kt, H.grid_tensor(g), closed=bool(closed))
        torch.cuda.synchronize()
        red, exp_valid, planned = ec.expected_q(full, batch.offsets, batch.traj_len, kt, g, closed, 7, first, count)
        bad, worst, share = ec.compare_analytic(env, red, planned)
        assert not bool(bad.any().item()) and torch.equal(valid, exp_valid), (closed, worst, share)
    window, n_windows = 32, 12
    env = ltp.envelopeBatch(batch, first, count, window, n_windows)
    torch.cuda.synchronize()
    zero = torch.zeros(count, dtype=torch.int32, device=DEV)
    red, _, planned = ec.expected_q(full, batch.offsets, batch.traj_len, zero, window * np.arange(n_windows + 1), 0, 7, first, count)
    bad, worst, share = ec.compare_analytic(env, red, planned)
    assert not bool(bad.any().item()), (worst, share)
    q, v, a = (x.cpu().numpy() for x in ltp.stateAt(batch, first, count, kt))
    win, _ = ltp.sampleWindow(batch, first, count, kt, 1)
    torch.cuda.synchronize()
    win = win.cpu().numpy()
    has = lens[first:first + count] > 0
    inside = has & (k[first:first + count] < lens[first:first + count])
    assert np.count_nonzero(inside) >= 20 and np.count_nonzero(has & ~inside) >= 5
    for arr, got in enumerate((q, v, a)):
        assert np.all(_agree(got[inside], win[inside, arr, :, 0], True)), arr
    assert np.all(_agree(q[has], win[has, 0, :, 0], True))     # past the end both hold the last position


def test_end_limit_verdict(oracle_mod):
    """States near q_max moving outwards stop beyond the range: LTP_STATUS_END_LIMIT exactly where the checker's last sample lies outside."""
    S = sc.states(oracle_mod, "panda")
    q0, v0, a0 = (S[k][600:664].copy() for k in ("q0", "v0", "a0"))      # generated start states: all pass checkInputs
    lim ={k: np.asarray(v) for k, v in S["lim"].items()}
    for p in range(24):
        j = p % 7
        q0[p, j] = lim["q_max"][j] - 0.005
        v0[p, j] = (0.3 if p % 2 == 0 else -0.3) * lim["v_max"][j]      # outwards / inwards
        a0[p, j] = 0.0
    E = sc.expected_stop(S["orc"], q0, v0, a0, "inputs")
    ltp, batch, rec, qs = _stop(dict(S, q0=q0, v0=v0, a0=a0), np.arange(64), "inputs", pow_rule="exact", end_limit=True)
    assert np.array_equal(rec["status"], E["status_end"])
    assert np.all(rec["status"][:24:2] & sc.END_LIMIT) and np.count_nonzero(rec["status"] == 0) >= 5
    beyond = np.any(qs > lim["q_max"][None, :], axis=1)
    assert np.all(beyond[:24:2])                                 # the closed-form standstill lies outside there too


def test_plan_stop_from(oracle_mod):
    """planStopFrom = stateAt, the clamp of a_0 to +-a_max, planStopBatch: the checker applied to stateAt's output after the clamp,
    bit for bit; without the clamp and with check="inputs" the rejected set is the oracle's checkInputs on those states."""
    import torch
    n = 512
    ltp, dof, lim = H.planner("panda", "exact")
    batch = ltp.planSwitchTimesBatch(*H.tensors(H.queries(lim, n)))
    torch.cuda.synchronize()
    lens = batch.traj_len.cpu().numpy()
    k = np.random.default_rng(8).integers(0, np.maximum(lens, 1)).astype(np.int32)
    kt = torch.from_numpy(k).to(DEV)
    orc = oracle_mod.Oracle(dof, H.TS, exact_pow=True, **lim)
    q, v, a = (x.cpu().numpy() for x in ltp.stateAt(batch, 0, n, kt))
    over = np.abs(a) > orc.a_max[None, :]
    print("states with |a| > a_max:", int(np.count_nonzero(np.any(over, axis=1))), "of", n)
    ac = np.clip(a, -orc.a_max, orc.a_max)
    stop = ltp.planStopFrom(batch, 0, n, kt)
    torch.cuda.synchronize()
    assert stop is not batch and stop.inputs[0] is stop.q_stop
    assert _bits_equal(stop.inputs[3].cpu().numpy(), ac) and _bits_equal(stop.inputs[1].cpu().numpy(), q)
    E = sc.expected_stop(orc, q, v, ac, "braking", rows=False)
    _assert_records(_host(stop), stop.q_stop.cpu().numpy(), E, np.arange(n), "planStopFrom")
    assert np.all(E["status"] == 0)
    raw = ltp.planStopFrom(batch, 0, n, kt, clamp_acceleration=False, check="inputs")
    torch.cuda.synchronize()
    ok = sc.accepted(orc, q, v, a, "inputs")
    st = raw.status.cpu().numpy()
    assert np.array_equal(st == 0, ok) and np.all(st[~ok] == sc.INVALID_INPUT)
    # a sub-range in the other layout starts from the same states
    sub = ltp.planStopFrom(batch, 100, 65, kt[100:165].contiguous(), layout="joint_major")
    torch.cuda.synchronize()
    assert _bits_equal(sub.q_stop.cpu().numpy().T, stop.q_stop.cpu().numpy()[100:165])


def _two_sets(lim):
    return [dict(lim, v_max=[f * x for x in lim["v_max"]], a_max=[f * x for x in lim["a_max"]], j_max=[f * x for x in lim["j_max"]])
            for f in (1.0, 0.5)]


def test_limit_sets(oracle_mod):
    """Two limit sets: each state gets what a handle with its set gives, bit for bit; a bad index gives LTP_STATUS_BAD_LIMIT_SET."""
    import torch
    n = 200
    ltp, dof, lim = H.planner("panda")
    sets = _two_sets(lim)
    ltp.setLimitSets(*[np.array([s[key] for s in sets], dtype=np.float64) for key in ("q_min", "q_max", "v_max", "a_max", "j_max")])
    _, q0, v0, a0 = H.queries(sets[1], n)             # drawn for the slower set: they pass checkInputs under both
    a0[7, 2] = 0.8 * lim["a_max"][2]                  # beyond the slower set's a_max only
    ix = (np.arange(n) % 2).astype(np.int32)
    ix[5], ix[6] = 7, -1
    S = dict(dof=dof, lim=lim, ts=H.TS, q0=q0, v0=v0, a0=a0)
    idx = np.arange(n)
    _, batch, rec, qs = _stop(S, idx, "inputs", ltp=ltp, limit_set=torch.from_numpy(ix).to(DEV))
    bad = (ix < 0) | (ix > 1)
    assert np.all(rec["status"][bad] == BAD_LIMIT_SET) and np.all(rec["traj_len"][bad] == 0) and np.all(rec["slowest"][bad] == -1)
    assert np.all(np.isnan(qs[bad]))
    assert rec["status"][7] == sc.INVALID_INPUT and rec["status"][8] == 0
    for s in (0, 1):
        _, _, one, qs_one = _stop(dict(S, lim=sets[s]), idx, "inputs")
        mine = (ix == s)
        for key in REC_KEYS:
            assert np.all(_agree(rec[key][mine], one[key][mine], True)), (s, key)
        assert np.all(_agree(qs[mine], qs_one[mine], True)), s
    off = rec["offsets"]
    assert np.array_equal(off, sc.offsets_of(rec["traj_len"], dof, ltp._lib.ltp_row_stride))
    # the shield's clamp reads each state's own set
    plan = ltp.planSwitchTimesBatch(*H.tensors(H.queries(sets[1], n)), limit_set=torch.from_numpy((np.arange(n) % 2).astype(np.int32)).to(DEV))
    stop = ltp.planStopFrom(plan, 10, 100, 40)
    torch.cuda.synchronize()
    am = np.array([sets[(10 + i) % 2]["a_max"] for i in range(100)])
    assert np.all(np.abs(stop.inputs[3].cpu().numpy()) <= am) and np.all(stop.status.cpu().numpy() == 0)


def test_refusals(oracle_mod):
    """LTP_SEMANTICS_MATLAB is refused; retimeBatch on a stop batch is refused until the handle plans with planSwitchTimesBatch
    again; a sample time changed between the stop plan and a reader is refused; null state arrays and incomplete records are refused."""
    import torch
    from longtermplanner_amd import LtpError, _abi
    S = sc.states(oracle_mod, "panda")
    idx = np.arange(65)
    ltp, batch, rec, _ = _stop(S, idx, "inputs")
    with pytest.raises(LtpError, match="stop plan"):
        ltp.retimeBatch(batch, uniform=2.0)
    with pytest.raises(LtpError, match="changed since the batch was planned"):
        ltp.setSampleTime(0.002)
        try:
            ltp.stateAt(batch, 0, 65, 3)
        finally:
            ltp.setSampleTime(S["ts"])
    ltp.stateAt(batch, 0, 65, 3)
    qs = H.tensors(H.queries(S["lim"], 65))
    plain = ltp.planSwitchTimesBatch(*qs)
    ltp.retimeBatch(plain, uniform=2.0)               # accepted again
    torch.cuda.synchronize()
    assert np.all(plain.t_required.cpu().numpy()[plain.status.cpu().numpy() == 0] >= 2.0)
    ltp.setSemantics("matlab")
    with pytest.raises(LtpError, match="MATLAB"):
        ltp.planStopBatch(*qs[1:])
    ltp.setSemantics("cpp")
    o = _abi.StopOpts(C.sizeof(_abi.StopOpts), 0, None)
    r = batch.c_records()
    q = _abi.Queries(None, qs[1].data_ptr(), qs[2].data_ptr(), None, 7, 1)
    assert ltp._lib.ltp_plan_stop_batch(ltp._h, 65, C.byref(q), C.byref(r), C.addressof(o), None, None) == H.INVALID
    q = _abi.Queries(None, qs[1].data_ptr(), qs[2].data_ptr(), qs[3].data_ptr(), 7, 1)
    r.t_scaled = None
    assert ltp._lib.ltp_plan_stop_batch(ltp._h, 65, C.byref(q), C.byref(r), C.addressof(o), None, None) == H.INVALID
    o.check = 2
    r = batch.c_records()
    assert ltp._lib.ltp_plan_stop_batch(ltp._h, 65, C.byref(q), C.byref(r), C.addressof(o), None, None) == H.INVALID
    o.check = 1                                       # a null q_goal, a null q_stop and null offsets are all admitted
    assert ltp._lib.ltp_plan_stop_batch(ltp._h, 65, C.byref(q), C.byref(r), C.addressof(o), None, ltp._stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(batch.status.cpu().numpy(), sc.expected_stop(S["orc"], *[x.cpu().numpy() for x in qs[1:]], "braking", rows=False)["status"])


def test_graph_capture_and_replay_on_rewritten_states(oracle_mod):
    """After ltp_reserve_batch the call enqueues only memset and kernel nodes: captured, then replayed after the states were
    rewritten in place, it gives what a fresh call gives."""
    import torch
    S = sc.states(oracle_mod, "panda")
    n = 1000
    ltp = _planner(7, S["lim"], S["ts"], pow_rule="exact")
    ltp._check(ltp._lib.ltp_reserve_batch(ltp._h, n))
    perm = np.random.default_rng(4).permutation(n)
    ins = _tensors([S["q0"], S["v0"], S["a0"]])
    batch = ltp.planStopBatch(*ins, check="braking")
    graph = H.capture(lambda: ltp.planStopBatch(*ins, batch=batch, check="braking"))
    H.replay(graph, [(t, np.ascontiguousarray(S[k][perm])) for t, k in zip(ins, ("q0", "v0", "a0"))], batch.t_scaled, batch.traj_len)
    got, got_qs = _host(batch), batch.q_stop.cpu().numpy()
    _, _, fresh, fresh_qs = _stop(S, perm, "braking", pow_rule="exact")
    for k in REC_KEYS + ("offsets",):
        assert np.all(_agree(got[k], fresh[k], True)), k
    assert np.all(_agree(got_qs, fresh_qs, True)) and np.count_nonzero(fresh["traj_len"]) > 900


def test_host_and_dropin_paths(oracle_mod, tmp_path):
    """planStopHost equals the device path (records, q_stop, offsets, rows; status with the end-limit verdict), and
    tests/cpp/stop_dropin_test.cc — LongTermPlanner::planStopBatch against two hand-computed lanes — passes."""
    import torch
    S = sc.states(oracle_mod, "panda")
    idx = np.arange(0, 1000, 25)
    for check in ("inputs", "braking"):
        ltp, batch, _, qs = _stop(S, idx, check)
        full = H.full_rows(ltp, batch)
        rec = _host(batch)
        r = ltp.planStopHost(S["q0"][idx], S["v0"][idx], S["a0"][idx], check=check)
        for k in REC_KEYS + ("offsets",):
            assert np.all(_agree(r[k], rec[k], True)), (check, k)
        assert np.all(_agree(r["q_stop"], qs, True))
        total = int(rec["offsets"][-1])
        assert _bits_equal(r["packed"], full.cpu().numpy()[:total])
        r2 = ltp.planStopHost(S["q0"][idx], S["v0"][idx], S["a0"][idx], sample=False, check=check)
        assert np.array_equal(r2["status"], rec["status"]) and "packed" not in r2
    src = open(os.path.join(ROOT, "tests", "cpp", "stop_dropin_test.cc")).read()
    raw = np.frombuffer(H.run_dropin(tmp_path, "stop_dropin_test", src, b""), dtype=np.float64)
    assert list(raw[[0, 2, 3]]) == [0.5, 0.5, 65.0] and abs(raw[1] + 0.8125) <= 1e-12
    one = _planner(2, dict(q_min=[-3.0] * 2, q_max=[3.0] * 2, v_max=[1.0] * 2, a_max=[2.0] * 2, j_max=[16.0] * 2), ts=0.0078125)
    h = one.planStopHost([[0.5, -1.0]], [[0.0, 0.75]], [[0.0, 0.0]], sample=False)
    assert _bits_equal(h["q_stop"][0], raw[:2]) and h["traj_len"][0] == 65
