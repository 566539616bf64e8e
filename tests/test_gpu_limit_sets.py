"""Limit sets on the GPU (ltp_set_limit_sets / ltp_bind_limit_sets, include/ltp_hip.h): a query that uses set s gets exactly what it
gets on a handle whose limits are set s — records, offsets, rows of every sampler, envelopes, run tables, restart states, the
end-limit verdict and retimes — plus bad indices, refusals, graph capture and the host path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TS = 0.001
REC_KEYS = ("t_opt", "t_scaled", "dir", "v_drive", "mod", "t_required", "slowest", "traj_len", "status")
LIM_KEYS = ("q_min", "q_max", "v_max", "a_max", "j_max")
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _set_list():
    """K = 5 sets of 7 joints: panda, the reference's S-ref, panda scaled to 0.25, a seeded wide fuzz, tight q ranges."""
    from longtermplanner_amd import limit_set
    _, panda = limit_set("panda")
    _, sref = limit_set("ref")
    slow = dict(panda, v_max=[0.25 * x for x in panda["v_max"]], a_max=[0.25 * x for x in panda["a_max"]],
                j_max=[0.25 * x for x in panda["j_max"]])
    rng = np.random.default_rng(7)
    lo = -rng.uniform(0.5, 4.0, 7)
    fuzz = dict(q_min=list(lo), q_max=list(lo + rng.uniform(0.5, 6.0, 7)), v_max=list(rng.uniform(0.2, 4.0, 7)),
                a_max=list(rng.uniform(0.5, 30.0, 7)), j_max=list(rng.uniform(5.0, 12000.0, 7)))
    tight = dict(panda, q_min=[x * 0.2 for x in panda["q_min"]], q_max=[x * 0.2 for x in panda["q_max"]])
    return [panda, sref, slow, fuzz, tight]


def _planner(lim, pow_rule="libm", max_samples=0, goal_check=False):
    from longtermplanner_amd import LongTermPlanner
    p = LongTermPlanner(7, TS, device=0, **lim)
    p.setPowRule(pow_rule)
    if max_samples:
        p.setMaxSamples(max_samples)
    if goal_check:
        p.setGoalCheck(True)
    return p


def _stack(sets):
    return [np.array([s[k] for s in sets], dtype=np.float64) for k in LIM_KEYS]


def _mixed(sets, n, seed=3):
    """Queries generated per set, query q taken from set gen[q]'s batch and assigned set idx[q]. 40 % of the queries of the scaled
    set (2) and of the tight set (4) are generated for panda: checkInputs then fails there for many of them."""
    from longtermplanner_amd import generate_queries
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(sets), n).astype(np.int32)
    gen = idx.copy()
    swap = ((idx == 2) | (idx == 4)) & (rng.random(n) < 0.4)   # and goals outside the tight ranges: goal-check verdicts
    gen[swap] = 0
    per = [generate_queries(n, s, seed=seed + 10 * k) for k, s in enumerate(sets)]
    qs = [np.ascontiguousarray(np.choose(gen[:, None], [p[f] for p in per])) for f in range(4)]
    return qs, idx


def _tensors(qs):
    import torch
    return [torch.from_numpy(x).to(DEV) for x in qs]


def _host(batch):
    import torch
    torch.cuda.synchronize()
    r = {k: getattr(batch, k).cpu().numpy().copy() for k in REC_KEYS}
    r["offsets"] = batch.offsets.cpu().numpy().view(np.uint64).copy()
    return r


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def _assert_records(a, b, mask, what):
    for k in REC_KEYS:
        bad = np.count_nonzero(np.any(_bits(a[k])[mask] != _bits(b[k])[mask], axis=1))
        assert bad == 0, f"{what}: {k} differs for {bad} queries"
    sa, sb = np.diff(a["offsets"].astype(np.int64)), np.diff(b["offsets"].astype(np.int64))
    assert np.array_equal(sa[mask], sb[mask]), f"{what}: per-plan sizes differ"


def _plan_mixed(sets, qs, idx, **kw):
    import torch
    p = _planner(sets[0], **kw)
    p.setLimitSets(*_stack(sets))
    ix = torch.from_numpy(idx).to(DEV)
    b = p.planSwitchTimesBatch(*_tensors(qs), limit_set=ix)
    return p, b


def _plan_each(sets, qs, **kw):
    out = []
    for s in sets:
        p = _planner(s, **kw)
        out.append((p, p.planSwitchTimesBatch(*_tensors(qs))))
    return out


def _gather(tile, offsets, plans):
    """The rows of `plans` (numpy indices) of a packed tile, concatenated (device)."""
    import torch
    off = torch.from_numpy(offsets.astype(np.int64)).to(tile.device)
    pl = torch.from_numpy(np.asarray(plans, dtype=np.int64)).to(tile.device)
    start, size = off[pl], off[pl + 1] - off[pl]
    total = int(size.sum().item())
    if total == 0:
        return tile[:0]
    base = torch.repeat_interleave(start - (torch.cumsum(size, 0) - size), size)
    return tile[base + torch.arange(total, device=tile.device)]


def _err(p):
    return (p._lib.ltp_last_error(p._h) or b"").decode()


def _lane_words(tables, lanes):
    """[lanes][114] words of (plan, joint) lanes of a run-table buffer (include/ltp_run_tables.hpp: table_word_index)."""
    W = tables.cpu().numpy()
    l = np.asarray(lanes, dtype=np.int64)[:, None]
    w = np.arange(114, dtype=np.int64)[None, :]
    return W[(l >> 6) * (114 * 64) + ((w >> 1) * 64 + (l & 63)) * 2 + (w & 1)]


def _same_bits(a, b):
    import torch
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and torch.equal(a.view(it), b.view(it))


@pytest.mark.parametrize("pow_rule", ["libm", "exact"])
@pytest.mark.parametrize("goal_check", [False, True])
def test_mixed_batch_matches_per_set_handles(pow_rule, goal_check):
    sets = _set_list()
    qs, idx = _mixed(sets, 100000)
    p, b = _plan_mixed(sets, qs, idx, pow_rule=pow_rule, goal_check=goal_check)
    p.endLimit(b, 0, b.n)
    mixed = _host(b)
    fired = {"invalid": 0, "end": 0, "goal": 0}
    for s, (ps, bs) in enumerate(_plan_each(sets, qs, pow_rule=pow_rule, goal_check=goal_check)):
        ps.endLimit(bs, 0, bs.n)
        ref = _host(bs)
        _assert_records(mixed, ref, idx == s, f"set {s}")
        st = ref["status"][idx == s]
        fired["invalid"] += int(np.count_nonzero(st & 1))
        fired["end"] += int(np.count_nonzero(st & 8))
        fired["goal"] += int(np.count_nonzero(st & 64))
    assert fired["invalid"] > 0 and fired["end"] > 0 and (fired["goal"] > 0) == goal_check, fired


def test_records_and_rows_match_the_cpu_oracle(oracle_mod, restated_host_libm):
    """The parity oracle (this host's libm is the one LTP_POW_LIBM restates), one per set: records bit for bit for every query the
    reference plans, dense rows within 1e-9 for a sample of them."""
    import torch
    from longtermplanner_amd.planner import unpack_trajectory
    sets = _set_list()
    n = 3000
    qs, idx = _mixed(sets, n, seed=21)
    p, b = _plan_mixed(sets, qs, idx)
    dev = _host(b)
    off = dev["offsets"]
    tile = torch.zeros(int(off[n]) + 32, dtype=torch.float64, device=DEV)
    p.sampleBatch(b, 0, n, tile)
    rows = tile.cpu().numpy()
    checked_rows = 0
    for s, lim in enumerate(sets):
        m = np.nonzero(idx == s)[0]
        orc = oracle_mod.Oracle(7, TS, **lim)
        orec = orc.plan_batch(*[x[m] for x in qs])
        assert np.array_equal(dev["traj_len"][m], np.asarray(orec["traj_len"])), s
        ok = np.asarray(orec["traj_len"]) > 0          # (the reference leaves the records of a failed query unformed)
        assert np.count_nonzero(ok) > 100
        for k in ("t_scaled", "v_drive", "t_required"):
            assert np.array_equal(dev[k][m][ok].view(np.uint64), np.asarray(orec[k])[ok].view(np.uint64)), (s, k)
        for k in ("mod", "slowest"):
            assert np.array_equal(dev[k][m][ok], np.asarray(orec[k])[ok]), (s, k)
        for i in np.nonzero(ok)[0][:40]:
            q = m[i]
            L, *ref = orc.get_trajectory(dev["t_scaled"][q], dev["dir"][q], dev["mod"][q], qs[1][q], qs[2][q], qs[3][q], dev["v_drive"][q])
            assert L == dev["traj_len"][q]
            got = unpack_trajectory(rows, int(off[q]), 7, L)
            for k in range(4):
                assert np.max(np.abs(got[k] - np.asarray(ref[k]).reshape(7, L))) < 1e-9, (s, q, k)
            checked_rows += 1
    assert checked_rows >= 150


def test_k_equals_n_against_per_query_oracles(oracle_mod, restated_host_libm):
    """One seeded random set per query (K = n, 20 k queries): every 40th query against the parity oracle built from its own limits."""
    from longtermplanner_amd import generate_queries
    import torch
    n = 20000
    rng = np.random.default_rng(99)
    base = _set_list()[0]
    scale = rng.uniform(0.3, 1.5, (n, 1))
    L = {k: np.ascontiguousarray(np.broadcast_to(np.asarray(base[k])[None, :] * (scale if k in ("v_max", "a_max", "j_max") else 1.0), (n, 7)))
         for k in LIM_KEYS}
    qs = [np.ascontiguousarray(x) for x in generate_queries(n, {k: np.min(L[k], 0) for k in LIM_KEYS}, seed=5)]
    p = _planner(base)
    p.setLimitSets(*[L[k] for k in LIM_KEYS])
    assert p.limitSets == n
    b = p.planSwitchTimesBatch(*_tensors(qs), limit_set=torch.arange(n, dtype=torch.int32, device=DEV))
    dev = _host(b)
    checked = 0
    for q in range(0, n, 40):
        orec = oracle_mod.Oracle(7, TS, **{k: list(L[k][q]) for k in LIM_KEYS}).plan_batch(*[x[q:q + 1] for x in qs])
        assert dev["traj_len"][q] == np.asarray(orec["traj_len"])[0], q
        if dev["traj_len"][q] > 0:
            for k in ("t_scaled", "v_drive", "t_required"):
                assert np.array_equal(dev[k][q:q + 1].view(np.uint64), np.asarray(orec[k]).view(np.uint64)), (q, k)
            checked += 1
    assert checked > 400


def test_k1_matches_unbound():
    import torch
    sets = _set_list()[:1]
    qs, _ = _mixed(sets, 50000, seed=8)
    p0 = _planner(sets[0])
    b0 = p0.planSwitchTimesBatch(*_tensors(qs), end_limit=True)
    p1 = _planner(sets[0])
    p1.setLimitSets(*_stack(sets))
    b1 = p1.planSwitchTimesBatch(*_tensors(qs), limit_set=torch.zeros(50000, dtype=torch.int32, device=DEV), end_limit=True)
    r0, r1 = _host(b0), _host(b1)
    _assert_records(r1, r0, np.ones(50000, bool), "K = 1")
    m = 2000
    t0 = torch.zeros(int(r0["offsets"][m]), dtype=torch.float64, device=DEV)
    t1 = torch.zeros(int(r1["offsets"][m]), dtype=torch.float64, device=DEV)
    p0.sampleBatch(b0, 0, m, t0)
    p1.sampleBatch(b1, 0, m, t1)
    assert _same_bits(t0, t1)


SAMPLERS = [("auto", "f64"), ("fused", "f64"), ("walk", "f64"), ("walk_streaming", "f64"), ("table", "f64"), ("auto", "f32")]


@pytest.mark.parametrize("cap", [0, 16, 32, 256])
def test_rows_of_every_sampler(cap):
    import torch
    sets = _set_list()
    n = 2000 if cap in (0, 256) else 30000
    qs, idx = _mixed(sets, n, seed=31 + cap)
    p, b = _plan_mixed(sets, qs, idx, max_samples=cap)
    each = _plan_each(sets, qs, max_samples=cap)
    mo = _host(b)["offsets"]
    for sampler, fmt in SAMPLERS:
        for verdict in ((True, False) if cap == 32 else (True,)):
            dt = torch.float32 if fmt == "f32" else torch.float64
            tile = torch.zeros(int(mo[n]) + 32, dtype=dt, device=DEV)
            p.sampleBatchEx(b, 0, n, tile, sampler=sampler, verdict=verdict)
            for s, (ps, bs) in enumerate(each):
                so = _host(bs)["offsets"]
                ts = torch.zeros(int(so[n]) + 32, dtype=dt, device=DEV)
                ps.sampleBatchEx(bs, 0, n, ts, sampler=sampler, verdict=verdict)
                plans = np.nonzero(idx == s)[0]
                assert _same_bits(_gather(tile, mo, plans), _gather(ts, so, plans)), (sampler, fmt, cap, verdict, s)
            st = _host(b)["status"]
            for s, (ps, bs) in enumerate(each):
                assert np.array_equal(st[idx == s], _host(bs)["status"][idx == s]), (sampler, fmt, cap, s)


def test_stride_rows():
    import torch
    sets = _set_list()
    n = 2000
    qs, idx = _mixed(sets, n, seed=41)
    p, b = _plan_mixed(sets, qs, idx)
    p.setSampleStride(4)
    b = p.planSwitchTimesBatch(*_tensors(qs), limit_set=torch.from_numpy(idx).to(DEV))
    mo = _host(b)["offsets"]
    tile = torch.zeros(int(mo[n]) + 32, dtype=torch.float64, device=DEV)
    p.sampleBatch(b, 0, n, tile)
    for s, lim in enumerate(sets):
        ps = _planner(lim)
        ps.setSampleStride(4)
        bs = ps.planSwitchTimesBatch(*_tensors(qs))
        so = _host(bs)["offsets"]
        ts = torch.zeros(int(so[n]) + 32, dtype=torch.float64, device=DEV)
        ps.sampleBatch(bs, 0, n, ts)
        plans = np.nonzero(idx == s)[0]
        assert _same_bits(_gather(tile, mo, plans), _gather(ts, so, plans)), s


def test_consumers():
    import torch
    sets = _set_list()
    n = 4000
    qs, idx = _mixed(sets, n, seed=51)
    p, b = _plan_mixed(sets, qs, idx)
    each = _plan_each(sets, qs)
    k = torch.from_numpy(np.random.default_rng(1).integers(0, 3000, n).astype(np.int32)).to(DEV)
    outs = {}
    for mode in ("analytic", "exhaustive"):
        p.setEnvelopeMode(mode)
        outs["env_" + mode] = p.envelopeBatch(b, 0, n, 100, 20).clone()
    outs["state"] = [x.clone() for x in p.stateAt(b, 0, n, k)]
    mo = _host(b)["offsets"]
    for fmt in (torch.float64, torch.float32):
        tile = torch.zeros(int(mo[n]) + 32, dtype=fmt, device=DEV)
        p.sampleBatch(b, 0, n, tile)
        outs[f"replan_{fmt}"] = [x.clone() for x in p.replanStates(b, 0, n, tile, k)]
    p.endLimit(b, 0, n)
    st = _host(b)["status"]
    for s, (ps, bs) in enumerate(each):
        m = torch.from_numpy(idx == s).to(DEV)
        for mode in ("analytic", "exhaustive"):
            ps.setEnvelopeMode(mode)
            e = ps.envelopeBatch(bs, 0, n, 100, 20)
            assert _same_bits(outs["env_" + mode][m], e[m]), (s, mode)
        for sa, sb in zip(outs["state"], ps.stateAt(bs, 0, n, k)):
            assert _same_bits(sa[m], sb[m]), s
        so = _host(bs)["offsets"]
        for fmt in (torch.float64, torch.float32):
            ts = torch.zeros(int(so[n]) + 32, dtype=fmt, device=DEV)
            ps.sampleBatch(bs, 0, n, ts)
            for sa, sb in zip(outs[f"replan_{fmt}"], ps.replanStates(bs, 0, n, ts, k)):
                assert _same_bits(sa[m], sb[m]), (s, fmt)
        ps.endLimit(bs, 0, n)
        assert np.array_equal(st[idx == s], _host(bs)["status"][idx == s]), s


def test_run_table_bytes_per_plan_and_joint():
    """The run tables of each (plan, joint) lane, word for word (zeroed buffers: a lane writes only the words of its own runs)."""
    import torch
    sets = _set_list()
    n = 3000
    qs, idx = _mixed(sets, n, seed=61)
    p, b = _plan_mixed(sets, qs, idx)
    words = int(p._lib.ltp_run_tables_bytes(p._h, n)) // 8
    tm = p.buildRunTables(b, 0, n, out=torch.zeros(words, dtype=torch.int64, device=DEV))
    for s, (ps, bs) in enumerate(_plan_each(sets, qs)):
        ts = ps.buildRunTables(bs, 0, n, out=torch.zeros(words, dtype=torch.int64, device=DEV))
        lanes = (np.nonzero(idx == s)[0][:, None] * 7 + np.arange(7)[None, :]).ravel()
        assert np.array_equal(_lane_words(tm, lanes), _lane_words(ts, lanes)), s


def test_retime_across_sets():
    import torch
    sets = _set_list()
    n = 20000
    qs, idx = _mixed(sets, n, seed=71)
    p, b = _plan_mixed(sets, qs, idx)
    rng = np.random.default_rng(4)
    group = torch.from_numpy(rng.integers(0, 50, n).astype(np.int32)).to(DEV)
    target = torch.from_numpy(rng.uniform(0.0, 6.0, n)).to(DEV)
    gt = p.retimeBatch(b, t_target=target, group=group, n_groups=50)
    mixed = _host(b)
    tq = torch.maximum(target, gt[group.long()])
    for s, (ps, bs) in enumerate(_plan_each(sets, qs)):
        ps.retimeBatch(bs, t_target=tq)
        _assert_records(mixed, _host(bs), idx == s, f"retime set {s}")


def test_bad_indices():
    import torch
    sets = _set_list()
    n = 20000
    qs, idx = _mixed(sets, n, seed=81)
    bad = idx.copy()
    pos = np.arange(5, n, 97)
    bad[pos] = np.array([-1, len(sets), 2 ** 31 - 1], dtype=np.int32)[np.arange(pos.size) % 3]
    p, b = _plan_mixed(sets, qs, bad, max_samples=32)
    p.endLimit(b, 0, n)
    r = _host(b)
    assert np.all(r["status"][pos] == 512) and np.all(r["traj_len"][pos] == 0) and np.all(r["slowest"][pos] == -1)
    assert np.all(np.diff(r["offsets"].astype(np.int64))[pos] == 0)
    p2, b2 = _plan_mixed(sets, qs, idx, max_samples=32)
    p2.endLimit(b2, 0, n)
    good = np.ones(n, bool)
    good[pos] = False
    r2 = _host(b2)
    for k in REC_KEYS:
        assert np.array_equal(_bits(r[k])[good], _bits(r2[k])[good]), k
    t1 = torch.zeros(int(r["offsets"][n]) + 32, dtype=torch.float64, device=DEV)
    t2 = torch.zeros(int(r2["offsets"][n]) + 32, dtype=torch.float64, device=DEV)
    p.sampleBatch(b, 0, n, t1)
    p2.sampleBatch(b2, 0, n, t2)
    plans = np.nonzero(good)[0]
    assert _same_bits(_gather(t1, r["offsets"], plans), _gather(t2, r2["offsets"], plans))
    gt = p.retimeBatch(b, uniform=10.0)
    assert gt is None and np.all(_host(b)["traj_len"][pos] == 0)


def test_refusals():
    import torch
    from longtermplanner_amd import _abi
    sets = _set_list()
    n = 1000
    qs, idx = _mixed(sets, n, seed=91)
    ix = torch.from_numpy(idx).to(DEV)
    p = _planner(sets[0])
    lib, h = p._lib, p._h
    assert lib.ltp_bind_limit_sets(h, C.c_void_p(ix.data_ptr())) == 1 and "no limit sets" in _err(p)
    p.setLimitSets(*_stack(sets))
    assert p.limitSets == 5
    # MATLAB semantics
    p.setSemantics("matlab")
    with pytest.raises(_abi.LtpError, match="MATLAB"):
        p.planSwitchTimesBatch(*_tensors(qs), limit_set=ix)
    p.setSemantics("cpp")
    # sets given for another dof
    p.setDoF(6)
    with pytest.raises(_abi.LtpError, match="dof"):
        p.planSwitchTimesBatch(*[t[:, :6].contiguous() for t in _tensors(qs)], limit_set=ix)
    p.setDoF(7)
    p.setLimitSets(*_stack(sets))
    # geometry: binding, n_sets and generation changed between planning and a consumer
    b = p.planSwitchTimesBatch(*_tensors(qs), limit_set=ix)
    out = torch.zeros(10, dtype=torch.float64, device=DEV)
    for change in ("bind", "n_sets", "generation"):
        b = p.planSwitchTimesBatch(*_tensors(qs), limit_set=ix, batch=b)
        if change == "bind":
            b.limit_set = ix.clone()
        elif change == "n_sets":
            p.setLimitSets(*_stack(sets[:4]))
        else:
            p.setLimitSets(*_stack(sets))
        with pytest.raises(_abi.LtpError, match="limit-set"):
            p.stateAt(b, 0, n, 0)
        p.setLimitSets(*_stack(sets))
    # multi entries refuse a bound planner
    lib.ltp_bind_limit_sets(h, C.c_void_p(ix.data_ptr()))
    arr = (C.c_void_p * 1)(h)
    rc = lib.ltp_plan_batch_multi(arr, 1, 0, None, None, None, None, None, None, None)
    assert rc == 1 and "multi" in _err(p)
    # the Python sharded wrappers remove a binding an earlier batch left: the user never bound anything
    p.planSwitchTimesBatch(*_tensors(qs), limit_set=ix)
    from longtermplanner_amd import LongTermPlanner
    sh = LongTermPlanner.planBatchSharded([p], *qs, sample=False)
    ref = _planner(sets[0]).planBatchHost(*qs, sample=False)
    assert np.array_equal(sh["t_scaled"].view(np.uint64), ref["t_scaled"].view(np.uint64))
    # unbinding restores the default path
    lib.ltp_bind_limit_sets(h, None)
    p0 = _planner(sets[0])
    r_unbound = _host(p.planSwitchTimesBatch(*_tensors(qs)))
    _assert_records(r_unbound, _host(p0.planSwitchTimesBatch(*_tensors(qs))), np.ones(n, bool), "unbound")
    # n_sets = 0 removes the sets and unbinds
    lib.ltp_bind_limit_sets(h, C.c_void_p(ix.data_ptr()))
    p.setLimitSets(None, None, None, None, None)
    assert p.limitSets == 0
    _assert_records(_host(p.planSwitchTimesBatch(*_tensors(qs))), r_unbound, np.ones(n, bool), "cleared")


def test_graph_capture_replays_new_queries_and_indices():
    import torch
    sets = _set_list()
    n = 4096
    qa, ia = _mixed(sets, n, seed=101)
    qb, ib = _mixed(sets, n, seed=102)
    p = _planner(sets[0], max_samples=32)
    p.setLimitSets(*_stack(sets))
    p._lib.ltp_reserve_batch(p._h, n)
    ins = _tensors(qa)
    ix = torch.from_numpy(ia).to(DEV)
    b = p.planSwitchTimesBatch(*ins, limit_set=ix)
    cap = n * 7 * 4 * 32
    tile = torch.zeros(cap, dtype=torch.float64, device=DEV)
    p.sampleBatch(b, 0, n, tile)   # warm-up: workspace and queue heads exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            p.planSwitchTimesBatch(*ins, limit_set=ix, batch=b)
            p.sampleBatch(b, 0, n, tile)
    for src, idx in ((qb, ib), (qa, ia)):
        for t, x in zip(ins, _tensors(src)):
            t.copy_(x)
        ix.copy_(torch.from_numpy(idx).to(DEV))
        tile.zero_()                   # (row padding is never written: compare against a zeroed tile like td)
        g.replay()
        torch.cuda.synchronize()
        got, rows = _host(b), tile.clone()
        q = _planner(sets[0], max_samples=32)
        q.setLimitSets(*_stack(sets))
        bd = q.planSwitchTimesBatch(*_tensors(src), limit_set=torch.from_numpy(idx).to(DEV))
        td = torch.zeros(cap, dtype=torch.float64, device=DEV)
        q.sampleBatch(bd, 0, n, td)
        _assert_records(got, _host(bd), np.ones(n, bool), "replay")
        assert _same_bits(rows, td)
    # new VALUES for the same number of sets: the table is reused in place at the same offsets, and a replay plans with them
    new_sets = sets[::-1]
    p.setLimitSets(*_stack(new_sets))
    tile.zero_()
    g.replay()
    torch.cuda.synchronize()
    q = _planner(sets[0], max_samples=32)
    q.setLimitSets(*_stack(new_sets))
    bd = q.planSwitchTimesBatch(*_tensors(qa), limit_set=torch.from_numpy(ia).to(DEV))
    td = torch.zeros(cap, dtype=torch.float64, device=DEV)
    q.sampleBatch(bd, 0, n, td)
    _assert_records(_host(b), _host(bd), np.ones(n, bool), "replay after new values")
    assert _same_bits(tile, td)


def test_host_paths_match_the_device_path():
    import torch
    sets = _set_list()
    n = 3000
    qs, idx = _mixed(sets, n, seed=111)
    p, b = _plan_mixed(sets, qs, idx)
    mo = _host(b)["offsets"]
    tile = torch.zeros(int(mo[n]) + 32, dtype=torch.float64, device=DEV)
    p.sampleBatch(b, 0, n, tile)
    dev = _host(b)
    rows = tile[: int(mo[n])].cpu().numpy()
    h = p.planBatchHost(*qs, limit_set=idx)
    for k in REC_KEYS:
        assert np.array_equal(_bits(h[k]), _bits(dev[k])), k
    assert np.array_equal(h["offsets"], mo) and np.array_equal(h["packed"].view(np.uint64), rows.view(np.uint64))
    # the host call leaves the handle's own binding and planned geometry alone
    p.stateAt(b, 0, n, 0)
    # a plain host call ignores the binding: the handle's own limits
    plain = p.planBatchHost(*qs, sample=False)
    ref = _planner(sets[0]).planBatchHost(*qs, sample=False)
    for k in REC_KEYS:
        assert np.array_equal(_bits(plain[k]), _bits(ref[k])), k


DROPIN_SETS = r"""
#include <long_term_planner/long_term_planner.h>
#include <cstdio>
#include <vector>
// in.bin: n, K, limits [5][K * 7], queries [4][n * 7], set index [n] (doubles). out.bin, three times (sets as given; after a
// change that re-creates the handle's configuration; after setDoF away and back): status, traj_len, t_scaled, offsets, packed
// (doubles), with a refusal flag between the second and the third.
int main(int argc, char** argv) {
  FILE* f = std::fopen(argv[1], "rb");
  double hdr[2];
  if (!f || std::fread(hdr, sizeof(double), 2, f) != 2) return 2;
  const long long n = (long long)hdr[0];
  const int K = (int)hdr[1];
  std::vector<double> lim(5 * K * 7), q(4 * n * 7), ixd(n);
  if (std::fread(lim.data(), sizeof(double), lim.size(), f) != lim.size()) return 2;
  if (std::fread(q.data(), sizeof(double), q.size(), f) != q.size()) return 2;
  if (std::fread(ixd.data(), sizeof(double), ixd.size(), f) != ixd.size()) return 2;
  std::fclose(f);
  std::vector<int> ix(ixd.begin(), ixd.end());
  auto own = [&](int k) { return std::vector<double>(lim.begin() + k * K * 7, lim.begin() + k * K * 7 + 7); };   // set 0
  long_term_planner::LongTermPlanner p(7, 0.001, own(0), own(1), own(2), own(3), own(4));
  const int rows = K * 7;
  p.setLimitSets(K, &lim[0], &lim[rows], &lim[2 * rows], &lim[3 * rows], &lim[4 * rows]);
  FILE* o = std::fopen(argv[2], "wb");
  auto run = [&]() {
    long_term_planner::BatchTrajectory out;
    p.planTrajectoryBatch(n, &q[0], &q[n * 7], &q[2 * n * 7], &q[3 * n * 7], ix.data(), out);
    for (long long i = 0; i < n; ++i) { const double s = out.status[i], l = out.length[i]; std::fwrite(&s, 8, 1, o); std::fwrite(&l, 8, 1, o); }
    std::fwrite(out.t_scaled.data(), 8, out.t_scaled.size(), o);
    for (auto v : out.offsets) { const double d = (double)v; std::fwrite(&d, 8, 1, o); }
    std::fwrite(out.packed.data(), 8, out.packed.size(), o);
  };
  run();
  p.setMaxSamples(0);                  // marks the configuration dirty: the sets are handed to the handle again
  run();
  p.setDoF(6);                         // the sets were given for 7 joints: not handed over, the call is refused
  double refused = 0.0;
  try { long_term_planner::BatchTrajectory out; p.planTrajectoryBatch(n, &q[0], &q[n * 7], &q[2 * n * 7], &q[3 * n * 7], ix.data(), out); }
  catch (const std::exception&) { refused = 1.0; }
  std::fwrite(&refused, 8, 1, o);
  p.setDoF(7);                         // back: the sets apply again
  run();
  std::fclose(o);
  return 0;
}
"""


def test_dropin_program_matches_the_device_path(tmp_path):
    """A compiled drop-in program (planTrajectoryBatch(..., limit_set, ...)) gives what planBatchHost(limit_set=...) gives, also after
    its configuration is handed to the handle again, and refuses the sets while the dof differs from theirs."""
    sets = _set_list()
    n = 400
    qs, idx = _mixed(sets, n, seed=121)
    src = tmp_path / "sets.cc"
    src.write_text(DROPIN_SETS)
    exe = tmp_path / "sets"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "longtermplanner_amd"), "-lltp_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "longtermplanner_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    lim = np.concatenate([a.reshape(-1) for a in _stack(sets)])
    blob = np.concatenate([[n, len(sets)], lim] + [x.reshape(-1) for x in qs] + [idx.astype(np.float64)])
    (tmp_path / "in.bin").write_bytes(blob.astype(np.float64).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    data = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    p = _planner(sets[0])
    p.setLimitSets(*_stack(sets))
    h = p.planBatchHost(*qs, limit_set=idx)
    total = int(h["offsets"][n])
    at = 0

    def one(at):
        sl = data[at: at + 2 * n].reshape(n, 2)
        at += 2 * n
        ts = data[at: at + n * 49]
        at += n * 49
        off = data[at: at + n + 1]
        at += n + 1
        packed = data[at: at + total]
        at += total
        assert np.array_equal(sl[:, 0], h["status"]) and np.array_equal(sl[:, 1], h["traj_len"])
        assert np.array_equal(ts.view(np.uint64), h["t_scaled"].reshape(-1).view(np.uint64))
        assert np.array_equal(off, h["offsets"].astype(np.float64))
        assert np.array_equal(packed.view(np.uint64), h["packed"].view(np.uint64))
        return at
    at = one(at)
    at = one(at)
    assert data[at] == 1.0
    at = one(at + 1)
    assert at == data.size
