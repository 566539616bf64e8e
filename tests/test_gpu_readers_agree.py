"""The readers of a planned batch agree with each other, bit for bit, on a sub-range of the batch.

Every reader is a lane-per-(plan, joint) kernel (or a work-queue kernel over the same plans) that turns a lane index into
(local plan, plan, joint), tests the range and reads the start state. This pins that index arithmetic: 130 plans (a partial wave
and a partial 256-lane block), dof 1, 7 and 9 (nine joints are two joint groups of k_sample), every call on plans [3, 103) only,
both semantics. All comparisons are exact; nothing here depends on a CPU checker (the seeds were chosen with it: the assertions on
the three kinds of plan below keep the test from passing vacuously).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, FIRST, COUNT = 130, 3, 100
TS = 0.004
K_UNIFORM = 230          # beyond the shortest plans of the range (the oracle's lengths: from 3, 182 and 211 samples for dof 1, 7, 9)
WINDOW, N_WINDOWS = 64, 12   # 768 samples: beyond the longest plan (672), so windows in, across and past the end all occur
GUARD = 7.0


def _limits(amd, dof):
    _, panda = amd.limit_set("panda")
    return {k: [v[j % 7] for j in range(dof)] for k, v in panda.items()}


def _queries(amd, lim):
    qg, q0, v0, a0 = amd.generate_queries(N, lim, seed=11)
    # an END_LIMIT plan (the recipe of test_end_limit_failures_keep_the_trajectory: query 191 of the seed-77 pool fails cc:59-61 at
    # this sample time for all three dof) and two plans without a trajectory (test_invalid_queries_are_flagged_and_skipped)
    for dst, src in zip((qg, q0, v0, a0), amd.generate_queries(1, lim, seed=77, first_query=191)):
        dst[10] = src[0]
    q0[20, 0] = lim["q_max"][0] + 0.5
    v0[50, -1] = -(lim["v_max"][-1] + 0.5)
    return qg, q0, v0, a0


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _states(ltp, batch, entry, head_args, k, torch):
    """ltp_state_at_batch / ltp_replan_states_batch on [FIRST, FIRST + COUNT) into buffers with a guard row behind them."""
    out = [torch.full((COUNT + 1, ltp.dof), GUARD, dtype=torch.float64, device="cuda") for _ in range(3)]
    per_plan = None if isinstance(k, int) else k
    ltp._bind(batch)
    rec = batch.c_records()
    ltp._check(getattr(ltp._lib, entry)(ltp._h, FIRST, COUNT, C.byref(batch.queries), C.byref(rec), *head_args,
                                        per_plan.data_ptr() if per_plan is not None else None, k if per_plan is None else 0,
                                        *[x.data_ptr() for x in out], ltp.dof, 1, ltp._stream()))
    torch.cuda.synchronize()
    out = np.stack([x.cpu().numpy() for x in out])          # [q, v, a][COUNT + 1][dof]
    assert np.all(out[:, COUNT] == GUARD), entry + " wrote behind its range"
    return out[:, :COUNT]


@pytest.mark.parametrize("semantics", ["cpp", "matlab"])
@pytest.mark.parametrize("dof", [1, 7, 9])
def test_readers_agree_on_a_sub_range(dof, semantics):
    import torch
    import longtermplanner_amd as amd
    lim = _limits(amd, dof)
    ltp = amd.LongTermPlanner(dof, TS, device=0, **lim)
    ltp.setSemantics(semantics)
    ins = [torch.from_numpy(x).cuda() for x in _queries(amd, lim)]
    batch = ltp.planSwitchTimesBatch(*ins)
    torch.cuda.synchronize()
    planned = batch.status.clone()
    st0 = planned.cpu().numpy()
    lens_all = batch.traj_len.cpu().numpy()
    off = batch.offsets.cpu().numpy().view(np.uint64)
    lens = lens_all[FIRST:FIRST + COUNT]
    has = lens > 0
    assert np.count_nonzero(~has) >= 1, "the range holds no plan without a trajectory"
    assert np.count_nonzero(has & (lens <= K_UNIFORM)) >= 1, "the range holds no plan shorter than the sample index"

    # ---- status: every call that forms the end-limit verdict forms the same one, inside the range only ----
    cap = int(off[FIRST + COUNT] - off[FIRST])
    tile = torch.full((cap + 64,), GUARD, dtype=torch.float64, device="cuda")
    words = int(ltp._lib.ltp_run_tables_bytes(ltp._h, COUNT)) // 8
    tables = torch.full((words + 64,), 7, dtype=torch.int64, device="cuda")
    env_walk = torch.full((COUNT + 1, dof, N_WINDOWS, 2), GUARD, dtype=torch.float64, device="cuda")
    ltp.setEnvelopeMode("analytic")
    rows = {}

    def sample(name, **kw):
        tile.fill_(GUARD)
        ltp.sampleBatch(batch, FIRST, COUNT, tile[:cap], **kw)
        torch.cuda.synchronize()
        rows[name] = tile[:cap].cpu().numpy()
        assert torch.all(tile[cap:] == GUARD), name + " wrote behind its tile"

    calls = {
        "endLimit": lambda: ltp.endLimit(batch, FIRST, COUNT),
        "sampleBatch fused": lambda: sample("fused", tables=False, walk=False),
        "sampleBatch walk": lambda: sample("walk", walk=True),
        "buildRunTables": lambda: ltp.buildRunTables(batch, FIRST, COUNT, out=tables),
        "envelope walk": lambda: ltp.envelopeBatch(batch, FIRST, COUNT, WINDOW, N_WINDOWS, out=env_walk),
    }
    status = {}
    for name, call in calls.items():
        batch.status.copy_(planned)                          # a fresh copy of the planned records' status
        call()
        torch.cuda.synchronize()
        status[name] = batch.status.cpu().numpy()
    batch.status.copy_(planned)
    if semantics == "cpp":
        assert ltp.lastSamplerKernel().startswith("k_envelope_walk")
        assert np.count_nonzero(status["endLimit"][FIRST:FIRST + COUNT] & amd.STATUS_END_LIMIT) >= 1, "the range holds no END_LIMIT plan"
    else:
        assert np.array_equal(status["endLimit"], st0)       # LTPlanner.m has no position limits: no verdict in these semantics
    outside = np.r_[0:FIRST, FIRST + COUNT:N]
    for name, st in status.items():
        print(name, "status bits in the range:", np.bincount(st[FIRST:FIRST + COUNT]).nonzero()[0])
        assert np.array_equal(st, status["endLimit"]), name
        assert np.array_equal(st[outside], st0[outside]), name
    assert torch.all(tables[words:] == 7) and torch.all(env_walk[COUNT] == GUARD)
    assert np.array_equal(rows["fused"], rows["walk"])

    # ---- the analytic envelope: the register walk == k_envelope's analytic form through the table pass, in every window ----
    env_tab = torch.full((COUNT + 1, dof, N_WINDOWS, 2), GUARD, dtype=torch.float64, device="cuda")
    ltp.setTablePass(1)
    ltp.envelopeBatch(batch, FIRST, COUNT, WINDOW, N_WINDOWS, out=env_tab)
    torch.cuda.synchronize()
    assert "run tables from k_build_tables" in ltp.lastSamplerKernel()
    ltp.setTablePass(0)
    assert np.array_equal(batch.status.cpu().numpy(), status["endLimit"])
    batch.status.copy_(planned)
    assert torch.all(env_tab[COUNT] == GUARD)
    ew, et = env_walk[:COUNT].cpu().numpy(), env_tab[:COUNT].cpu().numpy()
    assert np.all(np.isnan(ew[~has])) and np.all(np.isfinite(ew[has]))
    assert _eq(ew, et)

    # ---- the state at sample k: stateAt == float64 replanStates == column k of the rows == sample 0 of the window from k ----
    R = ltp.windowRowStride(1)
    k_plan = (np.arange(COUNT, dtype=np.int32) * 37) % 700   # per plan: inside, at and beyond the end
    k_plan[5] = -5                                           # below 0: sample 0
    for k_host, k in ((k_plan, torch.from_numpy(k_plan).cuda()), (np.full(COUNT, K_UNIFORM, dtype=np.int32), K_UNIFORM)):
        assert np.count_nonzero(has & (lens <= k_host)) >= 1
        at = _states(ltp, batch, "ltp_state_at_batch", (), k, torch)
        re = _states(ltp, batch, "ltp_replan_states_batch", (batch.offsets.data_ptr(), tile.data_ptr(), cap), k, torch)
        assert _eq(at, re)
        start = np.stack([x.cpu().numpy()[FIRST:FIRST + COUNT] for x in ins[1:]])
        assert _eq(at[:, ~has], start[:, ~has])              # no trajectory: the start state carries over
        win = torch.full((COUNT + 1, 4, dof, R), GUARD, dtype=torch.float64, device="cuda")
        valid = torch.full((COUNT + 1,), 7, dtype=torch.int32, device="cuda")
        ltp.sampleWindow(batch, FIRST, COUNT, k, 1, out=win, valid=valid)
        torch.cuda.synchronize()
        assert torch.all(win[COUNT] == GUARD) and int(valid[COUNT]) == 7
        win = win[:COUNT, :3, :, 0].cpu().numpy().transpose(1, 0, 2)   # [q, v, a][COUNT][dof]
        kc = np.clip(k_host, 0, np.maximum(lens - 1, 0))     # beyond the end: the last state
        inside = has & (k_host < lens)
        assert np.array_equal(valid[:COUNT].cpu().numpy(), inside.astype(np.int32))
        assert np.all(np.isnan(win[:, ~has]))
        assert _eq(win[:, inside], at[:, inside])
        assert _eq(win[0, has], at[0, has])                  # past the end the window holds the last position
        col = np.full_like(at, np.nan)
        for i in np.nonzero(has)[0]:
            stride = ltp.windowRowStride(int(lens[i]))       # ltp_row_stride: the padded row of a trajectory, too
            rel = int(off[FIRST + i] - off[FIRST])
            col[:, i] = rows["walk"][rel:rel + 4 * dof * stride].reshape(4, dof, stride)[:3, :, kc[i]]
        assert _eq(col[:, has], at[:, has])
    assert np.array_equal(batch.status.cpu().numpy(), st0)   # none of these readers touches the status
