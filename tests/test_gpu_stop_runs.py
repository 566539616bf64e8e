"""Stop plans and stop horizons outside the named sets, on the GPU. tests/test_gpu_stop.py and tests/test_gpu_stop_knots.py pin
ltp_plan_stop_batch and ltp_stop_knots_batch on panda / S-ref / 30-DoF states at 1 ms: one regime of optBraking, whose branch test
`r[1] < -t_sample` depends on the sample time. Here the states are those of tests/stop_census.py — samples of the oracle's rows of
every run-census batch (sample times of 0.05 to 1 s, dyadic inputs) and of the soft dense batch (jerk-dominated limits) — and every
handle runs at its batch's own sample time. The stop plans are a run structure the stop rows never had: 1 to 4 samples in bulk,
switch indices 3..6 collided in every lane, a NEGATIVE first fill (phase 2 keeps its negative duration), the last correction
dropped, exact multiples of the sample time; a joint at rest has a non-zero standstill time where a_max / j_max <= Ts.

Records, q_stop, offsets, rows, every sampler, float32, the end-limit verdict and planStopFrom are compared with
tests/stop_checker.py, and stopKnots with the composition Y of tests/horizon_helpers.py and with the oracle's optBraking on the
device's own knot states, class by class: a mismatch names the optBraking classes of the lanes concerned and the source lanes they
were sampled from, and every class that tests/test_stop_census_cpu.py says a batch holds must be present in its comparison.

Tolerances are the suite's own: bit identity under pow_rule "exact" against the oracle's exact-pow twin and under "libm" behind the
restated_host_libm fixture; 1e-9 with j bit-identical for rows."""
import numpy as np
import pytest

import branch_census as bc
import horizon_helpers as H
import knots_checker as kc
import run_census as rc
import stop_census as sn
import stop_checker as sc
import stop_knots_checker as skc
from gpu_helpers import DEV, REC_KEYS, _agree, _bits_equal, _host, _planner, _rows, _tensors

pytestmark = pytest.mark.gpu


def _stop(S, idx, check, layout="query_major", ltp=None, **kw):
    """planStopBatch of the states S[idx] at the batch's own sample time: (batch, host records, host q_stop [n][dof])."""
    import torch
    ins = _tensors([S["q0"][idx], S["v0"][idx], S["a0"][idx]], layout)
    batch = ltp.planStopBatch(*ins, layout=layout, check=check, **kw)
    torch.cuda.synchronize()
    qs = batch.q_stop.cpu().numpy()
    return batch, _host(batch), np.ascontiguousarray(qs if layout == "query_major" else qs.T)


def _assert_stop_classes(dev, ref, cen, must, what, keys=REC_KEYS + ("q_stop",), where=None):
    """dev == ref bit for bit, optBraking class by class: dev and ref hold arrays [m][dof]... / [m] over the same m states, cen the
    stop_checker.census of those states; every class of `must` is non-empty and compared as its own group. where(states [m]) names
    the source of the states concerned."""
    m, dof = cen[sc.CLASSES[0]].shape
    bad = {}
    for k in keys:
        same = _agree(dev[k], ref[k], True)
        lanes = ~same.reshape(m, dof, -1).all(axis=2) if same.ndim > 1 else np.repeat(~same[:, None], dof, axis=1)
        if lanes.any():
            bad[k] = lanes
    for cls in sc.CLASSES:
        lanes = cen[cls]
        if cls in must:
            assert lanes.any(), f"{what}: no lane of class {cls} in this comparison: it would prove nothing about it"
        for k, b in bad.items():
            hit = b & lanes
            assert not hit.any(), (f"{what}: class {cls}: {k} differs from the checker (bits): {sn.describe(cen, hit)}"
                                   + (f"; {where(hit.any(axis=1))}" if where else ""))
    assert not bad, f"{what}: {sorted(bad)} differ outside every class"


def _cut(cen, idx):
    return {k: v[idx] for k, v in cen.items()}


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
@pytest.mark.parametrize("name", sn.BATCHES)
def test_records_q_stop_and_offsets_by_class(request, oracle_mod, name, pow_rule):
    """planStopBatch with the handle at the batch's own sample time: records and q_stop have the checker's bits (under "exact" its
    exact-pow twin's) in both layouts and both check modes, over the whole batch and over a sub-range whose count * dof is no
    multiple of 64; the offsets are the scan of the padded row sizes, also under a cap of 3 samples and a stride of 2 — the rows
    are that short."""
    if pow_rule == "libm":
        request.getfixturevalue("restated_host_libm")
    S = sn.knot_states(oracle_mod, name)
    cen = sn.census(oracle_mod, name)
    must = sn.present(oracle_mod, name)
    n, dof = S["q0"].shape
    ltp = _planner(dof, S["lim"], S["ts"], pow_rule=pow_rule)
    stride_of = ltp._lib.ltp_row_stride
    first, count = H.odd_range(n, dof)
    assert (count * dof) % 64 != 0
    for check in ("braking", "inputs"):
        E = sn.expected(oracle_mod, name, check, exact_pow=(pow_rule == "exact"))
        for layout in ("query_major", "joint_major"):
            for idx in (np.arange(n), np.arange(first, first + count)):
                what = f"{name} Ts {S['ts']} {pow_rule} {check} {layout} states [{idx[0]}, {idx[-1] + 1})"
                _, rec, qs = _stop(S, idx, check, layout, ltp=ltp)
                _assert_stop_classes(dict(rec, q_stop=qs), {k: E[k][idx] for k in REC_KEYS + ("q_stop",)}, _cut(cen, idx), must, what,
                                     where=lambda st: sn.describe_source(oracle_mod, name, np.isin(np.arange(n), idx[st])))
                assert np.array_equal(rec["offsets"], sc.offsets_of(rec["traj_len"], dof, stride_of)), what
        if check == "braking":
            assert not rec["status"].any() and np.all(rec["traj_len"] > 0), what
            ties = sn.tied(E)[idx]
            assert name not in sn.TIED or ties.sum() >= sn.FLOOR, "states whose slowest joint is the first of several with the same standstill time"
            assert np.all(rec["slowest"][ties] == np.argmax(rec["t_opt"][ties][:, :, 6], axis=1)), what
        else:
            print(f"{name} {pow_rule}: checkInputs admits {int(E['accepted'].sum())} of {n} states")
    E = sn.expected(oracle_mod, name, "braking", exact_pow=(pow_rule == "exact"))
    ltp.setMaxSamples(3)
    ltp.setSampleStride(2)
    _, rec2, qs2 = _stop(S, np.arange(n), "braking", ltp=ltp)
    assert np.array_equal(rec2["traj_len"], E["traj_len"]) and _bits_equal(qs2, E["q_stop"])
    off = sc.offsets_of(E["traj_len"], dof, stride_of, max_samples=3, stride=2)
    assert np.array_equal(rec2["offsets"], off) and off[-1] == 4 * dof * 32 * n, "at most 3 stored samples: one padded line per row"
    assert all(ltp.storedSamples(int(L)) == min(-(-int(L) // 2), 3) for L in np.unique(E["traj_len"]))


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
def test_more_joints_than_joint_slots_tie_inside_a_slot(request, oracle_mod, pow_rule):
    """stop_census.wide_states: 24 joints in 8 joint slots at Ts 1, every state's slowest joint tied with its copies 8 and 16 joints
    on — the joints ONE wave of k_stop goes through in ascending order, so its strict comparison decides `slowest`. Records and
    q_stop have the checker's bits in both layouts and check modes, class by class; `slowest` is below 8 in every state."""
    if pow_rule == "libm":
        request.getfixturevalue("restated_host_libm")
    W = sn.wide_states(oracle_mod)
    n, dof = W["q0"].shape
    orc = oracle_mod.Oracle(dof, W["ts"], exact_pow=True, **W["lim"]) if pow_rule == "exact" else W["orc"]
    cen = sc.census(W["orc"], W["v0"], W["a0"])
    must = sn.present(oracle_mod, "soft_1")
    ltp = _planner(dof, W["lim"], W["ts"], pow_rule=pow_rule)
    first, count = H.odd_range(n, dof)
    for check in ("braking", "inputs"):
        E = sc.expected_stop(orc, W["q0"], W["v0"], W["a0"], check, rows=False)
        for layout in ("query_major", "joint_major"):
            for idx in (np.arange(n), np.arange(first, first + count)):
                what = f"soft_1 on {dof} joints {pow_rule} {check} {layout} states [{idx[0]}, {idx[-1] + 1})"
                _, rec, qs = _stop(W, idx, check, layout, ltp=ltp)
                _assert_stop_classes(dict(rec, q_stop=qs), {k: E[k][idx] for k in REC_KEYS + ("q_stop",)}, _cut(cen, idx), must, what,
                                     where=lambda st: sn.describe_source(oracle_mod, "soft_1", np.isin(np.arange(len(sn.knot_states(oracle_mod, "soft_1")["q0"])), idx[st])))
                assert np.all(rec["slowest"] < sn.WIDE_SLOTS) and np.all(sn.tied(rec)), what
                assert np.array_equal(rec["offsets"], sc.offsets_of(rec["traj_len"], dof, ltp._lib.ltp_row_stride)), what


@pytest.mark.parametrize("name", sn.BATCHES)
def test_rows_by_class(oracle_mod, name):
    """Rows of the stop batch against getTrajectory on the checker's records by the dense-row rule (1e-9, j bit-identical); fused =
    walk = table bit for bit; float32 rows are the float64 rows rounded once; the verdict of ltp_end_limit_batch and the sampler's
    are the checker's status_end (bulk on the soft dense batch). A mismatch names the optBraking classes and the run-census classes
    of the stop lanes concerned."""
    import torch
    from longtermplanner_amd import unpack_trajectory
    S = sn.knot_states(oracle_mod, name)
    cen, runs = sn.census(oracle_mod, name), sn.stop_runs(oracle_mod, name)
    E = sn.expected(oracle_mod, name, "braking", rows=True)
    n, dof = S["q0"].shape
    ltp = _planner(dof, S["lim"], S["ts"])

    def names(lanes):
        lanes = np.asarray(lanes, dtype=bool)
        states = lanes if lanes.ndim == 1 else lanes.any(axis=1)
        return f"{sn.describe(cen, lanes)}; as rows: {rc.describe(runs, lanes)}; {sn.describe_source(oracle_mod, name, states)}"
    batch, before, _ = _stop(S, np.arange(n), "braking", ltp=ltp, end_limit=True)
    bad = before["status"] != E["status_end"]
    assert not bad.any(), f"{name}: the verdict of ltp_end_limit_batch differs from the checker's status_end: {names(bad)}"
    full = torch.zeros(int(before["offsets"][-1]) + 32, dtype=torch.float64, device=DEV)
    ltp.sampleBatchEx(batch, 0, n, full, sampler="fused")
    rec = _host(batch)
    bad = rec["status"] != E["status_end"]
    assert not bad.any(), f"{name}: the sampler's end-limit verdict differs from the checker's status_end: {names(bad)}"
    assert np.array_equal(rec["traj_len"], E["traj_len"]) and np.all(rec["traj_len"] > 0)
    ends = int(np.count_nonzero(E["status_end"] & sc.END_LIMIT))
    if name == sn.SOFT_DENSE:
        assert ends >= 100, ends
    host = full.cpu().numpy()
    far, jerk, worst = np.zeros((n, dof), dtype=bool), np.zeros((n, dof), dtype=bool), 0.0
    for p in range(n):
        got = np.stack(unpack_trajectory(host, int(rec["offsets"][p]), dof, int(rec["traj_len"][p])))
        exp = E["rows"][p]
        d = np.abs(got[:3] - exp[:3])
        worst = max(worst, float(d.max()))
        far[p] = ~_agree(got[:3], exp[:3], False).all(axis=(0, 2))
        jerk[p] = (got[3].view(np.uint64) != exp[3].view(np.uint64)).any(axis=1)
    print(f"{name}: rows of {n} stop plans of {int(rec['traj_len'].min())}-{int(rec['traj_len'].max())} samples, worst |d| of q, v, a {worst:.3e}, "
          f"{ends} end outside the range")
    assert not far.any(), f"{name}: rows differ from the checker's by {worst:.3e} (1e-9): {names(far)}"
    assert not jerk.any(), f"{name}: jerk rows differ from the checker's in a bit: {names(jerk)}"
    for cls in sn.present(oracle_mod, name):
        assert cen[cls].any()
    for cls, c in runs["totals"].items():
        assert c == int(runs["masks"][cls].sum()) and (c == 0 or (rec["traj_len"] > 0)[runs["masks"][cls].any(axis=1)].all()), cls
    off = rec["offsets"].astype(np.int64)

    def plans_that_differ(a, b):
        it = np.uint64 if a.dtype == np.float64 else np.uint32
        at = np.nonzero(a.view(it) != b.view(it))[0]
        return np.isin(np.arange(n), np.clip(np.searchsorted(off, at, side="right") - 1, 0, n - 1))
    for sampler in ("walk", "table"):
        other = torch.zeros_like(full)
        ltp.sampleBatchEx(batch, 0, n, other, sampler=sampler)
        torch.cuda.synchronize()
        assert np.array_equal(_host(batch)["status"], rec["status"]), sampler
        if not torch.equal(other.view(torch.int64), full.view(torch.int64)):
            raise AssertionError(f"{name}: sampler {sampler}: rows differ from the fused sampler's: {names(plans_that_differ(other.cpu().numpy(), host))}")
    want = full.to(torch.float32)
    for sampler in ("fused", "walk", "table"):
        f32 = torch.zeros(full.numel(), dtype=torch.float32, device=DEV)
        ltp.sampleBatchEx(batch, 0, n, f32, sampler=sampler)
        torch.cuda.synchronize()
        if not torch.equal(f32.view(torch.int32), want.view(torch.int32)):
            raise AssertionError(f"{name}: float32 rows ({sampler}) are not the float64 rows rounded once: "
                                 f"{names(plans_that_differ(f32.cpu().numpy(), want.cpu().numpy()))}")


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
@pytest.mark.parametrize("name", tuple(rc.COARSE))
def test_plan_stop_from_on_the_coarse_batches(request, oracle_mod, name, pow_rule):
    """planStopFrom on the run-census batch as the device planned it = stateAt, the clamp of a_0 to +-a_max, planStopBatch: the
    checker on stateAt's states after the clamp, bit for bit, three draws of one sample per plan. At a coarse sample time the clamp
    is a bulk path: at least 100 of the states exceed a_max before it."""
    import torch
    if pow_rule == "libm":
        request.getfixturevalue("restated_host_libm")
    R = _rows(oracle_mod, name, pow_rule)
    ltp, batch, n, dof, ts = R["ltp"], R["batch"], R["n"], R["dof"], R["ts"]
    lens = R["rec"]["traj_len"].astype(np.int64)
    has = lens > 0
    orc = oracle_mod.Oracle(dof, ts, exact_pow=(pow_rule == "exact"), **R["lim"])
    rng = np.random.default_rng(8)
    clamped, seen = 0, {k: 0 for k in sc.CLASSES}
    for draw in range(3):
        k = rng.integers(0, np.maximum(lens, 1)).astype(np.int32)
        kt = torch.from_numpy(k).to(DEV)
        q, v, a = (x.cpu().numpy() for x in ltp.stateAt(batch, 0, n, kt))
        ac = np.clip(a, -orc.a_max, orc.a_max)
        stop = ltp.planStopFrom(batch, 0, n, kt)
        torch.cuda.synchronize()
        assert _bits_equal(stop.inputs[3].cpu().numpy()[has], ac[has]) and _bits_equal(stop.inputs[1].cpu().numpy()[has], q[has])
        clamped += int(np.count_nonzero(np.any(np.abs(a[has]) > orc.a_max[None, :], axis=1)))
        E = sc.expected_stop(orc, q[has], v[has], ac[has], "braking", rows=False)
        cen = sc.census(orc, v[has], ac[has])
        dev = {key: val[has] for key, val in _host(stop).items() if key in REC_KEYS}
        dev["q_stop"] = stop.q_stop.cpu().numpy()[has]
        plans = np.nonzero(has)[0]
        _assert_stop_classes(dev, E, cen, (), f"{name} {pow_rule} planStopFrom draw {draw}",
                             where=lambda st: f"sampled at plan {plans[st][:3]} sample {k[has][st][:3]}: {rc.describe(R['cen'], np.isin(np.arange(n), plans[st]))}")
        assert not E["status"].any()
        for key in sc.CLASSES:
            seen[key] += int(cen[key].sum())
    print(f"{name} {pow_rule}: {clamped} of {3 * int(has.sum())} states exceed a_max before the clamp; lanes per class {seen}")
    assert clamped >= 100, clamped
    for key in sn.present(oracle_mod, name):
        assert seen[key] >= sn.FLOOR, (name, key, seen)


_DENSE = {}


def _planned(oracle_mod, name, pow_rule):
    """The batch the knot states are read from, planned on the device at its own sample time: dict ltp, batch, n, dof, ts, lim, lens,
    t_scaled, describe (of whole plans, by the source census)."""
    if name != sn.SOFT_DENSE:
        R = _rows(oracle_mod, name, pow_rule)
        return dict(ltp=R["ltp"], batch=R["batch"], n=R["n"], dof=R["dof"], ts=R["ts"], lim=R["lim"], lens=R["rec"]["traj_len"],
                    t_scaled=R["rec"]["t_scaled"], cen=R["cen"], describe=lambda plans: rc.describe(R["cen"], plans))
    if pow_rule not in _DENSE:
        dof, n, ts = bc.DENSE_BATCH
        orc, lim, qs, orec, cen = bc.soft_batch(oracle_mod, dof, n, ts)
        m = sn.ROWS_N
        cen = {k: v[:m] for k, v in cen.items() if k != "totals"}
        ltp = _planner(dof, lim, ts, pow_rule=pow_rule)
        batch = ltp.planSwitchTimesBatch(*_tensors([x[:m] for x in qs]))
        rec = _host(batch)
        assert np.array_equal(rec["traj_len"] > 0, orec["status"][:m] != 0) and (rec["traj_len"] == 0).sum() >= 3, "OPT_FAILED plans among the planned ones"
        _DENSE[pow_rule] = dict(ltp=ltp, batch=batch, n=m, dof=dof, ts=ts, lim=lim, lens=rec["traj_len"], t_scaled=rec["t_scaled"], cen=cen,
                                describe=lambda plans: bc.describe(cen, plans))
    return _DENSE[pow_rule]


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
@pytest.mark.parametrize("name", sn.BATCHES)
def test_stop_knots_against_the_composition(oracle_mod, name, pow_rule):
    """stopKnots against Y in both acceleration modes on the three smallest grids, a uniform k swept over 0 .. 8 and per-plan starts
    with negative and past-the-end ones, the whole batch and an odd sub-range. ref_0.05 holds the lanes with kMaxSegments runs, six
    batches take more passes than one, dyadic_grid and dyadic_moving_1 hold the rows of 1 to 4 samples: asserted, not assumed."""
    D = _planned(oracle_mod, name, pow_rule)
    ltp, batch, n, dof, lens = D["ltp"], D["batch"], D["n"], D["dof"], D["lens"]
    assert list(kc.SMALL_GRIDS) == ["unit", "two", "duplicates"]
    if name != sn.SOFT_DENSE:
        held = rc.assert_reader_shapes(name, D["cen"], lens, D["t_scaled"], D["ts"], kc.SMALL_GRIDS["unit"])
        print(f"{name} {pow_rule}: {held}")
    rng = np.random.default_rng(99)
    first, count = H.odd_range(n, dof)
    assert (count * dof) % 64 != 0
    refused = 0
    for gname, g in kc.SMALL_GRIDS.items():
        ku = H.uniform_starts(rng, lens)
        assert np.count_nonzero(ku < 0) > 0 and np.count_nonzero(ku >= lens) > 0
        for k in list(range(9)) + [ku]:
            what = f"{name} Ts {D['ts']} {pow_rule} grid {gname} k {'per plan' if not isinstance(k, int) else k}"
            refused += H.assert_stop_knots(ltp, batch, k, g, 0, n, what, describe=D["describe"])
        H.assert_stop_knots(ltp, batch, ku, g, first, count, f"{name} {pow_rule} grid {gname}, plans [{first}, {first + count})", describe=D["describe"])
    print(f"{name} {pow_rule}: {refused} elements with |a| > a_max")
    if name in rc.COARSE:
        assert refused >= 100, refused


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
@pytest.mark.parametrize("name", sn.BATCHES)
def test_stop_knots_against_the_oracle(request, oracle_mod, name, pow_rule):
    """The oracle's optBraking (under "exact" its exact-pow twin) at the batch's own sample time, applied on the host to the
    device's own knot states of up to 176 plans (spread over the batch and aimed at every class), gives the device's bits in both
    modes, class by class; a
    joint at rest stops where it is, in no time or — where a_max / j_max <= Ts — in a_max / j_max, as the CPU census established."""
    import torch
    if pow_rule == "libm":
        request.getfixturevalue("restated_host_libm")
    D = _planned(oracle_mod, name, pow_rule)
    ltp, batch, n, dof, lens, ts = D["ltp"], D["batch"], D["n"], D["dof"], D["lens"], D["ts"]
    g = kc.SMALL_GRIDS["duplicates"]
    N = len(g)
    orc = oracle_mod.Oracle(dof, ts, exact_pow=(pow_rule == "exact"), **D["lim"])
    kh = H.uniform_starts(np.random.default_rng(8), lens)
    if name == sn.SOFT_DENSE:                      # rows of up to 2 487 samples against a grid of 160: every third plan starts near its end
        kh[::3] = np.maximum(lens[::3].astype(np.int64) - 20, 0)
    k = torch.from_numpy(kh).to(DEV)
    rows, valid = ltp.sampleKnots(batch, 0, n, k, H.grid_tensor(g))
    every = rows[..., :N].cpu().numpy()
    lanes_of = lambda x: np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(-1, dof)             # [(plan, knot)][joint]
    # the plans whose knot states go through the host loop: 64 spread over the batch and, class by class, up to 16 of the plans
    # that hold the class (a rare one sits in few plans: dir_from_a in 14 of the 1000 of panda_0.1)
    planned = np.nonzero(lens > 0)[0]
    pick = set(planned[np.linspace(0, len(planned) - 1, min(64, len(planned))).astype(np.int64)].tolist())
    whole = sc.census(orc, lanes_of(every[:, 1]), lanes_of(skc.clamped(every[:, 2], orc.a_max)))
    for cls in sn.present(oracle_mod, name):
        holds = np.nonzero(whole[cls].reshape(n, N * dof).any(axis=1) & (lens > 0))[0]
        assert len(holds), f"{name}: no knot state of class {cls} in the whole batch"
        pick |= set(holds[np.linspace(0, len(holds) - 1, min(16, len(holds))).astype(np.int64)].tolist())
    pick = np.array(sorted(pick))
    states = every[pick]
    m = len(pick)
    cen = sc.census(orc, lanes_of(states[:, 1]), lanes_of(skc.clamped(states[:, 2], orc.a_max)))
    for cls in sn.present(oracle_mod, name):
        assert cen[cls].any(), f"{name}: no knot state of class {cls}"
    for clamp, accel in ((True, skc.CLAMP), (False, skc.STRICT)):
        got, v2 = ltp.stopKnots(batch, 0, n, k, H.grid_tensor(g), clamp_acceleration=clamp)
        got = got[..., :N].cpu().numpy()[pick]
        exp = skc.expected(orc, states, orc.a_max, accel)
        same = _agree(got, exp, True)
        bad = lanes_of(~same[:, 0]) | lanes_of(~same[:, 1])
        where = np.unique(pick[np.nonzero(bad.any(axis=1))[0] // N])
        assert not bad.any(), (f"{name} Ts {ts} {pow_rule} clamp={clamp}: q_stop or t_stop differs from the oracle's optBraking (bits): {sn.describe(cen, bad)}; "
                               f"plans {where[:5]}: {D['describe'](np.isin(np.arange(n), where))}")
        assert torch.equal(valid, v2)
    # a joint at rest
    tj = orc.a_max / orc.j_max
    rest = (states[:, 1] == 0.0) & (states[:, 2] == 0.0)
    assert rest.sum() >= sn.FLOOR
    want_t = np.broadcast_to(np.where(tj > ts, 0.0, tj)[None, :, None], rest.shape)
    assert _bits_equal(got[:, 0][rest], states[:, 0][rest]), f"{name}: a joint at rest does not stop at the position it holds"
    assert _bits_equal(got[:, 1][rest], np.ascontiguousarray(want_t[rest])), f"{name}: t_stop of a joint at rest is not {np.where(tj > ts, 0.0, tj)}"
