"""SHA-256 of everything the host-pointer entry points return, for seeded queries: run it from two builds, diff the output.

Covers planBatchHost (rows / no rows / duration scalar and per query / limit_set), planEnvelopeHost, getTrajectoryBatchHost, the
one-lane calls, roots (both widths, both size branches) and the two sharded calls (two handles on device 0), for panda, the
reference's limits and 30-DoF under both pow rules, at one batch size per tier of ltp_capi_host.hip (fused, arena, staged).

The readers of a planned batch follow, at one modest batch size: sampleWindow / sampleHorizon / sampleKnots (float64 and float32)
and envelopeKnots (open and closed) into zero-filled tensors, each with a per-plan start tensor and with one int start, and
planWindowHost / planHorizonHost / planKnotsHost / planEnvelopeKnotsHost. Starts: tests/horizon_checker.draw_starts; grids: mpc,
duplicates and one of tests/knots_checker.GRIDS."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np
import longtermplanner_amd as amd

CAP = 16    # setMaxSamples for the arena and staged sizes: rows of a few MB
READER_N = {"panda": 300, "ref": 300, "ref30": 120}


def emit(tag, name, value):
    arrays = value if isinstance(value, dict) else {"": value}
    for key in sorted(arrays):
        a = np.ascontiguousarray(arrays[key])
        print(f"{tag} {name}{'.' if key else ''}{key} {a.dtype}{list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()}")


def tier_sizes(dof):
    per = 161 * dof + 28        # arena bytes per query (arena_layout: 4 inputs, 9 record arrays, offsets); 8 MiB selects the tier
    return {"fused": min(18, 128 // dof), "arena": round(2000 * 1155 / per), "staged": round(9000 * 1155 / per)}


def planner(dof, ts, lim, rule, cap):
    p = amd.LongTermPlanner(dof, ts, device=0, **lim)
    p.setPowRule(rule)
    p.setMaxSamples(cap)
    return p


def batch_entries(tag, dof, ts, lim, rule, n, cap):
    ltp, twin = planner(dof, ts, lim, rule, cap), planner(dof, ts, lim, rule, cap)
    q = amd.generate_queries(n, lim, seed=17)
    q[1][min(3, n - 1), 0] = 99.0                                # rejected by checkInputs
    rng = np.random.default_rng(23)
    rows = ltp.planBatchHost(*q, sample=True)
    emit(tag, "planBatchHost.rows", rows)
    emit(tag, "planBatchHost.norows", ltp.planBatchHost(*q, sample=False))
    emit(tag, "planBatchHost.duration_scalar", ltp.planBatchHost(*q, sample=True, duration=3.0))
    emit(tag, "planBatchHost.duration_each", ltp.planBatchHost(*q, sample=False, duration=rng.uniform(0.5, 4.0, n)))
    scale = np.array([1.0, 0.8, 0.6])[:, None]
    ltp.setLimitSets(*[scale * np.asarray(lim[k])[None, :] for k in ("q_min", "q_max", "v_max", "a_max", "j_max")])
    emit(tag, "planBatchHost.limit_set", ltp.planBatchHost(*q, sample=True, limit_set=rng.integers(0, 3, n)))
    ltp.setLimitSets(None, None, None, None, None)
    rec, env = ltp.planEnvelopeHost(*q, 32, 4)
    emit(tag, "planEnvelopeHost.records", rec)
    emit(tag, "planEnvelopeHost.env", env)
    emit(tag, "getTrajectoryBatchHost", ltp.getTrajectoryBatchHost(rows["t_scaled"], rows["dir"], rows["mod"], q[1], q[2], q[3], rows["v_drive"]))
    emit(tag, "planBatchSharded", amd.LongTermPlanner.planBatchSharded([ltp, twin], *q, sample=True))
    rec, env = amd.LongTermPlanner.planEnvelopeSharded([ltp, twin], *q, 32, 4)
    emit(tag, "planEnvelopeSharded.records", rec)
    emit(tag, "planEnvelopeSharded.env", env)


def one_lane_entries(tag, dof, ts, lim, rule):
    ltp = planner(dof, ts, lim, rule, 0)
    qg, q0, v0, a0 = amd.generate_queries(8, lim, seed=29)
    out = []
    for i in range(8):
        j = i % dof
        out.append([float(ltp.checkInputs(q0[i], v0[i], a0[i]))])
        ok, qb, t, d = ltp.optBraking(j, v0[i, j], a0[i, j])
        out.append([qb, d, *t])
        ok, t, d, m = ltp.optSwitchTimes(j, qg[i, j], q0[i, j], v0[i, j], a0[i, j], lim["v_max"][j])
        out.append([ok, d, m, *t])
        ok2, t2, vd, m2, case = ltp.timeScaling(j, qg[i, j], q0[i, j], v0[i, j], a0[i, j], d, float(np.sum(t)) * 1.5 + 0.1)
        out.append([ok2, vd, m2, case, *t2])
    emit(tag, "one_lane", np.array([x for row in out for x in row], dtype=np.float64))
    rng = np.random.default_rng(31)
    for dt, sizes in ((np.float64, (1000, 80000)), (np.float32, (1000, 150000))):      # arena / device-scratch branch (8 MiB)
        for n in sizes:
            emit(tag, f"roots.{np.dtype(dt).name}.n{n}", ltp.roots(rng.uniform(-2.0, 2.0, (n, 7)).astype(dt), dtype=dt))


def reader_entries(tag, dof, ts, lim, rule, n):
    import torch
    from horizon_checker import draw_starts
    from knots_checker import GRIDS
    ltp = planner(dof, ts, lim, rule, 0)
    q = [np.ascontiguousarray(x) for x in amd.generate_queries(n, lim, seed=37)]
    q[1][min(3, n - 1), 0] = 99.0                                # rejected by checkInputs: NaN rows, valid 0
    dev = "cuda:0"
    batch = ltp.planSwitchTimesBatch(*[torch.from_numpy(x).to(dev) for x in q])
    torch.cuda.synchronize()
    lens, t_scaled = batch.traj_len.cpu().numpy(), batch.t_scaled.cpu().numpy()
    rng = np.random.default_rng(41)
    N, s = 32, 3
    k_window, k_horizon = draw_starts(rng, lens, t_scaled, N, 1), draw_starts(rng, lens, t_scaled, N, s)
    grids = {name: GRIDS[name] for name in ("mpc", "duplicates", "one")}

    def rows(call, n_elements, dtype):
        out = torch.zeros((n, 4, dof, ltp.windowRowStride(n_elements)), dtype=dtype, device=dev)   # the row padding is not written
        r, v = call(out, torch.zeros((n,), dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        return {"rows": r.cpu().numpy(), "valid": v.cpu().numpy()}

    def env(call, m):
        r, v = call(torch.zeros((n, dof, m, 2), dtype=torch.float64, device=dev), torch.zeros((n,), dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        return {"env": r.cpu().numpy(), "valid": v.cpu().numpy()}

    for how, kw, kh in (("each", torch.from_numpy(k_window).to(dev), torch.from_numpy(k_horizon).to(dev)), ("uniform", 37, 37)):
        for dtype in (torch.float64, torch.float32):
            f = str(dtype).split(".")[1]
            emit(tag, f"sampleWindow.{how}.{f}", rows(lambda o, v: ltp.sampleWindow(batch, 0, n, kw, N, out=o, valid=v), N, dtype))
            emit(tag, f"sampleHorizon.{how}.{f}", rows(lambda o, v: ltp.sampleHorizon(batch, 0, n, kh, N, s, out=o, valid=v), N, dtype))
            for name, g in grids.items():
                emit(tag, f"sampleKnots.{name}.{how}.{f}", rows(lambda o, v: ltp.sampleKnots(batch, 0, n, kh, g, out=o, valid=v), len(g), dtype))
        for name in ("mpc", "duplicates"):                       # `one` has no interval
            for closed in (False, True):
                g = grids[name]
                emit(tag, f"envelopeKnots.{name}.{how}.{'closed' if closed else 'open'}",
                     env(lambda o, v: ltp.envelopeKnots(batch, 0, n, kh, g, closed=closed, out=o, valid=v), len(g) - 1))
    for how, kw, kh in (("each", k_window, k_horizon), ("uniform", 37, 37)):
        host = {"planWindowHost": ltp.planWindowHost(*q, kw, N), "planHorizonHost": ltp.planHorizonHost(*q, kh, N, s)}
        for name, g in grids.items():
            host[f"planKnotsHost.{name}"] = ltp.planKnotsHost(*q, kh, g)
        for name in ("mpc", "duplicates"):
            for closed in (False, True):
                host[f"planEnvelopeKnotsHost.{name}.{'closed' if closed else 'open'}"] = ltp.planEnvelopeKnotsHost(*q, kh, grids[name], closed=closed)
        for name, (rec, out, valid) in host.items():
            emit(tag, f"{name}.{how}.records", rec)
            emit(tag, f"{name}.{how}.out", out)
            emit(tag, f"{name}.{how}.valid", valid)


def main():
    for limits, ts in (("panda", 0.001), ("ref", 0.004), ("ref30", 0.002)):
        dof, lim = amd.limit_set(limits)
        sizes = tier_sizes(dof)
        print(f"# {limits}: dof {dof}, n per tier {sizes}")
        for rule in ("libm", "exact"):
            for tier, n in sizes.items():
                batch_entries(f"{limits}/{rule}/{tier}/n{n}", dof, ts, lim, rule, n, 0 if tier == "fused" else CAP)
            one_lane_entries(f"{limits}/{rule}", dof, ts, lim, rule)
            reader_entries(f"{limits}/{rule}/readers/n{READER_N[limits]}", dof, ts, lim, rule, READER_N[limits])


if __name__ == "__main__":
    main()
