"""Cost of limit sets (ltp_set_limit_sets / ltp_bind_limit_sets, include/ltp_hip.h) on one device: a 1 M x 7-DoF batch with
panda-derived limits, four lines — switching times plus the end-limit verdict, full rows at the headline shape (the first
--rows plans, whole trajectories), first-32 rows, ltp_state_at_batch — each in four cases: unbound, K = 1 (every index 0),
K = 8 (panda with v / a / j scaled 1.0 ... 0.3) and K = n (one random set per query, v / a / j scaled 0.3 ... 1.0). The
queries are generated for the slowest set of each case, so that every query passes checkInputs in every case.
Prints one JSON line per (line, case): median / min milliseconds (events around the call on the current stream), and the host
wall time of one in-place ltp_set_limit_sets per case. Run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel split.

    python tools/limit_sets_bench.py [--n 1000000] [--iters 10] [--rows 20000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIM = ("q_min", "q_max", "v_max", "a_max", "j_max")


def _time(fn, warmup, iters):
    import torch
    times = []
    for it in range(warmup + iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            times.append(e0.elapsed_time(e1))
    return round(float(np.median(times)), 4), round(float(np.min(times)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=20000, help="plans whose whole trajectories the full-rows line writes")
    args = ap.parse_args()
    import torch
    from longtermplanner_amd import LongTermPlanner, limit_set

    dof, panda = limit_set("panda")
    n = args.n
    dev = "cuda:0"
    rng = np.random.default_rng(2026)
    scale_k8 = np.linspace(1.0, 0.3, 8)
    scale_kn = rng.uniform(0.3, 1.0, n)

    def sets_of(scales):
        return [np.ascontiguousarray(np.outer(scales if k in ("v_max", "a_max", "j_max") else np.ones(len(scales)), panda[k]))
                for k in LIM]

    cases = [("unbound", None, None), ("K=1", sets_of(np.ones(1)), np.zeros(n, np.int32)),
             ("K=8", sets_of(scale_k8), rng.integers(0, 8, n).astype(np.int32)),
             ("K=n", sets_of(scale_kn), np.arange(n, dtype=np.int32))]
    # queries valid under the slowest set of any case (0.3 x panda's v / a / j)
    gen_lim = dict(panda, **{k: [0.3 * x for x in panda[k]] for k in ("v_max", "a_max", "j_max")})
    gen = LongTermPlanner(dof, 0.001, device=0, **gen_lim)
    qg, q0, v0, a0 = gen.generateQueries(n, seed=2026)
    for name, sets, idx in cases:
        ltp = LongTermPlanner(dof, 0.001, device=0, **panda)
        ix = None
        set_ms = None
        if sets is not None:
            ltp.setLimitSets(*sets)                 # first call: allocates the table
            t0 = time.perf_counter()
            ltp.setLimitSets(*sets)                 # in place: upload + the powers of the limits under both pow rules
            set_ms = round((time.perf_counter() - t0) * 1e3, 3)
            ix = torch.from_numpy(idx).to(dev)
        holder = {}

        def plan():
            holder["b"] = ltp.planSwitchTimesBatch(qg, q0, v0, a0, batch=holder.get("b"), end_limit=True, limit_set=ix)
        lines = {"switch_times+end_limit": _time(plan, args.warmup, args.iters)}
        b = holder["b"]
        torch.cuda.synchronize()
        m = min(args.rows, n)
        total = int(b.offsets[m].item())
        tile = torch.empty(max(total, 2), dtype=torch.float64, device=dev)
        lines[f"rows_whole_first_{m}"] = _time(lambda: ltp.sampleBatch(b, 0, m, tile), args.warmup, args.iters)
        lines["state_at"] = _time(lambda: ltp.stateAt(b, 0, n, 500), args.warmup, args.iters)
        ltp.setMaxSamples(32)
        plan()
        b = holder["b"]
        torch.cuda.synchronize()
        tile32 = torch.empty(max(int(b.offsets[n].item()), 2), dtype=torch.float64, device=dev)
        lines["rows_first_32"] = _time(lambda: ltp.sampleBatch(b, 0, n, tile32), args.warmup, args.iters)
        planned = int((b.status == 0).sum().item())
        if set_ms is not None:
            print(json.dumps({"line": "ltp_set_limit_sets", "case": name, "n_sets": int(sets[0].shape[0]), "dof": dof, "ms": set_ms}), flush=True)
        for line, (med, mn) in lines.items():
            print(json.dumps({"line": line, "case": name, "n": n, "dof": dof, "ms_median": med, "ms_min": mn, "iters": args.iters,
                              "planned_queries": planned}), flush=True)
        del tile, tile32, holder


if __name__ == "__main__":
    main()
