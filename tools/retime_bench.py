"""Cost of ltp_retime_batch (include/ltp_hip.h) on one device: a 1 M x 7-DoF panda batch is planned once, then retimed in place to
k x T* (k = 1.5 and 10, through t_target) and to synchronised groups of 8 (each group at its slowest member's time). Every timed
iteration first restores the planned records (a device copy, outside the timed span), so each retime starts from the same batch.
Prints one JSON line per case: median / min milliseconds of the retime call (events around it on the current stream), how many
queries were retimed. Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel split (k_group_time, k_retime,
k_scaling_slow, k_finalize_lens, k_scan_*).

    python tools/retime_bench.py [--n 1000000] [--iters 20] [--pow libm|exact]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REC = ("t_scaled", "v_drive", "mod", "t_required", "traj_len", "status")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pow", default="libm", choices=("libm", "exact"))
    args = ap.parse_args()
    import torch
    from longtermplanner_amd import LongTermPlanner, limit_set

    dof, lim = limit_set("panda")
    ltp = LongTermPlanner(dof, 0.001, device=0, **lim)
    ltp.setPowRule(args.pow)
    n = args.n
    qg, q0, v0, a0 = ltp.generateQueries(n, seed=2026)
    batch = ltp.planSwitchTimesBatch(qg, q0, v0, a0)
    torch.cuda.synchronize()
    saved = {k: getattr(batch, k).clone() for k in REC}
    saved_off = batch.offsets.clone()
    ok = (batch.status == 0) & (batch.slowest >= 0)
    t_star = batch.t_opt[torch.arange(n, device=qg.device), batch.slowest.clamp(min=0).long(), 6]
    group = (torch.randperm(n, device=qg.device) // 8).to(torch.int32)
    cases = [("uniform k=1.5", dict(t_target=(1.5 * t_star).contiguous())),
             ("uniform k=10", dict(t_target=(10.0 * t_star).contiguous())),
             ("groups of 8", dict(group=group, n_groups=(n + 7) // 8))]
    for name, kw in cases:
        times = []
        for it in range(args.warmup + args.iters):
            for k in REC:
                getattr(batch, k).copy_(saved[k])
            batch.offsets.copy_(saved_off)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ltp.retimeBatch(batch, **kw)
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times.append(e0.elapsed_time(e1))
        retimed = int(((batch.t_required != saved["t_required"]) & ok).sum().item())
        print(json.dumps({"case": name, "n": n, "dof": dof, "pow_rule": args.pow, "retime_ms_median": round(float(np.median(times)), 4),
                          "retime_ms_min": round(float(np.min(times)), 4), "iters": args.iters, "retimed_queries": retimed,
                          "planned_queries": int(ok.sum().item())}), flush=True)


if __name__ == "__main__":
    main()
