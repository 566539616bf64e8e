"""Cost of ltp_plan_stop_batch (include/ltp_hip.h) on one device: 1 M x 7-DoF panda start states from generateQueries, planned to
standstill with and without q_stop, and — in the same process, on the same batch — ltp_plan_switch_times_batch, the entry a
stop plan stands next to (no solver and no queue on the stop side). Prints one JSON line per case: median / min milliseconds of the
call (events around it on the current stream: k_stop plus the three scan kernels) and the achieved GB/s against the algorithmic
bytes: per (query, joint) 24 B read and 56 + 56 + 8 + 8 + 1 B written (+ 8 B with q_stop), per query 20 B of records and 8 B of
offsets. Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel split (k_stop, k_finalize_lens, k_scan_*).

    python tools/stop_bench.py [--n 1000000] [--iters 20] [--pow libm|exact] [--check inputs|braking]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pow", default="libm", choices=("libm", "exact"))
    ap.add_argument("--check", default="inputs", choices=("inputs", "braking"))
    args = ap.parse_args()
    import torch
    from longtermplanner_amd import LongTermPlanner, _abi, limit_set

    dof, lim = limit_set("panda")
    ltp = LongTermPlanner(dof, 0.001, device=0, **lim)
    ltp.setPowRule(args.pow)
    n = args.n
    qg, q0, v0, a0 = ltp.generateQueries(n, seed=2026)
    stop = ltp.planStopBatch(q0, v0, a0, check=args.check)
    plain = ltp.planSwitchTimesBatch(qg, q0, v0, a0)
    torch.cuda.synchronize()

    def raw_stop(q_stop):
        o = _abi.StopOpts(C.sizeof(_abi.StopOpts), _abi.STOP_CHECKS[args.check], q_stop)
        rec = stop.c_records()
        ltp._bind(stop)
        ltp._check(ltp._lib.ltp_plan_stop_batch(ltp._h, n, C.byref(stop.queries), C.byref(rec), C.addressof(o), stop.offsets.data_ptr(),
                                                ltp._stream()))

    lane = 24 + 56 + 56 + 8 + 8 + 1
    cases = [("ltp_plan_stop_batch with q_stop", lambda: raw_stop(stop.q_stop.data_ptr()), n * (dof * (lane + 8) + 28)),
             ("ltp_plan_stop_batch without q_stop", lambda: raw_stop(None), n * (dof * lane + 28)),
             ("ltp_plan_switch_times_batch", lambda: ltp.planSwitchTimesBatch(qg, q0, v0, a0, batch=plain), None)]
    for name, call, nbytes in cases:
        times = []
        for it in range(args.warmup + args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times.append(e0.elapsed_time(e1))
        med = float(np.median(times))
        line = {"case": name, "n": n, "dof": dof, "pow_rule": args.pow, "ms_median": round(med, 4), "ms_min": round(float(np.min(times)), 4),
                "iters": args.iters}
        if nbytes is not None:
            line.update(check=args.check, algorithmic_bytes=nbytes, gb_per_s_median=round(nbytes / med / 1e6, 1),
                        planned=int((stop.status == 0).sum().item()))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
