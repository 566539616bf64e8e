"""Latency of the single-call (host pointer) entry points: latency_probe.py [calls] [batch_calls].

`calls` (default 64) timed calls per line — choose it so that a line's window lasts a second or more (25 000 for the ~40 us
lines); `batch_calls` (default 0 = skip) timed planBatchHost(sample=True) calls at an arena-tier and a staged-tier size
(ltp_capi_host.hip), rows capped at 16 samples."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import longtermplanner_amd as amd
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 64
batch_calls = int(sys.argv[2]) if len(sys.argv) > 2 else 0
D, lim = amd.limit_set("panda")
ltp = amd.LongTermPlanner(D, 0.001, device=0, **lim)
qg, q0, v0, a0 = amd.generate_queries(64, lim, seed=3)
traj = amd.Trajectory()
lines = [("planTrajectory (7-DoF, ~1700 samples)", calls, lambda i: ltp.planTrajectory(qg[i], q0[i], v0[i], a0[i], traj)),
         ("planBatchHost n=1 switch-only", calls, lambda i: ltp.planBatchHost(qg[i], q0[i], v0[i], a0[i], sample=False)),
         ("checkInputs", calls, lambda i: ltp.checkInputs(q0[i], v0[i], a0[i])),
         ("optSwitchTimes", calls, lambda i: ltp.optSwitchTimes(0, qg[i, 0], q0[i, 0], v0[i, 0], a0[i, 0], lim["v_max"][0]))]
if batch_calls:
    capped = amd.LongTermPlanner(D, 0.001, device=0, **lim)
    capped.setMaxSamples(16)
    for n in (2000, 9000):
        q = amd.generate_queries(n, lim, seed=3)
        lines.append((f"planBatchHost n={n} rows (cap 16)", batch_calls, lambda i, q=q: capped.planBatchHost(*q, sample=True)))
for name, count, fn in lines:
    for i in range(5): fn(i)
    t0 = time.perf_counter()
    for i in range(count): fn(i % 64)
    print(f"{name:45s} {(time.perf_counter() - t0) / count * 1e6:9.1f} us per call")
