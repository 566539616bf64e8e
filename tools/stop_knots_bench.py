"""Cost of ltp_stop_knots_batch (include/ltp_hip.h) on one device, next to the composition of merged calls that gives the same
answer: a 1 M x 7-DoF panda batch is planned once per pow rule; then, per grid and alternating in one process, each from k = 0 and
from k uniform in [0, traj_len) per plan,
  a     the stop-horizon call (clamp mode): [n, 2, dof, R] doubles;
  b     the composition: ltp_sample_knots_batch, a permute to [n * N, dof] states, torch.clamp of the accelerations, ONE
        ltp_plan_stop_batch(check = braking) over n * N states — in chunks of --chunk plans (the stop batch of all n * N states
        holds 137 bytes of records per state and joint), the chunks' times summed;
  c     ltp_sample_knots_batch on the same grid (the states at the knots: twice the bytes of a, none of its arithmetic).
Each launch (for b: each chunk, all of its calls) is timed with device events on the current stream; after the warm-up every
variant is launched --iters times. Prints a table: median / min / max milliseconds per 1 M plans, then per (grid, start) the
condition "median of a below the minimum of b" and the ratio a / c. Grids: mpc (40 knots to 240), geometric (59 knots to 4096).

    python tools/stop_knots_bench.py [--n 1000000] [--iters 20] [--warmup 3] [--grids mpc geometric] [--pow libm exact] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from window_bench import named_grid, timed   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--grids", nargs="+", default=["mpc", "geometric"], metavar="NAME")
    ap.add_argument("--pow", nargs="+", default=["libm", "exact"], choices=["libm", "exact"])
    ap.add_argument("--chunk", type=int, default=100_000, help="plans per chunk of the composition")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from longtermplanner_amd import LongTermPlanner, limit_set

    dof, lim = limit_set("panda")
    n = args.n
    chunk = min(args.chunk, n)
    lines = []
    for pow_rule in args.pow:
        ltp = LongTermPlanner(dof, 0.001, device=0, **lim)
        ltp.setPowRule(pow_rule)
        qg, q0, v0, a0 = ltp.generateQueries(n, seed=2026)
        batch = ltp.planSwitchTimesBatch(qg, q0, v0, a0)
        torch.cuda.synchronize()
        dev = qg.device
        planned = int((batch.traj_len > 0).sum().item())
        gen = torch.Generator(device=dev)
        gen.manual_seed(9)
        k_uniform = (torch.rand(n, device=dev, generator=gen, dtype=torch.float64) * batch.traj_len.clamp(min=1)).to(torch.int32)
        valid = torch.empty(n, dtype=torch.int32, device=dev)
        am = torch.as_tensor(lim["a_max"], dtype=torch.float64, device=dev)
        lines += [f"stop_knots_bench: pow rule {pow_rule}, n = {n} x {dof}-DoF panda, planned {planned}, median traj_len "
                  f"{int(batch.traj_len.float().median().item())}, iters {args.iters}, warm-up {args.warmup}, chunk {chunk}, device {torch.cuda.get_device_name(0)}",
                  f"{'grid':<10} {'N':>4} {'variant':<58} {'ms median':>10} {'ms min':>8} {'ms max':>8}"]
        for name in args.grids:
            g = named_grid(name)
            N = len(g)
            R = ltp.windowRowStride(N)
            grid = torch.from_numpy(g).to(dev)
            out = torch.empty((n, 2, dof, R), dtype=torch.float64, device=dev)
            rows = torch.empty((n, 4, dof, R), dtype=torch.float64, device=dev)
            crow = torch.empty((chunk, 4, dof, R), dtype=torch.float64, device=dev)
            state = {"stop": None}

            def composed(k):
                """The chunks' device times, summed (ms)."""
                total = 0.0
                for first in range(0, n, chunk):
                    count = min(chunk, n - first)
                    kk = k if isinstance(k, int) else k[first:first + count]

                    def one():
                        r, _ = ltp.sampleKnots(batch, first, count, kk, grid, out=crow[:count], valid=valid[:count])
                        st = r[..., :N].permute(1, 0, 3, 2).reshape(4, count * N, dof)
                        q, v, a = (st[x].contiguous() for x in range(3))
                        state["stop"] = ltp.planStopBatch(q, v, torch.clamp(a, min=-am, max=am), check="braking", batch=state["stop"])
                    total += timed(one)
                return total

            variants = []
            for tag, k in (("k = 0", 0), ("k uniform", k_uniform)):
                variants += [(f"a stop horizons, clamp, {tag}", lambda k=k: timed(lambda: ltp.stopKnots(batch, 0, n, k, grid, out=out, valid=valid))),
                             (f"b knots + permute + clamp + stop batch of n * N states, {tag}", lambda k=k: composed(k)),
                             (f"c knots call on the same grid, {tag}", lambda k=k: timed(lambda: ltp.sampleKnots(batch, 0, n, k, grid, out=rows, valid=valid)))]
            times = [[] for _ in variants]
            for it in range(args.warmup + args.iters):
                for v, (_, fn) in enumerate(variants):
                    ms = fn()
                    if it >= args.warmup:
                        times[v].append(ms)
            scaled = [np.array(t) * 1.0e6 / n for t in times]      # ms per 1 M plans
            for v, (what, _) in enumerate(variants):
                t = scaled[v]
                lines.append(f"{name:<10} {N:>4} {what:<58} {np.median(t):>10.3f} {t.min():>8.3f} {t.max():>8.3f}")
            for tag, at in (("k = 0", 0), ("k uniform", 3)):
                a, b_min, c = float(np.median(scaled[at])), float(scaled[at + 1].min()), float(np.median(scaled[at + 2]))
                lines.append(f"{name:<10} {N:>4} {tag}: a median {a:.3f} ms {'<' if a < b_min else '>='} b minimum {b_min:.3f} ms ({b_min / a:.1f} x a); "
                             f"a / c = {a / c:.2f} (c median {c:.3f} ms)")
            del out, rows, crow
            state["stop"] = None
            torch.cuda.empty_cache()
        del batch, ltp
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
