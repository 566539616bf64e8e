"""Cost of ltp_envelope_knots_batch (include/ltp_hip.h) on one device, next to the ways a shield gets the same answer without it: a
1 M x 7-DoF panda batch is planned once; then, per grid and alternating in one process, each from k = 0 and from k uniform in
[0, traj_len) per plan,
  E     the horizon-envelope call on the grid's edges, closed = 1;
  A     ltp_sample_window_batch of g[M] + 1 samples of all four arrays (over as many of the plans as --dense-gb of buffer hold, scaled
        to the whole batch) plus a torch min / max reduction of its q rows per interval: the window call, the reduction, their sum;
  B     ltp_envelope_batch in analytic mode (k_envelope_walk) with the nearest uniform windows, M windows of round(g[M] / M) samples
        — from sample 0 of every plan, whatever k is: it cannot start anywhere else;
  C     ltp_sample_knots_batch on the same grid (the rows at the knots, not what lies between them).
Each launch is timed with device events on the current stream; after the warm-up every variant is launched --iters times. Prints a
table: median / min / max milliseconds per 1 M plans. Grids: mpc (40 edges to 240), geometric (59 edges to 4096).

    python tools/envelope_knots_bench.py [--n 1000000] [--iters 20] [--warmup 3] [--grids mpc geometric] [--out FILE]
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
    ap.add_argument("--dense-gb", type=float, default=24.0, help="largest buffer of the dense window the call is compared with")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from longtermplanner_amd import LongTermPlanner, limit_set

    dof, lim = limit_set("panda")
    n = args.n
    ltp = LongTermPlanner(dof, 0.001, device=0, **lim)
    ltp.setEnvelopeMode("analytic")
    ltp.setTablePass(0)
    qg, q0, v0, a0 = ltp.generateQueries(n, seed=2026)
    batch = ltp.planSwitchTimesBatch(qg, q0, v0, a0)
    torch.cuda.synchronize()
    dev = qg.device
    planned = int((batch.traj_len > 0).sum().item())
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    k_uniform = (torch.rand(n, device=dev, generator=gen, dtype=torch.float64) * batch.traj_len.clamp(min=1)).to(torch.int32)
    valid = torch.empty(n, dtype=torch.int32, device=dev)
    lines = [f"envelope_knots_bench: n = {n} x {dof}-DoF panda, planned {planned}, median traj_len {int(batch.traj_len.float().median().item())}, "
             f"iters {args.iters}, warm-up {args.warmup}, device {torch.cuda.get_device_name(0)}",
             f"{'grid':<10} {'M':>4} {'variant':<66} {'ms median':>10} {'ms min':>8} {'ms max':>8}"]
    for name in args.grids:
        g = named_grid(name)
        M, span = len(g) - 1, int(g[-1]) + 1
        grid = torch.from_numpy(g).to(dev)
        env = torch.empty((n, dof, M, 2), dtype=torch.float64, device=dev)
        rows = torch.empty((n, 4, dof, ltp.windowRowStride(M + 1)), dtype=torch.float64, device=dev)
        Rd = ltp.windowRowStride(span)
        nd = int(min(n, args.dense_gb * 1e9 // (32 * dof * Rd)))
        dense = torch.empty((nd, 4, dof, Rd), dtype=torch.float64, device=dev)
        red = torch.empty((nd, dof, M, 2), dtype=torch.float64, device=dev)
        lo_at = [int(x) for x in g[:-1]]
        hi_at = [int(max(a, b)) for a, b in zip(g[:-1], g[1:])]                 # closed = 1: the knot sample k + g[w + 1] included
        window = max(1, int(round(float(g[-1]) / M)))

        def reduce_rows():
            q = dense[:, 0]
            for w in range(M):
                piece = q[:, :, lo_at[w]:hi_at[w] + 1]
                torch.amin(piece, dim=2, out=red[:, :, w, 0])
                torch.amax(piece, dim=2, out=red[:, :, w, 1])

        variants = []
        for tag, k in (("k = 0", 0), ("k uniform", k_uniform)):
            variants += [(f"E horizon envelopes, closed = 1, {tag}", n, lambda k=k: ltp.envelopeKnots(batch, 0, n, k, grid, closed=True, out=env, valid=valid)),
                         (f"A dense window of {span} samples, {nd} plans, {tag}", nd, lambda k=k: ltp.sampleWindow(batch, 0, nd, k, span, out=dense, valid=valid)),
                         (f"A torch min / max of its q rows per interval, {nd} plans", nd, reduce_rows),
                         (f"B envelopeBatch {M} windows of {window} from sample 0 (analytic walk)", n, lambda: ltp.envelopeBatch(batch, 0, n, window, M, out=env)),
                         (f"C knots call on the same grid, {tag}", n, lambda k=k: ltp.sampleKnots(batch, 0, n, k, grid, out=rows, valid=valid))]
        times = [[] for _ in variants]
        for it in range(args.warmup + args.iters):
            for v, (_, _, fn) in enumerate(variants):
                ms = timed(fn)
                if it >= args.warmup:
                    times[v].append(ms)
        scaled = [np.array(times[v]) * 1.0e6 / variants[v][1] for v in range(len(variants))]      # ms per 1 M plans
        for v, (what, _, _) in enumerate(variants):
            t = scaled[v]
            lines.append(f"{name:<10} {M:>4} {what:<66} {np.median(t):>10.3f} {t.min():>8.3f} {t.max():>8.3f}")
        per = len(variants) // 2
        for tag, at in (("k = 0", 0), ("k uniform", per)):
            e, a, b = float(np.median(scaled[at])), float(np.median(scaled[at + 1]) + np.median(scaled[at + 2])), float(np.median(scaled[at + 3]))
            lines.append(f"{name:<10} {M:>4} {tag}: E {e:.3f} ms; A window + reduction {a:.3f} ms ({a / e:.1f} x E); B {b:.3f} ms ({b / e:.2f} x E)")
        del env, rows, dense, red
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
