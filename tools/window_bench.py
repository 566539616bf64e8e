"""Cost of ltp_sample_window_batch (include/ltp_hip.h) on one device, next to the existing capped sampler: a 1 M x 7-DoF panda batch
is planned once; then, per N in {32, 64, 128} and alternating in one process,
  A(a)  the window call, float64, k = 0 for every plan;
  A(b)  the window call, float64, k uniform in [0, traj_len) per plan;
  B     the capped sampler at max_samples = N (sampleBatchEx, verdict=False) on the same queries planned by a second handle with that
        cap, with the offsets that plan's scan produced (the scan itself is part of planning and not in the timed span).
Each launch is timed with device events on the current stream; after the warm-up every variant is launched --iters times. Prints a
table: median / min milliseconds per 1 M plans, and for the window call the bytes it writes (32 * dof * N per planned plan) over the
median time as a share of the 8 TB/s HBM peak.

With --stride N:s [N:s ...] the tool measures the strided horizon call (ltp_sample_horizon_batch) instead: per pair, alternating in
one process, the horizon of N elements s samples apart, the dense window of N * s samples that holds the same samples (the only way
to get them without the call), and the dense window of N samples (stride 1), each from k = 0 and from k uniform in [0, traj_len).

With --knots NAME [NAME ...] it measures the knot-grid call (ltp_sample_knots_batch) on named grids: per grid, alternating in one
process, the knots call, the dense window of g[N-1] + 1 samples that holds the same samples (over as many of the plans as
--dense-gb of buffer hold, scaled to the whole batch) and, for the uniform grids uNxS (g[w] = w * S), the strided horizon call that
writes the same buffer — each from k = 0 and from k uniform in [0, traj_len). Grids: mpc (16 knots 1 apart, 12 four apart, 12
sixteen apart: 40 knots to 240), geometric (59 knots to 4096), u32x10, u64x5.

    python tools/window_bench.py [--n 1000000] [--iters 20] [--warmup 3] [--stride 32:4 32:10 64:5] [--knots mpc geometric] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stride_table(args, ltp, batch, n, dof, planned, k_uniform, valid):
    """The horizon call against the dense windows that hold the same samples; returns the lines of the table."""
    import torch
    dev = valid.device
    lines = [f"window_bench --stride: n = {n} x {dof}-DoF panda, planned {planned}, iters {args.iters}, warm-up {args.warmup}, device {torch.cuda.get_device_name(0)}",
             f"{'N':>4} {'s':>3} {'variant':<44} {'ms median':>10} {'ms min':>8} {'ms max':>8} {'GB written':>11}"]
    for pair in args.stride:
        N, s = (int(x) for x in pair.split(":"))
        hor = torch.empty((n, 4, dof, ltp.windowRowStride(N)), dtype=torch.float64, device=dev)
        dense = torch.empty((n, 4, dof, ltp.windowRowStride(N * s)), dtype=torch.float64, device=dev)
        variants = []
        for tag, k in (("k = 0", 0), ("k uniform", k_uniform)):
            variants += [(f"H horizon N = {N}, s = {s}, {tag}", N, lambda k=k: ltp.sampleHorizon(batch, 0, n, k, N, s, out=hor, valid=valid)),
                         (f"D dense window of N * s = {N * s}, {tag}", N * s, lambda k=k: ltp.sampleWindow(batch, 0, n, k, N * s, out=dense, valid=valid)),
                         (f"W dense window of N = {N} (stride 1), {tag}", N, lambda k=k: ltp.sampleWindow(batch, 0, n, k, N, out=hor, valid=valid))]
        times = [[] for _ in variants]
        for it in range(args.warmup + args.iters):
            for v, (_, _, fn) in enumerate(variants):
                ms = timed(fn)
                if it >= args.warmup:
                    times[v].append(ms)
        scale = 1.0e6 / n
        for v, (name, elements, _) in enumerate(variants):
            t = np.array(times[v]) * scale
            lines.append(f"{N:>4} {s:>3} {name:<44} {np.median(t):>10.3f} {t.min():>8.3f} {t.max():>8.3f} {32.0 * dof * elements * planned / 1e9:>11.2f}")
        for tag, h, d in (("k = 0", 0, 1), ("k uniform", 3, 4)):
            med, lo = float(np.median(times[h])) * scale, float(np.min(times[d])) * scale
            lines.append(f"{N:>4} {s:>3} criterion, {tag}: horizon median {med:.3f} ms {'<' if med < lo else '>='} dense window minimum {lo:.3f} ms: {'met' if med < lo else 'NOT met'}")
        del hor, dense
    return lines


def named_grid(name):
    if name == "mpc":
        return np.array(list(range(16)) + [16 + 4 * i for i in range(12)] + [64 + 16 * i for i in range(12)], dtype=np.int32)
    if name == "geometric":
        return np.unique(np.floor(np.concatenate([[0.0], np.geomspace(1.0, 4096.0, 69)])).astype(np.int64)).astype(np.int32)
    if name.startswith("u") and "x" in name:
        N, s = (int(x) for x in name[1:].split("x"))
        return (np.arange(N) * s).astype(np.int32)
    raise SystemExit(f"unknown grid {name}: mpc, geometric or uNxS")


def knots_table(args, ltp, batch, n, dof, planned, k_uniform, valid):
    """The knots call against the dense window that holds the same samples and, on uniform grids, the strided call."""
    import torch
    dev = valid.device
    lines = [f"window_bench --knots: n = {n} x {dof}-DoF panda, planned {planned}, iters {args.iters}, warm-up {args.warmup}, device {torch.cuda.get_device_name(0)}",
             f"{'grid':<10} {'N':>4} {'variant':<52} {'ms median':>10} {'ms min':>8} {'ms max':>8}"]
    for name in args.knots:
        g = named_grid(name)
        N, span = len(g), int(g[-1]) + 1
        grid = torch.from_numpy(g).to(dev)
        out = torch.empty((n, 4, dof, ltp.windowRowStride(N)), dtype=torch.float64, device=dev)
        Rd = ltp.windowRowStride(span)
        nd = int(min(n, args.dense_gb * 1e9 // (32 * dof * Rd)))        # plans the dense window's buffer may hold
        dense = torch.empty((nd, 4, dof, Rd), dtype=torch.float64, device=dev)
        uniform = name.startswith("u")
        s = int(g[1] - g[0]) if uniform and N > 1 else 1
        variants = []
        for tag, k in (("k = 0", 0), ("k uniform", k_uniform)):
            variants += [(f"K knots, {tag}", n, lambda k=k: ltp.sampleKnots(batch, 0, n, k, grid, out=out, valid=valid)),
                         (f"D dense window of {span} samples, {nd} plans, {tag}", nd, lambda k=k: ltp.sampleWindow(batch, 0, nd, k, span, out=dense, valid=valid))]
            if uniform:
                variants.append((f"H strided horizon N = {N}, s = {s}, {tag}", n, lambda k=k: ltp.sampleHorizon(batch, 0, n, k, N, s, out=out, valid=valid)))
        times = [[] for _ in variants]
        for it in range(args.warmup + args.iters):
            for v, (_, _, fn) in enumerate(variants):
                ms = timed(fn)
                if it >= args.warmup:
                    times[v].append(ms)
        per = len(variants) // 2
        scaled = [np.array(times[v]) * 1.0e6 / variants[v][1] for v in range(len(variants))]      # ms per 1 M plans
        for v, (what, _, _) in enumerate(variants):
            t = scaled[v]
            lines.append(f"{name:<10} {N:>4} {what:<52} {np.median(t):>10.3f} {t.min():>8.3f} {t.max():>8.3f}")
        for tag, at in (("k = 0", 0), ("k uniform", per)):
            med, lo = float(np.median(scaled[at])), float(scaled[at + 1].min())
            lines.append(f"{name:<10} {N:>4} criterion, {tag}: knots median {med:.3f} ms {'<' if med < lo else '>='} dense window minimum {lo:.3f} ms: {'met' if med < lo else 'NOT met'}")
            if uniform:
                h = float(np.median(scaled[at + 2]))
                lines.append(f"{name:<10} {N:>4} search, {tag}: knots median {med:.3f} ms / strided median {h:.3f} ms = {med / h:.3f}")
        del out, dense
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stride", nargs="+", default=None, metavar="N:s", help="measure the strided horizon call at these (N, s) pairs instead")
    ap.add_argument("--knots", nargs="+", default=None, metavar="NAME", help="measure the knot-grid call on these named grids instead")
    ap.add_argument("--dense-gb", type=float, default=48.0, help="--knots: largest buffer of the dense window it is compared with")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from longtermplanner_amd import LongTermPlanner, limit_set

    dof, lim = limit_set("panda")
    n = args.n
    ltp = LongTermPlanner(dof, 0.001, device=0, **lim)
    qg, q0, v0, a0 = ltp.generateQueries(n, seed=2026)
    batch = ltp.planSwitchTimesBatch(qg, q0, v0, a0)
    torch.cuda.synchronize()
    planned = int((batch.traj_len > 0).sum().item())
    gen = torch.Generator(device=qg.device)
    gen.manual_seed(9)
    k_uniform = (torch.rand(n, device=qg.device, generator=gen, dtype=torch.float64) * batch.traj_len.clamp(min=1)).to(torch.int32)
    valid = torch.empty(n, dtype=torch.int32, device=qg.device)
    if args.stride or args.knots:
        text = "\n".join((knots_table if args.knots else stride_table)(args, ltp, batch, n, dof, planned, k_uniform, valid))
        print(text, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    lines = [f"window_bench: n = {n} x {dof}-DoF panda, planned {planned}, iters {args.iters}, warm-up {args.warmup}, device {torch.cuda.get_device_name(0)}",
             f"{'N':>4} {'variant':<38} {'ms median':>10} {'ms min':>8} {'GB written':>11} {'share of 8 TB/s':>16}"]
    for N in (32, 64, 128):
        R = ltp.windowRowStride(N)
        win = torch.empty((n, 4, dof, R), dtype=torch.float64, device=qg.device)
        cap = LongTermPlanner(dof, 0.001, device=0, **lim)
        cap.setMaxSamples(N)
        cbatch = cap.planSwitchTimesBatch(qg, q0, v0, a0)
        rows = torch.empty(int(cbatch.offsets[n].item()), dtype=torch.float64, device=qg.device)
        variants = [("A(a) window, k = 0", lambda: ltp.sampleWindow(batch, 0, n, 0, N, out=win, valid=valid)),
                    ("A(b) window, k uniform in [0, len)", lambda: ltp.sampleWindow(batch, 0, n, k_uniform, N, out=win, valid=valid)),
                    ("B    capped sampler, no offsets scan", lambda: cap.sampleBatchEx(cbatch, 0, n, rows, verdict=False))]
        times = [[] for _ in variants]
        for it in range(args.warmup + args.iters):
            for v, (_, fn) in enumerate(variants):
                ms = timed(fn)
                if it >= args.warmup:
                    times[v].append(ms)
        kernel = cap.lastSamplerKernel()
        for v, (name, _) in enumerate(variants):
            med, lo = float(np.median(times[v])), float(np.min(times[v]))
            scale = 1.0e6 / n
            if v < 2:
                written = 32.0 * dof * N * planned
                lines.append(f"{N:>4} {name:<38} {med * scale:>10.3f} {lo * scale:>8.3f} {written / 1e9:>11.2f} {100.0 * written / (med * 1e-3) / PEAK:>15.1f}%")
            else:
                lines.append(f"{N:>4} {name + ' (' + kernel + ')':<38} {med * scale:>10.3f} {lo * scale:>8.3f}")
        del win, rows, cbatch, cap
    lines.append("B times sampleBatchEx(verdict=False) at max_samples = N alone: the offsets scan its rows need (part of planning that batch) is NOT in")
    lines.append("the timed span, while the window call needs no scan at all: B is a lower bound of the capped path, not a like-for-like total.")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
