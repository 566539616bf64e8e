"""Cost of ltp_envelope_knots_arrays_batch (include/ltp_hip.h) on one device: a 1 M x 7-DoF panda batch is planned once; then, on
the 40-edge MPC grid (39 intervals over 240 samples), closed = 1, k uniform in [0, traj_len) per plan, alternating in one process,
  A1, A3, A7, A15  the arrays call with the masks q, q|v, q|v|a and q|v|a|j;
  E                ltp_envelope_knots_batch (the q-only kernel the new one stands next to), to hold A1 against;
  W + R            the composed alternative to A15: ltp_sample_window_batch of g[M] + 1 samples of all four arrays (over as many of
                   the plans as --dense-gb of buffer hold, scaled to the whole batch) plus a torch min / max reduction of its rows per
                   interval (the window already holds the last position and the zeros past the end).
Each launch is timed with device events on the current stream; after the warm-up every variant is launched --iters times. Prints
median / min / max milliseconds per --n plans and the bytes each call stores per second, then the share of v pairs (and q pairs)
that are bit-identical to the exhaustive reduction of the window rows over the plans the dense buffer holds.

    python tools/envelope_arrays_bench.py [--n 1000000] [--iters 10] [--warmup 2] [--dense-gb 24] [--out FILE]
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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dense-gb", type=float, default=24.0, help="largest buffer of the dense window the call is compared with")
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
    dev = qg.device
    planned = int((batch.traj_len > 0).sum().item())
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    k = (torch.rand(n, device=dev, generator=gen, dtype=torch.float64) * batch.traj_len.clamp(min=1)).to(torch.int32)
    valid = torch.empty(n, dtype=torch.int32, device=dev)
    g = named_grid("mpc")
    M, span = len(g) - 1, int(g[-1]) + 1
    grid = torch.from_numpy(g).to(dev)
    env = torch.empty((n, 4, dof, M, 2), dtype=torch.float64, device=dev)
    Rd = ltp.windowRowStride(span)
    nd = int(min(n, args.dense_gb * 1e9 // (32 * dof * Rd)))
    dense = torch.empty((nd, 4, dof, Rd), dtype=torch.float64, device=dev)
    red = torch.empty((nd, 4, dof, M, 2), dtype=torch.float64, device=dev)
    lo_at = [int(x) for x in g[:-1]]
    hi_at = [int(max(a, b)) for a, b in zip(g[:-1], g[1:])]                 # closed = 1: the knot sample k + g[w + 1] included

    def reduce_rows():
        for w in range(M):
            piece = dense[:, :, :, lo_at[w]:hi_at[w] + 1]
            torch.amin(piece, dim=3, out=red[:, :, :, w, 0])
            torch.amax(piece, dim=3, out=red[:, :, :, w, 1])

    pair_bytes = n * dof * M * 16
    variants = [(f"A{mask:<2} arrays call, mask {mask} ({bin(mask).count('1')} arrays)", n, bin(mask).count("1") * pair_bytes,
                 lambda mask=mask: ltp.envelopeKnotsArrays(batch, 0, n, k, grid, arrays=mask, closed=True,
                                                           out=env.view(-1)[:n * bin(mask).count("1") * dof * M * 2], valid=valid))
                for mask in (1, 3, 7, 15)]
    variants += [("E   envelopeKnots (q only, the existing kernel)", n, pair_bytes,
                  lambda: ltp.envelopeKnots(batch, 0, n, k, grid, closed=True, out=env.view(-1)[:n * dof * M * 2].view(n, dof, M, 2), valid=valid)),
                 (f"W   dense window of {span} samples, four arrays, {nd} plans", nd, nd * 4 * dof * Rd * 8,
                  lambda: ltp.sampleWindow(batch, 0, nd, k[:nd].contiguous(), span, out=dense, valid=valid[:nd])),
                 (f"R   torch min / max of its rows per interval, {nd} plans", nd, nd * 4 * dof * M * 16, reduce_rows)]
    times = [[] for _ in variants]
    for it in range(args.warmup + args.iters):
        for v, (_, _, _, fn) in enumerate(variants):
            ms = timed(fn)
            if it >= args.warmup:
                times[v].append(ms)
    lines = [f"envelope_arrays_bench: n = {n} x {dof}-DoF panda, planned {planned}, median traj_len {int(batch.traj_len.float().median().item())}, "
             f"grid mpc (M = {M}), closed = 1, k uniform, iters {args.iters}, warm-up {args.warmup}, device {torch.cuda.get_device_name(0)}",
             f"{'variant':<62} {'ms median':>10} {'ms min':>8} {'ms max':>8} {'GB stored':>10} {'GB/s':>8}"]
    med = []
    for v, (what, plans, nbytes, _) in enumerate(variants):
        t = np.array(times[v])
        scaled = t * float(n) / plans                                       # ms per n plans
        med.append(float(np.median(scaled)))
        lines.append(f"{what:<62} {np.median(scaled):>10.3f} {scaled.min():>8.3f} {scaled.max():>8.3f} {nbytes / 1e9:>10.3f} "
                     f"{nbytes / 1e6 / float(np.median(t)):>8.1f}")
    lines.append(f"A1 / E = {med[0] / med[4]:.3f}; composed W + R = {med[5] + med[6]:.3f} ms per {n} plans = {(med[5] + med[6]) / med[3]:.1f} x A15")
    # the shares of bit-identical pairs against the exhaustive reduction, over the plans the dense buffer holds
    ltp.sampleWindow(batch, 0, nd, k[:nd].contiguous(), span, out=dense, valid=valid[:nd])
    reduce_rows()
    got, _ = ltp.envelopeKnotsArrays(batch, 0, nd, k[:nd].contiguous(), grid, arrays=15, closed=True)
    torch.cuda.synchronize()
    real = ~torch.isnan(red)
    for x, name in enumerate("qvaj"):
        same = (got[:, x].contiguous().view(torch.int64) == red[:, x].contiguous().view(torch.int64)) & real[:, x]
        equal = (got[:, x] == red[:, x]) & real[:, x]
        d = torch.nan_to_num((got[:, x] - red[:, x]).abs(), nan=0.0)
        cnt = max(int(real[:, x].sum().item()), 1)
        lines.append(f"{name}: bit-identical to the exhaustive reduction {int(same.sum().item()) / cnt:.6f}, equal {int(equal.sum().item()) / cnt:.6f}, "
                     f"worst |d| {float(d.max().item()):.3e} ({nd} plans)")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
