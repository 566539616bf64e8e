"""Cost of ltp_first_exit_batch (include/ltp_hip.h) on one device: a 1 M x 7-DoF panda batch is planned once; then, alternating in
one process, for the masks q, qv and qvaj, the horizons 240 and 2^30, k = 0 and k uniform in [0, traj_len) per plan, and two kinds
of boxes —
  inside    one box per joint (stride 0) that no plan leaves: every stretch passes the quick reject, the bulk path;
  fraction  per (plan, array, joint) lo = min + u1 (max - min), hi = max - u2 (max - min) of the row's own range over the whole plan,
            u uniform in (0.05, 0.45): nearly every lane bisects —
  F         the call;
  E         ltp_envelope_knots_arrays_batch with ONE interval [0, horizon) and the same mask from the same k: the walk the call's cost
            is expected to be that of (a figure, not a gate);
  Y         the composition the call replaces, on as many plans as its buffer holds, scaled to the whole batch. H = 240:
            ltp_sample_window_batch of 240 samples of all four arrays (the window call has no array subset) plus the torch reduction
            to the first index outside the box (compare, any, argmax over the selected arrays). H = 2^30: the full sampler's rows
            (ltp_sample_batch from sample 0, k = 0 only) plus the torch reduction over the packed rows (gather of each element's box,
            compare, scatter-amin of the sample index; the element -> row and element -> sample maps are built once, untimed).
Each launch is timed with device events on the current stream; after the warm-up every variant is launched --iters times. Prints
median / min / max milliseconds per --n plans, then per line whether the call's median lies below the composition's minimum, and
the number of (plan, array, joint) entries in which the call differs from the exhaustive first index of the window rows (H = 240, k
uniform, fraction boxes, all --n plans in pieces) — the measured form of the q / v guarantee.

    python tools/first_exit_bench.py [--n 1000000] [--iters 10] [--warmup 2] [--dense-gb 24] [--full-gb 4] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from window_bench import timed   # noqa: E402

WHOLE = 1 << 30
LETTERS = "qvaj"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dense-gb", type=float, default=24.0, help="largest buffer of the dense window the call is compared with")
    ap.add_argument("--full-gb", type=float, default=4.0, help="largest buffer of full rows the whole-plan call is compared with")
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
    L = batch.traj_len
    planned = int((L > 0).sum().item())
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    k_uniform = (torch.rand(n, device=dev, generator=gen, dtype=torch.float64) * L.clamp(min=1)).to(torch.int32)
    k_zero = torch.zeros(n, dtype=torch.int32, device=dev)
    whole_grid = torch.tensor([0, WHOLE], dtype=torch.int32, device=dev)
    # the rows' own ranges over the whole plan, from the envelope call (v, a, j: with the 0 behind the last sample)
    rng_env, _ = ltp.envelopeKnotsArrays(batch, 0, n, 0, whole_grid, arrays=15)
    mn, mx = rng_env[..., 0, 0].contiguous(), rng_env[..., 0, 1].contiguous()            # [n, 4, dof]
    del rng_env
    u = 0.05 + 0.40 * torch.rand((2, n, 4, dof), device=dev, generator=gen, dtype=torch.float64)
    f_lo, f_hi = (mn + u[0] * (mx - mn)).contiguous(), (mx - u[1] * (mx - mn)).contiguous()
    del u
    far = torch.full((4, dof), 1e9, dtype=torch.float64, device=dev)
    boxes = {"inside": (lambda mask: ({LETTERS[x]: (-far[x]).contiguous() for x in sel(mask)}, {LETTERS[x]: far[x].contiguous() for x in sel(mask)})),
             "fraction": (lambda mask: ({LETTERS[x]: f_lo[:, x].contiguous() for x in sel(mask)}, {LETTERS[x]: f_hi[:, x].contiguous() for x in sel(mask)}))}

    def box4(kind, count):
        if kind == "inside":
            return (-far)[None].expand(count, 4, dof), far[None].expand(count, 4, dof)
        return f_lo[:count], f_hi[:count]

    out = torch.empty((n, 4, dof), dtype=torch.int32, device=dev)
    env = torch.empty((n, 4, dof, 1, 2), dtype=torch.float64, device=dev)
    valid = torch.empty(n, dtype=torch.int32, device=dev)
    # the dense window of the H = 240 composition
    H = 240
    Rd = ltp.windowRowStride(H)
    nd = int(min(n, args.dense_gb * 1e9 // (32 * dof * Rd)))
    dense = torch.empty((nd, 4, dof, Rd), dtype=torch.float64, device=dev)
    first_w = torch.empty((nd, 4, dof), dtype=torch.int64, device=dev)

    def reduce_window(kind, planes, k):
        lo, hi = box4(kind, nd)
        x = dense[:, planes, :, :H]
        outside = (x < lo[:, planes, :, None]) | (x > hi[:, planes, :, None])
        at = outside.to(torch.int8).argmax(dim=3)
        first_w[:, :len(planes)] = torch.where(outside.any(dim=3), k[:nd, None, None].long() + at, torch.full_like(at, -1))

    # the full rows of the whole-plan composition: as many plans from the start of the batch as --full-gb holds
    offsets = batch.offsets
    nf = int(min(n, max(1, int(torch.searchsorted(offsets[:n + 1].long(), int(args.full_gb * 1e9 // 8)).item()) - 1)))
    total = int(offsets[nf].item())
    full = torch.empty(max(total, 2), dtype=torch.float64, device=dev)
    Lf = L[:nf].long()
    stride = (Lf + 31) // 32 * 32
    rows_per_plan = 4 * dof
    row_start = (offsets[:nf].long()[:, None] + torch.arange(rows_per_plan, device=dev)[None, :] * stride[:, None]).reshape(-1)   # [nf * 28]
    row_len = stride[:, None].expand(nf, rows_per_plan).reshape(-1)
    row_id = torch.repeat_interleave(torch.arange(nf * rows_per_plan, device=dev), row_len)                                        # element -> row
    pos = (torch.arange(total, device=dev) - row_start[row_id]).to(torch.int32)                                                   # element -> sample
    real = pos < Lf.repeat_interleave(rows_per_plan)[row_id].to(torch.int32)                                                      # (padding of a row)
    big = torch.iinfo(torch.int32).max
    first_f = torch.empty(nf * rows_per_plan, dtype=torch.int32, device=dev)

    def reduce_full(kind):
        lo, hi = box4(kind, nf)
        lo_r, hi_r = lo.reshape(-1), hi.reshape(-1)
        x = full[:total]
        outside = ((x < lo_r[row_id]) | (x > hi_r[row_id])) & real
        first_f.fill_(big)
        first_f.scatter_reduce_(0, row_id, torch.where(outside, pos, torch.full_like(pos, big)), "amin")

    lines = [f"first_exit_bench: n = {n} x {dof}-DoF panda, planned {planned}, median traj_len {int(L.float().median().item())}, iters {args.iters}, "
             f"warm-up {args.warmup}, device {torch.cuda.get_device_name(0)}; window composition on {nd} plans, full-row composition on {nf} plans "
             f"({total * 8 / 1e9:.2f} GB of rows), both scaled to {n}",
             f"{'line':<44} {'F median':>9} {'F min':>8} {'F max':>8} {'E median':>9} {'Y median':>9} {'Y min':>8}  F median < Y min"]
    all_below = True
    for kind in ("inside", "fraction"):
        for arrays in ("q", "qv", "qvaj"):
            mask = sum(1 << LETTERS.index(c) for c in arrays)
            planes = sel(mask)
            A = len(planes)
            lo_by, hi_by = boxes[kind](mask)
            for horizon in (H, WHOLE):
                for kname, k in (("0", k_zero), ("uniform", k_uniform)):
                    grid = torch.tensor([0, horizon], dtype=torch.int32, device=dev)
                    call = lambda: ltp.firstExit(batch, 0, n, k, horizon, arrays=mask, lo=lo_by, hi=hi_by, out=out.view(-1)[:n * A * dof])
                    envl = lambda: ltp.envelopeKnotsArrays(batch, 0, n, k, grid, arrays=mask, out=env.view(-1)[:n * A * dof * 2], valid=valid)
                    if horizon == H:
                        comp = [(nd, lambda: ltp.sampleWindow(batch, 0, nd, k[:nd].contiguous(), H, out=dense, valid=valid[:nd])),
                                (nd, lambda: reduce_window(kind, planes, k))]
                    elif kname == "0":
                        comp = [(nf, lambda: ltp.sampleBatch(batch, 0, nf, full)), (nf, lambda: reduce_full(kind))]
                    else:
                        comp = []          # the full sampler has no start per plan: the k = 0 line is the whole-plan yardstick
                    tf, te, ty = [], [], []
                    for it in range(args.warmup + args.iters):
                        a, b = timed(call), timed(envl)
                        c = sum(timed(fn) * float(n) / plans for plans, fn in comp)
                        if it >= args.warmup:
                            tf.append(a), te.append(b), ty.append(c)
                    tf, te, ty = np.array(tf), np.array(te), np.array(ty)
                    below = (not comp) or float(np.median(tf)) < float(ty.min())
                    all_below &= below
                    what = f"{kind:<8} {arrays:<4} H {'2^30' if horizon == WHOLE else horizon:<5} k {kname}"
                    lines.append(f"{what:<44} {np.median(tf):>9.3f} {tf.min():>8.3f} {tf.max():>8.3f} {np.median(te):>9.3f} "
                                 + (f"{np.median(ty):>9.3f} {ty.min():>8.3f}  {'yes' if below else 'NO'}" if comp else f"{'-':>9} {'-':>8}  (no composition from k per plan)"))
    lines.append(f"the call's median lies below the composition's minimum on every line: {'yes' if all_below else 'NO'}")
    # the measured form of the q / v guarantee: entries that differ from the exhaustive first index of the window rows, all n plans
    differ = {c: 0 for c in LETTERS}
    later = {c: 0 for c in LETTERS}
    for p0 in range(0, n, nd):
        c = min(nd, n - p0)
        kk = k_uniform[p0:p0 + c].contiguous()
        ltp.sampleWindow(batch, p0, c, kk, H, out=dense[:c], valid=valid[:c])
        x = dense[:c, :, :, :H]
        outside = (x < f_lo[p0:p0 + c, :, :, None]) | (x > f_hi[p0:p0 + c, :, :, None])
        at = outside.to(torch.int8).argmax(dim=3)
        want = torch.where(outside.any(dim=3), kk[:, None, None].long() + at, torch.full_like(at, -1))
        want[L[p0:p0 + c] <= 0] = -2
        got = ltp.firstExit(batch, p0, c, kk, H, arrays=15, lo={a: f_lo[p0:p0 + c, x].contiguous() for x, a in enumerate(LETTERS)},
                            hi={a: f_hi[p0:p0 + c, x].contiguous() for x, a in enumerate(LETTERS)}).long()
        torch.cuda.synchronize()
        for x, a in enumerate(LETTERS):
            d = got[:, x] != want[:, x]
            differ[a] += int(d.sum().item())
            later[a] += int((d & ((got[:, x] > want[:, x]) | (got[:, x] == -1)) & (want[:, x] >= 0)).sum().item())
    lines.append(f"entries that differ from the exhaustive first index of the window rows (H = 240, k uniform, fraction boxes, {n} plans x {dof} joints): "
                 + ", ".join(f"{a} {differ[a]} ({later[a]} later or none)" for a in LETTERS))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def sel(mask):
    return [x for x in range(4) if mask >> x & 1]


if __name__ == "__main__":
    main()
