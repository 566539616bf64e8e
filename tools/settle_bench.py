"""Cost of ltp_settle_batch (include/ltp_hip.h) on one device: a 1 M x 7-DoF panda batch is planned once; then, alternating in one
process, for the masks q, qv and qvaj, the horizons 240 and 2^30, k = 0 and k uniform in [0, traj_len) per plan, and two kinds of
boxes —
  ends      per (plan, array, joint) [e - u1 w, e + u2 w] around the row's resting value e (the last position for q, 0 for v, a, j),
            w the row's range over the whole plan with e included, u uniform in (0.05, 0.45): nearly every lane settles at an index
            inside its plan, found by bisection;
  fraction  per (plan, array, joint) lo = min + u1 (max - min), hi = max - u2 (max - min) of the row's own range: q mostly rests
            outside (LTP_SETTLE_NOT_YET from the resting state alone) —
  S         the call;
  Y         the composition the call replaces, on as many plans as its buffer holds, scaled to the whole batch. H = 240:
            ltp_sample_window_batch of 240 samples of all four arrays (the window call has no array subset) plus the torch
            reduction to the last index outside the box (compare, the largest step + 1 over the selected arrays, NOT_YET where that
            is the window's last). H = 2^30: the full sampler's rows (ltp_sample_batch from sample 0, k = 0 only) plus the torch
            reduction over the packed rows (gather of each element's box, compare, scatter-amax of the sample index, the resting
            state's verdict; the element -> row and element -> sample maps are built once, untimed).
Next to it, as a cost yardstick only: with one box per joint that no plan leaves both ltp_first_exit_batch (F) and this call walk
the whole horizon and find nothing — the ratio S / F per line, no bar set.
Each launch is timed with device events on the current stream; after the warm-up every variant is launched --iters times. Prints
median / min / max milliseconds per --n plans, then per line whether the call's median lies below the composition's minimum, and
the number of (plan, array, joint) entries in which the call differs from the exhaustive reverse scan of the window rows (H = 240,
k uniform, both kinds of boxes, all --n plans in pieces) — the measured form of the q / v guarantee.

    python tools/settle_bench.py [--n 1000000] [--iters 10] [--warmup 2] [--dense-gb 24] [--full-gb 4] [--out FILE]
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
NOT_YET, NO_PLAN = -3, -2


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
    # the rows' own ranges over the whole plan, from the envelope call (v, a, j: with the 0 behind the last sample), and the resting
    # values: the envelope from k = traj_len holds the last position twice
    rng_env, _ = ltp.envelopeKnotsArrays(batch, 0, n, 0, whole_grid, arrays=15)
    mn, mx = rng_env[..., 0, 0].contiguous(), rng_env[..., 0, 1].contiguous()            # [n, 4, dof]
    del rng_env
    rest_env, _ = ltp.envelopeKnotsArrays(batch, 0, n, L.contiguous(), whole_grid, arrays=1)
    rest = torch.zeros_like(mn)
    rest[:, 0] = rest_env[:, 0, :, 0, 0]
    del rest_env
    u = 0.05 + 0.40 * torch.rand((4, n, 4, dof), device=dev, generator=gen, dtype=torch.float64)
    w = mx - mn
    f_lo, f_hi = (mn + u[0] * w).contiguous(), (mx - u[1] * w).contiguous()
    e_lo, e_hi = (rest - u[2] * w).contiguous(), (rest + u[3] * w).contiguous()
    del u, w
    far = torch.full((4, dof), 1e9, dtype=torch.float64, device=dev)
    families = {"ends": (e_lo, e_hi), "fraction": (f_lo, f_hi)}

    def by_letter(box4, mask, rows=slice(None)):
        return {LETTERS[x]: box4[rows, x].contiguous() for x in sel(mask)}

    out = torch.empty((n, 4, dof), dtype=torch.int32, device=dev)
    # the dense window of the H = 240 composition
    H = 240
    Rd = ltp.windowRowStride(H)
    nd = int(min(n, args.dense_gb * 1e9 // (32 * dof * Rd)))
    dense = torch.empty((nd, 4, dof, Rd), dtype=torch.float64, device=dev)
    valid = torch.empty(n, dtype=torch.int32, device=dev)
    last_w = torch.empty((nd, 4, dof), dtype=torch.int64, device=dev)
    steps = torch.arange(1, H + 1, device=dev, dtype=torch.int32)

    def reverse_scan(x, lo, hi, k):
        """The settling sample from window rows x [c, A, dof, H] of starts k [c]: the last outside step + 1, NOT_YET where that is H."""
        outside = (x < lo[..., None]) | (x > hi[..., None])
        after = (outside * steps).amax(dim=3).long()
        return torch.where(after == H, torch.full_like(after, NOT_YET), k[:, None, None].long() + after)

    def reduce_window(kind, planes, k):
        lo, hi = families[kind]
        last_w[:, :len(planes)] = reverse_scan(dense[:, planes, :, :H], lo[:nd, planes], hi[:nd, planes], k[:nd])

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
    last_f = torch.empty(nf * rows_per_plan, dtype=torch.int32, device=dev)

    def reduce_full(kind):
        lo, hi = families[kind]
        lo_r, hi_r, rest_r = lo[:nf].reshape(-1), hi[:nf].reshape(-1), rest[:nf].reshape(-1)
        x = full[:total]
        outside = ((x < lo_r[row_id]) | (x > hi_r[row_id])) & real
        last_f.fill_(-1)
        last_f.scatter_reduce_(0, row_id, torch.where(outside, pos, torch.full_like(pos, -1)), "amax")
        last_f.add_(1)
        last_f.masked_fill_((rest_r < lo_r) | (rest_r > hi_r), NOT_YET)

    lines = [f"settle_bench: n = {n} x {dof}-DoF panda, planned {planned}, median traj_len {int(L.float().median().item())}, iters {args.iters}, "
             f"warm-up {args.warmup}, device {torch.cuda.get_device_name(0)}; window composition on {nd} plans, full-row composition on {nf} plans "
             f"({total * 8 / 1e9:.2f} GB of rows), both scaled to {n}",
             f"{'line':<44} {'S median':>9} {'S min':>8} {'S max':>8} {'Y median':>9} {'Y min':>8}  S median < Y min"]
    all_below = True
    for kind in ("ends", "fraction"):
        for arrays in ("q", "qv", "qvaj"):
            mask = sum(1 << LETTERS.index(c) for c in arrays)
            planes = sel(mask)
            A = len(planes)
            lo_by, hi_by = by_letter(families[kind][0], mask), by_letter(families[kind][1], mask)
            for horizon in (H, WHOLE):
                for kname, k in (("0", k_zero), ("uniform", k_uniform)):
                    call = lambda: ltp.settle(batch, 0, n, k, horizon, arrays=mask, lo=lo_by, hi=hi_by, out=out.view(-1)[:n * A * dof])
                    if horizon == H:
                        comp = [(nd, lambda: ltp.sampleWindow(batch, 0, nd, k[:nd].contiguous(), H, out=dense, valid=valid[:nd])),
                                (nd, lambda: reduce_window(kind, planes, k))]
                    elif kname == "0":
                        comp = [(nf, lambda: ltp.sampleBatch(batch, 0, nf, full)), (nf, lambda: reduce_full(kind))]
                    else:
                        comp = []          # the full sampler has no start per plan: the k = 0 line is the whole-plan yardstick
                    ts_, ty = [], []
                    for it in range(args.warmup + args.iters):
                        a = timed(call)
                        c = sum(timed(fn) * float(n) / plans for plans, fn in comp)
                        if it >= args.warmup:
                            ts_.append(a), ty.append(c)
                    ts_, ty = np.array(ts_), np.array(ty)
                    below = (not comp) or float(np.median(ts_)) < float(ty.min())
                    all_below &= below
                    what = f"{kind:<8} {arrays:<4} H {'2^30' if horizon == WHOLE else horizon:<5} k {kname}"
                    lines.append(f"{what:<44} {np.median(ts_):>9.3f} {ts_.min():>8.3f} {ts_.max():>8.3f} "
                                 + (f"{np.median(ty):>9.3f} {ty.min():>8.3f}  {'yes' if below else 'NO'}" if comp else f"{'-':>9} {'-':>8}  (no composition from k per plan)"))
    lines.append(f"the call's median lies below the composition's minimum on every line: {'yes' if all_below else 'NO'}")
    # the cost yardstick: boxes no plan leaves, so that the first-exit call walks the whole horizon too
    lines.append(f"{'boxes no plan leaves':<44} {'S median':>9} {'S min':>8} {'F median':>9} {'F min':>8}  S / F (medians)")
    for arrays in ("q", "qv", "qvaj"):
        mask = sum(1 << LETTERS.index(c) for c in arrays)
        A = len(sel(mask))
        lo_by = {LETTERS[x]: (-far[x]).contiguous() for x in sel(mask)}
        hi_by = {LETTERS[x]: far[x].contiguous() for x in sel(mask)}
        for horizon in (H, WHOLE):
            for kname, k in (("0", k_zero), ("uniform", k_uniform)):
                call = lambda: ltp.settle(batch, 0, n, k, horizon, arrays=mask, lo=lo_by, hi=hi_by, out=out.view(-1)[:n * A * dof])
                exits = lambda: ltp.firstExit(batch, 0, n, k, horizon, arrays=mask, lo=lo_by, hi=hi_by, out=out.view(-1)[:n * A * dof])
                ts_, tf = [], []
                for it in range(args.warmup + args.iters):
                    a, b = timed(call), timed(exits)
                    if it >= args.warmup:
                        ts_.append(a), tf.append(b)
                ts_, tf = np.array(ts_), np.array(tf)
                what = f"inside   {arrays:<4} H {'2^30' if horizon == WHOLE else horizon:<5} k {kname}"
                lines.append(f"{what:<44} {np.median(ts_):>9.3f} {ts_.min():>8.3f} {np.median(tf):>9.3f} {tf.min():>8.3f}  {np.median(ts_) / np.median(tf):.2f}")
    # the measured form of the q / v guarantee: entries that differ from the exhaustive reverse scan of the window rows, all n plans
    for kind in ("ends", "fraction"):
        lo4, hi4 = families[kind]
        differ = {c: 0 for c in LETTERS}
        earlier = {c: 0 for c in LETTERS}
        for p0 in range(0, n, nd):
            c = min(nd, n - p0)
            kk = k_uniform[p0:p0 + c].contiguous()
            ltp.sampleWindow(batch, p0, c, kk, H, out=dense[:c], valid=valid[:c])
            want = reverse_scan(dense[:c, :, :, :H], lo4[p0:p0 + c], hi4[p0:p0 + c], kk)
            want[L[p0:p0 + c] <= 0] = NO_PLAN
            got = ltp.settle(batch, p0, c, kk, H, arrays=15, lo=by_letter(lo4, 15, slice(p0, p0 + c)), hi=by_letter(hi4, 15, slice(p0, p0 + c))).long()
            torch.cuda.synchronize()
            for x, a in enumerate(LETTERS):
                d = got[:, x] != want[:, x]
                differ[a] += int(d.sum().item())
                earlier[a] += int((d & (got[:, x] >= 0) & ((got[:, x] < want[:, x]) | (want[:, x] == NOT_YET))).sum().item())
        lines.append(f"entries that differ from the exhaustive reverse scan of the window rows (H = 240, k uniform, {kind} boxes, {n} plans x {dof} joints): "
                     + ", ".join(f"{a} {differ[a]} ({earlier[a]} earlier)" for a in LETTERS))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def sel(mask):
    return [x for x in range(4) if mask >> x & 1]


if __name__ == "__main__":
    main()
