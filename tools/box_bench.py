"""Cost of the two box readers (include/ltp_hip.h) on one device, --reader exit for ltp_first_exit_batch and --reader settle for
ltp_settle_batch: a 1 M x 7-DoF panda batch is planned once; then, alternating in one process, for the masks q, qv and qvaj, the
horizons 240 and 2^30, k = 0 and k uniform in [0, traj_len) per plan, and two kinds of boxes per reader —
  exit    inside    one box per joint (stride 0) that no plan leaves: every stretch passes the quick reject, the bulk path;
          fraction  per (plan, array, joint) lo = min + u1 (max - min), hi = max - u2 (max - min) of the row's own range over the
                    whole plan, u uniform in (0.05, 0.45): nearly every lane bisects;
  settle  ends      per (plan, array, joint) [e - u1 w, e + u2 w] around the row's resting value e (the last position for q, 0 for
                    v, a, j), w the row's range over the whole plan with e included: nearly every lane settles at an index inside
                    its plan, found by bisection;
          fraction  as above: q mostly rests outside (LTP_SETTLE_NOT_YET from the resting state alone) —
  F / S   the call;
  E       (exit) ltp_envelope_knots_arrays_batch with ONE interval [0, horizon) and the same mask from the same k: the walk the
          call's cost is expected to be that of (a figure, not a gate);
  Y       the composition the call replaces, on as many plans as its buffer holds, scaled to the whole batch. H = 240:
          ltp_sample_window_batch of 240 samples of all four arrays (the window call has no array subset) plus the torch reduction
          over the selected arrays (exit: compare, any, argmax to the first index outside; settle: compare, the largest step + 1,
          NOT_YET where that is the window's last). H = 2^30: the full sampler's rows (ltp_sample_batch from sample 0, k = 0 only)
          plus the torch reduction over the packed rows (gather of each element's box, compare, scatter-amin / -amax of the sample
          index, for settle the resting state's verdict; the element -> row and element -> sample maps are built once, untimed).
For settle, next to it, as a cost yardstick only: with one box per joint that no plan leaves both calls walk the whole horizon and
find nothing — the ratio S / F per line, no bar set.
Each launch is timed with device events on the current stream; after the warm-up every variant is launched --iters times. Prints
median / min / max milliseconds per --n plans, then per line whether the call's median lies below the composition's minimum, and
the number of (plan, array, joint) entries in which the call differs from the exhaustive scan of the window rows (H = 240, k
uniform, the reader's per-plan boxes, all --n plans in pieces) — the measured form of the q / v guarantee.

    python tools/box_bench.py --reader exit|settle [--n 1000000] [--iters 10] [--warmup 2] [--dense-gb 24] [--full-gb 4] [--out FILE]
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
NONE, NO_PLAN, NOT_YET = -1, -2, -3
H = 240                          # the horizon of the window composition


def sel(mask):
    return [x for x in range(4) if mask >> x & 1]


def by_letter(box4, mask, rows=slice(None)):
    """The dict by array letter the readers take, from boxes [n, 4, dof] (rows: a slice of plans) or [4, dof] (one box per joint)."""
    return {LETTERS[x]: (box4[x] if box4.dim() == 2 else box4[rows, x]).contiguous() for x in sel(mask)}


def measure(variants, args):
    """Every variant (a list of (plans, fn): its launches, each scaled from its plans to --n) timed alternately; the times after the
    warm-up as one array per variant."""
    times = [[] for _ in variants]
    for it in range(args.warmup + args.iters):
        for t, launches in zip(times, variants):
            ms = sum(timed(fn) * float(args.n) / plans for plans, fn in launches)
            if it >= args.warmup:
                t.append(ms)
    return [np.array(t) for t in times]


class Exit:
    """ltp_first_exit_batch: the first outside sample."""
    name, letter, kinds, checked = "first_exit_bench", "F", ("inside", "fraction"), ("fraction",)
    scan, side = "first index", "later or none"

    @staticmethod
    def call(ltp, *args, **kw):
        return ltp.firstExit(*args, **kw)

    @staticmethod
    def families(ltp, batch, mn, mx, far, gen):
        import torch
        u = 0.05 + 0.40 * torch.rand((2, *mn.shape), device=mn.device, generator=gen, dtype=torch.float64)
        return {"inside": (-far, far), "fraction": ((mn + u[0] * (mx - mn)).contiguous(), (mx - u[1] * (mx - mn)).contiguous())}, None

    @staticmethod
    def extras_buffer(n, dof, dev):
        import torch
        return torch.empty((n, 4, dof, 1, 2), dtype=torch.float64, device=dev)

    @staticmethod
    def extras(ltp, batch, n, k, horizon, mask, A, dof, env, valid):
        """E: the envelope walk of one interval [0, horizon), into the buffers main() holds."""
        import torch
        grid = torch.tensor([0, horizon], dtype=torch.int32, device=k.device)
        return [("E", [(n, lambda: ltp.envelopeKnotsArrays(batch, 0, n, k, grid, arrays=mask, out=env.view(-1)[:n * A * dof * 2], valid=valid))])]

    @staticmethod
    def yardstick(ltp, batch, n, dof, far, starts, out, args):
        return []

    @staticmethod
    def of_window(x, lo, hi, k):
        """The first exit from window rows x [c, A, dof, H] of starts k [c]."""
        import torch
        outside = (x < lo[..., None]) | (x > hi[..., None])
        at = outside.to(torch.int8).argmax(dim=3)
        return torch.where(outside.any(dim=3), k[:, None, None].long() + at, torch.full_like(at, NONE))

    @staticmethod
    def of_rows(outside, pos, row_id, answer, lo_r, hi_r, rest_r):
        import torch
        big = torch.iinfo(torch.int32).max
        answer.fill_(big)
        answer.scatter_reduce_(0, row_id, torch.where(outside, pos, torch.full_like(pos, big)), "amin")

    @staticmethod
    def excused(got, want):
        return ((got > want) | (got == NONE)) & (want >= 0)


class Settle:
    """ltp_settle_batch: the last outside sample + 1."""
    name, letter, kinds, checked = "settle_bench", "S", ("ends", "fraction"), ("ends", "fraction")
    scan, side = "reverse scan", "earlier"

    @staticmethod
    def call(ltp, *args, **kw):
        return ltp.settle(*args, **kw)

    @staticmethod
    def families(ltp, batch, mn, mx, far, gen):
        import torch
        n, L = mn.shape[0], batch.traj_len
        # the resting values: the envelope from k = traj_len holds the last position twice
        whole_grid = torch.tensor([0, WHOLE], dtype=torch.int32, device=mn.device)
        rest_env, _ = ltp.envelopeKnotsArrays(batch, 0, n, L.contiguous(), whole_grid, arrays=1)
        rest = torch.zeros_like(mn)
        rest[:, 0] = rest_env[:, 0, :, 0, 0]
        u = 0.05 + 0.40 * torch.rand((4, *mn.shape), device=mn.device, generator=gen, dtype=torch.float64)
        w = mx - mn
        return {"ends": ((rest - u[2] * w).contiguous(), (rest + u[3] * w).contiguous()),
                "fraction": ((mn + u[0] * w).contiguous(), (mx - u[1] * w).contiguous())}, rest

    @staticmethod
    def extras_buffer(n, dof, dev):
        return None

    @staticmethod
    def extras(ltp, batch, n, k, horizon, mask, A, dof, env, valid):
        return []

    @staticmethod
    def yardstick(ltp, batch, n, dof, far, starts, out, args):
        """The cost yardstick: boxes no plan leaves, so that the first-exit call walks the whole horizon too. S / F per line."""
        lines = [f"{'boxes no plan leaves':<44} {'S median':>9} {'S min':>8} {'F median':>9} {'F min':>8}  S / F (medians)"]
        for arrays in ("q", "qv", "qvaj"):
            mask = sum(1 << LETTERS.index(a) for a in arrays)
            A = len(sel(mask))
            lo_by, hi_by = by_letter(-far, mask), by_letter(far, mask)
            for horizon in (H, WHOLE):
                for kname, k in starts:
                    call = lambda: ltp.settle(batch, 0, n, k, horizon, arrays=mask, lo=lo_by, hi=hi_by, out=out.view(-1)[:n * A * dof])
                    exits = lambda: ltp.firstExit(batch, 0, n, k, horizon, arrays=mask, lo=lo_by, hi=hi_by, out=out.view(-1)[:n * A * dof])
                    ts_, tf = measure([[(n, call)], [(n, exits)]], args)
                    what = f"inside   {arrays:<4} H {'2^30' if horizon == WHOLE else horizon:<5} k {kname}"
                    lines.append(f"{what:<44} {np.median(ts_):>9.3f} {ts_.min():>8.3f} {np.median(tf):>9.3f} {tf.min():>8.3f}  {np.median(ts_) / np.median(tf):.2f}")
        return lines

    @staticmethod
    def of_window(x, lo, hi, k):
        """The settling sample from window rows x [c, A, dof, H] of starts k [c]: the last outside step + 1, NOT_YET where that is H."""
        import torch
        steps = torch.arange(1, H + 1, device=x.device, dtype=torch.int32)
        outside = (x < lo[..., None]) | (x > hi[..., None])
        after = (outside * steps).amax(dim=3).long()
        return torch.where(after == H, torch.full_like(after, NOT_YET), k[:, None, None].long() + after)

    @staticmethod
    def of_rows(outside, pos, row_id, answer, lo_r, hi_r, rest_r):
        import torch
        answer.fill_(-1)
        answer.scatter_reduce_(0, row_id, torch.where(outside, pos, torch.full_like(pos, -1)), "amax")
        answer.add_(1)
        answer.masked_fill_((rest_r < lo_r) | (rest_r > hi_r), NOT_YET)

    @staticmethod
    def excused(got, want):
        return (got >= 0) & ((got < want) | (want == NOT_YET))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reader", choices=("exit", "settle"), required=True)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dense-gb", type=float, default=24.0, help="largest buffer of the dense window the call is compared with")
    ap.add_argument("--full-gb", type=float, default=4.0, help="largest buffer of full rows the whole-plan call is compared with")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    R = {"exit": Exit, "settle": Settle}[args.reader]
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
    far = torch.full((4, dof), 1e9, dtype=torch.float64, device=dev)                     # one box per joint that no plan leaves
    families, rest = R.families(ltp, batch, mn, mx, far, gen)

    def box4(kind, count):
        lo, hi = families[kind]
        return (lo[None].expand(count, 4, dof), hi[None].expand(count, 4, dof)) if lo.dim() == 2 else (lo[:count], hi[:count])

    out = torch.empty((n, 4, dof), dtype=torch.int32, device=dev)
    env = R.extras_buffer(n, dof, dev)
    valid = torch.empty(n, dtype=torch.int32, device=dev)
    starts = (("0", k_zero), ("uniform", k_uniform))
    # the dense window of the H = 240 composition
    Rd = ltp.windowRowStride(H)
    nd = int(min(n, args.dense_gb * 1e9 // (32 * dof * Rd)))
    dense = torch.empty((nd, 4, dof, Rd), dtype=torch.float64, device=dev)
    answer_w = torch.empty((nd, 4, dof), dtype=torch.int64, device=dev)

    def reduce_window(kind, planes, k):
        lo, hi = box4(kind, nd)
        answer_w[:, :len(planes)] = R.of_window(dense[:, planes, :, :H], lo[:, planes], hi[:, planes], k[:nd])

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
    answer_f = torch.empty(nf * rows_per_plan, dtype=torch.int32, device=dev)

    def reduce_full(kind):
        lo, hi = box4(kind, nf)
        lo_r, hi_r = lo.reshape(-1), hi.reshape(-1)
        x = full[:total]
        outside = ((x < lo_r[row_id]) | (x > hi_r[row_id])) & real
        R.of_rows(outside, pos, row_id, answer_f, lo_r, hi_r, None if rest is None else rest[:nf].reshape(-1))

    c = R.letter
    lines = [f"{R.name}: n = {n} x {dof}-DoF panda, planned {planned}, median traj_len {int(L.float().median().item())}, iters {args.iters}, "
             f"warm-up {args.warmup}, device {torch.cuda.get_device_name(0)}; window composition on {nd} plans, full-row composition on {nf} plans "
             f"({total * 8 / 1e9:.2f} GB of rows), both scaled to {n}"]
    all_below = True
    for kind in R.kinds:
        for arrays in ("q", "qv", "qvaj"):
            mask = sum(1 << LETTERS.index(a) for a in arrays)
            planes = sel(mask)
            A = len(planes)
            lo_by, hi_by = by_letter(families[kind][0], mask), by_letter(families[kind][1], mask)
            for horizon in (H, WHOLE):
                for kname, k in starts:
                    call = [(n, lambda: R.call(ltp, batch, 0, n, k, horizon, arrays=mask, lo=lo_by, hi=hi_by, out=out.view(-1)[:n * A * dof]))]
                    extras = R.extras(ltp, batch, n, k, horizon, mask, A, dof, env, valid)
                    if horizon == H:
                        comp = [(nd, lambda: ltp.sampleWindow(batch, 0, nd, k[:nd].contiguous(), H, out=dense, valid=valid[:nd])),
                                (nd, lambda: reduce_window(kind, planes, k))]
                    elif kname == "0":
                        comp = [(nf, lambda: ltp.sampleBatch(batch, 0, nf, full)), (nf, lambda: reduce_full(kind))]
                    else:
                        comp = []          # the full sampler has no start per plan: the k = 0 line is the whole-plan yardstick
                    if len(lines) == 1:
                        lines.append(f"{'line':<44} {c + ' median':>9} {c + ' min':>8} {c + ' max':>8} " + "".join(f"{e + ' median':>9} " for e, _ in extras)
                                     + f"{'Y median':>9} {'Y min':>8}  {c} median < Y min")
                    tc, *te, ty = measure([call] + [launches for _, launches in extras] + [comp], args)
                    below = (not comp) or float(np.median(tc)) < float(ty.min())
                    all_below &= below
                    what = f"{kind:<8} {arrays:<4} H {'2^30' if horizon == WHOLE else horizon:<5} k {kname}"
                    lines.append(f"{what:<44} {np.median(tc):>9.3f} {tc.min():>8.3f} {tc.max():>8.3f} " + "".join(f"{np.median(t):>9.3f} " for t in te)
                                 + (f"{np.median(ty):>9.3f} {ty.min():>8.3f}  {'yes' if below else 'NO'}" if comp else f"{'-':>9} {'-':>8}  (no composition from k per plan)"))
    lines.append(f"the call's median lies below the composition's minimum on every line: {'yes' if all_below else 'NO'}")
    lines += R.yardstick(ltp, batch, n, dof, far, starts, out, args)
    # the measured form of the q / v guarantee: entries that differ from the exhaustive scan of the window rows, all n plans
    for kind in R.checked:
        lo4, hi4 = families[kind]
        differ = {a: 0 for a in LETTERS}
        excused = {a: 0 for a in LETTERS}
        for p0 in range(0, n, nd):
            cnt = min(nd, n - p0)
            kk = k_uniform[p0:p0 + cnt].contiguous()
            ltp.sampleWindow(batch, p0, cnt, kk, H, out=dense[:cnt], valid=valid[:cnt])
            want = R.of_window(dense[:cnt, :, :, :H], lo4[p0:p0 + cnt], hi4[p0:p0 + cnt], kk)
            want[L[p0:p0 + cnt] <= 0] = NO_PLAN
            got = R.call(ltp, batch, p0, cnt, kk, H, arrays=15, lo=by_letter(lo4, 15, slice(p0, p0 + cnt)), hi=by_letter(hi4, 15, slice(p0, p0 + cnt))).long()
            torch.cuda.synchronize()
            for x, a in enumerate(LETTERS):
                d = got[:, x] != want[:, x]
                differ[a] += int(d.sum().item())
                excused[a] += int((d & R.excused(got[:, x], want[:, x])).sum().item())
        lines.append(f"entries that differ from the exhaustive {R.scan} of the window rows (H = 240, k uniform, {kind} boxes, {n} plans x {dof} joints): "
                     + ", ".join(f"{a} {differ[a]} ({excused[a]} {R.side})" for a in LETTERS))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
