"""The yardstick of the tests of settling (ltp_settle_batch, include/ltp_hip.h) — a helper, not a test: the EXHAUSTIVE scan of full
rows. For plan i, array X and joint j, with k clamped to [0, traj_len], reach = k + H and O = the samples t of [k, reach) with
S_X(t) < lo or S_X(t) > hi: -3 (SETTLE_NOT_YET) when sample reach - 1 is in O, else max(O) + 1, or k when O is empty; -2
(EXIT_NO_PLAN) for a plan without a trajectory. S_X(t) is tests/first_exit_checker.py's: the full row's element t for t < traj_len
and, past the end, the last position for q and +0.0 for v, a and j. Behind sample traj_len nothing changes any more, so the scan
covers [k, min(reach, traj_len + 1)) and its last sample stands for sample reach - 1. It runs in torch on whatever device its
tensors live on: tests/test_settle_cpu.py pins it against a plain Python loop without a GPU, tests/test_gpu_settle.py uses it on
the device."""
from first_exit_checker import _gather, default_boxes, fraction_boxes, pack_full_rows, row_ranges, selected   # noqa: F401 (re-exported)

EXIT_NO_PLAN, SETTLE_NOT_YET = -2, -3
WHOLE = 1 << 30


def expected(full, offsets, lens, k, horizon, dof, first, count, lo, hi, mask=15, budget=1 << 24):
    """The settling samples of plans [first, first + count). k: the starts of those `count` plans (tensor, or an int for all);
    lo / hi: float64 [count, 4, dof], the box of every (plan, array, joint) — all four arrays, whatever the mask. Returns (settle
    int32 [count, A, dof], settle_all int32 [count])."""
    import torch
    dev = full.device
    arrays = selected(mask)
    H = int(horizon)
    assert 1 <= H <= WHOLE
    L = lens[first:first + count].long().to(dev)
    o = offsets[first:first + count].long().to(dev)
    if not hasattr(k, "shape"):
        k = torch.full((count,), int(k), dtype=torch.int64)
    kk = torch.minimum(k.long().to(dev).clamp(min=0), L)
    out = torch.zeros((count, 4, dof), dtype=torch.int64, device=dev)
    need_t = (L - kk + 1).clamp(max=H)                                                      # samples scanned: the last one is reach - 1, or the resting state
    need = need_t.cpu().tolist()
    c0 = 0
    while c0 < count:
        # as many plans as keep the chunk's [c, 4, dof, span] under the budget
        c1 = c0 + 1
        span = need[c0]
        while c1 < count:
            s = max(span, need[c1])
            if (c1 + 1 - c0) * 4 * dof * s > budget:
                break
            span, c1 = s, c1 + 1
        step = torch.arange(span, device=dev)[None, :]
        t = kk[c0:c1, None] + step
        x = _gather(full, o[c0:c1], L[c0:c1], dof, t)
        scanned = (step < need_t[c0:c1, None])[:, None, None, :]
        outside = ((x < lo[c0:c1, :, :, None]) | (x > hi[c0:c1, :, :, None])) & scanned     # false for NaN
        after = (outside * (step + 1)[:, None, None, :]).max(dim=3).values                   # the last outside step + 1, 0 for none
        at_end = after == need_t[c0:c1, None, None]                                         # the horizon's last sample is outside
        out[c0:c1] = torch.where(at_end, torch.full_like(after, SETTLE_NOT_YET), kk[c0:c1, None, None] + after)
        c0 = c1
    out[L <= 0] = EXIT_NO_PLAN
    out = out[:, arrays].contiguous()
    return out.to(torch.int32), fold_all(out).to(torch.int32)


def fold_all(table):
    """settle_all of a table [count, A, dof]: the maximum of the entries read as unsigned 32-bit ints — -2 (no plan) above -3 (not
    yet) above every index."""
    flat = table.reshape(table.shape[0], -1).long()
    top = (flat & 0xFFFFFFFF).max(dim=1).values
    return top - ((top >> 31) << 32)


def end_boxes(full, offsets, lens, dof, seed):
    """The boxes of a tolerance around the value each row comes to rest at, for every plan of the batch: per (plan, array, joint)
    [e - u1 * w, e + u2 * w] with e the row's resting value (the last position for q, 0 for v, a, j), w the row's own range with the
    resting value included and u uniform in (0.05, 0.45) from a seeded generator. e lies in the range, so some sample lies at least
    w / 2 from it: every non-constant row starts or peaks outside its box and rests inside it; a constant row (w == 0) gets the
    degenerate box [e, e], which it never leaves. Returns (lo, hi) [n, 4, dof]; NaN for a plan without a trajectory."""
    import torch
    dev = full.device
    n = int(lens.shape[0])
    L = lens[:n].long().to(dev)
    mn, mx = row_ranges(full, offsets, lens, dof, 0, n)
    e = _gather(full, offsets[:n].long().to(dev), L, dof, L.clamp(min=0)[:, None])[..., 0]  # S_X(traj_len): the resting state
    e[L <= 0] = float("nan")
    mn, mx = torch.minimum(mn, e), torch.maximum(mx, e)
    g = torch.Generator().manual_seed(seed)
    u = (0.05 + 0.40 * torch.rand((2, *mn.shape), generator=g, dtype=torch.float64)).to(dev)
    w = mx - mn
    return (e - u[0] * w).contiguous(), (e + u[1] * w).contiguous()
