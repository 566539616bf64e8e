"""The yardstick of the tests of the box readers (ltp_first_exit_batch and ltp_settle_batch, include/ltp_hip.h) — a helper, not a
test: the EXHAUSTIVE scan of full rows. For plan i, array X and joint j, with k clamped to [0, traj_len] and reach = k + H, O is
the set of trajectory samples t in [k, reach) with S_X(t) < lo or S_X(t) > hi; S_X(t) is the full row's element t for t < traj_len
and, past the end, the last position for q and +0.0 for v, a and j — what ltp_sample_knots_batch stores there.

  first exits (expected_exits): min(O), or -1 (EXIT_NONE) where O is empty;
  settling (expected_settle): -3 (SETTLE_NOT_YET) when sample reach - 1 is in O, else max(O) + 1, or k where O is empty. Behind
    sample traj_len nothing changes any more, so the scan covers [k, min(reach, traj_len + 1)) and its last sample stands for
    sample reach - 1;

-2 (EXIT_NO_PLAN) in both for a plan without a trajectory. It runs in torch on whatever device its tensors live on:
tests/test_first_exit_cpu.py and tests/test_settle_cpu.py pin each reduction against a plain Python loop without a GPU,
tests/test_gpu_first_exit.py and tests/test_gpu_settle.py use them on the device.

The full-row layout is tests/horizon_checker.py's: array x of joint j of a plan starts (x * dof + j) * stride behind the plan's
offset, stride = traj_len rounded up to 32."""
import numpy as np

from envelope_checker import selected

EXIT_NONE, EXIT_NO_PLAN, SETTLE_NOT_YET = -1, -2, -3
WHOLE = 1 << 30


def _gather(full, o, L, dof, t):
    """S_X(t) for every array and joint of a chunk of plans: [c, 4, dof, span] from t [c, span] (t >= 0)."""
    import torch
    dev = full.device
    planned = L > 0
    rows = torch.arange(4 * dof, device=dev).view(1, 4, dof, 1)
    stride = ((L + 31) // 32 * 32).view(-1, 1, 1, 1)
    tc = torch.minimum(t, (L - 1).clamp(min=0)[:, None])[:, None, None, :]
    idx = o.view(-1, 1, 1, 1) + rows * stride + tc
    idx = torch.where(planned.view(-1, 1, 1, 1), idx, torch.zeros_like(idx))
    x = full[idx]
    rests = torch.tensor([False, True, True, True], device=dev).view(1, 4, 1, 1)
    past = (t >= L[:, None])[:, None, None, :] & rests
    return torch.where(past, torch.zeros_like(x), x)


def row_ranges(full, offsets, lens, dof, first, count, chunk=64):
    """(min, max) [count, 4, dof] of every row over its own samples [0, traj_len); NaN for a plan without a trajectory."""
    import torch
    dev = full.device
    L = lens[first:first + count].long().to(dev)
    o = offsets[first:first + count].long().to(dev)
    mn = torch.full((count, 4, dof), float("nan"), dtype=torch.float64, device=dev)
    mx = mn.clone()
    for c0 in range(0, count, chunk):
        c1 = min(count, c0 + chunk)
        Lc = L[c0:c1]
        span = max(int(Lc.max().item()), 1)
        t = torch.arange(span, device=dev)[None, :].expand(c1 - c0, span)
        x = _gather(full, o[c0:c1], Lc, dof, torch.minimum(t, (Lc - 1).clamp(min=0)[:, None]))   # (clamped: the last sample repeats)
        mn[c0:c1] = x.min(dim=3).values
        mx[c0:c1] = x.max(dim=3).values
    mn[L <= 0] = float("nan")
    mx[L <= 0] = float("nan")
    return mn, mx


def _scan(full, offsets, lens, k, horizon, dof, first, count, lo, hi, mask, budget, fill, reduce, fold):
    """The frame of both scans over plans [first, first + count): k clamped, chunks of plans chosen under the budget, S_X(t)
    gathered for t = k + step and compared with the box. reduce(outside [c, 4, dof, span], step [1, span], kk [c], need_t [c]) gives
    the chunk's answers [c, 4, dof]; need_t = min(H, traj_len - k + 1) is the number of samples of the horizon that can differ.
    Returns (table int32 [count, A, dof], fold(table) int32 [count])."""
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
    out = torch.full((count, 4, dof), fill, dtype=torch.int64, device=dev)
    need_t = (L - kk + 1).clamp(max=H)                                                      # the span reaches the one sample past the end
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
        x = _gather(full, o[c0:c1], L[c0:c1], dof, kk[c0:c1, None] + step)
        outside = (x < lo[c0:c1, :, :, None]) | (x > hi[c0:c1, :, :, None])                 # false for NaN
        out[c0:c1] = reduce(outside, step, kk[c0:c1], need_t[c0:c1])
        c0 = c1
    out[L <= 0] = EXIT_NO_PLAN
    out = out[:, arrays].contiguous()
    return out.to(torch.int32), fold(out).to(torch.int32)


def _first_true(outside, step, kk, need_t):
    """The first exit: the first True of the chunk's span. The span is at most H, and a plan whose own need is shorter has
    need = traj_len - k + 1: behind it every sample repeats sample traj_len, which the need holds."""
    import torch
    any_out = outside.any(dim=3)
    at = outside.to(torch.int8).argmax(dim=3)                                               # the first True
    return torch.where(any_out, kk[:, None, None] + at, torch.full_like(at, EXIT_NONE))


def _last_true(outside, step, kk, need_t):
    """Settling: the last True + 1 among the need_t samples scanned, NOT_YET where that is the horizon's last sample."""
    import torch
    scanned = (step < need_t[:, None])[:, None, None, :]
    after = ((outside & scanned) * (step + 1)[:, None, None, :]).max(dim=3).values          # the last outside step + 1, 0 for none
    at_end = after == need_t[:, None, None]                                                 # the horizon's last sample is outside
    return torch.where(at_end, torch.full_like(after, SETTLE_NOT_YET), kk[:, None, None] + after)


def expected_exits(full, offsets, lens, k, horizon, dof, first, count, lo, hi, mask=15, budget=1 << 24):
    """The first exits of plans [first, first + count). k: the starts of those `count` plans (tensor, or an int for all); lo / hi:
    float64 [count, 4, dof], the box of every (plan, array, joint) — all four arrays, whatever the mask. Returns (exit int32
    [count, A, dof], first_any int32 [count])."""
    return _scan(full, offsets, lens, k, horizon, dof, first, count, lo, hi, mask, budget, EXIT_NONE, _first_true, fold_any)


def expected_settle(full, offsets, lens, k, horizon, dof, first, count, lo, hi, mask=15, budget=1 << 24):
    """The settling samples of plans [first, first + count), arguments as expected_exits. Returns (settle int32 [count, A, dof],
    settle_all int32 [count])."""
    return _scan(full, offsets, lens, k, horizon, dof, first, count, lo, hi, mask, budget, 0, _last_true, fold_all)


def fold_any(table):
    """first_any of a table [count, A, dof]: the minimum over the real indices, -1 where all are -1, -2 for a plan without a trajectory."""
    import torch
    flat = table.reshape(table.shape[0], -1).long()
    big = torch.iinfo(torch.int64).max
    real = torch.where(flat >= 0, flat, torch.full_like(flat, big)).min(dim=1).values
    none = flat.max(dim=1).values                                                           # no real index: -1 or -2 throughout
    return torch.where(real == big, none, real)


def fold_all(table):
    """settle_all of a table [count, A, dof]: the maximum of the entries read as unsigned 32-bit ints — -2 (no plan) above -3 (not
    yet) above every index."""
    flat = table.reshape(table.shape[0], -1).long()
    top = (flat & 0xFFFFFFFF).max(dim=1).values
    return top - ((top >> 31) << 32)


def default_boxes(count, limits, dev, set_index=None):
    """The default boxes [count, 4, dof] of a call: q_min / q_max, -+v_max, -+a_max, -+j_max. limits: a dict of [dof] lists, or —
    with set_index (tensor [count]) — of [K, dof] arrays."""
    import torch
    rows = [torch.as_tensor(np.asarray(limits[key], dtype=np.float64)).to(dev) for key in ("q_min", "q_max", "v_max", "a_max", "j_max")]
    if set_index is not None:
        rows = [r[set_index.long().to(dev)] for r in rows]                                  # [count, dof]
    else:
        rows = [r[None, :].expand(count, -1) for r in rows]
    lo = torch.stack([rows[0], -rows[2], -rows[3], -rows[4]], dim=1).contiguous()
    hi = torch.stack([rows[1], rows[2], rows[3], rows[4]], dim=1).contiguous()
    return lo, hi


def fraction_boxes(mn, mx, seed):
    """Boxes per (plan, array, joint) from the row's own range: lo = min + u1 * (max - min), hi = max - u2 * (max - min), u uniform
    in (0.05, 0.45) from a seeded generator. Almost every lane has an exit and none sits on a sample by construction; a constant
    row (range 0) gets the degenerate box [value, value], which it never leaves."""
    import torch
    g = torch.Generator().manual_seed(seed)
    u = (0.05 + 0.40 * torch.rand((2, *mn.shape), generator=g, dtype=torch.float64)).to(mn.device)
    w = mx - mn
    return (mn + u[0] * w).contiguous(), (mx - u[1] * w).contiguous()


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
