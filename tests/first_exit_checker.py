"""The yardstick of the tests of the first exits (ltp_first_exit_batch, include/ltp_hip.h) — a helper, not a test: the EXHAUSTIVE
scan of full rows. For plan i, array X and joint j the first trajectory sample t in [k, k + H) with S_X(t) < lo or S_X(t) > hi,
k clamped to [0, traj_len]; S_X(t) is the full row's element t for t < traj_len and, past the end, the last position for q and +0.0
for v, a and j — what ltp_sample_knots_batch stores there. -1 (EXIT_NONE) where no sample of the horizon lies outside, -2
(EXIT_NO_PLAN) for a plan without a trajectory. It runs in torch on whatever device its tensors live on:
tests/test_first_exit_cpu.py pins it against a plain Python loop without a GPU, tests/test_gpu_first_exit.py uses it on the device.

The full-row layout is tests/horizon_checker.py's: array x of joint j of a plan starts (x * dof + j) * stride behind the plan's
offset, stride = traj_len rounded up to 32."""
import numpy as np

from envelope_arrays_checker import selected                 # noqa: F401 (re-exported for the tests)
from horizon_checker import pack_full_rows                   # noqa: F401

EXIT_NONE, EXIT_NO_PLAN = -1, -2
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


def expected(full, offsets, lens, k, horizon, dof, first, count, lo, hi, mask=15, budget=1 << 24):
    """The first exits of plans [first, first + count). k: the starts of those `count` plans (tensor, or an int for all); lo / hi:
    float64 [count, 4, dof], the box of every (plan, array, joint) — all four arrays, whatever the mask. Returns (exit int32
    [count, A, dof], first_any int32 [count])."""
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
    out = torch.full((count, 4, dof), EXIT_NONE, dtype=torch.int64, device=dev)
    need = (L - kk + 1).clamp(max=H).cpu().tolist()                                         # the span reaches the one sample past the end
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
        t = kk[c0:c1, None] + torch.arange(span, device=dev)[None, :]
        x = _gather(full, o[c0:c1], L[c0:c1], dof, t)
        outside = (x < lo[c0:c1, :, :, None]) | (x > hi[c0:c1, :, :, None])                 # false for NaN
        any_out = outside.any(dim=3)
        at = outside.to(torch.int8).argmax(dim=3)                                           # the first True
        out[c0:c1] = torch.where(any_out, kk[c0:c1, None, None] + at, torch.full_like(at, EXIT_NONE))
        c0 = c1
    out[L <= 0] = EXIT_NO_PLAN
    out = out[:, arrays].contiguous()
    return out.to(torch.int32), fold_any(out).to(torch.int32)


def fold_any(table):
    """first_any of a table [count, A, dof]: the minimum over the real indices, -1 where all are -1, -2 for a plan without a trajectory."""
    import torch
    flat = table.reshape(table.shape[0], -1).long()
    big = torch.iinfo(torch.int64).max
    real = torch.where(flat >= 0, flat, torch.full_like(flat, big)).min(dim=1).values
    none = flat.max(dim=1).values                                                           # no real index: -1 or -2 throughout
    return torch.where(real == big, none, real)


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
    """The boxes of the GPU tests, per (plan, array, joint) from the row's own range: lo = min + u1 * (max - min), hi = max - u2 *
    (max - min), u uniform in (0.05, 0.45) from a seeded generator. Almost every lane has an exit and none sits on a sample by
    construction; a constant row (range 0) gets the degenerate box [value, value], which it never leaves."""
    import torch
    g = torch.Generator().manual_seed(seed)
    u = (0.05 + 0.40 * torch.rand((2, *mn.shape), generator=g, dtype=torch.float64)).to(mn.device)
    w = mx - mn
    return (mn + u[0] * w).contiguous(), (mx - u[1] * w).contiguous()
