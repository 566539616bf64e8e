"""The yardstick of the horizon-envelope tests (ltp_envelope_knots_batch, include/ltp_hip.h) — a helper, not a test: what the
envelope of interval w of an edge list g must hold, reduced from the q rows ltp_sample_batch wrote for the same batch; the `valid`
formula; and the acceptance rule of the analytic envelope form. It runs on whatever device its tensors live on, so
tests/test_envelope_knots_cpu.py pins it against a plain Python loop without a GPU and tests/test_gpu_envelope_knots.py uses it on
the device. The edge lists are the grids of tests/knots_checker.py.

Interval w holds the trajectory samples t with a_w <= t <= b_w, a_w = max(k, 0) + g[w], b_w = max(a_w, max(k, 0) + g[w + 1] - 1 +
closed), every t clamped to traj_len - 1; the full-row layout is tests/horizon_checker.py's."""
import numpy as np

from horizon_checker import int_view, pack_full_rows, valid_formula   # noqa: F401 (re-exported for the tests)
from knots_checker import GRIDS, MAX_KNOTS   # noqa: F401

MAX_INTERVALS = MAX_KNOTS - 1
EDGE_GRIDS = {name: g for name, g in GRIDS.items() if len(g) >= 2}      # "one" has a single edge: a refusal case only


def expected(full, offsets, lens, k, g, closed, dof, first, count, chunk=256):
    """The envelopes of plans [first, first + count) on the edges g: gathers q[min(t, L - 1)] for t = max(k, 0) + o, o in
    [g[0], g[M] + closed), and reduces per interval by the definition above. k: the starts of those `count` plans (tensor); g: the
    M + 1 edges (array or tensor). Returns (env float64 [count, dof, M, 2] — NaN for a plan without a trajectory —, valid int32
    [count], planned bool [count])."""
    import torch
    dev = full.device
    g = torch.as_tensor(np.asarray(g.cpu() if hasattr(g, "cpu") else g).astype(np.int64))
    M = int(g.numel()) - 1
    assert M >= 1
    closed = int(bool(closed))
    lo_at = (g[:-1] - g[0]).tolist()
    hi_at = (torch.maximum(g[:-1], g[1:] - 1 + closed) - g[0]).tolist()
    span = max(hi_at) + 1
    L = lens[first:first + count].long().to(dev)
    o = offsets[first:first + count].long().to(dev)
    kk = k.long().to(dev).clamp(min=0)
    planned = L > 0
    env = torch.full((count, dof, M, 2), float("nan"), dtype=torch.float64, device=dev)
    steps = torch.arange(span, device=dev) + int(g[0])
    joints = torch.arange(dof, device=dev).view(1, dof, 1)
    for c0 in range(0, count, chunk):
        c1 = min(count, c0 + chunk)
        Lc = L[c0:c1]
        tc = torch.minimum(kk[c0:c1, None] + steps[None, :], (Lc - 1).clamp(min=0)[:, None])       # [c, span]
        stride = (Lc + 31) // 32 * 32
        idx = o[c0:c1].view(-1, 1, 1) + joints * stride.view(-1, 1, 1) + tc[:, None, :]           # array 0 = q
        idx = torch.where(planned[c0:c1].view(-1, 1, 1), idx, torch.zeros_like(idx))
        q = full[idx]                                                                             # [c, dof, span]
        for w in range(M):
            piece = q[:, :, lo_at[w]:hi_at[w] + 1]
            env[c0:c1, :, w, 0] = piece.min(dim=2).values
            env[c0:c1, :, w, 1] = piece.max(dim=2).values
    env[~planned] = float("nan")
    return env, valid_formula(L, kk, g[:-1].to(dev)), planned


def compare(got, red, planned):
    """The project's acceptance rule for the analytic envelope form against reduced rows (tests/test_gpu_edge.py::
    test_analytic_envelopes_agree_with_the_exhaustive_form), per plan: returns (bad [count] bool — the NaN pattern differs, a
    minimum below / a maximum above the samples' own, or |d| > 1e-12 —, worst |d|, share of bit-identical values)."""
    import torch
    count = got.shape[0]
    nan_bad = torch.isnan(got) != torch.isnan(red)
    d = torch.nan_to_num((got - red).abs(), nan=0.0)
    outside = (got[..., 0] < red[..., 0]) | (got[..., 1] > red[..., 1])
    bad = nan_bad.reshape(count, -1).any(dim=1) | (d > 1e-12).reshape(count, -1).any(dim=1) | outside.reshape(count, -1).any(dim=1)
    real = ~torch.isnan(red)
    same = (int_view(got) == int_view(red)) & real
    share = float(same.sum().item()) / max(int(real.sum().item()), 1)
    return bad, float(d.max().item()) if d.numel() else 0.0, share
