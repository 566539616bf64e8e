"""The yardstick of the tests of the two horizon-envelope calls — the q-only ltp_envelope_knots_batch and ltp_envelope_knots_arrays_batch
for q, v, a and j (include/ltp_hip.h) — a helper, not a test: what the envelope of interval w of an edge list g must hold, reduced from
the rows ltp_sample_batch wrote for the same batch (array x of a plan sits x * dof * stride behind array 0 of the full-row layout of
tests/horizon_checker.py), with the rule for the samples past the end; the `valid` formula; and the two acceptance rules. It runs on
whatever device its tensors live on: tests/envelope_cpu_helpers.py pins it against a plain Python loop without a GPU,
tests/envelope_helpers.py uses it on the device. The edge lists are the grids of tests/knots_checker.py.

Interval w holds the trajectory samples t with a_w <= t <= b_w, a_w = max(k, 0) + g[w], b_w = max(a_w, max(k, 0) + g[w + 1] - 1 +
closed). Sample t of array X is the full row's element t for t < traj_len; past the end it is the last position for q and +0.0 for
v, a and j — what ltp_sample_knots_batch stores there."""
import numpy as np

from horizon_checker import int_view, pack_full_rows, valid_formula   # noqa: F401 (re-exported for the tests)
from knots_checker import GRIDS, MAX_KNOTS   # noqa: F401

MAX_INTERVALS = MAX_KNOTS - 1
EDGE_GRIDS = {name: g for name, g in GRIDS.items() if len(g) >= 2}      # "one" has a single edge: a refusal case only
ENV_Q, ENV_V, ENV_A, ENV_J = 1, 2, 4, 8
NAMES = "qvaj"


def selected(mask):
    """The arrays of a mask in the order of their planes: indices into q, v, a, j."""
    assert 1 <= mask <= 15
    return [x for x in range(4) if mask >> x & 1]


def expected(full, offsets, lens, k, g, closed, dof, first, count, mask=15, chunk=256):
    """The envelopes of plans [first, first + count) on the edges g for the arrays of `mask`. k: the starts of those `count` plans
    (tensor); g: the M + 1 edges (array or tensor). Returns (env float64 [count, A, dof, M, 2] — NaN for a plan without a
    trajectory —, valid int32 [count], planned bool [count])."""
    import torch
    dev = full.device
    g = torch.as_tensor(np.asarray(g.cpu() if hasattr(g, "cpu") else g).astype(np.int64))
    M = int(g.numel()) - 1
    assert M >= 1
    closed = int(bool(closed))
    arrays = selected(mask)
    A = len(arrays)
    lo_at = (g[:-1] - g[0]).tolist()
    hi_at = (torch.maximum(g[:-1], g[1:] - 1 + closed) - g[0]).tolist()
    span = max(hi_at) + 1
    L = lens[first:first + count].long().to(dev)
    o = offsets[first:first + count].long().to(dev)
    kk = k.long().to(dev).clamp(min=0)
    planned = L > 0
    env = torch.full((count, A, dof, M, 2), float("nan"), dtype=torch.float64, device=dev)
    steps = torch.arange(span, device=dev) + int(g[0])
    rows = torch.tensor([[x * dof + j for j in range(dof)] for x in arrays], device=dev).view(1, A, dof, 1)
    rests = torch.tensor([x > 0 for x in arrays], device=dev).view(1, A, 1, 1)          # v, a, j: +0.0 past the end
    for c0 in range(0, count, chunk):
        c1 = min(count, c0 + chunk)
        Lc = L[c0:c1]
        t = kk[c0:c1, None] + steps[None, :]                                            # [c, span]
        tc = torch.minimum(t, (Lc - 1).clamp(min=0)[:, None])
        stride = (Lc + 31) // 32 * 32
        idx = o[c0:c1].view(-1, 1, 1, 1) + rows * stride.view(-1, 1, 1, 1) + tc[:, None, None, :]
        idx = torch.where(planned[c0:c1].view(-1, 1, 1, 1), idx, torch.zeros_like(idx))
        x = full[idx]                                                                   # [c, A, dof, span]
        past = (t >= Lc[:, None])[:, None, None, :] & rests
        x = torch.where(past, torch.zeros_like(x), x)
        for w in range(M):
            piece = x[..., lo_at[w]:hi_at[w] + 1]
            env[c0:c1, :, :, w, 0] = piece.min(dim=3).values
            env[c0:c1, :, :, w, 1] = piece.max(dim=3).values
    env[~planned] = float("nan")
    return env, valid_formula(L, kk, g[:-1].to(dev)), planned


def expected_q(full, offsets, lens, k, g, closed, dof, first, count, chunk=256):
    """expected(mask = q) without the plane axis: env [count, dof, M, 2], what the q-only call and ltp_envelope_batch return."""
    env, valid, planned = expected(full, offsets, lens, k, g, closed, dof, first, count, mask=ENV_Q, chunk=chunk)
    return env[:, 0], valid, planned


def compare_analytic(got, red, planned):
    """q and v: the project's acceptance rule for an analytic envelope form against reduced rows (tests/test_gpu_edge.py::
    test_analytic_envelopes_agree_with_the_exhaustive_form), per plan, on planes [count, dof, M, 2]: returns (bad [count] bool — the
    NaN pattern differs, a minimum below / a maximum above the samples' own, or |d| > 1e-12 —, worst |d|, share of bit-identical
    values)."""
    import torch
    count = got.shape[0]
    nan_bad = torch.isnan(got) != torch.isnan(red)
    d = torch.nan_to_num((got - red).abs(), nan=0.0)
    outside = (got[..., 0] < red[..., 0]) | (got[..., 1] > red[..., 1])
    bad = nan_bad.reshape(count, -1).any(dim=1) | (d > 1e-12).reshape(count, -1).any(dim=1) | outside.reshape(count, -1).any(dim=1)
    real = ~torch.isnan(red)
    same = (int_view(got.contiguous()) == int_view(red.contiguous())) & real
    share = float(same.sum().item()) / max(int(real.sum().item()), 1)
    return bad, float(d.max().item()) if d.numel() else 0.0, share


def compare_equal(got, red, planned):
    """a and j: the NaN pattern identical and the values EQUAL under == (so -0.0 and +0.0 count as one), per plan: bad [count] bool."""
    import torch
    count = got.shape[0]
    both_nan = torch.isnan(got) & torch.isnan(red)
    return (~((got == red) | both_nan)).reshape(count, -1).any(dim=1)


def compare(got, red, planned, mask=15):
    """Every plane of a call [count, A, dof, M, 2] by its rule. Returns (bad [count] bool, {array name: (worst |d|, bit-identical
    share)} for q and v)."""
    import torch
    bad = torch.zeros(got.shape[0], dtype=torch.bool, device=got.device)
    figures = {}
    for x, arr in enumerate(selected(mask)):
        if arr <= 1:
            b, worst, share = compare_analytic(got[:, x], red[:, x], planned)
            figures[NAMES[arr]] = (worst, share)
        else:
            b = compare_equal(got[:, x], red[:, x], planned)
        bad |= b
    return bad, figures
