"""The yardstick of the horizon readers (ltp_sample_window_batch, ltp_sample_horizon_batch, ltp_sample_knots_batch,
include/ltp_hip.h) — a helper, not a test: what a reader must hold, gathered from the full rows ltp_sample_batch wrote for the same
batch; the `valid` formula; the draw of the starts; and the shares of a batch that reach the cases the kernel treats differently.
It runs on whatever device its tensors live on, so tests/test_horizon_cpu.py and tests/test_knots_cpu.py pin it against plain Python
loops without a GPU and the GPU modules use it on the device.

The three readers have one index rule: element w of a row is trajectory sample t = max(k, 0) + g[w]. The window has g = arange(N)
(window_grid), the strided horizon g = s * arange(N) (stride_grid), a knot grid is its own g (tests/knots_checker.py has the grids
the tests use). Full-row layout of plan p (ltp_sample_batch): offsets[p] + (array * dof + joint) * stride + t with stride =
ltp_row_stride(traj_len) = traj_len rounded up to 32, arrays q, v, a, j."""
import numpy as np

TS = 0.001


def window_grid(N):
    """The grid of the dense window [k, k + N)."""
    return np.arange(N, dtype=np.int64)


def stride_grid(N, s):
    """The grid of the strided horizon k, k + s, ..., k + (N - 1) * s."""
    return int(s) * np.arange(N, dtype=np.int64)


def switch_indices(t_scaled, ts=TS):
    """Sampled switch indices of every (plan, joint, phase): floor for even phases, ceil for odd ones (cc:751-757)."""
    x = np.nan_to_num(t_scaled / ts, nan=0.0, posinf=0.0, neginf=0.0)
    sw = np.where(np.arange(7) % 2 == 0, np.floor(x), np.ceil(x))
    return np.clip(sw, -1, 2 ** 30).astype(np.int64)


def int_view(t):
    import torch
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def expected(full, offsets, lens, k, g, dof, first, count):
    """What the reader of plans [first, first + count) on the grid g must hold, as integers on the device of `full`: element w of a
    row is the full row's element k + g[w] while that is a sample of the trajectory; past the end q is the last sample's and v, a,
    j are +0.0. k: the starts of those `count` plans; g: the offsets (array or tensor). Returns (bits [count, 4, dof, N], valid
    [count], planned [count]); the bits of a plan without a trajectory mean nothing (such a plan must be NaN)."""
    import torch
    dev = full.device
    g = torch.as_tensor(np.asarray(g.cpu() if hasattr(g, "cpu") else g).astype(np.int64)).to(dev)
    L = lens[first:first + count].long()
    o = offsets[first:first + count].long()
    kk = k.long().clamp(min=0)
    t = kk[:, None] + g[None, :]
    real = t < L[:, None]
    tc = torch.minimum(t, (L - 1).clamp(min=0)[:, None])
    stride = (L + 31) // 32 * 32
    rowi = torch.arange(4 * dof, device=dev).view(1, 4, dof, 1)
    idx = o.view(-1, 1, 1, 1) + rowi * stride.view(-1, 1, 1, 1) + tc[:, None, None, :]
    planned = L > 0
    idx = torch.where(planned.view(-1, 1, 1, 1), idx, torch.zeros_like(idx))
    exp = int_view(full)[idx]
    exp[:, 1:] = torch.where(real[:, None, None, :], exp[:, 1:], torch.zeros_like(exp[:, 1:]))
    return exp, valid_formula(L, kk, g), planned


def valid_formula(L, kk, g):
    """The number of w with k + g[w] < traj_len, 0 for traj_len == 0; L, kk: int64 tensors [count], kk already >= 0; g: int64 tensor [N]."""
    import torch
    real = kk[:, None] + g[None, :] < L[:, None]
    return torch.where(L > 0, real.sum(dim=1), torch.zeros_like(L)).int()


def strided_valid(L, kk, N, s):
    """The closed form include/ltp_hip.h documents for the strided horizon (s = 1: the window): min(N, ceil(max(0, traj_len - k) / s)),
    0 for traj_len == 0; L, kk: int64 tensors, kk already >= 0."""
    import torch
    left = (L - kk).clamp(min=0)
    return torch.where(L > 0, ((left + (int(s) - 1)) // int(s)).clamp(max=N), torch.zeros_like(L)).int()


def draw_starts(rng, lens, t_scaled, N, s):
    """k per plan by plan index mod 6, over the span N * s — 0, 1: uniform in [0, traj_len); 2, 3: a switch index of a random
    (joint, phase) minus s times a uniform draw from [0, N), which puts that index ON the grid; 4: uniform in
    [traj_len - N * s, traj_len + N * s); 5: cycling through {0, traj_len - 1, traj_len, traj_len + 5, -3}."""
    n, dof = t_scaled.shape[:2]
    L = lens.astype(np.int64)
    sw = switch_indices(t_scaled)
    kind = np.arange(n) % 6
    uni = rng.integers(0, np.maximum(L, 1))
    tgt = sw[np.arange(n), rng.integers(0, dof, n), rng.integers(0, 7, n)] - s * rng.integers(0, N, n)
    end = L - N * s + rng.integers(0, 2 * N * s, n)
    cyc = np.stack([np.zeros(n, dtype=np.int64), L - 1, L, L + 5, np.full(n, -3)], axis=1)[np.arange(n), (np.arange(n) // 6) % 5]
    k = np.select([kind <= 1, kind <= 3, kind == 4], [uni, tgt, end], cyc)
    return k.astype(np.int32)


def coverage(k, N, s, lens, t_scaled):
    """Four shares of the batch (plans with a trajectory only), span = the samples k .. k + (N - 1) * s:
    on-grid  a switch index exactly on a grid sample k + w * s, w < N, and below traj_len (s = 1: a switch index inside the window);
    skipped  some joint has two consecutive distinct switch indices a < b, both inside the span and trajectory samples, with no
             grid sample in [a, b): the stretch between them is stepped over (s = 1: cannot occur);
    ends     k + (N - 1) * s >= traj_len: the horizon ends past the trajectory;
    starts   k >= traj_len: it starts there."""
    L = lens.astype(np.int64)
    kk = np.maximum(k.astype(np.int64), 0)
    sw = switch_indices(t_scaled)
    has = L > 0
    K, LL = kk[:, None, None], L[:, None, None]
    last = K + (N - 1) * s
    on = (sw >= K) & ((sw - K) % s == 0) & (sw <= last) & (sw < LL)
    srt = np.sort(sw, axis=2)
    a, b = srt[:, :, :-1], srt[:, :, 1:]
    inside = (a >= K) & (b <= last) & (b < LL) & (b > a)
    cell = lambda x: (np.maximum(x - K, 0) + s - 1) // s       # the first grid element at or after x
    skipped = inside & (cell(a) == cell(b))
    return (float(np.mean(on.any(axis=(1, 2)) & has)), float(np.mean(skipped.any(axis=(1, 2)) & has)),
            float(np.mean(has & (last[:, 0, 0] >= L))), float(np.mean(has & (kk >= L))))


def assert_coverage(k, N, s, lens, t_scaled, what):
    """The conditions under which a comparison of bits says something: required shares of the batch, not measurements."""
    on, skipped, ends, starts = coverage(k, N, s, lens, t_scaled)
    planned = float(np.mean(lens > 0))
    print(f"{what}: on-grid {on:.3f}, skipped {skipped:.3f}, ends {ends:.3f}, starts {starts:.3f}, planned {planned:.3f}")
    assert on >= 0.30 and ends >= 0.10 and starts >= 0.03 and planned >= 0.95, (what, on, ends, starts, planned)
    if s > 1 and N >= 32:
        assert skipped >= 0.05, (what, skipped)


def pack_full_rows(trajs, dof):
    """Host plans [(L, q, v, a, j)] with arrays [dof][L] (L == 0: no trajectory) in the full-row layout: (full float64 [total],
    offsets int64 [n + 1], lens int32 [n])."""
    lens = np.array([t[0] for t in trajs], dtype=np.int32)
    stride = (lens.astype(np.int64) + 31) // 32 * 32
    offsets = np.concatenate([[0], np.cumsum(4 * dof * stride)]).astype(np.int64)
    full = np.zeros(max(int(offsets[-1]), 2))
    for p, (L, *arrs) in enumerate(trajs):
        for x, arr in enumerate(arrs):
            for j in range(dof):
                at = int(offsets[p]) + (x * dof + j) * int(stride[p])
                full[at:at + L] = arr[j][:L]
    return full, offsets, lens
