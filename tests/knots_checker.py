"""The grids of the knot-grid horizon tests (ltp_sample_knots_batch, include/ltp_hip.h) and a host-side proxy for "runs parked" —
a helper, not a test. What a horizon on a grid g must hold and its `valid` formula are tests/horizon_checker.py's, for every grid
alike. tests/test_knots_cpu.py pins the stretch logic against a plain Python loop without a GPU, tests/test_gpu_knots.py uses it on
the device.

Element w of a row is trajectory sample t = max(k, 0) + g[w]."""
import numpy as np

from horizon_checker import TS, switch_indices

MAX_KNOTS = 512


def mpc_grid():
    """16 knots one sample apart (0 .. 15), then 12 four apart (16 .. 60), then 12 sixteen apart (64 .. 240): 40 knots over 240 samples."""
    g = list(range(16)) + [16 + 4 * i for i in range(12)] + [64 + 16 * i for i in range(12)]
    assert len(g) == 40 and g[-1] == 240
    return np.array(g, dtype=np.int32)


def geometric_grid(n, last):
    """n geometrically spaced offsets from 0 to `last`, rounded down, duplicates removed."""
    g = np.unique(np.floor(np.concatenate([[0.0], np.geomspace(1.0, float(last), n - 1)])).astype(np.int64))
    return g.astype(np.int32)


def wide_grid():
    """A geometric grid of 200 offsets from 0 to 5999 with duplicates removed (150 knots): whole trajectories, every stretch met."""
    return np.unique(np.floor(np.geomspace(1.0, 6000.0, 200)).astype(np.int64) - 1).astype(np.int32)


GRIDS = {
    "mpc": mpc_grid(),
    "geometric": geometric_grid(70, 4096),
    "duplicates": np.array([0, 0, 1, 5, 5, 5, 9, 30, 30, 31, 100, 100, 250, 251, 251, 400, 1000, 1000], dtype=np.int32),
    "from37": (37 + 3 * np.arange(20) ** 2).astype(np.int32),
    "one": np.array([11], dtype=np.int32),
    "n33": (7 * np.arange(33)).astype(np.int32),
    "n65": (np.arange(65) ** 2 // 3).astype(np.int32),
    "max": (8 * np.arange(MAX_KNOTS)).astype(np.int32),
}
# The grids of the smallest shapes: 25 knots (24 intervals) for batches whose rows have 1 to 153 samples (tests/run_census.py) —
# one sample apart, two apart, and one that holds duplicates and reaches past the longest row.
SMALL_GRIDS = {
    "unit": np.arange(25, dtype=np.int32),
    "two": (2 * np.arange(25)).astype(np.int32),
    "duplicates": np.array([0, 0, 1, 2, 2, 2, 3, 5, 5, 6, 9, 9, 14, 15, 15, 22, 40, 40, 41, 80, 150, 150, 151, 152, 160], dtype=np.int32),
}


def _stretch_counts(k, g, lens, t_scaled, ts=TS):
    """Per (plan, joint): how many distinct stretches hold a real knot, and how many stretches lie from the first to the last of
    them. A stretch lies between consecutive distinct switch indices of the joint, cut at 0 and traj_len; g is non-decreasing, so
    the real knots are a prefix of the grid and their stretch numbers do not decrease."""
    sw = switch_indices(t_scaled, ts)
    g = np.asarray(g, dtype=np.int64)
    L = lens.astype(np.int64)
    n, dof = sw.shape[:2]
    cuts = np.sort(np.concatenate([np.clip(sw, 0, L[:, None, None]), np.zeros((n, dof, 1), dtype=np.int64),
                                   np.broadcast_to(L[:, None, None], (n, dof, 1))], axis=2), axis=2)
    fresh = np.concatenate([np.ones((n, dof, 1), dtype=bool), cuts[:, :, 1:] != cuts[:, :, :-1]], axis=2)      # distinct cuts only
    t = np.maximum(k.astype(np.int64), 0)[:, None] + g[None, :]                                                # [n, N]
    ids = ((cuts[:, :, None, :] <= t[:, None, :, None]) & fresh[:, :, None, :]).sum(axis=3)                    # [n, dof, N]
    real = (t < L[:, None]) & (L > 0)[:, None]
    n_real = real.sum(axis=1)
    changes = ((ids[:, :, 1:] != ids[:, :, :-1]) & real[:, None, 1:]).sum(axis=2)
    held = np.where(n_real[:, None] > 0, changes + 1, 0)
    last = np.take_along_axis(ids, np.broadcast_to(np.maximum(n_real - 1, 0)[:, None, None], (n, dof, 1)), axis=2)[:, :, 0]
    span = np.where(n_real[:, None] > 0, last - ids[:, :, 0] + 1, 0)
    return held, span


def stretches(k, g, lens, t_scaled, ts=TS):
    """Per plan the largest number, over its joints, of distinct stretches that hold a real knot (0 for a plan without a trajectory
    or without a real knot). The kernel's runs are cut at least at the switch indices, so a value above the runs a lane parks per
    pass (6) implies a second pass."""
    return _stretch_counts(k, g, lens, t_scaled, ts)[0].max(axis=1)


def skipped(k, g, lens, t_scaled):
    """Per plan: some joint has, between the first and the last stretch that hold a knot, one that holds none."""
    held, span = _stretch_counts(k, g, lens, t_scaled)
    return (span > held).any(axis=1)


def aimed_starts(k, g, lens, t_scaled):
    """Starts that put a stretch BETWEEN two consecutive knots, for batches whose stretches are long against the grid's span (a
    uniform draw then rarely steps over one). Per plan: a joint's consecutive distinct switch indices a < b, both inside the
    trajectory, and a knot w with g[w] <= a - 1, b - a < g[w + 1] - g[w] and a - 1 + g[w + 1] - g[w] < traj_len; the start
    a - 1 - g[w] puts knot w on sample a - 1 and knot w + 1 at or past b, both real, so the stretch [a, b) holds none. Among a
    plan's candidates one is taken by plan index; a plan without a candidate keeps its start from `k`."""
    sw = np.sort(switch_indices(t_scaled), axis=2)
    g = np.asarray(g, dtype=np.int64)
    gap = np.diff(g)
    out = k.astype(np.int32).copy()
    for p in range(len(lens)):
        L = int(lens[p])
        if L <= 0 or gap.size == 0:
            continue
        a, b = sw[p, :, :-1].ravel(), sw[p, :, 1:].ravel()
        ok = (a > 0) & (b > a) & (b < L)
        A, B = a[ok][:, None], b[ok][:, None]
        cand = np.argwhere((g[None, :-1] <= A - 1) & (B - A < gap[None, :]) & (A - 1 + gap[None, :] < L))
        if len(cand):
            i, w = cand[(p * 7919) % len(cand)]
            out[p] = int(A[i, 0]) - 1 - int(g[w])
    return out


def coverage(k, g, lens, t_scaled):
    """Shares of the batch: planned; horizons that end past traj_len; horizons that start there; plans with a skipped stretch."""
    L = lens.astype(np.int64)
    kk = np.maximum(k.astype(np.int64), 0)
    has = L > 0
    g = np.asarray(g, dtype=np.int64)
    return (float(np.mean(has)), float(np.mean(has & (kk + g[-1] >= L))), float(np.mean(has & (kk + g[0] >= L))),
            float(np.mean(skipped(k, g, lens, t_scaled))))
