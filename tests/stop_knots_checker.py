"""What a stop horizon (ltp_stop_knots_batch, include/ltp_hip.h) must hold, from the CPU oracle alone (test infrastructure, not a
test module, like stop_checker.py). The grids are knots_checker.GRIDS.

expected applies, per element of the knot states, the acceleration rule, the oracle's optBraking, one addition and the running
sum of the phases — nothing else. tests/test_stop_knots_cpu.py pins it by an independent path: stop_checker.expected_stop on the
same states, clamped, gives the same bits."""
import numpy as np

from knots_checker import GRIDS  # noqa: F401  (the grids of the stop-horizon tests)

CLAMP, STRICT = 0, 1      # LTP_STOP_ACCEL_*


def beyond(a, a_max):
    """LTP_STOP_CHECK_BRAKING's comparison per element: |a| > a_max (a NaN is not beyond). a: [n][dof][N]; a_max: [dof] or [n][dof]."""
    am = np.asarray(a_max, dtype=np.float64)
    am = am[None, :, None] if am.ndim == 1 else am[:, :, None]
    with np.errstate(invalid="ignore"):
        return np.abs(a) > am


def clamped(a, a_max):
    """a > a_max ? a_max : (a < -a_max ? -a_max : a) per element; a NaN passes (torch.clamp)."""
    am = np.asarray(a_max, dtype=np.float64)
    am = np.broadcast_to(am[None, :, None] if am.ndim == 1 else am[:, :, None], a.shape)
    with np.errstate(invalid="ignore"):
        return np.where(a > am, am, np.where(a < -am, -am, a))


def expected(orc, rows_at_knots, a_max, accel):
    """rows_at_knots: [n][>= 3][dof][N], the planes q, v, a of the knot states (what ltp_sample_knots_batch stores in elements
    [0, N) of its rows). a_max: [dof], the oracle's own. Returns [n][2][dof][N]: q_stop = q + optBraking's q and t_stop = element
    6 of the running sum of its phases, from (v, a') with a' the clamped acceleration (CLAMP) or a itself (STRICT: NaN in both
    planes where |a| > a_max)."""
    rows = np.asarray(rows_at_knots, dtype=np.float64)
    n, _, dof, N = rows.shape
    q, v, a = rows[:, 0], rows[:, 1], rows[:, 2]
    ab = clamped(a, a_max) if accel == CLAMP else a
    refused = beyond(a, a_max) if accel == STRICT else np.zeros(a.shape, dtype=bool)
    out = np.full((n, 2, dof, N), np.nan)
    for p in range(n):
        for j in range(dof):
            for w in range(N):
                if refused[p, j, w]:
                    continue
                qb, t_rel, _ = orc.opt_braking(j, v[p, j, w], ab[p, j, w])
                s = 0.0
                for x in range(7):                     # the running sum of cc:105 with t_rel[3..6] = 0
                    s = t_rel[x] if x == 0 else s + t_rel[x]
                out[p, 0, j, w] = q[p, j, w] + qb
                out[p, 1, j, w] = s
    return out
