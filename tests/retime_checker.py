"""The checker of ltp_retime_batch (test infrastructure, not a test module): the CPU oracle composed into the retime rule of
include/ltp_hip.h. For every eligible query whose target T_q exceeds its optimum T*, every joint goes through the oracle's
timeScaling (cc:358-645) with T_q, then the fallback of cc:50-55, then traj_len (cc:716-719); every other query keeps the records
Oracle.plan_batch gave it."""
import numpy as np

STATUS_END_LIMIT, STATUS_OVERFLOW = 8, 32


def needs_fallback(t):
    """cc:50-55: max_element(t) <= 0, with std::max_element's scan (a NaN in the first place wins every comparison)."""
    mx = t[0]
    for k in range(1, 7):
        if mx < t[k]:
            mx = t[k]
    return mx <= 0.0


def device_eligible(rec):
    """Eligibility from device records (LTP_STATUS_* bits)."""
    return ((rec["status"] & ~(STATUS_END_LIMIT | STATUS_OVERFLOW)) == 0) & (rec["slowest"] >= 0)


def oracle_eligible(orec):
    """Eligibility from Oracle.plan_batch records (status 1 = planned, before sampling)."""
    return (orec["status"] != 0) & (orec["slowest"] >= 0)


def t_star(rec):
    n = rec["slowest"].shape[0]
    s = np.clip(rec["slowest"], 0, None)
    return rec["t_opt"][np.arange(n), s, 6]


def own_targets(tstar, uniform=0.0, t_target=None):
    """max(T*, t_uniform, t_target[q]); a request wins only by being larger, finite and >= 0."""
    T = tstar.copy()
    T = np.where(uniform > T, uniform, T)
    if t_target is not None:
        r = np.asarray(t_target, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            win = (r > T) & (r >= 0.0) & np.isfinite(r)
        T = np.where(win, r, T)
    return T


def group_times(eligible, own, group, n_groups):
    """group_time[g]: the largest own target of the eligible members of g (0 without such members)."""
    gt = np.zeros(n_groups)
    for q in np.nonzero(eligible)[0]:
        g = int(group[q])
        if 0 <= g < n_groups and own[q] > gt[g]:
            gt[g] = own[q]
    return gt


def targets(rec, eligible, uniform=0.0, t_target=None, group=None, n_groups=0):
    """(T_q for every query, group_time or None); T_q is meaningful where `eligible`."""
    ts = t_star(rec)
    own = own_targets(ts, uniform, t_target)
    if group is None:
        return own, None
    gt = group_times(eligible, own, group, n_groups)
    T = own.copy()
    for q in range(T.size):
        g = int(group[q])
        if 0 <= g < n_groups and gt[g] > T[q]:
            T[q] = gt[g]
    return T, gt


def retime(orc, orec, qg, q0, v0, a0, T):
    """Records of the retime of Oracle.plan_batch's records `orec` to per-query targets T (NaN = none). Returns (records dict,
    retimed mask, per-query accepted-case counts [n][9] (case 0 = fallback))."""
    D = orc.dof
    out = {k: np.array(v, copy=True) for k, v in orec.items() if isinstance(v, np.ndarray)}
    n = qg.shape[0]
    elig = oracle_eligible(orec)
    ts = t_star(orec)
    with np.errstate(invalid="ignore"):
        retimed = elig & (T > ts)
    cases = np.zeros((n, 9), dtype=np.int64)
    for q in np.nonzero(retimed)[0]:
        for j in range(D):
            ok, t, vd, mod, case = orc.time_scaling(j, qg[q, j], q0[q, j], v0[q, j], a0[q, j], orec["dir"][q, j], T[q])
            cases[q, case] += 1
            if needs_fallback(t):
                t = orec["t_opt"][q, j].copy()
            out["t_scaled"][q, j] = t
            out["v_drive"][q, j] = vd
            out["mod"][q, j] = mod
        out["t_required"][q] = T[q]
        out["traj_len"][q] = orc.traj_len(out["t_scaled"][q])
    return out, retimed, cases


def trajectory(orc, rec, q, q0, v0, a0):
    """get_trajectory of query q of a (checker) record set: (length, q, v, a, j)."""
    return orc.get_trajectory(rec["t_scaled"][q], rec["dir"][q], rec["mod"][q], q0[q], v0[q], a0[q], rec["v_drive"][q])
