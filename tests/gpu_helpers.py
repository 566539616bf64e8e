"""What the class-by-class GPU modules share (test infrastructure, not a test module): tests/test_gpu_branches.py (planner branches,
tests/branch_census.py) and tests/test_gpu_runs.py (the sampler's run structure, tests/run_census.py). A planner handle with its
policy set, queries as device tensors, a batch's records on the host, the run-census batches with their full rows (_rows, which
tests/test_gpu_envelope_knots.py reads too), bit comparison, and the yardsticks cut from full rows. R is a dict with "host" (the
full float64 rows on the host), "rec" (the batch's host records) and "dof"."""
import numpy as np

from branch_census import TS

TOL = 1e-9
DEV = "cuda:0"
REC_KEYS = ("t_opt", "t_scaled", "dir", "v_drive", "mod", "t_required", "slowest", "traj_len", "status")


def _planner(dof, lim, ts=TS, pow_rule="libm", semantics="cpp", max_samples=0, stride=1):
    from longtermplanner_amd import LongTermPlanner
    ltp = LongTermPlanner(dof, ts, device=0, **lim)
    ltp.setPowRule(pow_rule)
    ltp.setSemantics(semantics)
    if max_samples:
        ltp.setMaxSamples(max_samples)
    if stride != 1:
        ltp.setSampleStride(stride)
    return ltp


def _tensors(qs, layout="query_major"):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x if layout == "query_major" else x.T)).to(DEV) for x in qs]


def _host(batch):
    import torch
    torch.cuda.synchronize()
    r = {k: getattr(batch, k).cpu().numpy().copy() for k in REC_KEYS}
    r["offsets"] = batch.offsets.cpu().numpy().view(np.uint64).copy()
    return r


_R = {}


def _rows(oracle_mod, name, pow_rule="libm", semantics="cpp"):
    """A named batch of tests/run_census.py planned on the device with its full float64 rows (the fused sampler; MATLAB semantics:
    the table pass), the oracle's records and rows for the same pow rule, and the run census of the oracle's records. Once per
    process."""
    import torch
    import run_census as rc
    key = (name, pow_rule, semantics)
    if key not in _R:
        orc, lim, ts, qs, orec, cen = rc.batch(oracle_mod, name, semantics, exact_pow=(pow_rule == "exact"))
        n, dof = len(orec["status"]), orc.dof
        ltp = _planner(dof, lim, ts, pow_rule=pow_rule, semantics=semantics)
        batch = ltp.planSwitchTimesBatch(*_tensors(qs))
        off = _host(batch)["offsets"]
        full = torch.zeros(int(off[-1]) + 32, dtype=torch.float64, device=DEV)
        ltp.sampleBatchEx(batch, 0, n, full, sampler="fused")
        rec = _host(batch)
        _R[key] = dict(name=name, n=n, dof=dof, ts=ts, lim=lim, qs=qs, orc=orc, orec=orec, cen=cen, ltp=ltp, batch=batch, rec=rec, full=full,
                       host=full.cpu().numpy(), orows=rc.all_rows(oracle_mod, name, semantics, exact_pow=(pow_rule == "exact")))
    return _R[key]


def _agree(a, b, exact):
    """Elementwise: the same bits (or both NaN); without `exact`, floating-point values within 1e-9."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return a == b
    same = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
    if exact:
        return same
    with np.errstate(invalid="ignore"):
        return same | (np.abs(a - b) <= TOL)


def _plan_rows(R, p, length=None):
    from longtermplanner_amd import unpack_trajectory
    L = int(R["rec"]["traj_len"][p])
    return np.stack(unpack_trajectory(R["host"], int(R["rec"]["offsets"][p]), R["dof"], L))     # [4][dof][L]


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    it = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(it), b.view(it))


def _window_expected(R, k, N, stride=1):
    """[n][4][dof][N] from the full rows: element s is sample k + s * stride while that is a sample; past the end q holds the last
    position and v, a, j are +0.0; a plan without a trajectory is NaN. And valid [n]."""
    n, dof = len(R["rec"]["traj_len"]), R["dof"]
    exp = np.full((n, 4, dof, N), np.nan)
    valid = np.zeros(n, dtype=np.int32)
    for p in range(n):
        L = int(R["rec"]["traj_len"][p])
        if L <= 0:
            continue
        rows = _plan_rows(R, p)
        kk = max(int(k[p]), 0)
        idx = kk + np.arange(N) * stride
        real = idx < L
        exp[p] = rows[:, :, np.minimum(idx, L - 1)]
        exp[p, 1:][:, :, ~real] = 0.0
        valid[p] = min(-(-max(L - kk, 0) // stride), N)
    return exp, valid
