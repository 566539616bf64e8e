"""Host-side mirror of the reference's ``LongTermPlanner`` class on top of the C ABI.

Same names, argument meaning and return conventions as
/root/reference/include/long_term_planner/long_term_planner.h:61-308 (constructor, planTrajectory,
checkInputs, setLimits, setSampleTime, setDoF and the four protected methods), plus the batched
calls that are the reason this package exists. Every method runs on the GPU through
libltp_hip.so; nothing here computes planner arithmetic on the host.
"""
import ctypes as C
import numbers
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _abi

_dp = C.POINTER(C.c_double)


def _vec(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))


def _ptr(a):
    return a.ctypes.data_as(_dp)


def _host_records(n, dof):
    """The zeroed record arrays of a *Host / *Sharded call (the result dict) and the ltp_records that points at them."""
    r = dict(t_opt=np.zeros((n, dof, 7)), t_scaled=np.zeros((n, dof, 7)), dir=np.zeros((n, dof)), v_drive=np.zeros((n, dof)),
             mod=np.zeros((n, dof), dtype=np.int8), t_required=np.zeros(n), slowest=np.zeros(n, dtype=np.int32),
             traj_len=np.zeros(n, dtype=np.int32), status=np.zeros(n, dtype=np.int32))
    return r, _abi.Records(*[r[k].ctypes.data for k in _abi.RECORD_FIELDS])   # (written out: a single planTrajectory pays for this)


def _query_arrays(dof, queries, dofless=False):
    """(q_goal, q_0, v_0, a_0) as four contiguous float64 arrays [n, dof] for the C ABI, and n. dofless: a planner without joints
    (the reference's dummy constructor) gets one query of no columns whatever was passed — planBatchHost's form; elsewhere dof = 0
    cannot be reshaped and raises."""
    ins = [np.ascontiguousarray(np.zeros((1, 0)) if dofless and not dof else np.asarray(x, dtype=np.float64).reshape(-1, dof))
           for x in queries]
    return ins, ins[0].shape[0]


def _layout(layout, n, dof):
    """(shape, query_stride, joint_stride) of n queries of dof joints as the device calls take them: "query_major" is [n, dof],
    anything else [dof, n]."""
    return ((n, dof), dof, 1) if layout == "query_major" else ((dof, n), 1, n)


def _take_packed(lib, packed, offsets):
    """numpy copy of the offsets[-1] doubles the library handed out as *packed, which goes back to it (ltp_free_host)."""
    total = int(offsets[-1])
    out = np.ctypeslib.as_array(packed, shape=(max(total, 1),))[:total].copy()
    lib.ltp_free_host(packed)
    return out


@dataclass
class Trajectory:
    """reference struct Trajectory (long_term_planner.h:37-45): q/v/a/j are [joint][sample]."""
    dof: int = 0
    t_sample: float = 0.0
    length: int = 0
    q: List = field(default_factory=list)
    v: List = field(default_factory=list)
    a: List = field(default_factory=list)
    j: List = field(default_factory=list)


def unpack_trajectory(packed, offset, dof, length):
    """Views [dof][length] of q, v, a, j inside a packed buffer (layout: include/ltp_hip.h)."""
    stride = _abi.lib().ltp_row_stride(int(length))
    blk = packed[offset: offset + 4 * dof * stride].reshape(4, dof, stride)
    return blk[0, :, :length], blk[1, :, :length], blk[2, :, :length], blk[3, :, :length]


class DeviceBatch:
    """Device-resident records of one ltp_plan_switch_times_batch call (torch tensors)."""

    def __init__(self, n, dof, device):
        import torch
        f64 = dict(dtype=torch.float64, device=device)
        self.n, self.dof = n, dof
        self.t_opt = torch.empty((n, dof, 7), **f64)
        self.t_scaled = torch.empty((n, dof, 7), **f64)
        self.dir = torch.empty((n, dof), **f64)
        self.v_drive = torch.empty((n, dof), **f64)
        self.mod = torch.empty((n, dof), dtype=torch.int8, device=device)
        self.t_required = torch.empty((n,), **f64)
        self.slowest = torch.empty((n,), dtype=torch.int32, device=device)
        self.traj_len = torch.empty((n,), dtype=torch.int32, device=device)
        self.status = torch.empty((n,), dtype=torch.int32, device=device)
        self.offsets = torch.empty((n + 1,), dtype=torch.int64, device=device)   # uint64 on the device side
        self.limit_set = None   # int32 CUDA tensor [n]: the limit set of each query (planSwitchTimesBatch(limit_set=...)), or None

    def c_records(self):
        return _abi.Records(*[getattr(self, k).data_ptr() for k in _abi.RECORD_FIELDS])


class LongTermPlanner:
    def __init__(self, dof=0, t_sample=0.001, q_min=(), q_max=(), v_max=(), a_max=(), j_max=(), device=0):
        # default arguments reproduce the reference's dummy constructor (long_term_planner.h:103-105)
        self._lib = _abi.lib()
        self._h = C.c_void_p()
        arrs = [_vec(x) for x in (q_min, q_max, v_max, a_max, j_max)]
        for a in arrs:
            if a.size < dof:
                raise ValueError("limit vectors need at least dof entries")
        rc = self._lib.ltp_create(int(dof), float(t_sample), *[_ptr(a) for a in arrs], int(device), C.byref(self._h))
        if rc != _abi.LTP_OK:
            raise _abi.LtpError(rc, "ltp_create failed (no HIP device? the planner has no CPU fallback)")
        self.device = int(device)
        self._a_max, self._set_a_max = arrs[3].copy(), None   # host copies for planStopFrom's clamp (the handle's own, the sets' [K, dof])
        # device copies of host knot grids (sampleKnots), per (content, device of the batch): the grids say nothing about the handle
        # or its batches, so an entry stays right whatever is reconfigured, and a batch on another device gets its own copy
        self._knots_cache = {}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.ltp_destroy(h)
            self._h = None

    def _check(self, rc):
        if rc != _abi.LTP_OK:
            raise _abi.LtpError(rc, (self._lib.ltp_last_error(self._h) or b"").decode())

    # ---- configuration (long_term_planner.h:176-205) ----
    def setLimits(self, q_min, q_max, v_max, a_max, j_max):
        arrs = [_vec(x) for x in (q_min, q_max, v_max, a_max, j_max)]
        n = min(a.size for a in arrs)
        self._check(self._lib.ltp_set_limits(self._h, n, *[_ptr(a) for a in arrs]))
        self._a_max = arrs[3].copy()

    def setLimitSets(self, q_min, q_max, v_max, a_max, j_max):
        """NEW: limit sets (ltp_set_limit_sets): five arrays of shape [K, dof], set s = row s; all None removes the sets. A batch planned
        with planSwitchTimesBatch(..., limit_set=idx) or planBatchHost(..., limit_set=idx) gives query q exactly what a planner whose
        limits are set idx[q] gives it (include/ltp_hip.h)."""
        arrs = (q_min, q_max, v_max, a_max, j_max)
        if all(a is None for a in arrs):
            self._check(self._lib.ltp_set_limit_sets(self._h, 0, None, None, None, None, None))
            self._set_a_max = None
            return
        if any(a is None for a in arrs):
            raise ValueError("setLimitSets: give all five arrays, or None for all of them")
        arrs = [np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in arrs]
        D = self.dof
        if any(a.ndim != 2 or a.shape != arrs[0].shape for a in arrs) or arrs[0].shape[1] != D or arrs[0].shape[0] < 1:
            raise ValueError(f"setLimitSets: five arrays of one shape [K >= 1, dof = {D}] expected, got {[a.shape for a in arrs]}")
        self._check(self._lib.ltp_set_limit_sets(self._h, arrs[0].shape[0], *[_ptr(a) for a in arrs]))
        self._set_a_max = arrs[3].copy()

    @property
    def limitSets(self):
        """NEW: the number of limit sets (setLimitSets)."""
        return self._lib.ltp_get_limit_sets(self._h)

    def _bind(self, batch):
        """Bind the batch's limit-set index (or none) before a device-pointer batch call: Python users never bind themselves."""
        ix = getattr(batch, "limit_set", None)
        self._check(self._lib.ltp_bind_limit_sets(self._h, ix.data_ptr() if ix is not None else None))

    def setSampleTime(self, t_sample):
        self._check(self._lib.ltp_set_sample_time(self._h, float(t_sample)))

    def setDoF(self, dof):
        self._check(self._lib.ltp_set_dof(self._h, int(dof)))

    def setMaxSamples(self, max_samples):
        """NEW: store only the first max_samples samples of every trajectory; 0 = all (reference)."""
        self._check(self._lib.ltp_set_max_samples(self._h, int(max_samples)))

    def setSampleStride(self, stride):
        """NEW: store every stride-th sample (0, stride, 2*stride, ...); 1 = every sample (reference)."""
        self._check(self._lib.ltp_set_sample_stride(self._h, int(stride)))

    def setGoalCheck(self, enabled=True):
        """NEW, off by default: reject queries whose q_goal lies outside [q_min, q_max] up front with
        LTP_STATUS_GOAL_OUTSIDE (64) instead of planning them and failing the end-limit check (cc:59-61)."""
        self._check(self._lib.ltp_set_goal_check(self._h, 1 if enabled else 0))

    def setSemantics(self, semantics):
        """NEW: "cpp" (default: src/long_term_planner.cc, the parity reference) or "matlab" (the MATLAB original
        LTPlanner.m where it diverges: positional root picks, zeros instead of failures, no position limits, 1-based sampler with
        cumsum integration; include/ltp_hip.h LTP_SEMANTICS_MATLAB)."""
        code = {"cpp": _abi.SEMANTICS_CPP, "matlab": _abi.SEMANTICS_MATLAB}.get(semantics, semantics)
        self._check(self._lib.ltp_set_semantics(self._h, int(code)))

    def setEnvelopeMode(self, mode):
        """NEW: "analytic" (default since round 6: the samples at the ends of each run stretch and either side of the
        roots of q'(m), a few evaluations per run; identical to the exhaustive form in 8.8e9 soaked values, <= 1e-12 by construction) or
        "exhaustive" (every sample of a window: the bits of the reduced rows by construction)."""
        code = {"exhaustive": 0, "analytic": 1}.get(mode, mode)
        self._check(self._lib.ltp_set_envelope_mode(self._h, int(code)))

    def setPowRule(self, rule):
        """NEW: how the reference's pow(x, 3 | 4 | 6) and pow(x, 1.0 / 2) are formed — "libm" (default: glibc's pow restated operation
        for operation: the bits of a reference built with gcc + glibc on an FMA host; include/ltp_hip.h LTP_POW_LIBM) or "exact"
        (one rounding of the exact product, sqrt: within 1 ulp of any libm, faster stage kernels)."""
        code = {"exact": _abi.POW_EXACT, "libm": _abi.POW_LIBM}.get(rule, rule)
        self._check(self._lib.ltp_set_pow_rule(self._h, int(code)))

    def lastMatlabFlags(self):
        """MATLAB semantics: flags of the latest one-lane call (optBraking / optSwitchTimes / timeScaling): 1 = complex intermediate, 2 = error."""
        return self._lib.ltp_debug_last_matlab_flags(self._h)

    def matlabRoots(self, poly):
        """MATLAB's roots() as the MATLAB-semantics kernels compute it (device): (complex roots [n][degree] in MATLAB's order, nroots, status)."""
        poly = np.ascontiguousarray(np.atleast_2d(np.asarray(poly, dtype=np.float64)))
        n, deg = poly.shape[0], poly.shape[1] - 1
        re = np.zeros((n, deg)); im = np.zeros((n, deg)); nr = np.zeros(n, dtype=np.int32); st = np.zeros(n, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        self._check(self._lib.ltp_debug_roots_matlab_host(self._h, n, deg, _ptr(poly), _ptr(re), _ptr(im), nr.ctypes.data_as(ip), st.ctypes.data_as(ip)))
        return re + 1j * im, nr, st

    def setTablePass(self, mode, workspace_bytes=None):
        """NEW: where the run tables are built (include/ltp_hip.h, ltp_set_table_pass) — 0 automatic; 1 never the block-wide fused
        build (rows: k_sample_walk_*, envelopes: the table pass); -1 always the fused build (rows: k_sample, envelopes: in the
        kernel). Results are bit-identical either way."""
        self._check(self._lib.ltp_set_table_pass(self._h, int(mode)))
        if workspace_bytes is not None:
            self._check(self._lib.ltp_set_table_workspace(self._h, int(workspace_bytes)))

    def storedSamples(self, traj_len):
        return self._lib.ltp_stored_samples(self._h, int(traj_len))

    @property
    def dof(self):
        return self._lib.ltp_get_dof(self._h)

    @property
    def t_sample(self):
        return self._lib.ltp_get_sample_time(self._h)

    # ---- the reference's public calls ----
    def checkInputs(self, q_0, v_0, a_0):
        ok = C.c_int()
        self._check(self._lib.ltp_check_inputs_host(self._h, _ptr(_vec(q_0)), _ptr(_vec(v_0)), _ptr(_vec(a_0)), C.byref(ok)))
        return bool(ok.value)

    def planTrajectory(self, q_goal, q_0, v_0, a_0, traj: Trajectory):
        """long_term_planner.h:144-150 / src/long_term_planner.cc:7-63. `traj` is overwritten only if the
        reference would have overwritten it (status has none of the pre-sampling failure bits)."""
        r = self.planBatchHost(q_goal, q_0, v_0, a_0, sample=True)
        st = int(r["status"][0])
        if st & _abi.STATUS_BEFORE_SAMPLING:
            return False
        n = int(r["traj_len"][0])
        q, v, a, j = unpack_trajectory(r["packed"], int(r["offsets"][0]), self.dof, n)
        traj.dof, traj.t_sample, traj.length = self.dof, self.t_sample, n
        traj.q, traj.v, traj.a, traj.j = q.copy(), v.copy(), a.copy(), j.copy()
        return (st & ~_abi.STATUS_MATLAB_COMPLEX) == 0   # the informational MATLAB bit does not make a plan fail

    # ---- the reference's protected methods (exposed to tests through a subclass there) ----
    def optBraking(self, joint, v_0, a_0, t_rel=None):
        t = np.zeros(7) if t_rel is None else np.array(t_rel, dtype=np.float64)
        q = C.c_double(); d = C.c_double()
        self._check(self._lib.ltp_opt_braking_host(self._h, int(joint), float(v_0), float(a_0), C.byref(q), _ptr(t), C.byref(d)))
        return True, q.value, t, d.value

    def optSwitchTimes(self, joint, q_goal, q_0, v_0, a_0, v_drive, t=None):
        tt = np.zeros(7) if t is None else np.array(t, dtype=np.float64)
        d = C.c_double(); m = C.create_string_buffer(1); ok = C.c_int()
        self._check(self._lib.ltp_opt_switch_times_host(self._h, int(joint), float(q_goal), float(q_0), float(v_0), float(a_0),
                                                        float(v_drive), _ptr(tt), C.byref(d), m, C.byref(ok)))
        return bool(ok.value), tt, d.value, m.raw[0]

    def timeScaling(self, joint, q_goal, q_0, v_0, a_0, dir_, t_required, scaled_t=None):
        tt = np.zeros(7) if scaled_t is None else np.array(scaled_t, dtype=np.float64)
        vd = C.c_double(); m = C.create_string_buffer(1); ok = C.c_int(); case = C.c_int()
        self._check(self._lib.ltp_time_scaling_host(self._h, int(joint), float(q_goal), float(q_0), float(v_0), float(a_0),
                                                    float(dir_), float(t_required), _ptr(tt), C.byref(vd), m, C.byref(ok),
                                                    C.byref(case)))
        return bool(ok.value), tt, vd.value, m.raw[0], case.value

    def getTrajectory(self, t, dir_, mod_jerk_profile, q_0, v_0, a_0, v_drive):
        r = self.getTrajectoryBatchHost(np.asarray(t, dtype=np.float64).reshape(1, self.dof, 7), dir_, mod_jerk_profile, q_0, v_0, a_0, v_drive)
        n = int(r["traj_len"][0])
        q, v, a, j = unpack_trajectory(r["packed"], 0, self.dof, n)
        return Trajectory(self.dof, self.t_sample, n, q.copy(), v.copy(), a.copy(), j.copy())

    # ---- batched host-pointer calls (numpy in, numpy out; synchronous) ----
    def planBatchHost(self, q_goal, q_0, v_0, a_0, sample=True, duration=None, limit_set=None):
        """duration (NEW): None plans as the reference does; a number or an [n] array asks every query / each query to take that
        long (ltp_plan_retimed_host: plan, ltp_retime_batch, sample; a request at or below a query's optimum leaves it as planned).
        limit_set (NEW): [n] int array, query q uses set limit_set[q] of setLimitSets (ltp_plan_batch_sets_host)."""
        ins, n = _query_arrays(self.dof, (q_goal, q_0, v_0, a_0), dofless=True)
        if limit_set is not None:
            if duration is not None:
                raise ValueError("planBatchHost: duration and limit_set together are not supported")
            ix = np.ascontiguousarray(np.asarray(limit_set, dtype=np.int32).reshape(n))
            return self._plan_host(self._lib.ltp_plan_batch_sets_host, (self._h,), n, ins, (ix.ctypes.data_as(C.POINTER(C.c_int)),), sample)
        if duration is None:
            return self._plan_host(self._lib.ltp_plan_batch_host, (self._h,), n, ins, (), sample)
        per_query = np.ndim(duration) > 0
        target = np.ascontiguousarray(np.asarray(duration, dtype=np.float64).reshape(n)) if per_query else None
        return self._plan_host(self._lib.ltp_plan_retimed_host, (self._h,), n, ins,
                               (_ptr(target) if per_query else None, 0.0 if per_query else float(duration)), sample)

    def _plan_host(self, entry, handles, n, ins, args, sample, tail=()):
        """The frame of the host planners (ins: their [n, dof] input arrays): zeroed records and offsets, entry(*handles, n, *inputs,
        *args, &records, *tail, offsets, &packed or NULL), check; the records dict with "offsets" and, when sampled, "packed"."""
        r, rec = _host_records(n, ins[0].shape[1])
        offsets = np.zeros(n + 1, dtype=np.uint64)
        packed = _dp()
        self._check(entry(*handles, n, *[_ptr(x) for x in ins], *args, C.byref(rec), *tail, offsets.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                          C.byref(packed) if sample else None))
        r["offsets"] = offsets
        if sample:
            r["packed"] = _take_packed(self._lib, packed, offsets)
        return r

    def planEnvelopeHost(self, q_goal, q_0, v_0, a_0, window, n_windows):
        """NEW: stages 1-3 + on-device envelope consumer for numpy arrays (ltp_plan_envelope_host). Returns (records dict,
        env[n][dof][n_windows][2])."""
        D = self.dof
        ins, n = _query_arrays(D, (q_goal, q_0, v_0, a_0))
        r, rec = _host_records(n, D)
        env = np.zeros((n, D, int(n_windows), 2))
        self._check(self._lib.ltp_plan_envelope_host(self._h, n, *[_ptr(x) for x in ins], int(window), int(n_windows), C.byref(rec), _ptr(env)))
        return r, env

    def getTrajectoryBatchHost(self, t, dir_, mod, q_0, v_0, a_0, v_drive):
        D = self.dof
        t = np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(-1, D, 7))
        n = t.shape[0]
        f = [np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(n, D)) for x in (dir_, q_0, v_0, a_0, v_drive)]
        modb = np.ascontiguousarray(np.asarray(mod, dtype=np.int8).reshape(n, D))
        traj_len = np.zeros(n, dtype=np.int32); status = np.zeros(n, dtype=np.int32)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        packed = _dp()
        self._check(self._lib.ltp_get_trajectory_host(self._h, n, _ptr(t), _ptr(f[0]), modb.ctypes.data_as(C.POINTER(C.c_byte)),
                                                      _ptr(f[1]), _ptr(f[2]), _ptr(f[3]), _ptr(f[4]),
                                                      traj_len.ctypes.data_as(C.POINTER(C.c_int)), status.ctypes.data_as(C.POINTER(C.c_int)),
                                                      offsets.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(packed)))
        return dict(traj_len=traj_len, status=status, offsets=offsets, packed=_take_packed(self._lib, packed, offsets))

    @staticmethod
    def planBatchSharded(planners, q_goal, q_0, v_0, a_0, sample=True):
        """NEW: one process, several devices. `planners`: identically configured LongTermPlanner objects,
        normally one per device; shard g plans the contiguous query range shard_range(n, g, len(planners)) on its own
        device and host thread (ltp_plan_batch_multi); the result dict is that of ONE planBatchHost call over all queries."""
        one = planners[0]
        ins, n = _query_arrays(one.dof, (q_goal, q_0, v_0, a_0))
        return one._plan_host(one._lib.ltp_plan_batch_multi, (LongTermPlanner._multi_handles(planners), len(planners)), n, ins, (), sample)

    @staticmethod
    def _multi_handles(planners):
        """The handle array of a *_multi call. The sharded entries take no limit sets (include/ltp_hip.h): a binding that an earlier
        planSwitchTimesBatch(limit_set=...) left on a planner is removed first, so the Python user, who never binds, is not refused."""
        for pl in planners:
            pl._check(pl._lib.ltp_bind_limit_sets(pl._h, None))
        return (C.c_void_p * len(planners))(*[pl._h for pl in planners])

    # ---- device-resident shards, one process: k planners, per-shard torch tensors, no host copies ----
    @staticmethod
    def _shard_args(planners, batches, streams=None):
        handles = LongTermPlanner._multi_handles(planners)
        shards = (_abi.Shard * len(planners))()
        for g, (pl, b) in enumerate(zip(planners, batches)):
            shards[g].in_ = b.queries
            shards[g].out = b.c_records()
            shards[g].offsets = b.offsets.data_ptr()
            shards[g].stream = streams[g].cuda_stream if streams is not None else pl._stream().value
        return handles, shards

    @staticmethod
    def planSwitchTimesSharded(planners, shard_inputs, n, layout="query_major", batches=None, end_limit=False, streams=None):
        """NEW: ltp_plan_switch_times_multi. shard_inputs[g] = (q_goal, q_0, v_0, a_0) CUDA tensors of shard g — the queries
        shard_range(n, g, k) of one batch of n — on planners[g]'s device. Returns the per-shard DeviceBatch list; the work
        is enqueued on streams[g] (default: each device's current stream), not waited for."""
        k = len(planners)
        if batches is None:
            batches = [None] * k
        out = []
        for g, (pl, ins) in enumerate(zip(planners, shard_inputs)):
            cnt, q = LongTermPlanner._queries(*ins, layout)
            out.append(pl._adopt(batches[g], cnt, q, ins, None))
        handles, shards = LongTermPlanner._shard_args(planners, out, streams)
        planners[0]._check(planners[0]._lib.ltp_plan_switch_times_multi(handles, k, int(n), shards, 1 if end_limit else 0))
        return out

    @staticmethod
    def envelopeSharded(planners, batches, n, window, n_windows, outs=None, streams=None):
        """NEW: ltp_envelope_multi over the shards planned by planSwitchTimesSharded; returns per-shard [count, dof, n_windows, 2]."""
        import torch
        k = len(planners)
        if outs is None:
            outs = [torch.empty((b.n, pl.dof, n_windows, 2), dtype=torch.float64, device=b.offsets.device) for pl, b in zip(planners, batches)]
        handles, shards = LongTermPlanner._shard_args(planners, batches, streams)
        envs = (C.c_void_p * k)(*[o.data_ptr() for o in outs])
        planners[0]._check(planners[0]._lib.ltp_envelope_multi(handles, k, int(n), shards, int(window), int(n_windows), envs))
        return outs

    @staticmethod
    def stateAtSharded(planners, batches, n, sample_index, streams=None, outs=None):
        """NEW: ltp_state_at_multi; sample_index: int, or a list of per-shard int32 CUDA tensors. Returns per shard [q, v, a]
        laid out like the shard's queries (outs: reuse these tensors — with side streams, buffers that are allocated once
        are the safe choice: the caching allocator does not know about work pending on another stream)."""
        import torch
        k = len(planners)
        if outs is None:
            outs = [[torch.empty_like(b.inputs[1]) for _ in range(3)] for b in batches]
        handles, shards = LongTermPlanner._shard_args(planners, batches, streams)
        per = None if isinstance(sample_index, int) else (C.c_void_p * k)(*[x.data_ptr() for x in sample_index])
        ptrs = [(C.c_void_p * k)(*[o[i].data_ptr() for o in outs]) for i in range(3)]
        planners[0]._check(planners[0]._lib.ltp_state_at_multi(handles, k, int(n), shards, per, sample_index if per is None else 0, *ptrs))
        return outs

    @staticmethod
    def synchronizeSharded(planners, batches, streams=None):
        handles, shards = LongTermPlanner._shard_args(planners, batches, streams)
        planners[0]._check(planners[0]._lib.ltp_synchronize_multi(handles, len(planners), shards))

    @staticmethod
    def planEnvelopeSharded(planners, q_goal, q_0, v_0, a_0, window, n_windows):
        """NEW: planEnvelopeHost over several planners / devices from one process (ltp_plan_envelope_multi_host)."""
        lib = planners[0]._lib
        D = planners[0].dof
        ins, n = _query_arrays(D, (q_goal, q_0, v_0, a_0))
        r, rec = _host_records(n, D)
        env = np.zeros((n, D, int(n_windows), 2))
        handles = LongTermPlanner._multi_handles(planners)
        planners[0]._check(lib.ltp_plan_envelope_multi_host(handles, len(planners), n, *[_ptr(x) for x in ins], int(window), int(n_windows),
                                                           C.byref(rec), _ptr(env)))
        return r, env

    def lastSamplerKernel(self):
        """Name of the kernel that wrote the rows / envelopes of this handle's latest sampleBatch / envelopeBatch call."""
        return (self._lib.ltp_last_sampler_kernel(self._h) or b"").decode()

    def reserveTables(self, n):
        self._check(self._lib.ltp_reserve_tables(self._h, int(n)))

    # ---- batched device calls (torch CUDA tensors, asynchronous on torch's current stream) ----
    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _queries(q_goal, q_0, v_0, a_0, layout):
        n, D = (q_0.shape if layout == "query_major" else q_0.shape[::-1])
        _, sq, sj = _layout(layout, n, D)
        for x in (q_goal, q_0, v_0, a_0):
            assert x.is_cuda and x.is_contiguous() and x.dtype.is_floating_point and x.element_size() == 8
        return n, _abi.Queries(q_goal.data_ptr(), q_0.data_ptr(), v_0.data_ptr(), a_0.data_ptr(), sq, sj)

    def generateQueries(self, n, seed=12345, first_query=0, layout="query_major"):
        """Synthetic batch on the device (ltp_generate_queries_batch); returns q_goal, q_0, v_0, a_0."""
        import torch
        shape, sq, sj = _layout(layout, n, self.dof)
        out = [torch.empty(shape, dtype=torch.float64, device=f"cuda:{self.device}") for _ in range(4)]
        self._check(self._lib.ltp_generate_queries_batch(self._h, n, seed, first_query, *[x.data_ptr() for x in out], sq, sj, self._stream()))
        return out

    def planSwitchTimesBatch(self, q_goal, q_0, v_0, a_0, layout="query_major", batch: Optional[DeviceBatch] = None,
                             end_limit=False, limit_set=None):
        """Stages 1-3 + traj_len + packed offsets for a device batch (ltp_plan_switch_times_batch). end_limit=True also
        runs planTrajectory's end-limit check (cc:59-61) without sampling (ltp_end_limit_batch), so that status == 0 is
        exactly planTrajectory's bool; sampleBatch / envelopeBatch apply that check themselves. limit_set (NEW): int32 CUDA
        tensor [n], query q uses set limit_set[q] of setLimitSets; kept on the batch (unchanged until its last consumer call),
        which every consumer wrapper binds again."""
        n, q = self._queries(q_goal, q_0, v_0, a_0, layout)
        batch = self._adopt(batch, n, q, (q_goal, q_0, v_0, a_0), limit_set)
        return self._plan_device(self._lib.ltp_plan_switch_times_batch, batch, (), end_limit)

    def _adopt(self, batch, n, queries, inputs, limit_set):
        """The DeviceBatch a device planner fills: `batch` if it has the shape, else a new one; it keeps the query struct, the input
        tensors (the readers read q_0/v_0/a_0 again: the tensors stay alive with the batch) and the limit-set index (checked here)."""
        import torch
        if limit_set is not None and not (limit_set.is_cuda and limit_set.is_contiguous() and limit_set.dtype == torch.int32
                                          and limit_set.numel() == n):
            raise ValueError("limit_set: a contiguous int32 CUDA tensor of n entries expected")
        if batch is None or batch.n != n or batch.dof != self.dof:
            batch = DeviceBatch(n, self.dof, inputs[1].device)
        batch.queries, batch.inputs, batch.limit_set = queries, inputs, limit_set
        return batch

    def _plan_device(self, entry, batch, opts, end_limit):
        """The tail of a device planner: bind the batch's limit sets, entry(h, n, &queries, &records, *opts, offsets, stream), check,
        and planTrajectory's end-limit verdict if asked for."""
        self._bind(batch)
        rec = batch.c_records()
        self._check(entry(self._h, batch.n, C.byref(batch.queries), C.byref(rec), *opts, batch.offsets.data_ptr(), self._stream()))
        if end_limit:
            self.endLimit(batch, 0, batch.n)
        return batch

    def retimeBatch(self, batch: DeviceBatch, t_target=None, uniform=0.0, group=None, n_groups=None):
        """NEW: retime a batch planned by planSwitchTimesBatch in place (ltp_retime_batch; the rules are in include/ltp_hip.h):
        each eligible query takes max(its optimum, uniform, t_target[q], its group's time). t_target: float64 CUDA tensor [n] or
        None; group: int32 CUDA tensor [n] of group ids or None (ids outside [0, n_groups) = no group; n_groups defaults to
        max(group) + 1). Returns the float64 tensor [n_groups] of group times when groups are given, else None. Asynchronous on
        torch's current stream, like the other batch calls."""
        import torch
        gt = None
        if group is not None:
            assert group.is_cuda and group.is_contiguous() and group.dtype == torch.int32 and group.numel() == batch.n
            if n_groups is None:
                n_groups = int(group.max().item()) + 1 if batch.n else 1
            gt = torch.empty((max(int(n_groups), 1),), dtype=torch.float64, device=batch.offsets.device)
        if t_target is not None:
            assert t_target.is_cuda and t_target.is_contiguous() and t_target.dtype == torch.float64 and t_target.numel() == batch.n
        o = _abi.RetimeOpts(C.sizeof(_abi.RetimeOpts), t_target.data_ptr() if t_target is not None else None, float(uniform),
                            group.data_ptr() if group is not None else None, int(n_groups) if group is not None else 0,
                            gt.data_ptr() if gt is not None else None)
        self._bind(batch)
        rec = batch.c_records()
        self._check(self._lib.ltp_retime_batch(self._h, batch.n, C.byref(batch.queries), C.byref(rec), C.addressof(o),
                                               batch.offsets.data_ptr(), self._stream()))
        return gt

    def planStopBatch(self, q_0, v_0, a_0, layout="query_major", batch: Optional[DeviceBatch] = None, check="inputs", limit_set=None,
                      end_limit=False):
        """NEW: stop plans (ltp_plan_stop_batch; the contract is in include/ltp_hip.h): every joint of every query brakes to rest as
        hard as it may, by optBraking, from the state (q_0, v_0, a_0). Returns a DeviceBatch like planSwitchTimesBatch's that also
        holds `q_stop`, the standstill positions laid out like the states (NaN for a rejected query); batch.inputs keeps (q_stop, q_0,
        v_0, a_0). Every consumer wrapper (sampleBatchEx, sampleWindow, sampleKnots, envelopeKnots, stateAt, endLimit, ...) takes the
        batch unchanged; retimeBatch refuses it. check: "inputs" = checkInputs as planTrajectory applies it, "braking" = only
        |a_0| > a_max. q_stop is optBraking's closed form; the last sampled position is getTrajectory's and differs from it by the
        discretisation."""
        import torch
        n, q = self._queries(q_0, q_0, v_0, a_0, layout)
        q_stop = getattr(batch, "q_stop", None)
        if q_stop is None or q_stop.shape != q_0.shape or q_stop.device != q_0.device:
            q_stop = torch.empty_like(q_0)
        q.q_goal = q_stop.data_ptr()      # no reader reads the goal; a caller who looks at it finds the standstill position
        batch = self._adopt(batch, n, q, (q_stop, q_0, v_0, a_0), limit_set)
        if check not in _abi.STOP_CHECKS:
            raise ValueError(f"check: one of {sorted(_abi.STOP_CHECKS)} expected, got {check!r}")
        batch.q_stop = q_stop
        o = _abi.StopOpts(C.sizeof(_abi.StopOpts), _abi.STOP_CHECKS[check], q_stop.data_ptr())
        return self._plan_device(self._lib.ltp_plan_stop_batch, batch, (C.addressof(o),), end_limit)

    def _a_max_of(self, limit_set, dev):
        """a_max per joint as a float64 tensor on `dev`: [dof] of the handle's own limits, or [count, dof] of each query's limit set."""
        import torch
        if limit_set is None:
            return torch.as_tensor(self._a_max[:self.dof], dtype=torch.float64, device=dev)
        if self._set_a_max is None:
            raise ValueError("the batch has a limit-set index but the planner has no limit sets (setLimitSets)")
        return torch.as_tensor(self._set_a_max, dtype=torch.float64, device=dev)[limit_set.long()]

    def planStopFrom(self, batch: DeviceBatch, first, count, sample_index, clamp_acceleration=True, check="braking", layout="query_major",
                     stop_batch: Optional[DeviceBatch] = None, end_limit=False):
        """NEW, the shield's call: stop plans from where plans [first, first+count) of a planned batch are at trajectory sample
        `sample_index` (int or int32 CUDA tensor [count]): stateAt, then optionally torch.clamp of the acceleration to +-a_max per
        joint (per limit set when the batch has an index), then planStopBatch, all on the current stream.
        Why the clamp exists: sampled accelerations of the reference's own trajectories exceed a_max — by rounding (about 1e-15
        relative) somewhere in most plans, and by discretisation up to a few percent (panda limits at 1 ms: a_max / j_max is two
        samples). With |a_0| > a_max optBraking's first phase (a_max - a_0) / j_max is negative and the reference's sampler would
        index below zero, so the library rejects such a state in both check modes and alters nothing silently; this wrapper offers
        the clamp by name. With the clamp the stop rows START FROM THE CLAMPED ACCELERATION, not from the sampled one (q and v are
        the sampled ones). check defaults to "braking": mid-trajectory states also fail checkInputs' other rules now and then (q at
        the range's edge, the third rule), which does not make their braking profile undefined. Returns the stop batch."""
        import torch
        q0, v0, a0 = self.stateAt(batch, first, count, sample_index, layout=layout)
        ls =batch.limit_set[first:first + count] if getattr(batch, "limit_set", None) is not None else None
        if clamp_acceleration:
            am = self._a_max_of(ls, a0.device)
            if layout != "query_major":
                am = am.t().contiguous() if am.dim() == 2 else am[:, None]
            a0 = torch.clamp(a0, min=-am, max=am).contiguous()
        return self.planStopBatch(q0, v0, a0, layout=layout, batch=stop_batch, check=check, limit_set=ls, end_limit=end_limit)

    def planStopHost(self, q_0, v_0, a_0, sample=True, check="inputs"):
        """NEW: stop plans for numpy states [n, dof] (ltp_plan_stop_host: the stop plan, then the sampler or the end-limit check).
        Returns the records dict of planBatchHost plus "q_stop" [n, dof] (NaN for a rejected query)."""
        ins, n = _query_arrays(self.dof, (q_0, v_0, a_0))
        q_stop = np.zeros((n, self.dof))
        r = self._plan_host(self._lib.ltp_plan_stop_host, (self._h,), n, ins, (_abi.STOP_CHECKS[check],), sample, tail=(_ptr(q_stop),))
        r["q_stop"] = q_stop
        return r

    def endLimit(self, batch: DeviceBatch, first, count):
        """planTrajectory's end-limit check (cc:59-61) for plans [first, first+count) without sampling (ltp_end_limit_batch)."""
        self._bind(batch)
        rec = batch.c_records()
        self._check(self._lib.ltp_end_limit_batch(self._h, first, count, C.byref(batch.queries), C.byref(rec), self._stream()))

    def sampleBatch(self, batch: DeviceBatch, first, count, out, streaming=True, dry=False, spread=0, tables=None, walk=None, auto_waves=None, verdict=True):
        """getTrajectory for plans [first, first+count) into the float64 CUDA tensor `out` (ltp_sample_batch).
        dry=True is a diagnostic: same stores, no arithmetic (ceiling of the store pattern). tables: None = automatic, True / False =
        force the table pass / the fused build; walk: None = automatic, True / False = force / forbid k_sample_walk_* (run tables built
        inside the sampler's block: by itself for capped, float32 and sparse rows and in MATLAB semantics); auto_waves=False keeps
        the walk kernel's builder / streaming-wave form also for caps of at most 32 samples (flag bit 7; by itself: k_sample_walk_auto_*);
        verdict=False (flag bit 4): capped rows without the end-limit verdict — the walk kernels stop at the cap, STATUS_END_LIMIT is then
        not formed by this call (same rows)."""
        import torch
        self._bind(batch)
        rec = batch.c_records()
        fn = self._lib.ltp_sample_batch_f32 if out.dtype == torch.float32 else self._lib.ltp_sample_batch   # float32 tile -> float rows
        assert out.dtype in (torch.float32, torch.float64)
        self._check(fn(self._h, first, count, C.byref(batch.queries), C.byref(rec), batch.offsets.data_ptr(),
                       out.data_ptr(), out.numel(), (1 if streaming else 0) | (2 if dry else 0) | (int(spread) << 8)
                       | (0 if tables is None else (4 if tables else 8)) | (0 if walk is None else (64 if walk else 32)) | (128 if auto_waves is False else 0) | (0 if verdict else 16), self._stream()))

    SAMPLERS = {"auto": 0, "fused": 1, "walk": 2, "walk_streaming": 3, "table": 4}

    def sampleBatchEx(self, batch: DeviceBatch, first, count, out, sampler="auto", nontemporal=True, verdict=True, interleave=0, dry=False):
        """getTrajectory for plans [first, first+count) through ltp_sample_batch_ex: the policy as the named fields of ltp_sample_opts
        (sampler: "auto" | "fused" | "walk" | "walk_streaming" | "table"). The same rows whatever the fields say."""
        import torch
        from ._abi import SampleOpts
        assert out.dtype in (torch.float32, torch.float64)
        o = SampleOpts(C.sizeof(SampleOpts), 1 if out.dtype == torch.float32 else 0, 0 if nontemporal else 1, self.SAMPLERS[sampler],
                       0 if verdict else 1, int(interleave), 1 if dry else 0)
        self._bind(batch)
        rec = batch.c_records()
        self._check(self._lib.ltp_sample_batch_ex(self._h, first, count, C.byref(batch.queries), C.byref(rec), batch.offsets.data_ptr(),
                                                  out.data_ptr(), out.numel(), C.addressof(o), self._stream()))

    def envelopeBatch(self, batch: DeviceBatch, first, count, window, n_windows, out=None):
        """NEW (on-device consumer): [count, dof, n_windows, 2] = min / max of q over windows of `window`
        samples of plans [first, first+count), without storing the trajectories (ltp_envelope_batch)."""
        import torch
        if out is None:
            out = torch.empty((count, self.dof, n_windows, 2), dtype=torch.float64, device=batch.offsets.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float64 and out.numel() >= count * self.dof * n_windows * 2
        self._bind(batch)
        rec = batch.c_records()
        self._check(self._lib.ltp_envelope_batch(self._h, first, count, C.byref(batch.queries), C.byref(rec), int(window),
                                                 int(n_windows), out.data_ptr(), self._stream()))
        return out

    def buildRunTables(self, batch: DeviceBatch, first, count, out=None):
        """NEW (the consumer HOOK): the packed run tables of plans [first, first+count) in a caller buffer
        (ltp_build_tables_batch; format and device functions: include/ltp_run_tables.hpp). Returns an int64 CUDA tensor of
        ltp_run_tables_bytes / 8 words; lane (plan - first) * dof + joint."""
        import torch
        words = int(self._lib.ltp_run_tables_bytes(self._h, count)) // 8
        if out is None:
            out = torch.empty(max(words, 2), dtype=torch.int64, device=batch.offsets.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.int64      # (the size is checked by the library)
        self._bind(batch)
        rec = batch.c_records()
        self._check(self._lib.ltp_build_tables_batch(self._h, first, count, C.byref(batch.queries), C.byref(rec), out.data_ptr(),
                                                     out.numel() * 8, self._stream()))
        return out

    def replanStates(self, batch: DeviceBatch, first, count, tile, sample_index, layout="query_major"):
        """NEW: start states (q_0, v_0, a_0) of the next plans = sample k of the trajectories that
        sampleBatch(batch, first, count, tile) wrote. sample_index: int or int32 CUDA tensor [count]."""
        import torch
        shape, sq, sj = _layout(layout, count, self.dof)
        out = [torch.empty(shape, dtype=torch.float64, device=tile.device) for _ in range(3)]
        self._bind(batch)
        rec = batch.c_records()
        per_plan = None if isinstance(sample_index, int) else sample_index
        fn = self._lib.ltp_replan_states_f32_batch if tile.dtype == torch.float32 else self._lib.ltp_replan_states_batch
        self._check(fn(self._h, first, count, C.byref(batch.queries), C.byref(rec), batch.offsets.data_ptr(),
                       tile.data_ptr(), tile.numel(), per_plan.data_ptr() if per_plan is not None else None,
                       sample_index if per_plan is None else 0, *[x.data_ptr() for x in out], sq, sj, self._stream()))
        return out

    def stateAt(self, batch: DeviceBatch, first, count, sample_index, layout="query_major"):
        """NEW: (q, v, a) at trajectory sample k of plans [first, first+count) straight from the records
        (ltp_state_at_batch) — no sampled rows needed. sample_index: int or int32 CUDA tensor [count]."""
        import torch
        shape, sq, sj = _layout(layout, count, self.dof)
        out = [torch.empty(shape, dtype=torch.float64, device=batch.offsets.device) for _ in range(3)]
        self._bind(batch)
        rec = batch.c_records()
        per_plan = None if isinstance(sample_index, int) else sample_index
        self._check(self._lib.ltp_state_at_batch(self._h, first, count, C.byref(batch.queries), C.byref(rec),
                                                 per_plan.data_ptr() if per_plan is not None else None,
                                                 sample_index if per_plan is None else 0, *[x.data_ptr() for x in out], sq, sj, self._stream()))
        return out

    def windowRowStride(self, n_samples):
        """Elements per row of a window of n_samples samples (ltp_row_stride): the last dimension of sampleWindow's tensor."""
        return self._lib.ltp_row_stride(int(n_samples))

    # ---- what the readers of a planned batch (windows, horizons, knot grids, horizon envelopes) share: each rule once ----
    @staticmethod
    def _start(start, count):
        """(first_sample pointer, uniform_first) of a device reader's `start`: an integer (numpy's included: traj_len arithmetic
        gives those) is every plan's start; anything else must be an int32 CUDA tensor of at least `count` starts."""
        if isinstance(start, numbers.Integral):
            return None, int(start)
        import torch
        assert start.is_cuda and start.is_contiguous() and start.dtype == torch.int32 and start.numel() >= count
        return start.data_ptr(), 0

    @staticmethod
    def _valid(valid, count, dev):
        """The int32 tensor of `count` per-plan counts a device reader fills: the caller's, or a new one."""
        import torch
        if valid is None:
            valid = torch.empty((count,), dtype=torch.int32, device=dev)
        assert valid.is_cuda and valid.is_contiguous() and valid.dtype == torch.int32 and valid.numel() >= count
        return valid

    def _rows(self, out, dtype, count, n_elements, dev):
        """The rows tensor [count, 4, dof, R], R = ltp_row_stride(n_elements), of a row reader — the caller's `out`, which must agree
        with a `dtype` given beside it, or a new one of `dtype` (default float64) — and its LTP_ROWS_* format."""
        import torch
        if out is None:
            out = torch.empty((count, 4, self.dof, self.windowRowStride(n_elements)), dtype=dtype or torch.float64, device=dev)
        assert out.is_cuda and out.is_contiguous() and out.dtype in (torch.float32, torch.float64)
        assert dtype is None or out.dtype == dtype
        return out, 1 if out.dtype == torch.float32 else 0

    def _read(self, entry, batch, first, count, opts, out):
        """The tail of a device reader: bind the batch's limit sets, its records, entry(..., &opts, out, capacity, stream), check."""
        self._bind(batch)
        rec = batch.c_records()
        self._check(entry(self._h, first, count, C.byref(batch.queries), C.byref(rec), C.addressof(opts), out.data_ptr(), out.numel(),
                          self._stream()))

    def _sample_rows(self, entry, make_opts, batch, first, count, start, n_elements, out, dtype, valid):
        """sampleWindow, sampleHorizon and sampleKnots: rows and valid by the rules above, the entry's own opts struct from
        make_opts(format, first_sample, uniform_first, valid), the call. Returns (rows, valid)."""
        dev = batch.offsets.device
        out, fmt = self._rows(out, dtype, count, n_elements, dev)
        valid = self._valid(valid, count, dev)
        self._read(entry, batch, first, count, make_opts(fmt, *self._start(start, count), valid.data_ptr()), out)
        return out, valid

    def _plan_reader_host(self, entry, queries, start, args, shape):
        """The body of the four plan*Host readers: the query arrays, zeroed records, the zeroed output [n, *shape] and valid [n], the
        start (a scalar for every plan, or an [n] int array), and entry(h, n, queries, first_sample, uniform_first, *args, records,
        output, valid). Returns (records dict, output, valid)."""
        D = self.dof
        ins, n = _query_arrays(D, queries)
        r, rec = _host_records(n, D)
        out = np.zeros((n, *shape))
        valid = np.zeros(n, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        per_plan = None if np.ndim(start) == 0 else np.ascontiguousarray(np.asarray(start, dtype=np.int32).reshape(n))
        self._check(entry(self._h, n, *[_ptr(x) for x in ins], per_plan.ctypes.data_as(ip) if per_plan is not None else None,
                          int(start) if per_plan is None else 0, *args, C.byref(rec), _ptr(out), valid.ctypes.data_as(ip)))
        return r, out, valid

    def sampleWindow(self, batch: DeviceBatch, first, count, start, n_samples, out=None, dtype=None, valid=None):
        """NEW (horizon windows, ltp_sample_window_batch): the n_samples trajectory samples [k, k + n_samples) of plans
        [first, first+count), k = start (an int for every plan, or an int32 CUDA tensor [count]). Returns (rows, valid): rows is
        [count, 4, dof, R] with R = ltp_row_stride(n_samples) — slice [..., :n_samples], the rest of a row is not written — of
        dtype torch.float64 (default) or torch.float32; valid is the int32 tensor [count] of real samples per plan. Past the end
        of a plan q holds its last position and v, a, j are +0.0; plans without a trajectory are NaN (include/ltp_hip.h)."""
        O, N = _abi.WindowOpts, int(n_samples)
        return self._sample_rows(self._lib.ltp_sample_window_batch, lambda fmt, k_each, k, v: O(C.sizeof(O), fmt, N, k_each, k, v),
                                 batch, first, count, start, N, out, dtype, valid)

    def planWindowHost(self, q_goal, q_0, v_0, a_0, start, n_samples):
        """NEW: stages 1-3 + the horizon windows for numpy arrays (ltp_plan_window_host). start: an int, or an [n] int array.
        Returns (records dict, rows[n][4][dof][R], valid[n]); status carries END_LIMIT like planBatchHost(sample=False)."""
        N = int(n_samples)
        return self._plan_reader_host(self._lib.ltp_plan_window_host, (q_goal, q_0, v_0, a_0), start, (N,),
                                      (4, self.dof, self.windowRowStride(N)))

    def sampleHorizon(self, batch: DeviceBatch, first, count, start, n_samples, stride, out=None, dtype=None, valid=None):
        """NEW (strided horizon windows, ltp_sample_horizon_batch): element w of a row is trajectory sample k + w * stride of plans
        [first, first+count), k = start (an int for every plan, or an int32 CUDA tensor [count]). Shapes, dtypes, the hold and NaN
        rules and the return value are sampleWindow's; valid counts the real elements, min(n_samples, ceil((traj_len - k) / stride)).
        stride = 1 is sampleWindow."""
        O, N, s = _abi.HorizonOpts, int(n_samples), int(stride)
        return self._sample_rows(self._lib.ltp_sample_horizon_batch, lambda fmt, k_each, k, v: O(C.sizeof(O), fmt, N, s, k_each, k, v),
                                 batch, first, count, start, N, out, dtype, valid)

    def planHorizonHost(self, q_goal, q_0, v_0, a_0, start, n_samples, stride):
        """NEW: stages 1-3 + the strided horizon windows for numpy arrays (ltp_plan_horizon_host). start: an int, or an [n] int
        array. Returns (records dict, rows[n][4][dof][R], valid[n]); status carries END_LIMIT like planBatchHost(sample=False)."""
        N = int(n_samples)
        return self._plan_reader_host(self._lib.ltp_plan_horizon_host, (q_goal, q_0, v_0, a_0), start, (N, int(stride)),
                                      (4, self.dof, self.windowRowStride(N)))

    @staticmethod
    def _host_knots(knots):
        """A host knot grid as a contiguous int32 array, its FORM checked (ValueError): one dimension, integers. Nothing is rounded
        or flattened on the way; an integer beyond int32 becomes the nearest int32, which the content rule refuses like itself."""
        g = np.asarray(knots)
        if g.size == 0 and g.ndim == 1:
            return np.zeros(0, dtype=np.int32)           # an empty list has no integer type of its own; the length rule refuses it
        if g.ndim != 1:
            raise ValueError("knots must be a one-dimensional list of offsets")
        if g.dtype.kind not in "iu":
            raise ValueError("knots must be integers")
        top = np.iinfo(np.int32).max
        g = np.minimum(g, top) if g.dtype.kind == "u" else np.clip(g, np.iinfo(np.int32).min, top)
        return np.ascontiguousarray(g.astype(np.int32))

    @classmethod
    def _checked_knots(cls, knots):
        """_host_knots plus the CONTENT rule ltp_plan_knots_host applies (include/ltp_hip.h), as ValueError."""
        g = cls._host_knots(knots)
        if not 1 <= g.size <= _abi.MAX_KNOTS:
            raise ValueError(f"knots must be a list of 1 .. {_abi.MAX_KNOTS} offsets")
        if g.min() < 0 or g.max() > _abi.KNOT_OFFSET_MAX or np.any(np.diff(g.astype(np.int64)) < 0):
            raise ValueError("knots must be non-decreasing offsets in [0, 2^30]")
        return g

    def _device_knots(self, knots, dev):
        """The device copy of a host grid: validated, uploaded once and kept per content (and device)."""
        import torch
        g = self._checked_knots(knots)
        cache = self._knots_cache
        key = (g.tobytes(), str(dev))
        if key not in cache:
            if len(cache) >= 16:                     # a controller has a handful of grids; anything else should pass device tensors
                cache.pop(next(iter(cache)))
            cache[key] = torch.from_numpy(g).to(dev)
        return cache[key]

    def _grid(self, grid, dev):
        """The device grid of sampleKnots / envelopeKnots: an int32 CUDA tensor [N] as it is (not looked at on the host), or a host
        sequence through _device_knots (checked: ValueError; uploaded once per content)."""
        import torch
        if isinstance(grid, torch.Tensor):
            assert grid.is_cuda and grid.is_contiguous() and grid.dtype == torch.int32 and grid.dim() == 1
            return grid
        return self._device_knots(grid, dev)

    def sampleKnots(self, batch: DeviceBatch, first, count, start, knots, out=None, dtype=None, valid=None):
        """NEW (knot-grid horizons, ltp_sample_knots_batch): element w of a row is trajectory sample k + knots[w] of plans
        [first, first+count), k = start (an int for every plan, or an int32 CUDA tensor [count]). knots: N <= 512 non-decreasing
        offsets in [0, 2^30] — an int32 CUDA tensor [N] (not looked at on the host: a tensor that breaks the rule gives unspecified
        values, nothing worse; its content may be rewritten between the replays of a captured call), or a host sequence / array
        (checked: ValueError; uploaded once per content). Shapes, dtypes, the hold and NaN rules and the return value are
        sampleHorizon's with n_samples = N; valid counts the w with k + knots[w] < traj_len."""
        grid = self._grid(knots, batch.offsets.device)
        O, N = _abi.KnotsOpts, int(grid.numel())
        g = grid.data_ptr() if N else None            # an empty tensor has no storage to point at; the length rule refuses the grid
        return self._sample_rows(self._lib.ltp_sample_knots_batch, lambda fmt, k_each, k, v: O(C.sizeof(O), fmt, N, k, g, k_each, v),
                                 batch, first, count, start, N, out, dtype, valid)

    def planKnotsHost(self, q_goal, q_0, v_0, a_0, start, knots):
        """NEW: stages 1-3 + the knot-grid horizons for numpy arrays (ltp_plan_knots_host). start: an int, or an [n] int array;
        knots: a host sequence of integer offsets (its form is checked here as sampleKnots checks it: ValueError for a grid that
        is not one-dimensional or not of integers; its content by the library: LtpError for a decreasing, negative, beyond-2^30,
        empty or too long grid). Returns
        (records dict, rows[n][4][dof][R], valid[n]); status carries END_LIMIT like planBatchHost(sample=False)."""
        g = self._host_knots(knots)
        N = int(g.size)
        return self._plan_reader_host(self._lib.ltp_plan_knots_host, (q_goal, q_0, v_0, a_0), start,
                                      (N, g.ctypes.data_as(C.POINTER(C.c_int))),
                                      (4, self.dof, self.windowRowStride(max(N, 1))))   # rows to point at also for the grid the library refuses

    def stopKnots(self, batch: DeviceBatch, first, count, sample_index, knots, clamp_acceleration=True, out=None, valid=None):
        """NEW (stop horizons, ltp_stop_knots_batch; the contract is in include/ltp_hip.h): if plans [first, first+count) are followed
        up to trajectory sample k + knots[w] and every joint brakes from there as hard as it may (optBraking), where does it come to
        rest and how long does that take — for every knot of the grid, in one kernel. k = sample_index (an int for every plan, or an
        int32 CUDA tensor [count]); knots as sampleKnots takes them (an int32 CUDA tensor, not looked at on the host, or a host
        sequence: checked, ValueError, uploaded once per content). clamp_acceleration=True clamps each knot's acceleration to
        +-a_max of its joint first (planStopFrom's clamp); False brakes from the sampled one and stores NaN where |a| > a_max, per
        (plan, joint, knot). Returns (out.view(count, 2, dof, R), valid): out[:, 0] is q_stop, out[:, 1] t_stop, R =
        ltp_row_stride(N) — slice [..., :N], the rest of a row is not written; float64. Past the end of a plan the robot rests:
        q_stop is its last position and t_stop 0; plans without a trajectory are NaN. valid counts the w with k + knots[w] < traj_len.
        The robot's stop time from knot w is out[:, 1].amax(dim=1)."""
        import torch
        dev = batch.offsets.device
        grid = self._grid(knots, dev)
        O, N = _abi.StopKnotsOpts, int(grid.numel())
        shape = (count, 2, self.dof, self.windowRowStride(max(N, 1)))
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=dev)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float64
        valid = self._valid(valid, count, dev)
        k_each, k = self._start(sample_index, count)
        o = O(C.sizeof(O), N, _abi.STOP_ACCEL_CLAMP if clamp_acceleration else _abi.STOP_ACCEL_STRICT, k,
              grid.data_ptr() if N else None, k_each, valid.data_ptr())
        self._read(self._lib.ltp_stop_knots_batch, batch, first, count, o, out)
        return out.view(shape), valid

    def planStopKnotsHost(self, q_goal, q_0, v_0, a_0, sample_index, knots, clamp_acceleration=True):
        """NEW: stages 1-3 + the stop horizons for numpy arrays (ltp_plan_stop_knots_host). sample_index: an int, or an [n] int
        array; knots: a host sequence of integer offsets (form: ValueError, as planKnotsHost; content by the library: LtpError for
        a decreasing, negative, beyond-2^30, empty or too long grid). Returns (records dict, out[n][2][dof][R], valid[n]); status
        carries END_LIMIT like planBatchHost(sample=False)."""
        g = self._host_knots(knots)
        N = int(g.size)
        accel = _abi.STOP_ACCEL_CLAMP if clamp_acceleration else _abi.STOP_ACCEL_STRICT
        return self._plan_reader_host(self._lib.ltp_plan_stop_knots_host, (q_goal, q_0, v_0, a_0), sample_index,
                                      (N, g.ctypes.data_as(C.POINTER(C.c_int)), accel),
                                      (2, self.dof, self.windowRowStride(max(N, 1))))   # an output to point at also for the grid the library refuses

    def envelopeKnots(self, batch: DeviceBatch, first, count, start, edges, closed=False, out=None, valid=None):
        """NEW (horizon envelopes, ltp_envelope_knots_batch): env[count, dof, M, 2] = min / max of q of plans [first, first+count)
        over the trajectory samples between the edges k + edges[w] and k + edges[w + 1] of a knot grid, k = start (an int for every
        plan, or an int32 CUDA tensor [count]). edges: the M + 1 <= 512 non-decreasing offsets in [0, 2^30] sampleKnots takes, at
        least two — an int32 CUDA tensor (not looked at on the host: a tensor that breaks the rule gives unspecified values, nothing
        worse; its content may be rewritten between the replays of a captured call), or a host sequence / array (checked:
        ValueError; uploaded once per content). closed=False: interval w holds the samples [k + edges[w], k + edges[w + 1]);
        closed=True: it also holds the knot sample k + edges[w + 1]. Intervals past the end hold the last position twice, plans
        without a trajectory NaN; the values are the analytic envelope form's (setEnvelopeMode does not apply). Returns (env,
        valid); valid[i] counts the w with k + edges[w] < traj_len. status is not touched."""
        return self._envelope_knots(batch, first, count, start, edges, None, closed, out, valid)

    def planEnvelopeKnotsHost(self, q_goal, q_0, v_0, a_0, start, edges, closed=False):
        """NEW: stages 1-3 + the horizon envelopes for numpy arrays (ltp_plan_envelope_knots_host). start: an int, or an [n] int
        array; edges: a host sequence of integer offsets (form: ValueError, as planKnotsHost; content by the library: LtpError for a
        decreasing, negative or beyond-2^30 grid, fewer than 2 or more than 512 edges). Returns (records dict, env[n][dof][M][2],
        valid[n]); status carries END_LIMIT like planBatchHost(sample=False)."""
        return self._plan_envelope_knots_host((q_goal, q_0, v_0, a_0), start, edges, None, closed)

    @staticmethod
    def _env_arrays(arrays):
        """The LTP_ENV_* mask of envelopeKnotsArrays: a non-empty string over "qvaj" without repeats (any order: the planes always
        come in the order q, v, a, j), or an int in 1 .. 15. ValueError for anything else."""
        if isinstance(arrays, str):
            if not arrays or len(set(arrays)) != len(arrays) or any(c not in _abi.ENV_ARRAYS for c in arrays):
                raise ValueError('arrays must be a non-empty string over "qvaj" without repeats, or an int mask in 1 .. 15')
            return sum(_abi.ENV_ARRAYS[c] for c in arrays)
        if isinstance(arrays, bool) or not isinstance(arrays, (int, np.integer)) or not 1 <= int(arrays) <= 15:
            raise ValueError('arrays must be a non-empty string over "qvaj" without repeats, or an int mask in 1 .. 15')
        return int(arrays)

    def envelopeKnotsArrays(self, batch: DeviceBatch, first, count, start, edges, arrays="qvaj", closed=False, out=None, valid=None):
        """NEW (horizon envelopes of q, v, a and j, ltp_envelope_knots_arrays_batch): env[count, A, dof, M, 2] = min / max of each
        selected array of plans [first, first+count) over the trajectory samples between the edges k + edges[w] and k + edges[w + 1].
        arrays: a string over "qvaj" or an int mask (LTP_ENV_Q = 1, _V = 2, _A = 4, _J = 8); plane x of env is the x-th selected array
        in the order q, v, a, j. start, edges, closed, valid and the rules for a grid are envelopeKnots'; arrays="q" gives its bits.
        Past the end of a plan v, a and j are 0: an interval that reaches past the last sample also holds 0, one that starts there
        holds {0, 0} (q: the last position twice). The peak of |x| over an interval is max(-env[..., 0], env[..., 1]). A bad
        `arrays` or a bad host edge list raises ValueError before anything is uploaded. Returns (env, valid); status is not touched."""
        return self._envelope_knots(batch, first, count, start, edges, self._env_arrays(arrays), closed, out, valid)

    def planEnvelopeKnotsArraysHost(self, q_goal, q_0, v_0, a_0, start, edges, arrays="qvaj", closed=False):
        """NEW: stages 1-3 + the horizon envelopes of q, v, a and j for numpy arrays (ltp_plan_envelope_knots_arrays_host):
        planEnvelopeKnotsHost plus `arrays` (envelopeKnotsArrays' rule: ValueError). Returns (records dict, env[n][A][dof][M][2],
        valid[n]); status carries END_LIMIT like planBatchHost(sample=False)."""
        return self._plan_envelope_knots_host((q_goal, q_0, v_0, a_0), start, edges, self._env_arrays(arrays), closed)

    @staticmethod
    def _env_count(mask):
        """A of an LTP_ENV_* mask: the number of arrays it selects."""
        return bin(mask).count("1")

    def _envelope_knots(self, batch, first, count, start, edges, mask, closed, out, valid):
        """envelopeKnots (mask None: ltp_envelope_knots_batch, env[count, dof, M, 2]) and envelopeKnotsArrays (a checked mask:
        ltp_envelope_knots_arrays_batch, env[count, A, dof, M, 2])."""
        import torch
        dev = batch.offsets.device
        if not isinstance(edges, torch.Tensor) and self._host_knots(edges).size < 2:
            raise ValueError("edges must hold at least 2 offsets (one interval)")       # before anything is uploaded
        grid = self._grid(edges, dev)
        M = int(grid.numel()) - 1
        shape = (count,) + (() if mask is None else (self._env_count(mask),)) + (self.dof, max(M, 0), 2)
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=dev)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float64
        valid = self._valid(valid, count, dev)
        k_each, k = self._start(start, count)
        O = _abi.EnvelopeKnotsOpts if mask is None else _abi.EnvelopeArraysOpts
        o = O(C.sizeof(O), M, int(bool(closed)), k, *(() if mask is None else (mask, 0)),
              grid.data_ptr() if grid.numel() else None, k_each, valid.data_ptr())
        self._read(self._lib.ltp_envelope_knots_batch if mask is None else self._lib.ltp_envelope_knots_arrays_batch, batch, first, count, o, out)
        return out, valid

    def _plan_envelope_knots_host(self, queries, start, edges, mask, closed):
        """planEnvelopeKnotsHost (mask None: ltp_plan_envelope_knots_host) and planEnvelopeKnotsArraysHost (a checked mask)."""
        g = self._host_knots(edges)
        M = int(g.size) - 1
        if g.size == 0:
            g = np.zeros(1, dtype=np.int32)           # a pointer the library may look at; the length rule refuses the grid
        args = (M, g.ctypes.data_as(C.POINTER(C.c_int)), int(bool(closed)))
        if mask is None:
            return self._plan_reader_host(self._lib.ltp_plan_envelope_knots_host, queries, start, args, (self.dof, max(M, 1), 2))
        return self._plan_reader_host(self._lib.ltp_plan_envelope_knots_arrays_host, queries, start, args + (mask,),
                                      (self._env_count(mask), self.dof, max(M, 1), 2))
    @staticmethod
    def _exit_horizon(horizon):
        """The horizon of firstExit: an int in 1 .. 2^30. ValueError for anything else."""
        if isinstance(horizon, bool) or not isinstance(horizon, numbers.Integral) or not 1 <= int(horizon) <= _abi.EXIT_HORIZON_MAX:
            raise ValueError("horizon must be an int in 1 .. 2^30")
        return int(horizon)

    @staticmethod
    def _exit_boxes(lo, hi, mask, count, dof):
        """The boxes of firstExit: lo / hi are None or dicts by array letter ("q", "v", "a", "j") of arrays shaped [dof] (one box per
        joint for the whole call) or [count, dof] — every given one the same of the two. Returns ([lo by array index], [hi by array
        index], per_plan); ValueError for a letter that is no array or is not selected, a bad shape or mixed shapes."""
        sides, kinds = [], set()
        for name, side in (("lo", lo), ("hi", hi)):
            slots = [None] * 4
            if side is not None:
                if not isinstance(side, dict):
                    raise ValueError(f'{name} must be None or a dict by array letter, e.g. {{"q": tensor}}')
                for key, value in side.items():
                    if not isinstance(key, str) or key not in _abi.ENV_ARRAYS:
                        raise ValueError(f'{name}: "{key}" is none of "q", "v", "a", "j"')
                    if not mask & _abi.ENV_ARRAYS[key]:
                        raise ValueError(f'{name}: a box is given for "{key}", which `arrays` does not select')
                    if value is None:
                        continue
                    shape = tuple(value.shape) if hasattr(value, "shape") else None
                    if shape == (dof,):
                        kinds.add(False)
                    elif shape == (count, dof):
                        kinds.add(True)
                    else:
                        raise ValueError(f'{name}["{key}"] must have the shape [dof] = [{dof}] or [count, dof] = [{count}, {dof}]')
                    slots["qvaj".index(key)] = value
            sides.append(slots)
        if len(kinds) > 1:
            raise ValueError("the boxes of one call are all [dof] or all [count, dof]")
        return sides[0], sides[1], bool(kinds and kinds.pop())

    def _box_horizon_read(self, entry, O, batch, first, count, k, horizon, arrays, lo, hi, fold, out):
        """firstExit and settle behind their two names: the mask, the horizon and the boxes are validated (ValueError before any device
        work), then the entry of that name fills the int32 table [count, A, dof]. O: the entry's options struct (the two are the same field for field
        up to the last pointer); fold: False, True or an int32 CUDA tensor [count] for the per-plan fold (first_any / settle_all)."""
        import torch
        mask = self._env_arrays(arrays)
        H = self._exit_horizon(horizon)
        lo_by, hi_by, per_plan = self._exit_boxes(lo, hi, mask, count, batch.dof)
        A = self._env_count(mask)
        dev = batch.offsets.device
        shape = (count, A, self.dof)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=dev)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.int32
        for t in lo_by + hi_by:
            assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float64)
        folded = None
        if fold is not False and fold is not None:
            folded = self._valid(None if fold is True else fold, count, dev)
        k_each, k_all = self._start(k, count)
        P = C.c_void_p * 4
        o = O(C.sizeof(O), mask, H, k_all, k_each, P(*[t.data_ptr() if t is not None else None for t in lo_by]),
              P(*[t.data_ptr() if t is not None else None for t in hi_by]), self.dof if per_plan else 0, 1,
              folded.data_ptr() if folded is not None else None)
        self._read(getattr(self._lib, entry), batch, first, count, o, out)
        out = out.view(shape)
        return (out, folded) if folded is not None else out

    def _plan_box_horizon_host(self, entry, q_goal, q_0, v_0, a_0, k, horizon, arrays, lo, hi, fold):
        """planFirstExitHost and planSettleHost behind their two names: the same validation, then the entry of that name (stages 1-3 + the reader) on
        numpy arrays. Returns (records dict, table[n][A][dof]) and, with fold, the per-plan fold [n] as a third."""
        mask = self._env_arrays(arrays)
        H = self._exit_horizon(horizon)
        D = self.dof
        ins, n = _query_arrays(D, (q_goal, q_0, v_0, a_0))
        def as_arrays(side):
            if not isinstance(side, dict):
                return side                               # None, or what _exit_boxes refuses
            return {key: (v if v is None else np.asarray(v, dtype=np.float64)) for key, v in side.items()}
        lo_by, hi_by, per_plan = self._exit_boxes(as_arrays(lo), as_arrays(hi), mask, n, D)
        lo_by = [None if b is None else np.ascontiguousarray(b, dtype=np.float64) for b in lo_by]
        hi_by = [None if b is None else np.ascontiguousarray(b, dtype=np.float64) for b in hi_by]
        r, rec = _host_records(n, D)
        out = np.zeros((n, self._env_count(mask), D), dtype=np.int32)
        folded = np.zeros(n, dtype=np.int32) if fold else None
        ip = C.POINTER(C.c_int)
        per = None if np.ndim(k) == 0 else np.ascontiguousarray(np.asarray(k, dtype=np.int32).reshape(n))
        P = _dp * 4
        self._check(getattr(self._lib, entry)(
            self._h, n, *[_ptr(x) for x in ins], per.ctypes.data_as(ip) if per is not None else None, int(k) if per is None else 0, H, mask,
            P(*[_ptr(b) if b is not None else None for b in lo_by]), P(*[_ptr(b) if b is not None else None for b in hi_by]), int(per_plan),
            C.byref(rec), out.ctypes.data_as(ip), folded.ctypes.data_as(ip) if folded is not None else None))
        return (r, out, folded) if fold else (r, out)

    def firstExit(self, batch: DeviceBatch, first, count, k, horizon, arrays="q", lo=None, hi=None, any=False, out=None):
        """NEW (first exits, ltp_first_exit_batch; the contract is in include/ltp_hip.h): exit[count, A, dof] (int32) = the smallest
        trajectory sample t in [k, k + horizon) at which the selected array of joint j of plans [first, first+count) lies outside
        its box (x < lo or x > hi; NaN never exits), -1 (LTP_EXIT_NONE) for none, -2 (LTP_EXIT_NO_PLAN) for a plan without a
        trajectory. k: an int for every plan, or an int32 CUDA tensor [count]; below 0 counts as 0, beyond traj_len as traj_len.
        horizon: 1 .. 2^30 samples (2^30: the whole plan and the rest after it). arrays: envelopeKnotsArrays' string over "qvaj" or
        int mask; plane x is the x-th selected array in the order q, v, a, j. lo / hi: dicts by array letter of float64 CUDA
        tensors [dof] or [count, dof] (all of one call the same of the two); a side that is not given is the plan's own limit
        (q_min / q_max, -+v_max, -+a_max, -+j_max; under bound limit sets the plan's own set). Sampled accelerations exceed a_max by
        rounding in most plans, so with the default a box most plans exit: pass a margin. With arrays="q", k=0, horizon=2**30 and no
        boxes, exit != -1 is the path-limit verdict the reference does not form. any: True (or an int32 CUDA tensor [count] to
        fill) also returns the minimum over the table per plan (-1 where all are -1). A bad mask, horizon or box raises ValueError
        before any device work. Returns exit, or (exit, first_any); status is not touched."""
        return self._box_horizon_read("ltp_first_exit_batch", _abi.FirstExitOpts, batch, first, count, k, horizon, arrays, lo, hi, any, out)

    def planFirstExitHost(self, q_goal, q_0, v_0, a_0, k, horizon, arrays="q", lo=None, hi=None, any=False):
        """NEW: stages 1-3 + the first exits for numpy arrays (ltp_plan_first_exit_host). k: an int, or an [n] int array; horizon,
        arrays, lo / hi as firstExit takes them, the boxes as numpy arrays [dof] or [n, dof] (ValueError for a bad mask, horizon or
        box, before any device work). Returns (records dict, exit[n][A][dof]) and, with any=True, first_any[n] as a third;
        status carries END_LIMIT like planBatchHost(sample=False)."""
        return self._plan_box_horizon_host("ltp_plan_first_exit_host", q_goal, q_0, v_0, a_0, k, horizon, arrays, lo, hi, any)

    def settle(self, batch: DeviceBatch, first, count, k, horizon, arrays="q", lo=None, hi=None, all=False, out=None):
        """NEW (settling, ltp_settle_batch; the contract is in include/ltp_hip.h): settle[count, A, dof] (int32) = the trajectory
        sample from which the selected array of joint j of plans [first, first+count) is inside its box and stays inside for the
        rest of [k, k + horizon): the last outside sample of the horizon + 1, k where none is outside ("inside throughout"), -3
        (LTP_SETTLE_NOT_YET) where sample k + horizon - 1 is outside — past the end of the plan that is the resting state: the last
        position for q, 0 for v, a, j —, -2 (LTP_EXIT_NO_PLAN) for a plan without a trajectory. k, horizon, arrays, lo / hi: as
        firstExit takes them, validated by the same helpers (ValueError before any device work). all: True (or an int32 CUDA
        tensor [count] to fill) also returns the sample from which every selected array of every joint of the plan is inside: the
        maximum over the table, -3 where any entry is. Returns settle, or (settle, settle_all); status is not touched."""
        return self._box_horizon_read("ltp_settle_batch", _abi.SettleOpts, batch, first, count, k, horizon, arrays, lo, hi, all, out)

    def planSettleHost(self, q_goal, q_0, v_0, a_0, k, horizon, arrays="q", lo=None, hi=None, all=False):
        """NEW: stages 1-3 + settling for numpy arrays (ltp_plan_settle_host). The arguments are planFirstExitHost's (ValueError
        for a bad mask, horizon or box, before any device work). Returns (records dict, settle[n][A][dof]) and, with all=True,
        settle_all[n] as a third; status carries END_LIMIT like planBatchHost(sample=False)."""
        return self._plan_box_horizon_host("ltp_plan_settle_host", q_goal, q_0, v_0, a_0, k, horizon, arrays, lo, hi, all)

    def arrival(self, batch: DeviceBatch, first, count, k, q_goal, q_tol, v_tol=None):
        """NEW (a convenience over settle, no C entry of its own): the sample from which every joint of a plan is within q_tol of
        q_goal — and, with v_tol, no faster than v_tol — for the rest of the plan and after it: settle over the whole plan (horizon
        2^30) from k with the q boxes [q_goal - q_tol, q_goal + q_tol] and, with v_tol, the v boxes [-v_tol, v_tol], returning
        settle_all [count] (int32): -3 where a joint does not come to rest inside its tolerance, -2 for a plan without a
        trajectory. q_goal: a float64 CUDA tensor [dof] or [count, dof]; q_tol / v_tol: a float, or a tensor that broadcasts
        against q_goal."""
        import torch
        q_goal = torch.as_tensor(q_goal, dtype=torch.float64, device=batch.offsets.device)
        lo = {"q": (q_goal - q_tol).contiguous()}
        hi = {"q": (q_goal + q_tol).contiguous()}
        if v_tol is not None:
            speed = (torch.zeros_like(q_goal) + v_tol).contiguous()
            lo["v"], hi["v"] = (-speed).contiguous(), speed
        return self.settle(batch, first, count, k, _abi.EXIT_HORIZON_MAX, arrays="q" if v_tol is None else "qv", lo=lo, hi=hi, all=True)[1]

    def roots(self, poly, dtype=np.float64):
        """roots<T>() of the reference's roots.h:22-34 on the device: all eigenvalues of the companion matrix of each
        polynomial (rows of `poly`, highest coefficient first), as a complex array in Eigen's output order."""
        dt = np.dtype(dtype)
        poly = np.ascontiguousarray(np.atleast_2d(np.asarray(poly, dtype=dt)))
        n, deg = poly.shape[0], poly.shape[1] - 1
        re = np.zeros((n, deg), dtype=dt); im = np.zeros((n, deg), dtype=dt)
        if dt == np.float32:
            fp = C.POINTER(C.c_float)
            self._check(self._lib.ltp_roots_f32_host(self._h, n, deg, poly.ctypes.data_as(fp), re.ctypes.data_as(fp), im.ctypes.data_as(fp)))
        else:
            self._check(self._lib.ltp_roots_f64_host(self._h, n, deg, _ptr(poly), _ptr(re), _ptr(im)))
        # the two parts stored as they are: re + 1j * im would turn a -0 of either part into +0 (Eigen's second of a pair with a zero
        # imaginary part is (re, -0))
        out = np.empty((n, deg), dtype=np.complex64 if dt == np.float32 else np.complex128)
        out.real, out.imag = re, im
        return out

    # ---- diagnostics for the parity tests ----
    def debugMathProbe(self, x, y):
        x, y = _vec(x), _vec(y)
        out = np.zeros((x.size, 8))
        self._check(self._lib.ltp_debug_math_probe_host(self._h, x.size, _ptr(x), _ptr(y), _ptr(out)))
        return out

    @staticmethod
    def powRuleMatchingHostLibm(probes=0):
        """NEW: ("libm" | "exact" | None, mismatches vs the libm rule, mismatches vs the exact rule) — which pow rule has the bits of the
        C library this process runs on, i.e. of a reference built on this host (ltp_hip.h ltp_host_libm_pow_rule; host only)."""
        import ctypes as C
        from . import _abi
        a, b = C.c_longlong(), C.c_longlong()
        r = _abi.lib().ltp_host_libm_pow_rule(int(probes), C.byref(a), C.byref(b))
        return ({1: "libm", 0: "exact"}.get(r), a.value, b.value)

    def debugLibmPow(self, x, y):
        """pow(x, y) elementwise by the device's restated glibc pow (the arithmetic of setPowRule("libm"))."""
        x, y = _vec(x), _vec(y)
        if y.size != x.size:
            x, y = (np.ascontiguousarray(a, dtype=np.float64) for a in np.broadcast_arrays(x, y))     # the C call reads x.size of both
        out = np.zeros(x.size)
        self._check(self._lib.ltp_debug_libm_pow_host(self._h, x.size, _ptr(x), _ptr(y), _ptr(out)))
        return out

    def debugRootsProbe(self, degree, coef):
        coef = np.ascontiguousarray(np.asarray(coef, dtype=np.float64).reshape(-1, 7))
        out = np.zeros(coef.shape[0])
        self._check(self._lib.ltp_debug_roots_probe_host(self._h, coef.shape[0], int(degree), _ptr(coef), _ptr(out)))
        return out
