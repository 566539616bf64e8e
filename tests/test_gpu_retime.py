"""ltp_retime_batch on the GPU against the checker (tests/retime_checker.py: the CPU oracle composed into the retime rule of
include/ltp_hip.h): no-op requests, records, rows, groups, idempotence, refusals, the host and drop-in paths, graph capture."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import retime_checker as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = 0.001
REC_KEYS = ("t_opt", "t_scaled", "dir", "v_drive", "mod", "t_required", "slowest", "traj_len", "status")


def _planner(name, pow_rule="libm", max_samples=0):
    from longtermplanner_amd import LongTermPlanner, limit_set
    dof, lim = limit_set(name)
    ltp = LongTermPlanner(dof, TS, device=0, **lim)
    ltp.setPowRule(pow_rule)
    if max_samples:
        ltp.setMaxSamples(max_samples)
    return ltp, dof, lim


def _queries(lim, n, seed):
    from longtermplanner_amd import generate_queries
    return [np.ascontiguousarray(x) for x in generate_queries(n, lim, seed=seed)]


def _plan(ltp, qs, batch=None):
    import torch
    ts = [torch.from_numpy(x).to("cuda:0") for x in qs]
    return ltp.planSwitchTimesBatch(*ts, batch=batch)


def _host(batch):
    import torch
    torch.cuda.synchronize()
    r = {k: getattr(batch, k).cpu().numpy().copy() for k in REC_KEYS}
    r["offsets"] = batch.offsets.cpu().numpy().view(np.uint64).copy()
    return r


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def _assert_bit_equal(a, b, keys=REC_KEYS + ("offsets",), what=""):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs in {np.count_nonzero(_bits(a[k]) != _bits(b[k]))} bytes"


def _oracle(oracle_mod, dof, lim, pow_rule):
    # the libm-rule device has the bits of the default oracle where this host's libm is the restated glibc; the exact rule those
    # of the exact-pow twin everywhere
    return oracle_mod.Oracle(dof, TS, **lim, exact_pow=(pow_rule == "exact"))


def _bit_exact_expected(pow_rule):
    from longtermplanner_amd import LongTermPlanner
    return pow_rule == "exact" or LongTermPlanner.powRuleMatchingHostLibm()[0] == "libm"


def _compare_records(dev, chk, exact, what, mask):
    dev = {k: v[mask] for k, v in dev.items() if k in REC_KEYS}
    chk = {k: v[mask] for k, v in chk.items() if k in REC_KEYS}
    for k in ("t_scaled", "v_drive"):
        if exact:
            bad = np.count_nonzero(_bits(dev[k]) != _bits(chk[k]))
            assert bad == 0, f"{what}: {k} not bit-identical ({bad} bytes)"
        else:
            d = np.abs(dev[k] - chk[k])
            assert np.nanmax(d) < 1e-9, f"{what}: {k} max |d| {np.nanmax(d)}"
    assert np.array_equal(dev["mod"], chk["mod"]), what
    assert np.array_equal(_bits(dev["t_required"]), _bits(chk["t_required"])), what
    assert np.array_equal(dev["traj_len"], chk["traj_len"]), what


def _case_line(retimed, cases):
    """The accepted-case census of a retime as data: `cases` is retime_checker.retime's [n][9] (case 0 = fallback)."""
    per_case = [int(x) for x in cases.sum(axis=0)]
    lanes = sum(per_case)
    return dict(retimed=int(retimed.sum()), lanes=lanes, lanes_of_other_queries=int(cases[~retimed].sum()), per_case=per_case,
                queue_b_share=sum(per_case[3:]) / max(lanes, 1))


def _checker_case(oracle_mod, dof, lim, pow_rule, qs, dev_plain, T):
    orc = _oracle(oracle_mod, dof, lim, pow_rule)
    orec = orc.plan_batch(*qs)
    assert np.array_equal(rc.oracle_eligible(orec), rc.device_eligible(dev_plain))
    return rc.retime(orc, orec, *qs, T)


def test_no_op_requests_leave_every_bit(oracle_mod):
    """Requests at or below T*, NaN, negative, infinite or absent: records and offsets keep their bits."""
    import torch
    ltp, dof, lim = _planner("panda")
    qs = _queries(lim, 20000, seed=11)
    batch = _plan(ltp, qs)
    before = _host(batch)
    ts = rc.t_star(before)
    rng = np.random.default_rng(5)
    req = ts * rng.uniform(0.0, 1.0, ts.size)          # at or below the optimum
    r = rng.random(ts.size)
    req[r < 0.1] = np.nan
    req[(r >= 0.1) & (r < 0.2)] = -1.0
    req[(r >= 0.2) & (r < 0.25)] = np.inf
    req[(r >= 0.25) & (r < 0.35)] = ts[(r >= 0.25) & (r < 0.35)]
    elig = rc.device_eligible(before)
    small = float(np.min(ts[elig])) * 0.5
    for kw in (dict(), dict(uniform=small), dict(t_target=torch.from_numpy(req).to("cuda:0")),
               dict(t_target=torch.from_numpy(req).to("cuda:0"), uniform=small)):
        ltp.retimeBatch(batch, **kw)
        _assert_bit_equal(_host(batch), before, what=f"no-op {sorted(kw)}")


@pytest.mark.parametrize("name,n,pow_rule", [("panda", 20000, "libm"), ("panda", 20000, "exact"), ("ref", 20000, "libm"),
                                             ("ref", 20000, "exact"), ("ref30", 3000, "libm"), ("ref30", 3000, "exact")])
def test_records_match_the_checker(oracle_mod, name, n, pow_rule):
    import torch
    ltp, dof, lim = _planner(name, pow_rule)
    qs = _queries(lim, n, seed=2000 + n)
    exact = _bit_exact_expected(pow_rule)
    plain = None
    rng = np.random.default_rng(n)
    for k in (1.05, 1.5, 3.0, 10.0, "random", "uniform"):
        batch = _plan(ltp, qs)
        if plain is None:
            plain = _host(batch)
        ts = rc.t_star(plain)
        if k == "random":
            # some requests win, some are below the optimum, some are not requests at all
            T = ts * rng.uniform(0.5, 4.0, n)
            T[rng.random(n) < 0.05] = np.nan
            ltp.retimeBatch(batch, t_target=torch.from_numpy(T).to("cuda:0"))
            T_eff = rc.own_targets(ts, 0.0, T)
        elif k == "uniform":
            u = 2.0 * float(np.median(ts))
            ltp.retimeBatch(batch, uniform=u)
            T_eff = rc.own_targets(ts, u, None)
        else:
            ltp.retimeBatch(batch, uniform=0.0, t_target=torch.from_numpy(k * ts).to("cuda:0"))
            T_eff = k * ts
        dev = _host(batch)
        chk, retimed, cases = _checker_case(oracle_mod, dof, lim, pow_rule, qs, plain, T_eff)
        assert np.array_equal(retimed, rc.device_eligible(plain) & (T_eff > ts))
        _compare_records(dev, chk, exact, f"{name} {pow_rule} k={k}", retimed)
        # untouched queries keep their bits; retimed ones lose END_LIMIT / OVERFLOW and have status 0 or NONFINITE
        keep = ~retimed
        for key in REC_KEYS:
            assert np.array_equal(_bits(dev[key][keep]), _bits(plain[key][keep])), (k, key)
        assert np.all((dev["status"][retimed] & ~16) == 0)
        assert np.array_equal(dev["status"][retimed] == 0, chk["traj_len"][retimed] > 0)
        # offsets: the scan of the new lengths
        sizes = np.array([4 * dof * ltp._lib.ltp_row_stride(int(l)) if st == 0 else 0 for l, st in zip(dev["traj_len"], dev["status"])],
                         dtype=np.uint64)
        assert np.array_equal(dev["offsets"], np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64))
        line = _case_line(retimed, cases)
        print(f"{name} n={n} {pow_rule} k={k}: retimed {line['retimed']}, fallback joints {line['per_case'][0]}, "
              f"queue B share {line['queue_b_share']:.4f} (c1 {line['per_case'][1]}, c2 {line['per_case'][2]})")
        # every joint of every retimed query, and of no other, ended in exactly one case. (Nothing is asserted about WHICH cases: the
        # named sets reach c1 / c2 almost only — tests/test_branch_census_cpu.py; the rare ones are retimed in tests/test_gpu_branches.py)
        assert line["lanes"] == dof * line["retimed"] and line["lanes_of_other_queries"] == 0, line


@pytest.mark.parametrize("sampler,max_samples", [("fused", 0), ("walk", 0), ("auto", 400)])
def test_rows_match_the_checker(oracle_mod, sampler, max_samples):
    import torch
    from longtermplanner_amd import unpack_trajectory
    ltp, dof, lim = _planner("panda", "libm", max_samples)
    n = 2000
    qs = _queries(lim, n, seed=31)
    batch = _plan(ltp, qs)
    plain = _host(batch)
    rng = np.random.default_rng(3)
    T = rc.t_star(plain) * rng.uniform(1.05, 2.0, n)
    ltp.retimeBatch(batch, t_target=torch.from_numpy(T).to("cuda:0"))
    total = int(batch.offsets[n].item())
    out = torch.zeros(max(total, 2), dtype=torch.float64, device="cuda:0")
    ltp.sampleBatchEx(batch, 0, n, out, sampler=sampler)
    dev = _host(batch)
    rows = out.cpu().numpy()
    orc = _oracle(oracle_mod, dof, lim, "libm")
    orec = orc.plan_batch(*qs)
    chk, retimed, _ = rc.retime(orc, orec, *qs, rc.own_targets(rc.t_star(plain), 0.0, T))
    worst = 0.0
    q_min, q_max = np.asarray(lim["q_min"]), np.asarray(lim["q_max"])
    for p in range(n):
        if chk["traj_len"][p] <= 0 or not rc.oracle_eligible(orec)[p]:
            continue
        L, q, v, a, j = rc.trajectory(orc, chk, p, qs[1], qs[2], qs[3])
        assert L == dev["traj_len"][p]
        stored = ltp.storedSamples(L)
        gq, gv, ga, gj = unpack_trajectory(rows, int(dev["offsets"][p]), dof, stored)
        for g, o in ((gq, q), (gv, v), (ga, a), (gj, j)):
            worst = max(worst, float(np.max(np.abs(g - o[:, :stored]))))
        end_out = bool(np.any((q[:, L - 1] < q_min) | (q[:, L - 1] > q_max)))
        assert bool(dev["status"][p] & 8) == end_out, p
    assert worst < 1e-9, worst
    print(f"rows {sampler} cap {max_samples}: {retimed.sum()} retimed plans, max |d| {worst:.3e}")


def test_groups_synchronise_arrival(oracle_mod):
    import torch
    ltp, dof, lim = _planner("panda")
    n = 20000
    qs = _queries(lim, n, seed=77)
    rng = np.random.default_rng(8)
    bad = rng.random(n) < 0.02                            # non-eligible members: checkInputs fails (|v_0| > v_max)
    qs[2][bad, 0] = 10.0 * np.asarray(lim["v_max"])[0]
    perm = rng.permutation(n)
    group = np.empty(n, dtype=np.int32)
    g, i = 0, 0
    while i < n:
        s = int(rng.integers(1, 17))
        group[perm[i:i + s]] = g
        g, i = g + 1, i + s
    n_groups = g
    out_of_range = rng.random(n) < 0.03
    group[out_of_range] = np.where(rng.random(out_of_range.sum()) < 0.5, -1, n_groups + 5)
    batch = _plan(ltp, qs)
    plain = _host(batch)
    elig = rc.device_eligible(plain)
    assert (~elig).sum() >= bad.sum() > 0
    gt = ltp.retimeBatch(batch, uniform=0.0, group=torch.from_numpy(group).to("cuda:0"), n_groups=n_groups)
    dev = _host(batch)
    gt = gt.cpu().numpy()
    T, gt_host = rc.targets(plain, elig, 0.0, None, group, n_groups)
    assert np.array_equal(_bits(gt), _bits(gt_host))
    # each query = a per-query retime to its group's time
    batch2 = _plan(ltp, qs)
    ltp.retimeBatch(batch2, t_target=torch.from_numpy(np.where(elig, T, np.nan)).to("cuda:0"))
    _assert_bit_equal(_host(batch2), dev, what="group vs per-query")
    # arrival: every sampled member within the accept window of its group's time
    total = int(batch.offsets[n].item())
    out = torch.zeros(max(total, 2), dtype=torch.float64, device="cuda:0")
    ltp.sampleBatchEx(batch, 0, n, out)
    dev = _host(batch)
    in_group = elig & (group >= 0) & (group < n_groups) & ((dev["status"] & ~8) == 0)
    dur = (dev["traj_len"] - 1) * TS
    Tg = gt[np.clip(group, 0, n_groups - 1)]
    ok = (dur >= Tg - 0.1) & (dur <= Tg + 0.01 + TS)
    assert np.all(ok[in_group]), np.nonzero(in_group & ~ok)[0][:10]
    print(f"groups: {n_groups} groups, {in_group.sum()} members within the accept window of their group's time")


def test_retime_is_idempotent_and_a_longer_request_replaces_a_shorter_one(oracle_mod):
    import torch
    ltp, dof, lim = _planner("ref")
    qs = _queries(lim, 20000, seed=4)
    batch = _plan(ltp, qs)
    ltp.retimeBatch(batch, uniform=2.0)
    once = _host(batch)
    ltp.retimeBatch(batch, uniform=2.0)
    _assert_bit_equal(_host(batch), once, what="twice")
    ts = rc.t_star(once)
    longer = torch.from_numpy(np.maximum(ts, 2.0) * 1.7).to("cuda:0")
    ltp.retimeBatch(batch, t_target=longer)
    fresh = _plan(ltp, qs)
    ltp.retimeBatch(fresh, t_target=longer)
    _assert_bit_equal(_host(batch), _host(fresh), what="longer after shorter")


def test_refusals_name_their_reason():
    import torch
    from longtermplanner_amd import _abi
    ltp, dof, lim = _planner("panda")
    qs = _queries(lim, 256, seed=1)
    batch = _plan(ltp, qs)
    lib = ltp._lib
    rec = batch.c_records()

    def call(opts):
        rcode = lib.ltp_retime_batch(ltp._h, batch.n, C.byref(batch.queries), C.byref(rec), opts, batch.offsets.data_ptr(), ltp._stream())
        return rcode, (lib.ltp_last_error(ltp._h) or b"").decode()

    size = C.sizeof(_abi.RetimeOpts)
    msgs = []
    g = torch.zeros(batch.n, dtype=torch.int32, device="cuda:0")
    gt = torch.zeros(4, dtype=torch.float64, device="cuda:0")
    cases = [None,
             _abi.RetimeOpts(size - 8, None, 1.0, None, 0, None),
             _abi.RetimeOpts(size + 4, None, 1.0, None, 0, None),
             _abi.RetimeOpts(size, None, float("nan"), None, 0, None),
             _abi.RetimeOpts(size, None, -1.0, None, 0, None),
             _abi.RetimeOpts(size, None, float("inf"), None, 0, None),
             _abi.RetimeOpts(size, None, 0.0, g.data_ptr(), 0, gt.data_ptr()),
             _abi.RetimeOpts(size, None, 0.0, g.data_ptr(), 4, None)]
    for o in cases:
        rcode, m = call(None if o is None else C.addressof(o))
        assert rcode == 1, m
        msgs.append(m)
    # a newer caller's struct: zero bytes beyond ours are accepted, a non-zero one is refused
    buf = (C.c_ubyte * (size + 8))()
    newer = _abi.RetimeOpts(size + 8, None, 0.0, None, 0, None)
    C.memmove(buf, C.addressof(newer), size)
    assert call(C.addressof(buf))[0] == 0
    buf[size + 3] = 1
    rcode, m = call(C.addressof(buf))
    assert rcode == 1
    msgs.append(m)
    assert len({msgs[i] for i in (0, 1, 2, 3, 4, 6, 7, 8)}) == 8, msgs
    assert msgs[3] == msgs[5]
    # a changed batch geometry
    ltp.setSampleTime(0.002)
    valid = _abi.RetimeOpts(size, None, 1.0, None, 0, None)
    rcode, m = call(C.addressof(valid))
    assert rcode == 1 and "changed since the batch was planned" in m
    # MATLAB semantics
    ltp2, _, _ = _planner("panda")
    ltp2.setSemantics("matlab")
    b2 = _plan(ltp2, qs)
    with pytest.raises(_abi.LtpError) as e:
        ltp2.retimeBatch(b2, uniform=1.0)
    assert "LTP_SEMANTICS_MATLAB" in str(e.value)
    print("refusals:", msgs + [m, str(e.value)])


def test_host_path_equals_the_device_path(oracle_mod):
    import torch
    from longtermplanner_amd import unpack_trajectory
    ltp, dof, lim = _planner("panda")
    n = 500
    qs = _queries(lim, n, seed=9)
    batch = _plan(ltp, qs)
    ts = rc.t_star(_host(batch))
    T = ts * np.random.default_rng(2).uniform(0.5, 3.0, n)
    ltp.retimeBatch(batch, t_target=torch.from_numpy(T).to("cuda:0"))
    total = int(batch.offsets[n].item())
    out = torch.zeros(max(total, 2), dtype=torch.float64, device="cuda:0")
    ltp.sampleBatch(batch, 0, n, out)
    dev = _host(batch)
    host = ltp.planBatchHost(*qs, sample=True, duration=T)
    _assert_bit_equal(host, dev, what="host vs device")
    rows = out.cpu().numpy()
    for p in range(0, n, 25):
        L = int(dev["traj_len"][p])
        for a, b in zip(unpack_trajectory(host["packed"], int(host["offsets"][p]), dof, L), unpack_trajectory(rows, int(dev["offsets"][p]), dof, L)):
            assert np.array_equal(a, b), p
    # a uniform duration, and the default that changes nothing
    hu = ltp.planBatchHost(*qs, sample=False, duration=2.5)
    assert np.all(hu["t_required"][rc.device_eligible(hu)] == np.maximum(2.5, ts[rc.device_eligible(hu)]))
    _assert_bit_equal(ltp.planBatchHost(*qs, sample=False), ltp.planBatchHost(*qs, sample=False, duration=0.0),
                      keys=REC_KEYS + ("offsets",), what="duration 0")


DROPIN = r'''
#include "long_term_planner/long_term_planner.h"
#include <cstdio>
#include <cstring>
using namespace long_term_planner;
static bool same(const Trajectory& a, const Trajectory& b) {
  if (a.length != b.length || a.q.size() != b.q.size()) return false;
  for (std::size_t i = 0; i < a.q.size(); ++i)
    if (a.q[i] != b.q[i] || a.v[i] != b.v[i] || a.a[i] != b.a[i] || a.j[i] != b.j[i]) return false;
  return true;
}
int main(int argc, char** argv) {
  const int dof = 7, n = 6;
  std::vector<double> q_min = {-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973};
  std::vector<double> q_max = {2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973};
  std::vector<double> v_max = {2.175, 2.175, 2.175, 2.175, 2.61, 2.61, 2.61};
  std::vector<double> a_max = {15.0, 7.5, 10.0, 12.5, 15.0, 20.0, 20.0};
  std::vector<double> j_max = {7500.0, 3750.0, 5000.0, 6250.0, 7500.0, 10000.0, 10000.0};
  LongTermPlanner ltp(dof, 0.001, q_min, q_max, v_max, a_max, j_max);
  std::vector<double> in(4 * n * dof);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 2;
  std::fclose(f);
  FILE* o = std::fopen(argv[2], "wb");
  int fails = 0;
  for (int p = 0; p < n; ++p) {
    auto vec = [&](int k) { return std::vector<double>(in.begin() + (k * n + p) * dof, in.begin() + (k * n + p + 1) * dof); };
    const auto qg = vec(0), q0 = vec(1), v0 = vec(2), a0 = vec(3);
    BatchTrajectory b;
    ltp.planTrajectoryBatch(1, qg.data(), q0.data(), v0.data(), a0.data(), b);
    const double t_star = b.t_opt[(std::size_t)b.slowest[0] * 7 + 6];
    Trajectory ref, t;
    const bool r0 = ltp.planTrajectory(qg, q0, v0, a0, ref);
    for (double d : {0.0, -1.0, 0.5 * t_star, t_star}) {
      Trajectory tt;
      const bool r = ltp.planTrajectory(qg, q0, v0, a0, d, tt);
      if (r != r0 || !same(tt, ref)) { ++fails; std::printf("plan %d: duration %g differs from planTrajectory\n", p, d); }
    }
    const double T = 3.0 * t_star;
    const bool r = ltp.planTrajectory(qg, q0, v0, a0, T, t);
    const double hdr[3] = {T, (double)t.length, r ? 1.0 : 0.0};
    std::fwrite(hdr, sizeof(double), 3, o);
    for (int j = 0; j < dof; ++j) {
      std::fwrite(t.q[j].data(), sizeof(double), t.length, o); std::fwrite(t.v[j].data(), sizeof(double), t.length, o);
      std::fwrite(t.a[j].data(), sizeof(double), t.length, o); std::fwrite(t.j[j].data(), sizeof(double), t.length, o);
    }
  }
  std::fclose(o);
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
'''


def test_dropin_timed_plan_trajectory(oracle_mod, tmp_path):
    from longtermplanner_amd import limit_set
    dof, lim = limit_set("panda")
    n = 6
    qs = _queries(lim, n, seed=123)
    src = tmp_path / "timed.cc"
    src.write_text(DROPIN)
    exe = tmp_path / "timed"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "longtermplanner_amd"), "-lltp_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "longtermplanner_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    (tmp_path / "in.bin").write_bytes(np.concatenate([x.reshape(-1) for x in qs]).astype(np.float64).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    data = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    orc = oracle_mod.Oracle(dof, TS, **lim)
    orec = orc.plan_batch(*qs)
    at = 0
    for p in range(n):
        T, L, ok = data[at], int(data[at + 1]), data[at + 2]
        at += 3
        rows = data[at: at + 4 * dof * L].reshape(dof, 4, L)
        at += 4 * dof * L
        Tq = np.full(n, np.nan)
        Tq[p] = T
        chk, retimed, _ = rc.retime(orc, orec, *qs, Tq)
        assert retimed[p]
        Lc, q, v, a, j = rc.trajectory(orc, chk, p, qs[1], qs[2], qs[3])
        assert L == Lc
        for k, ref in enumerate((q, v, a, j)):
            assert np.max(np.abs(rows[:, k, :] - ref)) < 1e-9, (p, k)


def test_graph_capture_of_plan_retime_sample():
    """One capture and replay of plan + retime + sample on one stream after ltp_reserve_batch; on replay (new queries in the same
    buffers) the records and rows equal an uncaptured run."""
    import torch
    ltp, dof, lim = _planner("panda")
    n = 4096
    qa, qb = _queries(lim, n, seed=50), _queries(lim, n, seed=51)
    assert ltp._lib.ltp_reserve_batch(ltp._h, n) == 0
    ins = [torch.from_numpy(x).to("cuda:0") for x in qa]
    target = torch.full((n,), 2.0, dtype=torch.float64, device="cuda:0")
    totals = []
    for q in (qb, qa):                           # the row capacity both query sets need
        batch = _plan(ltp, q)
        ltp.retimeBatch(batch, t_target=target, uniform=0.5)
        totals.append(int(batch.offsets[n].item()))
    out = torch.zeros(max(totals), dtype=torch.float64, device="cuda:0")
    batch = ltp.planSwitchTimesBatch(*ins)

    def step():
        ltp.planSwitchTimesBatch(*ins, batch=batch)
        ltp.retimeBatch(batch, t_target=target, uniform=0.5)
        ltp.sampleBatchEx(batch, 0, n, out, sampler="walk")

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                   # eager warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for x, y in zip(ins, qb):
        x.copy_(torch.from_numpy(y))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    replayed, rows_r = _host(batch), out.cpu().numpy().copy()
    out.zero_()
    step()
    torch.cuda.synchronize()
    eager, rows_e = _host(batch), out.cpu().numpy().copy()
    _assert_bit_equal(replayed, eager, what="graph replay")
    assert np.array_equal(rows_r, rows_e)
    assert rc.device_eligible(eager).sum() > 0.9 * n and np.all(eager["t_required"][rc.device_eligible(eager)] >= 2.0)
