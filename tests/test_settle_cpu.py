"""Settling (ltp_settle_batch, include/ltp_hip.h) without a device: the symbols, the options struct, the validation that runs
before anything is launched, the Python wrappers' ValueError cases, the drop-in header's new method under plain g++, the settling
rule of the kernel on the host (tests/cpp/crossings_test.cc last, also under the address, undefined-behaviour and float-cast
sanitizers), the yardstick of the GPU tests (tests/box_checker.py) against a plain loop over the CPU oracle's trajectories, and
the condition the GPU tests' two box families rest on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import box_checker as sc
from envelope_checker import selected
from horizon_checker import TS, pack_full_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NAMES = ("ltp_settle_elements", "ltp_settle_batch", "ltp_plan_settle_host")


@pytest.fixture(scope="module")
def abi():
    from longtermplanner_amd import _abi
    _abi.build()
    return _abi


def _header():
    return open(os.path.join(ROOT, "include", "ltp_hip.h")).read()


def test_settle_symbols_are_declared_bound_and_exported(abi):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = C.CDLL(abi.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} is not declared in include/ltp_hip.h"
        assert n in abi.exported_symbols(), f"{n} is not declared in _abi._SIGNATURES"
        assert hasattr(lib, n), f"{n} is not exported"
        args = re.search(r"\b%s\s*\(([^;]*)\);" % n, text, flags=re.S).group(1)
        assert len(args.split(",")) == len(abi._SIGNATURES[n][1]), n
    # the host entry takes ltp_plan_first_exit_host's arguments, the device entry and the element count their siblings'
    for ours, theirs in zip(NAMES, ("ltp_first_exit_elements", "ltp_first_exit_batch", "ltp_plan_first_exit_host")):
        assert abi._SIGNATURES[ours][0] is abi._SIGNATURES[theirs][0] and len(abi._SIGNATURES[ours][1]) == len(abi._SIGNATURES[theirs][1])
        assert all(a is b for a, b in zip(abi._SIGNATURES[ours][1], abi._SIGNATURES[theirs][1])), ours
    assert int(re.search(r"#define LTP_SETTLE_NOT_YET\s+\((-?\d+)\)", text).group(1)) == abi.SETTLE_NOT_YET == sc.SETTLE_NOT_YET == -3
    assert abi.EXIT_NO_PLAN == sc.EXIT_NO_PLAN == -2 and abi.EXIT_HORIZON_MAX == sc.WHOLE == 1 << 30
    from longtermplanner_amd import LongTermPlanner
    assert all(hasattr(LongTermPlanner, name) for name in ("settle", "planSettleHost", "arrival"))
    dropin = open(os.path.join(ROOT, "include", "long_term_planner", "long_term_planner.h")).read()
    assert "planSettleBatch" in dropin
    # the header names what the call does not do and what it guarantees
    doc = _header()
    doc = doc[doc.index("SETTLING"):doc.index("} ltp_settle_opts;")]
    for words in ("first ENTRY", "every exit in between", "which array or joint decided settle_all", "float32", "per-array", "*_multi", "fusing",
                  "exhaustive by construction", "IS outside the box, bit for bit", "<= 1e-12", "unsigned atomicMax", "exactly one kernel",
                  "LTP_SETTLE_NOT_YET", "resting state"):
        assert re.search(r"\s+".join(re.escape(w) for w in words.split()), doc), words
    # the rule is host-testable: no HIP header behind it
    rule = open(os.path.join(ROOT, "longtermplanner_amd", "csrc", "ltp_crossings.hpp")).read()
    assert "hip_runtime" not in rule and "LTP_KNOTS_HD" in rule
    for name in ("last_outside_candidate", "candidate_after", "bisect_inside", "locate_last_outside", "last_outside", "last_outside_constant"):
        assert re.search(r"\b%s\(" % name, rule), name


def test_settle_opts_is_the_c_struct(abi):
    fields = re.search(r"typedef struct \{([^}]*)\} ltp_settle_opts;", _header(), flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    O, F = abi.SettleOpts, abi.FirstExitOpts
    assert re.findall(r"(\w+)(?:\[4\])?;", fields) == [f[0] for f in O._fields_] == ["size", "arrays", "horizon", "uniform_first", "first_sample", "lo", "hi",
                                                                                   "box_query_stride", "box_joint_stride", "settle_all"]
    assert C.sizeof(O) == 112
    assert O.first_sample.offset == 16 and O.lo.offset == 24 and O.hi.offset == 56
    assert O.box_query_stride.offset == 88 and O.box_joint_stride.offset == 96 and O.settle_all.offset == 104
    # ltp_first_exit_opts field for field, settle_all where first_any stands
    assert C.sizeof(F) == 112
    for (name, kind), (f_name, f_kind) in zip(O._fields_, F._fields_):
        assert kind is f_kind and getattr(O, name).offset == getattr(F, f_name).offset and (name == f_name or (name, f_name) == ("settle_all", "first_any"))


def test_settle_calls_are_refused_without_a_handle(abi):
    """A call without a handle is LTP_ERR_INVALID_ARGUMENT whatever its opts hold: nothing is dereferenced, nothing launched, no
    crash on the malformed structs (the strict size rule among them). Which check refuses what on a live handle is
    tests/test_gpu_settle.py::test_refusals_and_bounds."""
    lib = abi.lib()
    O = abi.SettleOpts
    q, r = abi.Queries(), abi.Records()
    P = C.c_void_p * 4

    def call(o):
        return lib.ltp_settle_batch(None, 0, 0, C.byref(q), C.byref(r), C.addressof(o) if o is not None else None, None, 0, None)
    good = dict(size=C.sizeof(O), arrays=15, horizon=240, box_joint_stride=1)
    assert call(O(**good)) == INVALID
    assert call(None) == INVALID
    for bad in (dict(size=0), dict(size=C.sizeof(O) - 8), dict(size=C.sizeof(O) + 4), dict(arrays=0), dict(arrays=16), dict(arrays=-1), dict(horizon=0),
                dict(horizon=-1), dict(horizon=(1 << 30) + 1), dict(arrays=1, lo=P(None, 64, None, None)), dict(hi=P(64, None, None, None), box_joint_stride=0)):
        assert call(O(**dict(good, **bad))) == INVALID, bad
    elements = lib.ltp_settle_elements
    assert elements(None, 10, 15) == 0
    host = lib.ltp_plan_settle_host
    one = np.zeros(4, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    for arrays, horizon, per_plan in ((15, 240, 0), (0, 240, 0), (16, 240, 0), (1, 0, 0), (1, (1 << 30) + 1, 0), (1, 1, 2)):
        assert host(None, 0, None, None, None, None, None, 0, horizon, arrays, None, None, per_plan, None, one, None) == INVALID


def test_mask_horizon_and_boxes_are_checked_by_the_python_wrappers(abi):
    """settle and planSettleHost turn `arrays` into the mask and validate the horizon and the boxes' letters and shapes through
    firstExit's helpers before they touch a device: a call with a bad one never reaches the batch it is given."""
    import torch
    from longtermplanner_amd import LongTermPlanner
    ltp = LongTermPlanner.__new__(LongTermPlanner)              # no handle, no device: the refusals below come first

    class NoBatch:
        dof = 7

        class offsets:
            device = "cpu"
    z = np.zeros((5, 7))
    box, per_plan, wrong = torch.zeros(7, dtype=torch.float64), torch.zeros((5, 7), dtype=torch.float64), torch.zeros(6, dtype=torch.float64)
    for bad in ("", "x", "qq", "qvajq", "Q", 0, 16, -1, 2.0, None, True, ["q"]):
        with pytest.raises(ValueError):
            ltp.settle(NoBatch, 0, 5, 0, 240, arrays=bad)
        with pytest.raises(ValueError):
            ltp.planSettleHost(z, z, z, z, 0, 240, arrays=bad)
    for bad in (0, -1, (1 << 30) + 1, 2.5, None, True, "240"):
        with pytest.raises(ValueError):
            ltp.settle(NoBatch, 0, 5, 0, bad)
        with pytest.raises(ValueError):
            ltp.planSettleHost(z, z, z, z, 0, bad)
    for kw in (dict(lo={"v": box}), dict(hi={"x": box}), dict(lo={"q": wrong}), dict(lo={"q": torch.zeros((4, 7), dtype=torch.float64)}),
               dict(lo=[box]), dict(lo={"q": box}, hi={"q": per_plan}), dict(arrays="qv", lo={"q": box, "v": per_plan}), dict(hi={0: box}),
               dict(lo={"q": 0.5})):
        with pytest.raises(ValueError):
            ltp.settle(NoBatch, 0, 5, 0, 240, **dict(dict(arrays="q"), **kw))
    # (planSettleHost's boxes need the handle's dof: tests/test_gpu_settle.py::test_refusals_and_bounds)
    # arrival's boxes go through the same helper: a goal of the wrong shape is refused there
    with pytest.raises(ValueError):
        ltp.arrival(NoBatch, 0, 5, 0, torch.zeros(6, dtype=torch.float64), 1e-3)
    with pytest.raises(ValueError):
        ltp.arrival(NoBatch, 0, 5, 0, torch.zeros((4, 7), dtype=torch.float64), 1e-3, v_tol=0.01)


DROPIN = r'''
#include "long_term_planner/long_term_planner.h"
#include <cstdio>
int main() {
  using namespace long_term_planner;
  std::vector<double> lo = {-1.0}, hi = {1.0}, one = {1.0};
  try {
    LongTermPlanner ltp(1, 0.001, lo, hi, one, one, one);
    std::vector<int> settle, all;
    const double qg = 0.5, z = 0.0, v_box = 0.25;
    const double* his[4] = {nullptr, &v_box, nullptr, nullptr};
    const int k = 3;
    const long long ok = ltp.planSettleBatch(1, &qg, &z, &z, &z, &k, 0, 1 << 30, LTP_ENV_Q | LTP_ENV_V, nullptr, his, false, settle, &all);
    std::printf("%lld %zu %zu\n", ok, settle.size(), all.size());
    return settle.size() == 2u && all.size() == 1u && LTP_SETTLE_NOT_YET == -3 && LTP_EXIT_NO_PLAN == -2 ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 2;
  }
}
'''


def test_dropin_header_with_plan_settle_batch_compiles_with_plain_gxx(abi, tmp_path):
    src = tmp_path / "settle.cc"
    src.write_text(DROPIN)
    exe = tmp_path / "settle"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "longtermplanner_amd"), "-lltp_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "longtermplanner_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_last_outside_on_the_host(tmp_path, flags):
    """The kernel's settling rule (ltp_crossings.hpp) over random runs of the sampler's magnitudes, Ts in {1e-3, 1/1024, 4e-3},
    stretches of 1 .. 3000 samples and boxes at fractions of the stretch's own range, boxes centred on the stretch's last sample
    (and boxes that hold everything, nothing, one side), against the exhaustive reverse loop over the same fma expressions: a and j
    identical; q and v never later, the reported sample outside, every skipped outside sample outside by <= 1e-12 (counted and
    printed). Degenerate, NaN, infinite and 1e300 coefficients: results and evaluated indices inside [m0, m1], at most 6 + 31
    evaluations per call, nothing undefined. A stand-alone host program with its own main, compiled here, once more with the
    sanitizers; nothing sanitized is loaded into Python."""
    exe = tmp_path / "crossings_test"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "longtermplanner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "crossings_test.cc"), "-o", str(exe)])
    r = subprocess.run([str(exe), "last"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
    assert "earlier than the exhaustive loop by rounding alone" in r.stdout


@pytest.fixture(scope="module")
def oracle_plans(oracle_mod):
    """60 panda plans of the CPU oracle with their trajectories — the seed of the GPU tests' panda batches —, packed into the
    full-row layout (computed once, not modified)."""
    from longtermplanner_amd import generate_queries, limit_set
    dof, lim = limit_set("panda")
    n = 60
    qs = [np.ascontiguousarray(x) for x in generate_queries(n, lim, seed=4242)]
    orc = oracle_mod.Oracle(dof, TS, **lim)
    o = orc.plan_batch(*qs, sample=True)
    trajs = []
    for p in range(n):
        if o["status"][p] == 0:
            trajs.append((0, *[np.zeros((dof, 0))] * 4))
        else:
            trajs.append(orc.get_trajectory(o["t_scaled"][p], o["dir"][p], o["mod"][p], qs[1][p], qs[2][p], qs[3][p], o["v_drive"][p]))
    full, offsets, lens = pack_full_rows(trajs, dof)
    assert np.mean(lens > 0) > 0.9
    return dof, lim, trajs, full, offsets, lens


def _loop(trajs, dof, first, count, k, H, lo, hi):
    """The plain loop: per (plan, array, joint) the samples of [k, k + H) outside the box, the samples past the end by their rule:
    -3 when the horizon's last sample is outside, else the last outside sample + 1, else k."""
    out = np.zeros((count, 4, dof), dtype=np.int64)
    for i in range(count):
        L = trajs[first + i][0]
        if L == 0:
            out[i] = sc.EXIT_NO_PLAN
            continue
        k0 = min(max(int(k[i]), 0), L)
        reach = k0 + H
        for x in range(4):
            arr = trajs[first + i][1 + x]
            for j in range(dof):
                def outside(t):
                    s = arr[j][t] if t < L else (arr[j][L - 1] if x == 0 else 0.0)
                    return s < lo[i, x, j] or s > hi[i, x, j]
                if outside(min(reach - 1, L)):                      # behind sample L nothing changes any more
                    out[i, x, j] = sc.SETTLE_NOT_YET
                    continue
                out[i, x, j] = k0
                for t in range(min(reach - 1, L), k0 - 1, -1):
                    if outside(t):
                        out[i, x, j] = t + 1
                        break
    return out


@pytest.mark.parametrize("horizon", [1, 2, 64, 240, 1 << 30])
def test_checker_against_a_plain_loop(oracle_plans, horizon):
    """The checker's gather, the rule past the end, the last index, NOT_YET and settle_all are what a loop over (plan, array, joint,
    t) reads from the oracle's own trajectories: starts below 0, inside, at traj_len - 1, at traj_len and past it; boxes around each
    row's resting value (end_boxes), boxes at fractions of each row's range, boxes that exclude 0 (v, a, j never settle past the
    end), the default boxes, and a chunk budget small enough for several chunks."""
    import torch
    dof, lim, trajs, full, offsets, lens = oracle_plans
    n = len(trajs)
    rng = np.random.default_rng(31 + horizon % 97)
    k = rng.integers(-3, lens.astype(np.int64) + 4).astype(np.int32)
    k[0::9] = -3
    k[1::9] = lens[1::9]
    k[2::9] = lens[2::9] - 1
    k[3::9] = lens[3::9] + 5
    first, count = 3, n - 5
    T = [torch.from_numpy(x) for x in (full, offsets, lens)]
    kt = torch.from_numpy(k[first:first + count])
    mn, mx = sc.row_ranges(*T, dof, first, count, chunk=7)
    lo, hi = sc.fraction_boxes(mn, mx, seed=5)
    e_lo, e_hi = (b[first:first + count] for b in sc.end_boxes(*T, dof, seed=6))
    # end_boxes is what its docstring says: around the resting value, by 5 .. 45 % of the range that includes it
    for i in range(count):
        L = trajs[first + i][0]
        for x in range(4):
            if not L:
                assert bool(torch.isnan(e_lo[i]).all()) and bool(torch.isnan(e_hi[i]).all())
                continue
            rows = trajs[first + i][1 + x]
            rest = rows[:, -1] if x == 0 else np.zeros(dof)
            w = np.maximum(rows.max(axis=1), rest) - np.minimum(rows.min(axis=1), rest)
            below, above = rest - e_lo[i, x].numpy(), e_hi[i, x].numpy() - rest
            assert (below >= 0.05 * w - 1e-15).all() and (below <= 0.45 * w + 1e-15).all() and (above >= 0.05 * w - 1e-15).all() and (above <= 0.45 * w + 1e-15).all()
    d_lo, d_hi = sc.default_boxes(count, lim, "cpu")
    above0 = torch.full_like(lo, 1e-9)                             # every array's box excludes 0 from below: v, a, j never settle past the end
    seen = dict(index=0, at_k=0, not_yet=0, at_len=0)
    for name, (b_lo, b_hi) in dict(ends=(e_lo, e_hi), fractions=(lo, hi), default=(d_lo, d_hi), above=(above0, torch.full_like(hi, 1e9))).items():
        want = _loop(trajs, dof, first, count, k[first:first + count], horizon, b_lo.numpy(), b_hi.numpy())
        got, got_all = sc.expected_settle(*T, kt, horizon, dof, first, count, b_lo, b_hi, budget=4 * dof * 5000)
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want), name
        for i in range(count):
            w = want[i]
            folded = -2 if (w == -2).any() else -3 if (w == -3).any() else w.max()
            assert int(got_all[i]) == folded, (name, i)
        L = lens[first:first + count].astype(np.int64)[:, None, None]
        k0 = np.minimum(np.maximum(k[first:first + count].astype(np.int64), 0)[:, None, None], L)
        seen["index"] += int(((want > k0) & (L > 0)).sum())
        seen["at_k"] += int(((want == k0) & (L > 0)).sum())
        seen["not_yet"] += int((want == sc.SETTLE_NOT_YET).sum())
        seen["at_len"] += int(((want == L) & (L > 0) & (k0 < L)).sum())
        # a sub-mask is its planes of the full mask, in the order q, v, a, j
        for mask in (1, 2, 12, 9):
            part, part_all = sc.expected_settle(*T, kt, horizon, dof, first, count, b_lo, b_hi, mask=mask)
            assert np.array_equal(part.numpy(), want[:, selected(mask)])
            assert torch.equal(part_all, sc.fold_all(torch.from_numpy(want[:, selected(mask)])).int())
    # (H = 1 admits no index above k; a row whose last sample is outside while its resting value is inside — the jerk rows — shows
    # as the index traj_len where the horizon reaches past the end)
    assert seen["at_k"] > 0 and seen["not_yet"] > 0 and (horizon == 1 or seen["index"] > 0) and (horizon < sc.WHOLE or seen["at_len"] > 0), seen
    uni, _ = sc.expected_settle(*T, 7, horizon, dof, first, count, e_lo, e_hi)
    assert np.array_equal(uni.numpy(), _loop(trajs, dof, first, count, np.full(count, 7), horizon, e_lo.numpy(), e_hi.numpy()))


def test_fold_all_orders_the_codes_as_unsigned():
    import torch
    table = torch.tensor([[[5, 9], [0, 3]], [[5, -3], [7, 1]], [[-2, -2], [-2, -2]], [[0, 0], [0, 0]], [[-3, -2], [4, 4]]], dtype=torch.int32)
    assert sc.fold_all(table).tolist() == [9, -3, -2, 0, -2]


def test_both_box_families_give_both_outcomes(oracle_plans):
    """The condition the GPU tests rest on, on the oracle's rows of the panda seed they use: with end_boxes, k = 0 and H = 2^30 at
    least 90 % of the lanes of planned plans have 0 < s <= traj_len (only constant rows are excepted: every other row starts or
    peaks outside such a box and rests inside it); with box_checker.fraction_boxes the bulk answer for q is NOT_YET. Both
    families go to the GPU, so neither outcome is the only one tested."""
    import torch
    dof, lim, trajs, full, offsets, lens = oracle_plans
    n = len(trajs)
    T = [torch.from_numpy(x) for x in (full, offsets, lens)]
    planned = torch.from_numpy(lens > 0)
    L = T[2].long()[:, None, None]
    e_lo, e_hi = sc.end_boxes(*T, dof, seed=7)
    s, _ = sc.expected_settle(*T, 0, sc.WHOLE, dof, 0, n, e_lo, e_hi)
    inside = ((s > 0) & (s <= L))[planned]
    mn, mx = sc.row_ranges(*T, dof, 0, n)
    constant = (e_lo == e_hi)[planned]                             # range 0 with the resting value included: the degenerate box
    assert bool((inside | constant).all()), "a non-constant row does not settle inside its end box"
    assert float(inside.double().mean()) >= 0.9, float(inside.double().mean())
    assert not bool((s[planned] == sc.SETTLE_NOT_YET).any())
    f_lo, f_hi = sc.fraction_boxes(mn, mx, seed=7)
    s, _ = sc.expected_settle(*T, 0, sc.WHOLE, dof, 0, n, f_lo, f_hi)
    q = s[planned][:, 0]
    assert float((q == sc.SETTLE_NOT_YET).double().mean()) > 0.5, "fraction boxes: q mostly rests outside (the goal is an extreme of the row)"
    assert int((s[planned] >= 0).sum()) > 0
