"""First exits (ltp_first_exit_batch, include/ltp_hip.h) without a device: the symbols, the options struct, the validation that
runs before anything is launched, the Python wrapper's ValueError cases, the drop-in header's new method under plain g++, the
first-exit rule of the kernel on the host (tests/cpp/crossings_test.cc first, also under the address, undefined-behaviour and
float-cast sanitizers), and the yardstick of the GPU tests (tests/box_checker.py) against a plain loop over the CPU oracle's
trajectories."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import box_checker as fc
from envelope_checker import selected
from horizon_checker import TS, pack_full_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NAMES = ("ltp_first_exit_elements", "ltp_first_exit_batch", "ltp_plan_first_exit_host")


@pytest.fixture(scope="module")
def abi():
    from longtermplanner_amd import _abi
    _abi.build()
    return _abi


def _header():
    return open(os.path.join(ROOT, "include", "ltp_hip.h")).read()


def test_first_exit_symbols_are_declared_bound_and_exported(abi):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = C.CDLL(abi.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} is not declared in include/ltp_hip.h"
        assert n in abi.exported_symbols(), f"{n} is not declared in _abi._SIGNATURES"
        assert hasattr(lib, n), f"{n} is not exported"
        args = re.search(r"\b%s\s*\(([^;]*)\);" % n, text, flags=re.S).group(1)
        assert len(args.split(",")) == len(abi._SIGNATURES[n][1]), n
    for name, value in (("LTP_EXIT_NONE", abi.EXIT_NONE), ("LTP_EXIT_NO_PLAN", abi.EXIT_NO_PLAN)):
        assert int(re.search(r"#define %s\s+\((-?\d+)\)" % name, text).group(1)) == value
    assert (abi.EXIT_NONE, abi.EXIT_NO_PLAN) == (fc.EXIT_NONE, fc.EXIT_NO_PLAN) == (-1, -2) and abi.EXIT_HORIZON_MAX == fc.WHOLE == 1 << 30
    from longtermplanner_amd import LongTermPlanner
    assert hasattr(LongTermPlanner, "firstExit") and hasattr(LongTermPlanner, "planFirstExitHost")
    dropin = open(os.path.join(ROOT, "include", "long_term_planner", "long_term_planner.h")).read()
    assert "planFirstExitBatch" in dropin
    # the header names what the call does not do, and the two remarks a caller needs
    doc = _header()
    doc = doc[doc.index("FIRST EXITS"):doc.index("} ltp_first_exit_opts;")]
    for words in ("first ENTRY", "LAST exit", "which array or joint won", "float32", "per-array", "*_multi", "fusing", "exceed a_max by rounding",
                  "PATH-limit verdict"):
        assert re.search(r"\s+".join(re.escape(w) for w in words.split()), doc), words
    # the rule is host-testable: no HIP header behind it
    rule = open(os.path.join(ROOT, "longtermplanner_amd", "csrc", "ltp_crossings.hpp")).read()
    assert "hip_runtime" not in rule and "LTP_KNOTS_HD" in rule and "first_outside" in rule


def test_first_exit_opts_is_the_c_struct(abi):
    fields = re.search(r"typedef struct \{([^}]*)\} ltp_first_exit_opts;", _header(), flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    O = abi.FirstExitOpts
    assert re.findall(r"(\w+)(?:\[4\])?;", fields) == [f[0] for f in O._fields_] == ["size", "arrays", "horizon", "uniform_first", "first_sample", "lo", "hi",
                                                                                   "box_query_stride", "box_joint_stride", "first_any"]
    assert C.sizeof(O) == 112
    assert O.first_sample.offset == 16 and O.lo.offset == 24 and O.hi.offset == 56
    assert O.box_query_stride.offset == 88 and O.box_joint_stride.offset == 96 and O.first_any.offset == 104
    assert C.sizeof(abi.EnvelopeArraysOpts) == 48                 # the struct this one stands next to is what it was


def test_first_exit_calls_are_refused_without_a_handle(abi):
    """A call without a handle is LTP_ERR_INVALID_ARGUMENT whatever its opts hold: nothing is dereferenced, nothing launched, no
    crash on the malformed structs (the strict size rule among them). Which check refuses what on a live handle is
    tests/test_gpu_first_exit.py::test_refusals_and_bounds."""
    lib = abi.lib()
    O = abi.FirstExitOpts
    q, r = abi.Queries(), abi.Records()
    P = C.c_void_p * 4

    def call(o):
        return lib.ltp_first_exit_batch(None, 0, 0, C.byref(q), C.byref(r), C.addressof(o) if o is not None else None, None, 0, None)
    good = dict(size=C.sizeof(O), arrays=15, horizon=240, box_joint_stride=1)
    assert call(O(**good)) == INVALID
    assert call(None) == INVALID
    for bad in (dict(size=0), dict(size=C.sizeof(O) - 8), dict(size=C.sizeof(O) + 4), dict(arrays=0), dict(arrays=16), dict(arrays=-1), dict(horizon=0),
                dict(horizon=-1), dict(horizon=(1 << 30) + 1), dict(arrays=1, lo=P(None, 64, None, None)), dict(hi=P(64, None, None, None), box_joint_stride=0)):
        assert call(O(**dict(good, **bad))) == INVALID, bad
    elements = lib.ltp_first_exit_elements
    assert elements(None, 10, 15) == 0
    host = lib.ltp_plan_first_exit_host
    one = np.zeros(4, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    for arrays, horizon, per_plan in ((15, 240, 0), (0, 240, 0), (16, 240, 0), (1, 0, 0), (1, (1 << 30) + 1, 0), (1, 1, 2)):
        assert host(None, 0, None, None, None, None, None, 0, horizon, arrays, None, None, per_plan, None, one, None) == INVALID


def test_mask_horizon_and_boxes_are_checked_by_the_python_wrapper(abi):
    """firstExit and planFirstExitHost turn `arrays` into the mask and validate the horizon and the boxes' letters and shapes before
    they touch a device: a call with a bad one never reaches the batch it is given."""
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
            ltp.firstExit(NoBatch, 0, 5, 0, 240, arrays=bad)
        with pytest.raises(ValueError):
            ltp.planFirstExitHost(z, z, z, z, 0, 240, arrays=bad)
    for bad in (0, -1, (1 << 30) + 1, 2.5, None, True, "240"):
        with pytest.raises(ValueError):
            ltp.firstExit(NoBatch, 0, 5, 0, bad)
        with pytest.raises(ValueError):
            ltp.planFirstExitHost(z, z, z, z, 0, bad)
    for kw in (dict(lo={"v": box}), dict(hi={"x": box}), dict(lo={"q": wrong}), dict(lo={"q": torch.zeros((4, 7), dtype=torch.float64)}),
               dict(lo=[box]), dict(lo={"q": box}, hi={"q": per_plan}), dict(arrays="qv", lo={"q": box, "v": per_plan}), dict(hi={0: box}),
               dict(lo={"q": 0.5})):
        with pytest.raises(ValueError):
            ltp.firstExit(NoBatch, 0, 5, 0, 240, **dict(dict(arrays="q"), **kw))
    boxes = LongTermPlanner._exit_boxes
    assert boxes(None, None, 1, 5, 7) == ([None] * 4, [None] * 4, False)
    lo_by, hi_by, each = boxes({"v": box}, {"q": box, "v": None}, 3, 5, 7)
    assert lo_by[1] is box and hi_by[0] is box and lo_by[0] is None and hi_by[1] is None and each is False
    assert boxes({"j": per_plan}, None, 8, 5, 7)[2] is True


DROPIN = r'''
#include "long_term_planner/long_term_planner.h"
#include <cstdio>
int main() {
  using namespace long_term_planner;
  std::vector<double> lo = {-1.0}, hi = {1.0}, one = {1.0};
  try {
    LongTermPlanner ltp(1, 0.001, lo, hi, one, one, one);
    std::vector<int> exits, any;
    const double qg = 0.5, z = 0.0, v_box = 0.25;
    const double* his[4] = {nullptr, &v_box, nullptr, nullptr};
    const int k = 3;
    const long long ok = ltp.planFirstExitBatch(1, &qg, &z, &z, &z, &k, 0, 1 << 30, LTP_ENV_Q | LTP_ENV_V, nullptr, his, false, exits, &any);
    std::printf("%lld %zu %zu\n", ok, exits.size(), any.size());
    return exits.size() == 2u && any.size() == 1u && LTP_EXIT_NONE == -1 && LTP_EXIT_NO_PLAN == -2 ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 2;
  }
}
'''


def test_dropin_header_with_plan_first_exit_batch_compiles_with_plain_gxx(abi, tmp_path):
    src = tmp_path / "first_exit.cc"
    src.write_text(DROPIN)
    exe = tmp_path / "first_exit"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "longtermplanner_amd"), "-lltp_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "longtermplanner_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_first_outside_on_the_host(tmp_path, flags):
    """The kernel's first-exit rule (ltp_crossings.hpp) over random runs of the sampler's magnitudes, Ts in {1e-3, 1/1024, 4e-3},
    stretches of 1 .. 3000 samples and boxes at fractions of the stretch's own range (and boxes that hold everything, nothing, one
    side), against the exhaustive loop over the same fma expressions: a and j identical; q and v never earlier, the reported sample
    outside, every skipped outside sample outside by <= 1e-12 (counted and printed). Degenerate, NaN, infinite and 1e300
    coefficients: results and evaluated indices inside [m0, m1], at most 6 + 31 evaluations per call, nothing undefined. A
    stand-alone host program, compiled here, once more with the sanitizers."""
    exe = tmp_path / "crossings_test"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "longtermplanner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "crossings_test.cc"), "-o", str(exe)])
    r = subprocess.run([str(exe), "first"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
    assert "later than the exhaustive loop by rounding alone" in r.stdout


@pytest.fixture(scope="module")
def oracle_plans(oracle_mod):
    """60 panda plans of the CPU oracle with their trajectories, packed into the full-row layout (computed once, not modified)."""
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
    """The plain loop: per (plan, array, joint) the first t of [k, k + H) outside the box, the samples past the end by their rule."""
    out = np.full((count, 4, dof), fc.EXIT_NONE, dtype=np.int64)
    for i in range(count):
        L = trajs[first + i][0]
        if L == 0:
            out[i] = fc.EXIT_NO_PLAN
            continue
        k0 = min(max(int(k[i]), 0), L)
        for x in range(4):
            arr = trajs[first + i][1 + x]
            for j in range(dof):
                for t in range(k0, min(k0 + H, L + 1)):             # behind sample L nothing changes any more
                    s = arr[j][t] if t < L else (arr[j][L - 1] if x == 0 else 0.0)
                    if s < lo[i, x, j] or s > hi[i, x, j]:
                        out[i, x, j] = t
                        break
    return out


@pytest.mark.parametrize("horizon", [1, 2, 64, 240, 1 << 30])
def test_checker_against_a_plain_loop(oracle_plans, horizon):
    """The checker's gather, the rule past the end, the first index and first_any are what a loop over (plan, array, joint, t) reads
    from the oracle's own trajectories: starts below 0, inside and at or past the end; boxes at fractions of each row's range, boxes
    that exclude 0 (an exit only past the end), the default boxes, and a chunk budget small enough for several chunks."""
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
    mn, mx = fc.row_ranges(*T, dof, first, count, chunk=7)
    for i in range(count):
        L = trajs[first + i][0]
        for x in range(4):
            if L:
                assert np.array_equal(mn[i, x].numpy(), trajs[first + i][1 + x].min(axis=1)) and np.array_equal(mx[i, x].numpy(), trajs[first + i][1 + x].max(axis=1))
            else:
                assert bool(torch.isnan(mn[i]).all()) and bool(torch.isnan(mx[i]).all())
    lo, hi = fc.fraction_boxes(mn, mx, seed=5)
    w = (mx - mn)[lens[first:first + count] > 0]
    assert bool(((lo >= mn + 0.05 * (mx - mn)) & (hi <= mx - 0.05 * (mx - mn)))[lens[first:first + count] > 0].all()) and float(w.max()) > 0
    d_lo, d_hi = fc.default_boxes(count, lim, "cpu")
    assert d_lo.shape == (count, 4, dof) and float(d_lo[0, 1, 0]) == -lim["v_max"][0] and float(d_hi[0, 0, 2]) == lim["q_max"][2]
    above = torch.full_like(lo, 1e-9)                              # every array's box excludes 0 from below: v, a, j exit past the end at the latest
    seen = dict(exit=0, none=0, past=0, at_k=0)
    for name, (b_lo, b_hi) in dict(fractions=(lo, hi), default=(d_lo, d_hi), above=(above, torch.full_like(hi, 1e9))).items():
        want = _loop(trajs, dof, first, count, k[first:first + count], horizon, b_lo.numpy(), b_hi.numpy())
        got, got_any = fc.expected_exits(*T, kt, horizon, dof, first, count, b_lo, b_hi, budget=4 * dof * 5000)
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want), name
        for i in range(count):
            real = want[i][want[i] >= 0]
            assert int(got_any[i]) == (real.min() if real.size else want[i].max()), (name, i)
        L = lens[first:first + count].astype(np.int64)[:, None, None]
        k0 = np.minimum(np.maximum(k[first:first + count].astype(np.int64), 0)[:, None, None], L)
        seen["exit"] += int((want >= 0).sum())
        seen["none"] += int((want == -1).sum())
        seen["past"] += int(((want == L) & (L > 0)).sum())
        seen["at_k"] += int(((want == k0) & (L > 0)).sum())
        # a sub-mask is its planes of the full mask, in the order q, v, a, j
        for mask in (1, 2, 12, 9):
            part, part_any = fc.expected_exits(*T, kt, horizon, dof, first, count, b_lo, b_hi, mask=mask)
            assert np.array_equal(part.numpy(), want[:, selected(mask)])
            assert torch.equal(part_any, fc.fold_any(torch.from_numpy(want[:, selected(mask)])).int())
    assert all(v > 0 for v in seen.values()), seen
    uni, _ = fc.expected_exits(*T, 7, horizon, dof, first, count, lo, hi)
    assert np.array_equal(uni.numpy(), _loop(trajs, dof, first, count, np.full(count, 7), horizon, lo.numpy(), hi.numpy()))
