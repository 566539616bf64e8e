"""Horizon envelopes (ltp_envelope_knots_batch, include/ltp_hip.h) without a device: the symbols, the options struct, the validation
that runs before anything is launched, the drop-in header's new method under plain g++, the host arithmetic of the kernel's interval
walk (tests/cpp/envelope_knots_ranges_test.cc, also under the address and undefined-behaviour sanitizers), and the yardstick of the
GPU tests (tests/envelope_checker.py) against a plain loop over the CPU oracle's trajectories (tests/envelope_cpu_helpers.py)."""
import ctypes as C

import numpy as np
import pytest

import envelope_checker as ec
import envelope_cpu_helpers as eh
from envelope_cpu_helpers import INVALID, abi, oracle_plans   # noqa: F401 (fixtures)

NAMES = ("ltp_envelope_knots_elements", "ltp_envelope_knots_batch", "ltp_plan_envelope_knots_host")


def test_envelope_knots_symbols_are_declared_and_exported(abi):
    eh.assert_declared_and_exported(abi, NAMES)
    assert ec.MAX_INTERVALS == abi.MAX_KNOTS - 1 == 511
    from longtermplanner_amd import LongTermPlanner
    assert hasattr(LongTermPlanner, "envelopeKnots") and hasattr(LongTermPlanner, "planEnvelopeKnotsHost")
    # the header says which rule does not apply and which form the values have
    doc = eh.header()
    at = doc.index("HORIZON ENVELOPES")
    assert "ltp_set_envelope_mode" in doc[at:doc.index("} ltp_envelope_knots_opts;")]


def test_envelope_knots_opts_is_the_c_struct(abi):
    O = abi.EnvelopeKnotsOpts
    eh.assert_opts_is_the_c_struct(abi, NAMES, "ltp_envelope_knots_opts", O,
                                   ["size", "n_intervals", "closed", "uniform_first", "edge_offsets", "first_sample", "valid"])
    assert C.sizeof(O) == 40
    assert O.edge_offsets.offset == 16 and O.first_sample.offset == 24 and O.valid.offset == 32
    assert C.sizeof(abi.KnotsOpts) == 40                         # the struct this one stands next to is what it was


def test_envelope_knots_calls_are_refused_without_a_handle(abi):
    """A call without a handle is LTP_ERR_INVALID_ARGUMENT whatever its opts hold: nothing is dereferenced, nothing launched, no
    crash on the malformed structs. Which check refuses what on a live handle is tests/test_gpu_envelope_knots.py::test_refusals."""
    lib = abi.lib()
    O = abi.EnvelopeKnotsOpts
    q, r = abi.Queries(), abi.Records()

    def call(o):
        return lib.ltp_envelope_knots_batch(None, 0, 0, C.byref(q), C.byref(r), C.addressof(o) if o is not None else None, None, 0, None)
    good = dict(size=C.sizeof(O), n_intervals=39, closed=0, edge_offsets=64)     # a pointer nobody follows
    assert call(O(**good)) == INVALID
    assert call(None) == INVALID
    for bad in (dict(size=0), dict(size=C.sizeof(O) - 8), dict(size=C.sizeof(O) + 4), dict(closed=2), dict(closed=-1), dict(n_intervals=0),
                dict(n_intervals=-1), dict(n_intervals=ec.MAX_INTERVALS + 1), dict(edge_offsets=None)):
        assert call(O(**dict(good, **bad))) == INVALID, bad
    assert lib.ltp_envelope_knots_elements(None, 10, 4) == 0
    g = (C.c_int * 3)(0, 4, 9)
    host = lib.ltp_plan_envelope_knots_host
    assert host(None, 0, None, None, None, None, None, 0, 2, g, 0, None, None, None) == INVALID
    assert host(None, 0, None, None, None, None, None, 0, 2, None, 0, None, None, None) == INVALID


def test_host_edges_are_checked_by_the_python_wrapper(abi):
    """envelopeKnots validates a host edge list through the knots rule (plus: at least two edges) before it touches a device; a
    call with a bad list never reaches the batch it is given."""
    from longtermplanner_amd import LongTermPlanner
    check = LongTermPlanner._checked_knots
    for name, g in ec.EDGE_GRIDS.items():
        assert np.array_equal(check(g), g), name
    assert "one" not in ec.EDGE_GRIDS and len(ec.GRIDS["one"]) == 1
    ltp = LongTermPlanner.__new__(LongTermPlanner)              # no handle, no device: the refusals below come first

    class NoBatch:
        class offsets:
            device = "cpu"
    for bad in ([], [11], ec.GRIDS["one"], [3, 2], [0, 5, 4, 9], [-1, 0], [0, (1 << 30) + 1], list(range(ec.MAX_INTERVALS + 2)), [0.5, 1.5],
                [[0, 1], [2, 3]]):
        with pytest.raises(ValueError):
            ltp.envelopeKnots(NoBatch, 0, 1, 0, bad)


DROPIN = r'''
#include "long_term_planner/long_term_planner.h"
#include <cstdio>
int main() {
  using namespace long_term_planner;
  std::vector<double> lo = {-1.0}, hi = {1.0}, one = {1.0};
  try {
    LongTermPlanner ltp(1, 0.001, lo, hi, one, one, one);
    std::vector<double> env;
    std::vector<int> valid;
    const std::vector<int> edges = {0, 1, 2, 3, 8, 8, 16, 64, 240};
    const double qg = 0.5, z = 0.0;
    const int k = 3;
    const long long ok = ltp.planEnvelopeKnotsBatch(1, &qg, &z, &z, &z, &k, 0, edges, true, env, &valid);
    std::printf("%lld %zu %zu\n", ok, env.size(), valid.size());
    return env.size() == 8u * 2u && valid.size() == 1u ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 2;
  }
}
'''


def test_dropin_header_with_plan_envelope_knots_batch_compiles_with_plain_gxx(abi, tmp_path):
    eh.compile_dropin(tmp_path, "envelope_knots", DROPIN)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_envelope_knots_ranges_on_the_host(tmp_path, flags):
    """The kernel's interval walk (ltp_intervals.hpp) over random cut lists. Valid grids: the stretches of interval w unite to
    exactly [a_w, min(b_w, len - 1)], in order, each inside one run; at most one interval is carried across a cut. All grids, the
    contract-breaking ones included: every index in [0, M), each pair written once, at most M + runs steps. A stand-alone host
    program, compiled here, once more with the sanitizers."""
    eh.run_rule_program(tmp_path, "envelope_knots_ranges_test", flags)


@pytest.mark.parametrize("closed", [0, 1])
@pytest.mark.parametrize("grid", ["duplicates", "from37", "n33"])
def test_checker_against_a_plain_loop(oracle_plans, grid, closed):
    """The checker's gather, clamp, per-interval reduction and `valid` for mask q are what a loop over (plan, joint, w, t) reads from
    the oracle's own trajectories, byte for byte: starts below 0, inside and at or past the end. expected_q is that plane."""
    import torch
    env, valid, planned, args, (held, ended_in, singles) = eh.plain_loop(oracle_plans, grid, closed, ec.ENV_Q)
    assert held > 0 and ended_in > 0 and (singles > 0 or grid != "duplicates")
    red, valid_q, planned_q = ec.expected_q(*args, chunk=16)
    assert red.shape == env[:, 0].shape and red.numpy().tobytes() == env[:, 0].tobytes()
    assert torch.equal(valid_q, valid) and torch.equal(planned_q, planned)
    # the acceptance rule accepts the yardstick itself, and refuses a value outside the samples, a far value and a NaN
    bad, worst, share = ec.compare_analytic(red.clone(), red, planned)
    assert not bad.any() and worst == 0.0 and share == 1.0
    pi = int(np.nonzero(planned.numpy())[0][0])
    for change in (lambda x: x[pi, 0, 0, 0].sub_(1e-15), lambda x: x[pi, 0, 0, 1].add_(1e-15), lambda x: x[pi, 0, 0, 0].add_(1e-11),
                   lambda x: x[pi, 0, 0, 0].fill_(float("nan"))):
        other = red.clone()
        change(other)
        assert bool(ec.compare_analytic(other, red, planned)[0][pi])
