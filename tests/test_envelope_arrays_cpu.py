"""Horizon envelopes of q, v, a and j (ltp_envelope_knots_arrays_batch, include/ltp_hip.h) without a device: the symbols, the
options struct, the validation that runs before anything is launched, the Python wrapper's ValueError cases, the drop-in header's
new method under plain g++, the candidate rule of the kernel on the host (tests/cpp/envelope_arrays_extremes_test.cc, also under the
address, undefined-behaviour and float-cast sanitizers), and the yardstick of the GPU tests (tests/envelope_checker.py) against a
plain loop over the CPU oracle's trajectories (tests/envelope_cpu_helpers.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import envelope_checker as ac
import envelope_cpu_helpers as eh
from envelope_cpu_helpers import INVALID, ROOT, abi, oracle_plans   # noqa: F401 (fixtures)

NAMES = ("ltp_envelope_knots_arrays_elements", "ltp_envelope_knots_arrays_batch", "ltp_plan_envelope_knots_arrays_host")


def test_envelope_arrays_symbols_are_declared_bound_and_exported(abi):
    eh.assert_declared_and_exported(abi, NAMES)
    text = eh.header(comments=False)
    for name, value in (("LTP_ENV_Q", abi.ENV_Q), ("LTP_ENV_V", abi.ENV_V), ("LTP_ENV_A", abi.ENV_A), ("LTP_ENV_J", abi.ENV_J)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value
    assert (abi.ENV_Q, abi.ENV_V, abi.ENV_A, abi.ENV_J) == (ac.ENV_Q, ac.ENV_V, ac.ENV_A, ac.ENV_J) == (1, 2, 4, 8)
    from longtermplanner_amd import LongTermPlanner
    assert hasattr(LongTermPlanner, "envelopeKnotsArrays") and hasattr(LongTermPlanner, "planEnvelopeKnotsArraysHost")
    dropin = open(os.path.join(ROOT, "include", "long_term_planner", "long_term_planner.h")).read()
    assert "planEnvelopeKnotsArraysBatch" in dropin
    # the contract of the q-only call no longer calls the other three arrays out of scope
    doc = eh.header()
    old = doc[doc.index("HORIZON ENVELOPES"):doc.index("} ltp_envelope_knots_opts;")]
    assert "Out of scope: envelopes of v, a or j" not in old and "ltp_envelope_knots_arrays_batch" in old


def test_envelope_arrays_opts_is_the_c_struct(abi):
    O = abi.EnvelopeArraysOpts
    eh.assert_opts_is_the_c_struct(abi, NAMES, "ltp_envelope_arrays_opts", O,
                                   ["size", "n_intervals", "closed", "uniform_first", "arrays", "reserved", "edge_offsets", "first_sample", "valid"])
    assert C.sizeof(O) == 48
    assert O.arrays.offset == 16 and O.reserved.offset == 20
    assert O.edge_offsets.offset == 24 and O.first_sample.offset == 32 and O.valid.offset == 40
    assert C.sizeof(abi.EnvelopeKnotsOpts) == 40                 # the struct this one stands next to is what it was


def test_envelope_arrays_calls_are_refused_without_a_handle(abi):
    """A call without a handle is LTP_ERR_INVALID_ARGUMENT whatever its opts hold: nothing is dereferenced, nothing launched, no
    crash on the malformed structs. Which check refuses what on a live handle is tests/test_gpu_envelope_arrays.py::test_refusals."""
    lib = abi.lib()
    O = abi.EnvelopeArraysOpts
    q, r = abi.Queries(), abi.Records()

    def call(o):
        return lib.ltp_envelope_knots_arrays_batch(None, 0, 0, C.byref(q), C.byref(r), C.addressof(o) if o is not None else None, None, 0, None)
    good = dict(size=C.sizeof(O), n_intervals=39, closed=0, arrays=15, reserved=0, edge_offsets=64)     # a pointer nobody follows
    assert call(O(**good)) == INVALID
    assert call(None) == INVALID
    for bad in (dict(size=0), dict(size=C.sizeof(O) - 8), dict(size=C.sizeof(O) + 4), dict(closed=2), dict(closed=-1), dict(n_intervals=0),
                dict(n_intervals=-1), dict(n_intervals=ac.MAX_INTERVALS + 1), dict(edge_offsets=None), dict(arrays=0), dict(arrays=16),
                dict(arrays=-1), dict(reserved=1)):
        assert call(O(**dict(good, **bad))) == INVALID, bad
    elements = lib.ltp_envelope_knots_arrays_elements
    assert elements(None, 10, 4, 15) == 0
    g = (C.c_int * 3)(0, 4, 9)
    host = lib.ltp_plan_envelope_knots_arrays_host
    for arrays in (15, 0, 16):
        assert host(None, 0, None, None, None, None, None, 0, 2, g, 0, arrays, None, None, None) == INVALID
    assert host(None, 0, None, None, None, None, None, 0, 2, None, 0, 15, None, None, None) == INVALID


def test_arrays_and_host_edges_are_checked_by_the_python_wrapper(abi):
    """envelopeKnotsArrays turns `arrays` into the mask and validates a host edge list before it touches a device: a call with a
    bad one never reaches the batch it is given."""
    from longtermplanner_amd import LongTermPlanner
    mask = LongTermPlanner._env_arrays
    assert mask("qvaj") == 15 and mask("q") == 1 and mask("v") == 2 and mask("aj") == 12 and mask("jq") == 9 and mask(7) == 7 and mask(np.int32(3)) == 3
    ltp = LongTermPlanner.__new__(LongTermPlanner)              # no handle, no device: the refusals below come first

    class NoBatch:
        class offsets:
            device = "cpu"
    for bad in ("", "x", "qq", "qvajq", "Q", 0, 16, -1, 2.0, None, True, ["q"]):
        with pytest.raises(ValueError):
            ltp.envelopeKnotsArrays(NoBatch, 0, 1, 0, [0, 4, 9], arrays=bad)
        with pytest.raises(ValueError):
            ltp.planEnvelopeKnotsArraysHost(None, None, None, None, 0, [0, 4, 9], arrays=bad)
    for bad in ([], [11], [3, 2], [0, 5, 4, 9], [-1, 0], [0, (1 << 30) + 1], list(range(ac.MAX_INTERVALS + 2)), [0.5, 1.5], [[0, 1], [2, 3]]):
        with pytest.raises(ValueError):
            ltp.envelopeKnotsArrays(NoBatch, 0, 1, 0, bad)


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
    const long long ok = ltp.planEnvelopeKnotsArraysBatch(1, &qg, &z, &z, &z, &k, 0, edges, true, LTP_ENV_V | LTP_ENV_A | LTP_ENV_J, env, &valid);
    std::printf("%lld %zu %zu\n", ok, env.size(), valid.size());
    return env.size() == 3u * 8u * 2u && valid.size() == 1u ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 2;
  }
}
'''


def test_dropin_header_with_plan_envelope_knots_arrays_batch_compiles_with_plain_gxx(abi, tmp_path):
    eh.compile_dropin(tmp_path, "envelope_arrays", DROPIN)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_envelope_arrays_extremes_on_the_host(tmp_path, flags):
    """The kernel's candidate rule (ltp_extremes.hpp) over random runs of the sampler's magnitudes, Ts in {1e-3, 1/1024, 4e-3},
    stretches of 1 .. 3000 samples, against the exhaustive loop over the same fma expressions: v inside it and within 1e-12, a and j
    equal; c[6] == 0, c[5] == c[6] == 0, stretches of 1, 2 and 3 samples; NaN, infinite and 1e300 coefficients (every candidate
    index inside [m0, m1], nothing undefined). A stand-alone host program, compiled here, once more with the sanitizers."""
    eh.run_rule_program(tmp_path, "envelope_arrays_extremes_test", flags)


@pytest.mark.parametrize("closed", [0, 1])
@pytest.mark.parametrize("grid", ["duplicates", "from37", "n33"])
def test_checker_against_a_plain_loop(oracle_plans, grid, closed):
    """The checker's gather, the rule past the end, the per-interval reduction of all four arrays and `valid` are what a loop over
    (plan, array, joint, w, t) reads from the oracle's own trajectories: starts below 0, inside and at or past the end; intervals
    that end past the end and intervals that start there both occur. A sub-mask is the planes of the full one."""
    import torch
    env, valid, planned, args, (starts_past, ends_past, _) = eh.plain_loop(oracle_plans, grid, closed, 15)
    assert starts_past > 0 and ends_past > 0
    # a sub-mask is its planes of the full mask, in the order q, v, a, j
    for mask in (1, 2, 12, 9):
        part, valid2, _ = ac.expected(*args, mask=mask, chunk=16)
        assert np.array_equal(part.numpy().view(np.int64), env[:, ac.selected(mask)].view(np.int64)) and torch.equal(valid, valid2)
    assert ac.selected(12) == [2, 3] and ac.selected(9) == [0, 3]
    # the acceptance rules accept the yardstick itself; q and v refuse a value outside the samples, a far value and a NaN, a and j
    # any other value and a NaN, and take -0.0 for +0.0
    red = torch.from_numpy(env)
    bad, figures = ac.compare(red.clone(), red, planned)
    assert not bad.any() and figures == {"q": (0.0, 1.0), "v": (0.0, 1.0)}
    pi = int(np.nonzero(planned.numpy())[0][0])
    for x in (0, 1):
        for change in (lambda t: t[pi, x, 0, 0, 0].sub_(1e-15), lambda t: t[pi, x, 0, 0, 1].add_(1e-15), lambda t: t[pi, x, 0, 0, 0].add_(1e-11),
                       lambda t: t[pi, x, 0, 0, 0].fill_(float("nan"))):
            other = red.clone()
            change(other)
            assert bool(ac.compare(other, red, planned)[0][pi]), x
    for x in (2, 3):
        for change in (lambda t: t[pi, x, 0, 0, 0].sub_(1.0), lambda t: t[pi, x, 0, 0, 1].add_(1.0), lambda t: t[pi, x, 0, 0, 0].fill_(float("nan"))):
            other = red.clone()
            change(other)
            assert bool(ac.compare(other, red, planned)[0][pi]), x
    zeros = (red[:, 2:] == 0.0)
    assert bool(zeros.any())
    flipped = torch.where(torch.cat([torch.zeros_like(red[:, :2], dtype=torch.bool), zeros], dim=1), -red, red)
    assert not ac.compare(flipped, red, planned)[0].any()
