"""Strided horizon windows (ltp_sample_horizon_batch, include/ltp_hip.h) on the GPU: element w of a row is trajectory sample
k + w * s. Compared with the rows the full-row sampler wrote for the same batch (tests/horizon_checker.py, itself pinned to a plain
loop by tests/test_horizon_cpu.py), with the window call (stride 1, and a dense window decimated), the oracle, the strided sampler
and ltp_state_at_batch; the hold and NaN rules, `valid`, float32, other batch kinds, refusals, the host and drop-in paths and graph
capture. The batches, their sizes and the planner helpers are tests/horizon_helpers.py's."""
import ctypes as C

import numpy as np
import pytest

import horizon_checker as hc
import horizon_helpers as H
from horizon_helpers import DEV, INVALID

pytestmark = pytest.mark.gpu

PAIRS = [(1, 7), (32, 2), (32, 10), (33, 3), (64, 5), (100, 4), (16, 50), (64, 64)]


def _assert_horizon(ltp, batch, full, k_host, N, s, first, count, what, dtype=None):
    """One horizon call over plans [first, first + count) with starts k_host[first:first + count], compared with the full rows. The
    buffer is pre-filled with a pattern: elements [N, R) of a row must keep it. `valid` is also held against the closed form."""
    return H.assert_rows(lambda k, out: ltp.sampleHorizon(batch, first, count, k, N, s, out=out), ltp, batch, full, k_host, hc.stride_grid(N, s),
                         first, count, what, dtype, stride=s)


@pytest.mark.parametrize("name,n,pow_rule", [("panda", 3000, "libm"), ("panda", 3000, "exact"), ("ref", 2000, "libm"), ("ref", 2000, "exact"),
                                             ("ref30", 300, "libm"), ("ref30", 300, "exact")])
def test_bits_against_full_rows(name, n, pow_rule):
    """Every real element of every horizon has the bits of the row sampleBatch wrote at k + w * s, every element past the end follows
    the hold rule, `valid` follows its formula — no plan excepted; at first = 0, count = n and at a sub-range whose count * dof is
    no multiple of 64. The coverage conditions are asserted first."""
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch(name, n, pow_rule)
    rng = np.random.default_rng(99)
    for N, s in PAIRS:
        k = hc.draw_starts(rng, lens, t_scaled, N, s)
        hc.assert_coverage(k, N, s, lens, t_scaled, f"{name} {pow_rule} N={N} s={s}")
        _assert_horizon(ltp, batch, full, k, N, s, 0, n, f"{name} {pow_rule} N={N} s={s} whole batch")
        first, count = H.odd_range(n, dof)
        assert (count * dof) % 64 != 0
        _assert_horizon(ltp, batch, full, k, N, s, first, count, f"{name} {pow_rule} N={N} s={s} plans [{first}, {first + count})")


@pytest.mark.parametrize("N", [32, 33, 100])
def test_stride_one_is_the_window_call(N):
    """sampleHorizon(s = 1) and sampleWindow give identical buffers, padding included, and identical `valid`."""
    import torch
    n = 3000
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    k = torch.from_numpy(hc.draw_starts(np.random.default_rng(12), lens, t_scaled, N, 1)).to(DEV)
    R = ltp.windowRowStride(N)
    a, va = ltp.sampleWindow(batch, 0, n, k, N, out=torch.full((n, 4, dof, R), 7.25, dtype=torch.float64, device=DEV))
    b, vb = ltp.sampleHorizon(batch, 0, n, k, N, 1, out=torch.full((n, 4, dof, R), 7.25, dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(hc.int_view(a), hc.int_view(b)) and torch.equal(va, vb)
    assert int((va > 0).sum().item()) > 0.5 * n


@pytest.mark.parametrize("N,s", [(32, 10), (33, 3)])
def test_decimated_dense_window(N, s):
    """horizon(k, N, s)[..., w] == window(k, N * s)[..., w * s] for every element, hold and NaN elements included."""
    import torch
    n = 3000
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    k = torch.from_numpy(hc.draw_starts(np.random.default_rng(13), lens, t_scaled, N, s)).to(DEV)
    dense, _ = ltp.sampleWindow(batch, 0, n, k, N * s)
    hor, _ = ltp.sampleHorizon(batch, 0, n, k, N, s)
    torch.cuda.synchronize()
    assert torch.equal(hc.int_view(hor)[..., :N], hc.int_view(dense)[..., :N * s:s].contiguous())


def test_wide_spans():
    """Spans that hold whole trajectories: more runs with a grid sample than a lane parks in one pass."""
    n = 500
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    k = np.zeros(n, dtype=np.int32)
    k[1::4] = 17
    k[2::4] = (lens[2::4] // 2).astype(np.int32)
    for N, s in ((2048, 2), (1366, 3), (256, 16)):
        assert np.mean((lens > 0) & (lens <= (N - 1) * s)) > 0.5      # wholly inside the span, from any k >= 0
        _assert_horizon(ltp, batch, full, k, N, s, 0, n, f"wide N={N} s={s} k mixed")
        _assert_horizon(ltp, batch, full, k, N, s, 3, n - 10, f"wide N={N} s={s} sub-range")


@pytest.mark.parametrize("N,s", [(32, 10), (100, 4)])
def test_float32_horizons(N, s):
    """float32 horizons are the float64 horizons rounded once, and equal the float32 sampler's rows where the sample is real."""
    import torch
    n = 2000
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    k = hc.draw_starts(np.random.default_rng(5), lens, t_scaled, N, s)
    r64, v64 = _assert_horizon(ltp, batch, full, k, N, s, 0, n, f"f64 N={N} s={s}")
    full32 = H.full_rows(ltp, batch, torch.float32)
    r32, v32 = _assert_horizon(ltp, batch, full32, k, N, s, 0, n, f"f32 N={N} s={s}", dtype=torch.float32)
    assert torch.equal(v32, v64)
    planned = batch.traj_len > 0
    a, b = r32[planned][..., :N], r64[planned][..., :N].to(torch.float32)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "float32 horizon is not (float) of the float64 horizon"


def test_horizons_against_the_oracle(oracle_mod):
    """q, v, a and j of the real elements against the CPU oracle's own trajectories at k + w * s, 1e-9 (the project's parity bar)."""
    import torch
    n, N, s = 200, 32, 10
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    orc = oracle_mod.Oracle(dof, H.TS, **lim)
    o = orc.plan_batch(*qs, sample=True)
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    lens = batch.traj_len.cpu().numpy()
    assert np.array_equal(lens, o["traj_len"])
    k = hc.draw_starts(np.random.default_rng(3), lens, batch.t_scaled.cpu().numpy(), N, s)
    rows, valid = ltp.sampleHorizon(batch, 0, n, torch.from_numpy(k).to(DEV), N, s)
    rows, valid = rows.cpu().numpy()[..., :N], valid.cpu().numpy()
    worst, checked, n_real, n_all = 0.0, 0, 0, 0
    for p in range(n):
        if o["status"][p] == 0:
            continue
        L, q, v, a, j = orc.get_trajectory(o["t_scaled"][p], o["dir"][p], o["mod"][p], qs[1][p], qs[2][p], qs[3][p], o["v_drive"][p])
        t = max(int(k[p]), 0) + s * np.arange(N)
        real = t < L
        assert valid[p] == real.sum()
        for arr, ref in enumerate((q, v, a, j)):
            if real.any():
                worst = max(worst, float(np.max(np.abs(rows[p, arr][:, real] - ref[:, t[real]]))))
        n_real += int(real.sum())
        n_all += N
        checked += 1
    print(f"oracle: {checked} plans, {n_real} of {n_all} elements real, worst {worst:.3e}")
    assert checked > 0.95 * n and 2 * n_real >= n_all and worst <= 1e-9, (checked, n_real, n_all, worst)


def test_strided_sampler_at_k_zero():
    """A second handle with setSampleStride(4) and setMaxSamples(64) stores samples 0, 4, 8, ...: they equal horizon(k = 0, N = 64,
    s = 4) of the first handle's batch in every real element."""
    import torch
    import longtermplanner_amd as amd
    n, N, s = 300, 64, 4
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    hor, valid = ltp.sampleHorizon(batch, 0, n, 0, N, s)
    hor, valid = hor.cpu().numpy(), valid.cpu().numpy()
    p2, _, _ = H.planner("panda")
    p2.setSampleStride(s)
    p2.setMaxSamples(N)
    b2 = p2.planSwitchTimesBatch(*H.tensors(qs))
    torch.cuda.synchronize()
    off = b2.offsets.cpu().numpy().view(np.uint64)
    dec = torch.zeros(max(int(off[-1]), 2), dtype=torch.float64, device=DEV)
    p2.sampleBatch(b2, 0, n, dec)
    torch.cuda.synchronize()
    hd = dec.cpu().numpy()
    assert np.array_equal(b2.traj_len.cpu().numpy(), lens)
    compared = 0
    for p in range(n):
        if lens[p] <= 0:
            continue
        stored = p2.storedSamples(int(lens[p]))
        assert stored == valid[p] == min(N, -(-int(lens[p]) // s))
        got = amd.unpack_trajectory(hd, int(off[p]), dof, stored)
        for arr in range(4):
            assert np.array_equal(np.ascontiguousarray(got[arr]).view(np.uint64), np.ascontiguousarray(hor[p, arr, :, :stored]).view(np.uint64)), (p, arr)
        compared += stored
    assert compared > 0.5 * n * N


@pytest.mark.parametrize("kind", ["retimed", "limit_sets", "matlab"])
def test_other_batch_kinds(kind):
    """A retimed batch, a batch with three bound limit sets, MATLAB semantics (full rows from the walk sampler): the bit comparison
    of test_bits_against_full_rows, n = 1000, at (32, 10) and (33, 3)."""
    n = 1000
    ltp, dof, batch, full, lens, t_scaled = H.other_batch(kind, n)
    rng = np.random.default_rng(21)
    for N, s in ((32, 10), (33, 3)):
        k = hc.draw_starts(rng, lens, t_scaled, N, s)
        print(kind, N, s, "on-grid / skipped / ends / starts:", hc.coverage(k, N, s, lens, t_scaled))
        _assert_horizon(ltp, batch, full, k, N, s, 0, n, f"{kind} N={N} s={s}")
        first, count = H.odd_range(n, dof)
        _assert_horizon(ltp, batch, full, k, N, s, first, count, f"{kind} N={N} s={s} sub-range")


def test_failed_plans_are_nan_and_neighbours_unaffected():
    """Every fifth query violates checkInputs: its horizons are NaN in all four arrays, valid is 0; every other plan has the bits it
    has in a batch without the failures."""
    import torch
    n, N, s = 1000, 32, 10
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    k = hc.draw_starts(np.random.default_rng(8), lens, t_scaled, N, s)
    good, _ = _assert_horizon(ltp, batch, full, k, N, s, 0, n, "intact batch")
    bad_qs = [x.copy() for x in qs]
    bad_qs[1][::5, 2] = 50.0
    ltp2, _, _ = H.planner("panda")
    b2 = ltp2.planSwitchTimesBatch(*H.tensors(bad_qs))
    rows, valid = ltp2.sampleHorizon(b2, 0, n, torch.from_numpy(k).to(DEV), N, s)
    torch.cuda.synchronize()
    st, tl = b2.status.cpu().numpy(), b2.traj_len.cpu().numpy()
    assert np.all(st[::5] & 1) and np.all(tl[::5] == 0)
    assert bool(torch.isnan(rows[::5][..., :N]).all().item()) and int(valid[::5].abs().sum().item()) == 0
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[::5] = False
    assert torch.equal(rows[keep][..., :N].view(torch.int64), good[keep][..., :N].view(torch.int64))


def test_per_plan_starts_equal_uniform_starts_and_state_at():
    import torch
    n, N, s = 1000, 32, 10
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    for k0 in (0, np.int32(37), np.int64(600)):
        uni, vu = ltp.sampleHorizon(batch, 0, n, k0, N, s)
        k0 = int(k0)
        per, vp = ltp.sampleHorizon(batch, 0, n, torch.full((n,), k0, dtype=torch.int32, device=DEV), N, s)
        torch.cuda.synchronize()
        planned = batch.traj_len > 0
        assert torch.equal(uni[planned][..., :N].view(torch.int64), per[planned][..., :N].view(torch.int64)) and torch.equal(vu, vp)
        q, v, a = ltp.stateAt(batch, 0, n, k0)
        real = batch.traj_len > k0               # stateAt clamps to the last sample; the horizon holds q and rests
        for arr, ref in enumerate((q, v, a)):
            assert torch.equal(uni[real][:, arr, :, 0].contiguous().view(torch.int64), ref[real].contiguous().view(torch.int64)), (k0, arr)
    assert int((batch.traj_len > 0).sum().item()) > 0.5 * n and int((batch.traj_len > 37).sum().item()) > 0.5 * n


def test_refusals():
    """Each refusal is LTP_ERR_INVALID_ARGUMENT and its text names the reason; nothing is written."""
    import torch
    from longtermplanner_amd import _abi
    n, N, s = 64, 32, 10
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    O = _abi.HorizonOpts
    out = torch.full((n, 4, dof, ltp.windowRowStride(N)), H.PATTERN, dtype=torch.float64, device=DEV)
    call = H.reader_call(ltp._lib.ltp_sample_horizon_batch, ltp, batch, n, out)
    good = dict(size=C.sizeof(O), format=0, n_samples=N, stride=s)
    H.common_refusals(ltp, batch, n, dof, call, O, good, out, out.numel() - 1, "ltp_window_elements")
    for bad, text in ((dict(stride=0), "stride"), (dict(stride=-1), "stride"), (dict(stride=(1 << 30) // N + 1), "span"),
                      (dict(n_samples=1 << 16, stride=(1 << 14) + 1), "span"), (dict(n_samples=0), "n_samples"), (dict(n_samples=-1), "n_samples"),
                      (dict(format=2), "format")):
        rc, msg = call(O(**dict(good, **bad)))
        assert rc == INVALID and text in msg, (bad, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == H.PATTERN).all().item()), "a refused call wrote to the buffer"
    # the largest admitted span: n_samples * stride == 2^30 exactly is a call like any other
    rc, msg = call(O(**dict(good, stride=(1 << 30) // N)))
    assert rc == 0, msg
    assert call(O(**good))[0] == 0


DROPIN = r'''
#include "long_term_planner/long_term_planner.h"
#include <cstdio>
using namespace long_term_planner;
int main(int argc, char** argv) {
  const int dof = 7, n = 40, N = 48, stride = 6;
  std::vector<double> q_min = {-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973};
  std::vector<double> q_max = {2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973};
  std::vector<double> v_max = {2.175, 2.175, 2.175, 2.175, 2.61, 2.61, 2.61};
  std::vector<double> a_max = {15.0, 7.5, 10.0, 12.5, 15.0, 20.0, 20.0};
  std::vector<double> j_max = {7500.0, 3750.0, 5000.0, 6250.0, 7500.0, 10000.0, 10000.0};
  LongTermPlanner ltp(dof, 0.001, q_min, q_max, v_max, a_max, j_max);
  std::vector<double> in(4 * n * dof);
  std::vector<int> k(n);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size() || std::fread(k.data(), sizeof(int), k.size(), f) != k.size()) return 2;
  std::fclose(f);
  std::vector<double> rows;
  std::vector<int> valid;
  BatchTrajectory b;
  const long long ok = ltp.planHorizonBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, N, stride, rows, &valid, &b);
  FILE* o = std::fopen(argv[2], "wb");
  std::fwrite(rows.data(), sizeof(double), rows.size(), o);
  std::fwrite(valid.data(), sizeof(int), valid.size(), o);
  std::fwrite(b.status.data(), sizeof(int), b.status.size(), o);
  std::fclose(o);
  std::printf("%lld ok, %zu doubles\n", ok, rows.size());
  return 0;
}
'''


def test_host_and_dropin_paths(tmp_path):
    """planHorizonHost equals the device path bitwise and its status carries END_LIMIT like planBatchHost(sample=False); a small C++
    program gives the same bytes through LongTermPlanner::planHorizonBatch."""
    import torch
    n, N, s = 40, 48, 6
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    qs[0][3, 1] = 2.5                               # a goal beyond joint 1's range: planned, then END_LIMIT
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    lens = batch.traj_len.cpu().numpy()
    k = hc.draw_starts(np.random.default_rng(1), lens, batch.t_scaled.cpu().numpy(), N, s)
    R = ltp.windowRowStride(N)
    dev_rows, dev_valid = ltp.sampleHorizon(batch, 0, n, torch.from_numpy(k).to(DEV), N, s, out=torch.zeros((n, 4, dof, R), dtype=torch.float64, device=DEV))
    dev_rows, dev_valid = dev_rows.cpu().numpy(), dev_valid.cpu().numpy()
    assert 0 < int((dev_valid > 0).sum()) and int((dev_valid < N).sum()) > 0
    rec, rows, valid = ltp.planHorizonHost(*qs, k, N, s)
    assert np.array_equal(rows.view(np.uint8), dev_rows.view(np.uint8)) and np.array_equal(valid, dev_valid)
    plain = ltp.planBatchHost(*qs, sample=False)
    assert np.array_equal(rec["status"], plain["status"]) and (rec["status"][3] & 8) and np.array_equal(rec["traj_len"], lens)
    _, rows_u, valid_u = ltp.planHorizonHost(*qs, 5, N, s)
    du, dv = ltp.sampleHorizon(batch, 0, n, 5, N, s, out=torch.zeros((n, 4, dof, R), dtype=torch.float64, device=DEV))
    assert np.array_equal(rows_u.view(np.uint8), du.cpu().numpy().view(np.uint8)) and np.array_equal(valid_u, dv.cpu().numpy())

    raw = H.run_dropin(tmp_path, "horizon", DROPIN, np.concatenate([x.reshape(-1) for x in qs]).astype(np.float64).tobytes() + k.astype(np.int32).tobytes())
    H.assert_dropin_bytes(raw, rows, valid, rec["status"])


def test_graph_capture_and_replay_with_new_starts():
    """The call allocates nothing: captured on one stream (one kernel node) and replayed once after first_sample was rewritten in
    place, it gives the horizons of the new starts."""
    import torch
    n, N, s = 1000, 32, 10
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    rng = np.random.default_rng(77)
    ka, kb = hc.draw_starts(rng, lens, t_scaled, N, s), hc.draw_starts(rng, lens, t_scaled, N, s)
    assert np.count_nonzero(ka != kb) > 0.5 * n
    R = ltp.windowRowStride(N)
    k = torch.from_numpy(ka).to(DEV)
    out = torch.zeros((n, 4, dof, R), dtype=torch.float64, device=DEV)
    valid = torch.zeros((n,), dtype=torch.int32, device=DEV)
    g = H.capture(lambda: ltp.sampleHorizon(batch, 0, n, k, N, s, out=out, valid=valid))
    H.replay(g, [(k, kb)], out, valid)
    exp, exp_valid, planned = hc.expected(full, batch.offsets, batch.traj_len, k, hc.stride_grid(N, s), dof, 0, n)
    assert torch.equal(out.view(torch.int64)[..., :N][planned], exp[planned]) and torch.equal(valid, exp_valid)
    assert bool(torch.isnan(out[~planned][..., :N]).all().item())
