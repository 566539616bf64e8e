"""Horizon windows (ltp_sample_window_batch, include/ltp_hip.h) on the GPU: the samples [k, k + N) of planned batches against the
rows the existing full-row sampler wrote for the same batch (itself pinned to the CPU oracle), the hold and NaN rules, `valid`,
float32, the oracle directly, retimed / limit-set / MATLAB batches, refusals, the host and drop-in paths and graph capture."""
import ctypes as C

import numpy as np
import pytest

import horizon_checker as hc
import horizon_helpers as H
from horizon_helpers import DEV, INVALID, TS

pytestmark = pytest.mark.gpu


def _assert_window(ltp, batch, full, k_host, N, first, count, what, dtype=None):
    """One window call over plans [first, first + count) with starts k_host[first:first + count], compared with the full rows. The
    buffer is pre-filled with a pattern: elements [N, R) of a row must keep it. `valid` is also held against the closed form."""
    return H.assert_rows(lambda k, out: ltp.sampleWindow(batch, first, count, k, N, out=out), ltp, batch, full, k_host, hc.window_grid(N),
                         first, count, what, dtype, stride=1)


@pytest.mark.parametrize("N", [1, 31, 32, 33, 64, 100])
def test_window_elements(N):
    ltp, dof, _ = H.planner("panda")
    for count in (1, 3, 1000):
        assert ltp._lib.ltp_window_elements(ltp._h, count, N) == count * 4 * dof * ltp._lib.ltp_row_stride(N)


@pytest.mark.parametrize("name,n,pow_rule", [("panda", 3000, "libm"), ("panda", 3000, "exact"), ("ref", 2000, "libm"), ("ref", 2000, "exact"),
                                             ("ref30", 300, "libm"), ("ref30", 300, "exact")])
def test_bits_against_full_rows(name, n, pow_rule):
    """Every real sample of every window has the bits of the row sampleBatch wrote, every sample past the end follows the hold rule,
    `valid` follows its formula — no plan excepted; at first = 0, count = n and at a sub-range whose count * dof is no multiple of 64."""
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch(name, n, pow_rule)
    rng = np.random.default_rng(99)
    for N in (1, 32, 33, 64, 100, 256):
        k = hc.draw_starts(rng, lens, t_scaled, N, 1)
        hc.assert_coverage(k, N, 1, lens, t_scaled, f"{name} {pow_rule} N={N}")
        _assert_window(ltp, batch, full, k, N, 0, n, f"{name} {pow_rule} N={N} whole batch")
        first, count = H.odd_range(n, dof)
        assert (count * dof) % 64 != 0
        _assert_window(ltp, batch, full, k, N, first, count, f"{name} {pow_rule} N={N} plans [{first}, {first + count})")


def test_wide_windows():
    """N = 4096: most plans lie wholly inside the window, so every one of their runs does — more runs than a lane parks in one pass."""
    n, N = 500, 4096
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    assert np.mean((lens > 0) & (lens <= N)) > 0.5
    k = np.zeros(n, dtype=np.int32)
    k[1::4] = 17
    k[2::4] = (lens[2::4] // 2).astype(np.int32)
    _assert_window(ltp, batch, full, k, N, 0, n, "wide k mixed")
    _assert_window(ltp, batch, full, k, N, 3, n - 10, "wide sub-range")


@pytest.mark.parametrize("N", [32, 100])
def test_float32_windows(N):
    """float32 windows are the float64 windows rounded once, and equal the float32 sampler's rows where the sample is real."""
    import torch
    n = 2000
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    k = hc.draw_starts(np.random.default_rng(5), lens, t_scaled, N, 1)
    r64, v64 = _assert_window(ltp, batch, full, k, N, 0, n, f"f64 N={N}")
    full32 = H.full_rows(ltp, batch, torch.float32)
    r32, v32 = _assert_window(ltp, batch, full32, k, N, 0, n, f"f32 N={N}", dtype=torch.float32)
    assert torch.equal(v32, v64)
    planned = batch.traj_len > 0
    a, b = r32[planned][..., :N], r64[planned][..., :N].to(torch.float32)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "float32 window is not (float) of the float64 window"


def test_windows_against_the_oracle(oracle_mod):
    """q, v, a and j of the windows against the CPU oracle's own trajectories, 1e-9 (the bar of tests/test_gpu_parity.py)."""
    import torch
    n, N = 200, 100
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    orc = oracle_mod.Oracle(dof, TS, **lim)
    o = orc.plan_batch(*qs, sample=True)
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    lens = batch.traj_len.cpu().numpy()
    assert np.array_equal(lens, o["traj_len"])
    k = hc.draw_starts(np.random.default_rng(3), lens, batch.t_scaled.cpu().numpy(), N, 1)
    rows, valid = ltp.sampleWindow(batch, 0, n, torch.from_numpy(k).to(DEV), N)
    rows, valid = rows.cpu().numpy()[..., :N], valid.cpu().numpy()
    worst, checked = 0.0, 0
    for p in range(n):
        if o["status"][p] == 0:
            continue
        L, q, v, a, j = orc.get_trajectory(o["t_scaled"][p], o["dir"][p], o["mod"][p], qs[1][p], qs[2][p], qs[3][p], o["v_drive"][p])
        t = max(int(k[p]), 0) + np.arange(N)
        real = t < L
        assert valid[p] == real.sum()
        tc = np.minimum(t, L - 1)
        for arr, ref in enumerate((q, v, a, j)):
            want = ref[:, tc] if arr == 0 else np.where(real[None, :], ref[:, tc], 0.0)
            worst = max(worst, float(np.max(np.abs(rows[p, arr] - want))))
        checked += 1
    assert checked > 0.95 * n and worst <= 1e-9, (checked, worst)


def test_failed_plans_are_nan_and_neighbours_unaffected():
    """Every fifth query violates checkInputs (q_0 outside its range): its windows are NaN in all four arrays, valid is 0; every other
    plan has the bits it has in a batch without the failures."""
    import torch
    n, N = 1000, 64
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    k = hc.draw_starts(np.random.default_rng(8), lens, t_scaled, N, 1)
    good, _ = _assert_window(ltp, batch, full, k, N, 0, n, "intact batch")
    bad_qs = [x.copy() for x in qs]
    bad_qs[1][::5, 2] = 50.0
    ltp2, _, _ = H.planner("panda")
    b2 = ltp2.planSwitchTimesBatch(*H.tensors(bad_qs))
    kt = torch.from_numpy(k).to(DEV)
    rows, valid = ltp2.sampleWindow(b2, 0, n, kt, N)
    torch.cuda.synchronize()
    st, tl = b2.status.cpu().numpy(), b2.traj_len.cpu().numpy()
    assert np.all(st[::5] & 1) and np.all(tl[::5] == 0)
    assert bool(torch.isnan(rows[::5][..., :N]).all().item()) and int(valid[::5].abs().sum().item()) == 0
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[::5] = False
    assert torch.equal(rows[keep][..., :N].view(torch.int64), good[keep][..., :N].view(torch.int64))


@pytest.mark.parametrize("kind", ["retimed", "limit_sets", "matlab"])
def test_other_batch_kinds(kind):
    """A retimed batch, a batch with three bound limit sets, MATLAB semantics (full rows from the walk sampler): the bit comparison of
    test_bits_against_full_rows, n = 1000, N = 64."""
    n, N = 1000, 64
    ltp, dof, batch, full, lens, t_scaled = H.other_batch(kind, n)
    k = hc.draw_starts(np.random.default_rng(21), lens, t_scaled, N, 1)
    print(kind, "switch inside / skipped / ends past / starts past:", hc.coverage(k, N, 1, lens, t_scaled))
    _assert_window(ltp, batch, full, k, N, 0, n, kind)
    first, count = H.odd_range(n, dof)
    _assert_window(ltp, batch, full, k, N, first, count, kind + " sub-range")


def test_per_plan_starts_equal_uniform_starts_and_state_at():
    import torch
    n, N = 1000, 64
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    for k0 in (0, np.int32(37), np.int64(600)):             # numpy integers are plain starts too
        uni, vu = ltp.sampleWindow(batch, 0, n, k0, N)
        k0 = int(k0)
        per, vp = ltp.sampleWindow(batch, 0, n, torch.full((n,), k0, dtype=torch.int32, device=DEV), N)
        torch.cuda.synchronize()
        planned = batch.traj_len > 0
        assert torch.equal(uni[planned][..., :N].view(torch.int64), per[planned][..., :N].view(torch.int64)) and torch.equal(vu, vp)
        for s in (0, N - 1):
            q, v, a = ltp.stateAt(batch, 0, n, k0 + s)
            # stateAt clamps to the last sample (v, a of that sample); the window holds q and rests: compare where k0 + s is a sample
            real = (batch.traj_len > k0 + s)
            for arr, ref in enumerate((q, v, a)):
                assert torch.equal(uni[real][:, arr, :, s].contiguous().view(torch.int64), ref[real].contiguous().view(torch.int64)), (k0, s, arr)
            assert int(real.sum().item()) > 0.5 * n


def test_refusals():
    """Each refusal is LTP_ERR_INVALID_ARGUMENT and its text names the reason; nothing is written."""
    import torch
    from longtermplanner_amd import _abi
    n, N = 64, 32
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    O = _abi.WindowOpts
    out = torch.full((n, 4, dof, ltp.windowRowStride(N)), H.PATTERN, dtype=torch.float64, device=DEV)
    call = H.reader_call(ltp._lib.ltp_sample_window_batch, ltp, batch, n, out)
    good = dict(size=C.sizeof(O), format=0, n_samples=N)
    H.common_refusals(ltp, batch, n, dof, call, O, good, out, out.numel() - 1, "ltp_window_elements")
    for bad, text in ((dict(n_samples=0), "n_samples"), (dict(n_samples=-1), "n_samples"), (dict(format=2), "format")):
        rc, msg = call(O(**dict(good, **bad)))
        assert rc == INVALID and text in msg, (bad, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == H.PATTERN).all().item()), "a refused call wrote to the buffer"
    assert call(O(**good))[0] == 0


DROPIN = r'''
#include "long_term_planner/long_term_planner.h"
#include <cstdio>
using namespace long_term_planner;
int main(int argc, char** argv) {
  const int dof = 7, n = 40, N = 48;
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
  const long long ok = ltp.planWindowBatch(n, in.data(), in.data() + n * dof, in.data() + 2 * n * dof, in.data() + 3 * n * dof, k.data(), 0, N, rows, &valid, &b);
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
    """planWindowHost equals the device path bitwise and its status carries END_LIMIT like planBatchHost(sample=False); a small C++
    program gives the same bytes through LongTermPlanner::planWindowBatch."""
    import torch
    n, N = 40, 48
    ltp, dof, lim = H.planner("panda")
    qs = H.queries(lim, n)
    qs[0][3, 1] = 2.5                               # a goal beyond joint 1's range: planned, then END_LIMIT
    batch = ltp.planSwitchTimesBatch(*H.tensors(qs))
    lens = batch.traj_len.cpu().numpy()
    k = hc.draw_starts(np.random.default_rng(1), lens, batch.t_scaled.cpu().numpy(), N, 1)
    R = ltp.windowRowStride(N)
    dev_rows, dev_valid = ltp.sampleWindow(batch, 0, n, torch.from_numpy(k).to(DEV), N, out=torch.zeros((n, 4, dof, R), dtype=torch.float64, device=DEV))
    dev_rows, dev_valid = dev_rows.cpu().numpy(), dev_valid.cpu().numpy()
    rec, rows, valid = ltp.planWindowHost(*qs, k, N)
    assert np.array_equal(rows.view(np.uint8), dev_rows.view(np.uint8)) and np.array_equal(valid, dev_valid)
    plain = ltp.planBatchHost(*qs, sample=False)
    assert np.array_equal(rec["status"], plain["status"]) and (rec["status"][3] & 8) and np.array_equal(rec["traj_len"], lens)
    _, rows_u, valid_u = ltp.planWindowHost(*qs, 5, N)
    du, dv = ltp.sampleWindow(batch, 0, n, 5, N, out=torch.zeros((n, 4, dof, R), dtype=torch.float64, device=DEV))
    assert np.array_equal(rows_u.view(np.uint8), du.cpu().numpy().view(np.uint8)) and np.array_equal(valid_u, dv.cpu().numpy())

    raw = H.run_dropin(tmp_path, "window", DROPIN, np.concatenate([x.reshape(-1) for x in qs]).astype(np.float64).tobytes() + k.astype(np.int32).tobytes())
    H.assert_dropin_bytes(raw, rows, valid, rec["status"])


def test_graph_capture_and_replay_with_new_starts():
    """The call allocates nothing: captured on one stream and replayed once after first_sample was rewritten in place, it gives the
    windows of the new starts."""
    import torch
    n, N = 1000, 64
    ltp, dof, lim, qs, batch, full, lens, t_scaled = H.batch("panda", n)
    rng = np.random.default_rng(77)
    ka, kb = hc.draw_starts(rng, lens, t_scaled, N, 1), hc.draw_starts(rng, lens, t_scaled, N, 1)
    assert np.count_nonzero(ka != kb) > 0.5 * n
    R = ltp.windowRowStride(N)
    k = torch.from_numpy(ka).to(DEV)
    out = torch.zeros((n, 4, dof, R), dtype=torch.float64, device=DEV)
    valid = torch.zeros((n,), dtype=torch.int32, device=DEV)
    g = H.capture(lambda: ltp.sampleWindow(batch, 0, n, k, N, out=out, valid=valid))
    H.replay(g, [(k, kb)], out, valid)
    exp, exp_valid, planned = hc.expected(full, batch.offsets, batch.traj_len, k, hc.window_grid(N), dof, 0, n)
    assert torch.equal(out.view(torch.int64)[..., :N][planned], exp[planned]) and torch.equal(valid, exp_valid)
    assert bool(torch.isnan(out[~planned][..., :N]).all().item())
