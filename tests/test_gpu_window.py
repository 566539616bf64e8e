"""Horizon windows (ltp_sample_window_batch, include/ltp_hip.h) on the GPU: the samples [k, k + N) of planned batches against the
rows the existing full-row sampler wrote for the same batch (itself pinned to the CPU oracle), the hold and NaN rules, `valid`,
float32, the oracle directly, retimed / limit-set / MATLAB batches, refusals, the host and drop-in paths and graph capture."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = 0.001
DEV = "cuda:0"
SEED = 4242
INVALID = 1


def _planner(name, pow_rule="libm", semantics="cpp"):
    from longtermplanner_amd import LongTermPlanner, limit_set
    dof, lim = limit_set(name)
    ltp = LongTermPlanner(dof, TS, device=0, **lim)
    ltp.setPowRule(pow_rule)
    ltp.setSemantics(semantics)
    return ltp, dof, lim


def _queries(lim, n, seed=SEED):
    from longtermplanner_amd import generate_queries
    return [np.ascontiguousarray(x) for x in generate_queries(n, lim, seed=seed)]


def _tensors(qs):
    import torch
    return [torch.from_numpy(x).to(DEV) for x in qs]


def _full_rows(ltp, batch, dtype=None):
    """Whole rows of every plan of the batch through the existing sampler (sampleBatch): the yardstick."""
    import torch
    n = batch.n
    total = int(batch.offsets[n].item())
    full = torch.zeros(max(total, 2), dtype=dtype or torch.float64, device=DEV)
    ltp.sampleBatch(batch, 0, n, full)
    torch.cuda.synchronize()
    return full


def _switch_indices(t_scaled):
    """Sampled switch indices of every (plan, joint, phase): floor for even phases, ceil for odd ones (cc:751-757)."""
    x = np.nan_to_num(t_scaled / TS, nan=0.0, posinf=0.0, neginf=0.0)
    sw = np.where(np.arange(7) % 2 == 0, np.floor(x), np.ceil(x))
    return np.clip(sw, -1, 2 ** 30).astype(np.int64)


def _draw_starts(rng, lens, t_scaled, N):
    """k per plan by plan index mod 6 — 0, 1: uniform in [0, traj_len); 2, 3: a switch index of a random (joint, phase) minus a
    uniform draw from [0, N); 4: uniform in [traj_len - N, traj_len + N); 5: cycling through {0, traj_len - 1, traj_len, traj_len + 5, -3}."""
    n, dof = t_scaled.shape[:2]
    L = lens.astype(np.int64)
    sw = _switch_indices(t_scaled)
    kind = np.arange(n) % 6
    uni = rng.integers(0, np.maximum(L, 1))
    tgt = sw[np.arange(n), rng.integers(0, dof, n), rng.integers(0, 7, n)] - rng.integers(0, N, n)
    end = L - N + rng.integers(0, 2 * N, n)
    cyc = np.stack([np.zeros(n, dtype=np.int64), L - 1, L, L + 5, np.full(n, -3)], axis=1)[np.arange(n), (np.arange(n) // 6) % 5]
    k = np.select([kind <= 1, kind <= 3, kind == 4], [uni, tgt, end], cyc)
    return k.astype(np.int32)


def _coverage(k, N, lens, t_scaled):
    """Shares of the batch: plans with a switch index inside the window, windows that end past traj_len, windows that start at or
    past it, plans with a trajectory."""
    L = lens.astype(np.int64)
    kk = np.maximum(k.astype(np.int64), 0)
    sw = _switch_indices(t_scaled)
    inside = (sw >= kk[:, None, None]) & (sw < (kk + N)[:, None, None]) & (sw < L[:, None, None])
    has = L > 0
    return (np.mean(inside.any(axis=(1, 2)) & has), np.mean(has & (kk + N > L)), np.mean(has & (kk >= L)), np.mean(has))


def _assert_coverage(k, N, lens, t_scaled, what):
    sw, ends, starts, planned = _coverage(k, N, lens, t_scaled)
    print(f"{what}: switch inside {sw:.3f}, ends past {ends:.3f}, starts past {starts:.3f}, planned {planned:.3f}")
    assert sw >= 0.30 and ends >= 0.10 and starts >= 0.03 and planned >= 0.95, (what, sw, ends, starts, planned)


def _int_view(t):
    import torch
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def _expected(full, offsets, lens, k, N, dof, first, count):
    """What the window of plans [first, first + count) must hold, from the full rows (on the device, as integers): element s of a
    row is the full row's element k + s while that is a sample of the trajectory; past the end q is the last sample's and v, a, j
    are +0.0. Returns (bits [count, 4, dof, N], valid [count], planned [count])."""
    import torch
    L = lens[first:first + count].long()
    o = offsets[first:first + count].long()
    kk = k.long().clamp(min=0)
    t = kk[:, None] + torch.arange(N, device=DEV)[None, :]
    real = t < L[:, None]
    tc = torch.minimum(t, (L - 1).clamp(min=0)[:, None])
    stride = (L + 31) // 32 * 32
    rowi = torch.arange(4 * dof, device=DEV).view(1, 4, dof, 1)
    idx = o.view(-1, 1, 1, 1) + rowi * stride.view(-1, 1, 1, 1) + tc[:, None, None, :]
    planned = L > 0
    idx = torch.where(planned.view(-1, 1, 1, 1), idx, torch.zeros_like(idx))
    exp = _int_view(full)[idx]
    exp[:, 1:] = torch.where(real[:, None, None, :], exp[:, 1:], torch.zeros_like(exp[:, 1:]))
    valid = torch.where(planned, (L - kk).clamp(min=0, max=N), torch.zeros_like(L)).int()
    return exp, valid, planned


def _assert_window(ltp, batch, full, k_host, N, first, count, what, dtype=None):
    """One window call over plans [first, first + count) with starts k_host[first:first + count], compared with the full rows. The
    buffer is pre-filled with a pattern: elements [N, R) of a row must keep it."""
    import torch
    dof = batch.dof
    R = ltp.windowRowStride(N)
    k = torch.from_numpy(np.ascontiguousarray(k_host[first:first + count])).to(DEV)
    out = torch.full((count, 4, dof, R), 7.25, dtype=dtype or torch.float64, device=DEV)
    rows, valid = ltp.sampleWindow(batch, first, count, k, N, out=out)
    torch.cuda.synchronize()
    exp, exp_valid, planned = _expected(full, batch.offsets, batch.traj_len, k, N, dof, first, count)
    got = _int_view(rows)[..., :N]
    bad = (got != exp).flatten(1).any(dim=1) & planned
    assert int(bad.sum().item()) == 0, f"{what}: {int(bad.sum().item())} plans differ from the full rows, first local plan {int(bad.nonzero()[0].item())}"
    assert bool(torch.isnan(rows[~planned][..., :N]).all().item()), f"{what}: a plan without a trajectory is not NaN"
    assert torch.equal(valid, exp_valid), f"{what}: valid differs"
    if R > N:
        assert bool((rows[..., N:] == 7.25).all().item()), f"{what}: elements [N, R) of a row were written"
    return rows, valid


_CACHE = {}


def _batch(name, n, pow_rule="libm", semantics="cpp"):
    """Planned batch + its full float64 rows + host copies of traj_len and t_scaled; the latest one is kept."""
    key = (name, n, pow_rule, semantics)
    if _CACHE.get("key") != key:
        _CACHE.clear()
        ltp, dof, lim = _planner(name, pow_rule, semantics)
        qs = _queries(lim, n)
        batch = ltp.planSwitchTimesBatch(*_tensors(qs))
        full = _full_rows(ltp, batch)
        _CACHE.update(key=key, v=(ltp, dof, lim, qs, batch, full, batch.traj_len.cpu().numpy(), batch.t_scaled.cpu().numpy()))
    return _CACHE["v"]


def _odd_range(n, dof):
    """A sub-range of [0, n) whose count * dof is not a multiple of 64."""
    first, count = 7, n - 20
    while (count * dof) % 64 == 0:
        count -= 1
    return first, count


@pytest.mark.parametrize("N", [1, 31, 32, 33, 64, 100])
def test_window_elements(N):
    ltp, dof, _ = _planner("panda")
    for count in (1, 3, 1000):
        assert ltp._lib.ltp_window_elements(ltp._h, count, N) == count * 4 * dof * ltp._lib.ltp_row_stride(N)


@pytest.mark.parametrize("name,n,pow_rule", [("panda", 3000, "libm"), ("panda", 3000, "exact"), ("ref", 2000, "libm"), ("ref", 2000, "exact"),
                                             ("ref30", 300, "libm"), ("ref30", 300, "exact")])
def test_bits_against_full_rows(name, n, pow_rule):
    """Every real sample of every window has the bits of the row sampleBatch wrote, every sample past the end follows the hold rule,
    `valid` follows its formula — no plan excepted; at first = 0, count = n and at a sub-range whose count * dof is no multiple of 64."""
    ltp, dof, lim, qs, batch, full, lens, t_scaled = _batch(name, n, pow_rule)
    rng = np.random.default_rng(99)
    for N in (1, 32, 33, 64, 100, 256):
        k = _draw_starts(rng, lens, t_scaled, N)
        _assert_coverage(k, N, lens, t_scaled, f"{name} {pow_rule} N={N}")
        _assert_window(ltp, batch, full, k, N, 0, n, f"{name} {pow_rule} N={N} whole batch")
        first, count = _odd_range(n, dof)
        assert (count * dof) % 64 != 0
        _assert_window(ltp, batch, full, k, N, first, count, f"{name} {pow_rule} N={N} plans [{first}, {first + count})")


def test_wide_windows():
    """N = 4096: most plans lie wholly inside the window, so every one of their runs does — more runs than a lane parks in one pass."""
    n, N = 500, 4096
    ltp, dof, lim, qs, batch, full, lens, t_scaled = _batch("panda", n)
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
    ltp, dof, lim, qs, batch, full, lens, t_scaled = _batch("panda", n)
    k = _draw_starts(np.random.default_rng(5), lens, t_scaled, N)
    r64, v64 = _assert_window(ltp, batch, full, k, N, 0, n, f"f64 N={N}")
    full32 = _full_rows(ltp, batch, torch.float32)
    r32, v32 = _assert_window(ltp, batch, full32, k, N, 0, n, f"f32 N={N}", dtype=torch.float32)
    assert torch.equal(v32, v64)
    planned = batch.traj_len > 0
    a, b = r32[planned][..., :N], r64[planned][..., :N].to(torch.float32)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "float32 window is not (float) of the float64 window"


def test_windows_against_the_oracle(oracle_mod):
    """q, v, a and j of the windows against the CPU oracle's own trajectories, 1e-9 (the bar of tests/test_gpu_parity.py)."""
    import torch
    n, N = 200, 100
    ltp, dof, lim = _planner("panda")
    qs = _queries(lim, n)
    orc = oracle_mod.Oracle(dof, TS, **lim)
    o = orc.plan_batch(*qs, sample=True)
    batch = ltp.planSwitchTimesBatch(*_tensors(qs))
    lens = batch.traj_len.cpu().numpy()
    assert np.array_equal(lens, o["traj_len"])
    k = _draw_starts(np.random.default_rng(3), lens, batch.t_scaled.cpu().numpy(), N)
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
    ltp, dof, lim, qs, batch, full, lens, t_scaled = _batch("panda", n)
    k = _draw_starts(np.random.default_rng(8), lens, t_scaled, N)
    good, _ = _assert_window(ltp, batch, full, k, N, 0, n, "intact batch")
    bad_qs = [x.copy() for x in qs]
    bad_qs[1][::5, 2] = 50.0
    ltp2, _, _ = _planner("panda")
    b2 = ltp2.planSwitchTimesBatch(*_tensors(bad_qs))
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
    import torch
    n, N = 1000, 64
    ltp, dof, lim = _planner("panda", semantics="matlab" if kind == "matlab" else "cpp")
    qs = _queries(lim, n)
    if kind == "limit_sets":
        scaled = [dict(lim, v_max=[f * x for x in lim["v_max"]], a_max=[f * x for x in lim["a_max"]], j_max=[f * x for x in lim["j_max"]])
                  for f in (1.0, 0.5, 0.25)]
        ltp.setLimitSets(*[np.array([s[key] for s in scaled], dtype=np.float64) for key in ("q_min", "q_max", "v_max", "a_max", "j_max")])
        # queries drawn for the slowest set pass checkInputs under all three
        idx = torch.from_numpy((np.arange(n) % 3).astype(np.int32)).to(DEV)
        qs = _queries(scaled[2], n)
        batch = ltp.planSwitchTimesBatch(*_tensors(qs), limit_set=idx)
    else:
        batch = ltp.planSwitchTimesBatch(*_tensors(qs))
    if kind == "retimed":
        torch.cuda.synchronize()
        slowest = batch.slowest.cpu().numpy().clip(0)
        t_star = batch.t_opt.cpu().numpy()[np.arange(n), slowest, 6]
        ltp.retimeBatch(batch, uniform=1.5 * float(np.median(t_star)))
    full = _full_rows(ltp, batch)
    if kind == "matlab":
        assert ltp.lastSamplerKernel().startswith("k_sample_walk_matlab")
    lens, t_scaled = batch.traj_len.cpu().numpy(), batch.t_scaled.cpu().numpy()
    k = _draw_starts(np.random.default_rng(21), lens, t_scaled, N)
    print(kind, "switch inside / ends past / starts past / planned:", _coverage(k, N, lens, t_scaled))
    assert np.mean(lens > 0) > 0.9
    _assert_window(ltp, batch, full, k, N, 0, n, kind)
    first, count = _odd_range(n, dof)
    _assert_window(ltp, batch, full, k, N, first, count, kind + " sub-range")


def test_per_plan_starts_equal_uniform_starts_and_state_at():
    import torch
    n, N = 1000, 64
    ltp, dof, lim, qs, batch, full, lens, t_scaled = _batch("panda", n)
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
    ltp, dof, lim = _planner("panda")
    qs = _queries(lim, n)
    batch = ltp.planSwitchTimesBatch(*_tensors(qs))
    lib, O = ltp._lib, _abi.WindowOpts
    R = ltp.windowRowStride(N)
    out = torch.full((n, 4, dof, R), 7.25, dtype=torch.float64, device=DEV)
    rec = batch.c_records()

    def call(o=None, raw=None, out_ptr=None, capacity=None, q=True, r=True):
        if raw is None and o is not None:
            raw = C.addressof(o)
        rc = lib.ltp_sample_window_batch(ltp._h, 0, n, C.byref(batch.queries) if q else None, C.byref(rec) if r else None, raw,
                                         out.data_ptr() if out_ptr is None else out_ptr, out.numel() if capacity is None else capacity, ltp._stream())
        return rc, (lib.ltp_last_error(ltp._h) or b"").decode()

    good = dict(size=C.sizeof(O), format=0, n_samples=N)
    assert call(O(**good))[0] == 0
    out.fill_(7.25)
    for kw, text in ((dict(q=False), "null"), (dict(r=False), "null"), (dict(raw=None), "NULL"), (dict(out_ptr=0), "null"),
                     (dict(out_ptr=out.data_ptr() + 8), "aligned"), (dict(capacity=out.numel() - 1), "ltp_window_elements")):
        rc, msg = call(O(**good), **kw) if "raw" not in kw else call()
        assert rc == INVALID and text in msg, (kw, rc, msg)
    for bad, text in ((dict(n_samples=0), "n_samples"), (dict(n_samples=-1), "n_samples"), (dict(format=2), "format"), (dict(size=C.sizeof(O) - 8), "size"),
                      (dict(size=C.sizeof(O) + 4), "multiple of 8")):
        rc, msg = call(O(**dict(good, **bad)))
        assert rc == INVALID and text in msg, (bad, rc, msg)
    # a newer caller's struct: zero bytes beyond the known fields pass, non-zero ones are refused
    buf = (C.c_ubyte * (C.sizeof(O) + 8))()
    newer = O(**dict(good, size=C.sizeof(O) + 8))
    C.memmove(buf, C.addressof(newer), C.sizeof(O))
    rc, msg = call(raw=C.addressof(buf))
    assert rc == 0, msg
    buf[C.sizeof(O) + 3] = 1
    rc, msg = call(raw=C.addressof(buf))
    assert rc == INVALID and "beyond the fields" in msg
    out.fill_(7.25)
    # the geometry rule, in ltp_state_at_batch's words
    for change, undo in ((lambda: ltp.setDoF(6), lambda: ltp.setDoF(dof)), (lambda: ltp.setSampleTime(0.002), lambda: ltp.setSampleTime(TS))):
        change()
        rc, msg = call(O(**good))
        rc2 = lib.ltp_state_at_batch(ltp._h, 0, n, C.byref(batch.queries), C.byref(rec), None, 0, out.data_ptr(), out.data_ptr(), out.data_ptr(), dof, 1, ltp._stream())
        msg2 = (lib.ltp_last_error(ltp._h) or b"").decode()
        assert rc == INVALID and rc2 == INVALID and msg == msg2 and "changed since the batch was planned" in msg
        undo()
    torch.cuda.synchronize()
    assert bool((out == 7.25).all().item()), "a refused call wrote to the buffer"
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
    ltp, dof, lim = _planner("panda")
    qs = _queries(lim, n)
    qs[0][3, 1] = 2.5                               # a goal beyond joint 1's range: planned, then END_LIMIT
    batch = ltp.planSwitchTimesBatch(*_tensors(qs))
    lens = batch.traj_len.cpu().numpy()
    k = _draw_starts(np.random.default_rng(1), lens, batch.t_scaled.cpu().numpy(), N)
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

    src, exe = tmp_path / "window.cc", tmp_path / "window"
    src.write_text(DROPIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "longtermplanner_amd"), "-lltp_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "longtermplanner_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    (tmp_path / "in.bin").write_bytes(np.concatenate([x.reshape(-1) for x in qs]).astype(np.float64).tobytes() + k.astype(np.int32).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    raw = (tmp_path / "out.bin").read_bytes()
    nb = rows.nbytes
    assert len(raw) == nb + 8 * n
    assert raw[:nb] == rows.tobytes() and raw[nb:nb + 4 * n] == valid.tobytes() and raw[nb + 4 * n:] == rec["status"].astype(np.int32).tobytes()


def test_graph_capture_and_replay_with_new_starts():
    """The call allocates nothing: captured on one stream and replayed once after first_sample was rewritten in place, it gives the
    windows of the new starts."""
    import torch
    n, N = 1000, 64
    ltp, dof, lim, qs, batch, full, lens, t_scaled = _batch("panda", n)
    rng = np.random.default_rng(77)
    ka, kb = _draw_starts(rng, lens, t_scaled, N), _draw_starts(rng, lens, t_scaled, N)
    assert np.count_nonzero(ka != kb) > 0.5 * n
    R = ltp.windowRowStride(N)
    k = torch.from_numpy(ka).to(DEV)
    out = torch.zeros((n, 4, dof, R), dtype=torch.float64, device=DEV)
    valid = torch.zeros((n,), dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ltp.sampleWindow(batch, 0, n, k, N, out=out, valid=valid)       # eager warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ltp.sampleWindow(batch, 0, n, k, N, out=out, valid=valid)
    k.copy_(torch.from_numpy(kb))
    out.zero_()
    valid.zero_()
    g.replay()
    torch.cuda.synchronize()
    exp, exp_valid, planned = _expected(full, batch.offsets, batch.traj_len, k, N, dof, 0, n)
    assert torch.equal(out.view(torch.int64)[..., :N][planned], exp[planned]) and torch.equal(valid, exp_valid)
    assert bool(torch.isnan(out[~planned][..., :N]).all().item())
