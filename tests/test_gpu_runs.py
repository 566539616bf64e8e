"""Every branch of the trajectory sampler on the GPU. At their own sample times the named limit sets have phases hundreds of samples
long: their dense-row figures establish the agreement with the oracle in the middle of long phases (tests/test_run_census_cpu.py).
Here every batch is one of tests/run_census.py: the project's generator under sample times of the order of the phases, and dyadic
inputs whose switching times fall on exact multiples of the sample time. Sampled switch indices collide, fills are empty or
negative, up to five correction terms land on one sample, the last correction is dropped, rows have 1 to 153 samples — shorter than
a padded row, than any cap and than any window. Rows, every sampler, the readers (knot grids included), the envelopes, a user consumer, MATLAB semantics,
the single-call kernel, limit sets and retime are compared with the CPU oracle (or with each other where the suite claims bits),
class by class: a mismatch names the run-census classes of the lanes concerned.

Tolerances are the suite's own: dense_compare.TOL = 1e-9 for q / v / a / j; bit identity of records and jerk rows under pow_rule
"exact" against the oracle's exact-pow twin and under "libm" behind the restated_host_libm fixture."""
import ctypes as C
import os

import numpy as np
import pytest

import horizon_checker as hc
import horizon_helpers as H
import knots_checker as kc
import retime_checker as rtc
import run_census as rc
from dense_compare import TOL
from gpu_helpers import DEV, REC_KEYS, _agree, _bits_equal, _host, _plan_rows, _planner, _rows, _tensors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLERS = ("fused", "walk", "walk_streaming", "table", "auto")
END_LIMIT, OVERFLOW, MATLAB_COMPLEX = 8, 32, 256


def _plans(n, which):
    m = np.zeros(n, dtype=bool)
    m[np.asarray(which, dtype=np.int64)] = True
    return m


def _compare_with_the_oracle(R, what, exact, status=True):
    """Lengths and verdicts plan by plan, records (bits where `exact`, else 1e-9), every q / v / a / j sample within 1e-9 and, where
    `exact`, jerk rows bit for bit."""
    cen, rec, orec, n = R["cen"], R["rec"], R["orec"], R["n"]
    planned = orec["status"] != 0
    dev_planned = (rec["status"] & ~(END_LIMIT | MATLAB_COMPLEX)) == 0
    assert np.array_equal(dev_planned, planned), f"{what}: planned verdicts differ: {rc.describe(cen, dev_planned != planned)}"
    bad = planned & (rec["traj_len"] != orec["traj_len"])
    assert not bad.any(), f"{what}: lengths differ: {rc.describe(cen, bad)}"
    if status:
        end = (rec["status"] & END_LIMIT) != 0
        assert np.array_equal(end, orec["status"] == 2), f"{what}: end-limit verdicts differ: {rc.describe(cen, end != (orec['status'] == 2))}"
    for k in ("t_scaled", "dir", "mod", "v_drive"):
        lanes = ~_agree(rec[k], orec[k], exact).reshape(n, R["dof"], -1).all(axis=2) & planned[:, None]
        assert not lanes.any(), f"{what}: {k} differs from the oracle ({'bits' if exact else '1e-9'}): {rc.describe(cen, lanes)}"
    worst = np.zeros(4)
    far = np.zeros((n, R["dof"]), dtype=bool)
    jerk = np.zeros((n, R["dof"]), dtype=bool)
    for p in np.nonzero(planned)[0]:
        got, want = _plan_rows(R, p), np.stack(R["orows"][p][1:])
        d = np.abs(got - want)
        worst = np.maximum(worst, d.max(axis=(1, 2)))
        far[p] = d.max(axis=(0, 2)) > TOL
        jerk[p] = (got[3].view(np.uint64) != want[3].view(np.uint64)).any(axis=1)
    print(f"{what}: {int(planned.sum())} plans, max |d| q v a j {worst}, lanes whose jerk rows differ in a bit {int(jerk.sum())}")
    assert not far.any(), f"{what}: rows differ from the oracle's by {worst} (1e-9): {rc.describe(cen, far)}"
    if exact:
        assert not jerk.any(), f"{what}: jerk rows differ from the oracle's in a bit: {rc.describe(cen, jerk)}"


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
@pytest.mark.parametrize("name", rc.BATCHES)
def test_rows_on_the_devices_records(oracle_mod, name, pow_rule, request):
    """Planned and sampled on the device: "exact" against the exact-pow twin, "libm" against the parity oracle where this host's libm
    is the restated one. Records and jerk rows bit for bit, lengths and end-limit verdicts plan by plan, every sample within 1e-9."""
    if pow_rule == "libm":
        request.getfixturevalue("restated_host_libm")
    R = _rows(oracle_mod, name, pow_rule)
    _compare_with_the_oracle(R, f"{name} {pow_rule}", exact=True)
    # the end-limit verdict without rows (ltp_end_limit_batch: a register walk that stops at the first tail run) is the sampler's
    b = R["ltp"].planSwitchTimesBatch(*_tensors(R["qs"]), end_limit=True)
    bad = _host(b)["status"] != R["rec"]["status"]
    assert not bad.any(), f"{name} {pow_rule}: the verdict of ltp_end_limit_batch differs from the sampler's: {rc.describe(R['cen'], bad)}"


@pytest.mark.parametrize("name", rc.BATCHES)
def test_rows_on_the_oracles_records(oracle_mod, name):
    """ltp_get_trajectory_host on the oracle's own records: the sampler alone, on any host. Every sample within 1e-9, jerk rows
    bit for bit (the jerk array involves no power)."""
    orc, lim, ts, qs, orec, cen = rc.batch(oracle_mod, name)
    orows = rc.all_rows(oracle_mod, name)
    ltp = _planner(orc.dof, lim, ts)
    planned = np.nonzero(orec["status"] != 0)[0]
    r = ltp.getTrajectoryBatchHost(orec["t_scaled"][planned], orec["dir"][planned], orec["mod"][planned], qs[1][planned], qs[2][planned],
                                   qs[3][planned], orec["v_drive"][planned])
    bad = planned[r["traj_len"] != orec["traj_len"][planned]]
    assert bad.size == 0, f"{name}: lengths differ: {rc.describe(cen, _plans(len(orec['status']), bad))}"
    R = dict(host=r["packed"], rec=dict(traj_len=r["traj_len"], offsets=r["offsets"]), dof=orc.dof)
    far = np.zeros(cen["live"].shape, dtype=bool)
    jerk = np.zeros(cen["live"].shape, dtype=bool)
    worst = np.zeros(4)
    for i, p in enumerate(planned):
        got, want = _plan_rows(R, i), np.stack(orows[p][1:])
        d = np.abs(got - want)
        worst = np.maximum(worst, d.max(axis=(1, 2)))
        far[p] = d.max(axis=(0, 2)) > TOL
        jerk[p] = (got[3].view(np.uint64) != want[3].view(np.uint64)).any(axis=1)
    print(f"{name}: rows on the oracle's records: {planned.size} plans, max |d| q v a j {worst}")
    assert not far.any(), f"{name}: rows differ from the oracle's by {worst} (1e-9): {rc.describe(cen, far)}"
    assert not jerk.any(), f"{name}: jerk rows differ from the oracle's in a bit: {rc.describe(cen, jerk)}"


def _expected_tile(R, lo, hi, off2, stored, stride, numel, capacity=None):
    """What a tile of `numel` elements must hold after plans [lo, hi) were sampled with `stored` [n] samples per row at `stride`,
    cut from the full rows; untouched elements 0. off2: the offsets of that row format. A plan that ends beyond `capacity` elements
    stores nothing. Returns (tile, first element of each plan in the tile, overflow [n])."""
    n, rows = R["n"], 4 * R["dof"]
    off = R["rec"]["offsets"].astype(np.int64)
    L = R["rec"]["traj_len"].astype(np.int64)
    off2 = off2.astype(np.int64)
    st = np.where(L > 0, stored, 0).astype(np.int64)
    rs, rs2 = (L + 31) // 32 * 32, (st + 31) // 32 * 32
    rel = off2 - off2[lo]
    over = np.zeros(n, dtype=bool)
    if capacity is not None:
        over = (st > 0) & (rel[:n] + rows * rs2 > capacity)
    inside = np.zeros(n, dtype=bool)
    inside[lo:hi] = True
    st = np.where(inside & ~over, st, 0)
    cnt = rows * st
    pid = np.repeat(np.arange(n), cnt)
    local = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    r, w = local // np.maximum(st[pid], 1), local % np.maximum(st[pid], 1)
    exp = np.zeros(numel)
    exp[rel[pid] + r * rs2[pid] + w] = R["host"][off[pid] + r * rs[pid] + w * stride]
    return exp, rel, over


def _tile_mismatch(R, got, exp, rel, lo, hi):
    """[n] plans whose part of the tile differs."""
    g, e = got.cpu().numpy(), exp.cpu().numpy()
    it = np.uint64 if g.dtype == np.float64 else np.uint32
    at = np.nonzero(g.view(it) != e.view(it))[0]
    return _plans(R["n"], np.clip(np.searchsorted(rel[lo:hi + 1], at, side="right") - 1 + lo, lo, hi - 1))


@pytest.mark.parametrize("name", rc.BATCHES)
def test_every_sampler_has_the_bits_of_the_full_rows(oracle_mod, name):
    """fused, walk, walk_streaming, table and auto: whole rows as float64 and float32; caps 1, 2, 3, 16, 32, 33 (below, at and above
    kWalkAutoCap; below and above most lengths here); strides 2 and 7, which exceed many lengths; no verdict; interleaves 1 and 7; a
    sub-range; a tile too small for the last plans. The same samples of the full rows, bit for bit, and the same status words."""
    import torch
    R = _rows(oracle_mod, name)
    n, dof, cen = R["n"], R["dof"], R["cen"]
    L = R["rec"]["traj_len"].astype(np.int64)
    status = R["rec"]["status"]
    ltp = _planner(dof, R["lim"], R["ts"])
    tens = _tensors(R["qs"])
    lo, hi = min(37, n // 7), n - min(101, n // 5)
    cases = [(0, 1, dt, {}) for dt in (torch.float64, torch.float32)]
    cases += [(cap, 1, torch.float64, {}) for cap in (1, 2, 3, 16, 32, 33)]
    cases += [(0, 2, torch.float64, {}), (0, 7, torch.float64, {}), (3, 7, torch.float32, {}), (33, 2, torch.float32, {})]
    cases += [(cap, 1, torch.float64, dict(verdict=False)) for cap in (3, 33)]
    cases += [(cap, 1, torch.float64, dict(interleave=i)) for cap in (0, 16) for i in (1, 7)]
    cases += [(cap, s, torch.float64, dict(sub=True, interleave=7)) for cap, s in ((0, 1), (2, 1), (33, 2))]
    cases += [(cap, 1, torch.float64, dict(small=True)) for cap in (0, 3, 33)]
    for cap, stride, dt, kw in cases:
        kw = dict(kw)
        sub, small = kw.pop("sub", False), kw.pop("small", False)
        ltp.setMaxSamples(cap)
        ltp.setSampleStride(stride)
        want_cnt = -(-L // stride)
        stored = np.minimum(want_cnt, cap) if cap else want_cnt
        first, last = (lo, hi) if sub else (0, n)
        exp = None
        for sampler in SAMPLERS:
            b = ltp.planSwitchTimesBatch(*tens)
            off2 = _host(b)["offsets"]
            if exp is None:
                assert all(ltp.storedSamples(int(x)) == int(y) for x, y in zip(L[:50], stored[:50]) if x > 0)
                numel = int(off2[last] - off2[first]) + 32
                capacity = int(off2[first + (last - first) * 2 // 3] - off2[first]) + 5 if small else None
                if small:
                    numel = capacity
                exp, rel, over = _expected_tile(R, first, last, off2, stored, stride, numel, capacity)
                exp = torch.from_numpy(exp).to(DEV).to(dt)
                assert not small or over.sum() >= 20, "the small tile leaves plans out"
            tile = torch.zeros(numel, dtype=dt, device=DEV)
            ltp.sampleBatchEx(b, first, last - first, tile, sampler=sampler, **kw)
            torch.cuda.synchronize()
            what = f"{name}: cap {cap} stride {stride} {dt} {kw} plans [{first}, {last}){' small tile' if small else ''} sampler {sampler} ({ltp.lastSamplerKernel()})"
            if not torch.equal(tile.view(torch.int64 if dt == torch.float64 else torch.int32), exp.view(torch.int64 if dt == torch.float64 else torch.int32)):
                bad = _tile_mismatch(R, tile, exp, rel, first, last)
                raise AssertionError(f"{what}: rows of {int(bad.sum())} plans differ from the full rows: {rc.describe(cen, bad)}")
            st = _host(b)["status"]
            want_st = status.copy()
            if kw.get("verdict") is False:          # (the walk kernels then stop at the cap; the other samplers may still form the verdict)
                st, want_st = st & ~END_LIMIT, want_st & ~END_LIMIT
            want_st[:first] &= ~END_LIMIT
            want_st[last:] &= ~END_LIMIT
            want_st[over] |= OVERFLOW
            if small:                               # (a plan that stores nothing may or may not have been walked for its verdict)
                st, want_st = st | (END_LIMIT * over), want_st | (END_LIMIT * over)
            bad = st != want_st
            assert not bad.any(), f"{what}: status words differ: {st[bad][:5]} against {want_st[bad][:5]}: {rc.describe(cen, bad)}"


@pytest.mark.parametrize("name", rc.BATCHES)
def test_readers_have_the_bits_of_the_full_rows(oracle_mod, name):
    """stateAt and replanStates at k = 0, 1, traj_len - 1, traj_len, beyond and random; sampleWindow and sampleHorizon with N = 1, 4, 32
    and strides 1, 3, k drawn so that k + N * s lies past the end for most plans."""
    import torch
    R = _rows(oracle_mod, name)
    ltp, batch, n, dof, cen = R["ltp"], R["batch"], R["n"], R["dof"], R["cen"]
    lens = R["rec"]["traj_len"].astype(np.int64)
    tl = batch.traj_len
    has = torch.from_numpy(lens > 0).to(DEV)
    off = torch.from_numpy(R["rec"]["offsets"].astype(np.int64)).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    rng = np.random.default_rng(17)
    for mode in ("first", "second", "last", "length", "beyond", "random", "uniform"):
        k = {"first": lambda: torch.zeros(n, dtype=torch.int32, device=DEV), "second": lambda: torch.ones(n, dtype=torch.int32, device=DEV),
             "last": lambda: (tl - 1).clamp(min=0).to(torch.int32), "length": lambda: tl.to(torch.int32),
             "beyond": lambda: (tl + 1000).to(torch.int32), "uniform": lambda: 2,
             "random": lambda: (torch.rand(n, device=DEV, generator=gen) * tl.clamp(min=1)).to(torch.int32)}[mode]()
        want = ltp.replanStates(batch, 0, n, R["full"], k)
        got = ltp.stateAt(batch, 0, n, k)
        got_jm = ltp.stateAt(batch, 3, n - 5, k if isinstance(k, int) else k[3:n - 2].contiguous(), layout="joint_major")
        torch.cuda.synchronize()
        kk = torch.full((n,), k, dtype=torch.int64, device=DEV) if isinstance(k, int) else k.long()
        exp, _, _ = hc.expected(R["full"], off, tl, torch.minimum(kk, (tl.long() - 1).clamp(min=0)), hc.window_grid(1), dof, 0, n)   # the state past the end is the last sample's
        for x, (w, g, gj) in enumerate(zip(want, got, got_jm)):
            bad = (w.view(torch.int64) != g.view(torch.int64)).any(dim=1).cpu().numpy()
            assert not bad.any(), f"{name}: stateAt ({mode}) differs from replanStates: {rc.describe(cen, bad)}"
            assert torch.equal(w[3:n - 2].t().contiguous(), gj), (name, mode)
            bad = ((g.view(torch.int64) != exp[:, x, :, 0]).any(dim=1) & has).cpu().numpy()
            assert not bad.any(), f"{name}: stateAt ({mode}) differs from the full rows: {rc.describe(cen, bad)}"
    for N in (1, 4, 32):
        for s in (1, 3):
            # four plans of five: the span ends at or up to N * s samples past the last sample; the rest anywhere, some at 0
            k = np.where(rng.random(n) < 0.8, lens - rng.integers(0, N * s + 1, n), rng.integers(-2, np.maximum(lens, 1) + 3)).astype(np.int32)
            k[1::11] = 0
            past = (np.maximum(k, 0) + N * s > lens)[lens > 0].mean()
            assert N * s == 1 or past >= 0.5, (name, N, s, past)
            kt = torch.from_numpy(k).to(DEV)
            exp, exp_valid, planned = hc.expected(R["full"], off, tl, kt, hc.stride_grid(N, s), dof, 0, n)
            calls = [("sampleHorizon", lambda: ltp.sampleHorizon(batch, 0, n, kt, N, s))]
            if s == 1:
                calls.append(("sampleWindow", lambda: ltp.sampleWindow(batch, 0, n, kt, N)))
            for what, call in calls:
                rows, valid = call()
                torch.cuda.synchronize()
                got = rows[..., :N].contiguous()
                bad = ((got.view(torch.int64) != exp).reshape(n, -1).any(dim=1) & planned).cpu().numpy()
                assert not bad.any(), f"{name}: {what} N {N} stride {s}: {int(bad.sum())} plans differ from the full rows: {rc.describe(cen, bad)}"
                assert torch.isnan(got[~planned]).all() and torch.equal(valid, exp_valid), (name, what, N, s)


@pytest.mark.parametrize("name", rc.BATCHES)
def test_knot_grids_have_the_bits_of_the_full_rows(oracle_mod, name):
    """sampleKnots as float64 and float32 (the float64 rows rounded once) on the three smallest grids and the MPC grid, a uniform k
    swept over 0 .. 8 and per-plan starts with negative and past-the-end ones, the whole batch and an odd sub-range: the bits of
    the full rows, the hold rule past the end, `valid` by its formula. ref_0.05 holds the lanes with kMaxSegments runs, six batches
    take more passes than one, dyadic_grid and dyadic_moving_1 hold the rows of 1 to 4 samples: asserted, not assumed."""
    import torch
    R = _rows(oracle_mod, name)
    ltp, batch, n, dof, cen = R["ltp"], R["batch"], R["n"], R["dof"], R["cen"]
    lens = R["rec"]["traj_len"]
    held = rc.assert_reader_shapes(name, cen, lens, R["rec"]["t_scaled"], R["ts"], kc.SMALL_GRIDS["unit"])
    print(f"{name}: {held}")
    full = {torch.float64: R["full"], torch.float32: R["full"].to(torch.float32)}
    describe = lambda plans: rc.describe(cen, plans)
    rng = np.random.default_rng(31)
    first, count = H.odd_range(n, dof)
    assert (count * dof) % 64 != 0
    for gname, g in dict(kc.SMALL_GRIDS, mpc=kc.GRIDS["mpc"]).items():
        ku = H.uniform_starts(rng, lens)
        assert np.count_nonzero(ku < 0) > 0 and np.count_nonzero(ku >= lens) > 0
        read = lambda lo, m: (lambda k, out: ltp.sampleKnots(batch, lo, m, k, H.grid_tensor(g), out=out))
        for k in list(range(9)) + [ku]:
            kh = np.full(n, k, dtype=np.int32) if isinstance(k, int) else k
            for dt, rows in full.items():
                what = f"{name} sampleKnots {dt} grid {gname} k {'per plan' if not isinstance(k, int) else k}"
                H.assert_rows(read(0, n), ltp, batch, rows, kh, g, 0, n, what, dtype=dt, describe=describe)
        for dt, rows in full.items():
            H.assert_rows(read(first, count), ltp, batch, rows, ku, g, first, count, f"{name} sampleKnots {dt} grid {gname}, plans [{first}, {first + count})",
                          dtype=dt, describe=describe)


@pytest.fixture(scope="module")
def consumer():
    from longtermplanner_amd import _abi
    _abi.lib()
    path = os.path.join(ROOT, "tests", "cpp", "libexample_consumer.so")
    assert os.path.exists(path), "tests/cpp/libexample_consumer.so is missing: run __graft_entry__.build()"
    lib = C.CDLL(path)
    lib.example_peak_velocity.restype = C.c_int
    lib.example_peak_velocity.argtypes = [C.c_void_p, C.c_longlong, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


@pytest.mark.parametrize("name", rc.BATCHES)
def test_envelopes_and_a_user_consumer_equal_the_reduced_rows(oracle_mod, consumer, name):
    """envelopeBatch with windows of 1, 2 and 5 samples: the exhaustive form has the bits of the reduced rows; the analytic form agrees
    with it by the rule of test_analytic_envelopes_agree_with_the_exhaustive_form (NaN pattern and statuses identical, within the
    samples, within 1e-12). And ltp_build_tables_batch through the peak-velocity consumer of tests/cpp/example_consumer.hip: the
    maximum |v|, its first sample and the count above a threshold are those of the rows, bit for bit."""
    import torch
    R = _rows(oracle_mod, name)
    ltp, n, dof, cen = R["ltp"], R["n"], R["dof"], R["cen"]
    tl = R["batch"].traj_len
    off = torch.from_numpy(R["rec"]["offsets"].astype(np.int64)).to(DEV)
    zero = torch.zeros(n, dtype=torch.int32, device=DEV)
    tens = _tensors(R["qs"])
    try:
        for window, n_windows, table_pass in ((1, 40, 0), (2, 24, -1), (5, 9, 1), (5, 36, 0)):
            ltp.setTablePass(table_pass)
            W = window * n_windows
            bits, _, planned = hc.expected(R["full"], off, tl, zero, hc.window_grid(W), dof, 0, n)          # past the end q holds the last position
            q = bits[:, 0].view(torch.float64).reshape(n, dof, n_windows, window)
            red = torch.stack([q.min(dim=3).values, q.max(dim=3).values], dim=3)
            res = {}
            for mode in ("exhaustive", "analytic"):
                ltp.setEnvelopeMode(mode)
                b = ltp.planSwitchTimesBatch(*tens)
                env = ltp.envelopeBatch(b, 0, n, window, n_windows)
                assert ("analytic" in ltp.lastSamplerKernel()) == (mode == "analytic"), ltp.lastSamplerKernel()
                torch.cuda.synchronize()
                res[mode] = (env, b.status.clone())
            ex, an = res["exhaustive"][0], res["analytic"][0]
            what = f"{name}: window {window} x {n_windows}, table pass {table_pass}"
            assert torch.equal(res["exhaustive"][1], torch.from_numpy(R["rec"]["status"]).to(DEV)), what
            bad = ((ex.view(torch.int64) != red.view(torch.int64)).reshape(n, -1).any(dim=1) & planned).cpu().numpy()
            assert not bad.any(), f"{what}: exhaustive envelopes differ from the reduced rows: {rc.describe(cen, bad)}"
            assert torch.isnan(ex[~planned]).all() and not torch.isnan(ex[planned]).any(), what
            assert torch.equal(torch.isnan(ex), torch.isnan(an)) and torch.equal(res["exhaustive"][1], res["analytic"][1]), what
            d = torch.nan_to_num((ex - an).abs(), nan=0.0)
            bad = (d > 1e-12).reshape(n, -1).any(dim=1).cpu().numpy()
            assert not bad.any(), f"{what}: analytic envelopes differ by {float(d.max())}: {rc.describe(cen, bad)}"
            out = ((an[..., 0] < ex[..., 0]) | (an[..., 1] > ex[..., 1])).reshape(n, -1).any(dim=1).cpu().numpy()
            assert not out.any(), f"{what}: an analytic envelope lies outside the samples: {rc.describe(cen, out)}"
    finally:
        ltp.setTablePass(0)
        ltp.setEnvelopeMode("analytic")
    # the consumer hook
    b = ltp.planSwitchTimesBatch(*tens)
    first = 5
    count = n - first
    tables = ltp.buildRunTables(b, first, count)
    lanes = count * dof
    thr = 0.35 * float(min(R["lim"]["v_max"]))
    mx = torch.full((lanes,), -7.0, dtype=torch.float64, device=DEV)
    at = torch.full((lanes,), -7, dtype=torch.int32, device=DEV)
    above = torch.full((lanes,), -7, dtype=torch.int64, device=DEV)
    assert consumer.example_peak_velocity(tables.data_ptr(), lanes, R["ts"], thr, mx.data_ptr(), at.data_ptr(), above.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(b.status.cpu().numpy()[first:], R["rec"]["status"][first:]), "the table pass forms the sampler's verdict"
    W = int(R["rec"]["traj_len"].max())
    bits, _, planned = hc.expected(R["full"], off, tl, zero, hc.window_grid(W), dof, 0, n)                   # past the end v is +0.0
    av = bits[first:, 1].view(torch.float64).abs()
    want_mx, want_at = av.max(dim=2).values, (av == av.max(dim=2, keepdim=True).values).to(torch.int32).argmax(dim=2)
    pl = planned[first:]
    mx, at, above = mx.view(count, dof), at.view(count, dof), above.view(count, dof)
    bad = np.zeros(n, dtype=bool)
    bad[first:] = (((mx.view(torch.int64) != want_mx.view(torch.int64)) | (at != want_at) | (above != (av > thr).sum(dim=2))).any(dim=1) & pl).cpu().numpy()
    assert not bad.any(), f"{name}: the consumer's reductions differ from the rows': {rc.describe(cen, bad)}"
    assert bool((mx[~pl] == -1.0).all()) and bool((at[~pl] == -1).all()) and bool((above[~pl] == 0).all())


@pytest.mark.parametrize("name", rc.MATLAB_BATCHES)
def test_matlab_semantics_by_class(oracle_mod, name):
    """Against the oracle's MATLAB twin: the 1-based corrections, mcut_*, mod()'s round-off rule on exact multiples and the
    last-joint-only acceleration tail. Rows on the twin's own records (the sampler alone): every sample within 1e-9, jerk rows bit
    for bit. Planned on the device: records within 1e-9 and, for the plans whose sampled switch indices are the twin's, the rows;
    every MATLAB sampler has the bits of the others."""
    import torch
    orc, lim, ts, qs, orec, cen = rc.batch(oracle_mod, name, "matlab")
    orows = rc.all_rows(oracle_mod, name, "matlab")
    n, dof = len(orec["status"]), orc.dof
    assert np.all(orec["status"] != 0)
    ltp = _planner(dof, lim, ts, semantics="matlab")
    r = ltp.getTrajectoryBatchHost(orec["t_scaled"], orec["dir"], orec["mod"], qs[1], qs[2], qs[3], orec["v_drive"])
    bad = r["traj_len"] != orec["traj_len"]
    assert not bad.any(), f"{name} matlab: lengths differ: {rc.describe(cen, bad)}"
    Rh = dict(host=r["packed"], rec=dict(traj_len=r["traj_len"], offsets=r["offsets"]), dof=dof)
    far, jerk, worst = np.zeros((n, dof), dtype=bool), np.zeros((n, dof), dtype=bool), np.zeros(4)
    for p in range(n):
        got, want = _plan_rows(Rh, p), np.stack(orows[p][1:])
        d = np.abs(got - want)
        worst = np.maximum(worst, d.max(axis=(1, 2)))
        far[p] = d.max(axis=(0, 2)) > TOL
        jerk[p] = (got[3].view(np.uint64) != want[3].view(np.uint64)).any(axis=1)
    print(f"{name} matlab: rows on the twin's records: max |d| q v a j {worst}")
    assert not far.any(), f"{name} matlab: rows differ from the twin's by {worst} (1e-9): {rc.describe(cen, far)}"
    assert not jerk.any(), f"{name} matlab: jerk rows differ from the twin's in a bit: {rc.describe(cen, jerk)}"
    # planned on the device
    R = _rows(oracle_mod, name, semantics="matlab")
    rec = R["rec"]
    assert np.array_equal((rec["status"] & ~MATLAB_COMPLEX) == 0, orec["status"] != 0)
    for k in ("t_scaled", "dir", "mod", "v_drive"):
        lanes = ~_agree(rec[k], orec[k], False).reshape(n, dof, -1).all(axis=2)
        assert not lanes.any(), f"{name} matlab: {k} differs from the twin (1e-9): {rc.describe(cen, lanes)}"
    same = (rc.switch_indices(rec["t_scaled"], ts) == cen["s"]).all(axis=(1, 2)) & (rec["traj_len"] == orec["traj_len"])
    print(f"{name} matlab: {int(same.sum())} of {n} plans have the twin's sampled switch indices")
    assert same.sum() >= 0.9 * n
    far = np.zeros((n, dof), dtype=bool)
    for p in np.nonzero(same)[0]:
        far[p] = np.abs(_plan_rows(R, p) - np.stack(orows[p][1:])).max(axis=(0, 2)) > TOL
    assert not far.any(), f"{name} matlab: rows of plans planned on the device differ from the twin's (1e-9): {rc.describe(cen, far)}"
    for sampler in ("walk", "walk_streaming", "table", "auto"):
        b = R["ltp"].planSwitchTimesBatch(*_tensors(qs))
        tile = torch.zeros_like(R["full"])
        R["ltp"].sampleBatchEx(b, 0, n, tile, sampler=sampler)
        torch.cuda.synchronize()
        if not torch.equal(tile.view(torch.int64), R["full"].view(torch.int64)):
            rel = rec["offsets"].astype(np.int64)
            raise AssertionError(f"{name} matlab: sampler {sampler}: rows differ: {rc.describe(R['cen'], _tile_mismatch(R, tile, R['full'], rel, 0, n))}")


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
def test_single_calls_have_the_bits_of_the_batch(oracle_mod, pow_rule):
    """planTrajectory (the single-call kernel) on 20 plans of every class, drawn from the batch that holds most of it: verdict,
    length and rows are the batch's, bit for bit."""
    from longtermplanner_amd import Trajectory
    rng = np.random.default_rng(23)
    best = {}
    for name in rc.BATCHES:
        for k, c in rc.batch(oracle_mod, name)[5]["totals"].items():
            if c > best.get(k, (0, None))[0]:
                best[k] = (c, name)
    calls = 0
    for k, (c, name) in sorted(best.items(), key=lambda kv: kv[1][1]):
        R = _rows(oracle_mod, name, pow_rule)
        lanes = np.argwhere(R["cen"]["masks"][k])
        for p in np.unique(lanes[rng.choice(len(lanes), min(20, len(lanes)), replace=False)][:, 0]):
            traj = Trajectory()
            ok = R["ltp"].planTrajectory(*[x[p] for x in R["qs"]], traj)
            calls += 1
            what = f"{name} {pow_rule}: class {k}: plan {p}: {rc.describe(R['cen'], _plans(R['n'], [p]))}"
            assert ok == (R["rec"]["status"][p] == 0), f"{what}: the single call returns {ok}, the batch's status is {R['rec']['status'][p]}"
            assert traj.length == R["rec"]["traj_len"][p], what
            if traj.length > 0:
                assert _bits_equal(np.stack([traj.q, traj.v, traj.a, traj.j]), _plan_rows(R, p)), f"{what}: the single call's rows differ from the batch's"
    print(f"{calls} single calls over {len(best)} classes")
    assert len(best) >= len(rc.CLASSES) - 4


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
def test_limit_sets_mix_coarse_and_fine_sets(oracle_mod, pow_rule):
    """One batch under Ts 0.1 whose queries use panda (rows of 7-31 samples, every lane collided) or the soft set (up to 250 samples,
    mostly uncollided): records, verdicts and rows have the bits of the per-set handles."""
    import torch
    from longtermplanner_amd import generate_queries, limit_set
    import branch_census as bc
    n, ts = 1200, 0.1
    sets = [limit_set("panda")[1], bc.soft_limits(7)]
    per = [generate_queries(n, s, seed=rc.SEED + 10 * k) for k, s in enumerate(sets)]
    idx = np.random.default_rng(3).integers(0, 2, n).astype(np.int32)
    qs = [np.ascontiguousarray(np.choose(idx[:, None], [p[f] for p in per])) for f in range(4)]
    ltp = _planner(7, sets[0], ts, pow_rule=pow_rule)
    ltp.setLimitSets(*[np.array([s[k] for s in sets], dtype=np.float64) for k in ("q_min", "q_max", "v_max", "a_max", "j_max")])
    b = ltp.planSwitchTimesBatch(*_tensors(qs), limit_set=torch.from_numpy(idx).to(DEV))
    off = _host(b)["offsets"]
    tile = torch.zeros(int(off[-1]) + 32, dtype=torch.float64, device=DEV)
    ltp.sampleBatchEx(b, 0, n, tile)
    mixed = _host(b)
    M = dict(host=tile.cpu().numpy(), rec=mixed, dof=7)
    for s, lim in enumerate(sets):
        ps = _planner(7, lim, ts, pow_rule=pow_rule)
        bs = ps.planSwitchTimesBatch(*_tensors(qs))
        offs = _host(bs)["offsets"]
        rows = torch.zeros(int(offs[-1]) + 32, dtype=torch.float64, device=DEV)
        ps.sampleBatchEx(bs, 0, n, rows)
        ref = _host(bs)
        S = dict(host=rows.cpu().numpy(), rec=ref, dof=7)
        cen = rc.census(ref["t_scaled"], ref["traj_len"], ts)
        m = idx == s
        for k in REC_KEYS:
            bad = ~_agree(mixed[k], ref[k], True).reshape(n, -1).all(axis=1) & m
            assert not bad.any(), f"set {s} {pow_rule}: {k} of {int(bad.sum())} queries differs from the per-set handle: {rc.describe(cen, bad)}"
        bad = _plans(n, [p for p in np.nonzero(m & (ref["traj_len"] > 0))[0] if not _bits_equal(_plan_rows(M, p), _plan_rows(S, p))])
        assert not bad.any(), f"set {s} {pow_rule}: rows differ from the per-set handle's: {rc.describe(cen, bad)}"
        t = cen["totals"]
        print(f"set {s} {pow_rule}: {int(m.sum())} queries; of all {n} under this set: cc781 {t['cc781_landed']}, w2 {t['w2']}, len <= 32 {t['len_le32']}")
    assert (mixed["traj_len"][idx == 0] <= 32).all() and (mixed["traj_len"][idx == 1] > 32).sum() >= 100


@pytest.mark.parametrize("pow_rule", ["exact", "libm"])
def test_retime_of_a_coarse_batch_matches_the_checker(oracle_mod, pow_rule):
    """soft_0.25 retimed to 1.5 x T*: records against retime_checker.retime (bits under "exact" and where this host's libm is the
    restated one, else 1e-9), rows of every retimed plan against the checker's trajectory within 1e-9."""
    import torch
    from longtermplanner_amd import LongTermPlanner, unpack_trajectory
    name = "soft_0.25"
    orc, lim, ts, qs, orec, _ = rc.batch(oracle_mod, name, exact_pow=(pow_rule == "exact"))
    n, dof = len(orec["status"]), orc.dof
    exact = pow_rule == "exact" or LongTermPlanner.powRuleMatchingHostLibm()[0] == "libm"
    ltp = _planner(dof, lim, ts, pow_rule=pow_rule)
    batch = ltp.planSwitchTimesBatch(*_tensors(qs))
    plain = _host(batch)
    assert np.array_equal(rtc.oracle_eligible(orec), rtc.device_eligible(plain))
    T = 1.5 * rtc.t_star(plain)
    ltp.retimeBatch(batch, t_target=torch.from_numpy(np.ascontiguousarray(T)).to(DEV))
    dev = _host(batch)
    chk, retimed, cases = rtc.retime(orc, orec, *qs, T)
    assert retimed.sum() >= 0.9 * n
    cen = rc.census(chk["t_scaled"], np.where(retimed, chk["traj_len"], 0), ts)
    print(f"{name} retimed {pow_rule}: {int(retimed.sum())} plans, traj_len {int(chk['traj_len'][retimed].min())}-{int(chk['traj_len'][retimed].max())}: {cen['totals']}")
    for key in ("t_scaled", "v_drive", "mod", "traj_len"):
        bad = ~_agree(dev[key], chk[key], exact).reshape(n, -1).all(axis=1) & retimed
        assert not bad.any(), f"{name} retimed {pow_rule}: {key} differs from the checker: {rc.describe(cen, bad)}"
    off = dev["offsets"]
    tile = torch.zeros(int(off[-1]) + 32, dtype=torch.float64, device=DEV)
    ltp.sampleBatchEx(batch, 0, n, tile)
    torch.cuda.synchronize()
    rows = tile.cpu().numpy()
    far = np.zeros((n, dof), dtype=bool)
    for p in np.nonzero(retimed)[0]:
        L, q, v, a, j = rtc.trajectory(orc, chk, p, qs[1], qs[2], qs[3])
        got = np.stack(unpack_trajectory(rows, int(off[p]), dof, L))
        far[p] = np.abs(got - np.stack([q, v, a, j])).max(axis=(0, 2)) > TOL
    assert not far.any(), f"{name} retimed {pow_rule}: rows differ from the checker's (1e-9): {rc.describe(cen, far)}"
