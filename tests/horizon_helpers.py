"""What the GPU modules of the four horizon readers share (test infrastructure, not a test module): tests/test_gpu_window.py,
tests/test_gpu_horizon.py, tests/test_gpu_knots.py and tests/test_gpu_envelope_knots.py. A planner by limit-set name, seeded queries,
a planned batch with its full rows (the yardstick of tests/horizon_checker.py), the retimed / limit-set / MATLAB batch, the refusals
every reader entry has in common, the compile-and-run harness of the drop-in programs and the graph-capture harness; and the
yardstick of the stop horizons (composition, assert_stop_knots), which tests/test_gpu_stop_knots.py, tests/test_gpu_stop_runs.py and
tests/test_gpu_structure.py share."""
import ctypes as C
import os
import subprocess

import numpy as np

import horizon_checker as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = 0.001
DEV = "cuda:0"
SEED = 4242
INVALID = 1
PATTERN = 7.25          # what a buffer holds before a call that must not write (all of) it


def planner(name, pow_rule="libm", semantics="cpp"):
    from longtermplanner_amd import LongTermPlanner, limit_set
    dof, lim = limit_set(name)
    ltp = LongTermPlanner(dof, TS, device=0, **lim)
    ltp.setPowRule(pow_rule)
    ltp.setSemantics(semantics)
    return ltp, dof, lim


def queries(lim, n, seed=SEED):
    from longtermplanner_amd import generate_queries
    return [np.ascontiguousarray(x) for x in generate_queries(n, lim, seed=seed)]


def tensors(qs):
    import torch
    return [torch.from_numpy(x).to(DEV) for x in qs]


def grid_tensor(g):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(g, dtype=np.int32))).to(DEV)


def full_rows(ltp, batch, dtype=None):
    """Whole rows of every plan of the batch through the existing sampler (sampleBatch): the yardstick."""
    import torch
    n = batch.n
    total = int(batch.offsets[n].item())
    full = torch.zeros(max(total, 2), dtype=dtype or torch.float64, device=DEV)
    ltp.sampleBatch(batch, 0, n, full)
    torch.cuda.synchronize()
    return full


_CACHE = {}


def batch(name, n, pow_rule="libm", semantics="cpp"):
    """Planned batch + its full float64 rows + host copies of traj_len and t_scaled; the latest one is kept."""
    key = (name, n, pow_rule, semantics)
    if _CACHE.get("key") != key:
        _CACHE.clear()
        ltp, dof, lim = planner(name, pow_rule, semantics)
        qs = queries(lim, n)
        b = ltp.planSwitchTimesBatch(*tensors(qs))
        full = full_rows(ltp, b)
        _CACHE.update(key=key, v=(ltp, dof, lim, qs, b, full, b.traj_len.cpu().numpy(), b.t_scaled.cpu().numpy()))
    return _CACHE["v"]


def odd_range(n, dof):
    """A sub-range of [0, n) whose count * dof is not a multiple of 64."""
    first, count = 7, n - 20
    while (count * dof) % 64 == 0:
        count -= 1
    return first, count


def other_batch(kind, n):
    """A panda batch of another kind with its full rows — "retimed": every plan stretched to 1.5 times the median optimum;
    "limit_sets": three bound limit sets by plan index mod 3; "matlab": MATLAB semantics (full rows from the walk sampler).
    Returns (ltp, dof, batch, full, traj_len, t_scaled), the last two on the host."""
    import torch
    ltp, dof, lim = planner("panda", semantics="matlab" if kind == "matlab" else "cpp")
    qs = queries(lim, n)
    if kind == "limit_sets":
        scaled = [dict(lim, v_max=[f * x for x in lim["v_max"]], a_max=[f * x for x in lim["a_max"]], j_max=[f * x for x in lim["j_max"]])
                  for f in (1.0, 0.5, 0.25)]
        ltp.setLimitSets(*[np.array([s[key] for s in scaled], dtype=np.float64) for key in ("q_min", "q_max", "v_max", "a_max", "j_max")])
        # queries drawn for the slowest set pass checkInputs under all three
        idx = torch.from_numpy((np.arange(n) % 3).astype(np.int32)).to(DEV)
        qs = queries(scaled[2], n)
        b = ltp.planSwitchTimesBatch(*tensors(qs), limit_set=idx)
    else:
        b = ltp.planSwitchTimesBatch(*tensors(qs))
    if kind == "retimed":
        torch.cuda.synchronize()
        slowest = b.slowest.cpu().numpy().clip(0)
        t_star = b.t_opt.cpu().numpy()[np.arange(n), slowest, 6]
        ltp.retimeBatch(b, uniform=1.5 * float(np.median(t_star)))
    full = full_rows(ltp, b)
    if kind == "matlab":
        assert ltp.lastSamplerKernel().startswith("k_sample_walk_matlab")
    lens = b.traj_len.cpu().numpy()
    assert np.mean(lens > 0) > 0.9
    return ltp, dof, b, full, lens, b.t_scaled.cpu().numpy()


def assert_rows(read, ltp, b, full, k_host, g, first, count, what, dtype=None, stride=None, describe=None):
    """One call read(k, out) -> (rows, valid) of a row reader over plans [first, first + count) with starts
    k_host[first:first + count], compared with the full rows on the grid g (horizon_checker.expected). The buffer is pre-filled
    with a pattern: elements [N, R) of a row must keep it. stride: g is stride * arange(N), and `valid` is also held against the
    closed form the header documents for it. describe: names the plans that differ, given their mask over the whole batch."""
    import torch
    dof, N = b.dof, len(g)
    R = ltp.windowRowStride(N)
    k = torch.from_numpy(np.ascontiguousarray(k_host[first:first + count])).to(DEV)
    out = torch.full((count, 4, dof, R), PATTERN, dtype=dtype or torch.float64, device=DEV)
    rows, valid = read(k, out)
    torch.cuda.synchronize()
    exp, exp_valid, planned = hc.expected(full, b.offsets, b.traj_len, k, g, dof, first, count)
    got = hc.int_view(rows)[..., :N]
    bad = (got != exp).flatten(1).any(dim=1) & planned
    if describe is not None and bool(bad.any().item()):
        mask = np.zeros(b.n, dtype=bool)
        mask[first:first + count] = bad.cpu().numpy()
        raise AssertionError(f"{what}: {int(bad.sum().item())} plans differ from the full rows: {describe(mask)}")
    assert int(bad.sum().item()) == 0, f"{what}: {int(bad.sum().item())} plans differ from the full rows, first local plan {int(bad.nonzero()[0].item())}"
    assert bool(torch.isnan(rows[~planned][..., :N]).all().item()), f"{what}: a plan without a trajectory is not NaN"
    assert torch.equal(valid, exp_valid), f"{what}: valid differs"
    if stride is not None:
        closed = hc.strided_valid(b.traj_len[first:first + count].long(), k.long().clamp(min=0), N, stride)
        assert torch.equal(valid, closed), f"{what}: valid differs from min(N, ceil(max(0, traj_len - k) / s))"
    if R > N:
        assert bool((rows[..., N:] == PATTERN).all().item()), f"{what}: elements [N, R) of a row were written"
    return rows, valid


def composition(ltp, batch, first, count, k, grid, stopper=None):
    """Y, the yardstick of the stop horizons: sampleKnots, a permute to [count * N, dof] states, torch.clamp of the accelerations, ONE
    planStopBatch(check="braking") with the limit-set index repeated N times. Returns (yardstick [count, 2, dof, N], valid, beyond
    [count, dof, N]: |a| > a_max of the sampled accelerations).
    stopper: the planner that runs the stop step (default: ltp itself). A handle follows ONE bound limit-set index, so a batch with
    an index needs a second handle with the same sets for the count * N states' repeated index."""
    stopper = stopper or ltp
    import torch
    dof, N = batch.dof, int(grid.numel())
    rows, valid = ltp.sampleKnots(batch, first, count, k, grid)
    st = rows[..., :N].permute(1, 0, 3, 2).reshape(4, count * N, dof)        # [array][state = (plan, knot)][joint]
    q0, v0, a0 = (st[x].contiguous() for x in range(3))
    ls = getattr(batch, "limit_set", None)
    ls = ls[first:first + count].repeat_interleave(N).contiguous() if ls is not None else None
    am = stopper._a_max_of(ls, a0.device)
    beyond = (a0.abs() > am).view(count, N, dof).permute(0, 2, 1)
    sb = stopper.planStopBatch(q0, v0, torch.clamp(a0, min=-am, max=am).contiguous(), check="braking", limit_set=ls)
    y = torch.stack([sb.q_stop.view(count, N, dof).permute(0, 2, 1), sb.t_opt[..., 6].view(count, N, dof).permute(0, 2, 1)], dim=1)
    torch.cuda.synchronize()
    return y.contiguous(), valid, beyond


def assert_stop_knots(ltp, batch, k_host, g, first, count, what, modes=(True, False), stopper=None, describe=None):
    """stopKnots over plans [first, first + count) with starts k_host[first:first + count] (or one int for every plan) in both
    acceleration modes against Y: int64 views of the planned plans, NaN for the others, `valid` sampleKnots', PATTERN in [N, R).
    describe: names the plans that differ, given their mask over the whole batch. Returns the number of elements the strict mode
    refused."""
    import torch
    dof, N = batch.dof, len(g)
    R = ltp.windowRowStride(N)
    grid = grid_tensor(g)
    k = k_host if isinstance(k_host, int) else torch.from_numpy(np.ascontiguousarray(k_host[first:first + count])).to(DEV)
    y, y_valid, beyond = composition(ltp, batch, first, count, k, grid, stopper)
    planned = batch.traj_len[first:first + count] > 0
    refused = 0
    for clamp in modes:
        out = torch.full((count, 2, dof, R), PATTERN, dtype=torch.float64, device=DEV)
        got, valid = ltp.stopKnots(batch, first, count, k, grid, clamp_acceleration=clamp, out=out)
        torch.cuda.synchronize()
        exp = y if clamp else torch.where(beyond[:, None].expand_as(y), torch.full_like(y, float("nan")), y)
        bad = (hc.int_view(got[..., :N].contiguous()) != hc.int_view(exp)).flatten(1).any(dim=1) & planned
        nbad = int(bad.sum().item())
        if nbad and describe is not None:
            mask = np.zeros(batch.n, dtype=bool)
            mask[first:first + count] = bad.cpu().numpy()
            raise AssertionError(f"{what} clamp={clamp}: {nbad} plans differ from the composition: {describe(mask)}")
        assert nbad == 0, f"{what} clamp={clamp}: {nbad} plans differ from the composition, first local plan {int(bad.nonzero()[0].item())}"
        assert bool(torch.isnan(got[~planned][..., :N]).all().item()), f"{what}: a plan without a trajectory is not NaN"
        assert torch.equal(valid, y_valid), f"{what}: valid differs from sampleKnots'"
        if R > N:
            assert bool((got[..., N:] == PATTERN).all().item()), f"{what}: elements [N, R) of a row were written"
        if not clamp:
            refused = int((beyond & planned[:, None, None]).sum().item())
    return refused


def uniform_starts(rng, lens):
    """Uniform over [-10, traj_len + 50); every eighth plan starts at -3 and the one after it at traj_len + 5, so that negative starts
    and starts past the end occur in the smallest batch too."""
    L = lens.astype(np.int64)
    k = rng.integers(-10, L + 50)
    i = np.arange(len(L)) % 8
    return np.where(i == 6, -3, np.where(i == 7, L + 5, k)).astype(np.int32)


def reader_call(entry, ltp, b, n, out, capacity=None):
    """The `call` closure of a reader's refusal test: entry(handle, 0, n, queries, records, opts, buffer, capacity, stream) with
    any argument replaced — o: an opts struct, raw: its address instead, out_ptr / capacity: instead of buf's (buf: `out` unless
    given; capacity: buf.numel() unless a default is given here), q / r = False: NULL queries / records. Returns (rc, last error)."""
    rec = b.c_records()
    default = capacity

    def call(o=None, raw=None, out_ptr=None, capacity=None, q=True, r=True, buf=None):
        buf = out if buf is None else buf
        if raw is None and o is not None:
            raw = C.addressof(o)
        if capacity is None:
            capacity = buf.numel() if default is None else default
        rc = entry(ltp._h, 0, n, C.byref(b.queries) if q else None, C.byref(rec) if r else None, raw,
                   buf.data_ptr() if out_ptr is None else out_ptr, capacity, ltp._stream())
        return rc, (ltp._lib.ltp_last_error(ltp._h) or b"").decode()
    return call


def common_refusals(ltp, b, n, dof, call, O, good, out, short, elements_name):
    """The refusals every reader entry shares, against `call` (reader_call) and the fields `good` of a call that passes: each is
    LTP_ERR_INVALID_ARGUMENT with a text that names the reason — null queries, records and opts; a null or misaligned buffer; the
    capacity `short` (one element too few: the text names `elements_name`); a `size` too small or no multiple of 8; a newer
    caller's struct, whose zero tail passes and whose non-zero tail is refused; a geometry changed since the batch was planned, in
    the words of ltp_state_at_batch. `out` holds PATTERN afterwards, as it must after the refused calls."""
    import torch
    lib = ltp._lib
    rec = b.c_records()
    assert call(O(**good))[0] == 0
    torch.cuda.synchronize()
    out.fill_(PATTERN)
    for kw, text in ((dict(q=False), "null"), (dict(r=False), "null"), (dict(raw=None), "NULL"), (dict(out_ptr=0), "null"),
                     (dict(out_ptr=out.data_ptr() + 8), "aligned"), (dict(capacity=short), elements_name)):
        rc, msg = call(O(**good), **kw) if "raw" not in kw else call()
        assert rc == INVALID and text in msg, (kw, rc, msg)
    for bad, text in ((dict(size=C.sizeof(O) - 8), "size"), (dict(size=C.sizeof(O) + 4), "multiple of 8")):
        rc, msg = call(O(**dict(good, **bad)))
        assert rc == INVALID and text in msg, (bad, rc, msg)
    assert bool((out == PATTERN).all().item()), "a refused call wrote to the buffer"
    # a newer caller's struct: zero bytes beyond the known fields pass, non-zero ones are refused
    buf = (C.c_ubyte * (C.sizeof(O) + 8))()
    newer = O(**dict(good, size=C.sizeof(O) + 8))
    C.memmove(buf, C.addressof(newer), C.sizeof(O))
    rc, msg = call(raw=C.addressof(buf))
    assert rc == 0, msg
    buf[C.sizeof(O) + 3] = 1
    rc, msg = call(raw=C.addressof(buf))
    assert rc == INVALID and "beyond the fields" in msg
    torch.cuda.synchronize()
    out.fill_(PATTERN)
    # the geometry rule, in ltp_state_at_batch's words
    for change, undo in ((lambda: ltp.setDoF(6), lambda: ltp.setDoF(dof)), (lambda: ltp.setSampleTime(0.002), lambda: ltp.setSampleTime(TS))):
        change()
        rc, msg = call(O(**good))
        rc2 = lib.ltp_state_at_batch(ltp._h, 0, n, C.byref(b.queries), C.byref(rec), None, 0, out.data_ptr(), out.data_ptr(), out.data_ptr(), dof, 1, ltp._stream())
        msg2 = (lib.ltp_last_error(ltp._h) or b"").decode()
        assert rc == INVALID and rc2 == INVALID and msg == msg2 and "changed since the batch was planned" in msg
        undo()
    torch.cuda.synchronize()
    assert bool((out == PATTERN).all().item()), "a refused call wrote to the buffer"


def run_dropin(tmp_path, name, source, payload):
    """Compile `source` — a program on the drop-in header — with plain g++ -Wall against the library, run it on the bytes `payload`
    (argv[1]) and return the bytes it wrote (argv[2])."""
    src, exe = tmp_path / (name + ".cc"), tmp_path / name
    src.write_text(source)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "longtermplanner_amd"), "-lltp_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "longtermplanner_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    (tmp_path / "in.bin").write_bytes(payload)
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return (tmp_path / "out.bin").read_bytes()


def assert_dropin_bytes(raw, out, valid, status):
    """What every drop-in program writes: the output array, valid, the status words — the bytes of the host call."""
    nb, n = out.nbytes, len(valid)
    assert len(raw) == nb + 8 * n
    assert raw[:nb] == out.tobytes() and raw[nb:nb + 4 * n] == valid.tobytes() and raw[nb + 4 * n:] == status.astype(np.int32).tobytes()


def capture(call):
    """call() once eagerly on a side stream (the warm-up capture needs), then captured into a graph: the call allocates nothing."""
    import torch
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        call()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    return graph


def replay(graph, rewrites, out, valid):
    """Rewrite device inputs in place — rewrites: (tensor, host array) pairs —, clear the outputs, replay once, wait."""
    import torch
    for t, new in rewrites:
        t.copy_(torch.from_numpy(new))
    out.zero_()
    valid.zero_()
    graph.replay()
    torch.cuda.synchronize()
