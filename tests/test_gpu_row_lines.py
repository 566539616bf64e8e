"""Dense rows end on a 64-byte line: every sampler writes a row of `slen` stored samples up to ltp_row_line(slen) — the samples, then
+0.0 — and nothing beyond (include/ltp_hip.h, ltp_sample_batch). Checked element by element over whole tiles pre-filled with 7.25,
for every writer (fused build, table pass, walk kernels in both forms, the one-launch small path) and every row format whose rows
end differently: whole rows, caps that leave a single partial line (1, 3), a cap inside a line (37), a whole-line cap (64), every
3rd sample; float64 and float32."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_PLANS = 400
SEED = 2025
REJECTED = 11            # a plan without a trajectory in the middle of the first items
FILL = 7.25
GUARD = 64               # elements of the tile before the first and after the last plan of a call
FORMATS = [(0, 1), (37, 1), (1, 1), (3, 1), (64, 1), (0, 3)]          # (cap, stride)


@pytest.fixture(scope="module")
def amd():
    import longtermplanner_amd as m
    return m


@pytest.fixture(scope="module", params=[7, 9])
def planned(request, amd):
    """Planner, device queries and the host copy of the same queries for `dof` joints: panda at 7, the reference limits at 9 (an
    item of the fused build is a group of 8 joints, of the table pass 7: two groups per plan)."""
    import torch
    dof = request.param
    _, lim = amd.limit_set("panda") if dof == 7 else amd.limit_set("ref", dof=9)
    ltp = amd.LongTermPlanner(dof, 0.001, device=0, **lim)
    host = [x.copy() for x in amd.generate_queries(N_PLANS, lim, seed=SEED)]
    host[1][REJECTED, 0] = 99.0                                       # q_0 outside the limits: checkInputs rejects the plan
    dev = [torch.from_numpy(x).cuda() for x in host]
    return dof, ltp, dev, host


def _geometry(ltp, traj_len, esize):
    lib = ltp._lib
    slen = np.array([ltp.storedSamples(int(l)) if l > 0 else 0 for l in traj_len], dtype=np.int64)
    stride = np.array([lib.ltp_row_stride(int(s)) for s in slen], dtype=np.int64)
    line = np.array([lib.ltp_row_line(int(s), esize) for s in slen], dtype=np.int64)
    return slen, stride, line


def _classes(dof, offsets, slen, stride, line, first, count):
    """uint8 per element of the tile of a call over plans [first, first + count), GUARD elements either side: 0 = not written,
    1 = a sample, 2 = the zeros that finish a row's last line."""
    off0 = int(offsets[first])
    total = int(offsets[first + count]) - off0
    cls = np.zeros(GUARD + total + GUARD, dtype=np.uint8)
    for p in range(first, first + count):
        if slen[p] <= 0:
            continue
        at = GUARD + int(offsets[p]) - off0
        rows = cls[at: at + 4 * dof * stride[p]].reshape(4 * dof, stride[p])
        rows[:, :slen[p]] = 1
        rows[:, slen[p]:line[p]] = 2
    return total, cls


def _bits(t):
    import torch
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _sample(ltp, b, first, count, total, dtype, fill, how):
    import torch
    big = torch.full((GUARD + total + GUARD,), fill, dtype=dtype, device="cuda")
    ltp.sampleBatch(b, first, count, big[GUARD: GUARD + total], **how)
    return big


def _check(got, ref, cls, what):
    """got: the call into a tile of FILL; ref: the same call into a tile of zeros; cls: _classes on the device"""
    import torch
    fill = _bits(torch.full((1,), FILL, dtype=got.dtype, device="cuda"))
    want = torch.where(cls == 1, _bits(ref), torch.where(cls == 2, torch.zeros_like(fill), fill))
    bad = torch.nonzero(_bits(got) != want)
    if bad.numel():
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} elements differ, first at tile element {i - GUARD} (class {int(cls[i])}): "
                             f"{float(got[i])!r}, in the zeroed tile {float(ref[i])!r}")


WRITERS = {"fused": dict(tables=False, walk=False), "table": dict(tables=True, walk=False), "walk": dict(walk=True, auto_waves=False),
           "auto": dict(walk=True)}


def _kernel_is(writer, name):
    return {"fused": name == "k_sample", "table": name.startswith("k_sample_tab_"),
            "walk": name.startswith("k_sample_walk_") and "auto" not in name, "auto": "_walk_auto_" in name or "_walk_matlab_auto_" in name}[writer]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("cap,stride", FORMATS)
def test_rows_end_on_a_line_and_nothing_else_is_written(amd, planned, cap, stride, f32):
    import torch
    dof, ltp, dev, _ = planned
    dtype, esize = (torch.float32, 4) if f32 else (torch.float64, 8)
    ltp.setMaxSamples(cap); ltp.setSampleStride(stride)
    try:
        b = ltp.planSwitchTimesBatch(*dev)
        torch.cuda.synchronize()
        traj_len = b.traj_len.cpu().numpy()
        offsets = b.offsets.cpu().numpy().astype(np.int64)
        slen, rstride, line = _geometry(ltp, traj_len, esize)
        assert traj_len[REJECTED] == 0 and (traj_len > 0).sum() >= N_PLANS * 3 // 4
        assert np.array_equal(np.diff(offsets), 4 * dof * rstride)
        assert np.all(line >= slen) and np.all(line <= rstride)
        per_line = 64 // esize
        if cap == 0:
            # rows that end at every place of a line
            assert set(slen[slen > 0] % per_line) == set(range(per_line)), sorted(set(slen[slen > 0] % per_line))
        elif cap == 64:
            assert np.all(line[slen == 64] == 64) and (slen == 64).sum() > N_PLANS // 2
        else:
            assert (slen == cap).sum() > N_PLANS // 2 and np.all(line[slen == cap] == -(-cap // per_line) * per_line)
        writers = ["fused", "table", "walk"] + (["auto"] if 0 < cap <= 32 else [])
        sub_first, sub_count = 40, N_PLANS - 43
        full = _classes(dof, offsets, slen, rstride, line, 0, N_PLANS)
        sub = _classes(dof, offsets, slen, rstride, line, sub_first, sub_count)
        full_cls, sub_cls = torch.from_numpy(full[1]).cuda(), torch.from_numpy(sub[1]).cuda()
        assert int((full_cls == 2).sum()) > 0 or cap == 64
        first_ref = None
        for w in writers:
            how = WRITERS[w]
            ref = _sample(ltp, b, 0, N_PLANS, full[0], dtype, 0.0, how)
            assert _kernel_is(w, ltp.lastSamplerKernel()), (w, ltp.lastSamplerKernel())
            got = _sample(ltp, b, 0, N_PLANS, full[0], dtype, FILL, how)
            sref = _sample(ltp, b, sub_first, sub_count, sub[0], dtype, 0.0, how)
            sgot = _sample(ltp, b, sub_first, sub_count, sub[0], dtype, FILL, how)
            torch.cuda.synchronize()
            _check(got, ref, full_cls, (w, "whole range"))
            _check(sgot, sref, sub_cls, (w, "sub-range"))
            # the samples themselves: every writer stores the same bits, and they are trajectories (q starts at q_0 + ..., not zeros)
            if first_ref is None:
                first_ref = ref
                assert int((_bits(ref)[full_cls == 1] != 0).sum()) > int((full_cls == 1).sum()) // 8      # (q alone is a quarter)
            else:
                assert torch.equal(_bits(ref), _bits(first_ref)), (w, "differs from", writers[0])
    finally:
        ltp.setMaxSamples(0); ltp.setSampleStride(1)


@pytest.mark.parametrize("cap,stride", FORMATS)
def test_small_single_call_path_finishes_the_line_too(amd, planned, cap, stride):
    """n * dof <= 128: one launch of k_plan_small writes the rows (stream_rows, the fused build's writer) into pinned host memory.
    Samples as the batched fused sampler stores them, zeros from the last sample to the end of the row's line (and, as ever on this
    path, to the end of the row: the packed host buffer is deterministic)."""
    import torch
    dof, ltp, dev, host = planned
    n = 128 // dof
    assert REJECTED < n
    ltp.setMaxSamples(cap); ltp.setSampleStride(stride)
    try:
        r = ltp.planBatchHost(*[x[:n] for x in host], sample=True)
        b = ltp.planSwitchTimesBatch(*dev)
        tile = torch.full((int(b.offsets[n].item()),), FILL, dtype=torch.float64, device="cuda")
        ltp.sampleBatch(b, 0, n, tile, tables=False, walk=False)
        torch.cuda.synchronize()
        tile = tile.cpu().numpy()
        traj_len = b.traj_len.cpu().numpy()[:n]
        offsets = b.offsets.cpu().numpy().astype(np.int64)[:n + 1]
        assert np.array_equal(r["traj_len"], traj_len) and np.array_equal(r["offsets"].astype(np.int64), offsets)
        slen, rstride, line = _geometry(ltp, traj_len, 8)
        assert traj_len[REJECTED] == 0 and (slen > 0).sum() >= n // 2
        packed = np.asarray(r["packed"])
        for p in range(n):
            if slen[p] <= 0:
                continue
            at = int(offsets[p])
            rows = packed[at: at + 4 * dof * rstride[p]].reshape(4 * dof, rstride[p])
            want = tile[at: at + 4 * dof * rstride[p]].reshape(4 * dof, rstride[p])
            assert np.array_equal(rows[:, :slen[p]].view(np.int64), want[:, :slen[p]].view(np.int64)), p
            assert not rows[:, slen[p]:].view(np.int64).any(), p                  # +0.0, bit for bit
            assert not want[:, slen[p]:line[p]].view(np.int64).any() and np.all(want[:, line[p]:] == FILL), p
    finally:
        ltp.setMaxSamples(0); ltp.setSampleStride(1)
