"""SURVEY.md §8(e) on the hardware a single-GPU box has: one batch cut into k virtual shards on device 0 must give the bits
of the unsharded run — through the one-process C ABI overload (ltp_plan_batch_multi, one handle + host thread per shard),
through the C++ class (planTrajectoryBatchSharded, tests/cpp/dropin_tests.cc) and through bench.py's one-process-per-rank
path (self-spawned ranks, gloo for the barrier, every rank on device 0)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("limits,n,k", [("panda", 1001, 3), ("ref", 777, 2), ("ref30", 130, 4), ("ref", 3, 5)])
def test_virtual_shards_are_bit_identical_to_the_unsharded_batch(limits, n, k):
    import longtermplanner_amd as amd
    D, lim = amd.limit_set(limits)
    one = amd.LongTermPlanner(D, 0.002, device=0, **lim)
    shards = [amd.LongTermPlanner(D, 0.002, device=0, **lim) for _ in range(k)]
    qg, q0, v0, a0 = amd.generate_queries(n, lim, seed=31)
    if n > 100:
        q0[17, 0] = 99.0                                       # a rejected query inside a shard
    want = one.planBatchHost(qg, q0, v0, a0, sample=True)
    got = amd.LongTermPlanner.planBatchSharded(shards, qg, q0, v0, a0, sample=True)
    for key in want:
        assert want[key].tobytes() == got[key].tobytes(), key
    assert want["packed"].size > 0
    # switching times only: same records, status includes the end-limit verdict, nothing sampled
    got0 = amd.LongTermPlanner.planBatchSharded(shards, qg, q0, v0, a0, sample=False)
    for key in got0:
        assert want[key].tobytes() == got0[key].tobytes(), key
    # shards must be configured alike
    shards[-1].setSampleTime(0.004)
    with pytest.raises(amd.LtpError):
        amd.LongTermPlanner.planBatchSharded(shards, qg, q0, v0, a0)


@pytest.mark.parametrize("limits,n,k,layout", [("panda", 20011, 3, "query_major"), ("ref", 5003, 8, "joint_major"), ("ref30", 1300, 4, "query_major"),
                                               ("ref", 3, 5, "query_major")])
def test_device_resident_shards_match_the_unsharded_calls(limits, n, k, layout):
    """ltp_plan_switch_times_multi / ltp_envelope_multi / ltp_state_at_multi (k handles, one host thread and stream per shard,
    shard-local device arrays, nothing through the host): every shard's records, envelopes and restart states must have the
    bits of the corresponding rows of ONE unsharded call over the whole batch."""
    import torch
    import longtermplanner_amd as amd
    from longtermplanner_amd.parallel import shard_range
    D, lim = amd.limit_set(limits)
    Ts = 0.002
    one = amd.LongTermPlanner(D, Ts, device=0, **lim)
    planners = [amd.LongTermPlanner(D, Ts, device=0, **lim) for _ in range(k)]
    streams = [torch.cuda.Stream() for _ in range(k)]
    whole = one.generateQueries(n, seed=77, layout="query_major")
    if n > 100:
        whole[1][n // 2, 0] = 99.0                                # a rejected query inside a shard
    torch.cuda.synchronize()
    shard_in = []
    for g in range(k):
        f, c = shard_range(n, g, k)
        part = [x[f:f + c] for x in whole]
        shard_in.append([p.t().contiguous() if layout == "joint_major" else p.contiguous() for p in part])
    W, K = 40, 12
    want = one.planSwitchTimesBatch(*whole)
    want_env = one.envelopeBatch(want, 0, n, W, K)                # sets END_LIMIT bits like the sharded call below
    idx = torch.arange(n, dtype=torch.int32, device="cuda") % 700
    want_state = one.stateAt(want, 0, n, idx)
    want_state_u = one.stateAt(want, 0, n, 150)
    torch.cuda.synchronize()
    got = amd.LongTermPlanner.planSwitchTimesSharded(planners, shard_in, n, layout=layout, streams=streams)
    got_env = amd.LongTermPlanner.envelopeSharded(planners, got, n, W, K, streams=streams)
    per_idx = [idx[shard_range(n, g, k)[0]:sum(shard_range(n, g, k))].contiguous() for g in range(k)]
    got_state = amd.LongTermPlanner.stateAtSharded(planners, got, n, per_idx, streams=streams)
    got_state_u = amd.LongTermPlanner.stateAtSharded(planners, got, n, 150, streams=streams)
    amd.LongTermPlanner.synchronizeSharded(planners, got, streams)
    for g in range(k):
        f, c = shard_range(n, g, k)
        assert got[g].n == c
        for key in ("t_opt", "t_scaled", "dir", "v_drive", "mod", "t_required", "slowest", "traj_len", "status"):
            a, b = getattr(got[g], key), getattr(want, key)[f:f + c]
            assert torch.equal(a.view(torch.uint8), b.contiguous().view(torch.uint8)), (g, key)
        lo = want.offsets[f:f + c + 1] - want.offsets[f]
        assert torch.equal(got[g].offsets, lo), g
        assert torch.equal(got_env[g].view(torch.int64), want_env[f:f + c].contiguous().view(torch.int64)), g      # NaN rows included
        for x in range(3):
            for gs, ws in ((got_state, want_state), (got_state_u, want_state_u)):
                a = gs[g][x].t() if layout == "joint_major" else gs[g][x]
                assert torch.equal(a.contiguous().view(torch.int64), ws[x][f:f + c].contiguous().view(torch.int64)), (g, x)
    # the end-limit verdict without rows or envelopes: planTrajectory's bool per shard
    got2 = amd.LongTermPlanner.planSwitchTimesSharded(planners, shard_in, n, layout=layout, end_limit=True, streams=streams)
    amd.LongTermPlanner.synchronizeSharded(planners, got2, streams)
    assert torch.equal(torch.cat([b.status for b in got2]), want.status)
    # the host-pointer form of the envelope call (what the C++ planEnvelopeBatchSharded uses)
    host = [x.cpu().numpy() for x in whole]
    r1, e1 = one.planEnvelopeHost(*host, W, K)
    rk, ek = amd.LongTermPlanner.planEnvelopeSharded(planners, *host, W, K)
    assert e1.tobytes() == ek.tobytes() and e1.tobytes() == want_env.cpu().numpy().tobytes()
    for key in r1:
        assert r1[key].tobytes() == rk[key].tobytes(), key
    # shards must be configured alike, and a handle may appear only once
    planners[-1].setSampleTime(0.004)
    with pytest.raises(amd.LtpError):
        amd.LongTermPlanner.planSwitchTimesSharded(planners, shard_in, n, layout=layout, streams=streams)
    planners[-1].setSampleTime(Ts)
    if k > 1:
        with pytest.raises(amd.LtpError):
            amd.LongTermPlanner.planSwitchTimesSharded([planners[0]] * k, shard_in, n, layout=layout, streams=streams)


def test_config4_ten_million_queries_in_eight_shards(oracle_mod):
    """BASELINE.json configs[3] at its real size on the hardware at hand: 10 M x 7-DoF queries cut 8 ways. A GPU box allows six
    processes on its card, so the 8-way cut runs as eight device-resident shards of ONE process (bench.py --one-process:
    eight handles, streams and host threads on device 0) and the one-process-per-rank path as four gloo ranks sharing the
    device, with full sampling (3.86 TB of rows). All of them must agree with the unsharded batch in an order-independent
    checksum of every record, the ok-count and the bytes; the queries either side of every shard boundary are checked
    against the oracle."""
    import torch
    import longtermplanner_amd as amd
    from longtermplanner_amd.parallel import shard_range
    G = 10_000_000
    keys = ("records_checksum", "plans_ok_frac", "mean_traj_len", "bytes_per_plan")

    def line(*args, tile="8"):
        env = dict(os.environ)
        for kk in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(kk, None)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--no-cpu-baseline", "--no-secondary", "--steps", "1", "--warmup", "0",
                            "--tile-gib", tile, "--global-batch", str(G), "--checksum", *args], capture_output=True, text=True, timeout=900, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        out = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, p.stdout
        return json.loads(out[0])

    one = line("--gpus", "1", "--switch-only", "--end-limit")
    eight = line("--gpus", "8", "--one-process", "--device", "0", "--switch-only", "--end-limit")
    # (n_gpus counts DISTINCT devices — all eight shards sit on device 0 here — and n_shards the shards)
    assert eight["n_gpus"] == 1 and eight["n_shards"] == 8 and eight["scaling"] == "strong" and eight["config"]["global_batch"] == G
    assert one["n_gpus"] == 1 and one["config"]["global_batch"] == G
    for key in keys:
        assert eight["config"][key] == one["config"][key], key
    # four ranks (processes) sharing the device, every trajectory sampled: the status words now come from the sampler's
    # end-limit check and must still add up to the same checksum
    four = line("--gpus", "4", "--backend", "gloo", "--device", "0", tile="96")
    assert four["n_gpus"] == 4 and four["scaling"] == "strong"
    assert four["roofline"]["kernel"] == "k_sample" and four["config"]["plans_ok_is"] == "planTrajectory's bool"
    for key in keys:
        assert four["config"][key] == one["config"][key], key
    assert abs(four["config"]["bytes_per_plan"] - 385_800) < 2_000      # 384 938 B per panda plan
    torch.cuda.empty_cache()

    # shard boundaries against the oracle: eight device-resident shards, the three queries either side of every `first`
    D, lim = amd.limit_set("panda")
    planners = [amd.LongTermPlanner(D, 0.001, device=0, **lim) for _ in range(8)]
    ins = []
    for g in range(8):
        f, c = shard_range(G, g, 8)
        assert c == 1_250_000 and f == g * 1_250_000
        ins.append(planners[g].generateQueries(c, seed=12345, first_query=f))
    got = amd.LongTermPlanner.planSwitchTimesSharded(planners, ins, G, end_limit=True)
    amd.LongTermPlanner.synchronizeSharded(planners, got)
    orc = oracle_mod.Oracle(D, 0.001, **lim)
    for g in range(8):
        f, c = shard_range(G, g, 8)
        for lo, cnt in ((0, 3), (c - 3, 3), (c // 2, 2)):
            host = amd.generate_queries(cnt, lim, seed=12345, first_query=f + lo)
            for x, y in zip(host, ins[g]):
                assert np.array_equal(x, y[lo:lo + cnt].cpu().numpy()), "device generator == host generator at 10 M-scale indices"
            o = orc.plan_batch(*host, sample=True)
            sl = slice(lo, lo + cnt)
            assert np.array_equal(got[g].traj_len[sl].cpu().numpy(), o["traj_len"])
            assert np.array_equal(got[g].slowest[sl].cpu().numpy(), o["slowest"])
            assert np.array_equal(got[g].mod[sl].cpu().numpy(), o["mod"])
            assert np.array_equal(got[g].dir[sl].cpu().numpy(), o["dir"])
            assert np.array_equal(got[g].status[sl].cpu().numpy() == 0, o["status"] == 1)      # planTrajectory's bool
            for key in ("t_opt", "t_scaled", "v_drive", "t_required"):
                assert np.max(np.abs(getattr(got[g], key)[sl].cpu().numpy() - o[key])) <= 1e-9, (g, key)


def _bench(*args):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--no-cpu-baseline", "--no-secondary", "--steps", "1", "--warmup", "1",
                        "--tile-gib", "8", *args], capture_output=True, text=True, timeout=600, env=env)
    return p


def test_bench_spawns_its_ranks_and_shards_one_global_batch():
    """`python bench.py --gpus 2` run plainly starts two rank processes (never an n_gpus: 1 line), and one global batch cut
    into 1, 2 and 3 contiguous shards has the same record checksum, ok-count and bytes."""
    lines = {}
    for world in (1, 2, 3):
        p = _bench("--gpus", str(world), "--backend", "gloo", "--device", "0", "--global-batch", "30001", "--limits", "ref", "--checksum")
        assert p.returncode == 0, p.stderr[-2000:]
        out = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, p.stdout
        lines[world] = json.loads(out[0])
        assert lines[world]["n_gpus"] == world and lines[world]["scaling"] == "strong"
        assert lines[world]["config"]["global_batch"] == 30001
    for world in (2, 3):
        for key in ("records_checksum", "plans_ok_frac", "mean_traj_len", "bytes_per_plan"):
            assert lines[world]["config"][key] == lines[1]["config"][key], (world, key)
    # weak scaling (the default): N ranks x --batch queries
    p = _bench("--gpus", "2", "--backend", "gloo", "--device", "0", "--batch", "20000")
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["config"]["global_batch"] == 40000
    assert line["config"]["backend"].startswith("gloo") and line["config"]["rank_devices"] == [0, 0]


def test_two_rank_bench_line_is_complete():
    """An N > 1 line carries everything the N = 1 line does: roofline (HIP events of rank 0), cpu_baseline (rank 0, after the timed
    steps), the backend that carried the barrier and the device of every rank — so that the first 8-GPU run yields a complete record."""
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--device", "0", "--batch", "40000",
                        "--steps", "2", "--warmup", "1", "--tile-gib", "16", "--full", "--no-secondary"], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    out = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(out) == 1, p.stdout
    line = json.loads(out[0])
    assert line["n_gpus"] == 2 and line["config"]["backend"].startswith("gloo") and line["config"]["rank_devices"] == [0, 0]
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and r["unit"] == "GB/s" and 0.0 < r["frac"] < 1.0 and r["kernel"] == "k_sample"
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and "traffic" in r
    c = line["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "plans/s" and c["value"] > 0 and 1 <= c["cores"] <= 32 and "rank 0 of 2" in c["measured_on"]
    assert c["cores"] <= c["host_cores_affinity"] and "sample" in c


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _check_nccl_line(line):
    c = line["config"]
    assert line["n_gpus"] == 1 and c["backend"].startswith("nccl") and "world size 1" in c["backend"] and c["rank_devices"] == [0]
    assert "all_gather of t_required" in c["sharding"]
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["kernel"] == "k_sample" and 0.0 < r["frac"] < 1.0 and r["launches_timed"] >= 2
    assert line["value"] > 0 and line["steps"] == 2 and c["plans_ok_frac"] > 0.99


def test_nccl_branch_runs_at_world_size_one():
    """everything bench.py does with torch.distributed when N > 1 — init_process_group("nccl", device_id=...),
    the all_gather of the rank devices, barrier, all_reduce(MAX) of the elapsed time, all_reduce(SUM) of the counters and of the
    checksum, the optional --gather of t_required, all on DEVICE tensors — runs over RCCL at world size 1, and the line it prints
    has the numbers of the run without a process group."""
    args = ("--batch", "40000", "--steps", "2", "--tile-gib", "16", "--checksum")
    p = _bench("--gpus", "1", "--force-dist", "--backend", "nccl", "--gather", *args)
    assert p.returncode == 0, p.stderr[-3000:]
    out = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(out) == 1, p.stdout
    line = json.loads(out[0])
    _check_nccl_line(line)
    q = _bench("--gpus", "1", *args)
    assert q.returncode == 0, q.stderr[-3000:]
    plain = json.loads([ln for ln in q.stdout.splitlines() if ln.startswith("{")][0])
    assert plain["config"]["backend"].startswith("none")
    for key in ("records_checksum", "plans_ok_frac", "mean_traj_len", "bytes_per_plan", "global_batch"):
        assert line["config"][key] == plain["config"][key], key


def test_nccl_branch_under_torch_distributed_run():
    """The driver's own launch line for N > 1, with one rank: `python -m torch.distributed.run --nnodes=1 --nproc-per-node 1
    --master-addr 127.0.0.1 --master-port P bench.py --gpus 1 ...`. WORLD_SIZE is in the environment, so the rank creates its
    RCCL process group; the line must be complete, cpu_baseline included (rank 0 runs it while the group is alive)."""
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "40000", "--steps", "2",
                        "--warmup", "1", "--tile-gib", "16", "--full", "--no-secondary", "--gather", "--checksum"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    out = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(out) == 1, p.stdout
    line = json.loads(out[0])
    _check_nccl_line(line)
    c = line["cpu_baseline"]
    assert c["kind"] == "port" and c["value"] > 0 and c["cores"] >= 1


def test_two_batches_in_flight_give_the_same_records():
    """`bench.py --switch-only --in-flight 2` alternates its steps between two handles on two streams (the queue-B kernel of
    one step runs under the next step's stages): the records are those of one batch at a time."""
    sums = {}
    for k in (1, 2, 3):
        p = _bench("--switch-only", "--batch", "30001", "--limits", "ref", "--checksum", "--in-flight", str(k), "--steps", "5", "--end-limit")
        assert p.returncode == 0, p.stderr[-2000:]
        line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
        assert line["config"]["batches_in_flight"] == k and line["steps"] == 5
        sums[k] = (line["config"]["records_checksum"], line["config"]["plans_ok_frac"], line["config"]["mean_traj_len"])
    assert sums[2] == sums[1] and sums[3] == sums[1]
    p = _bench("--in-flight", "2")                        # only the switching-times workload can be interleaved like this
    assert p.returncode != 0


def test_bench_never_reports_fewer_gpus_than_requested():
    # a launcher that started a different number of ranks: refuse (exit code, no JSON line)
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "1"], capture_output=True, text=True,
                       timeout=300, env=env)
    assert p.returncode != 0 and "{" not in p.stdout
    # more ranks than devices, nccl: every rank needs its own GPU -> non-zero exit, no line
    import torch
    if torch.cuda.device_count() >= 2:
        return
    p = _bench("--gpus", "2", "--batch", "1000")
    assert p.returncode != 0 and not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


def test_default_bench_line_says_what_bounds_every_line(tmp_path):
    """stdout of the driver's command (`python bench.py`, here with --steps 1) is ONE line under 4 KB — the headline with
    `roofline` and `cpu_baseline` — and the secondary workloads' full records are in --secondary-file, one JSON line each.
    VERDICT r4 item 4: headline AND every secondary entry carry a
    roofline block that names the bound that applies to THAT workload: `hbm` with a kernel, algorithmic GB/s and a fraction of 8 TB/s for the
    row writers; `valu_f64` for the envelope consumer (flop rate against the binary64 vector peak, the committed issue-slot share beside it);
    `latency/valu_f64` without a fraction for the switching-times lines, quoting the committed PMC figures (profiles/bench_counters.json,
    with provenance) where the workload has them. And `rccl_world1`: the nccl branch ran at world size 1 in a child process."""
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    sec_file = str(tmp_path / "bench_secondary.jsonl")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "1", "--warmup", "1", "--secondary-file", sec_file],
                       capture_output=True, text=True, timeout=1200, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    out = p.stdout.splitlines()
    assert len(out) == 1 and out[0].startswith("{") and len(out[0]) < 4096, (len(out), len(out[-1]), p.stdout[-2000:])
    line = json.loads(out[0])
    side = [json.loads(x) for x in open(sec_file).read().splitlines()]
    assert line["secondary"]["count"] == len([x for x in side if x["kind"] == "secondary"]) and line["secondary"]["file"] == sec_file
    assert len([n for n in p.stderr.splitlines() if n.startswith("bench.py secondary: ")]) == line["secondary"]["count"]
    assert line["n_gpus"] == 1 and line["config"]["pow_rule"] == "libm" and line["config"]["workload_key"] == "panda:1000000:f64"
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["kernel"] == "k_sample" and 0.5 < r["frac"] < 1.0 and r["traffic"] is None
    assert r["traffic_from_profile"]["write_bytes_per_launch"] > 1.9e11 and "NOT measured in this run" in r["traffic_from_profile"]["source"]
    w1 = line["rccl_world1"]
    assert w1["ok"] and w1["backend"].startswith("nccl") and w1["rank_devices"] == [0]
    assert [x for x in side if x["kind"] == "rccl_world1"][0]["records_checksum"] > 0
    assert line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["cores"] >= 1
    sec = [x for x in side if x["kind"] == "secondary"]
    assert len(sec) >= 16 and not [s_ for s_ in sec if "error" in s_], [s_.get("error") for s_ in sec]
    bounds = {"hbm": 0, "valu_f64": 0, "latency/valu_f64": 0}
    for s_ in sec:
        rr = s_["roofline"]
        bounds[rr["bound"]] += 1
        key = s_["config"]["workload_key"]
        if rr["bound"] == "hbm":
            assert rr["unit"] == "GB/s" and rr["peak"] == 8000.0 and 0.0 < rr["frac"] < 1.0 and rr["kernel"].startswith("k_sample"), (key, rr)
            assert abs(rr["frac"] - rr["achieved"] / rr["peak"]) < 1e-3
        elif rr["bound"] == "valu_f64":
            assert rr["unit"] == "TFLOP/s" and rr["peak"] == 78.6 and "envelope" in key and "k_envelope" in rr["kernel"], (key, rr)
            if "analytic" not in key:
                assert 0.0 < rr["frac"] < 0.5 and 0.5 < rr["issue_slots_used_frac_from_profile"] <= 1.0, rr
        else:
            assert rr["frac"] is None and rr["achieved"] is None and "switch_only" in key, (key, rr)
            if key in ("panda:100000:f64:switch_only", "panda:1000000:f64:switch_only", "panda:100000:f64:switch_only:pow_exact"):
                assert 0.0 < rr["valu_issue_frac"] < 1.0 and "NOT measured in this run" in rr["counters_from_profile"]["source"], (key, rr)
    assert bounds["hbm"] >= 6 and bounds["valu_f64"] == 2 and bounds["latency/valu_f64"] >= 8, bounds
    walk = [s_ for s_ in sec if s_["config"]["workload_key"] in ("panda:1000000:f64:first256", "panda:1000000:f64:stride4", "panda:1000000:f32")]
    assert len(walk) == 3 and all(w["roofline"]["traffic_from_profile"]["write_bytes_per_launch"] > 0 for w in walk)


def test_plain_bench_line_and_dumped_outputs(tmp_path, oracle_mod):
    """A plain run (no --full) times the headline only — no cpu_baseline, rccl_world1 or secondary workloads — with exactly --steps
    timed steps. --dump-outputs writes what the last step computed: two runs with the same arguments write the same arrays, and the
    sampled records and rows are the oracle's (1e-9, as smoke())."""
    import numpy as np
    from longtermplanner_amd import LongTermPlanner, limit_set
    lines, dumps = [], []
    for r in range(2):
        d = str(tmp_path / f"run{r}")
        p = _bench("--batch", "40000", "--steps", "3", "--dump-outputs", d)
        assert p.returncode == 0, p.stderr[-3000:]
        out = p.stdout.splitlines()
        assert len(out) == 1 and out[0].startswith("{"), p.stdout[-2000:]
        lines.append(json.loads(out[0]))
        dumps.append({f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))})
    line = lines[0]
    for k in ("cpu_baseline", "rccl_world1", "secondary"):
        assert k not in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["roofline"]["launches_timed"] % 3 == 0
    assert abs(line["value"] - 40000 / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3
    a, b = dumps
    assert sorted(a) == sorted(b) and {"plan_index", "t_opt", "t_scaled", "traj_len", "status", "offsets", "rows_qvaj", "rows_len", "rows_plan_index"} <= set(a)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and a[k].tobytes() == b[k].tobytes(), k
    assert sum(x.nbytes for x in a.values()) <= 64 << 20 and len(a["plan_index"]) == 16384 and a["rows_qvaj"].shape[:2] == (4, 7)
    assert a["rows_qvaj"].shape[2] == a["rows_len"].sum() and len(a["rows_plan_index"]) > 0
    dof, lim = limit_set("panda")
    orc = oracle_mod.Oracle(dof, 0.001, **lim)
    ltp = LongTermPlanner(dof, 0.001, device=0, **lim)
    queries = [x.cpu().numpy() for x in ltp.generateQueries(40000, seed=12345)]      # the batch bench.py planned (--seed default)
    pi = a["plan_index"].astype(np.int64)
    for i in (0, len(pi) // 2, len(pi) - 1):
        qg, q0, v0, a0 = (x[pi[i]:pi[i] + 1] for x in queries)
        o = orc.plan_batch(qg, q0, v0, a0, sample=False)
        assert a["traj_len"][i] == o["traj_len"][0] and np.max(np.abs(a["t_scaled"][i] - o["t_scaled"][0])) < 1e-9
    starts = np.concatenate([[0], np.cumsum(a["rows_len"])]).astype(np.int64)
    for i in (0, len(a["rows_len"]) - 1):
        p_ = int(a["rows_plan_index"][i])
        qg, q0, v0, a0 = (x[p_:p_ + 1] for x in queries)
        o = orc.plan_batch(qg, q0, v0, a0, sample=False)
        n, q, v, acc, j = orc.get_trajectory(o["t_scaled"][0], o["dir"][0], o["mod"][0], q0[0], v0[0], a0[0], o["v_drive"][0])
        assert n == a["rows_len"][i]
        got = a["rows_qvaj"][:, :, starts[i]:starts[i + 1]]
        assert max(np.max(np.abs(got[0] - q)), np.max(np.abs(got[1] - v)), np.max(np.abs(got[2] - acc)), np.max(np.abs(got[3] - j))) < 1e-9
