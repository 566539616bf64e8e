"""What the device-free tests of the two horizon-envelope calls share (tests/test_envelope_knots_cpu.py, tests/test_envelope_arrays_cpu.py)
— a helper, not a test, and nothing here needs a device: the built library, the oracle's plans in the full-row layout, the checks of
a call's three C entries against the header, the g++ lines of the drop-in and rule programs, and the plain loop that pins
tests/envelope_checker.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import envelope_checker as ec
from horizon_checker import TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


@pytest.fixture(scope="module")
def abi():
    from longtermplanner_amd import _abi
    _abi.build()
    return _abi


def header(comments=True):
    text = open(os.path.join(ROOT, "include", "ltp_hip.h")).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def assert_declared_and_exported(abi, names):
    """Each entry is declared in the header, bound in _abi._SIGNATURES and exported by the library."""
    text = header(comments=False)
    lib = C.CDLL(abi.LIB_PATH)
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} is not declared in include/ltp_hip.h"
        assert n in abi.exported_symbols(), f"{n} is not declared in _abi._SIGNATURES"
        assert hasattr(lib, n), f"{n} is not exported"


def assert_opts_is_the_c_struct(abi, names, c_name, O, fields):
    """The header's struct c_name and _abi's O hold `fields` in this order; the header's prototypes of `names` and _abi's agree in
    the number of arguments."""
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % c_name, header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == [f[0] for f in O._fields_] == fields
    text = header(comments=False)
    for n in names:
        args = re.search(r"\b%s\s*\(([^;]*)\);" % n, text, flags=re.S).group(1)
        assert len(args.split(",")) == len(abi._SIGNATURES[n][1]), n


def compile_dropin(tmp_path, name, source):
    """`source` — a program on the drop-in header — under plain g++ -Wall -Werror against the library."""
    src, exe = tmp_path / (name + ".cc"), tmp_path / name
    src.write_text(source)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "longtermplanner_amd"), "-lltp_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "longtermplanner_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def run_rule_program(tmp_path, name, flags):
    """tests/cpp/<name>.cc — a stand-alone host program on a header of longtermplanner_amd/csrc — compiled with `flags` and run:
    it ends with OK."""
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "longtermplanner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", name + ".cc"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]


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
    full, offsets, lens = ec.pack_full_rows(trajs, dof)
    assert np.mean(lens > 0) > 0.9
    return dof, trajs, full, offsets, lens


def plain_loop(oracle_plans, grid, closed, mask):
    """The checker's gather, the rule past the end, the per-interval reduction of the arrays of `mask` and `valid` are what a loop
    over (plan, array, joint, w, t) reads from the oracle's own trajectories: starts below 0, inside and at or past the end. q holds
    the loop's bytes; v, a and j its values under == (where an interval holds both zeros, which one a minimum keeps is not part of
    the rule), {0, 0} from the end on and 0 inside an interval that reaches past it. Returns (env [count, A, dof, M, 2] as numpy,
    valid, planned, the checker's arguments (full, offsets, lens, k, g, closed, dof, first, count) as tensors, and the numbers of
    (plan, interval) pairs that start at or past the end, end there, and hold one sample)."""
    import torch
    dof, trajs, full, offsets, lens = oracle_plans
    g = ec.GRIDS[grid]
    M = len(g) - 1
    n = len(trajs)
    rng = np.random.default_rng(31 + closed)
    k = rng.integers(-5, lens.astype(np.int64) + 41).astype(np.int32)
    k[0::9] = -3
    k[1::9] = lens[1::9]
    k[2::9] = lens[2::9] - 1
    assert np.any(k < 0) and np.any(k >= lens) and np.any((k > 0) & (k < lens))
    first, count = 3, n - 5
    args = (*[torch.from_numpy(x) for x in (full, offsets, lens, k[first:first + count])], g, closed, dof, first, count)
    env, valid, planned = ec.expected(*args, mask=mask, chunk=16)
    env = env.numpy()
    arrays = ec.selected(mask)
    assert env.shape == (count, len(arrays), dof, M, 2)
    held = ended_in = singles = 0
    for i in range(count):
        L = trajs[first + i][0]
        assert bool(planned[i]) == (L > 0)
        if L == 0:
            assert int(valid[i]) == 0 and np.isnan(env[i]).all()
            continue
        k0 = max(int(k[first + i]), 0)
        n_real = 0
        for w in range(M):
            a = k0 + int(g[w])
            b = max(a, k0 + int(g[w + 1]) - 1 + closed)
            n_real += a < L
            held += a >= L
            ended_in += a < L <= b
            singles += a == b
            for x, arr in enumerate(arrays):
                rows = trajs[first + i][1 + arr]
                for j in range(dof):
                    lo, hi = env[i, x, j, w]
                    if arr == 0:
                        samples = [rows[j][min(t, L - 1)] for t in range(a, b + 1)]
                        assert lo.tobytes() == np.float64(min(samples)).tobytes() and hi.tobytes() == np.float64(max(samples)).tobytes(), (i, j, w)
                        continue
                    samples = [rows[j][t] if t < L else 0.0 for t in range(a, b + 1)]
                    assert lo == min(samples) and hi == max(samples), (i, arr, j, w)
                    if a >= L:
                        assert lo == 0.0 and hi == 0.0
                    elif L <= b:
                        assert lo <= 0.0 <= hi
        assert int(valid[i]) == n_real
    return env, valid, planned, args, (held, ended_in, singles)
