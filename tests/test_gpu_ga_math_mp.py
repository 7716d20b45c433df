"""GPU, GA layer: GA_Fill / GA_Scale / GA_Add / GA_Copy / GA_?dot, their patch forms,
the general path and the aborts, on 1, 2 and 3 ranks sharing one GPU
(tests/ga_math_worker.py is one rank).  Expected values: the numpy restatement in
test_gpu_ga_math.py, compared as raw bits.

Every rank process runs under its own time limit (a watcher thread each); once a
launch ends in anything but the outcome its test expects, the remaining tests of this
file start nothing."""
import os
import socket
import subprocess
import sys
import threading

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORKER = os.path.join(HERE, "ga_math_worker.py")

_broken = []


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(mode, n, limit=90, extra_env=None):
    """[(exit status, output)] of the n ranks"""
    if _broken:
        pytest.fail(f"not started: an earlier launch of this file went wrong ({_broken[0]})")
    port = str(free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(n), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=port, COMEX_AMD_JOBID=f"m{port}", COMEX_AMD_STAGING_MB="16",
                   TEST_STACK_DUMP_S=str(limit - 15))
        env.update(extra_env or {})
        # the ranks are this process's own children: the node rendezvous is named after the
        # parent's pid, so a wrapper process per rank would keep them from meeting
        procs.append(subprocess.Popen([sys.executable, WORKER, mode], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    res = [None] * n

    def watch(r, p):   # each rank ends by itself or is killed at its own time limit
        try:
            out, _ = p.communicate(timeout=limit)
            res[r] = (p.returncode, out)
        except subprocess.TimeoutExpired:
            p.kill()
            out, _ = p.communicate()
            res[r] = (124, out + f"\n[killed after {limit} s]")

    watchers = [threading.Thread(target=watch, args=(r, p)) for r, p in enumerate(procs)]
    for t in watchers:
        t.start()
    for t in watchers:
        t.join()
    return res


def tails(res):
    return "\n".join(f"--- rank {r}: status {rc} ---\n{out[-2500:]}" for r, (rc, out) in enumerate(res))


def launch_ok(mode, n, **kw):
    res = launch(mode, n, **kw)
    for r, (rc, out) in enumerate(res):
        if rc != 0 or f"RANK {r} OK" not in out:
            _broken.append(f"{mode} on {n} ranks: rank {r} status {rc}")
            pytest.fail(f"rank {r} rc={rc}\n{tails(res)}")
    return [out for _, out in res]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_ga_math_ranks(n):
    """whole-array calls, patch forms, the general path (another block map, shifted
    patches, temporaries destroyed) and the ordering against a pending NGA_NbAcc;
    every dot product is the same bits on every rank"""
    outs = launch_ok("all", n)
    for out in outs:
        for section in ("whole", "patch", "general", "order"):
            assert f"SECTION {section} OK" in out, out[-2000:]
        assert "GA on-device calls: fill" in out   # GA_Print_stats counts the new calls
    dots = [[ln for ln in out.splitlines() if ln.startswith("DOT ")] for out in outs]
    assert len(dots[0]) == 13, dots[0]
    for d in dots[1:]:
        assert d == dots[0], (d, dots[0])


@pytest.mark.gpu
def test_ga_math_64bit_offsets():
    """a 1-D C_DBL array of 2**29 + 3 elements (byte offsets past 2**32): GA_Fill,
    GA_Ddot = 2**29 + 3 exactly, NGA_Get of the last three elements and of three
    straddling byte offset 2**32"""
    launch_ok("big", 1)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2])
def test_ga_math_tall_arrays(n):
    """C_DBL and C_FLOAT arrays of [70001 * n + 1, 3]: NGA_Fill_patch, NGA_Scale_patch,
    NGA_Add_patch and the dot products on a patch of which every rank holds more than 65535
    rows of two elements (the worker asserts it), and GA_Fill on the whole array; the
    comparison covers the column outside the patch and the first and last rows"""
    outs = launch_ok("tall", n)
    dots = [[ln for ln in out.splitlines() if ln.startswith("DOT ")] for out in outs]
    assert len(dots[0]) == 2, dots[0]
    for d in dots[1:]:
        assert d == dots[0], (d, dots[0])


@pytest.mark.gpu
@pytest.mark.parametrize("mode,message,env", [
    ("abort-type", "type mismatch", None),
    ("abort-trans", "transposed patches", None),
    ("abort-host", "host segment", {"COMEX_AMD_SEGMENT": "host"}),
], ids=["type", "transpose", "host-segment"])
def test_ga_math_aborts(mode, message, env):
    """GA_Ddot on a C_FLOAT array, a transposed NGA_Copy_patch and GA_Fill on an array in
    a host segment end every rank through GA_Error: the message and a non-zero status
    (the checks come before the call's first sync or launch)"""
    res = launch(mode, 2, limit=60, extra_env=env)
    for r, (rc, out) in enumerate(res):
        ok = rc not in (0, 3, 124, 137) and "ABORT EXPECTED" in out and message in out and "NOT REACHED" not in out
        if not ok:
            _broken.append(f"{mode}: rank {r} status {rc}")
            pytest.fail(f"rank {r} rc={rc}\n{tails(res)}")
