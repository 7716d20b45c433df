"""GPU, GA layer: GA_Zgemm / GA_Cgemm / NGA_Matmul_patch on complex arrays, on 1, 2 and 3
ranks sharing one GPU (tests/ga_zgemm_worker.py is one rank).  Exact integer data is compared
as raw bits against the integer product; random data has to give the same bits on every rank
and on every rank count.  GA_Dgemm with trans 'C' still ends through GA_Error.

Every rank process runs under its own time limit (a watcher thread each); once a launch
ends in anything but what it was started for, the remaining tests of this file start nothing."""
import os
import socket
import subprocess
import sys
import threading

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORKER = os.path.join(HERE, "ga_zgemm_worker.py")

_broken = []
_gemm_lines = {}   # rank count -> the "ZGEMM ..." lines of its run


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(mode, n, limit=90):
    """[(exit status, output)] of the n ranks"""
    if _broken:
        pytest.fail(f"not started: an earlier launch of this file went wrong ({_broken[0]})")
    port = str(free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(n), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=port, COMEX_AMD_JOBID=f"z{port}", COMEX_AMD_STAGING_MB="16",
                   TEST_STACK_DUMP_S=str(limit - 15))
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


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_ga_zgemm_ranks(n):
    """exact products of both complex types on REGULAR maps (NN, TN, CN, NC; three panels of
    k), shifted patches on three differing irregular maps (a one-row block of C with 2 and 3
    ranks), no array left alive, the calls counted by GA_Print_stats under gemm; the sha256 of
    every random-data C (a second panel through beta = (1, 0)) is the same on every rank, and
    the same as on the rank counts run before this one"""
    res = launch("all", n)
    for r, (rc, out) in enumerate(res):
        if rc != 0 or f"RANK {r} OK" not in out:
            _broken.append(f"{n} ranks: rank {r} status {rc}")
            pytest.fail(f"rank {r} rc={rc}\n{tails(res)}")
    outs = [out for _, out in res]
    for r, out in enumerate(outs):
        for section in ("exact", "maps", "bits"):
            assert f"SECTION {section} OK" in out, out[-2000:]
        stats = [ln for ln in out.splitlines() if f"[{r}] GA on-device calls: fill" in ln]
        assert len(stats) == 1, out[-2000:]
        calls = 8 + 2 + (1 if n == 2 else 0) + 6   # exact, maps (+ the one-row case), bits
        assert stats[0].endswith(f"gemm {calls}"), stats[0]
    lines = [[ln for ln in out.splitlines() if ln.startswith("ZGEMM ")] for out in outs]
    assert len(lines[0]) == 6, lines[0]
    for ln in lines[1:]:
        assert ln == lines[0], (ln, lines[0])
    _gemm_lines[n] = lines[0]
    for other, theirs in _gemm_lines.items():
        assert theirs == lines[0], f"{n} ranks and {other} ranks gave different bits:\n{lines[0]}\n{theirs}"


@pytest.mark.gpu
def test_ga_dgemm_still_refuses_conjugate_transpose():
    """the negative control: 'C' is for complex arrays only, GA_Dgemm answers as before --
    through GA_Error, with its message and a non-zero status, before any sync or launch"""
    res = launch("abort-dgemm-c", 1, limit=60)
    for r, (rc, out) in enumerate(res):
        ok = (rc not in (0, 3, 124, 137) and "ABORT EXPECTED" in out and "NOT REACHED" not in out
              and "GA_Dgemm: trans 'C' is not one of N n T t" in out)
        if not ok:
            _broken.append(f"abort-dgemm-c: rank {r} status {rc}")
            pytest.fail(f"rank {r} rc={rc}\n{tails(res)}")
