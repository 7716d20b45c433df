"""GPU, GA layer: GA_Dgemm / GA_Sgemm / NGA_Matmul_patch on 1, 2 and 3 ranks sharing one
GPU (tests/ga_gemm_worker.py is one rank).  Exact integer data is compared as raw bits
against the int64 product; random data has to give the same bits on every rank and on
every rank count.

Every rank process runs under its own time limit (a watcher thread each); once a
launch ends in anything but success, the remaining tests of this file start nothing."""
import os
import socket
import subprocess
import sys
import threading

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORKER = os.path.join(HERE, "ga_gemm_worker.py")

_broken = []
_gemm_lines = {}   # rank count -> the "GEMM ..." lines of its run


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(n, limit=90):
    """[(exit status, output)] of the n ranks"""
    if _broken:
        pytest.fail(f"not started: an earlier launch of this file went wrong ({_broken[0]})")
    port = str(free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(n), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=port, COMEX_AMD_JOBID=f"g{port}", COMEX_AMD_STAGING_MB="16",
                   TEST_STACK_DUMP_S=str(limit - 15))
        # the ranks are this process's own children: the node rendezvous is named after the
        # parent's pid, so a wrapper process per rank would keep them from meeting
        procs.append(subprocess.Popen([sys.executable, WORKER], cwd=ROOT, env=env, stdout=subprocess.PIPE,
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
def test_ga_gemm_ranks(n):
    """exact products on REGULAR maps, shifted patches on three differing irregular maps
    (a one-row block of C with 2 and 3 ranks), no array left alive, the call counted by
    GA_Print_stats; the sha256 of every random-data C is the same on every rank, and the
    same as on the rank counts run before this one"""
    res = launch(n)
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
        calls = 8 + 4 + (1 if n == 2 else 0) + 6   # exact, maps (+ the one-row case), bits
        assert stats[0].endswith(f"gemm {calls}"), stats[0]
    lines = [[ln for ln in out.splitlines() if ln.startswith("GEMM ")] for out in outs]
    assert len(lines[0]) == 6, lines[0]
    for ln in lines[1:]:
        assert ln == lines[0], (ln, lines[0])
    _gemm_lines[n] = lines[0]
    for other, theirs in _gemm_lines.items():
        assert theirs == lines[0], f"{n} ranks and {other} ranks gave different bits:\n{lines[0]}\n{theirs}"
