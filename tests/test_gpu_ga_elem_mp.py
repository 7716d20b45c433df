"""GPU, GA layer: GA_Abs_value / GA_Add_constant / GA_Recip / GA_Elem_multiply / _divide /
_maximum / _minimum, their patch forms, the general path, NGA_Select_elem and the
zero-divisor abort, on 1, 2 and 3 ranks sharing one GPU (tests/ga_elem_worker.py is one
rank).  Expected values: the numpy restatement in test_gpu_ga_elem.py, compared as raw bits.

Every rank process runs under its own time limit (a watcher thread each); once a launch
ends in anything but the outcome its test expects, the remaining tests of this file start
nothing."""
import os
import socket
import subprocess
import sys
import threading

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORKER = os.path.join(HERE, "ga_elem_worker.py")

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
                   MASTER_PORT=port, COMEX_AMD_JOBID=f"e{port}", COMEX_AMD_STAGING_MB="16",
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
def test_ga_elem_ranks(n):
    """whole-array and patch forms on a 37 x 53 and a 5 x 6 x 7 array, in place, the general
    path (another block map, shifted patches, temporaries destroyed), NGA_Select_elem min and
    max for the six types -- equal to numpy's first occurrence in C order (checked by every
    rank) and the same SEL line on every rank -- the tie whose lower index lives on the higher
    rank, and a 2-element array, of which one of three ranks owns nothing"""
    outs = launch_ok("all", n)
    for out in outs:
        for section in ("forms", "general", "select"):
            assert f"SECTION {section} OK" in out, out[-2000:]
        assert "GA on-device calls: fill" in out          # the existing line's text is kept
        assert "GA element-wise calls: abs" in out and "select" in out   # GA_Print_stats counts the new calls
    sels = [[ln for ln in out.splitlines() if ln.startswith("SEL ")] for out in outs]
    assert len(sels[0]) == 48 + (6 if n > 1 else 0) + 16, (len(sels[0]), sels[0])
    for s in sels[1:]:
        assert s == sels[0], (s, sels[0])
    if n > 1:
        ties = [ln for ln in sels[0] if ln.startswith("SEL tie-")]
        assert len(ties) == 6 and all(ln.endswith("[0, 1]") for ln in ties), ties


@pytest.mark.gpu
def test_ga_elem_divide_zero_divisor_aborts():
    """GA_Elem_divide with a single zero in g_b on 2 ranks: every rank -- the one whose block
    holds the zero and the other -- prints the zero-divisor message and ends through
    GA_Error with a non-zero status.  The kernel has completed and the stream is synchronised
    before that, so no rank is left waiting in a barrier (none is killed at its time limit)"""
    res = launch("abort-zero", 2, limit=60)
    for r, (rc, out) in enumerate(res):
        ok = (rc not in (0, 3, 124, 137) and "ABORT EXPECTED" in out and "zero divisor" in out
              and "NOT REACHED" not in out)
        if not ok:
            _broken.append(f"abort-zero: rank {r} status {rc}")
            pytest.fail(f"rank {r} rc={rc}\n{tails(res)}")
