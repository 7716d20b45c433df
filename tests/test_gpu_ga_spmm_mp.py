"""GPU, GA layer: NGA_Sprs_array_sprsdns_multiply, _create_from_dense and _create_from_sparse on 1, 2 and
3 ranks sharing one GPU (tests/ga_spmm_worker.py is one rank), the 2 x 5 matrix on 4 ranks, where a
rank writes its rows through scratch, and two aborts on 2 ranks.  Expected values: the numpy
restatements of test_gpu_sprs.py / test_gpu_spmm.py of the whole matrix, compared as raw bits by
every rank.

Every rank process runs under its own time limit (a watcher thread each); once a launch ends in
anything but the outcome its test expects, the remaining tests of this file start nothing."""
import os
import socket
import subprocess
import sys
import threading

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORKER = os.path.join(HERE, "ga_spmm_worker.py")

_broken = []
_digests = {}   # rank count -> the DIGEST lines of its ranks


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(mode, n, limit=120, extra_env=None):
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


def product_stats(out):
    m = [ln for ln in out.splitlines() if "GA sparse-product calls:" in ln]
    assert len(m) == 1, out[-2000:]
    return dict(kv.rsplit(" ", 1) for kv in m[0].split("calls: ")[1].split(", "))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_ga_spmm_ranks(n):
    """S B for a 37 x 53 matrix with an empty row block and duplicates, the 2 x 5 one and a block-diagonal one;
    f64, complex f32 and C_LONG; n = 1, 5, 70; B under NGA_Create, a chunk and the column cuts; the four
    route counters predicted from the block maps; C through NGA_Get and through each rank's own block; C on
    the row cuts; create_from_dense under three kinds of map against the add_element construction;
    create_from_sparse against the model; the round trip.  The same DIGEST lines on every rank AND on every
    rank count for inexact data; no global array left behind; the new statistics line once, the old one as
    it was"""
    outs = launch_ok("all", n)
    for out in outs:
        for section in ("products", "conversions"):
            assert f"SECTION {section} OK" in out, out[-2000:]
        counts = product_stats(out)
        assert set(counts) == {"sprsdns", "from_dense", "from_sparse"}
        assert all(int(v) > 0 for v in counts.values()), counts
        old = [ln for ln in out.splitlines() if "GA sparse-array calls: assemble" in ln]
        assert len(old) == 1, out[-2000:]
        old = dict(kv.rsplit(" ", 1) for kv in old[0].split("calls: ")[1].split(", "))
        assert set(old) == {"assemble", "matvec", "get_diag", "shift_diag", "scale", "diag_left", "diag_right"}
        assert int(old["assemble"]) > 0 and int(old["matvec"]) == 0
        assert len([ln for ln in out.splitlines() if ln.startswith("ROUTES ")]) == 1
    for tag, least in (("DIGEST ", 60), ("DIGESTN ", 30)):
        digests = [[ln for ln in out.splitlines() if ln.startswith(tag)] for out in outs]
        assert len(digests[0]) >= least, len(digests[0])
        for s in digests[1:]:
            assert s == digests[0]
        if tag == "DIGEST ":
            _digests[n] = digests[0]
    for other in _digests.values():   # inexact data: the same bits on any rank count (the order contract)
        assert other == _digests[n]


@pytest.mark.gpu
def test_ga_spmm_rows_in_another_ranks_block():
    """4 ranks, 2 x 5: rank 2 owns row 1, which lies in rank 1's block of the product: through scratch and put"""
    outs = launch_ok("four", 4)
    for out in outs:
        assert "SECTION four OK" in out
        assert int(product_stats(out)["sprsdns"]) == 6


@pytest.mark.gpu
@pytest.mark.parametrize("mode,message", [("abort-rows", "has 4 rows, 6 are needed"),
                                          ("abort-rank1", "has rank 1, a matrix of rank 2 is needed")])
def test_ga_spmm_aborts(mode, message):
    """on 2 ranks: every rank prints the message and ends through GA_Error with a non-zero status; none is
    killed at its time limit and none reaches the line after the call"""
    res = launch(mode, 2, limit=60)
    for r, (rc, out) in enumerate(res):
        ok = (rc not in (0, 3, 124, 137) and "ABORT EXPECTED" in out and message in out and "NOT REACHED" not in out)
        if not ok:
            _broken.append(f"{mode}: rank {r} status {rc}")
            pytest.fail(f"rank {r} rc={rc}\n{tails(res)}")
