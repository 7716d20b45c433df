"""The rank launcher of the multi-rank GA tests (test_gpu_ga_*_mp.py): one Launcher per test file.

Every rank process runs under its own time limit (a watcher thread each).  Once a launch of an
instance ends in anything but the outcome its test expects, the later launches of that instance
fail with "not started: ..." and start no process: nothing more goes to a GPU that a rank may
have left in a bad state."""
import os
import socket
import subprocess
import sys
import threading

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class Launcher:
    def __init__(self, worker, jobid, limit=90, marker=None):
        """worker: the script that is one rank (a name in tests/, or a path); jobid: the letter before
        the port in COMEX_AMD_JOBID; limit: the default time limit of a rank in seconds; marker: see tails()"""
        self.worker, self.jobid, self.limit, self.marker = os.path.join(HERE, worker), jobid, limit, marker
        self.broken = []

    def launch(self, mode, n, limit=None, extra_env=None):
        """[(exit status, output)] of the n ranks, in rank order; mode None: the worker gets no argument"""
        if self.broken:
            pytest.fail(f"not started: an earlier launch of this file went wrong ({self.broken[0]})")
        limit = self.limit if limit is None else limit
        port = str(free_port())
        procs = []
        for r in range(n):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(n), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=port, COMEX_AMD_JOBID=f"{self.jobid}{port}", COMEX_AMD_STAGING_MB="16",
                       TEST_STACK_DUMP_S=str(limit - 15))
            env.update(extra_env or {})
            # the ranks are this process's own children: the node rendezvous is named after the
            # parent's pid, so a wrapper process per rank would keep them from meeting
            procs.append(subprocess.Popen([sys.executable, self.worker] + ([] if mode is None else [mode]), cwd=ROOT,
                                          env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
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

    def tails(self, res, marker=None):
        """the end of every rank's output; with a marker (the constructor's by default), 3000
        characters from its first occurrence instead, where a rank printed it"""
        marker = marker or self.marker

        def tail(out):
            i = out.find(marker) if marker else -1
            return out[i:i + 3000] if i >= 0 else out[-2500:]
        return "\n".join(f"--- rank {r}: status {rc} ---\n{tail(out)}" for r, (rc, out) in enumerate(res))

    def _went_wrong(self, what, res, r):
        self.broken.append(f"{what}: rank {r} status {res[r][0]}")
        pytest.fail(f"rank {r} rc={res[r][0]}\n{self.tails(res)}")

    def launch_ok(self, mode, n, **kw):
        """the outputs of the n ranks, every one of which ended with status 0 and its RANK <r> OK line"""
        res = self.launch(mode, n, **kw)
        for r, (rc, out) in enumerate(res):
            if rc != 0 or f"RANK {r} OK" not in out:
                self._went_wrong(f"{n} ranks" if mode is None else f"{mode} on {n} ranks", res, r)
        return [out for _, out in res]

    def expect_abort(self, mode, n, messages, limit=60, extra_env=None):
        """every rank ends through GA_Error: a non-zero status that is neither the worker's own
        exit after the call (3) nor a kill, ABORT EXPECTED and every message printed, and the
        line after the call not reached"""
        res = self.launch(mode, n, limit=limit, extra_env=extra_env)
        for r, (rc, out) in enumerate(res):
            ok = (rc not in (0, 3, 124, 137) and "ABORT EXPECTED" in out and all(m in out for m in messages)
                  and "NOT REACHED" not in out)
            if not ok:
                self._went_wrong(mode, res, r)
        return res
