"""What the rank workers of the multi-rank GA tests (tests/ga_*_worker.py) share: the type
constants, a global array beside its numpy model, small helpers, and run(), the main() of a worker.

A worker prints "SECTION <name> OK" after each of its sections, GA_Print_stats' lines, and
"RANK <r> OK" at the end; a mode "abort..." prints "ABORT EXPECTED" just before a call that must
end the process through GA_Error, "NOT REACHED" if it returns, and then exits with status 3.
tests/mp_launch.py reads all of these."""
import ctypes
import os
import sys

import numpy as np

import ga_amd
import test_gpu_ga_math as K

ia = ga_amd.int_array
C_INT, C_LONG, C_FLOAT, C_DBL, C_SCPL, C_DCPL = 1001, 1002, 1003, 1004, 1006, 1007
OP_OF = {C_INT: K.INT, C_LONG: K.LNG, C_FLOAT: K.FLT, C_DBL: K.DBL, C_SCPL: K.CPL, C_DCPL: K.DCP}
DOT_OF = {C_INT: "I", C_LONG: "L", C_FLOAT: "F", C_DBL: "D", C_SCPL: "C", C_DCPL: "Z"}


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class GA:
    """a global array and its numpy model (C order)"""

    def __init__(self, L, t, dims, name, irreg=None):
        self.L, self.t, self.dims, self.op = L, t, list(dims), OP_OF[t]
        self.dt = K.DT[self.op]
        if irreg:
            block, amap = irreg
            self.g = L.NGA_Create_irreg(t, len(dims), ia(dims), name, ia(block), ia(amap))
        else:
            self.g = L.NGA_Create(t, len(dims), ia(dims), name, None)
        assert self.g > 0
        self.model = np.zeros(dims, dtype=self.dt)

    def lohi(self):
        return ia([0] * len(self.dims)), ia([d - 1 for d in self.dims])

    def put(self, vals, rank):
        """rank 0 writes the whole array; everyone syncs"""
        vals = np.ascontiguousarray(vals.reshape(self.dims), dtype=self.dt)
        self.L.GA_Sync()   # no rank still reads the old values
        if rank == 0:
            lo, hi = self.lohi()
            self.L.NGA_Put(self.g, lo, hi, vp(vals), ia(self.dims[1:]))
        self.L.GA_Sync()
        self.model = vals.copy()

    def get(self):
        out = np.empty(self.dims, dtype=self.dt)
        lo, hi = self.lohi()
        self.L.NGA_Get(self.g, lo, hi, vp(out), ia(self.dims[1:]))
        return out

    def check(self, what):
        got = self.get()
        assert got.tobytes() == self.model.tobytes(), \
            f"{what}: {np.count_nonzero(got != self.model)} of {got.size} elements differ"

    def destroy(self):
        self.L.GA_Destroy(self.g)


def sl(lo, hi):
    return tuple(slice(a, b + 1) for a, b in zip(lo, hi))


def flat(x):
    return np.ascontiguousarray(x).reshape(-1)


def blocks_of(L, g, nd, size):
    out = []
    for q in range(size):
        lo, hi = (ctypes.c_int * nd)(), (ctypes.c_int * nd)()
        L.NGA_Distribution(g, q, lo, hi)
        out.append((list(lo), list(hi)))
    return out


def run(sections, aborts=None, bare=None, check_live=False):
    """One rank, from GA_Initialize to "RANK <r> OK"; the mode is the first argument ("all" without one).
    sections: [(name, fn(L, rank, size))], or {mode: such a list} with the list under "all" for every
    other mode.  aborts(L, rank, size, mode) serves the modes "abort...".  bare: {mode: fn}, modes
    that are one function without sections or statistics.  check_live: no section may leave a
    global array alive."""
    import faulthandler
    faulthandler.dump_traceback_later(int(os.environ.get("TEST_STACK_DUMP_S", "600")), exit=False)
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    rank, size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    L = ga_amd.lib()
    assert L.GA_Initialize() == 0
    if aborts and mode.startswith("abort"):
        aborts(L, rank, size, mode)
        sys.exit(3)
    if bare and mode in bare:
        bare[mode](L, rank, size)
    else:
        if isinstance(sections, dict):
            sections = sections.get(mode, sections["all"])
        live0 = L.gaamd_ga_live_arrays()
        for name, fn in sections:
            fn(L, rank, size)
            L.GA_Sync()
            if check_live:
                assert L.gaamd_ga_live_arrays() == live0, "a call left a global array alive"
            print(f"SECTION {name} OK", flush=True)
        sys.stdout.flush()
        L.GA_Print_stats()
    L.GA_Terminate()
    print(f"RANK {rank} OK", flush=True)
