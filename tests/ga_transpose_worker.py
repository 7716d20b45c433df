"""One rank of the GA_Transpose / GA_Symmetrize tests
(test_gpu_ga_transpose_mp.py starts 1, 2 or 3 of these on one GPU).

Modes (argv[1]):
  all       the sections below, each printing "SECTION <name> OK"
    transpose  REGULAR maps, A 37 x 53 -> B 53 x 37, C_INT / C_DBL / C_DCPL (one case per
               element size), index-unique values; NGA_Get of all of B is A.T as bits, A
               is unchanged
    maps       A and B on differing irregular maps: with 2 and 3 ranks one rank owns a
               single row of B and another a single column of A; the cuts the other way
               round; and a case where every rank's mirror patch lies wholly in its own
               block of A (the path without a get)
    symm       a square 70 x 70 C_DBL and C_FLOAT on irregular maps, random finite data:
               0.5 * (A + A.T) as bits, and equal to its own transpose as bits
    bits       random data: "TR <case> <sha256 of the whole result>", which the launcher
               compares across ranks and across rank counts
  abort-*   a call that must end the process through GA_Error; prints "ABORT EXPECTED" just
            before it and "NOT REACHED" if it returns
Prints "RANK <r> OK" on success.
"""
import ctypes
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import ga_amd  # noqa: E402
from ga_worker import run  # noqa: E402

ia = ga_amd.int_array
C_INT, C_FLOAT, C_DBL, C_DCPL = 1001, 1003, 1004, 1007
DT = {C_INT: np.dtype(np.int32), C_FLOAT: np.dtype(np.float32), C_DBL: np.dtype(np.float64),
      C_DCPL: np.dtype(np.complex128)}
# the calls of mode "all", which the launcher finds again in GA_Print_stats
N_TRANSPOSE, N_SYMM = 3 + 3 + 1, 2 + 2


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class GA:
    """a global array and its numpy model (C order)"""

    def __init__(self, L, t, dims, name, irreg=None):
        self.L, self.t, self.dims, self.dt = L, t, list(dims), DT[t]
        nd = len(dims)
        if irreg:
            block, amap = irreg
            self.g = L.NGA_Create_irreg(t, nd, ia(dims), name, ia(block), ia(amap))
        else:
            self.g = L.NGA_Create(t, nd, ia(dims), name, None)
        assert self.g > 0
        self.model = np.zeros(dims, dtype=self.dt)

    def put(self, vals, rank):
        """rank 0 writes the whole array; everyone syncs"""
        vals = np.ascontiguousarray(vals, dtype=self.dt).reshape(self.dims)
        self.L.GA_Sync()
        if rank == 0:
            self.L.NGA_Put(self.g, ia([0] * len(self.dims)), ia([d - 1 for d in self.dims]), vp(vals), ia(self.dims[1:]))
        self.L.GA_Sync()
        self.model = vals.copy()

    def get(self):
        out = np.empty(self.dims, dtype=self.dt)
        self.L.NGA_Get(self.g, ia([0] * len(self.dims)), ia([d - 1 for d in self.dims]), vp(out), ia(self.dims[1:]))
        return out

    def check(self, what):
        got = self.get()
        assert got.tobytes() == self.model.tobytes(), \
            f"{what}: {np.count_nonzero(got != self.model)} of {got.size} elements differ"

    def destroy(self):
        self.L.GA_Destroy(self.g)


def unique(t, rows, cols):
    """index-unique values of type t"""
    k = np.arange(rows * cols).reshape(rows, cols)
    if t == C_INT:
        return k - 700
    if t == C_DBL:
        return k + 0.25
    return (k + 0.5) + 1j * (-k - 3.0)


def transpose_into(L, a, b, what):
    L.GA_Transpose(a.g, b.g)
    b.model = np.ascontiguousarray(a.model.T)
    b.check(what)
    a.check(f"{what} left A alone")


def transpose(L, rank, size):
    for t in (C_INT, C_DBL, C_DCPL):
        a, b = GA(L, t, [37, 53], b"a"), GA(L, t, [53, 37], b"b")
        a.put(unique(t, 37, 53), rank)
        b.put(np.full([53, 37], 9), rank)
        transpose_into(L, a, b, f"GA_Transpose type {t}")
        a.destroy()
        b.destroy()


def one_row(L, g, proc, axis):
    lo, hi = (ctypes.c_int * 2)(), (ctypes.c_int * 2)()
    L.NGA_Distribution(g, proc, lo, hi)
    assert hi[axis] - lo[axis] == 0, (list(lo), list(hi))


def maps(L, rank, size):
    t = C_DBL
    rows, cols = 41, 29          # A is 41 x 29, B is 29 x 41
    # 1. B cut along its rows, (2, 3 ranks) one rank owning a single row of it; A cut along
    #    its columns, another rank owning a single column
    b_rows = {1: [0], 2: [0, 28], 3: [0, 14, 15]}[size]
    a_cols = {1: [0], 2: [0, 1], 3: [0, 1, 11]}[size]
    a = GA(L, t, [rows, cols], b"a", irreg=([1, size], [0] + a_cols))
    b = GA(L, t, [cols, rows], b"b", irreg=([size, 1], b_rows + [0]))
    if size > 1:
        one_row(L, b.g, 1, 0)                              # rank 1's block of B is one row
        one_row(L, a.g, 0, 1)                              # rank 0's block of A is one column
    a.put(unique(t, rows, cols), rank)
    transpose_into(L, a, b, "maps: B by rows, A by columns")
    a.destroy()
    b.destroy()
    # 2. the cuts the other way round and at other places: every mirror patch crosses blocks
    a = GA(L, t, [rows, cols], b"a", irreg=([size, 1], [0, 13, 30][:size] + [0]))
    b = GA(L, t, [cols, rows], b"b", irreg=([1, size], [0] + [0, 7, 22][:size]))
    a.put(unique(t, rows, cols), rank)
    transpose_into(L, a, b, "maps: A by rows, B by columns")
    a.destroy()
    b.destroy()
    # 3. A cut along its rows and B along its columns at the same places: a rank's block of B
    #    is the transpose of its own block of A, so the mirror patch lies wholly in that block
    cut = [0, 1, 20][:size]
    a = GA(L, t, [rows, cols], b"a", irreg=([size, 1], cut + [0]))
    b = GA(L, t, [cols, rows], b"b", irreg=([1, size], [0] + cut))
    a.put(unique(t, rows, cols), rank)
    transpose_into(L, a, b, "maps: the mirror in the rank's own block")
    a.destroy()
    b.destroy()


def finite(rng, t, n):
    return (rng.standard_normal((n, n)) * 10.0 ** rng.integers(-3, 4, (n, n))).astype(DT[t])


def symmetrize(L, rank, size, t, irreg, seed, n=70):
    a = GA(L, t, [n, n], b"s", irreg=irreg)
    a.put(finite(np.random.default_rng(seed), t, n), rank)
    L.GA_Symmetrize(a.g)
    a.model = DT[t].type(0.5) * (a.model + a.model.T)
    assert a.model.dtype == DT[t]
    got = a.get()
    assert got.tobytes() == a.model.tobytes(), f"GA_Symmetrize type {t}: not 0.5 * (A + A.T) as bits"
    assert got.tobytes() == np.ascontiguousarray(got.T).tobytes(), "the result is not its own transpose"
    a.destroy()
    return got


def symm(L, rank, size):
    symmetrize(L, rank, size, C_DBL, ([size, 1], [0, 23, 24][:size] + [0]), 11)
    symmetrize(L, rank, size, C_FLOAT, ([1, size], [0] + [0, 40, 69][:size]), 12)


def bits(L, rank, size):
    rng = np.random.default_rng(77)
    # random bit patterns behind C_DBL: NaN payloads and -0 travel through get, kernel and put
    raw = rng.integers(0, 1 << 64, (45, 67), dtype=np.uint64).view(np.float64)
    a = GA(L, C_DBL, [45, 67], b"a", irreg=([size, 1], [0, 20, 21][:size] + [0]))
    b = GA(L, C_DBL, [67, 45], b"b", irreg=([size, 1], [0, 5, 50][:size] + [0]))
    a.put(raw, rank)
    assert a.model.tobytes() == raw.tobytes()
    L.GA_Transpose(a.g, b.g)
    got = b.get()
    assert got.tobytes() == np.ascontiguousarray(raw.T).tobytes(), "GA_Transpose of random bits"
    print(f"TR transpose-bits {hashlib.sha256(got.tobytes()).hexdigest()}", flush=True)
    a.destroy()
    b.destroy()
    got = symmetrize(L, rank, size, C_DBL, ([1, size], [0] + [0, 31, 64][:size]), 21)
    print(f"TR symm-dbl {hashlib.sha256(got.tobytes()).hexdigest()}", flush=True)
    got = symmetrize(L, rank, size, C_FLOAT, ([size, 1], [0, 1, 35][:size] + [0]), 22)
    print(f"TR symm-flt {hashlib.sha256(got.tobytes()).hexdigest()}", flush=True)


def aborts(L, rank, size, mode):
    if mode == "abort-same":
        a = GA(L, C_DBL, [12, 12], b"a")
        print("ABORT EXPECTED", flush=True)
        L.GA_Transpose(a.g, a.g)
    elif mode == "abort-3d":
        a, b = GA(L, C_DBL, [4, 5, 6], b"a"), GA(L, C_DBL, [6, 5, 4], b"b")
        print("ABORT EXPECTED", flush=True)
        L.GA_Transpose(a.g, b.g)
    elif mode == "abort-type":
        a, b = GA(L, C_DBL, [10, 12], b"a"), GA(L, C_FLOAT, [12, 10], b"b")
        print("ABORT EXPECTED", flush=True)
        L.GA_Transpose(a.g, b.g)
    elif mode == "abort-dims":
        a, b = GA(L, C_DBL, [10, 12], b"a"), GA(L, C_DBL, [10, 12], b"b")
        print("ABORT EXPECTED", flush=True)
        L.GA_Transpose(a.g, b.g)
    elif mode == "abort-square":
        a = GA(L, C_DBL, [10, 12], b"a")
        print("ABORT EXPECTED", flush=True)
        L.GA_Symmetrize(a.g)
    elif mode == "abort-int":
        a = GA(L, C_INT, [12, 12], b"a")
        print("ABORT EXPECTED", flush=True)
        L.GA_Symmetrize(a.g)
    elif mode == "abort-host":
        a, b = GA(L, C_DBL, [10, 12], b"hostseg"), GA(L, C_DBL, [12, 10], b"b")
        print("ABORT EXPECTED", flush=True)
        L.GA_Transpose(a.g, b.g)
    print("NOT REACHED", flush=True)


if __name__ == "__main__":
    run([("transpose", transpose), ("maps", maps), ("symm", symm), ("bits", bits)], aborts, check_live=True)
