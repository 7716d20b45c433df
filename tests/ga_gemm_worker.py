"""One rank of the GA_Dgemm / GA_Sgemm / NGA_Matmul_patch tests
(test_gpu_ga_gemm_mp.py starts 1, 2 or 3 of these on one GPU).

Sections, each printing "SECTION <name> OK":
  exact   GA_Dgemm and GA_Sgemm, all four (ta, tb), integer-valued data whose every
          partial sum is exact, m, n, k = 150, 97, 2 * panel + 37 (three panels of k, the
          last one short), REGULAR maps; raw bits against the int64 product
  maps    NGA_Matmul_patch on patches shifted inside larger arrays whose three
          irregular block maps differ (with 2 and 3 ranks one rank's block of C is a
          single row); everything outside clo:chi unchanged
  bits    random data: "GEMM <case> <sha256 of the whole C>", which the launcher compares
          across ranks and across rank counts
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
C_FLOAT, C_DBL = 1003, 1004
DT = {C_FLOAT: np.dtype(np.float32), C_DBL: np.dtype(np.float64)}
TRANS = [("N", "N"), ("N", "T"), ("T", "N"), ("T", "T")]


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class GA:
    """a 2-D global array and its numpy model (C order)"""

    def __init__(self, L, t, dims, name, irreg=None):
        self.L, self.t, self.dims, self.dt = L, t, list(dims), DT[t]
        if irreg:
            block, amap = irreg
            self.g = L.NGA_Create_irreg(t, 2, ia(dims), name, ia(block), ia(amap))
        else:
            self.g = L.NGA_Create(t, 2, ia(dims), name, None)
        assert self.g > 0
        self.model = np.zeros(dims, dtype=self.dt)

    def put(self, vals, rank):
        """rank 0 writes the whole array; everyone syncs"""
        vals = np.ascontiguousarray(vals, dtype=self.dt).reshape(self.dims)
        self.L.GA_Sync()
        if rank == 0:
            self.L.NGA_Put(self.g, ia([0, 0]), ia([d - 1 for d in self.dims]), vp(vals), ia(self.dims[1:]))
        self.L.GA_Sync()
        self.model = vals.copy()

    def get(self):
        out = np.empty(self.dims, dtype=self.dt)
        self.L.NGA_Get(self.g, ia([0, 0]), ia([d - 1 for d in self.dims]), vp(out), ia(self.dims[1:]))
        return out

    def check(self, what):
        got = self.get()
        assert got.tobytes() == self.model.tobytes(), \
            f"{what}: {np.count_nonzero(got != self.model)} of {got.size} elements differ"

    def destroy(self):
        self.L.GA_Destroy(self.g)


def op(x, t):
    return x.T if t == "T" else x


def stored_dims(rows, cols, t):
    return [cols, rows] if t == "T" else [rows, cols]


def gemm_call(L, t, ta, tb, m, n, k, alpha, a, b, beta, c):
    fn = L.GA_Dgemm if t == C_DBL else L.GA_Sgemm
    fn(ta.encode(), tb.encode(), m, n, k, alpha, a.g, b.g, beta, c.g)


def exact(L, rank, size):
    panel = L.gaamd_ga_gemm_panel()
    m, n, k = 150, 97, 2 * panel + 37
    assert k <= 2100
    for t in (C_DBL, C_FLOAT):
        for ta, tb in TRANS:
            rng = np.random.default_rng(t + 10 * ord(ta) + ord(tb))
            a = GA(L, t, stored_dims(m, k, ta), b"a")
            b = GA(L, t, stored_dims(k, n, tb), b"b")
            c = GA(L, t, [m, n], b"c")
            a.put(rng.integers(-8, 9, a.dims), rank)
            b.put(rng.integers(-8, 9, b.dims), rank)   # random: not symmetric
            c.put(rng.integers(-8, 9, c.dims), rank)
            gemm_call(L, t, ta, tb, m, n, k, 2.0, a, b, -3.0, c)
            prod = op(a.model, ta).astype(np.int64) @ op(b.model, tb).astype(np.int64)
            c.model = (2 * prod - 3 * c.model.astype(np.int64)).astype(DT[t])
            tag = f"{'GA_Dgemm' if t == C_DBL else 'GA_Sgemm'} {ta}{tb}"
            c.check(tag)
            a.check(f"{tag} left a alone")
            b.check(f"{tag} left b alone")
            for x in (a, b, c):
                x.destroy()


def cuts(size, first):
    """`size` block starts: 0, then `first`, then (three ranks) a block of a single row"""
    return [0, first, first + 1][:size]


def maps(L, rank, size):
    """three irregular maps that differ; patches shifted inside larger arrays"""
    t = C_DBL
    m, n, k = 61, 45, 83
    for ta, tb in TRANS:
        rng = np.random.default_rng(10 * ord(ta) + ord(tb))
        ad, bd, cd = [r + 9 for r in stored_dims(m, k, ta)], [r + 11 for r in stored_dims(k, n, tb)], [m + 7, n + 6]
        # A cut along its rows, B along its columns, C along its rows with (2, 3 ranks) a
        # block of a single row inside the patch
        a = GA(L, t, ad, b"a", irreg=([size, 1], [0, 20, 50][:size] + [0]))
        b = GA(L, t, bd, b"b", irreg=([1, size], [0] + [0, 13, 30][:size]))
        c = GA(L, t, cd, b"c", irreg=([size, 1], cuts(size, 30) + [0]))
        if size == 3:
            lo, hi = (ctypes.c_int * 2)(), (ctypes.c_int * 2)()
            L.NGA_Distribution(c.g, 1, lo, hi)
            assert hi[0] - lo[0] == 0, (list(lo), list(hi))   # rank 1 owns one row of C
        a.put(rng.integers(-8, 9, ad), rank)
        b.put(rng.integers(-8, 9, bd), rank)
        c.put(rng.integers(-8, 9, cd), rank)
        alo, blo, clo = [4, 3], [5, 6], [2, 3]
        ash, bsh = stored_dims(m, k, ta), stored_dims(k, n, tb)
        ahi = [alo[0] + ash[0] - 1, alo[1] + ash[1] - 1]
        bhi = [blo[0] + bsh[0] - 1, blo[1] + bsh[1] - 1]
        chi = [clo[0] + m - 1, clo[1] + n - 1]
        al, be = np.array([2.0]), np.array([-3.0])
        L.NGA_Matmul_patch(ta.encode(), tb.encode(), vp(al), vp(be), a.g, ia(alo), ia(ahi), b.g, ia(blo), ia(bhi),
                           c.g, ia(clo), ia(chi))
        pa = a.model[alo[0]:ahi[0] + 1, alo[1]:ahi[1] + 1]
        pb = b.model[blo[0]:bhi[0] + 1, blo[1]:bhi[1] + 1]
        prod = op(pa, ta).astype(np.int64) @ op(pb, tb).astype(np.int64)
        sc = (slice(clo[0], chi[0] + 1), slice(clo[1], chi[1] + 1))
        c.model[sc] = (2 * prod - 3 * c.model[sc].astype(np.int64)).astype(DT[t])
        c.check(f"NGA_Matmul_patch {ta}{tb} (outside clo:chi unchanged)")
        a.check("a unchanged")
        b.check("b unchanged")
        for x in (a, b, c):
            x.destroy()
    if size == 2:
        # two ranks: the second one's block of C is the single last row of the patch
        a, b = GA(L, t, [40, 30], b"a"), GA(L, t, [30, 20], b"b")
        c = GA(L, t, [40, 20], b"c", irreg=([2, 1], [0, 39, 0]))
        rng = np.random.default_rng(3)
        a.put(rng.integers(-8, 9, a.dims), rank)
        b.put(rng.integers(-8, 9, b.dims), rank)
        c.put(rng.integers(-8, 9, c.dims), rank)
        L.GA_Dgemm(b"N", b"N", 40, 20, 30, 2.0, a.g, b.g, -3.0, c.g)
        c.model = (2 * (a.model.astype(np.int64) @ b.model.astype(np.int64)) - 3 * c.model.astype(np.int64)).astype(DT[t])
        c.check("GA_Dgemm with a one-row block of C")
        for x in (a, b, c):
            x.destroy()


def bits(L, rank, size):
    panel = L.gaamd_ga_gemm_panel()
    for t, name in ((C_DBL, "dbl"), (C_FLOAT, "flt")):
        for ta, tb in (("N", "N"), ("T", "N"), ("N", "T")):
            m, n, k = 139, 101, panel + 211
            rng = np.random.default_rng(t + ord(ta) + 3 * ord(tb))
            starts = [0, 41, 90][:size]
            a = GA(L, t, stored_dims(m, k, ta), b"a")
            b = GA(L, t, stored_dims(k, n, tb), b"b", irreg=([size, 1], starts + [0]))
            c = GA(L, t, [m, n], b"c")
            a.put(rng.uniform(-2, 2, a.dims), rank)
            b.put(rng.uniform(-2, 2, b.dims), rank)
            c.put(rng.uniform(-2, 2, c.dims), rank)
            gemm_call(L, t, ta, tb, m, n, k, 0.7071067811865476, a, b, -1.3, c)
            got = c.get()
            wide = np.longdouble if t == C_DBL else np.float64
            ref = wide(DT[t].type(0.7071067811865476)) * (op(a.model, ta).astype(wide) @ op(b.model, tb).astype(wide)) \
                + wide(DT[t].type(-1.3)) * c.model.astype(wide)
            # far looser than the kernel test's bound: only that it is the product at all
            assert np.max(np.abs(got.astype(wide) - ref)) < (1e-9 if t == C_DBL else 1e-2), "not the product"
            print(f"GEMM {name}-{ta}{tb} {hashlib.sha256(got.tobytes()).hexdigest()}", flush=True)
            for x in (a, b, c):
                x.destroy()


if __name__ == "__main__":
    run([("exact", exact), ("maps", maps), ("bits", bits)], check_live=True)
