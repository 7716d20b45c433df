"""One rank of the sparse x sparse tests (test_gpu_ga_spgemm_mp.py starts 1 to 4 of these on one GPU).

Modes:
  all          NGA_Sprs_array_matmat_multiply for a 37 x 53 A (an empty row block on 3 ranks, duplicates) times a
               53 x 41 B with duplicates and one without, A A for a 40 x 40 with duplicates (s_a == s_b), and the
               2 x 5 times a 5 x 3, and a 3 x 40 times a 40 x 100 000 whose row 0 has more than 1024 products in
               several 32768-column windows (the kernels' fallback); f64, complex f32 and C_LONG; everything is added by rank 0, so that the
               duplicates' order does not follow the rank count
  four         the 2 x 5 times the 5 x 3 on 4 ranks: the ranks 1 and 3 own no row of A
  abort-types  A of C_DBL, B of C_FLOAT
  abort-dims   a 5 x 6 A and a 5 x 4 B
               every rank must end through GA_Error; both print "ABORT EXPECTED" just before the call and
               "NOT REACHED" if it returns
Every rank models the WHOLE product with the restatement of test_gpu_spgemm.py (ref_spgemm on every rank's
rows of A and the row CSR of all of B) and compares raw bits: C against the add_element construction of the
model's triples and against the model's block CSR.  Results are printed as "DIGEST <case> <sha1>", which the
launcher compares across ranks and across rank counts.  Prints "RANK <r> OK" on success.
"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import ga_amd  # noqa: E402
import ga_spmm_worker as P  # noqa: E402
import ga_sprs_worker as W  # noqa: E402
import test_gpu_ga_math as K  # noqa: E402
import test_gpu_spgemm as G  # noqa: E402
import test_gpu_spmm as M  # noqa: E402
import test_gpu_sprs as S  # noqa: E402
from ga_worker import C_DBL, C_FLOAT, C_LONG, C_SCPL, OP_OF, run, vp  # noqa: E402

TYPES = (C_DBL, C_SCPL, C_LONG)


def elements(name):
    """(idim, jdim, i, j) in insertion order"""
    if name == "a37":        # 37 x 53, no entry in the rows 13 .. 24 (rank 1's on 3 ranks), every fourth element twice more
        idim, jdim, i, j, _, _ = P.matrix_elements("m37", 1)
        return idim, jdim, i, j
    if name in ("b41", "b41dup"):
        rng = np.random.default_rng(41)
        idim, jdim = 53, 41
        flat = rng.choice(idim * jdim, 330, replace=False)
        i, j = flat // jdim, flat % jdim
        keep = (i < 18) | (i > 35) | (j % 5 == 0)   # rows 18 .. 35 (rank 1's on 3 ranks) hold little
        i, j = i[keep], j[keep]
        if name == "b41dup":
            i, j = np.concatenate([i, i[::3], i[::3]]), np.concatenate([j, j[::3], j[::3]])
        perm = rng.permutation(len(i))
        return idim, jdim, i[perm], j[perm]
    if name == "sq40":
        rng = np.random.default_rng(40)
        flat = rng.choice(1600, 260, replace=False)
        i, j = flat // 40, flat % 40
        i, j = np.concatenate([i, i[::5]]), np.concatenate([j, j[::5]])
        perm = rng.permutation(len(i))
        return 40, 40, i[perm], j[perm]
    if name == "a3w":        # 3 x 40: row 0 names 30 rows of B, one of them twice; the rows 1 and 2 name two each
        i = np.array([0] * 31 + [1, 1, 2, 2])
        j = np.array(list(range(30)) + [7] + [30, 31, 38, 39])
        perm = np.random.default_rng(3).permutation(len(i))
        return 3, 40, i[perm], j[perm]
    if name == "b40w":       # 40 x 100 000, 42 entries a row: row 0 of A B has more than 1024 products and takes the
        rng = np.random.default_rng(4)   # fallback, its columns in the windows 0, 2 and 3 of 32768 (1 rank) with edges
        win = 32768
        pool = np.concatenate([np.arange(0, win), np.arange(2 * win, 100000)])
        i = np.repeat(np.arange(40), 42)
        j = np.concatenate([np.concatenate([rng.choice(pool, 40, replace=False), [0, win - 1, 2 * win, 3 * win, 99999][k % 5:][:2]])
                            for k in range(40)])
        j = np.concatenate([j, np.full(40 * 42 - len(j), 2 * win)])[:len(i)]   # short rows are filled with one edge column
        perm = rng.permutation(len(i))
        return 40, 100000, i[perm], j[perm]
    if name == "a2x5":
        idim, jdim, i, j, _ = S.ga_matrix("tiny", 1)
        return idim, jdim, i, j
    assert name == "b5x3"
    return 5, 3, np.array([0, 4, 4, 2, 1, 0, 4]), np.array([2, 0, 2, 1, 1, 0, 0])   # row 3 is empty; (4, 0) twice


class Sp:
    """a sparse array added by rank 0, and the model of every rank's part"""

    def __init__(self, L, t, name, rank, size):
        self.L, self.t, self.op, self.rank, self.size, self.name = L, t, OP_OF[t], rank, size, name
        self.dt = K.DT[self.op]
        self.idim, self.jdim, self.i, self.j = elements(name)
        self.v = M.values(self.op, len(self.i), np.random.default_rng(600 + self.op + len(name)))
        if self.op in K.UNS:
            self.v[self.v == 0] = 1
        src = np.zeros(len(self.i), dtype=np.int64)
        self.s = P.add_and_assemble(L, t, self.idim, self.jdim, self.i, self.j, self.v, src, rank)
        parts = S.ga_parts(self.i, self.j, self.v, src, size)
        self.csr = [S.ref_assemble(parts, self.idim, self.jdim, size, p) for p in range(size)]
        self.rows_all = G.ref_rows(S.ref_assemble(parts, self.idim, self.jdim, 1, 0))   # the row CSR of the whole matrix

    def stored(self):
        return P.read_csr(self.L, self.s, self.size, self.dt, self.csr[self.rank]["nrows"])


def model_product(a, b):
    """the triples of A B in global rows, rank by rank"""
    ii, jj, vv = [], [], []
    for c in a.csr:
        i, j, v, _ = G.ref_spgemm(a.op, c, b.rows_all, 0)
        ii.append(i + c["ilo"])
        jj.append(j)
        vv.append(v)
    return np.concatenate(ii), np.concatenate(jj), np.concatenate(vv)


def want_routes(a, b):
    me = a.csr[a.rank]
    if me["nrows"] == 0 or not me["blocks"]:
        return [0, 0]
    nnz = [len(c["jdx"]) for c in b.csr]
    if me["blocks"] == [a.rank] and nnz[a.rank] > 0:
        return [1, 0]
    return [0, sum(1 for p in me["blocks"] if nnz[p] > 0)]


def check(L, a, b, tag, identity):
    rank, size, t, dt = a.rank, a.size, a.t, a.dt
    a_before, b_before = a.stored(), b.stored()
    live, before = L.gaamd_ga_live_arrays(), ga_amd.spgemm_route_counts()
    s_c = L.NGA_Sprs_array_matmat_multiply(a.s, b.s)
    assert s_c > 0 and s_c not in (a.s, b.s)
    assert L.gaamd_ga_live_arrays() == live, "matmat left a global array alive"
    after = ga_amd.spgemm_route_counts()
    assert [x - y for x, y in zip(after, before)] == want_routes(a, b), (tag, want_routes(a, b), before, after)
    assert a.stored() == a_before and b.stored() == b_before, "matmat changed an operand"
    # against the model's block CSR and against the add_element construction of the model's triples
    ci, cj, cv = model_product(a, b)
    src = np.zeros(len(ci), dtype=np.int64)
    model = S.ref_assemble(S.ga_parts(ci, cj, cv, src, size), a.idim, b.jdim, size, rank)
    got = P.read_csr(L, s_c, size, dt, model["nrows"])
    assert got == P.model_csr(model), (tag, "C differs from the model")
    s_ref = P.add_and_assemble(L, t, a.idim, b.jdim, ci, cj, cv, src, rank)
    assert got == P.read_csr(L, s_ref, size, dt, model["nrows"]), (tag, "C differs from the add_element construction")
    idx, n = ctypes.POINTER(ctypes.c_int)(), ctypes.c_int()
    L.NGA_Sprs_array_col_block_list(s_c, ctypes.byref(idx), ctypes.byref(n))
    assert [idx[k] for k in range(n.value)] == model["blocks"], (tag, "col_block_list")
    W.libc.free(idx)
    lo, hi = ctypes.c_int(), ctypes.c_int()
    for p in range(size):
        L.NGA_Sprs_array_row_distribution(s_c, p, ctypes.byref(lo), ctypes.byref(hi))
        assert (lo.value, hi.value) == S.own_range(a.idim, size, p)
        L.NGA_Sprs_array_column_distribution(s_c, p, ctypes.byref(lo), ctypes.byref(hi))
        assert (lo.value, hi.value) == S.own_range(b.jdim, size, p)
    # the calls that take a sparse array work on C: matvec with the team of C's global counts, and the dense copy
    team = ga_amd.spmv_team(len(ci), a.idim)
    xv, yv = W.Vec(L, t, b.jdim, "regular", size, b"x"), W.Vec(L, t, a.idim, "regular", size, b"y")
    xv.put(M.values(a.op, b.jdim, np.random.default_rng(77)), rank)
    L.NGA_Sprs_array_matvec_multiply(s_c, xv.g, yv.g)
    parts_c = S.ga_parts(ci, cj, cv, src, size)
    want_y = np.concatenate([S.ref_spmv(a.op, S.ref_assemble(parts_c, a.idim, b.jdim, size, p), xv.model, 0, team)
                             for p in range(size)])
    assert yv.get().tobytes() == want_y.tobytes(), (tag, "matvec on C")
    for s_x in (s_c, s_ref):   # the same team on both: nnz_total is the same
        L.NGA_Sprs_array_matvec_multiply(s_x, xv.g, yv.g)
        assert yv.get().tobytes() == want_y.tobytes()
    L.GA_Sync()
    xv.destroy()
    yv.destroy()
    g_c = L.NGA_Sprs_array_create_from_sparse(s_c)
    dense = P.whole2(L, g_c, dt, a.idim, b.jdim)
    want_dense = np.zeros((a.idim, b.jdim), dtype=dt)
    want_dense[ci, cj] = cv
    assert dense.tobytes() == want_dense.tobytes(), (tag, "the dense copy of C")
    W.digest(f"matmat-{tag}", dense)
    if identity:   # B without duplicates, finite data: A times the dense copy of B, bit for bit
        g_b = L.NGA_Sprs_array_create_from_sparse(b.s)
        g_ab = L.NGA_Sprs_array_sprsdns_multiply(a.s, g_b)
        assert P.whole2(L, g_ab, dt, a.idim, b.jdim).tobytes() == dense.tobytes(), (tag, "the dense identity")
        L.GA_Sync()
        L.GA_Destroy(g_ab)
        L.GA_Destroy(g_b)
    L.GA_Sync()
    L.GA_Destroy(g_c)
    # a second call gives the same bits
    s_c2 = L.NGA_Sprs_array_matmat_multiply(a.s, b.s)
    assert P.read_csr(L, s_c2, size, dt, model["nrows"]) == got
    for s_x in (s_c2, s_ref, s_c):
        assert L.NGA_Sprs_array_destroy(s_x) == 1
    assert L.gaamd_ga_live_arrays() == live


def pairs(L, rank, size, which):
    live = L.gaamd_ga_live_arrays()
    for t in TYPES:
        for an, bn in which:
            a = Sp(L, t, an, rank, size)
            b = a if bn == an else Sp(L, t, bn, rank, size)
            check(L, a, b, f"{an}-{bn}-{ga_amd.OP_NAME[a.op]}", identity=bn == "b41")
            assert L.NGA_Sprs_array_destroy(a.s) == 1
            if b is not a:
                assert L.NGA_Sprs_array_destroy(b.s) == 1
    assert L.gaamd_ga_live_arrays() == live
    print(f"ROUTES {ga_amd.spgemm_route_counts()}", flush=True)


def products(L, rank, size):
    pairs(L, rank, size, (("a37", "b41dup"), ("a37", "b41"), ("sq40", "sq40"), ("a2x5", "b5x3"), ("a3w", "b40w")))
    r = ga_amd.spgemm_route_counts()
    assert r[0] > 0 if size == 1 else r[1] > 0, r


def four(L, rank, size):
    assert size == 4
    assert [S.own_range(2, 4, p) for p in range(4)] == [(0, 0), (1, 0), (1, 1), (2, 1)]
    pairs(L, rank, size, (("a2x5", "b5x3"),))
    r = ga_amd.spgemm_route_counts()
    assert (r[1] > 0) == (rank in (0, 2)) and r[0] == 0, r


def aborts(L, rank, size, mode):
    one = np.ones(1)

    def tiny(idim, jdim, t):
        s = L.NGA_Sprs_array_create(idim, jdim, t)
        if rank == 0:
            L.NGA_Sprs_array_add_element(s, idim - 1, jdim - 1, vp(one.astype(K.DT[OP_OF[t]])))
        L.NGA_Sprs_array_assemble(s)
        return s

    s_a = tiny(5, 6, C_DBL)
    s_b = tiny(6, 4, C_FLOAT) if mode == "abort-types" else tiny(5, 4, C_DBL)
    L.GA_Sync()
    print("ABORT EXPECTED", flush=True)
    L.NGA_Sprs_array_matmat_multiply(s_a, s_b)
    print("NOT REACHED", flush=True)


if __name__ == "__main__":
    run({"all": [("products", products)], "four": [("four", four)]}, aborts)
