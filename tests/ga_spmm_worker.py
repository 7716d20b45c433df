"""One rank of the sparse x dense and conversion tests (test_gpu_ga_spmm_mp.py starts 1 to 4 of these on
one GPU).

Modes:
  all          NGA_Sprs_array_sprsdns_multiply, _create_from_dense and _create_from_sparse on a 37 x 53
               matrix (an empty row block on 3 ranks, duplicates, everything added by rank 0 so that the
               duplicates' order does not follow the rank count), the 2 x 5 one (on 3 ranks one rank has no
               rows) and a block-diagonal one (B in place); f64, complex f32 and C_LONG; n = 1, 5, 70; B
               under NGA_Create, with a chunk, and under NGA_Create_irreg on the column cuts
  four         the 2 x 5 matrix on 4 ranks: row 1 belongs to rank 2 but lies in rank 1's block of the
               product and of the dense copy, so rank 2 writes through scratch
  abort-rows   sprsdns_multiply with a g_b of 4 rows where 6 are needed
  abort-rank1  create_from_dense of a 1-D array
               every rank must end through GA_Error; both print "ABORT EXPECTED" just before the call
               and "NOT REACHED" if it returns
Every rank models the WHOLE matrix with the restatements of test_gpu_sprs.py / test_gpu_spmm.py and
compares raw bits.  Results are printed as "DIGEST <case> <sha1>", which the launcher compares across
ranks and across rank counts ("DIGESTN ...": across ranks only).  Prints "RANK <r> OK" on success.
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
import ga_sprs_worker as W  # noqa: E402
import test_gpu_ga_math as K  # noqa: E402
import test_gpu_spmm as M  # noqa: E402
import test_gpu_sprs as S  # noqa: E402
from ga_worker import C_DBL, C_LONG, C_SCPL, OP_OF, run, vp  # noqa: E402

ia = ga_amd.int_array
TYPES = (C_DBL, C_SCPL, C_LONG)
WIDTHS = (1, 5, 70)


def matrix_elements(name, size):
    """(idim, jdim, i, j, src, full): full = duplicate-free with the whole diagonal stored"""
    if name == "m37":        # no entry in the rows 13 .. 24 (rank 1's on 3 ranks); every fourth element twice more
        rng = np.random.default_rng(37)
        idim, jdim = 37, 53
        flat = rng.choice(idim * jdim, 420, replace=False)
        i, j = flat // jdim, flat % jdim
        keep = (i < 13) | (i > 24)
        i, j = i[keep], j[keep]
        i, j = np.concatenate([i, i[::4], i[::4]]), np.concatenate([j, j[::4], j[::4]])
        perm = rng.permutation(len(i))
        return idim, jdim, i[perm], j[perm], np.zeros(len(i), dtype=np.int64), False
    if name == "full":       # 37 x 53, duplicate-free, the whole diagonal
        rng = np.random.default_rng(38)
        idim, jdim = 37, 53
        flat = np.union1d(rng.choice(idim * jdim, 300, replace=False), np.arange(idim) * (jdim + 1))
        flat = flat[rng.permutation(len(flat))]
        return idim, jdim, flat // jdim, flat % jdim, rng.integers(0, size, len(flat)), True
    if name == "tiny":
        return S.ga_matrix("tiny", size) + (False,)
    return W.bdiag(size) + (False,)


class SpMat:
    """a sparse array and the model of every rank's part"""

    def __init__(self, L, t, name, rank, size):
        self.L, self.t, self.op, self.rank, self.size = L, t, OP_OF[t], rank, size
        self.dt = K.DT[self.op]
        self.idim, self.jdim, i, j, src, self.full = matrix_elements(name, size)
        v = M.values(self.op, len(i), np.random.default_rng(500 + self.op + len(name)))
        if self.op in K.UNS:
            v[v == 0] = 1
        self.s = add_and_assemble(L, t, self.idim, self.jdim, i, j, v, src, rank)
        self.csr = [S.ref_assemble(S.ga_parts(i, j, v, src, size), self.idim, self.jdim, size, p) for p in range(size)]
        self.tag = f"{name}-{ga_amd.OP_NAME[self.op]}"

    def rows_of(self, p):
        return S.own_range(self.idim, self.size, p)

    def col_span(self, p):
        """the rows of B rank p needs: first column of its first non-empty block to the last of its last"""
        blocks = self.csr[p]["blocks"]
        if not blocks:
            return None
        return S.own_range(self.jdim, self.size, blocks[0])[0], S.own_range(self.jdim, self.size, blocks[-1])[1]

    def product(self, b, n):
        return np.concatenate([M.ref_spmm(self.op, c, b, 0, n) for c in self.csr])

    def dense(self):
        out = np.zeros((self.idim, self.jdim), dtype=self.dt)
        for c in self.csr:
            rows = S.entry_rows(c)
            for k in range(len(rows)):   # storage order: of duplicates the last wins
                out[c["ilo"] + rows[k], c["jdx"][k]] = c["val"][k]
        return out


def add_and_assemble(L, t, idim, jdim, i, j, v, src, rank):
    s = L.NGA_Sprs_array_create(idim, jdim, t)
    assert s > 0
    mine = np.flatnonzero(src == rank)
    vm = np.ascontiguousarray(v[mine])
    for k, (a, b) in enumerate(zip(np.asarray(i)[mine].tolist(), np.asarray(j)[mine].tolist())):
        L.NGA_Sprs_array_add_element(s, a, b, ctypes.c_void_p(vm.ctypes.data + k * vm.itemsize))
    assert L.NGA_Sprs_array_assemble(s) == 1
    return s


def read_csr(L, s, size, dt, nrows):
    """[(icol, offs, jdx, val)] of this rank's non-empty column blocks, through the access pointers"""
    out = []
    for icol in range(size):
        idx, jdx, val = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        L.NGA_Sprs_array_access_col_block(s, icol, ctypes.byref(idx), ctypes.byref(jdx), ctypes.byref(val))
        if not idx.value:
            assert not jdx.value and not val.value
            continue
        o = W.from_dev(idx.value, np.int32, nrows + 1)
        out.append((icol, o.tobytes(), W.from_dev(jdx.value, np.int32, int(o[-1])).tobytes(),
                    W.from_dev(val.value, dt, int(o[-1])).tobytes()))
    return out


def model_csr(csr):
    out = []
    for b, icol in enumerate(csr["blocks"]):
        o, s = csr["offs"][b], int(csr["start"][b])
        out.append((icol, o.tobytes(), csr["jdx"][s:s + o[-1]].tobytes(), csr["val"][s:s + o[-1]].tobytes()))
    return out


class Mat2:
    """a 2-D global array of rows x cols (C order) under one of three block maps"""

    def __init__(self, L, t, rows, cols, kind, size, name=b"b"):
        self.L, self.rows, self.cols, self.dt = L, rows, cols, K.DT[OP_OF[t]]
        if kind == "regular":
            self.g = L.NGA_Create(t, 2, ia([rows, cols]), name, None)
        elif kind == "chunk":
            self.g = L.NGA_Create(t, 2, ia([rows, cols]), name, ia([max(1, rows // 5), max(1, cols // 2)]))
        elif kind == "irreg":    # full rows on cuts that are neither NGA_Create's nor the matrix's
            nb = min(size, rows)
            cuts = [0] + [min(rows - 1, max(k, rows * k // nb - rows // 7 - 1)) for k in range(1, nb)]
            self.g = L.NGA_Create_irreg(t, 2, ia([rows, cols]), name, ia([nb, 1]), ia(cuts + [0]))
        else:                    # "cuts": full rows on the sparse array's cuts of `rows`, empty trailing blocks left out
            los = [S.own_range(rows, size, p)[0] for p in range(size)]
            los = [lo for lo in los if lo < rows]
            self.g = L.NGA_Create_irreg(t, 2, ia([rows, cols]), name, ia([len(los), 1]), ia(los + [0]))
        assert self.g > 0

    def put(self, vals, rank):
        self.L.GA_Sync()
        if rank == 0:
            self.L.NGA_Put(self.g, ia([0, 0]), ia([self.rows - 1, self.cols - 1]),
                           vp(np.ascontiguousarray(vals, dtype=self.dt)), ia([self.cols]))
        self.L.GA_Sync()

    def destroy(self):
        self.L.GA_Destroy(self.g)


def whole2(L, g, dt, rows, cols):
    out = np.empty((rows, cols), dtype=dt)
    L.NGA_Get(g, ia([0, 0]), ia([rows - 1, cols - 1]), vp(out), ia([cols]))
    return out


def block_of(L, g, p):
    lo, hi = ia([0, 0]), ia([0, 0])
    L.NGA_Distribution(g, p, lo, hi)
    return (lo[0], hi[0]), (lo[1], hi[1])


def own_block(L, g, rank, dt):
    """this rank's block read where it lies (NGA_Access), or None"""
    (r0, r1), (c0, c1) = block_of(L, g, rank)
    if r1 < r0 or c1 < c0:
        return None
    p, ld = ctypes.c_void_p(), ia([0])
    L.NGA_Access(g, ia([r0, c0]), ia([r1, c1]), ctypes.byref(p), ld)
    got = W.from_dev(p.value, dt, (r1 - r0 + 1) * ld[0]).reshape(r1 - r0 + 1, ld[0])[:, :c1 - c0 + 1]
    L.NGA_Release(g, ia([r0, c0]), ia([r1, c1]))
    return r0, r1, got


def routes(L):
    return ga_amd.spmm_route_counts()


def on_row_cuts(L, g, m):
    """block k of g is the k-th rank that owns rows, with all columns; the others own nothing"""
    owners = [p for p in range(m.size) if m.rows_of(p)[1] >= m.rows_of(p)[0]]
    for p in range(m.size):
        (r0, r1), (c0, c1) = block_of(L, g, p)
        if p < len(owners):
            assert (r0, r1) == m.rows_of(owners[p]) and c0 == 0, (m.tag, p, r0, r1)
        else:
            assert r1 < r0, (m.tag, p)
    return owners


def check_product(L, m, kind, n, per_count):
    rank, size = m.rank, m.size
    b = M.values(m.op, (m.jdim, n), np.random.default_rng(70 + m.op + n))
    bm = Mat2(L, m.t, m.jdim, n, kind, size)
    bm.put(b, rank)
    live, before = L.gaamd_ga_live_arrays(), routes(L)
    g_c = L.NGA_Sprs_array_sprsdns_multiply(m.s, bm.g)
    assert g_c > 0 and L.gaamd_ga_live_arrays() == live + 1
    after = routes(L)
    owners = on_row_cuts(L, g_c, m)
    if all(m.rows_of(p)[1] >= m.rows_of(p)[0] for p in range(size)):   # then it is row_distribution's set
        lo, hi = ctypes.c_int(), ctypes.c_int()
        for p in range(size):
            L.NGA_Sprs_array_row_distribution(m.s, p, ctypes.byref(lo), ctypes.byref(hi))
            assert block_of(L, g_c, p)[0] == (lo.value, hi.value)
    # the routes, predicted from the block maps
    want = [0, 0, 0, 0]
    if m.csr[rank]["nrows"] > 0:
        span = m.col_span(rank)
        if span is not None:
            (r0, r1), (c0, c1) = block_of(L, bm.g, rank)
            inplace = r0 <= span[0] and span[1] <= r1 and c0 == 0 and c1 == n - 1
            want[0 if inplace else 1] = 1
        want[2 if rank < len(owners) and owners[rank] == rank else 3] = 1
    assert [a - b0 for a, b0 in zip(after, before)] == want, (m.tag, kind, n, want, before, after)
    wantc = m.product(b, n)
    got = whole2(L, g_c, m.dt, m.idim, n)
    assert got.tobytes() == wantc.tobytes(), f"sprsdns {m.tag} {kind} n={n}: {np.count_nonzero(got != wantc)} elements differ"
    mine = own_block(L, g_c, rank, m.dt)
    if mine is not None:
        assert np.ascontiguousarray(mine[2]).tobytes() == wantc[mine[0]:mine[1] + 1].tobytes(), (m.tag, "own block")
    assert whole2(L, bm.g, m.dt, m.jdim, n).tobytes() == b.tobytes(), "sprsdns changed B"
    W.digest(f"sprsdns-{m.tag}-{kind}-{n}", got, per_count)
    L.GA_Sync()
    L.GA_Destroy(g_c)
    bm.destroy()
    assert L.gaamd_ga_live_arrays() == live - 1
    return got


# ---- sections ---------------------------------------------------------------------------
def products(L, rank, size):
    live = L.gaamd_ga_live_arrays()
    for name in ("m37", "tiny", "bdiag"):
        for t in TYPES:
            m = SpMat(L, t, name, rank, size)
            for n in WIDTHS:
                first = None
                for kind in ("regular", "chunk", "cuts"):
                    got = check_product(L, m, kind, n, per_count=name == "bdiag")
                    first = got if first is None else first
                    assert got.tobytes() == first.tobytes(), "the block map of g_b changed the product"
            assert L.NGA_Sprs_array_destroy(m.s) == 1
            assert L.gaamd_ga_live_arrays() == live
    r = routes(L)
    assert r[0] > 0 and r[2] > 0 and r[3] == 0 and (size == 1 or r[1] > 0), r
    print(f"ROUTES {r}", flush=True)


def dense_data(op, rows, cols):
    """about one element in four non-zero; -0.0, NaN and an imaginary part alone planted; zeros on the diagonal"""
    rng = np.random.default_rng(90 + op)
    a = M.values(op, (rows, cols), rng)
    if op in K.UNS:
        a[a == 0] = 1
    a[rng.random((rows, cols)) >= 0.25] = 0
    for d in range(0, min(rows, cols), 2):
        a[d, d] = 0
    if op not in K.UNS:
        a[1, 7], a[3, 0] = -0.0, np.nan
        if op in K.REAL:
            a[4, 9], a[5, 2] = complex(0.0, -2.5), complex(-0.0, -0.0)
    return a


def conversions(L, rank, size):
    live = L.gaamd_ga_live_arrays()
    for rows, cols in ((37, 53), (2, 5)):
        for t in TYPES:
            op, dt = OP_OF[t], K.DT[OP_OF[t]]
            a = dense_data(op, rows, cols) if rows > 2 else M.values(op, (rows, cols), np.random.default_rng(3 + op))
            keep = M.ref_keep(op, a, 0, 0)
            i, j = np.nonzero(keep)
            v = np.ascontiguousarray(a[i, j])
            assert rows == 2 or ((a[i, j] == 0).any() and len(i) < rows * cols // 2)
            src = np.zeros(len(i), dtype=np.int64)
            model = S.ref_assemble(S.ga_parts(i, j, v, src, size), rows, cols, size, rank)
            s_add = add_and_assemble(L, t, rows, cols, i, j, v, src, rank)
            by_add = read_csr(L, s_add, size, dt, model["nrows"])
            assert by_add == model_csr(model)
            for kind in ("regular", "chunk", "irreg"):
                am = Mat2(L, t, rows, cols, kind, size, b"a")
                am.put(a, rank)
                s_new = L.NGA_Sprs_array_create_from_dense(am.g)
                assert s_new > 0 and L.gaamd_ga_live_arrays() == live + 1   # `am` alone
                got = read_csr(L, s_new, size, dt, model["nrows"])
                assert got == by_add, (ga_amd.OP_NAME[op], rows, kind, "from_dense differs from the add_element construction")
                assert whole2(L, am.g, dt, rows, cols).tobytes() == a.tobytes(), "from_dense changed g_a"
                assert L.NGA_Sprs_array_destroy(s_new) == 1
                am.destroy()
            assert L.NGA_Sprs_array_destroy(s_add) == 1
    for name in ("m37", "tiny", "full"):
        for t in TYPES:
            m = SpMat(L, t, name, rank, size)
            g_d = L.NGA_Sprs_array_create_from_sparse(m.s)
            assert g_d > 0 and L.gaamd_ga_live_arrays() == live + 1
            on_row_cuts(L, g_d, m)
            want = m.dense()
            got = whole2(L, g_d, m.dt, m.idim, m.jdim)
            assert got.tobytes() == want.tobytes(), (m.tag, "from_sparse")
            W.digest(f"from_sparse-{m.tag}", got, per_count=name == "full")
            if m.full:   # duplicate-free, the whole diagonal, no stored zero: the round trip gives S back
                L.GA_Sync()
                s_back = L.NGA_Sprs_array_create_from_dense(g_d)
                assert read_csr(L, s_back, size, m.dt, m.csr[rank]["nrows"]) == model_csr(m.csr[rank]), (m.tag, "round trip")
                assert L.NGA_Sprs_array_destroy(s_back) == 1
            L.GA_Sync()
            L.GA_Destroy(g_d)
            assert L.NGA_Sprs_array_destroy(m.s) == 1
            assert L.gaamd_ga_live_arrays() == live


def four(L, rank, size):
    """2 x 5 on 4 ranks: the rows belong to the ranks 0 and 2, the blocks of the row-cut arrays to 0 and 1"""
    assert size == 4
    live = L.gaamd_ga_live_arrays()
    for t in TYPES:
        m = SpMat(L, t, "tiny", rank, size)
        assert [m.rows_of(p) for p in range(4)] == [(0, 0), (1, 0), (1, 1), (2, 1)]
        for n in (1, 5):
            check_product(L, m, "regular", n, per_count=False)
        g_d = L.NGA_Sprs_array_create_from_sparse(m.s)
        assert whole2(L, g_d, m.dt, 2, 5).tobytes() == m.dense().tobytes()
        L.GA_Sync()
        L.GA_Destroy(g_d)
        assert L.NGA_Sprs_array_destroy(m.s) == 1
    r = routes(L)
    assert (r[3] > 0) == (rank == 2) and (r[2] > 0) == (rank == 0), r
    assert L.gaamd_ga_live_arrays() == live
    print(f"ROUTES {r}", flush=True)


def aborts(L, rank, size, mode):
    s = L.NGA_Sprs_array_create(5, 6, C_DBL)
    one = np.ones(1)
    if rank == 0:
        L.NGA_Sprs_array_add_element(s, 4, 5, vp(one))
    L.NGA_Sprs_array_assemble(s)
    short = Mat2(L, C_DBL, 4, 3, "regular", size, b"short")
    vec = W.Vec(L, C_DBL, 9, "regular", size, b"vec")
    L.GA_Sync()
    print("ABORT EXPECTED", flush=True)
    if mode == "abort-rows":
        L.NGA_Sprs_array_sprsdns_multiply(s, short.g)
    else:
        L.NGA_Sprs_array_create_from_dense(vec.g)
    print("NOT REACHED", flush=True)


if __name__ == "__main__":
    run({"all": [("products", products), ("conversions", conversions)], "four": [("four", four)]}, aborts)
