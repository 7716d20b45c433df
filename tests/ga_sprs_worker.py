"""One rank of the sparse-array tests (test_gpu_ga_sprs_mp.py starts 1, 2 or 3 of these on one GPU).

Modes:
  all           the matrices of test_gpu_sprs.ga_matrix -- a seeded 3001 x 2500 one of about 40 000 entries and
                a 257 x 257 ladder, dealt to the ranks by a seeded permutation; the ladder added by rank 0
                alone; the large one with a rank that adds nothing; 2 x 5; one with an empty row block; a
                block-diagonal one (x in place); one with duplicates -- each section prints "SECTION <name> OK"
  abort-matvec  matvec into a g_v of jdim != idim elements
  abort-add     add_element after assemble
                every rank must end through GA_Error; both print "ABORT EXPECTED" just before the call
                and "NOT REACHED" if it returns
Every rank models the WHOLE matrix with the numpy restatement of test_gpu_sprs.py (ref_assemble per
rank, ref_spmv with the library's team) and compares raw bits: the distributions, the block list, the
block CSR read back through the access pointers, and every computing call.  The data are inexact
random values; the results are printed as "DIGEST <case> <sha1>", which the launcher compares across
ranks and across rank counts ("DIGESTN ...": across ranks only -- the duplicates' order follows the
dealing).  Prints "RANK <r> OK" on success.
"""
import ctypes
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import ga_amd  # noqa: E402
import test_gpu_ga_math as K  # noqa: E402
import test_gpu_sprs as S  # noqa: E402
from ga_worker import C_DBL, C_DCPL, C_FLOAT, C_INT, C_LONG, C_SCPL, OP_OF, run, vp  # noqa: E402

ia = ga_amd.int_array
ALL_CALLS = (C_INT, C_LONG, C_FLOAT, C_DBL, C_DCPL)
libc = ctypes.CDLL(None)
libc.free.argtypes = [ctypes.c_void_p]


def digest(case, arr, per_count=False):
    tag = "DIGESTN" if per_count else "DIGEST"
    print(f"{tag} {case} {hashlib.sha1(np.ascontiguousarray(arr).tobytes()).hexdigest()}", flush=True)


def from_dev(ptr, dt, n):
    out = np.empty(n, dtype=dt)
    if n:
        assert ga_amd.lib().gaamd_memcpy(vp(out), ctypes.c_void_p(ptr), out.nbytes) == 0
    return out


class Vec:
    """a 1-D global array under one of three block maps, and its numpy model"""

    def __init__(self, L, t, n, kind, size, name=b"v"):
        self.L, self.n, self.dt = L, n, K.DT[OP_OF[t]]
        if kind == "regular":
            self.g = L.NGA_Create(t, 1, ia([n]), name, None)
        elif kind == "chunk":
            self.g = L.NGA_Create(t, 1, ia([n]), name, ia([max(1, n // 5)]))
        elif kind == "irreg":     # cuts that are neither NGA_Create's nor the matrix's
            nb = min(size, n)
            cuts = [0] + [min(n - 1, max(k, n * k // nb - n // 7 - 1)) for k in range(1, nb)]
            self.g = L.NGA_Create_irreg(t, 1, ia([n]), name, ia([nb]), ia(cuts))
        else:                     # "cuts": the matrix's own row or column cuts, empty trailing blocks left out
            los = [S.own_range(n, size, p)[0] for p in range(size)]
            los = [lo for lo in los if lo < n]
            self.g = L.NGA_Create_irreg(t, 1, ia([n]), name, ia([len(los)]), ia(los))
        assert self.g > 0
        self.model = np.zeros(n, dtype=self.dt)

    def put(self, vals, rank):
        self.L.GA_Sync()
        if rank == 0:
            self.L.NGA_Put(self.g, ia([0]), ia([self.n - 1]), vp(np.ascontiguousarray(vals, dtype=self.dt)), ia([]))
        self.L.GA_Sync()
        self.model = np.array(vals, dtype=self.dt)

    def get(self):
        out = np.empty(self.n, dtype=self.dt)
        self.L.NGA_Get(self.g, ia([0]), ia([self.n - 1]), vp(out), ia([]))
        return out

    def destroy(self):
        self.L.GA_Destroy(self.g)


def whole(L, g, dt, n):
    out = np.empty(n, dtype=dt)
    L.NGA_Get(g, ia([0]), ia([n - 1]), vp(out), ia([]))
    return out


class Matrix:
    """a sparse array and the model of every rank's part"""

    def __init__(self, L, t, name, rank, size):
        self.L, self.t, self.op, self.rank, self.size, self.name = L, t, OP_OF[t], rank, size, name
        self.dt = K.DT[self.op]
        self.idim, self.jdim, i, j, src = S.ga_matrix(name, size) if name != "bdiag" else bdiag(size)
        v = S.ga_values(self.op, name, i, j)
        self.s = L.NGA_Sprs_array_create(self.idim, self.jdim, t)
        assert self.s > 0
        mine = np.flatnonzero(src == rank)
        vm = np.ascontiguousarray(v[mine])
        esz = self.dt.itemsize
        for k, (a, b) in enumerate(zip(i[mine].tolist(), j[mine].tolist())):
            L.NGA_Sprs_array_add_element(self.s, a, b, ctypes.c_void_p(vm.ctypes.data + k * esz))
        assert L.NGA_Sprs_array_assemble(self.s) == 1
        parts = S.ga_parts(i, j, v, src, size)
        self.csr = [S.ref_assemble(parts, self.idim, self.jdim, size, p) for p in range(size)]
        self.W = ga_amd.spmv_team(len(i), self.idim)
        self.tag = f"{name}-{ga_amd.OP_NAME[self.op]}"

    def rows_of(self, p):
        return S.own_range(self.idim, self.size, p)

    def check_structure(self):
        L, me = self.L, self.csr[self.rank]
        lo, hi = ctypes.c_int(-9), ctypes.c_int(-9)
        for p in range(self.size):
            L.NGA_Sprs_array_row_distribution(self.s, p, ctypes.byref(lo), ctypes.byref(hi))
            assert (lo.value, hi.value) == S.own_range(self.idim, self.size, p), (self.tag, "rows", p)
            L.NGA_Sprs_array_column_distribution(self.s, p, ctypes.byref(lo), ctypes.byref(hi))
            assert (lo.value, hi.value) == S.own_range(self.jdim, self.size, p), (self.tag, "columns", p)
        lst, n = ctypes.POINTER(ctypes.c_int)(), ctypes.c_int(-1)
        L.NGA_Sprs_array_col_block_list(self.s, ctypes.byref(lst), ctypes.byref(n))
        assert [lst[k] for k in range(n.value)] == me["blocks"], (self.tag, "block list")
        libc.free(lst)
        self.check_values("assembled", structure=True)

    def check_values(self, what, structure=False):
        """the block CSR of this rank, read back through the access pointers"""
        L, me = self.L, self.csr[self.rank]
        for icol in range(self.size):
            idx, jdx, val = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
            L.NGA_Sprs_array_access_col_block(self.s, icol, ctypes.byref(idx), ctypes.byref(jdx), ctypes.byref(val))
            if icol not in me["blocks"]:
                assert not idx.value and not jdx.value and not val.value, (self.tag, "an empty block has pointers")
                continue
            b = me["blocks"].index(icol)
            o, s = me["offs"][b], int(me["start"][b])
            cnt = int(o[-1])
            assert idx.value and jdx.value and val.value and cnt > 0
            if structure:
                assert from_dev(idx.value, np.int32, me["nrows"] + 1).tobytes() == o.tobytes(), (self.tag, "offsets", icol)
                assert from_dev(jdx.value, np.int32, cnt).tobytes() == me["jdx"][s:s + cnt].tobytes(), (self.tag, "jdx", icol)
            got = from_dev(val.value, self.dt, cnt)
            assert got.tobytes() == me["val"][s:s + cnt].tobytes(), (self.tag, what, "values of block", icol)

    def product(self, x):
        return np.concatenate([S.ref_spmv(self.op, c, x, 0, self.W) for c in self.csr])

    def matvec(self, xv, yv, what, per_count=False):
        L = self.L
        yv.put(K.gen(self.op, self.idim, np.random.default_rng(9)), self.rank)   # overwritten, not accumulated into
        live = L.gaamd_ga_live_arrays()
        L.NGA_Sprs_array_matvec_multiply(self.s, xv.g, yv.g)
        assert L.gaamd_ga_live_arrays() == live
        want = self.product(xv.model)
        got = yv.get()
        assert got.tobytes() == want.tobytes(), \
            f"matvec {self.tag} {what}: {np.count_nonzero(got != want)} of {got.size} rows differ (team {self.W})"
        assert xv.get().tobytes() == xv.model.tobytes(), "matvec changed x"
        digest(f"matvec-{self.tag}-{what}", got, per_count)
        return got

    def destroy(self):
        assert self.L.NGA_Sprs_array_destroy(self.s) == 1


def bdiag(size):
    """120 x 90, entries only where the column's block is the row's rank: with g_a on the column cuts every
    rank finds its x in place"""
    rng = np.random.default_rng(8)
    idim, jdim = 120, 90
    flat = rng.choice(idim * jdim, 4000, replace=False)
    i, j = flat // jdim, flat % jdim
    keep = S.owner(i, idim, size) == S.owner(j, jdim, size)
    i, j = i[keep], j[keep]
    return idim, jdim, i, j, rng.integers(0, size, len(i))


def routes(L):
    c = (ctypes.c_longlong * 4)()
    L.gaamd_ga_sprs_route_counts(c)
    return list(c)


# ---- sections ---------------------------------------------------------------------------
def products(L, rank, size):
    """matvec of every matrix under the three kinds of block map, C_SCPL included"""
    live = L.gaamd_ga_live_arrays()
    for name in S.GA_MATRICES + ("bdiag",):
        types = (C_INT, C_LONG, C_FLOAT, C_DBL, C_SCPL, C_DCPL) if name in ("rand", "ladder") else (C_DBL, C_INT, C_SCPL)
        for t in types:
            m = Matrix(L, t, name, rank, size)
            assert L.gaamd_ga_live_arrays() == live, "a sparse array holds no global array"
            m.check_structure()
            per_count = name in ("dups", "bdiag")   # bdiag's very elements follow the rank count
            x = K.gen(m.op, m.jdim, np.random.default_rng(20 + m.op))
            first = None
            for kx, ky in (("regular", "regular"), ("chunk", "irreg"), ("irreg", "chunk"), ("cuts", "cuts")):
                xv, yv = Vec(L, t, m.jdim, kx, size, b"x"), Vec(L, t, m.idim, ky, size, b"y")
                xv.put(x, rank)
                before = routes(L)
                got = m.matvec(xv, yv, f"{kx}-{ky}", per_count)
                again = m.matvec(xv, yv, f"{kx}-{ky}", per_count)
                assert got.tobytes() == again.tobytes()
                first = got if first is None else first
                assert got.tobytes() == first.tobytes(), "the block maps of g_a and g_v changed the product"
                after = routes(L)
                if kx == ky == "cuts" and m.csr[rank]["nrows"] > 0:   # y on the row cuts is written in place;
                    assert after[2] == before[2] + 2                     # x in place where its span is the rank's
                    if name == "bdiag" and len(m.csr[rank]["blocks"]):
                        assert after[0] == before[0] + 2
                xv.destroy()
                yv.destroy()
            m.destroy()
            assert L.gaamd_ga_live_arrays() == live
    r = routes(L)
    assert r[0] > 0 and r[2] > 0 and (size == 1 or (r[1] > 0 and r[3] > 0)), r
    print(f"ROUTES {r}", flush=True)


def others(L, rank, size):
    """get_diag, shift_diag, scale, diag_left, diag_right, duplicate + destroy of the original: after each the
    values are read back and the product is taken again"""
    live = L.gaamd_ga_live_arrays()
    for name in ("rand", "ladder", "gap", "dups"):
        for t in ALL_CALLS if name in ("rand", "ladder") else (C_DBL, C_LONG, C_DCPL):
            m = Matrix(L, t, name, rank, size)
            op, dt = m.op, m.dt
            rng = np.random.default_rng(30 + op)
            per_count = name == "dups"
            xv, yv = Vec(L, t, m.jdim, "regular", size, b"x"), Vec(L, t, m.idim, "irreg", size, b"y")
            xv.put(K.gen(op, m.jdim, rng), rank)

            def get_diag(what):
                g = ctypes.c_int(0)
                L.NGA_Sprs_array_get_diag(m.s, ctypes.byref(g))
                assert g.value > 0 and L.gaamd_ga_live_arrays() == live + 3
                want = np.zeros(m.idim, dtype=dt)
                lo, hi = ctypes.c_int(), ctypes.c_int()
                for p in range(size):   # on the row cuts; from the rank's own diagonal block only
                    L.NGA_Distribution(g.value, p, ctypes.byref(lo), ctypes.byref(hi))
                    r0, r1 = m.rows_of(p)
                    assert (lo.value, hi.value) == (r0, r1) or (r1 < r0 and hi.value < lo.value), (m.tag, p)
                    if p in m.csr[p]["blocks"]:
                        S.ref_diag_get(m.csr[p], m.csr[p]["blocks"].index(p), want[r0:r1 + 1])
                got = whole(L, g.value, dt, m.idim)
                assert got.tobytes() == want.tobytes(), (m.tag, what, np.flatnonzero(got != want)[:8])
                L.GA_Sync()
                L.GA_Destroy(g.value)
                # off a square matrix the row and column cuts differ, and which (i, i) lie in a rank's own
                # diagonal block follows the rank count
                digest(f"diag-{m.tag}-{what}", got, per_count or m.idim != m.jdim)
                return want

            d0 = get_diag("fresh")
            assert name != "ladder" or (d0 != 0).all()
            shift = S.SHIFT_C[op]
            L.NGA_Sprs_array_shift_diag(m.s, vp(K.scalar(op, shift)))
            for c in m.csr:
                c["val"] = S.ref_diag_shift(op, c, shift)
            m.check_values("shift_diag")
            m.matvec(xv, yv, "shifted", per_count)
            get_diag("shifted")
            alpha = K.ALPHA[op]
            L.NGA_Sprs_array_scale(m.s, vp(K.scalar(op, alpha)))
            for c in m.csr:
                c["val"] = K.ref_scale(op, c["val"], alpha)
            m.check_values("scale")
            m.matvec(xv, yv, "scaled", per_count)
            for left in (True, False):
                n = m.idim if left else m.jdim
                dv = Vec(L, t, n, "chunk" if left else "irreg", size, b"d")
                dv.put(K.gen(op, n, rng), rank)
                (L.NGA_Sprs_array_diag_left_multiply if left else L.NGA_Sprs_array_diag_right_multiply)(m.s, dv.g)
                for c in m.csr:
                    at = c["ilo"] + S.entry_rows(c) if left else c["jdx"].astype(np.int64)
                    c["val"] = S.mul(op, dv.model[at], c["val"])
                m.check_values("diag_left" if left else "diag_right")
                m.matvec(xv, yv, "left" if left else "right", per_count)
                assert dv.get().tobytes() == dv.model.tobytes()
                dv.destroy()
            # the copy lives on when the original is gone
            dup = L.NGA_Sprs_array_duplicate(m.s)
            assert dup > 0 and dup != m.s
            m.destroy()
            m.s = dup
            m.check_structure()
            m.matvec(xv, yv, "duplicate", per_count)
            m.destroy()
            xv.destroy()
            yv.destroy()
            assert L.gaamd_ga_live_arrays() == live, m.tag


def aborts(L, rank, size, mode):
    s = L.NGA_Sprs_array_create(6, 4, C_DBL)
    one = np.ones(1)
    if rank == 0:
        L.NGA_Sprs_array_add_element(s, 5, 3, vp(one))
    L.NGA_Sprs_array_assemble(s)
    xv, yv = Vec(L, C_DBL, 4, "regular", size, b"x"), Vec(L, C_DBL, 4, "regular", size, b"short")
    L.GA_Sync()
    print("ABORT EXPECTED", flush=True)
    if mode == "abort-matvec":
        L.NGA_Sprs_array_matvec_multiply(s, xv.g, yv.g)
    else:
        L.NGA_Sprs_array_add_element(s, 0, 0, vp(one))
    print("NOT REACHED", flush=True)


if __name__ == "__main__":
    run([("products", products), ("others", others)], aborts)
