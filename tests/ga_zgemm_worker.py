"""One rank of the GA_Zgemm / GA_Cgemm / complex NGA_Matmul_patch tests
(test_gpu_ga_zgemm_mp.py starts 1, 2 or 3 of these on one GPU).

Sections, each printing "SECTION <name> OK":
  exact   GA_Zgemm and GA_Cgemm on NN, TN, CN and NC, integer-valued parts whose every
          partial sum is exact, m, n, k = 150, 97, 2 * panel + 37 (three panels of k, the
          last one short), REGULAR maps; raw bits against the integer product; A and B
          unchanged
  maps    NGA_Matmul_patch on C_DCPL for NN and CT, patches shifted inside larger arrays
          whose three irregular block maps differ (with 2 and 3 ranks one rank's block of C
          is a single row); everything outside clo:chi unchanged
  bits    random data, k = panel + 211 (the second panel goes through beta = (1, 0)):
          "ZGEMM <case> <sha256 of the whole C>", which the launcher compares across ranks
          and across rank counts
Prints "RANK <r> OK" on success.
Mode abort-dgemm-c: GA_Dgemm with trans 'C' must still end the process through GA_Error;
prints "ABORT EXPECTED" just before the call and "NOT REACHED" if it returns.
"""
import ctypes
import hashlib

import numpy as np

import ga_gemm_worker as W   # the real worker's GA model and helpers (tests/ is sys.path[0])
from ga_gemm_worker import GA, cuts, ia, stored_dims, vp

from ga_amd._lib import DoubleComplex, SingleComplex  # noqa: E402  (ga_gemm_worker put the repository root on sys.path)
from ga_worker import run  # noqa: E402

C_DBL, C_SCPL, C_DCPL = 1004, 1006, 1007
W.DT[C_SCPL] = np.dtype(np.complex64)      # GA() looks its element type up there
W.DT[C_DCPL] = np.dtype(np.complex128)
DT = W.DT
AL_X, BE_X = 2 - 1j, -3 + 2j


def op(x, t):
    return x if t == "N" else x.T if t == "T" else x.conj().T


def ints(rng, dims):
    return rng.integers(-8, 9, dims) + 1j * rng.integers(-8, 9, dims)


def uniform(rng, dims):
    return rng.uniform(-2, 2, dims) + 1j * rng.uniform(-2, 2, dims)


def int_result(al, opa, opb, be, c0):
    """al * opa @ opb + be * c0 for integer-valued complex data, exact in int64, as complex128"""
    ar, ai = opa.real.astype(np.int64), opa.imag.astype(np.int64)
    br, bi = opb.real.astype(np.int64), opb.imag.astype(np.int64)
    pr, pi = ar @ br - ai @ bi, ar @ bi + ai @ br
    alr, ali, ber, bei = int(al.real), int(al.imag), int(be.real), int(be.imag)
    cr, ci = c0.real.astype(np.int64), c0.imag.astype(np.int64)
    return (alr * pr - ali * pi + ber * cr - bei * ci) + 1j * (alr * pi + ali * pr + ber * ci + bei * cr)


def gemm_call(L, t, ta, tb, m, n, k, alpha, a, b, beta, c):
    fn, S = (L.GA_Zgemm, DoubleComplex) if t == C_DCPL else (L.GA_Cgemm, SingleComplex)
    fn(ta.encode(), tb.encode(), m, n, k, S(alpha.real, alpha.imag), a.g, b.g, S(beta.real, beta.imag), c.g)


def exact(L, rank, size):
    panel = L.gaamd_ga_gemm_panel()
    m, n, k = 150, 97, 2 * panel + 37
    assert k <= 2100
    for t in (C_DCPL, C_SCPL):
        for ta, tb in (("N", "N"), ("T", "N"), ("C", "N"), ("N", "C")):
            rng = np.random.default_rng(t + 10 * ord(ta) + ord(tb))
            a = GA(L, t, stored_dims(m, k, "N" if ta == "N" else "T"), b"a")
            b = GA(L, t, stored_dims(k, n, "N" if tb == "N" else "T"), b"b")
            c = GA(L, t, [m, n], b"c")
            a.put(ints(rng, a.dims), rank)
            b.put(ints(rng, b.dims), rank)   # random: not Hermitian
            c.put(ints(rng, c.dims), rank)
            gemm_call(L, t, ta, tb, m, n, k, AL_X, a, b, BE_X, c)
            c.model = int_result(AL_X, op(a.model, ta), op(b.model, tb), BE_X, c.model).astype(DT[t])
            tag = f"{'GA_Zgemm' if t == C_DCPL else 'GA_Cgemm'} {ta}{tb}"
            c.check(tag)
            a.check(f"{tag} left a alone")
            b.check(f"{tag} left b alone")
            for x in (a, b, c):
                x.destroy()


def maps(L, rank, size):
    """three irregular maps that differ; patches shifted inside larger arrays"""
    t = C_DCPL
    m, n, k = 61, 45, 83
    for ta, tb in (("N", "N"), ("C", "T")):
        rng = np.random.default_rng(10 * ord(ta) + ord(tb))
        sa, sb = "N" if ta == "N" else "T", "N" if tb == "N" else "T"
        ad, bd, cd = [r + 9 for r in stored_dims(m, k, sa)], [r + 11 for r in stored_dims(k, n, sb)], [m + 7, n + 6]
        # A cut along its rows, B along its columns, C along its rows with (2, 3 ranks) a
        # block of a single row inside the patch
        a = GA(L, t, ad, b"a", irreg=([size, 1], [0, 20, 50][:size] + [0]))
        b = GA(L, t, bd, b"b", irreg=([1, size], [0] + [0, 13, 30][:size]))
        c = GA(L, t, cd, b"c", irreg=([size, 1], cuts(size, 30) + [0]))
        if size == 3:
            lo, hi = (ctypes.c_int * 2)(), (ctypes.c_int * 2)()
            L.NGA_Distribution(c.g, 1, lo, hi)
            assert hi[0] - lo[0] == 0, (list(lo), list(hi))   # rank 1 owns one row of C
        a.put(ints(rng, ad), rank)
        b.put(ints(rng, bd), rank)
        c.put(ints(rng, cd), rank)
        alo, blo, clo = [4, 3], [5, 6], [2, 3]
        ash, bsh = stored_dims(m, k, sa), stored_dims(k, n, sb)
        ahi = [alo[0] + ash[0] - 1, alo[1] + ash[1] - 1]
        bhi = [blo[0] + bsh[0] - 1, blo[1] + bsh[1] - 1]
        chi = [clo[0] + m - 1, clo[1] + n - 1]
        al, be = np.array([AL_X], dtype=DT[t]), np.array([BE_X], dtype=DT[t])
        L.NGA_Matmul_patch(ta.encode(), tb.encode(), vp(al), vp(be), a.g, ia(alo), ia(ahi), b.g, ia(blo), ia(bhi),
                           c.g, ia(clo), ia(chi))
        pa = a.model[alo[0]:ahi[0] + 1, alo[1]:ahi[1] + 1]
        pb = b.model[blo[0]:bhi[0] + 1, blo[1]:bhi[1] + 1]
        sc = (slice(clo[0], chi[0] + 1), slice(clo[1], chi[1] + 1))
        c.model[sc] = int_result(AL_X, op(pa, ta), op(pb, tb), BE_X, c.model[sc]).astype(DT[t])
        c.check(f"NGA_Matmul_patch {ta}{tb} (outside clo:chi unchanged)")
        a.check("a unchanged")
        b.check("b unchanged")
        for x in (a, b, c):
            x.destroy()
    if size == 2:
        # two ranks: the second one's block of C is the single last row of the patch
        a, b = GA(L, t, [30, 40], b"a"), GA(L, t, [30, 20], b"b")
        c = GA(L, t, [40, 20], b"c", irreg=([2, 1], [0, 39, 0]))
        rng = np.random.default_rng(3)
        a.put(ints(rng, a.dims), rank)
        b.put(ints(rng, b.dims), rank)
        c.put(ints(rng, c.dims), rank)
        gemm_call(L, t, "C", "N", 40, 20, 30, AL_X, a, b, BE_X, c)
        c.model = int_result(AL_X, op(a.model, "C"), b.model, BE_X, c.model).astype(DT[t])
        c.check("GA_Zgemm with a one-row block of C")
        for x in (a, b, c):
            x.destroy()


def bits(L, rank, size):
    panel = L.gaamd_ga_gemm_panel()
    al, be = 0.7071067811865476 - 0.4j, -1.3 + 0.6j
    for t, name in ((C_DCPL, "dcp"), (C_SCPL, "cpl")):
        for ta, tb in (("N", "N"), ("C", "N"), ("N", "C")):
            m, n, k = 139, 101, panel + 211
            rng = np.random.default_rng(t + ord(ta) + 3 * ord(tb))
            starts = [0, 41, 90][:size]
            a = GA(L, t, stored_dims(m, k, "N" if ta == "N" else "T"), b"a")
            b = GA(L, t, stored_dims(k, n, "N" if tb == "N" else "T"), b"b", irreg=([size, 1], starts + [0]))
            c = GA(L, t, [m, n], b"c")
            a.put(uniform(rng, a.dims), rank)
            b.put(uniform(rng, b.dims), rank)
            c.put(uniform(rng, c.dims), rank)
            gemm_call(L, t, ta, tb, m, n, k, al, a, b, be, c)
            got = c.get()
            ref = complex(DT[t].type(al)) * (op(a.model, ta).astype(np.complex128) @ op(b.model, tb).astype(np.complex128)) \
                + complex(DT[t].type(be)) * c.model.astype(np.complex128)
            # far looser than the kernel test's bound: only that it is the product at all
            assert np.max(np.abs(got.astype(np.complex128) - ref)) < (1e-9 if t == C_DCPL else 2e-2), "not the product"
            print(f"ZGEMM {name}-{ta}{tb} {hashlib.sha256(got.tobytes()).hexdigest()}", flush=True)
            for x in (a, b, c):
                x.destroy()


def aborts(L, rank, size, mode):
    assert mode == "abort-dgemm-c"
    a, b, c = GA(L, C_DBL, [12, 10], b"a"), GA(L, C_DBL, [12, 8], b"b"), GA(L, C_DBL, [10, 8], b"c")
    print("ABORT EXPECTED", flush=True)
    L.GA_Dgemm(b"C", b"N", 10, 8, 12, 1.0, a.g, b.g, 0.0, c.g)
    print("NOT REACHED", flush=True)


if __name__ == "__main__":
    run([("exact", exact), ("maps", maps), ("bits", bits)], aborts, check_live=True)
