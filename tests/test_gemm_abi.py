"""CPU: the argument checks of gaamd_gemm / gaamd_gemm_plan, the plan's tile grid and
the overlap rule.  Every code here is returned before anything is launched, so no
device is needed (the addresses are never dereferenced)."""
import ctypes

import numpy as np
import pytest

import ga_amd

DBL, FLT = ga_amd.COMEX_ACC_DBL, ga_amd.COMEX_ACC_FLT
BASE = 0x7F0000000000   # an address-shaped number; never read
A, B, C = BASE + (1 << 36), BASE + (2 << 36), BASE

# the codes of include/ga_amd.h
E_COUNT, E_OP, E_SCALAR, E_LD, E_ALIGN, E_OVERLAP = -3, -4, -5, -6, -8, -11


def both(op, ta, tb, m, n, k, lda, ldb, ldc, a=A, b=B, c=C, alpha=1.0, beta=1.0):
    """the plan's code; where that means no launch (an error, or 1: nothing to do) the
    entry point itself is called too and must agree.  A geometry that would launch is
    never handed to the entry point: the addresses are not memory."""
    prc, plan = ga_amd.gemm_plan(op, ta, tb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc)
    if prc != 0:
        rc = ga_amd.gemm(op, ta, tb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc)
        assert rc == (0 if prc == 1 else prc), (rc, prc)
    return prc


@pytest.mark.parametrize("op", [DBL, FLT])
@pytest.mark.parametrize("mnk", [(-1, 4, 4), (4, -1, 4), (4, 4, -1), (-5, -5, -5)])
def test_negative_extent(op, mnk):
    assert both(op, "N", "N", *mnk, 8, 8, 8) == E_COUNT


@pytest.mark.parametrize("op", [0, 1, 37, 40, 41, 42, 1004])
def test_op_other_than_dbl_flt(op):
    L = ga_amd.lib()
    v = np.ones(2)
    vp = v.ctypes.data_as(ctypes.c_void_p)
    plan = (ctypes.c_longlong * 6)()
    args = (op, ord("N"), ord("N"), 4, 4, 4, vp, ctypes.c_void_p(A), 4, ctypes.c_void_p(B), 4, vp, ctypes.c_void_p(C), 4)
    assert L.gaamd_gemm(*args, None) == E_OP
    assert L.gaamd_gemm_plan(*args, plan) == E_OP


@pytest.mark.parametrize("ta,tb", [("X", "N"), ("N", "C"), ("c", "n"), (0, "N"), ("N", 1)])
def test_trans_other_than_n_t(ta, tb):
    assert both(DBL, ta, tb, 4, 4, 4, 4, 4, 4) == E_OP


@pytest.mark.parametrize("ta", "NnTt")
@pytest.mark.parametrize("tb", "NnTt")
def test_every_spelling_of_trans_is_taken(ta, tb):
    assert ga_amd.gemm_plan(FLT, ta, tb, 4, 4, 4, 1.0, A, 4, B, 4, 1.0, C, 4)[0] == 0


def test_missing_scalar():
    for alpha, beta in ((None, 1.0), (1.0, None), (None, None)):
        assert ga_amd.gemm(DBL, "N", "N", 4, 4, 4, alpha, A, 4, B, 4, beta, C, 4) == E_SCALAR
        assert ga_amd.gemm_plan(DBL, "N", "N", 4, 4, 4, alpha, A, 4, B, 4, beta, C, 4)[0] == E_SCALAR


def test_ld_below_the_stored_row():
    m, n, k = 5, 7, 9
    # as stored: A m x k or k x m, B k x n or n x k, C m x n
    rows = {("N", "a"): k, ("T", "a"): m, ("N", "b"): n, ("T", "b"): k}
    for ta in "NT":
        for tb in "NT":
            la, lb = rows[ta, "a"], rows[tb, "b"]
            # m = n = 0 would end in "nothing to do" only after the checks
            assert ga_amd.gemm_plan(DBL, ta, tb, m, n, k, 1.0, A, la, B, lb, 1.0, C, n)[0] == 0
            assert both(DBL, ta, tb, m, n, k, la - 1, lb, n) == E_LD
            assert both(DBL, ta, tb, m, n, k, la, lb - 1, n) == E_LD
            assert both(DBL, ta, tb, m, n, k, la, lb, n - 1) == E_LD


def test_base_below_element_alignment():
    for op, off in ((DBL, 4), (DBL, 1), (FLT, 2), (FLT, 1)):
        assert both(op, "N", "N", 4, 4, 4, 4, 4, 4, a=A + off) == E_ALIGN
        assert both(op, "N", "N", 4, 4, 4, 4, 4, 4, b=B + off) == E_ALIGN
        assert both(op, "N", "N", 4, 4, 4, 4, 4, 4, c=C + off) == E_ALIGN
    # element alignment is enough: 8 for f64, 4 for f32
    assert ga_amd.gemm_plan(DBL, "N", "N", 4, 4, 4, 1.0, A + 8, 4, B + 24, 4, 1.0, C + 8, 4)[0] == 0
    assert ga_amd.gemm_plan(FLT, "N", "N", 4, 4, 4, 1.0, A + 4, 4, B + 12, 4, 1.0, C + 4, 4)[0] == 0


@pytest.mark.parametrize("op", [DBL, FLT])
@pytest.mark.parametrize("mnk", [(0, 5, 5), (5, 0, 5), (0, 0, 0), (0, 5, 0)])
def test_empty_c_is_success_without_a_launch(op, mnk):
    """no device here: a launch would fail, 0 shows there was none"""
    m, n, k = mnk
    assert ga_amd.gemm(op, "N", "N", m, n, k, 1.0, A, 8, B, 8, 1.0, C, 8) == 0
    assert ga_amd.gemm_plan(op, "N", "N", m, n, k, 1.0, A, 8, B, 8, 1.0, C, 8)[0] == 1


@pytest.mark.parametrize("op", [DBL, FLT])
def test_plan_gives_the_tiles_and_the_grid(op):
    rc, p0 = ga_amd.gemm_plan(op, "N", "N", 1, 1, 1, 1.0, A, 1, B, 1, 1.0, C, 1)
    assert rc == 0
    tm, tn, tk = p0["tm"], p0["tn"], p0["tk"]
    assert tm >= 16 and tn >= 16 and tk >= 4
    assert (p0["grid_m"], p0["grid_n"], p0["ksteps"]) == (1, 1, 1)
    ceil = lambda x, t: -(-x // t)   # noqa: E731
    for m in (1, tm - 1, tm, tm + 1, 2 * tm, 2 * tm + 3):
        for n in (1, tn - 1, tn, tn + 1, 2 * tn + 3):
            for k in (1, tk - 1, tk, tk + 1, 2 * tk + 3):
                for ta, tb in (("N", "N"), ("T", "T")):
                    big = max(m, n, k)
                    rc, p = ga_amd.gemm_plan(op, ta, tb, m, n, k, 1.0, A, big, B, big, 1.0, C, big)
                    assert rc == 0
                    assert (p["tm"], p["tn"], p["tk"]) == (tm, tn, tk)
                    assert (p["grid_m"], p["grid_n"], p["ksteps"]) == (ceil(m, tm), ceil(n, tn), ceil(k, tk)), (m, n, k)
    # k = 0 is legal: no k steps (the call scales C)
    rc, p = ga_amd.gemm_plan(op, "N", "N", 5, 5, 0, 1.0, A, 5, B, 5, 1.0, C, 5)
    assert rc == 0 and p["ksteps"] == 0


def test_overlap_is_judged_on_byte_spans():
    """ga_amd.h: first stored element to last.  C exactly A overlaps; C inside B's ld
    padding (no element shared) overlaps; C beginning where A's last element ends does
    not; A and B may overlap each other freely."""
    m, n, k, es = 6, 5, 4, 8
    # C exactly A (m x k stored with ld 8, C m x n with ld 8)
    assert both(DBL, "N", "N", m, n, k, 8, 8, 8, a=C) == E_OVERLAP
    assert both(DBL, "N", "N", m, n, k, 8, 8, 8, b=C) == E_OVERLAP
    # A's span is ((m - 1) * lda + k) elements: C adjacent after it, and A adjacent after C
    a_span = ((m - 1) * 8 + k) * es
    c_span = ((m - 1) * 8 + n) * es
    assert both(DBL, "N", "N", m, n, k, 8, 8, 8, a=C - a_span) == 0
    assert both(DBL, "N", "N", m, n, k, 8, 8, 8, a=C + c_span) == 0
    # one element closer on either side: the last byte of one meets the first of the other
    assert both(DBL, "N", "N", m, n, k, 8, 8, 8, a=C - a_span + es) == E_OVERLAP
    assert both(DBL, "N", "N", m, n, k, 8, 8, 8, a=C + c_span - es) == E_OVERLAP
    # C in the padding of B's rows: B is k x n with ld 16, C is m x 2 with ld 16, eight
    # columns to the right of B's elements -- no element shared, the spans interleave
    assert both(DBL, "N", "N", 3, 2, k, 8, 16, 16, b=C - 8 * es) == E_OVERLAP
    # transposed operands: the span follows the stored shape (A is k x m)
    at_span = ((k - 1) * 8 + m) * es
    assert both(DBL, "T", "N", m, n, k, 8, 8, 8, a=C - at_span) == 0
    assert both(DBL, "T", "N", m, n, k, 8, 8, 8, a=C - at_span + es) == E_OVERLAP
    # A and B are only read
    assert both(DBL, "N", "N", m, n, k, 8, 8, 8, a=A, b=A) == 0
    assert both(FLT, "N", "N", m, n, k, 8, 8, 8, a=A, b=A + 4) == 0


@pytest.mark.parametrize("op", [DBL, FLT])
@pytest.mark.parametrize("vec", [False, True], ids=["odd", "vec"])
def test_far_leading_dimensions_plan_like_compact_ones(op, vec):
    """the leading dimensions of tests/test_gpu_far_offsets.py (an operand's rows spread
    over 9 GiB) on each operand in turn: accepted, with the tiles and the grid of compact
    ones; the operands are 64 GiB apart, so no span meets another"""
    from test_gpu_far_offsets import far_ld, stored_shape
    es = 8 if op == DBL else 4
    rc, p0 = ga_amd.gemm_plan(op, "N", "N", 1, 1, 1, 1.0, A, 1, B, 1, 1.0, C, 1)
    m, n, k = p0["tm"] + 1, p0["tn"] + 1, p0["tk"] + 1
    for ta in "NT":
        for tb in "NT":
            ld = {w: stored_shape(w, ta, tb, m, n, k)[1] + 5 for w in "ABC"}
            rc, compact = ga_amd.gemm_plan(op, ta, tb, m, n, k, 2.0, A, ld["A"], B, ld["B"], -3.0, C, ld["C"])
            assert rc == 0 and (compact["grid_m"], compact["grid_n"], compact["ksteps"]) == (2, 2, 2)
            for which in "ABC":
                rows = stored_shape(which, ta, tb, m, n, k)[0]
                big = dict(ld)
                big[which] = far_ld(rows, es, vec)
                assert (rows - 1) * big[which] * es >= 9 << 30 and (big[which] * es % 16 == 0) == vec
                rc, p = ga_amd.gemm_plan(op, ta, tb, m, n, k, 2.0, A, big["A"], B, big["B"], -3.0, C, big["C"])
                assert rc == 0 and p == compact, (ta, tb, which, p, compact)
