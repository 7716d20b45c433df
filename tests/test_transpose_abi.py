"""CPU: the symbols of the transpose work, the argument checks of gaamd_transpose /
gaamd_transpose_acc / gaamd_transpose_plan, the plan's tile grid and the overlap rule.
Every code here is returned before anything is launched, so no device is needed (the
addresses are never dereferenced)."""
import ctypes

import pytest

import ga_amd

INT, DBL, FLT = ga_amd.COMEX_ACC_INT, ga_amd.COMEX_ACC_DBL, ga_amd.COMEX_ACC_FLT
CPL, DCP, LNG = ga_amd.COMEX_ACC_CPL, ga_amd.COMEX_ACC_DCP, ga_amd.COMEX_ACC_LNG
ESZ = {INT: 4, DBL: 8, FLT: 4, CPL: 8, DCP: 16, LNG: 8}
BASE = 0x7F0000000000   # an address-shaped number; never read
SRC, DST = BASE + (1 << 36), BASE

# the codes of include/ga_amd.h
E_COUNT, E_OP, E_SCALAR, E_LD, E_RANGE, E_ALIGN, E_OVERLAP = -3, -4, -5, -6, -7, -8, -11


def both(op, rows, cols, lds, ldd, src=SRC, dst=DST):
    """the plan's code; where that means no launch (an error, or 1: nothing to do) the
    entry point itself is called too and must agree.  A geometry that would launch is
    never handed to the entry point: the addresses are not memory."""
    prc, plan = ga_amd.transpose_plan(op, rows, cols, src, lds, dst, ldd)
    if prc != 0:
        rc = ga_amd.transpose(op, rows, cols, src, lds, dst, ldd)
        assert rc == (0 if prc == 1 else prc), (rc, prc)
    return prc


def test_the_five_symbols_exist():
    L = ga_amd.lib()
    for name in ("gaamd_transpose", "gaamd_transpose_acc", "gaamd_transpose_plan", "GA_Transpose", "GA_Symmetrize"):
        assert getattr(L, name) is not None, name
        assert name in ga_amd._lib.SIGNATURES


@pytest.mark.parametrize("op", sorted(ESZ))
def test_plan_gives_the_tiles_and_the_grid(op):
    rc, p0 = ga_amd.transpose_plan(op, 1, 1, SRC, 1, DST, 1)
    assert rc == 0
    tr, tc = p0["tile_rows"], p0["tile_cols"]
    # a tile row is a contiguous run of at least 128 bytes on either side, and fits LDS
    assert tr * ESZ[op] >= 128 and tc * ESZ[op] >= 128 and tr * tc * ESZ[op] <= 64 * 1024
    assert (p0["grid_rows"], p0["grid_cols"]) == (1, 1)
    ceil = lambda x, t: -(-x // t)   # noqa: E731
    for rows in (1, tr - 1, tr, tr + 1, 2 * tr + 1):
        for cols in (1, tc - 1, tc, tc + 1, 2 * tc + 1):
            rc, p = ga_amd.transpose_plan(op, rows, cols, SRC, cols, DST, rows)
            assert rc == 0
            assert (p["tile_rows"], p["tile_cols"]) == (tr, tc)
            assert (p["grid_rows"], p["grid_cols"]) == (ceil(rows, tr), ceil(cols, tc)), (rows, cols)


def test_one_tile_size_per_element_size():
    t = {op: ga_amd.transpose_plan(op, 1, 1, SRC, 1, DST, 1)[1]["tile_rows"] for op in ESZ}
    assert t[INT] == t[FLT] and t[DBL] == t[CPL] == t[LNG]


@pytest.mark.parametrize("op", sorted(ESZ))
@pytest.mark.parametrize("rc_", [(0, 5), (5, 0), (0, 0)])
def test_zero_extent_is_success_without_a_launch(op, rc_):
    """no device here: a launch would fail, 0 shows there was none"""
    rows, cols = rc_
    assert ga_amd.transpose_plan(op, rows, cols, SRC, 8, DST, 8)[0] == 1
    assert ga_amd.transpose(op, rows, cols, SRC, 8, DST, 8) == 0
    if op in (DBL, FLT):
        assert ga_amd.transpose_acc(op, rows, cols, 0.5, SRC, 8, DST, 8) == 0


@pytest.mark.parametrize("op", [INT, DBL, DCP])
@pytest.mark.parametrize("rc_", [(-1, 4), (4, -1), (-5, -5)])
def test_negative_extent(op, rc_):
    assert both(op, *rc_, 8, 8) == E_COUNT
    assert ga_amd.transpose_acc(DBL, *rc_, 0.5, SRC, 8, DST, 8) == E_COUNT


@pytest.mark.parametrize("op", [0, 1, 36, 43, 1004, -1])
def test_unknown_op(op):
    assert both(op, 4, 4, 4, 4) == E_OP


@pytest.mark.parametrize("op", [0, INT, CPL, DCP, LNG, 43])
def test_acc_takes_only_dbl_and_flt(op):
    half = (ctypes.c_double * 2)(0.5, 0.0)
    rc = ga_amd.lib().gaamd_transpose_acc(op, 4, 4, half, ctypes.c_void_p(SRC), 4, ctypes.c_void_p(DST), 4, None)
    assert rc == E_OP


def test_acc_alpha_missing():
    for op in (DBL, FLT):
        assert ga_amd.transpose_acc(op, 4, 4, None, SRC, 4, DST, 4) == E_SCALAR


def test_ld_below_the_stored_row():
    rows, cols = 5, 7   # src rows of 7, dst rows of 5
    for op in (INT, DBL, DCP):
        assert ga_amd.transpose_plan(op, rows, cols, SRC, cols, DST, rows)[0] == 0
        assert both(op, rows, cols, cols - 1, rows) == E_LD
        assert both(op, rows, cols, cols, rows - 1) == E_LD
    # acc: c is m x n (rows of n), b is n x m (rows of m)
    m, n = 5, 7
    assert ga_amd.transpose_acc(DBL, m, n, 0.5, SRC, m - 1, DST, n) == E_LD
    assert ga_amd.transpose_acc(DBL, m, n, 0.5, SRC, m, DST, n - 1) == E_LD


def test_base_below_element_alignment():
    for op, off in ((INT, 2), (INT, 1), (DBL, 2), (DBL, 4), (DCP, 2), (DCP, 8)):
        assert both(op, 4, 4, 4, 4, src=SRC + off) == E_ALIGN
        assert both(op, 4, 4, 4, 4, dst=DST + off) == E_ALIGN
    assert ga_amd.transpose_acc(FLT, 4, 4, 0.5, SRC + 2, 4, DST, 4) == E_ALIGN
    assert ga_amd.transpose_acc(FLT, 4, 4, 0.5, SRC, 4, DST + 2, 4) == E_ALIGN
    # element alignment is enough
    for op in (INT, DBL, DCP):
        assert ga_amd.transpose_plan(op, 4, 4, SRC + ESZ[op], 4, DST + 3 * ESZ[op], 4)[0] == 0


def test_two_to_the_31_tiles_or_more():
    rc, p = ga_amd.transpose_plan(DBL, 1, 1, SRC, 1, DST, 1)
    t = p["tile_rows"]
    side = t * (1 << 16)       # 2^16 x 2^16 tiles = 2^32
    lo, far = 1 << 12, 1 << 50   # the spans are 2^47 bytes each: far apart
    assert both(DBL, side, side, side, side, src=lo, dst=far) == E_RANGE
    # 2^15 x 2^15 tiles = 2^30 is in range
    half = t * (1 << 15)
    assert ga_amd.transpose_plan(DBL, half, half, lo, half, far, half)[0] == 0


def test_overlap_is_judged_on_byte_spans():
    """ga_amd.h: first stored element to last.  dst equal to src overlaps; dst inside
    src's ld padding (no element shared) overlaps; dst starting where src's last element
    ends does not."""
    rows, cols, es = 6, 5, 8
    assert both(DBL, rows, cols, 8, 8, src=SRC, dst=SRC) == E_OVERLAP
    s_span = ((rows - 1) * 8 + cols) * es          # src: rows x cols, ld 8
    d_span = ((cols - 1) * 8 + rows) * es          # dst: cols x rows, ld 8
    assert both(DBL, rows, cols, 8, 8, src=SRC, dst=SRC + s_span) == 0
    assert both(DBL, rows, cols, 8, 8, src=SRC, dst=SRC - d_span) == 0
    # one element closer on either side
    assert both(DBL, rows, cols, 8, 8, src=SRC, dst=SRC + s_span - es) == E_OVERLAP
    assert both(DBL, rows, cols, 8, 8, src=SRC, dst=SRC - d_span + es) == E_OVERLAP
    # dst in the padding of src's rows: src is 4 x 3 with ld 16, dst is 3 x 4 with ld 16,
    # eight columns to the right of src's elements -- no element shared, the spans interleave
    assert both(DBL, 4, 3, 16, 16, src=SRC, dst=SRC + 8 * es) == E_OVERLAP
    # the same rule for the accumulating form: c is the destination
    assert ga_amd.transpose_acc(DBL, rows, rows, 0.5, SRC, 8, SRC, 8) == E_OVERLAP
    assert ga_amd.transpose_acc(FLT, 3, 4, 0.5, SRC, 16, SRC + 8 * 4, 16) == E_OVERLAP


@pytest.mark.parametrize("op", [INT, DBL, DCP, FLT])
@pytest.mark.parametrize("vec", [False, True], ids=["odd", "vec"])
def test_far_leading_dimensions_plan_like_compact_ones(op, vec):
    """the leading dimensions of tests/test_gpu_far_offsets.py (T + 1 rows spread over
    9 GiB) on src, then on dst: accepted, with the tiles and the grid of compact ones (the
    plan reports no more than these); the accumulating form takes them up to its launch"""
    from test_gpu_far_offsets import compact_ld, far_ld
    rc, p0 = ga_amd.transpose_plan(op, 1, 1, SRC, 1, DST, 1)
    t = p0["tile_rows"] + 1
    small, big = compact_ld(t, ESZ[op], vec), far_ld(t, ESZ[op], vec)
    assert (t - 1) * big * ESZ[op] >= 9 << 30 and (big * ESZ[op] % 16 == 0) == (vec or ESZ[op] == 16)
    rc, compact = ga_amd.transpose_plan(op, t, t, SRC, small, DST, small)
    assert rc == 0 and (compact["grid_rows"], compact["grid_cols"]) == (2, 2)
    for lds, ldd in ((big, small), (small, big)):
        rc, p = ga_amd.transpose_plan(op, t, t, SRC, lds, DST, ldd)
        assert rc == 0 and p == compact, (lds, ldd, p, compact)
