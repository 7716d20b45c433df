"""CPU: the argument checks of gaamd_patch_elem1 / _elem2 / _select.  Every code here is
returned before anything is launched or allocated, so no device is needed (the addresses
are never dereferenced)."""
import ctypes

import numpy as np
import pytest

import ga_amd

DBL, FLT, DCP = ga_amd.COMEX_ACC_DBL, ga_amd.COMEX_ACC_FLT, ga_amd.COMEX_ACC_DCP
OPS = sorted(ga_amd.OP_DTYPE)
BASE = 0x7F0000000000   # an address-shaped number; never read
FAR1, FAR2 = BASE + (1 << 36), BASE + (2 << 36)

FN1 = [ga_amd.GAAMD_ELEM_ABS, ga_amd.GAAMD_ELEM_ADD_CONST, ga_amd.GAAMD_ELEM_RECIP]
FN2 = [ga_amd.GAAMD_ELEM_MUL, ga_amd.GAAMD_ELEM_DIV, ga_amd.GAAMD_ELEM_MAX, ga_amd.GAAMD_ELEM_MIN]

# the codes of include/ga_amd.h
E_NDIM, E_COUNT, E_OP, E_SCALAR, E_STRIDE, E_ALIGN, E_OVERLAP = -2, -3, -4, -5, -6, -8, -11


def calls(op, count, stride, base=BASE):
    """every fn of the two map entry points and both selects on one geometry"""
    got = {}
    for fn in FN1:
        got[f"elem1-{fn}"] = ga_amd.patch_elem1(op, fn, base, stride, count, scalar=1)
    for fn in FN2:
        got[f"elem2-{fn}"] = ga_amd.patch_elem2(op, fn, base + (1 << 36), stride, base + (2 << 36), stride, base,
                                                stride, count)
    for mx in (0, 1):
        got[f"select-{mx}"] = ga_amd.patch_select(op, mx, base, stride, count)[0]
    return got


def test_constants_match_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ga_amd.h")).read()
    for name in ("GAAMD_ELEM_ABS", "GAAMD_ELEM_ADD_CONST", "GAAMD_ELEM_RECIP", "GAAMD_ELEM_MUL", "GAAMD_ELEM_DIV",
                 "GAAMD_ELEM_MAX", "GAAMD_ELEM_MIN", "GAAMD_ZERO_DIVISOR"):
        m = re.search(rf"#define {name} (\d+)", hdr)
        assert m and int(m.group(1)) == getattr(ga_amd, name), name
    assert ga_amd.GAAMD_ZERO_DIVISOR == 2
    assert len(set(FN1 + FN2)) == 7


@pytest.mark.parametrize("ndim", [0, 8, -1])
def test_ndim_outside_1_to_7(ndim):
    L = ga_amd.lib()
    ll = ga_amd.ll_array
    v = np.ones(4)
    vp = v.ctypes.data_as(ctypes.c_void_p)
    cnt, st = ll([2] * 8), ll([64] * 8)
    idx = ctypes.c_longlong(0)
    p = ctypes.c_void_p(BASE)
    assert L.gaamd_patch_elem1(DBL, FN1[0], vp, p, st, cnt, ndim, None) == E_NDIM
    assert L.gaamd_patch_elem2(DBL, FN2[0], p, st, p, st, p, st, cnt, ndim, None) == E_NDIM
    assert L.gaamd_patch_select(DBL, 0, p, st, cnt, ndim, vp, None, ctypes.byref(idx), None) == E_NDIM


@pytest.mark.parametrize("op", [0, 1, 36, 43, 1004])
def test_unknown_op(op):
    L = ga_amd.lib()
    ll = ga_amd.ll_array
    v = np.ones(4)
    vp = v.ctypes.data_as(ctypes.c_void_p)
    cnt, st = ll([4, 4]), ll([64])
    idx = ctypes.c_longlong(0)
    p, q, r = (ctypes.c_void_p(x) for x in (BASE, FAR1, FAR2))
    for fn in FN1:
        assert L.gaamd_patch_elem1(op, fn, vp, p, st, cnt, 2, None) == E_OP
    for fn in FN2:
        assert L.gaamd_patch_elem2(op, fn, q, st, r, st, p, st, cnt, 2, None) == E_OP
    assert L.gaamd_patch_select(op, 1, p, st, cnt, 2, vp, None, ctypes.byref(idx), None) == E_OP


@pytest.mark.parametrize("op", OPS)
def test_unknown_fn(op):
    """a fn of the other entry point is unknown too"""
    for fn in [0, 8, -1, 100] + FN2:
        assert ga_amd.patch_elem1(op, fn, BASE, [64], [4, 4], scalar=1) == E_OP, fn
    for fn in [0, 8, -1, 100] + FN1:
        assert ga_amd.patch_elem2(op, fn, FAR1, [64], FAR2, [64], BASE, [64], [4, 4]) == E_OP, fn
    # with a count of zero as well: the code, not a silent success
    assert ga_amd.patch_elem1(op, 0, BASE, [64], [4, 0], scalar=1) == E_OP
    assert ga_amd.patch_elem2(op, 0, FAR1, [64], FAR2, [64], BASE, [64], [0, 4]) == E_OP


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("count", [[-1], [4, -2], [4, 0, -1]])
def test_negative_count(op, count):
    got = calls(op, count, [64, 4096][:len(count) - 1])
    assert set(got.values()) == {E_COUNT}, got


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("count", [[0], [4, 0], [0, 5, 3], [3, 1, 1, 1, 1, 1, 0]])
def test_zero_count_without_a_launch(op, count):
    """no device here: a launch (or the flag's allocation) would fail.  The map calls return
    0, RECIP and DIV included; select returns 1 with index -1"""
    strides = [64 << (3 * j) for j in range(len(count) - 1)]
    got = calls(op, count, strides)
    sel = {k: v for k, v in got.items() if k.startswith("select")}
    maps = {k: v for k, v in got.items() if not k.startswith("select")}
    assert set(maps.values()) == {0}, got
    assert set(sel.values()) == {1}, got
    for mx in (0, 1):
        rc, val, key, idx = ga_amd.patch_select(op, mx, BASE, strides, count)
        assert (rc, idx) == (1, -1)
    # ADD_CONST without its scalar on an empty patch: nothing to do, as gaamd_patch_scale
    assert ga_amd.patch_elem1(op, ga_amd.GAAMD_ELEM_ADD_CONST, BASE, strides, count) == 0


def test_missing_strides_scalar_and_results():
    L = ga_amd.lib()
    ll = ga_amd.ll_array
    v = np.ones(4)
    vp = v.ctypes.data_as(ctypes.c_void_p)
    idx = ctypes.c_longlong(0)
    p, q, r = (ctypes.c_void_p(x) for x in (BASE, FAR1, FAR2))
    cnt, st = ll([4, 4]), ll([64])
    for fn in FN1:
        assert L.gaamd_patch_elem1(DBL, fn, vp, p, None, cnt, 2, None) == E_STRIDE
    for fn in FN2:
        assert L.gaamd_patch_elem2(DBL, fn, q, None, r, st, p, st, cnt, 2, None) == E_STRIDE
        assert L.gaamd_patch_elem2(DBL, fn, q, st, r, None, p, st, cnt, 2, None) == E_STRIDE
        assert L.gaamd_patch_elem2(DBL, fn, q, st, r, st, p, None, cnt, 2, None) == E_STRIDE
    assert L.gaamd_patch_select(DBL, 0, p, None, cnt, 2, vp, None, ctypes.byref(idx), None) == E_STRIDE
    # only ADD_CONST needs the scalar
    assert L.gaamd_patch_elem1(DBL, ga_amd.GAAMD_ELEM_ADD_CONST, None, p, st, cnt, 2, None) == E_SCALAR
    # select: the value and the index are required, the key is not (checked before any launch:
    # with a count of zero the call gets past them)
    assert L.gaamd_patch_select(DBL, 0, p, st, cnt, 2, None, None, ctypes.byref(idx), None) == E_SCALAR
    assert L.gaamd_patch_select(DBL, 0, p, st, cnt, 2, vp, None, None, None) == E_SCALAR
    assert L.gaamd_patch_select(DBL, 0, p, st, ll([4, 0]), 2, vp, None, ctypes.byref(idx), None) == 1


def test_bases_below_dword_alignment_are_refused():
    for fn in FN1:
        assert ga_amd.patch_elem1(DBL, fn, BASE + 2, [], [8], scalar=1.0) == E_ALIGN
        assert ga_amd.patch_elem1(FLT, fn, BASE + 1, [], [8], scalar=1.0) == E_ALIGN
    for fn in FN2:
        assert ga_amd.patch_elem2(DBL, fn, FAR1 + 2, [], FAR2, [], BASE, [], [8]) == E_ALIGN
        assert ga_amd.patch_elem2(DBL, fn, FAR1 + 4, [62], FAR2, [64], BASE, [64], [4, 4]) == E_ALIGN
    assert ga_amd.patch_select(FLT, 0, BASE + 3, [], [8])[0] == E_ALIGN
    assert ga_amd.patch_select(DCP, 1, BASE, [66], [2, 2])[0] == E_ALIGN


@pytest.mark.parametrize("fn", FN2)
def test_elem2_partial_overlap_is_refused_and_exact_aliasing_is_not(fn):
    """gaamd_patch_add's rule.  An accepted geometry would go on to launch, which needs a
    device, so acceptance is shown on gaamd_patch_add_plan (the same check, reused) and on
    an empty patch; refusal on the entry point itself"""
    # shifted by one element; the same base with another leading dimension; last byte meets first
    assert ga_amd.patch_elem2(DBL, fn, BASE + 8, [], FAR1, [], BASE, [], [100]) == E_OVERLAP
    assert ga_amd.patch_elem2(DBL, fn, FAR1, [], BASE - 8, [], BASE, [], [100]) == E_OVERLAP
    assert ga_amd.patch_elem2(DBL, fn, BASE, [96], FAR1, [80], BASE, [80], [7, 5]) == E_OVERLAP
    assert ga_amd.patch_elem2(DBL, fn, BASE - 792, [], FAR1, [], BASE, [], [100]) == E_OVERLAP
    for cnt, st in (([100], []), ([7, 5], [80]), ([4, 3, 2], [64, 256])):
        for a, b in ((BASE, FAR1), (FAR1, BASE), (BASE, BASE)):   # c is a, c is b, c is both
            assert ga_amd.patch_add_plan(DBL, a, st, b, st, BASE, st, cnt)[0] == 0
    # the checks run on an empty patch too: exact aliasing passes them, partial overlap of a
    # non-empty patch does not
    assert ga_amd.patch_elem2(DBL, fn, BASE, [80], BASE, [80], BASE, [80], [7, 0]) == 0
