"""CPU: the argument checks of gaamd_patch_fill / _scale / _add / _dot and the
overlap rule of gaamd_patch_add.  Every code here is returned before anything is
launched, so no device is needed (the addresses are never dereferenced)."""
import ctypes

import numpy as np
import pytest

import ga_amd

DBL, FLT, DCP = ga_amd.COMEX_ACC_DBL, ga_amd.COMEX_ACC_FLT, ga_amd.COMEX_ACC_DCP
OPS = sorted(ga_amd.OP_DTYPE)
BASE = 0x7F0000000000   # an address-shaped number; never read

# the codes of include/ga_amd.h
E_NDIM, E_COUNT, E_OP, E_SCALAR, E_STRIDE, E_ALIGN, E_OVERLAP = -2, -3, -4, -5, -6, -8, -11


def calls(op, count, stride, base=BASE):
    """the four entry points on one geometry (the operands far apart)"""
    one = 1
    return {
        "fill": ga_amd.patch_fill(op, one, base, stride, count),
        "scale": ga_amd.patch_scale(op, one, base, stride, count),
        "add": ga_amd.patch_add(op, one, base + (1 << 36), stride, one, base + (2 << 36), stride, base, stride, count),
        "dot": ga_amd.patch_dot(op, base, stride, base + (1 << 36), stride, count)[0],
    }


@pytest.mark.parametrize("ndim", [0, 8, -1])
def test_ndim_outside_1_to_7(ndim):
    L = ga_amd.lib()
    ll = ga_amd.ll_array
    v = np.ones(2)
    vp = v.ctypes.data_as(ctypes.c_void_p)
    cnt, st = ll([2] * 8), ll([64] * 8)
    p = ctypes.c_void_p(BASE)
    assert L.gaamd_patch_fill(DBL, vp, p, st, cnt, ndim, None) == E_NDIM
    assert L.gaamd_patch_scale(DBL, vp, p, st, cnt, ndim, None) == E_NDIM
    assert L.gaamd_patch_add(DBL, vp, p, st, vp, p, st, p, st, cnt, ndim, None) == E_NDIM
    assert L.gaamd_patch_dot(DBL, p, st, p, st, cnt, ndim, vp, None) == E_NDIM


@pytest.mark.parametrize("op", [0, 1, 36, 43, 1004])
def test_unknown_op(op):
    L = ga_amd.lib()
    ll = ga_amd.ll_array
    v = np.ones(2)
    vp = v.ctypes.data_as(ctypes.c_void_p)
    cnt, st = ll([4, 4]), ll([64])
    p = ctypes.c_void_p(BASE)
    assert L.gaamd_patch_fill(op, vp, p, st, cnt, 2, None) == E_OP
    assert L.gaamd_patch_scale(op, vp, p, st, cnt, 2, None) == E_OP
    assert L.gaamd_patch_add(op, vp, p, st, vp, p, st, p, st, cnt, 2, None) == E_OP
    assert L.gaamd_patch_dot(op, p, st, p, st, cnt, 2, vp, None) == E_OP


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("count", [[-1], [4, -2], [4, 0, -1]])
def test_negative_count(op, count):
    got = calls(op, count, [64, 4096][:len(count) - 1])
    assert set(got.values()) == {E_COUNT}, got


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("count", [[0], [4, 0], [0, 5, 3], [3, 1, 1, 1, 1, 1, 0]])
def test_zero_count_is_success_without_a_launch(op, count):
    """no device here: a launch would fail, 0 shows there was none"""
    strides = [64 << (3 * j) for j in range(len(count) - 1)]
    got = calls(op, count, strides)
    assert set(got.values()) == {0}, got
    rc, out = ga_amd.patch_dot(op, BASE, strides, BASE + (1 << 36), strides, count)
    assert rc == 0 and out[0] == 0   # the sum of nothing


def test_missing_strides_and_scalars():
    L = ga_amd.lib()
    ll = ga_amd.ll_array
    v = np.ones(2)
    vp = v.ctypes.data_as(ctypes.c_void_p)
    p = ctypes.c_void_p(BASE)
    cnt, st = ll([4, 4]), ll([64])
    assert L.gaamd_patch_fill(DBL, vp, p, None, cnt, 2, None) == E_STRIDE
    assert L.gaamd_patch_dot(DBL, p, st, p, None, cnt, 2, vp, None) == E_STRIDE
    assert L.gaamd_patch_fill(DBL, None, p, st, cnt, 2, None) == E_SCALAR
    assert L.gaamd_patch_scale(DBL, None, p, st, cnt, 2, None) == E_SCALAR
    assert L.gaamd_patch_add(DBL, vp, p, st, None, p, st, p, st, cnt, 2, None) == E_SCALAR
    assert L.gaamd_patch_dot(DBL, p, st, p, st, cnt, 2, None, None) == E_SCALAR


def test_bases_below_dword_alignment_are_refused():
    assert ga_amd.patch_fill(DBL, 1.0, BASE + 2, [], [8]) == E_ALIGN
    assert ga_amd.patch_scale(FLT, 1.0, BASE + 1, [], [8]) == E_ALIGN
    assert ga_amd.patch_add_plan(DBL, BASE + 4, [62], BASE + (1 << 36), [64], BASE + (2 << 36), [64], [4, 4])[0] == E_ALIGN


def test_plan_merges_contiguous_levels_and_picks_the_width():
    far1, far2 = BASE + (1 << 36), BASE + (2 << 36)
    # a whole 3-D block of f64: one row of 16-byte vectors
    rc, p = ga_amd.patch_add_plan(DBL, far1, [80, 800], far2, [80, 800], BASE, [80, 800], [10, 10, 10])
    assert rc == 0 and p == {"width": 16, "levels": 0, "rows": 1, "nvec": 500}
    # a leading dimension larger than the row: rows stay; 7 f64 = 56 B rows -> 8-byte vectors
    rc, p = ga_amd.patch_add_plan(DBL, far1, [80], far2, [80], BASE, [80], [7, 5])
    assert rc == 0 and p == {"width": 8, "levels": 1, "rows": 5, "nvec": 7}
    # count-1 dimensions are dropped, the outer two merge (stride[2] = 3 * stride[1])
    rc, p = ga_amd.patch_add_plan(FLT, far1, [64, 64, 192], far2, [64, 64, 192], BASE, [64, 64, 192], [4, 1, 3, 2])
    assert rc == 0 and p == {"width": 16, "levels": 1, "rows": 6, "nvec": 1}
    # bases 4 bytes off: f64 moves one element per vector at dword alignment, dcomplex too
    rc, p = ga_amd.patch_add_plan(DBL, far1 + 4, [], far2 + 4, [], BASE + 4, [], [17])
    assert rc == 0 and p["width"] == 8 and p["nvec"] == 17
    rc, p = ga_amd.patch_add_plan(DCP, far1 + 8, [], far2 + 8, [], BASE + 8, [], [5])
    assert rc == 0 and p["width"] == 16 and p["nvec"] == 5
    # differing strides between operands: no merge
    rc, p = ga_amd.patch_add_plan(DBL, far1, [80], far2, [96], BASE, [80], [10, 4])
    assert rc == 0 and p["levels"] == 1 and p["rows"] == 4


def test_add_accepts_exact_aliasing():
    far = BASE + (1 << 36)
    for cnt, st in (([100], []), ([7, 5], [80]), ([4, 3, 2], [64, 256])):
        # c is a
        assert ga_amd.patch_add_plan(DBL, BASE, st, far, st, BASE, st, cnt)[0] == 0
        # c is b
        assert ga_amd.patch_add_plan(DBL, far, st, BASE, st, BASE, st, cnt)[0] == 0
        # c is both
        assert ga_amd.patch_add_plan(DBL, BASE, st, BASE, st, BASE, st, cnt)[0] == 0
    # a and b may overlap each other freely (both only read)
    assert ga_amd.patch_add_plan(DBL, far, [], far + 8, [], BASE, [], [100])[0] == 0


def test_add_rejects_partial_overlap():
    far = BASE + (1 << 36)
    # shifted by one element
    assert ga_amd.patch_add_plan(DBL, BASE + 8, [], far, [], BASE, [], [100])[0] == E_OVERLAP
    assert ga_amd.patch_add_plan(DBL, far, [], BASE - 8, [], BASE, [], [100])[0] == E_OVERLAP
    # the same base with another leading dimension
    assert ga_amd.patch_add_plan(DBL, BASE, [96], far, [80], BASE, [80], [7, 5])[0] == E_OVERLAP
    # the last byte of a meets the first of c
    assert ga_amd.patch_add_plan(DBL, BASE - 792, [], far, [], BASE, [], [100])[0] == E_OVERLAP
    # adjacent is fine
    assert ga_amd.patch_add_plan(DBL, BASE - 800, [], far, [], BASE, [], [100])[0] == 0
    assert ga_amd.patch_add_plan(DBL, BASE + 800, [], far, [], BASE, [], [100])[0] == 0
    # the entry point itself returns the code, before any launch
    assert ga_amd.patch_add(DBL, 1.0, BASE + 8, [], 1.0, far, [], BASE, [], [100]) == E_OVERLAP
    assert ga_amd.patch_add(DBL, 1.0, BASE, [96], 1.0, far, [80], BASE, [80], [7, 5]) == E_OVERLAP


@pytest.mark.parametrize("op", [DBL, FLT, DCP])
def test_far_strides_plan_like_compact_ones(op):
    """the strides of tests/test_gpu_far_offsets.py (rows 2 GiB + 48 apart) on a, b and c
    in turn: accepted, with the vector width, levels, rows and vectors a row of the same
    counts at compact strides (where those do not merge levels)"""
    from test_gpu_far_offsets import PATCH_SHAPES
    es = ga_amd.OP_DTYPE[op].itemsize
    far1, far2 = BASE + (1 << 36), BASE + (2 << 36)
    for count, stride in PATCH_SHAPES:
        for off in ((0, 4) if op == FLT else (0,)):
            # compact, with padding after every row and plane so that no levels merge
            pad = [(count[0] + 4) * es]
            for c in count[1:-1]:
                pad.append(pad[-1] * (c + 1))
            rc, compact = ga_amd.patch_add_plan(op, far1 + off, pad, far2 + off, pad, BASE + off, pad, count)
            assert rc == 0 and compact["levels"] == len(count) - 1, compact
            for which in range(3):
                st = [stride if w == which else pad for w in range(3)]
                rc, p = ga_amd.patch_add_plan(op, far1 + off, st[0], far2 + off, st[1], BASE + off, st[2], count)
                assert rc == 0 and p == compact, (count, which, p, compact)
