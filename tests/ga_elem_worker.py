"""One rank of the GA element-wise algebra and NGA_Select_elem tests
(test_gpu_ga_elem_mp.py starts 1, 2 or 3 of these on one GPU).

Modes:
  all         whole-array and patch forms, the general path, NGA_Select_elem -- each
              section prints "SECTION <name> OK"
  abort-zero  GA_Elem_divide with a single zero in g_b: every rank must end through
              GA_Error; prints "ABORT EXPECTED" just before it and "NOT REACHED" if it returns
Expected values: the numpy restatement of elem_alg.c / select.c in test_gpu_ga_elem.py.
Prints "RANK <r> OK" on success and "SEL <case> <value hex> <subscripts>" for every
NGA_Select_elem, which the launcher compares across ranks.
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
import test_gpu_ga_math as K  # noqa: E402
import test_gpu_ga_elem as E  # noqa: E402
from ga_worker import (C_DBL, C_DCPL, C_FLOAT, C_INT, C_LONG, C_SCPL, GA, OP_OF, blocks_of, flat, ia, run,  # noqa: E402
                       sl, vp)

TYPES = (C_INT, C_LONG, C_FLOAT, C_DBL, C_SCPL, C_DCPL)
ELEM2 = {E.MUL: "multiply", E.DIV: "divide", E.MAX: "maximum", E.MIN: "minimum"}


def elem1(L, fn, a, patch=None):
    """one unary call on the GA `a` (whole array or the C patch) and on its model"""
    op = a.op
    al = K.scalar(op, E.CONST[op])
    lohi = () if patch is None else (ia(patch[0]), ia(patch[1]))
    sfx = "" if patch is None else "_patch"
    if fn == E.ABS:
        getattr(L, "GA_Abs_value" + sfx)(a.g, *lohi)
    elif fn == E.ADD_CONST:
        getattr(L, "GA_Add_constant" + sfx)(a.g, *lohi, vp(al))
    else:
        getattr(L, "GA_Recip" + sfx)(a.g, *lohi)
    s = sl(*patch) if patch else tuple(slice(None) for _ in a.dims)
    vals, bad = E.ref_elem1(op, fn, flat(a.model[s]), E.CONST[op])
    assert not bad.any()
    a.model[s] = vals.reshape(a.model[s].shape)


def elem2(L, fn, a, b, c, patches=None):
    """c = fn(a, b) on whole arrays or on the C patches (alo, ahi, blo, bhi, clo, chi)"""
    name = "GA_Elem_" + ELEM2[fn]
    if patches is None:
        getattr(L, name)(a.g, b.g, c.g)
        sa = sb = sc = tuple(slice(None) for _ in c.dims)
    else:
        alo, ahi, blo, bhi, clo, chi = patches
        getattr(L, name + "_patch")(a.g, ia(alo), ia(ahi), b.g, ia(blo), ia(bhi), c.g, ia(clo), ia(chi))
        sa, sb, sc = sl(alo, ahi), sl(blo, bhi), sl(clo, chi)
    vals, bad = E.ref_elem2(a.op, fn, flat(a.model[sa].copy()), flat(b.model[sb].copy()))
    assert not bad.any()
    c.model[sc] = vals.reshape(c.model[sc].shape)


def fresh(op, n, rng):
    x = K.gen(op, n, rng)
    return E.nonzero(op, x)


# ---- sections ---------------------------------------------------------------------
def whole_and_patch(L, rank, size):
    for dims in ([37, 53], [5, 6, 7]):
        n = int(np.prod(dims))
        lo = [1] * len(dims)
        hi = [d - 2 for d in dims]
        for t in TYPES:
            op = OP_OF[t]
            rng = np.random.default_rng(100 * t + len(dims))
            a, b, c = (GA(L, t, dims, nm) for nm in (b"a", b"b", b"c"))
            tag = f"{ga_amd.OP_NAME[op]} {dims}"
            for patch in (None, (lo, hi)):
                where = "whole" if patch is None else "patch"
                for fn in E.FN1:
                    a.put(fresh(op, n, rng), rank)
                    elem1(L, fn, a, patch)
                    a.check(f"{E.FN_NAME[fn]} {where} {tag}")
                for fn in E.FN2:
                    a.put(fresh(op, n, rng), rank)
                    b.put(fresh(op, n, rng), rank)
                    c.put(fresh(op, n, rng), rank)
                    elem2(L, fn, a, b, c, None if patch is None else (lo, hi, lo, hi, lo, hi))
                    c.check(f"{E.FN_NAME[fn]} {where} {tag}")
                    a.check(f"{E.FN_NAME[fn]} {where} left a alone {tag}")
                    b.check(f"{E.FN_NAME[fn]} {where} left b alone {tag}")
            # in place: g_c is g_a, then g_b, then both
            a.put(fresh(op, n, rng), rank)
            b.put(fresh(op, n, rng), rank)
            elem2(L, E.MUL, a, b, a)
            a.check(f"GA_Elem_multiply(g_a, g_b, g_a) {tag}")
            b.check(f"in place left b alone {tag}")
            elem2(L, E.DIV, a, b, b)
            b.check(f"GA_Elem_divide(g_a, g_b, g_b) {tag}")
            elem2(L, E.MAX, a, a, a)
            a.check(f"GA_Elem_maximum(g_a, g_a, g_a) {tag}")
            for x in (a, b, c):
                x.destroy()


def general_path(L, rank, size):
    """a partner on another block map and shifted patches: through temporaries, all destroyed"""
    dims = [37, 53]
    n = dims[0] * dims[1]
    for t in (C_DBL, C_SCPL, C_INT):
        op = OP_OF[t]
        rng = np.random.default_rng(9 * t)
        live0 = L.gaamd_ga_live_arrays()
        a, c = GA(L, t, dims, b"a"), GA(L, t, dims, b"c")
        starts = [0, 10, 30][:size]
        b = GA(L, t, dims, b"irreg", irreg=([size, 1], starts + [0]))
        assert size == 1 or L.GA_Compare_distr(a.g, b.g) == 1
        live = L.gaamd_ga_live_arrays()
        assert live == live0 + 3
        for fn in E.FN2:
            a.put(fresh(op, n, rng), rank)
            b.put(fresh(op, n, rng), rank)
            c.put(fresh(op, n, rng), rank)
            elem2(L, fn, a, b, c)
            c.check(f"{E.FN_NAME[fn]} with g_b on another map")
            a.check("a unchanged")
            b.check("b unchanged")
            # g_c on the other map, in place with g_b
            elem2(L, fn, a, b, b)
            b.check(f"{E.FN_NAME[fn]} into the array on the other map")
            # shifted patches: a's patch against c's, b on c's patch
            alo, ahi, clo, chi = [2, 3], [20, 40], [15, 5], [33, 42]
            b.put(fresh(op, n, rng), rank)
            elem2(L, fn, a, b, c, (alo, ahi, clo, chi, clo, chi))
            c.check(f"{E.FN_NAME[fn]} with a shifted")
            # a shifted patch of c itself
            elem2(L, fn, c, b, c, (alo, ahi, clo, chi, clo, chi))
            c.check(f"{E.FN_NAME[fn]} of a shifted patch of c itself")
            assert L.gaamd_ga_live_arrays() == live, "a temporary of the general path is still alive"
        for x in (a, b, c):
            x.destroy()
        assert L.gaamd_ga_live_arrays() == live0


def select_call(L, a, opname):
    val = np.zeros(1, dtype=a.dt)
    idx = (ctypes.c_int * len(a.dims))()
    L.NGA_Select_elem(a.g, opname, vp(val), idx)
    return val, list(idx)


def select_check(L, a, case):
    """min and max against numpy's first occurrence in C order; SEL lines for the launcher"""
    for want_max, opname in ((0, b"min"), (1, b"max")):
        val, idx = select_call(L, a, opname)
        i, want, _ = E.ref_select(a.op, want_max, flat(a.model))
        want_idx = [int(v) for v in np.unravel_index(i, a.dims)]
        print(f"SEL {case}-{opname.decode()} {val.tobytes().hex()} {idx}", flush=True)
        assert (val.tobytes(), idx) == (want.tobytes(), want_idx), (case, opname, val, idx, want, want_idx)


def select(L, rank, size):
    for dims in ([37, 53], [5, 6, 7]):
        n = int(np.prod(dims))
        for t in TYPES:
            op = OP_OF[t]
            rng = np.random.default_rng(300 * t + len(dims))
            a = GA(L, t, dims, b"a")
            a.put(K.gen(op, n, rng), rank)
            select_check(L, a, f"{ga_amd.OP_NAME[op]}-{len(dims)}d")
            # duplicates of both extrema in every rank's block: the lowest C index wins
            x = E.distinct(op, n, rng).reshape(dims)
            for q, (lo, hi) in enumerate(blocks_of(L, a.g, len(dims), size)):
                if all(h >= l for l, h in zip(lo, hi)):
                    x[tuple(hi)] = E.extreme(op, 1, q)
                    x[tuple(lo)] = E.extreme(op, 0, q)
            a.put(x, rank)
            select_check(L, a, f"{ga_amd.OP_NAME[op]}-{len(dims)}d-dup")
            a.destroy()
    # a tie where the lower row-major index lives on the higher rank: columns 0, 1, .. start
    # a block each, so (1, 0) is rank 0's and (0, 1) the next rank's
    if size > 1:
        dims = [2, size + 2]
        for t in (C_DBL, C_INT, C_DCPL):
            a = GA(L, t, dims, b"tie", irreg=([1, size], [0] + list(range(size))))
            blk = blocks_of(L, a.g, 2, size)
            assert blk[0] == ([0, 0], [1, 0]) and blk[1][0] == [0, 1], blk
            x = E.distinct(a.op, 2 * (size + 2), np.random.default_rng(t)).reshape(dims)
            for want_max, opname in ((1, b"max"), (0, b"min")):
                y = x.copy()
                y[1, 0] = E.extreme(a.op, want_max, 0)
                y[0, 1] = E.extreme(a.op, want_max, 1)
                a.put(y, rank)
                val, idx = select_call(L, a, opname)
                print(f"SEL tie-{ga_amd.OP_NAME[a.op]}-{opname.decode()} {val.tobytes().hex()} {idx}", flush=True)
                assert idx == [0, 1] and val.tobytes() == y[0:1, 1].tobytes(), (opname, idx, val)
            a.destroy()
    # two elements: on three ranks one rank owns nothing
    for t in (C_DBL, C_FLOAT, C_LONG):
        a = GA(L, t, [2], b"two")
        if size == 3:
            owners = sum(all(h >= l for l, h in zip(lo, hi)) for lo, hi in blocks_of(L, a.g, 1, size))
            assert owners < size
        a.put(np.array([3, -4], dtype=a.dt), rank)
        select_check(L, a, f"two-{ga_amd.OP_NAME[a.op]}")
        elem1(L, E.ABS, a)
        a.check("GA_Abs_value of two elements")
        select_check(L, a, f"two-abs-{ga_amd.OP_NAME[a.op]}")
        # -0.0 against +0.0: the first one, with its sign
        if t != C_LONG:
            a.put(np.array([-0.0, 0.0], dtype=a.dt), rank)
            select_check(L, a, f"zeros-{ga_amd.OP_NAME[a.op]}")
        a.destroy()


def aborts(L, rank, size, mode):
    dims = [20, 30]
    a, b, c = (GA(L, C_DBL, dims, nm) for nm in (b"a", b"b", b"c"))
    ones = np.ones(dims)
    a.put(ones, rank)
    y = 2.0 * ones
    y[19, 29] = 0.0   # a single zero, in the last rank's block
    b.put(y, rank)
    print("ABORT EXPECTED", flush=True)
    L.GA_Elem_divide(a.g, b.g, c.g)
    print("NOT REACHED", flush=True)


if __name__ == "__main__":
    run([("forms", whole_and_patch), ("general", general_path), ("select", select)], aborts)
