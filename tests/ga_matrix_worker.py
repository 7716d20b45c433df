"""One rank of the GA diagonal / row-column scaling / norm tests
(test_gpu_ga_matrix_mp.py starts 1, 2 or 3 of these on one GPU).

Modes:
  all        the nine calls on REGULAR and irregular block maps, the round trips, the rank
             that owns no diagonal element, the 2-element vector on 3 ranks, the norms --
             each section prints "SECTION <name> OK"
  abort-len  GA_Scale_rows with a g_v one element too long: every rank must end through
             GA_Error; prints "ABORT EXPECTED" just before it and "NOT REACHED" if it returns
Expected values: the numpy restatement of matrix.c in test_gpu_matrix.py, compared as raw bits
by every rank.  Prints "RANK <r> OK" on success and "NORM <case> <hex of the double>" for every
norm, which the launcher compares across ranks and rank counts.
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
import test_gpu_matrix as M  # noqa: E402
from ga_worker import C_DBL, C_DCPL, C_FLOAT, C_INT, C_LONG, C_SCPL, GA, blocks_of, run, vp  # noqa: E402

TYPES = (C_DBL, C_FLOAT, C_INT, C_LONG, C_DCPL)   # one complex type for the scale and diagonal calls
NORM_TYPES = (C_DBL, C_FLOAT, C_INT, C_LONG, C_DCPL, C_SCPL)   # C_SCPL: norm_call's armci_msg_fgop branch
SHAPES = ([37, 53], [53, 37], [40, 40])


def cuts(n, size, shift):
    """`size` block starts over n elements, the interior ones moved by `shift`"""
    return [0] + [min(n - 1, max(1, n * k // size + shift)) for k in range(1, size)]


def matrix(L, t, dims, size, irreg):
    """REGULAR, or cut by rows into `size` uneven blocks"""
    if not irreg:
        return GA(L, t, dims, b"a")
    return GA(L, t, dims, b"a-irreg", irreg=([size, 1], cuts(dims[0], size, 3) + [0]))


def vector(L, t, n, size, irreg):
    """REGULAR, or cut elsewhere than any map above cuts the diagonal"""
    if not irreg:
        return GA(L, t, [n], b"v")
    nb = min(size, n)
    return GA(L, t, [n], b"v-irreg", irreg=([nb], cuts(n, nb, -5)))


def live_unchanged(L, live, what):
    assert L.gaamd_ga_live_arrays() == live, f"{what}: a temporary is still alive"


def call(L, name, *args):
    """one GA call; no temporary array is left behind by it"""
    live = L.gaamd_ga_live_arrays()
    getattr(L, name)(*args)
    live_unchanged(L, live, name)


def diag_calls(L, rank, size, a, v, tag):
    """the five diagonal calls and both round trips on the arrays a (2-D) and v (1-D)"""
    op, dims = a.op, a.dims
    n = min(dims)
    idx = np.arange(n)
    rng = np.random.default_rng(17 * op + dims[0])
    live = L.gaamd_ga_live_arrays()
    a.put(K.gen(op, dims[0] * dims[1], rng), rank)
    v.put(K.gen(op, n, rng), rank)
    call(L, "GA_Add_diagonal", a.g, v.g)
    a.model[idx, idx] = M.ref_diag_add(op, a.model[idx, idx], v.model)
    a.check(f"GA_Add_diagonal {tag}")
    v.check(f"GA_Add_diagonal left v alone {tag}")
    c = K.scalar(op, M.SHIFT_C[op])
    call(L, "GA_Shift_diagonal", a.g, vp(c))
    a.model[idx, idx] = M.ref_diag_add(op, a.model[idx, idx], c)
    a.check(f"GA_Shift_diagonal {tag}")
    # get then set restores the array's bits; set then get returns v's bits
    before = a.model.copy()
    call(L, "GA_Get_diag", a.g, v.g)
    v.model = a.model[idx, idx].copy()
    v.check(f"GA_Get_diag {tag}")
    a.check(f"GA_Get_diag left a alone {tag}")
    call(L, "GA_Zero_diagonal", a.g)
    a.model[idx, idx] = 0
    a.check(f"GA_Zero_diagonal {tag}")
    call(L, "GA_Set_diagonal", a.g, v.g)
    a.model = before
    a.check(f"GA_Get_diag, GA_Set_diagonal restores the bits {tag}")
    w = M.special_values(op, K.gen(op, n, rng))
    v.put(w, rank)
    call(L, "GA_Set_diagonal", a.g, v.g)
    v.put(np.zeros(n, dtype=a.dt), rank)
    call(L, "GA_Get_diag", a.g, v.g)
    v.model = w
    v.check(f"GA_Set_diagonal, GA_Get_diag returns v's bits {tag}")
    live_unchanged(L, live, tag)


def scale_calls(L, rank, size, a, tag, irreg):
    op, dims = a.op, a.dims
    rng = np.random.default_rng(23 * op + dims[1])
    live = L.gaamd_ga_live_arrays()
    for rows in (True, False):
        v = vector(L, a.t, dims[0] if rows else dims[1], size, irreg)
        a.put(K.gen(op, dims[0] * dims[1], rng), rank)
        v.put(K.gen(op, v.dims[0], rng), rank)
        call(L, "GA_Scale_rows" if rows else "GA_Scale_cols", a.g, v.g)
        a.model = M.ref_scale(op, a.model, v.model, rows)
        a.check(f"GA_Scale_{'rows' if rows else 'cols'} {tag}")
        v.check(f"scale left v alone {tag}")
        v.destroy()
    live_unchanged(L, live, tag)


# ---- sections ---------------------------------------------------------------------
def forms(L, rank, size):
    for dims in SHAPES:
        for t in TYPES:
            for a_irreg in (False, True):
                for v_irreg in (False, True):
                    a = matrix(L, t, dims, size, a_irreg)
                    v = vector(L, t, min(dims), size, v_irreg)
                    tag = f"{ga_amd.OP_NAME[a.op]} {dims} a {'irreg' if a_irreg else 'regular'} v " \
                          f"{'irreg' if v_irreg else 'regular'}"
                    diag_calls(L, rank, size, a, v, tag)
                    scale_calls(L, rank, size, a, tag, v_irreg)
                    a.destroy()
                    v.destroy()


def corners(L, rank, size):
    """a 53 x 7 array split by rows: with 2 ranks or more a rank owns no diagonal element;
    a vector of 2 elements: on 3 ranks a rank owns nothing of it"""
    for t in (C_DBL, C_INT, C_DCPL):
        a = GA(L, t, [53, 7], b"tall", irreg=([size, 1], [0, 30, 45][:size] + [0]))
        if size > 1:
            lo, hi = blocks_of(L, a.g, 2, size)[1]
            assert lo[0] >= 7, (lo, hi)   # its rows lie below the diagonal's last element
        v = GA(L, t, [7], b"v7")
        diag_calls(L, rank, size, a, v, f"{ga_amd.OP_NAME[a.op]} 53 x 7")
        scale_calls(L, rank, size, a, "53 x 7", False)
        a.destroy()
        v.destroy()
        a = GA(L, t, [2, 9], b"flat")
        v = GA(L, t, [2], b"v2")
        if size == 3:
            owners = sum(all(h >= l for l, h in zip(lo, hi)) for lo, hi in blocks_of(L, v.g, 1, size))
            assert owners < size
        diag_calls(L, rank, size, a, v, f"{ga_amd.OP_NAME[a.op]} 2 x 9")
        scale_calls(L, rank, size, a, "2 x 9", False)
        a.destroy()
        v.destroy()


def norm_call(L, a, which):
    nm = ctypes.c_double(-1.0)
    call(L, "GA_Norm1" if which == 1 else "GA_Norm_infinity", a.g, ctypes.byref(nm))
    return nm.value


def norms(L, rank, size):
    live = L.gaamd_ga_live_arrays()
    for dims in SHAPES + ([300], [2]):
        for t in NORM_TYPES:
            for irreg in (False, True):
                if irreg and len(dims) == 1:
                    continue
                a = matrix(L, t, dims, size, irreg) if len(dims) == 2 else GA(L, t, dims, b"a1")
                op = a.op
                n = int(np.prod(dims))
                rng = np.random.default_rng(31 * op + n)
                case = f"{ga_amd.OP_NAME[op]}-{'x'.join(map(str, dims))}-{'irreg' if irreg else 'regular'}"
                x = M.gen_exact(op, n, rng)
                assert M.exactly_summable(op, x)
                a.put(x, rank)
                got = norm_call(L, a, 1)
                want = float(M.ref_norm1_exact(op, x)[0])
                print(f"NORM one-{case} {np.float64(got).tobytes().hex()}", flush=True)
                assert np.float64(got).tobytes() == np.float64(want).tobytes(), (case, got, want)
                y = K.gen(op, n, rng)
                a.put(y, rank)
                got = norm_call(L, a, 0)
                want = float(M.ref_norm_inf(op, y)[0])
                print(f"NORM inf-{case} {np.float64(got).tobytes().hex()}", flush=True)
                assert np.float64(got).tobytes() == np.float64(want).tobytes(), (case, got, want)
                assert norm_call(L, a, 0) == got   # the same bits on every call
                a.check(f"the norms left the array alone {case}")
                a.destroy()
    live_unchanged(L, live, "norms")


def aborts(L, rank, size, mode):
    a = GA(L, C_DBL, [20, 30], b"a")
    v = GA(L, C_DBL, [21], b"v")   # one element too long for the rows
    a.put(np.ones([20, 30]), rank)
    print("ABORT EXPECTED", flush=True)
    L.GA_Scale_rows(a.g, v.g)
    print("NOT REACHED", flush=True)


if __name__ == "__main__":
    run([("forms", forms), ("corners", corners), ("norms", norms)], aborts)
