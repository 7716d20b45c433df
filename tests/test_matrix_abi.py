"""CPU: the argument checks of gaamd_patch_norm / gaamd_diagonal / gaamd_scale_rows /
gaamd_scale_cols, the exported names, and the numpy restatement of matrix.c (the ref_*
functions of test_gpu_matrix.py) against plain Python loops written from the reference's
expressions.  Every code here is returned before anything is launched or allocated, so no
device is needed (the addresses are never dereferenced)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ga_amd
import test_gpu_matrix as M
from ga_amd._lib import GA_LIB_PATH, LIB_PATH

INT, LNG, FLT, DBL, CPL, DCP = M.INT, M.LNG, M.FLT, M.DBL, M.CPL, M.DCP
OPS = sorted(ga_amd.OP_DTYPE)
BASE = 0x7F0000000000   # an address-shaped number; never read
FAR = BASE + (1 << 36)
E_NDIM, E_COUNT, E_OP, E_SCALAR, E_STRIDE, E_RANGE, E_ALIGN, E_OVERLAP = -2, -3, -4, -5, -6, -7, -8, -11
NEW_GA = ["GA_Shift_diagonal", "GA_Set_diagonal", "GA_Zero_diagonal", "GA_Add_diagonal", "GA_Get_diag",
          "GA_Scale_rows", "GA_Scale_cols", "GA_Norm1", "GA_Norm_infinity"]
USES_V = (M.GET, M.SET, M.ADD)
opid = dict(ids=lambda o: ga_amd.OP_NAME[o])


def test_constants_match_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ga_amd.h")).read()
    for name in ("GAAMD_NORM_ONE", "GAAMD_NORM_INF", "GAAMD_DIAG_GET", "GAAMD_DIAG_SET", "GAAMD_DIAG_ADD",
                 "GAAMD_DIAG_SHIFT", "GAAMD_DIAG_ZERO"):
        m = re.search(rf"#define {name} (\d+)", hdr)
        assert m and int(m.group(1)) == getattr(ga_amd, name), name
    assert len(set(M.FNS)) == 5 and ga_amd.GAAMD_NORM_ONE != ga_amd.GAAMD_NORM_INF


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3}


def test_exported_names():
    """the kernel library exports the four entry points and still no GA name; the GA library the
    nine new calls.  gaamd_diag stays the diagnostic entry point: the diagonal kernel is
    gaamd_diagonal"""
    core, ga = exported(LIB_PATH), exported(GA_LIB_PATH)
    for n in ("gaamd_patch_norm", "gaamd_diagonal", "gaamd_scale_rows", "gaamd_scale_cols", "gaamd_diag"):
        assert n in core, n
    assert not [n for n in core if n.startswith(("GA_", "NGA_"))]
    assert not [n for n in NEW_GA if n not in ga]
    assert ga_amd.lib().gaamd_diag.argtypes[0] is ctypes.c_char_p


# ---- gaamd_patch_norm ---------------------------------------------------------------
def norm_rc(op, kind, count, stride, base=BASE):
    return ga_amd.patch_norm(op, kind, base, stride, count)[0]


@pytest.mark.parametrize("kind", [ga_amd.GAAMD_NORM_ONE, ga_amd.GAAMD_NORM_INF])
def test_norm_codes(kind):
    L = ga_amd.lib()
    ll = ga_amd.ll_array
    out = np.ones(2)
    outp = out.ctypes.data_as(ctypes.c_void_p)
    p = ctypes.c_void_p(BASE)
    for ndim in (0, 8, -1):
        assert L.gaamd_patch_norm(DBL, kind, p, ll([64] * 8), ll([2] * 8), ndim, outp, None) == E_NDIM
    for op in (0, 1, 36, 43, 1004):
        assert norm_rc(op, kind, [4, 4], [64]) == E_OP
    for op in OPS:
        for count in ([-1], [4, -2], [4, 0, -1]):
            assert norm_rc(op, kind, count, [64, 4096][:len(count) - 1]) == E_COUNT
    assert L.gaamd_patch_norm(DBL, kind, p, None, ll([4, 4]), 2, outp, None) == E_STRIDE
    assert L.gaamd_patch_norm(DBL, kind, p, ll([64]), ll([4, 4]), 2, None, None) == E_SCALAR
    assert L.gaamd_patch_norm(DBL, kind, p, ll([64]), ll([4, 0]), 2, None, None) == E_SCALAR
    assert norm_rc(DBL, kind, [8], [], BASE + 2) == E_ALIGN
    assert norm_rc(FLT, kind, [8], [], BASE + 1) == E_ALIGN
    assert norm_rc(DCP, kind, [2, 2], [66]) == E_ALIGN
    assert norm_rc(DBL, kind, [2, 1 << 31], [64]) == E_RANGE


@pytest.mark.parametrize("op", OPS, **opid)
def test_norm_unknown_kind_and_zero_counts(op):
    for kind in (0, 3, -1, 100):
        assert norm_rc(op, kind, [4, 4], [64]) == E_OP
        assert norm_rc(op, kind, [4, 0], [64]) == E_OP   # with a count of zero as well
    for kind in (ga_amd.GAAMD_NORM_ONE, ga_amd.GAAMD_NORM_INF):
        for count in ([0], [4, 0], [0, 5, 3], [3, 1, 1, 1, 1, 1, 0]):
            rc, out = ga_amd.patch_norm(op, kind, BASE, [64 << (3 * j) for j in range(len(count) - 1)], count)
            # no device here: a launch would fail.  The type's zero is written (the wrapper presets 0xA5 bytes)
            assert rc == 0 and out.tobytes() == bytes(out.dtype.itemsize), (kind, count, rc, out)
            assert out.dtype == M.real_dt(op)


# ---- gaamd_diagonal ---------------------------------------------------------------
@pytest.mark.parametrize("op", OPS, **opid)
def test_diagonal_codes(op):
    esz = ga_amd.OP_DTYPE[op].itemsize
    step = 38 * esz
    for fn in M.FNS:
        v = FAR if fn in USES_V else None
        c = 1 if fn == M.SHIFT else None
        assert ga_amd.diag(op, fn, -1, BASE, step, v, esz, scalar=c) == E_COUNT
        assert ga_amd.diag(op, fn, 1 << 39, BASE, step, v, esz, scalar=c) == E_RANGE
        assert ga_amd.diag(op, fn, 37, 0, step, v, esz, scalar=c) == E_SCALAR            # a missing
        assert ga_amd.diag(op, fn, 37, BASE + 2, step, v, esz, scalar=c) == E_ALIGN
        assert ga_amd.diag(op, fn, 37, BASE, step + 2, v, esz, scalar=c) == E_ALIGN
        assert ga_amd.diag(op, fn, 0, BASE, step, v, esz, scalar=c) == 0                 # nothing to do, no launch
        assert ga_amd.diag(op, fn, 0, BASE + 1, step, v, esz, scalar=c) == E_ALIGN       # checked all the same
        if fn in USES_V:
            assert ga_amd.diag(op, fn, 37, BASE, step, None, esz) == E_SCALAR
            assert ga_amd.diag(op, fn, 37, BASE, step, FAR + 1, esz) == E_ALIGN
            assert ga_amd.diag(op, fn, 37, BASE, step, FAR, esz + 2) == E_ALIGN
            # v inside the matrix's span, v ending on a's first byte, a's last byte on v's first
            assert ga_amd.diag(op, fn, 37, BASE, step, BASE + 8 * esz, esz) == E_OVERLAP
            assert ga_amd.diag(op, fn, 37, BASE, step, BASE - 37 * esz + 4, esz) == E_OVERLAP
            assert ga_amd.diag(op, fn, 37, BASE, step, BASE + 36 * step + esz - 4, esz) == E_OVERLAP
            assert ga_amd.diag(op, fn, 37, BASE, -step, BASE - 30 * step, esz) == E_OVERLAP   # a negative step's span
            assert ga_amd.diag(op, fn, 0, BASE, step, BASE, esz) == 0                    # no element, no overlap
        else:
            assert ga_amd.diag(op, fn, 0, BASE, step, None, 2, scalar=c) == 0            # v and its step are not used
    assert ga_amd.diag(op, M.SHIFT, 37, BASE, step, None, 0) == E_SCALAR                 # SHIFT without its constant
    for fn in (0, 6, -1, 100):
        assert ga_amd.diag(op, fn, 37, BASE, step, FAR, esz, scalar=1) == E_OP
        assert ga_amd.diag(op, fn, 0, BASE, step, FAR, esz, scalar=1) == E_OP


def test_diagonal_unknown_op():
    for op in (0, 1, 36, 43, 1004):
        for fn in M.FNS:
            assert ga_amd.lib().gaamd_diagonal(op, fn, 4, ctypes.c_void_p(BASE), 72, ctypes.c_void_p(FAR), 8,
                                               ctypes.c_void_p(FAR), None) == E_OP


# ---- gaamd_scale_rows / _cols -------------------------------------------------------
@pytest.mark.parametrize("call", [ga_amd.scale_rows, ga_amd.scale_cols], ids=["rows", "cols"])
@pytest.mark.parametrize("op", OPS, **opid)
def test_scale_codes(op, call):
    esz = ga_amd.OP_DTYPE[op].itemsize
    rows_call = call is ga_amd.scale_rows
    assert call(op, -1, 5, BASE, 8, FAR) == E_COUNT
    assert call(op, 5, -1, BASE, 8, FAR) == E_COUNT
    assert call(op, 5, 9, BASE, 8, FAR) == E_STRIDE          # lda below the row
    assert call(op, 5, 8, BASE, 8, None) == E_SCALAR
    assert call(op, 1 << 31, 8, BASE, 8, FAR) == E_RANGE
    assert call(op, 5, 8, BASE + 2, 8, FAR) == E_ALIGN
    assert call(op, 5, 8, BASE, 8, FAR + 1) == E_ALIGN
    for r, c in ((0, 8), (5, 0), (0, 0)):
        assert call(op, r, c, BASE, 8, FAR) == 0             # nothing to do, no launch (none is possible here)
        assert call(op, r, c, BASE, 8, None) == 0
    # v overlapping a: inside it, in its ld padding, ending on its first byte, starting on its last
    nv = 5 if rows_call else 8
    span = (4 * 12 + 8) * esz
    for v in (BASE, BASE + 9 * esz, BASE - nv * esz + 4, BASE + span - 4):
        assert call(op, 5, 8, BASE, 12, v) == E_OVERLAP, hex(v)
    assert call(5, 5, 8, BASE, 12, FAR) == E_OP
    assert call(0, 5, 8, BASE, 12, FAR) == E_OP


# ---- the restatement against loops written from matrix.c ------------------------------------
def parts(op, x):
    """the element as the reference's C values: numpy scalars of the part type"""
    return (x.real, x.imag) if op in M.REAL else (x,)


def c_abs(x):   # GA_ABS, globalp.h:55
    return x if x >= 0 else -x


def loop_norm(op, kind, a):
    dt = M.real_dt(op)
    acc = None if kind == M.INF else dt.type(0)
    with np.errstate(over="ignore"):
        for i in range(a.shape[0]):
            for j in range(a.shape[1]):
                x = a[i, j]
                if op in M.REAL:
                    q = dt.type(math.sqrt(float(x.real * x.real + x.imag * x.imag)))   # (float)sqrt((double)..)
                else:
                    q = c_abs(x)
                if kind == M.ONE:
                    acc = acc + q
                elif acc is None or q > acc:
                    acc = q
    return np.array([acc], dtype=dt)


def loop_scale(op, a, v, rows):
    out = a.copy()
    with np.errstate(over="ignore"):
        for i in range(a.shape[0]):
            for j in range(a.shape[1]):
                m = v[i] if rows else v[j]
                if op in M.REAL:   # (dca[..]).real *= (buf[i]).real; .imag *= .imag
                    out[i, j] = complex(a[i, j].real * m.real, a[i, j].imag * m.imag)
                else:
                    out[i, j] = a[i, j] * m
    return out


def loop_diag_add(op, a, ld_shape, v):
    """*da += buf[i]; da += ld + 1 over min(rows, cols) elements; v of one element: the shift"""
    out = a.copy()
    with np.errstate(over="ignore"):
        for i in range(min(ld_shape)):
            y = v[i] if len(v) > 1 else v[0]
            if op in M.REAL:
                out[i, i] = complex(a[i, i].real + y.real, a[i, i].imag + y.imag)
            else:
                out[i, i] = a[i, i] + y
    return out


@pytest.mark.parametrize("shape", [(3, 5), (5, 3)])
@pytest.mark.parametrize("op", OPS, **opid)
def test_restatement_against_python_loops(op, shape):
    rng = np.random.default_rng(op + shape[0])
    n = shape[0] * shape[1]
    for small in (None, 50):
        a = M.K.gen(op, n, rng, small).reshape(shape)
        if op in M.UNS:
            a[0, 0] = np.iinfo(a.dtype).min
        elif op not in M.REAL:
            a[0, 1] = -0.0
        flat = a.reshape(-1)
        if op in M.UNS:   # sums that wrap: one answer in any order
            assert M.ref_norm1_exact(op, flat).tobytes() == loop_norm(op, M.ONE, a).tobytes()
        else:   # the loop is the forward sum of the per-element quantities
            q = M.ref_abs(op, flat)
            assert np.cumsum(q, dtype=q.dtype)[-1:].tobytes() == loop_norm(op, M.ONE, a).tobytes()
            e = M.gen_exact(op, n, rng).reshape(shape)   # exactly summable: one answer in any order
            assert M.ref_norm1_exact(op, e.reshape(-1)).tobytes() == loop_norm(op, M.ONE, e).tobytes()
        assert M.ref_norm_inf(op, flat).tobytes() == loop_norm(op, M.INF, a).tobytes()
        for rows in (True, False):
            v = M.K.gen(op, shape[0] if rows else shape[1], rng, small)
            assert M.ref_scale(op, a, v, rows).tobytes() == loop_scale(op, a, v, rows).tobytes()
        nd = min(shape)
        idx = np.arange(nd)
        for v in (M.K.gen(op, nd, rng, small), M.K.scalar(op, M.SHIFT_C[op])):
            want = loop_diag_add(op, a, shape, v)
            got = a.copy()
            got[idx, idx] = M.ref_diag_add(op, a[idx, idx], v)
            assert got.tobytes() == want.tobytes()
    # the signed zeros of the maximum: -0.0 only if every |x| is -0.0
    if op in (FLT, DBL):
        z = -np.zeros(4, dtype=ga_amd.OP_DTYPE[op])
        assert M.ref_norm_inf(op, z).tobytes() == z[:1].tobytes()
        z[2] = 0.0
        assert M.ref_norm_inf(op, z).tobytes() == np.zeros(1, dtype=z.dtype).tobytes()
