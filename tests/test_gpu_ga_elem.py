"""GPU, one rank, kernel level: gaamd_patch_elem1 / _elem2 / _select against a numpy
restatement of the reference loops (global/src/elem_alg.c, select.c), compared as raw bits.

The restatement (ref_elem1 / ref_elem2 below) uses one numpy operation per rounding and an
explicit astype where the reference widens to double; GA_ABS / GA_MAX / GA_MIN are
globalp.h:55-57 (x >= 0 ? x : -x, a >= b ? a : b, a <= b ? a : b):
  ABS        GA_ABS; complex: the portable branch of do_abs (270-288, 297-315), C_SCPL with
             the ratio and 1 + ratio^2 in float, sqrt and the product in double
  ADD_CONST  x + alpha; complex part by part                                     524-574
  RECIP      1 / x; complex the scaled form, in the element's real type          399-425, 454-480
  MUL        a * b; complex re = a.re*b.re - a.im*b.im, im = a.re*b.im + a.im*b.re
  DIV        a / b; complex the scaled form in double for both complex types     1136-1266
  MAX, MIN   GA_MAX / GA_MIN; complex by scaled squared moduli in double         1533-1720
Integers: sums and products wrap, quotients truncate, INT_MIN / -1 wraps to INT_MIN.
Each returns the values and a mask of the zero divisors, which stay unwritten.
Bit equality of / and sqrt rests on the device's f32 / f64 division and f64 square root
being correctly rounded; these tests are the check of that.

Constants of the kernels (ga_amd/csrc/gaamd_patch.hip, gaamd_select.hip):
  MAP_SHARE   a map workgroup streams 2048 bytes of a row at every vector width
  CHUNK       a select item is 256 vectors of 16 bytes: 4096 bytes of a contiguous run
  RANGE       a select workgroup takes 8 items: 32768 bytes
  FINAL_PASS  the final workgroup takes 1024 partials per pass
"""
import numpy as np
import pytest

import ga_amd
import test_gpu_ga_math as K
from test_gpu_ga_math import CPL, DBL, DCP, DT, FLT, INT, LNG, OPS, REAL, UNS

ABS, ADD_CONST, RECIP = ga_amd.GAAMD_ELEM_ABS, ga_amd.GAAMD_ELEM_ADD_CONST, ga_amd.GAAMD_ELEM_RECIP
MUL, DIV, MAX, MIN = ga_amd.GAAMD_ELEM_MUL, ga_amd.GAAMD_ELEM_DIV, ga_amd.GAAMD_ELEM_MAX, ga_amd.GAAMD_ELEM_MIN
FN1, FN2 = [ABS, ADD_CONST, RECIP], [MUL, DIV, MAX, MIN]
FN_NAME = {ABS: "abs", ADD_CONST: "add_const", RECIP: "recip", MUL: "mul", DIV: "div", MAX: "max", MIN: "min"}
ZERO_DIVISOR = ga_amd.GAAMD_ZERO_DIVISOR

MAP_SHARE = 2048
CHUNK, RANGE, FINAL_PASS = 256 * 16, 8 * 256 * 16, 1024
CONST = {INT: -7, LNG: 0x123456789, FLT: 0.7, DBL: -1.0 / 3.0, CPL: complex(0.7, -0.3), DCP: complex(-1.0 / 3.0, 0.3)}


# ---- the reference restated ------------------------------------------------------
def ga_abs(x):
    if x.dtype.kind == "i":
        u = np.dtype(f"u{x.dtype.itemsize}")
        return np.where(x >= 0, x, (np.zeros(1, u) - x.view(u)).view(x.dtype))
    return np.where(x >= 0, x, -x)


def ga_max(a, b):
    return np.where(a >= b, a, b)


def ga_min(a, b):
    return np.where(a <= b, a, b)


def int_div(a, b):
    """C's truncating quotient on two's-complement values, INT_MIN / -1 wrapping; b != 0"""
    u = np.dtype(f"u{a.dtype.itemsize}")
    zero = np.zeros(1, u)
    ua = np.where(a < 0, zero - a.view(u), a.view(u))
    ub = np.where(b < 0, zero - b.view(u), b.view(u))
    q = ua // np.where(ub == 0, np.ones(1, u), ub)
    return np.where((a < 0) != (b < 0), zero - q, q).astype(u).view(a.dtype)


def ref_elem1(op, fn, x, alpha=None):
    """(values, zero-divisor mask)"""
    dt = DT[op]
    none = np.zeros(x.shape, dtype=bool)
    with np.errstate(all="ignore"):
        if op in REAL:
            R = REAL[op].type
            re, im = x.real.copy(), x.imag.copy()
            if fn == ABS:
                mr, mi = ga_abs(re), ga_abs(im)
                first = mr >= mi
                num, den, m = np.where(first, im, re), np.where(first, re, im), np.where(first, mr, mi)
                x2 = num / den
                t = R(1) + x2 * x2
                if op == CPL:
                    res = (m.astype(np.float64) * np.sqrt(t.astype(np.float64))).astype(np.float32)
                else:
                    res = m * np.sqrt(t)
                res = np.where(first & (re == 0), R(0), res)
                return K._cplx(op, res, np.zeros_like(res)), none
            if fn == ADD_CONST:
                al = K.scalar(op, alpha)
                return K._cplx(op, re + al.real[0], im + al.imag[0]), none
            magr, magi = ga_abs(re), ga_abs(im)
            first = magr >= magi
            bad = first & ~(magr != 0)
            num, den = np.where(first, im, re), np.where(first, re, im)
            c = num / den
            d = R(1) / ((R(1) + c * c) * den)
            cd = np.where(first, (-c) * d, c * d)
            return K._cplx(op, np.where(first, d, cd), np.where(first, cd, -d)), bad
        if fn == ABS:
            return ga_abs(x), none
        if fn == ADD_CONST:
            if op in UNS:
                return (x.view(UNS[op]) + K.scalar(op, alpha).view(UNS[op])).view(dt), none
            return x + K.scalar(op, alpha)[0], none
        bad = x == 0
        if op in UNS:
            return np.where(x == 1, 1, np.where(x == -1, -1, 0)).astype(dt), bad
        return dt.type(1) / x, bad


def ref_elem2(op, fn, a, b):
    """(values, zero-divisor mask)"""
    dt = DT[op]
    none = np.zeros(a.shape, dtype=bool)
    with np.errstate(all="ignore"):
        if op in REAL:
            R = REAL[op]
            ar, ai, br, bi = a.real.copy(), a.imag.copy(), b.real.copy(), b.imag.copy()
            if fn == MUL:
                return K._cplx(op, ar * br - ai * bi, ar * bi + ai * br), none
            aR, aI, bR, bI = (v.astype(np.float64) for v in (ar, ai, br, bi))
            if fn == DIV:
                first = ga_abs(bR) >= ga_abs(bI)
                bad = first & ~(bR != 0)
                num, den = np.where(first, bI, bR), np.where(first, bR, bI)
                x1 = num / den
                x2 = 1.0 / (den * (1.0 + x1 * x1))
                re = np.where(first, (aR + aI * x1) * x2, (aR * x1 + aI) * x2)
                im = np.where(first, (aI - aR * x1) * x2, (aI * x1 - aR) * x2)
                return K._cplx(op, re.astype(R), im.astype(R)), bad
            x1 = ga_max(ga_max(ga_abs(aR), ga_abs(aI)), ga_max(ga_abs(bR), ga_abs(bI)))
            zero = x1 == 0.0
            x1 = 1.0 / x1
            aR, aI, bR, bI = aR * x1, aI * x1, bR * x1, bI * x1
            t1, t2 = aR * aR + aI * aI, bR * bR + bI * bI
            take_a = zero | (t1 > t2 if fn == MAX else t1 < t2)
            return np.where(take_a, a, b), none
        if fn == MUL:
            if op in UNS:
                return (a.view(UNS[op]) * b.view(UNS[op])).view(dt), none
            return a * b, none
        if fn == DIV:
            bad = b == 0
            return (int_div(a, b) if op in UNS else a / b), bad
        return (ga_max(a, b) if fn == MAX else ga_min(a, b)), none


def sel_key(op, x):
    if op in REAL:
        re, im = x.real.copy(), x.imag.copy()
        return re * re + im * im
    return x


def ref_select(op, want_max, x):
    """(index, element, key): numpy's first occurrence"""
    k = sel_key(op, x)
    i = int(np.argmax(k) if want_max else np.argmin(k))
    return i, x[i:i + 1], k[i:i + 1]


def test_restatement_on_known_values():
    """no GPU: the restatement against values worked out by hand from the reference's text"""
    f = np.float64
    # |3 + 4i| and |4 + 3i| by the scaled form: 4 * sqrt(1 + 0.75^2) = 5 exactly
    got, _ = ref_elem1(DCP, ABS, np.array([3 + 4j, 4 + 3j, 0j, -0.0 + 0j]))
    assert got.tolist() == [5 + 0j, 5 + 0j, 0j, 0j]
    # GA_ABS keeps -0.0 and INT_MIN
    got, _ = ref_elem1(DBL, ABS, np.array([-0.0, -2.5, 2.5]))
    assert got.tobytes() == np.array([-0.0, 2.5, 2.5]).tobytes()
    got, _ = ref_elem1(INT, ABS, np.array([-2 ** 31, -5, 5], dtype=np.int32))
    assert got.tolist() == [-2 ** 31, 5, 5]
    # 1 / (0 + 2i) = -0.5i ; 1 / (2 + 0i) = 0.5 - 0i
    got, bad = ref_elem1(DCP, RECIP, np.array([2j, 2 + 0j, 0j]))
    assert got[0] == -0.5j and got[1].real == 0.5 and bad.tolist() == [False, False, True]
    assert np.signbit(got[1].imag)   # -c * d with c = +0
    # truncation and the wrap
    a = np.array([7, -7, 7, -7, -2 ** 31, 5], dtype=np.int32)
    b = np.array([2, 2, -2, -2, -1, 0], dtype=np.int32)
    got, bad = ref_elem2(INT, DIV, a, b)
    assert got[:5].tolist() == [3, -3, -3, 3, -2 ** 31] and bad.tolist() == [False] * 5 + [True]
    # (1 + 2i) / (3 + 4i) = 0.44 + 0.08i to rounding; (1 + 2i) / (0 + 0i) is a zero divisor
    got, bad = ref_elem2(DCP, DIV, np.array([1 + 2j, 1 + 2j]), np.array([3 + 4j, 0j]))
    assert abs(got[0] - (0.44 + 0.08j)) < 1e-15 and bad.tolist() == [False, True]
    # NaN gives b; +0 against -0 gives a
    nan = f("nan")
    a, b = np.array([nan, 1.0, 0.0, -0.0]), np.array([1.0, nan, -0.0, 0.0])
    for fn in (MAX, MIN):
        got, _ = ref_elem2(DBL, fn, a, b)
        assert got.tobytes() == np.array([1.0, nan, 0.0, -0.0]).tobytes()
    # complex ties give b, both zero gives a
    a, b = np.array([3 + 4j, 0j, 1 + 0j]), np.array([4 + 3j, -0.0 - 0.0j, 2 + 0j])
    assert ref_elem2(DCP, MAX, a, b)[0].tobytes() == np.array([4 + 3j, 0j, 2 + 0j]).tobytes()
    assert ref_elem2(DCP, MIN, a, b)[0].tobytes() == np.array([4 + 3j, 0j, 1 + 0j]).tobytes()
    assert ref_select(DBL, 0, np.array([2.0, 1.0, 1.0]))[0] == 1
    assert ref_select(CPL, 1, np.array([1 + 1j, 3 - 4j, 4 + 3j], dtype=np.complex64))[0] == 1


# ---- device helpers --------------------------------------------------------------
@pytest.fixture(scope="module")
def bufs(gpu_lib):
    b = [ga_amd.DeviceBuffer(1 << 20) for _ in range(3)]
    yield b
    for x in b:
        x.free()


def nonzero(op, x):
    """random data without a zero divisor (a zero real part would be one for some forms)"""
    if op in REAL:
        assert (x.real != 0).all() and (x.imag != 0).all()
    else:
        assert (x != 0).all()
    return x


def shapes(op):
    esz = DT[op].itemsize
    n = (MAP_SHARE + 16) // esz   # one vector more than a workgroup's share
    return [([n], [n]), ([17, 5], [20, 5])]


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("op", OPS, ids=lambda o: ga_amd.OP_NAME[o])
def test_elem_bit_exact(gpu_lib, bufs, op, off):
    """every fn on a contiguous run and on a padded 17 x 5 patch, at a 16-byte-aligned base
    and 4 bytes off it; elem2 also with c aliasing a, b and both.  The whole buffer is
    compared: the bytes around and between the rows are the canary"""
    da, db, dc = bufs
    dt = DT[op]
    rng = np.random.default_rng(2000 * op + off)
    for count, ext in shapes(op):
        stride, base, offs, nbytes = K.geometry(op, count, ext, off)
        tag = (ga_amd.OP_NAME[op], off, count)
        A, B, C0 = (K.make_buf(op, nbytes, base, rng) for _ in range(3))
        a, b = nonzero(op, K.take(A, offs, dt)), nonzero(op, K.take(B, offs, dt))
        for fn in FN1:
            dc.upload(A)
            rc = ga_amd.patch_elem1(op, fn, dc.ptr + base, stride, count, scalar=CONST[op] if fn == ADD_CONST else None)
            assert rc == 0, (FN_NAME[fn], tag, rc)
            want = A.copy()
            vals, bad = ref_elem1(op, fn, a, CONST[op])
            assert not bad.any()
            K.put(want, offs, vals)
            assert np.array_equal(K.back(dc, nbytes), want), (FN_NAME[fn], tag)
        for fn in FN2:
            for alias in ("none", "a", "b", "both"):
                da.upload(A)
                db.upload(B)
                dc.upload(C0)
                out, before = {"none": (dc, C0), "a": (da, A), "b": (db, B), "both": (da, A)}[alias]
                pb, bb = (da, a) if alias == "both" else (db, b)
                rc = ga_amd.patch_elem2(op, fn, da.ptr + base, stride, pb.ptr + base, stride, out.ptr + base,
                                        stride, count)
                assert rc == 0, (FN_NAME[fn], alias, tag, rc)
                want = before.copy()
                vals, bad = ref_elem2(op, fn, a, bb)
                assert not bad.any()
                K.put(want, offs, vals)
                assert np.array_equal(K.back(out, nbytes), want), (FN_NAME[fn], alias, tag)
                if alias == "none":   # the inputs are only read
                    assert np.array_equal(da.download(np.uint8, nbytes), A)
                    assert np.array_equal(db.download(np.uint8, nbytes), B)


# ---- directed inputs ---------------------------------------------------------------
def directed(op):
    """(a, b): pairs chosen for what a plausible implementation gets wrong"""
    dt = DT[op]
    if op in UNS:
        lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
        a = [lo, lo, lo, hi, -1, 1, 0, 7, -7, 7, -7, lo + 1, hi, 0, 5, -5]
        b = [-1, 1, lo, -1, lo, -1, 3, 2, 2, -2, -2, -1, hi, 0, 0, 5]
        return np.array(a, dtype=dt), np.array(b, dtype=dt)
    if op in REAL:
        big = 1e200 if op == DCP else 1e30
        a = [3 + 4j, 4 + 3j, 3 + 3j, -3 + 3j, 0 + 2j, -0.0 + 2j, 2 + 0j, 2 - 0.0j, big + big * 1j, big - 0.5 * big * 1j,
             0.5 * big + big * 1j, 3 + 4j, 4 + 3j, 0j, complex(-0.0, 0.0), 1 + 1j, 0j, 1e-3 + 1e-3j]
        b = [1 + 2j, -2 + 1j, 5 - 5j, 0 + 1j, 3 + 0j, 1 - 1j, 0 - 3j, 4 + 4j, big - big * 1j, 0.5 * big + big * 1j,
             big + 0.25 * big * 1j, 4 + 3j, 3 + 4j, complex(-0.0, -0.0), 0j, 0j, 1 + 1j, complex(0.0, -0.0)]
        return np.array(a, dtype=dt), np.array(b, dtype=dt)
    # no NaN or infinity here: an operation that MAKES a NaN (inf - inf) gives it the host's
    # or the device's default sign, which is not the reference's to define
    a = [0.0, -0.0, 0.0, -0.0, 1.0, -1.5, 2.5, 1e-30, 3.0, 1.0, 0.0, -0.0, 7.0, -2.5, 1e30, -1e-30]
    b = [-0.0, 0.0, 0.0, -0.0, 3.0, 2.5, -1.5, 3.0, 1e-30, 3.0, 1.0, 2.0, 0.0, -0.0, 7.0, 1e30]
    return np.array(a, dtype=dt), np.array(b, dtype=dt)


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, ids=lambda o: ga_amd.OP_NAME[o])
def test_elem_directed_inputs(gpu_lib, bufs, op):
    """+-0, INT_MIN / LONG_MIN and INT_MIN / -1; complex with |re| > |im|, < and ==, zero real
    parts, parts near overflow, MAX / MIN ties and both-zero; real MAX / MIN with a NaN in a
    and in b.  Where an input is a zero divisor the call returns GAAMD_ZERO_DIVISOR and that
    element keeps its bytes"""
    da, db, dc = bufs
    dt = DT[op]
    a, b = directed(op)
    n = a.size
    c0 = K.gen(op, n, np.random.default_rng(op))
    for fn in FN1:
        for x in (a, b):
            dc.upload(x)
            rc = ga_amd.patch_elem1(op, fn, dc.ptr, [], [n], scalar=CONST[op] if fn == ADD_CONST else None)
            vals, bad = ref_elem1(op, fn, x, CONST[op])
            assert rc == (ZERO_DIVISOR if bad.any() else 0), (FN_NAME[fn], rc)
            want = np.where(bad, x, vals)
            ga_amd.sync()
            got = dc.download(dt, n)
            assert got.tobytes() == want.tobytes(), (FN_NAME[fn], x, got, want)
    for fn in FN2:
        for x, y in ((a, b), (b, a)):
            if fn == MUL and op in REAL:   # big * big overflows to inf - inf: a NaN of no defined sign
                x, y = x.copy(), y.copy()
                x[8:11], y[8:11] = 1 + 2j, 3 - 1j
            da.upload(x)
            db.upload(y)
            dc.upload(c0)
            rc = ga_amd.patch_elem2(op, fn, da.ptr, [], db.ptr, [], dc.ptr, [], [n])
            vals, bad = ref_elem2(op, fn, x, y)
            assert rc == (ZERO_DIVISOR if bad.any() else 0), (FN_NAME[fn], rc)
            want = np.where(bad, c0, vals)
            ga_amd.sync()
            got = dc.download(dt, n)
            assert got.tobytes() == want.tobytes(), (FN_NAME[fn], x, y, got, want)
    if op in (FLT, DBL):   # MAX / MIN with a NaN in a, in b and in both: the result is b (pure selects)
        nan = float("nan")
        x, y = np.array([nan, 1.0, nan, -2.0], dtype=dt), np.array([1.0, nan, nan, nan], dtype=dt)
        for fn in (MAX, MIN):
            da.upload(x)
            db.upload(y)
            dc.upload(c0)
            assert ga_amd.patch_elem2(op, fn, da.ptr, [], db.ptr, [], dc.ptr, [], [4]) == 0
            ga_amd.sync()
            assert dc.download(dt, 4).tobytes() == y.tobytes() == ref_elem2(op, fn, x, y)[0].tobytes(), FN_NAME[fn]
    if op in REAL:   # the scaled forms did not overflow
        big = a[8:11]
        for vals in (ref_elem1(op, ABS, big)[0], ref_elem1(op, RECIP, big)[0], ref_elem2(op, DIV, big, b[8:11])[0]):
            assert np.isfinite(vals.real).all() and np.isfinite(vals.imag).all()


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, ids=lambda o: ga_amd.OP_NAME[o])
def test_zero_divisor_first_middle_last(gpu_lib, bufs, op):
    """a zero divisor in the first, a middle and the last element of a run longer than one
    workgroup's share (floats: +0 and -0): the return is GAAMD_ZERO_DIVISOR, those elements are
    untouched, every other element is correct; without them the same call returns 0"""
    da, db, dc = bufs
    dt = DT[op]
    esz = dt.itemsize
    n = (MAP_SHARE + 16) // esz + 1
    rng = np.random.default_rng(77 + op)
    a, b0, c0 = (nonzero(op, K.gen(op, n, rng)) for _ in range(3))
    at = [0, n // 2, n - 1]
    zeros = np.zeros(3, dtype=dt)
    if op not in UNS:
        zeros[1] = -0.0 if op not in REAL else complex(-0.0, 0.0)
    b = b0.copy()
    b[at] = zeros
    for off in (0, 4):
        # RECIP in place
        dc.upload(b, offset=off)
        assert ga_amd.patch_elem1(op, RECIP, dc.ptr + off, [], [n]) == ZERO_DIVISOR
        vals, bad = ref_elem1(op, RECIP, b)
        assert np.flatnonzero(bad).tolist() == at
        assert dc.download(dt, n, offset=off).tobytes() == np.where(bad, b, vals).tobytes(), ("recip", off)
        dc.upload(b0, offset=off)
        assert ga_amd.patch_elem1(op, RECIP, dc.ptr + off, [], [n]) == 0
        # DIV into a third array
        da.upload(a, offset=off)
        db.upload(b, offset=off)
        dc.upload(c0, offset=off)
        assert ga_amd.patch_elem2(op, DIV, da.ptr + off, [], db.ptr + off, [], dc.ptr + off, [], [n]) == ZERO_DIVISOR
        vals, bad = ref_elem2(op, DIV, a, b)
        assert np.flatnonzero(bad).tolist() == at
        assert dc.download(dt, n, offset=off).tobytes() == np.where(bad, c0, vals).tobytes(), ("div", off)
        db.upload(b0, offset=off)
        assert ga_amd.patch_elem2(op, DIV, da.ptr + off, [], db.ptr + off, [], dc.ptr + off, [], [n]) == 0
        # the other fn never report one
        assert ga_amd.patch_elem2(op, MUL, da.ptr + off, [], db.ptr + off, [], dc.ptr + off, [], [n]) == 0
        ga_amd.sync()


# ---- select --------------------------------------------------------------------------
def distinct(op, n, rng):
    """n elements with pairwise distinct keys, none of them extreme (|key| small)"""
    dt = DT[op]
    p = rng.permutation(n)
    if op in UNS:
        return (p.astype(np.int64) - n // 2).astype(dt)
    if op in REAL:   # keys re^2 + 1 with re = 1 + p / 2^20: distinct in float32 for n < 2^20
        return K._cplx(op, (1.0 + p / float(1 << 20)).astype(REAL[op]), np.ones(n, dtype=REAL[op]))
    return (1.0 + p / float(1 << 20)).astype(dt) if n < (1 << 20) else (1.0 + p / float(1 << 26)).astype(dt)


def extreme(op, want_max, k=0):
    """an element better than everything distinct() makes; k picks among equal keys with
    different bits (complex: the same modulus)"""
    dt = DT[op]
    if op in UNS:
        return dt.type(np.iinfo(dt).max if want_max else np.iinfo(dt).min)
    if op in REAL:
        if want_max:
            return dt.type([complex(30, 40), complex(40, 30), complex(-30, 40)][k % 3])
        return dt.type([complex(0.5, 0), complex(0, 0.5), complex(-0.5, 0)][k % 3])
    return dt.type(1000.0 if want_max else -1000.0)


def select_both(op, dev, base, stride, count, x, tag):
    """min and max of the uploaded patch against numpy, twice"""
    for want_max in (0, 1):
        i, val, key = ref_select(op, want_max, x)
        for again in range(2):
            rc, gval, gkey, gi = ga_amd.patch_select(op, want_max, dev.ptr + base, stride, count)
            assert rc == 0, (tag, rc)
            assert (gi, gval.tobytes(), gkey.tobytes()) == (i, val.tobytes(), key.tobytes()), \
                (tag, "max" if want_max else "min", again, gi, i, gval, val, gkey, key)


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, ids=lambda o: ga_amd.OP_NAME[o])
def test_select_at_chunk_and_workgroup_boundaries(gpu_lib, bufs, op):
    """contiguous runs one element below, at and above one chunk and one workgroup's range,
    and a few ranges; the extremum first, last, duplicated inside one wave, and duplicated in
    two workgroups' ranges.  Among equal keys the lowest index, with that element's bits"""
    dev = bufs[0]
    dt = DT[op]
    esz = dt.itemsize
    rng = np.random.default_rng(300 + op)
    c, r = CHUNK // esz, RANGE // esz
    for n in (1, c - 1, c, c + 1, r - 1, r, r + 1, 2 * r + 1, 5 * r + 3):
        base_data = distinct(op, n, rng)
        places = {"first": [0], "last": [n - 1], "one wave": [n // 3, n // 3 + 5], "two ranges": [r // 2, r + r // 2]}
        for name, at in places.items():
            at = sorted(set(min(i, n - 1) for i in at))
            for want_max in (0, 1):
                x = base_data.copy()
                for k, i in enumerate(at):
                    x[i] = extreme(op, want_max, k)
                dev.upload(x)
                i, val, key = ref_select(op, want_max, x)
                assert i == min(at)
                rc, gval, gkey, gi = ga_amd.patch_select(op, want_max, dev.ptr, [], [n])
                assert rc == 0
                assert (gi, gval.tobytes(), gkey.tobytes()) == (i, val.tobytes(), key.tobytes()), \
                    (ga_amd.OP_NAME[op], n, name, want_max, gi, i, gval, val)
        dev.upload(base_data)
        select_both(op, dev, 0, [], [n], base_data, (ga_amd.OP_NAME[op], n, "distinct"))


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, ids=lambda o: ga_amd.OP_NAME[o])
def test_select_rows_tails_and_bases(gpu_lib, bufs, op):
    """a padded 17 x 5 patch at a 16-byte-aligned base and 4 bytes off it: the extremum in a
    row's tail (the last element of a row, past the last whole vector), and every position
    in turn; a 3-D patch with a count-1 dimension.  The buffer is only read"""
    dev = bufs[0]
    dt = DT[op]
    rng = np.random.default_rng(400 + op)
    for count, ext in (([17, 5], [20, 5]), ([6, 1, 4], [8, 2, 5])):
        for off in (0, 4):
            stride, base, offs, nbytes = K.geometry(op, count, ext, off)
            n = offs.size
            A = K.make_buf(op, nbytes, base, rng)
            for want_max in (0, 1):
                for pos in ([3 * count[0] + count[0] - 1] if count[0] == 17 else []) + [0, n - 1, n // 2]:
                    x = distinct(op, n, rng)
                    x[pos] = extreme(op, want_max)
                    img = A.copy()
                    K.put(img, offs, x)
                    dev.upload(img)
                    rc, gval, gkey, gi = ga_amd.patch_select(op, want_max, dev.ptr + base, stride, count)
                    assert (rc, gi, gval.tobytes()) == (0, pos, x[pos:pos + 1].tobytes()), (count, off, pos, gi)
                    assert np.array_equal(dev.download(np.uint8, nbytes), img)


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, ids=lambda o: ga_amd.OP_NAME[o])
def test_select_past_one_pass_of_the_final_workgroup(gpu_lib, bufs, op):
    """rows of one vector each: every row is one item, 8 rows a workgroup -- 1024 partials
    fill one pass of the final workgroup, 1025 need a second.  The extremum duplicated across
    the final-pass boundary (in partial 1023 and in partial 1024) and in the last partial"""
    dev = bufs[0]
    dt = DT[op]
    esz = dt.itemsize
    per_row = K.VEC // esz
    rng = np.random.default_rng(500 + op)
    for nwg in (FINAL_PASS - 1, FINAL_PASS, FINAL_PASS + 1, 2 * FINAL_PASS + 3):
        rows = 8 * (nwg - 1) + 3
        count, stride = [per_row, rows], [32]
        offs = K.offsets(esz, 0, count, stride)
        n = offs.size
        img = K.make_buf(op, 32 * rows, 0, rng)
        x = distinct(op, n, rng)
        for want_max in (0, 1):
            y = x.copy()
            at = [(8 * (FINAL_PASS - 1) + 2) * per_row, min(n - 1, (8 * FINAL_PASS + 1) * per_row), n - 1]
            at = sorted(set(min(a, n - 1) for a in at))
            for k, i in enumerate(at):
                y[i] = extreme(op, want_max, k)
            K.put(img, offs, y)
            dev.upload(img)
            i, val, key = ref_select(op, want_max, y)
            assert i == at[0]
            rc, gval, gkey, gi = ga_amd.patch_select(op, want_max, dev.ptr, stride, count)
            assert (rc, gi, gval.tobytes(), gkey.tobytes()) == (0, i, val.tobytes(), key.tobytes()), (nwg, gi, i)
        K.put(img, offs, x)
        dev.upload(img)
        select_both(op, dev, 0, stride, count, x, (ga_amd.OP_NAME[op], nwg, "distinct"))


@pytest.mark.gpu
def test_select_long_run_f64(gpu_lib):
    """one contiguous run of more than 1024 workgroup ranges (32 MiB of f64): the extremum
    duplicated either side of the final-pass boundary, then at the very end only"""
    per = RANGE // 8
    n = (FINAL_PASS + 1) * per + 1
    rng = np.random.default_rng(12)
    x = distinct(DBL, n, rng)
    dev = ga_amd.DeviceBuffer(x.nbytes)
    try:
        for at in ([FINAL_PASS * per - 1, FINAL_PASS * per], [n - 1]):
            for want_max in (0, 1):
                y = x.copy()
                y[at] = extreme(DBL, want_max)
                dev.upload(y)
                rc, gval, gkey, gi = ga_amd.patch_select(DBL, want_max, dev.ptr, [], [n])
                assert (rc, gi, gval[0]) == (0, at[0], y[at[0]]), (at, want_max, gi)
    finally:
        dev.free()


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, ids=lambda o: ga_amd.OP_NAME[o])
def test_select_all_equal_and_signed_zero_ties(gpu_lib, bufs, op):
    dev = bufs[0]
    dt = DT[op]
    n = 3 * RANGE // dt.itemsize + 5
    x = np.full(n, K.scalar(op, K.VALUE[op])[0], dtype=dt)
    dev.upload(x)
    for want_max in (0, 1):
        rc, gval, gkey, gi = ga_amd.patch_select(op, want_max, dev.ptr, [], [n])
        assert (rc, gi, gval.tobytes()) == (0, 0, x[:1].tobytes())
    if op in UNS:
        return
    # +0 and -0 are equal keys: the one at the lower index is returned, with its sign
    pz, nz = (complex(0.0, 0.0), complex(-0.0, -0.0)) if op in REAL else (0.0, -0.0)
    for want_max in (0, 1):
        if op in REAL and want_max:
            continue   # complex keys are >= 0: zeros are the minimum only
        fill = -1.0 if want_max else 1.0
        for first, second in ((pz, nz), (nz, pz)):
            y = np.full(n, fill, dtype=dt)
            i, j = n // 4, n // 4 + RANGE // dt.itemsize + 1   # in two workgroups' ranges
            y[i], y[j] = first, second
            dev.upload(y)
            rc, gval, gkey, gi = ga_amd.patch_select(op, want_max, dev.ptr, [], [n])
            assert (rc, gi, gval.tobytes()) == (0, i, y[i:i + 1].tobytes()), (want_max, first, gi, gval)


@pytest.mark.gpu
@pytest.mark.parametrize("op", [DBL, FLT], ids=["dbl", "flt"])
def test_select_rows_past_2_to_the_31(gpu_lib, op):
    """a 3-row patch with rows 2^31 + 48 bytes apart (the last one past byte 2^32); only the
    three rows are ever written or read.  The extremum in each row in turn: the index is
    row * 17 + position, the value comes from that row"""
    dt = DT[op]
    esz = dt.itemsize
    far = (1 << 31) + 48
    count, stride = [17, 3], [far]
    dev = ga_amd.DeviceBuffer(2 * far + 17 * esz + 256)
    rng = np.random.default_rng(600 + op)
    try:
        for off in ((0, 4) if op == FLT else (0,)):
            for row in (0, 1, 2):
                for want_max in (0, 1):
                    x = distinct(op, 51, rng).reshape(3, 17)
                    x[row, 16 - row] = extreme(op, want_max)
                    for r in range(3):
                        dev.upload(x[r], offset=off + r * far)
                    rc, gval, gkey, gi = ga_amd.patch_select(op, want_max, dev.ptr + off, stride, count)
                    assert (rc, gi, gval[0]) == (0, row * 17 + 16 - row, x[row, 16 - row]), (off, row, want_max, gi)
    finally:
        dev.free()
