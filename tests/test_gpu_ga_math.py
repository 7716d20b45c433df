"""GPU, one rank, kernel level: gaamd_patch_fill / _scale / _add / _dot against a
numpy restatement of the reference loops (global/src/global.npatch.c), compared as
raw bits.

The restatement (ref_* below) uses one numpy operation per rounding, complex numbers
through their real and imaginary parts in the reference's order:
  fill           stores the value                                         1528-1650
  scale real     x * alpha                                                1953-1966
  scale complex  re = x.re*al.re - x.im*al.im; im = al.im*x.re + x.im*al.re   1976-1986
  add real       alpha*a + beta*b (two products, one sum)                  2520-2525
  add complex    re = ((x.re*a.re - x.im*a.im) + y.re*b.re) - y.im*b.im
                 im = ((x.re*a.im + x.im*a.re) + y.re*b.im) + y.im*b.re   2537-2546
  dot            sum += a*b; complex re += a.re*b.re - b.im*a.im,
                 im += a.im*b.re + b.im*a.re (no conjugate)                938-1095
Integers in unsigned arithmetic (wraparound).

Constants of the kernels (ga_amd/csrc/gaamd_patch.hip), with cases either side:
  VEC      16-byte vectors where every base, stride and the row length allow, else
           8 or 4 bytes (one element per vector below the element's alignment):
           rows of 15, 16, 17 elements and bases 0 / 4 / 8 bytes off 16
  DOT_RANGE   a workgroup sums kDotItems = 8 items of kDotBS = 256 vectors: on a
           contiguous run 8 * 256 * 16 = 32768 bytes, 32768 / elemsize elements
  FINAL_PASS  the final workgroup takes kDotBS * kFinalPer = 256 * 4 = 1024 partials
           (4 consecutive partials per lane) per pass
"""
import math

import numpy as np
import pytest

import ga_amd

INT, DBL, FLT, CPL, DCP, LNG = (ga_amd.COMEX_ACC_INT, ga_amd.COMEX_ACC_DBL, ga_amd.COMEX_ACC_FLT,
                                ga_amd.COMEX_ACC_CPL, ga_amd.COMEX_ACC_DCP, ga_amd.COMEX_ACC_LNG)
OPS = [INT, LNG, FLT, DBL, CPL, DCP]
DT = ga_amd.OP_DTYPE
UNS = {INT: np.dtype(np.uint32), LNG: np.dtype(np.uint64)}
REAL = {CPL: np.dtype(np.float32), DCP: np.dtype(np.float64)}

VEC = 16
DOT_RANGE_BYTES = 8 * 256 * 16
FINAL_PASS = 256 * 4

ALPHA = {INT: -7, LNG: 0x123456789, FLT: 0.70710678, DBL: 0.7071067811865476, CPL: complex(0.7, -0.3),
         DCP: complex(0.7, -0.3)}
BETA = {INT: 5, LNG: -3, FLT: -1.3, DBL: -1.3, CPL: complex(-1.1, 0.45), DCP: complex(-1.1, 0.45)}
VALUE = {INT: -123456789, LNG: -0x123456789ABCDEF, FLT: 3.25, DBL: -2.0 / 3.0, CPL: complex(1.5, -2.25),
         DCP: complex(1.0 / 3.0, -2.0 / 7.0)}


# ---- the reference restated --------------------------------------------------
def scalar(op, v):
    return np.array([v], dtype=DT[op])


def _cplx(op, re, im):
    out = np.empty(re.shape, dtype=DT[op])
    out.real = re
    out.imag = im
    return out


def ref_fill(op, n, value):
    return np.full(n, scalar(op, value)[0], dtype=DT[op])


def ref_scale(op, x, alpha):
    al = scalar(op, alpha)
    if op in UNS:
        return (x.view(UNS[op]) * al.view(UNS[op])).view(DT[op])
    if op in REAL:
        ar, ai = al.real[0], al.imag[0]
        xr, xi = x.real.copy(), x.imag.copy()
        return _cplx(op, xr * ar - xi * ai, ai * xr + xi * ar)
    return x * al[0]


def ref_add(op, alpha, a, beta, b):
    al, be = scalar(op, alpha), scalar(op, beta)
    if op in UNS:
        u = UNS[op]
        return (al.view(u) * a.view(u) + be.view(u) * b.view(u)).view(DT[op])
    if op in REAL:
        xr, xi, yr, yi = al.real[0], al.imag[0], be.real[0], be.imag[0]
        ar, ai, br, bi = a.real.copy(), a.imag.copy(), b.real.copy(), b.imag.copy()
        re = ((xr * ar - xi * ai) + yr * br) - yi * bi
        im = ((xr * ai + xi * ar) + yr * bi) + yi * br
        return _cplx(op, re, im)
    return al[0] * a + be[0] * b


def ref_dot_exact(op, a, b):
    """the dot product where every partial sum is exact (integers; integer-valued
    floats): any order gives these bits"""
    if op in UNS:
        u = UNS[op]
        return np.array([(a.view(u) * b.view(u)).sum(dtype=u)], dtype=u).view(DT[op])
    if op in REAL:
        ar, ai, br, bi = (v.astype(np.float64) for v in (a.real, a.imag, b.real, b.imag))
        return scalar(op, complex((ar * br - bi * ai).sum(), (ai * br + bi * ar).sum()))
    return scalar(op, (a.astype(np.float64) * b.astype(np.float64)).sum())


# ---- data and geometry ---------------------------------------------------------
def gen(op, n, rng, small=None):
    """n elements; small = k: integer values in [-k, k] (floats: exactly representable)"""
    dt = DT[op]
    if small is not None:
        if op in REAL:
            return _cplx(op, rng.integers(-small, small + 1, n).astype(REAL[op]),
                         rng.integers(-small, small + 1, n).astype(REAL[op]))
        return rng.integers(-small, small + 1, n).astype(dt)
    if op in UNS:
        info = np.iinfo(dt)
        return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    if op in REAL:
        return _cplx(op, rng.uniform(-2, 2, n).astype(REAL[op]), rng.uniform(-2, 2, n).astype(REAL[op]))
    return rng.uniform(-2, 2, n).astype(dt)


def offsets(esz, base, count, stride):
    """byte offset of every element of the patch, dimension 0 fastest"""
    off = np.arange(count[0], dtype=np.int64) * esz
    for d in range(1, len(count)):
        off = (np.arange(count[d], dtype=np.int64)[:, None] * stride[d - 1] + off[None, :]).reshape(-1)
    return off + base


def take(buf, offs, dt):
    idx = offs[:, None] + np.arange(dt.itemsize)
    return np.ascontiguousarray(buf[idx]).view(dt).reshape(-1)


def put(buf, offs, vals):
    esz = vals.dtype.itemsize
    idx = offs[:, None] + np.arange(esz)
    buf[idx] = np.ascontiguousarray(vals).view(np.uint8).reshape(-1, esz)


def make_buf(op, nbytes, base, rng, small=None):
    """bytes that are valid elements at the patch's phase everywhere: the bytes around
    every row are the canary (compared with the whole buffer afterwards)"""
    esz = DT[op].itemsize
    ph = base % esz
    body = gen(op, nbytes // esz + 1, rng, small).view(np.uint8)
    out = np.zeros(nbytes, dtype=np.uint8)
    out[ph:] = body[:nbytes - ph]
    return out


# (count, block extents): the extents give the leading dimensions, larger than the rows
SHAPES = [([n], [n]) for n in (1, 3, 15, 16, 17, 1000)] + [
    ([5, 7], [9, 7]),
    ([257, 33], [260, 33]),
    ([6, 1, 4], [8, 2, 5]),
    ([3, 2, 1, 3], [4, 3, 2, 3]),
    ([2, 1, 3, 1, 2, 1, 2], [3, 1, 3, 2, 2, 1, 2]),
    ([16, 4, 3], [16, 4, 3]),          # a whole block: merges into one run
]
LEAD = 64   # canary bytes before the patch (keeps the base's alignment phase)


def geometry(op, count, ext, off):
    esz = DT[op].itemsize
    stride = [int(esz * np.prod(ext[:d + 1])) for d in range(len(count) - 1)]
    base = LEAD + off
    offs = offsets(esz, base, count, stride)
    nbytes = int(offs.max()) + esz + 48
    return stride, base, offs, nbytes


@pytest.fixture(scope="module")
def bufs(gpu_lib):
    size = 1 << 20
    b = [ga_amd.DeviceBuffer(size) for _ in range(3)]
    yield b
    for x in b:
        x.free()


def run(dev, host):
    dev.upload(host)


def back(dev, nbytes):
    ga_amd.sync()
    return dev.download(np.uint8, nbytes)


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 4, 8])
@pytest.mark.parametrize("op", OPS, ids=lambda o: ga_amd.OP_NAME[o])
def test_fill_scale_add_dot_bit_exact(gpu_lib, bufs, op, off):
    da, db, dc = bufs
    dt = DT[op]
    rng = np.random.default_rng(1000 * op + off)
    for count, ext in SHAPES:
        stride, base, offs, nbytes = geometry(op, count, ext, off)
        n = offs.size
        tag = (ga_amd.OP_NAME[op], off, count)
        A, B, C0 = (make_buf(op, nbytes, base, rng) for _ in range(3))
        a, b = take(A, offs, dt), take(B, offs, dt)
        # fill
        dc.upload(C0)
        assert ga_amd.patch_fill(op, VALUE[op], dc.ptr + base, stride, count) == 0
        want = C0.copy()
        put(want, offs, ref_fill(op, n, VALUE[op]))
        assert np.array_equal(back(dc, nbytes), want), ("fill", tag)
        # scale
        dc.upload(A)
        assert ga_amd.patch_scale(op, ALPHA[op], dc.ptr + base, stride, count) == 0
        want = A.copy()
        put(want, offs, ref_scale(op, a, ALPHA[op]))
        assert np.array_equal(back(dc, nbytes), want), ("scale", tag)
        # add into a third array, then with c aliased to a, then to b
        sum_ab = ref_add(op, ALPHA[op], a, BETA[op], b)
        for alias in ("none", "a", "b"):
            da.upload(A)
            db.upload(B)
            dc.upload(C0)
            out, before = {"none": (dc, C0), "a": (da, A), "b": (db, B)}[alias]
            assert ga_amd.patch_add(op, ALPHA[op], da.ptr + base, stride, BETA[op], db.ptr + base, stride,
                                    out.ptr + base, stride, count) == 0
            want = before.copy()
            put(want, offs, sum_ab)
            assert np.array_equal(back(out, nbytes), want), ("add", alias, tag)
            if alias == "none":   # the inputs are only read
                assert np.array_equal(da.download(np.uint8, nbytes), A)
                assert np.array_equal(db.download(np.uint8, nbytes), B)
        # dot: integers wrap; floats hold small integers, so every order gives the same bits
        small = None if op in UNS else 4
        IA, IB = make_buf(op, nbytes, base, rng, small), make_buf(op, nbytes, base, rng, small)
        da.upload(IA)
        db.upload(IB)
        rc, got = ga_amd.patch_dot(op, da.ptr + base, stride, db.ptr + base, stride, count)
        assert rc == 0
        want = ref_dot_exact(op, take(IA, offs, dt), take(IB, offs, dt))
        assert got.tobytes() == want.tobytes(), ("dot", tag, got, want)


@pytest.mark.gpu
def test_differing_leading_dimensions_per_operand(gpu_lib, bufs):
    """a, b and c each with its own strides (the kernel-level interface allows it)"""
    da, db, dc = bufs
    op, dt = DBL, DT[DBL]
    rng = np.random.default_rng(7)
    count = [37, 5, 3]
    geo = [geometry(op, count, ext, off) for ext, off in (([40, 5, 3], 0), ([37, 6, 3], 8), ([64, 7, 4], 0))]
    hosts = [make_buf(op, g[3], g[1], rng) for g in geo]
    for d, h in zip((da, db, dc), hosts):
        d.upload(h)
    (sa, ba, oa, _), (sb, bb, ob, _), (sc, bc, oc, nc) = geo
    assert ga_amd.patch_add(op, 2.5, da.ptr + ba, sa, -0.75, db.ptr + bb, sb, dc.ptr + bc, sc, count) == 0
    want = hosts[2].copy()
    put(want, oc, ref_add(op, 2.5, take(hosts[0], oa, dt), -0.75, take(hosts[1], ob, dt)))
    assert np.array_equal(back(dc, nc), want)


# ---- dot: exact sums at the workgroup and final-pass boundaries -----------------
def _dot_dev(op, a, b):
    da, db = ga_amd.DeviceBuffer(a.nbytes), ga_amd.DeviceBuffer(b.nbytes)
    try:
        da.upload(a)
        db.upload(b)
        rc, got = ga_amd.patch_dot(op, da.ptr, [], db.ptr, [], [a.size])
        assert rc == 0
        return got
    finally:
        da.free()
        db.free()


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, ids=lambda o: ga_amd.OP_NAME[o])
def test_dot_exact_at_workgroup_boundaries(gpu_lib, op):
    """1 workgroup (one element short of its range, and exactly it), 2 workgroups, a few"""
    per = DOT_RANGE_BYTES // DT[op].itemsize
    rng = np.random.default_rng(op)
    for n in (per - 1, per, per + 1, 2 * per, 2 * per + 1, 5 * per + 3):
        small = None if op in UNS else 7
        a, b = gen(op, n, rng, small), gen(op, n, rng, small)
        got = _dot_dev(op, a, b)
        assert got.tobytes() == ref_dot_exact(op, a, b).tobytes(), (n, got)


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, ids=lambda o: ga_amd.OP_NAME[o])
def test_dot_exact_past_one_pass_of_the_final_workgroup(gpu_lib, bufs, op):
    """rows of one vector each: every row is one item, 8 rows a workgroup -- 1024
    partials fill one pass of the final workgroup, 1025 need a second"""
    dt = DT[op]
    esz = dt.itemsize
    rng = np.random.default_rng(50 + op)
    per_row = VEC // esz
    for nwg in (FINAL_PASS - 1, FINAL_PASS, FINAL_PASS + 1, 2 * FINAL_PASS + 3):
        rows = 8 * (nwg - 1) + 3   # the last workgroup holds 3 items
        count, stride = [per_row, rows], [32]
        offs = offsets(esz, 0, count, stride)
        nbytes = 32 * rows
        small = None if op in UNS else 1   # f32: sums stay far below 2**24
        A, B = make_buf(op, nbytes, 0, rng, small), make_buf(op, nbytes, 0, rng, small)
        bufs[0].upload(A)
        bufs[1].upload(B)
        rc, got = ga_amd.patch_dot(op, bufs[0].ptr, stride, bufs[1].ptr, stride, count)
        assert rc == 0
        assert got.tobytes() == ref_dot_exact(op, take(A, offs, dt), take(B, offs, dt)).tobytes(), (nwg, got)


@pytest.mark.gpu
def test_dot_exact_long_run_f64(gpu_lib):
    """one contiguous run of more than 1024 workgroup ranges (f64: 4096 elements each)"""
    per = DOT_RANGE_BYTES // 8
    n = (FINAL_PASS + 1) * per + 1
    rng = np.random.default_rng(11)
    a, b = gen(DBL, n, rng, 7), gen(DBL, n, rng, 7)
    got = _dot_dev(DBL, a, b)
    assert got.tobytes() == ref_dot_exact(DBL, a, b).tobytes()


@pytest.mark.gpu
def test_dot_reproducible(gpu_lib):
    """the same f64 random input: identical bits twice, and with one library stream"""
    n = (1 << 20) + 3
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    first = _dot_dev(DBL, a, b)
    again = _dot_dev(DBL, a, b)
    assert first.tobytes() == again.tobytes()
    old = ga_amd.set_tuning("streams", 1)
    try:
        one = _dot_dev(DBL, a, b)
    finally:
        ga_amd.set_tuning("streams", old)
    assert one.tobytes() == first.tobytes()
    assert abs(first[0] - float(np.dot(a, b))) <= 1e-9 * float(np.abs(a * b).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("op", [DBL, FLT], ids=["dbl", "flt"])
def test_dot_rounding_bound(gpu_lib, op):
    """inputs of few significant bits (f64: 26, f32: 12), so every product is exact and
    the exact sum S is known: |got - S| <= gamma_n * sum|a_i b_i|, gamma_n = n u / (1 - n u),
    the bound of any summation order in the accumulator's precision (u = 2**-53 for f64,
    2**-24 for f32) -- an accumulator narrower than the type misses it"""
    n = 100003
    bits, u = (26, 2.0 ** -53) if op == DBL else (12, 2.0 ** -24)
    rng = np.random.default_rng(17)
    lim = 1 << (bits - 1)
    a = (rng.integers(-lim, lim, n) * 2.0 ** -(bits - 2)).astype(DT[op])
    b = (rng.integers(-lim, lim, n) * 2.0 ** -(bits - 2)).astype(DT[op])
    prods = a.astype(np.float64) * b.astype(np.float64)   # exact: at most 52 (24) significant bits
    S = math.fsum(prods.tolist())
    got = float(_dot_dev(op, a, b)[0])
    gamma = n * u / (1 - n * u)
    bound = gamma * math.fsum(np.abs(prods).tolist())
    print(f"dot rounding {ga_amd.OP_NAME[op]}: n={n} got={got!r} S={S!r} err={abs(got - S):.3e} bound={bound:.3e}")
    assert abs(got - S) <= bound
