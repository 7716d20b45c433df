"""GPU, one rank, kernel level: gaamd_gemm_cplx (ga_amd/csrc/gaamd_gemm_cplx.hip) on the
matrix cores, C = alpha * op(A) * op(B) + beta * C, row-major, f64 and f32 complex, op(X) = X,
its transpose ('T') or its conjugate transpose ('C').

The tile constants come from gaamd_gemm_cplx_plan per op, so the shapes follow the kernels:
every extent is swept over {1, T-1, T, T+1, 2T+3} of its own constant.  Matrices lie as in
test_gpu_gemm.py -- ld = extent + 5, a guard row before and after, everything around C checked
unchanged -- with the base one element and one PART past a 16-byte boundary, so an f64 complex
element is aligned to 8 bytes and an f32 complex one to 4: what ga_amd.h promises is enough.

  exact     parts integer-valued in [-8, 8], alpha = 2 - 1i, beta = -3 + 2i: every partial
            sum and every term of the epilogue is exact in f32
            (3 * 2 * 64 * 2100 + 5 * 16 < 2**24), so any correct kernel gives the bits of the
            integer product: all nine (ta, tb), both ops
  random    per part: |err| <= (2k + 6) u ((|al.re| + |al.im|) P + (|be.re| + |be.im|)
            (|C.re| + |C.im|)), P = (|A.re| + |A.im|) @ (|B.re| + |B.im|): a part is a sum of
            2k products in any order (2k roundings), the epilogue adds at most six more;
            derived, not measured (test_gemm_cplx_abi.py holds the order contract itself
            against it); the reference in np.clongdouble (f64) or complex128 (f32)
  special   beta == 0 does not read C; alpha == 0 does not read A and gives gaamd_patch_scale's
            bits; beta == (1, 0) adds C without products
  conj      'C' is 'T' on a conjugated copy, bit for bit
  position  a sub-rectangle computed alone has the bits it has in the whole product; a repeat
            has the same bits (what rank independence of GA_Zgemm rests on)
  far       one operand's rows spread over 9 GiB (test_gpu_far_offsets.py's checker)
"""
import numpy as np
import pytest

import ga_amd

DCP, CPL = ga_amd.COMEX_ACC_DCP, ga_amd.COMEX_ACC_CPL
DT = {DCP: np.dtype(np.complex128), CPL: np.dtype(np.complex64)}
RT = {DCP: np.dtype(np.float64), CPL: np.dtype(np.float32)}
U = {DCP: 2.0 ** -53, CPL: 2.0 ** -24}
NINE = [(ta, tb) for ta in "NTC" for tb in "NTC"]
PAD = 5          # ld = extent + PAD
AL_X, BE_X = 2 - 1j, -3 + 2j                              # the exact tests' scalars
AL_R, BE_R = 0.7071067811865476 - 0.4j, -1.3 + 0.6j      # the random tests'


def tiles(op):
    rc, p = ga_amd.gemm_cplx_plan(op, "N", "N", 1, 1, 1, 1j, 1 << 40, 1, 2 << 40, 1, 1j, 3 << 40, 1)
    assert rc == 0
    return p["tm"], p["tn"], p["tk"]


def sweep(t):
    return [1, t - 1, t, t + 1, 2 * t + 3]


class Mat:
    """a rows x cols complex matrix in a device buffer with ld = cols + PAD, a guard row
    before and after, and its base one element and one part past a 16-byte boundary; the
    image is kept as parts (the real type)"""

    def __init__(self, dev, vals, fill):
        self.dt = vals.dtype
        self.rt = vals.real.dtype
        self.rows, self.cols = vals.shape
        self.ld = self.cols + PAD
        self.img = np.array(fill(2 * (1 + (self.rows + 2) * self.ld) + 1), dtype=self.rt)
        self.first = 2 * (1 + self.ld) + 1            # part index of [0][0].re
        self.view()[:, :] = vals
        assert self.img.nbytes <= dev.nbytes
        self.dev = dev
        dev.upload(self.img)
        self.ptr = dev.ptr + self.first * self.rt.itemsize
        assert dev.ptr % 16 == 0 and self.ptr % self.dt.itemsize == self.rt.itemsize

    def view(self, img=None):
        img = self.img if img is None else img
        body = img[self.first:self.first + 2 * self.rows * self.ld].view(self.dt).reshape(self.rows, self.ld)
        return body[:, :self.cols]

    def at(self, i, j):
        return self.ptr + (i * self.ld + j) * self.dt.itemsize

    def download(self):
        return self.dev.download(self.rt, self.img.size)


def stored(x, t):
    """op(X) as it is stored for trans t: conj-transposing the stored matrix gives x back"""
    return np.ascontiguousarray(x if t == "N" else x.T if t == "T" else x.conj().T)


def cplx(rng_parts, shape):
    """a complex array from a function giving real arrays of a shape"""
    return rng_parts(shape) + 1j * rng_parts(shape)


@pytest.fixture(scope="module")
def bufs(gpu_lib):
    big = max(max(2 * t + 3 for t in tiles(op)[:2]) for op in (DCP, CPL))
    size = 16 * (2 + (max(big, 300) + 2) * (4200 + PAD))
    b = [ga_amd.DeviceBuffer(size) for _ in range(4)]
    yield b
    for x in b:
        x.free()


def run(op, ta, tb, alpha, beta, opa, opb, c0, bufs, guard_rng, cbuf=2):
    """gaamd_gemm_cplx on op(A) (m x k), op(B) (k x n) and C: the new C, with every guard
    element around C checked unchanged"""
    dt = DT[op]
    m, k = opa.shape
    n = opb.shape[1]
    junk = lambda cnt: guard_rng.integers(-99, 100, cnt)   # noqa: E731
    a = Mat(bufs[0], stored(opa, ta).astype(dt), junk)
    b = Mat(bufs[1], stored(opb, tb).astype(dt), junk)
    c = Mat(bufs[cbuf], c0.astype(dt), junk)
    rc = ga_amd.gemm_cplx(op, ta, tb, m, n, k, alpha, a.ptr, a.ld, b.ptr, b.ld, beta, c.ptr, c.ld)
    assert rc == 0, rc
    ga_amd.sync()
    out = c.download()
    got = c.view(out).copy()
    c.view(out)[:, :] = c.view()       # put the old C back: the rest must be the old image
    assert out.tobytes() == c.img.tobytes(), f"guard elements around C changed ({ta}{tb} {m}x{n}x{k})"
    return got


def int_product(opa, opb):
    """the complex product of integer-valued complex matrices, exact, as (re, im) in int64"""
    ar, ai = opa.real.astype(np.int64), opa.imag.astype(np.int64)
    br, bi = opb.real.astype(np.int64), opb.imag.astype(np.int64)
    return ar @ br - ai @ bi, ar @ bi + ai @ br


def int_axpby(al, pr, pi, be, c0):
    """al * (pr + i pi) + be * c0 in int64, as a complex array (exact while it fits the type)"""
    alr, ali, ber, bei = int(al.real), int(al.imag), int(be.real), int(be.imag)
    cr, ci = c0.real.astype(np.int64), c0.imag.astype(np.int64)
    return (alr * pr - ali * pi + ber * cr - bei * ci) + 1j * (alr * pi + ali * pr + ber * ci + bei * cr)


def exact_case(op, ta, tb, m, n, k, bufs, rng):
    dt = DT[op]
    ints = lambda shape: rng.integers(-8, 9, shape)   # noqa: E731
    opa, opb, c0 = cplx(ints, (m, k)), cplx(ints, (k, n)), cplx(ints, (m, n))   # random: not Hermitian
    got = run(op, ta, tb, AL_X, BE_X, opa, opb, c0, bufs, rng)
    want = int_axpby(AL_X, *int_product(opa, opb), BE_X, c0).astype(dt)
    differ = got.view(RT[op]).reshape(m, n, 2) != want.view(RT[op]).reshape(m, n, 2)
    assert got.tobytes() == want.tobytes(), \
        f"{ta}{tb} {m}x{n}x{k}: {np.count_nonzero(differ.any(axis=2))} of {got.size} differ, first at {np.argwhere(differ)[:1]}"


@pytest.mark.gpu
@pytest.mark.parametrize("ta,tb", NINE, ids=lambda t: t)
@pytest.mark.parametrize("op", [DCP, CPL], ids=["dcp", "cpl"])
def test_exact_integer_data(gpu_lib, bufs, op, ta, tb):
    tm, tn, tk = tiles(op)
    rng = np.random.default_rng(1000 * op + 10 * ord(ta) + ord(tb))
    shapes = []
    for m in sweep(tm):
        shapes.append((m, 7, 9))
    for n in sweep(tn):
        shapes.append((5, n, 9))
    for k in sweep(tk):                   # the cube: every k against every m and n
        for m in sweep(tm):
            for n in sweep(tn):
                shapes.append((m, n, k))
    shapes.append((tm + 1, tn + 1, 2085))   # many k steps, the last one short; still exact
    shapes.append((3, 2, 2100))
    for m, n, k in shapes:
        exact_case(op, ta, tb, m, n, k, bufs, rng)


_random_cache = {}


def random_case(op, shape):
    """operands, scalars and the high-precision reference with its per-part bound, computed
    once (no device needed: test_gemm_cplx_abi.py uses it too)"""
    key = (op, shape)
    if key not in _random_cache:
        m, n, k = shape
        dt = DT[op]
        wide, rwide = (np.clongdouble, np.longdouble) if op == DCP else (np.complex128, np.float64)
        rng = np.random.default_rng(7 * op + m + n + k)
        uni = lambda s: rng.uniform(-2, 2, s)   # noqa: E731
        opa, opb, c0 = cplx(uni, (m, k)).astype(dt), cplx(uni, (k, n)).astype(dt), cplx(uni, (m, n)).astype(dt)
        al, be = dt.type(AL_R), dt.type(BE_R)
        aw, bw, cw = opa.astype(wide), opb.astype(wide), c0.astype(wide)
        ref = wide(al) * (aw @ bw) + wide(be) * cw
        l1 = lambda z: np.abs(z.real).astype(rwide) + np.abs(z.imag).astype(rwide)   # noqa: E731
        P = l1(opa) @ l1(opb)
        bound = rwide(2 * k + 6) * rwide(U[op]) * (l1(al) * P + l1(be) * l1(c0))
        for x in (opa, opb, c0, ref, bound):
            x.setflags(write=False)
        _random_cache[key] = (opa, opb, c0, al, be, ref, bound)
    return _random_cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("ta,tb", [("N", "N"), ("T", "N"), ("C", "N"), ("N", "C")], ids=lambda t: t)
@pytest.mark.parametrize("shape", [(257, 131, 1000), (64, 64, 4099)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("op", [DCP, CPL], ids=["dcp", "cpl"])
def test_random_data_within_the_rounding_bound(gpu_lib, bufs, op, shape, ta, tb):
    opa, opb, c0, al, be, ref, bound = random_case(op, shape)
    got = run(op, ta, tb, complex(al), complex(be), opa, opb, c0, bufs, np.random.default_rng(5))
    wide = ref.dtype
    err_re = np.abs(got.astype(wide).real - ref.real)
    err_im = np.abs(got.astype(wide).imag - ref.imag)
    worst = float(max(np.max(err_re / bound), np.max(err_im / bound)))
    print(f"gemm_cplx {ga_amd.OP_NAME[op]} {ta}{tb} {shape}: max |err| / bound = {worst:.4f}")
    assert np.all(err_re <= bound) and np.all(err_im <= bound), \
        (worst, np.argwhere(err_re > bound)[:5], np.argwhere(err_im > bound)[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("op", [DCP, CPL], ids=["dcp", "cpl"])
def test_beta_zero_does_not_read_c_alpha_zero_does_not_read_a(gpu_lib, bufs, op):
    tm, tn, tk = tiles(op)
    dt = DT[op]
    rng = np.random.default_rng(op)
    ints = lambda shape: rng.integers(-8, 9, shape)   # noqa: E731
    m, n, k = tm + 3, tn + 2, 2 * tk + 1
    opa, opb = cplx(ints, (m, k)).astype(dt), cplx(ints, (k, n)).astype(dt)
    nan_c = np.full((m, n), np.nan + 1j * np.nan, dtype=dt)
    got = run(op, "N", "N", AL_X, 0j, opa, opb, nan_c, bufs, rng)
    assert not np.isnan(got).any()
    zero = np.zeros((m, n), dtype=dt)
    assert got.tobytes() == int_axpby(AL_X, *int_product(opa, opb), 0j, zero).astype(dt).tobytes()
    # alpha == 0: what gaamd_patch_scale gives on a copy of the same C, A full of NaN
    uni = lambda s: rng.uniform(-2, 2, s)   # noqa: E731
    c0 = cplx(uni, (m, n)).astype(dt)
    c0[0, 0], c0[1, 1], c0[2, 2] = 0.0, complex(-0.0, 3.0), complex(1.5, -0.0)
    copy = Mat(bufs[3], c0, lambda cnt: rng.integers(-99, 100, cnt))
    assert ga_amd.patch_scale(op, BE_R, copy.ptr, [copy.ld * dt.itemsize], [n, m]) == 0
    ga_amd.sync()
    scaled = copy.view(copy.download()).copy()
    assert not np.array_equal(scaled, c0)
    nan_a = np.full((m, k), np.nan + 1j * np.nan, dtype=dt)
    for ta, tb in NINE:
        got = run(op, ta, tb, 0j, BE_R, nan_a, opb, c0, bufs, rng)
        assert got.tobytes() == scaled.tobytes(), (ta, tb)
    # both zero: zeros, C (NaN) not read
    got = run(op, "N", "N", 0j, 0j, nan_a, opb, nan_c, bufs, rng)
    assert got.tobytes() == zero.tobytes()
    # k == 0 is alpha == 0: the scale again
    got = run(op, "N", "N", AL_X, BE_R, opa[:, :0], opb[:0, :], c0, bufs, rng)
    assert got.tobytes() == scaled.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("op", [DCP, CPL], ids=["dcp", "cpl"])
def test_beta_one_adds_c_without_products(gpu_lib, bufs, op):
    """beta exactly (1, 0): c = t + c part by part.  With products, u.im = 1 * c.im + 0 * c.re
    is NaN for c.re = inf; without them an infinity stays what it is.  Rows 0 and 3 of A are
    zero, so both accumulators there are +0 and t is a zero whose signs follow alpha's:
    (-2, +1) makes t.re = -0 - (+0) = -0, (-2, -1) makes t.im = -0 + -0 = -0 -- and x + (-0)
    is x for every x, -0 included.  (A t of +0 turns a -0 into +0: that is the sum's rule,
    not a disturbance by the kernel, and the full comparison below covers it.)"""
    tm, tn, tk = tiles(op)
    dt, rt = DT[op], RT[op]
    rng = np.random.default_rng(40 + op)
    ints = lambda shape: rng.integers(-8, 9, shape)   # noqa: E731
    m, n, k = tm + 3, tn + 2, 2 * tk + 1
    opa, opb, c0 = cplx(ints, (m, k)).astype(dt), cplx(ints, (k, n)).astype(dt), cplx(ints, (m, n)).astype(dt)
    opa[0, :] = opa[3, :] = 0
    inf = np.inf
    c0[0, 0], c0[0, 1], c0[3, 2], c0[3, 3] = complex(-0.0, 5.0), complex(inf, 2.0), complex(1.0, -inf), complex(3.0, -0.0)
    c0[0, n - 1], c0[3, n - 1] = complex(-inf, inf), complex(-0.0, -0.0)
    pr, pi = int_product(opa, opb)
    sr, si = pr.astype(rt), pi.astype(rt)
    assert not sr[0].any() and not si[3].any()
    for al in (-2 + 1j, -2 - 1j):
        for ta, tb in (("N", "N"), ("C", "T")):
            got = run(op, ta, tb, al, 1 + 0j, opa, opb, c0, bufs, rng)
            alr, ali = rt.type(al.real), rt.type(al.imag)
            with np.errstate(invalid="ignore"):
                want = np.empty((m, n), dtype=dt)
                want.real = (alr * sr - ali * si) + c0.real
                want.imag = (alr * si + ali * sr) + c0.imag
            assert not np.isnan(got.view(rt)).any(), "an infinity in C went through a product"
            assert got.tobytes() == want.tobytes(), (al, ta, tb)
            # the chosen places, spelled out: infinities as they were ...
            for i, j in ((0, 1), (3, 2), (0, n - 1)):
                assert got[i, j].tobytes() == c0[i, j].tobytes(), (al, i, j, got[i, j])
            # ... and the -0 of the part whose t is -0
            if al.imag > 0:
                assert np.signbit(got[0, 0].real) and got[0, 0].real == 0 and np.signbit(got[3, n - 1].real)
            else:
                assert np.signbit(got[3, 3].imag) and got[3, 3].imag == 0 and np.signbit(got[3, n - 1].imag)


@pytest.mark.gpu
@pytest.mark.parametrize("op", [DCP, CPL], ids=["dcp", "cpl"])
def test_conjugate_transpose_is_transpose_of_the_conjugate(gpu_lib, bufs, op):
    """'C' on A (on B) equals 'T' on a conjugated copy of A (of B), bit for bit, on random data:
    the conjugation is exact and comes before everything else"""
    shape = (257, 131, 1000)
    opa, opb, c0, al, be, ref, bound = random_case(op, shape)
    rng = np.random.default_rng(13)
    al, be = complex(al), complex(be)
    # the matrices are placed by hand: the SAME stored matrix S under 'C', conj(S) under 'T'
    for side in "AB":
        m, n, k = shape
        dt = DT[op]
        junk = lambda cnt: rng.integers(-99, 100, cnt)   # noqa: E731
        raw_a = np.ascontiguousarray(opa.T if side == "A" else opa)     # as stored: k x m for A's side
        raw_b = np.ascontiguousarray(opb.T if side == "B" else opb)     # n x k for B's side
        outs = []
        for t, conj in (("C", False), ("T", True)):
            a = Mat(bufs[0], raw_a.conj() if conj and side == "A" else raw_a, junk)
            b = Mat(bufs[1], raw_b.conj() if conj and side == "B" else raw_b, junk)
            c = Mat(bufs[2], c0, junk)
            ta, tb = (t, "N") if side == "A" else ("N", t)
            assert ga_amd.gemm_cplx(op, ta, tb, m, n, k, al, a.ptr, a.ld, b.ptr, b.ld, be, c.ptr, c.ld) == 0
            ga_amd.sync()
            outs.append(c.view(c.download()).copy())
        assert outs[0].tobytes() == outs[1].tobytes(), \
            f"'C' on {side}: {np.count_nonzero(outs[0] != outs[1])} elements differ from 'T' on the conjugate"
        assert dt == outs[0].dtype and not np.array_equal(outs[0], c0)


@pytest.mark.gpu
@pytest.mark.parametrize("ta,tb", [("N", "N"), ("T", "N"), ("C", "N"), ("N", "C"), ("C", "C")], ids=lambda t: t)
@pytest.mark.parametrize("op", [DCP, CPL], ids=["dcp", "cpl"])
def test_bits_do_not_depend_on_position(gpu_lib, bufs, op, ta, tb):
    shape = (257, 131, 1000)
    m, n, k = shape
    opa, opb, c0, al, be, ref, bound = random_case(op, shape)
    al, be = complex(al), complex(be)
    rng = np.random.default_rng(11)
    full = run(op, ta, tb, al, be, opa, opb, c0, bufs, rng)
    again = run(op, ta, tb, al, be, opa, opb, c0, bufs, rng)
    assert full.tobytes() == again.tobytes(), "the same call twice gave different bits"
    # rows 37.., columns 50.. alone: offset base pointers, the same ld
    i0, j0 = 37, 50
    junk = lambda cnt: rng.integers(-99, 100, cnt)   # noqa: E731
    a = Mat(bufs[0], stored(opa, ta), junk)
    b = Mat(bufs[1], stored(opb, tb), junk)
    c = Mat(bufs[3], c0, junk)
    pa = a.at(i0, 0) if ta == "N" else a.at(0, i0)
    pb = b.at(0, j0) if tb == "N" else b.at(j0, 0)
    rc = ga_amd.gemm_cplx(op, ta, tb, m - i0, n - j0, k, al, pa, a.ld, pb, b.ld, be, c.at(i0, j0), c.ld)
    assert rc == 0
    ga_amd.sync()
    out = c.download()
    sub = c.view(out)
    assert sub[i0:, j0:].tobytes() == full[i0:, j0:].tobytes(), \
        f"{np.count_nonzero(sub[i0:, j0:] != full[i0:, j0:])} elements differ from the whole product"
    sub[i0:, j0:] = c0[i0:, j0:]
    assert out.tobytes() == c.img.tobytes(), "elements outside the sub-rectangle changed"


# ---- far offsets: the checker and the geometry of test_gpu_far_offsets.py --------------------
@pytest.fixture(scope="module")
def far_alloc(gpu_lib):
    """the one allocation of that file's size; a failure to get it is a failure of the test"""
    from test_gpu_far_offsets import ALLOC
    dev = ga_amd.DeviceBuffer(ALLOC)
    assert dev.ptr % 256 == 0
    yield dev
    dev.free()


@pytest.mark.gpu
@pytest.mark.parametrize("which_far", ["A", "B", "C"])
@pytest.mark.parametrize("ta,tb", [("N", "N"), ("C", "T")], ids=lambda t: t)
def test_gemm_cplx_far(gpu_lib, far_alloc, ta, tb, which_far):
    """f64 complex, each of A, B and C in turn with its rows spread over 9 GiB: exact integer
    data, every row and every canary (the wrapped offsets included) as expected.  odd: an odd
    ld from a base 8 bytes past a 16-byte boundary; vec: everything on 16 bytes."""
    from test_gpu_far_offsets import COMPACT, FAR, Sparse, assert_clean, mat_geo, place_matrix
    op, dt = DCP, DT[DCP]
    tm, tn, tk = tiles(op)
    m, n, k = tm + 1, tn + 1, tk + 1
    rng = np.random.default_rng(10 * ord(ta) + ord(tb) + ord(which_far))
    ints = lambda shape: rng.integers(-8, 9, shape)   # noqa: E731
    for vec in (False, True):
        opa, opb, c0 = cplx(ints, (m, k)), cplx(ints, (k, n)), cplx(ints, (m, n))
        mats = {"A": stored(opa, ta), "B": stored(opb, tb), "C": c0}
        img = Sparse(far_alloc, 1300 + vec)
        placed = {}
        for name, zone in zip("ABC", COMPACT):
            vals = np.ascontiguousarray(mats[name]).astype(dt)
            geo = None
            if name == which_far:
                geo = mat_geo("gemm_cplx", vals.shape[0], vals.shape[1], 16, vec, base=FAR + (0 if vec else 8))
                assert geo.offs[-1] >= 9 << 30 and (geo.base % 16 == 0) == vec
            placed[name] = place_matrix(img, far_alloc, vals, geo, zone + (0 if vec else 8), f"matrix {name}")
        img.expect(placed["C"][2], int_axpby(AL_X, *int_product(opa, opb), BE_X, c0).astype(dt))
        img.seal()
        (pa, lda, _), (pb, ldb, _), (pc, ldc, _) = placed["A"], placed["B"], placed["C"]
        rc = ga_amd.gemm_cplx(op, ta, tb, m, n, k, AL_X, pa, lda, pb, ldb, BE_X, pc, ldc)
        assert rc == 0, rc
        ga_amd.sync()
        assert_clean(img, ("gemm_cplx", ta + tb, "far " + which_far, "vec" if vec else "odd"))
