"""GPU, one rank, kernel level: gaamd_gemm (ga_amd/csrc/gaamd_gemm.hip) on the matrix
cores, C = alpha * op(A) * op(B) + beta * C, row-major, f64 and f32.

The tile constants TM, TN, TK come from gaamd_gemm_plan, so the shapes follow the kernel:
every extent is swept over {1, T-1, T, T+1, 2T+3} of its own constant.

  exact     integer-valued data small enough that every partial sum is exact in the type
            (f32: |alpha * acc| + |beta * c| <= 2 * 64 * 2100 + 24 < 2**24), so any
            correct kernel gives the bits of the int64 product: all four (ta, tb),
            ld = extent + 5, bases one element past a 16-byte boundary, guard elements
            around C
  random    the elementwise bound (k + 3) * u * (|alpha| |op A| |op B| + |beta| |C|):
            an inner product summed in any order (k roundings) plus the three roundings
            of the epilogue; the reference in np.longdouble (f64) or float64 (f32)
  special   beta == 0 does not read C; alpha == 0 does not read A
  position  a sub-rectangle computed alone has the bits it has in the whole product; a
            repeat has the same bits (what rank independence of GA_Dgemm rests on)
"""
import numpy as np
import pytest

import ga_amd

DBL, FLT = ga_amd.COMEX_ACC_DBL, ga_amd.COMEX_ACC_FLT
DT = {DBL: np.dtype(np.float64), FLT: np.dtype(np.float32)}
U = {DBL: 2.0 ** -53, FLT: 2.0 ** -24}
TRANS = [("N", "N"), ("N", "T"), ("T", "N"), ("T", "T")]
PAD = 5          # ld = extent + PAD
ALPHA_R, BETA_R = 0.7071067811865476, -1.3


def tiles():
    rc, p = ga_amd.gemm_plan(DBL, "N", "N", 1, 1, 1, 1.0, 1 << 40, 1, 2 << 40, 1, 1.0, 3 << 40, 1)
    assert rc == 0
    return p["tm"], p["tn"], p["tk"]


def sweep(t):
    return [1, t - 1, t, t + 1, 2 * t + 3]


class Mat:
    """a rows x cols matrix in a device buffer with ld = cols + PAD, a guard row before
    and after, and its base one element past a 16-byte boundary"""

    def __init__(self, dev, vals, fill):
        self.dt = vals.dtype
        self.rows, self.cols = vals.shape
        self.ld = self.cols + PAD
        self.img = np.array(fill(1 + (self.rows + 2) * self.ld), dtype=self.dt)
        self.first = 1 + self.ld            # element index of [0][0]
        self.view()[:, :] = vals
        assert self.img.nbytes <= dev.nbytes
        self.dev = dev
        dev.upload(self.img)
        self.ptr = dev.ptr + self.first * self.dt.itemsize
        assert dev.ptr % 16 == 0 and (dev.ptr + self.dt.itemsize) % 16 != 0

    def view(self, img=None):
        img = self.img if img is None else img
        body = img[self.first:self.first + self.rows * self.ld].reshape(self.rows, self.ld)
        return body[:, :self.cols]

    def at(self, i, j):
        return self.ptr + (i * self.ld + j) * self.dt.itemsize

    def download(self):
        return self.dev.download(self.dt, self.img.size)


def stored(x, t):
    """op(X) as it is stored for trans t"""
    return np.ascontiguousarray(x.T if t == "T" else x)


@pytest.fixture(scope="module")
def bufs(gpu_lib):
    tm, tn, tk = tiles()
    big = max(2 * tm + 3, 2 * tn + 3, 300)
    size = 8 * (1 + (big + 2) * (4200 + PAD))
    b = [ga_amd.DeviceBuffer(size) for _ in range(4)]
    yield b
    for x in b:
        x.free()


def run(op, ta, tb, alpha, beta, opa, opb, c0, bufs, guard_rng):
    """gaamd_gemm on op(A) (m x k), op(B) (k x n) and C: the new C, with every guard
    element around C checked unchanged"""
    dt = DT[op]
    m, k = opa.shape
    n = opb.shape[1]
    junk = lambda cnt: guard_rng.integers(-99, 100, cnt)   # noqa: E731
    a = Mat(bufs[0], stored(opa, ta).astype(dt), junk)
    b = Mat(bufs[1], stored(opb, tb).astype(dt), junk)
    c = Mat(bufs[2], c0.astype(dt), junk)
    rc = ga_amd.gemm(op, ta, tb, m, n, k, alpha, a.ptr, a.ld, b.ptr, b.ld, beta, c.ptr, c.ld)
    assert rc == 0, rc
    ga_amd.sync()
    out = c.download()
    got = c.view(out).copy()
    c.view(out)[:, :] = c.view()       # put the old C back: the rest must be the old image
    assert out.tobytes() == c.img.tobytes(), f"guard elements around C changed ({ta}{tb} {m}x{n}x{k})"
    return got


def exact_case(op, ta, tb, m, n, k, bufs, rng):
    dt = DT[op]
    opa = rng.integers(-8, 9, (m, k))
    opb = rng.integers(-8, 9, (k, n))     # random: not symmetric, so a swapped store shows
    c0 = rng.integers(-8, 9, (m, n))
    got = run(op, ta, tb, 2.0, -3.0, opa, opb, c0, bufs, rng)
    want = (2 * (opa.astype(np.int64) @ opb.astype(np.int64)) - 3 * c0).astype(dt)
    bad = np.argwhere(got.view(np.uint8).reshape(m, n, -1) != want.view(np.uint8).reshape(m, n, -1))
    assert got.tobytes() == want.tobytes(), \
        f"{ta}{tb} {m}x{n}x{k}: {np.count_nonzero(got != want)} of {got.size} differ, first at {bad[0][:2] if len(bad) else None}"


@pytest.mark.gpu
@pytest.mark.parametrize("ta,tb", TRANS, ids=lambda t: t)
@pytest.mark.parametrize("op", [DBL, FLT], ids=["dbl", "flt"])
def test_exact_integer_data(gpu_lib, bufs, op, ta, tb):
    tm, tn, tk = tiles()
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
    """operands, scalars and the high-precision reference with its bound, computed once"""
    key = (op, shape)
    if key not in _random_cache:
        m, n, k = shape
        dt = DT[op]
        wide = np.longdouble if op == DBL else np.float64
        rng = np.random.default_rng(7 * op + m + n + k)
        opa = rng.uniform(-2, 2, (m, k)).astype(dt)
        opb = rng.uniform(-2, 2, (k, n)).astype(dt)
        c0 = rng.uniform(-2, 2, (m, n)).astype(dt)
        al, be = dt.type(ALPHA_R), dt.type(BETA_R)
        aw, bw, cw = opa.astype(wide), opb.astype(wide), c0.astype(wide)
        ref = wide(al) * (aw @ bw) + wide(be) * cw
        bound = wide(k + 3) * wide(U[op]) * (abs(wide(al)) * (np.abs(aw) @ np.abs(bw)) + abs(wide(be)) * np.abs(cw))
        for x in (opa, opb, c0, ref, bound):
            x.setflags(write=False)
        _random_cache[key] = (opa, opb, c0, al, be, ref, bound)
    return _random_cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("ta,tb", TRANS, ids=lambda t: t)
@pytest.mark.parametrize("shape", [(257, 131, 1000), (64, 64, 4099)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("op", [DBL, FLT], ids=["dbl", "flt"])
def test_random_data_within_the_rounding_bound(gpu_lib, bufs, op, shape, ta, tb):
    opa, opb, c0, al, be, ref, bound = random_case(op, shape)
    got = run(op, ta, tb, al, be, opa, opb, c0, bufs, np.random.default_rng(5))
    err = np.abs(got.astype(ref.dtype) - ref)
    worst = float(np.max(err / bound))
    print(f"gemm {ga_amd.OP_NAME[op]} {ta}{tb} {shape}: max |err| / bound = {worst:.4f}")
    assert np.all(err <= bound), (worst, np.argwhere(err > bound)[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("op", [DBL, FLT], ids=["dbl", "flt"])
def test_beta_zero_does_not_read_c_alpha_zero_does_not_read_a(gpu_lib, bufs, op):
    tm, tn, tk = tiles()
    dt = DT[op]
    rng = np.random.default_rng(op)
    m, n, k = tm + 3, tn + 2, 2 * tk + 1
    opa = rng.integers(-8, 9, (m, k)).astype(dt)
    opb = rng.integers(-8, 9, (k, n)).astype(dt)
    nan_c = np.full((m, n), np.nan, dtype=dt)
    got = run(op, "N", "N", 2.0, 0.0, opa, opb, nan_c, bufs, rng)
    assert not np.isnan(got).any()
    assert got.tobytes() == (2 * (opa.astype(np.int64) @ opb.astype(np.int64))).astype(dt).tobytes()
    # alpha == 0: exactly beta * C (the scale kernel's x * beta), A full of NaN
    c0 = rng.uniform(-2, 2, (m, n)).astype(dt)
    c0[0, 0], c0[1, 1] = 0.0, -0.0
    nan_a = np.full((m, k), np.nan, dtype=dt)
    for ta, tb in TRANS:
        got = run(op, ta, tb, 0.0, BETA_R, nan_a, opb, c0, bufs, rng)
        assert got.tobytes() == (c0 * dt.type(BETA_R)).tobytes(), (ta, tb)
    # both zero: zeros, C (NaN) not read
    got = run(op, "N", "N", 0.0, 0.0, nan_a, opb, nan_c, bufs, rng)
    assert got.tobytes() == np.zeros((m, n), dtype=dt).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("ta,tb", TRANS, ids=lambda t: t)
@pytest.mark.parametrize("op", [DBL, FLT], ids=["dbl", "flt"])
def test_bits_do_not_depend_on_position(gpu_lib, bufs, op, ta, tb):
    shape = (257, 131, 1000)
    m, n, k = shape
    opa, opb, c0, al, be, ref, bound = random_case(op, shape)
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
    pa = a.at(0, i0) if ta == "T" else a.at(i0, 0)
    pb = b.at(j0, 0) if tb == "T" else b.at(0, j0)
    rc = ga_amd.gemm(op, ta, tb, m - i0, n - j0, k, al, pa, a.ld, pb, b.ld, be, c.at(i0, j0), c.ld)
    assert rc == 0
    ga_amd.sync()
    out = c.download()
    sub = c.view(out)
    assert sub[i0:, j0:].tobytes() == full[i0:, j0:].tobytes(), \
        f"{np.count_nonzero(sub[i0:, j0:] != full[i0:, j0:])} elements differ from the whole product"
    sub[i0:, j0:] = c0[i0:, j0:]
    assert out.tobytes() == c.img.tobytes(), "elements outside the sub-rectangle changed"
