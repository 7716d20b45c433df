"""GPU, one rank, kernel level: gaamd_patch_norm, gaamd_diagonal, gaamd_scale_rows and
gaamd_scale_cols against a numpy restatement of the reference loops (global/src/matrix.c),
compared as raw bits.  The restatement (ref_* below) is checked on the CPU against plain Python
loops written from matrix.c's expressions (tests/test_matrix_abi.py).

  |x|          GA_ABS(x) = x >= 0 ? x : -x (INT_MIN wraps to itself, -0.0 stays -0.0);
               complex sqrt(re*re + im*im): two products, one sum, the correctly rounded root
  norm1        the sum of |x| in the element's own type (complex: its real type)   1118-1171
  norm inf     the maximum of |x|                                                  801-859
  add / shift  a += v / a += c, complex real and imaginary part each               1640-1690, 2080-2127
  scale        a *= v, complex re *= v.re and im *= v.im (not a complex product)   2494-2503, 2700-2710
Integers in unsigned arithmetic (wraparound).

Constants of the kernels, read from ga_amd/csrc/gaamd_patch.hip: a workgroup of the norm sums
kDotItems items of kDotBS vectors, the final workgroup takes kDotBS * kFinalPer partials per pass.
"""
import decimal
import os
import re

import numpy as np
import pytest

import ga_amd
import test_gpu_ga_math as K

INT, LNG, FLT, DBL, CPL, DCP = K.INT, K.LNG, K.FLT, K.DBL, K.CPL, K.DCP
OPS = K.OPS
DT, UNS, REAL = K.DT, K.UNS, K.REAL
ONE, INF = ga_amd.GAAMD_NORM_ONE, ga_amd.GAAMD_NORM_INF
GET, SET, ADD, SHIFT, ZERO = (ga_amd.GAAMD_DIAG_GET, ga_amd.GAAMD_DIAG_SET, ga_amd.GAAMD_DIAG_ADD,
                              ga_amd.GAAMD_DIAG_SHIFT, ga_amd.GAAMD_DIAG_ZERO)
FNS = [GET, SET, ADD, SHIFT, ZERO]
FN_NAME = {GET: "get", SET: "set", ADD: "add", SHIFT: "shift", ZERO: "zero"}
SHIFT_C = {INT: -7, LNG: 0x123456789, FLT: 0.7, DBL: -1.0 / 3.0, CPL: complex(0.7, -0.3), DCP: complex(-1.0 / 3.0, 0.3)}
opid = dict(ids=lambda o: ga_amd.OP_NAME[o])

_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ga_amd", "csrc",
                         "gaamd_patch.hip")).read()
K_DOT_BS, K_DOT_ITEMS, K_FINAL_PER = (int(re.search(rf"constexpr int {n} = (\d+);", _SRC).group(1))
                                      for n in ("kDotBS", "kDotItems", "kFinalPer"))


# ---- the reference restated --------------------------------------------------------
def real_dt(op):
    return REAL.get(op, DT[op])


def ref_abs(op, x):
    """the per-element quantity of both norms, in the element's (complex: real) type"""
    if op in UNS:
        u = UNS[op]
        return np.where(x >= 0, x, (np.zeros(1, dtype=u) - x.view(u)).view(DT[op]))
    if op in REAL:
        re_, im = x.real.copy(), x.imag.copy()
        return np.sqrt(re_ * re_ + im * im)
    return np.where(x >= 0, x, -x)


def max_key(q):
    """the order the maximum is taken in: as the values, with -0.0 (and INT_MIN) below +0"""
    u = np.dtype(f"u{q.dtype.itemsize}")
    return q.view(u) ^ u.type(1 << (8 * q.dtype.itemsize - 1))


def ref_norm_inf(op, x):
    q = ref_abs(op, x)
    return q[np.argmax(max_key(q)):][:1].copy()


def ref_norm1_exact(op, x):
    """norm1 where every partial sum is exact (integers; data checked by exactly_summable)"""
    q = ref_abs(op, x)
    if op in UNS:
        return np.array([q.view(UNS[op]).sum(dtype=UNS[op])]).view(DT[op])
    return np.array([q.astype(np.float64).sum()], dtype=q.dtype)


def ref_diag_add(op, a, v):
    """a + v, v an array or one element; complex part by part"""
    v = np.asarray(v, dtype=DT[op])
    if op in UNS:
        return (a.view(UNS[op]) + v.reshape(-1).view(UNS[op])).view(DT[op])
    if op in REAL:
        return K._cplx(op, a.real + v.real, a.imag + v.imag)
    return a + v


def ref_scale(op, a, v, rows):
    """a[i][j] * v[i] (rows) or * v[j]; complex re * v.re, im * v.im"""
    m = v[:, None] if rows else v[None, :]
    if op in UNS:
        return (a.view(UNS[op]) * m.view(UNS[op])).view(DT[op])
    if op in REAL:
        return K._cplx(op, a.real * m.real, a.imag * m.imag)
    return a * m


# ---- data ---------------------------------------------------------------------------
def gen_exact(op, n, rng):
    """data whose sum of |x| is exact in any order: integers; eighths in {-1/8, 0, 1/8};
    complex (3, 4) * k / 8 with k in {-1, 0, 0, 0, 1} in either arrangement, moduli 0 or 5/8"""
    if op in UNS:
        return K.gen(op, n, rng)
    if op in REAL:
        k = rng.choice(np.array([-1, 0, 0, 0, 1]), n).astype(REAL[op]) / 8
        sw = rng.integers(0, 2, n).astype(bool)
        return K._cplx(op, np.where(sw, 3 * k, -4 * k), np.where(sw, 4 * k, 3 * k))
    return (rng.integers(-1, 2, n) / 8).astype(DT[op])


def exactly_summable(op, x):
    """forward, reverse and pairwise sums of |x| in the element type agree bit for bit, and the
    sum in units of the grain stays below 2^24 / 2^53"""
    q = ref_abs(op, x)
    if op in UNS:
        return True
    fwd = np.cumsum(q, dtype=q.dtype)[-1]
    rev = np.cumsum(q[::-1], dtype=q.dtype)[-1]
    pair = q.sum(dtype=q.dtype)
    units = float(q.astype(np.float64).sum() * 8)
    return fwd.tobytes() == rev.tobytes() == pair.tobytes() and units < 2.0 ** (24 if q.dtype.itemsize == 4 else 53)


def long_run_elems(op):
    """a contiguous run whose norm needs a second pass of the final workgroup"""
    per_wg = K_DOT_ITEMS * K_DOT_BS * 16 // DT[op].itemsize
    return per_wg * (K_DOT_BS * K_FINAL_PER + 2) + 5


# (count, block extents, base offset in bytes)
def norm_shapes(op):
    esz = DT[op].itemsize
    out = []
    for off in (0, esz, 8 if esz == 4 else 4):
        out += [([1], [1], off), ([53, 37], [53, 37], off), ([53, 37], [64, 37], off), ([7, 6, 5], [8, 7, 5], off),
                ([300], [300], off)]
    return out


def test_exact_data_sets_are_order_independent():
    """CPU: the equality asserted for GAAMD_NORM_ONE tests the kernel, not the data"""
    for op in OPS:
        rng = np.random.default_rng(50 + op)
        for n in (1, 53 * 37, 7 * 6 * 5, 300, long_run_elems(op)):
            assert exactly_summable(op, gen_exact(op, n, rng)), (ga_amd.OP_NAME[op], n)
    # and the check can fail: thirds are not exactly summable
    assert not exactly_summable(FLT, (np.arange(1, 4000) / 3).astype(np.float32))


# ---- device plumbing ----------------------------------------------------------------
LEAD = 256


@pytest.fixture(scope="module")
def bufs(gpu_lib):
    b = [ga_amd.DeviceBuffer(40 << 20), ga_amd.DeviceBuffer(2 << 20)]
    yield b
    for x in b:
        x.free()


def back(dev, nbytes):
    ga_amd.sync()
    return dev.download(np.uint8, nbytes)


def norm_dev(dev, op, kind, base, stride, count):
    rc, out = ga_amd.patch_norm(op, kind, dev.ptr + base, stride, count)
    assert rc == 0, rc
    return out


def patch_image(op, count, ext, off, x):
    stride, base, offs, nbytes = K.geometry(op, count, ext, off)
    base += LEAD - K.LEAD
    offs = offs + (LEAD - K.LEAD)
    img = K.make_buf(op, nbytes + LEAD, base, np.random.default_rng(7))
    K.put(img, offs, x)
    return stride, base, img


# ---- norms ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, **opid)
def test_norm_exact_and_inf_on_shapes(gpu_lib, bufs, op):
    dev = bufs[0]
    rng = np.random.default_rng(11 * op)
    for count, ext, off in norm_shapes(op):
        n = int(np.prod(count))
        tag = (ga_amd.OP_NAME[op], count, ext, off)
        x = gen_exact(op, n, rng)
        assert exactly_summable(op, x), tag
        stride, base, img = patch_image(op, count, ext, off, x)
        dev.upload(img)
        got = norm_dev(dev, op, ONE, base, stride, count)
        assert got.tobytes() == ref_norm1_exact(op, x).tobytes(), (tag, got, ref_norm1_exact(op, x))
        y = K.gen(op, n, rng)
        stride, base, img = patch_image(op, count, ext, off, y)
        dev.upload(img)
        got = norm_dev(dev, op, INF, base, stride, count)
        assert got.tobytes() == ref_norm_inf(op, y).tobytes(), (tag, got, ref_norm_inf(op, y))
        assert back(dev, img.size).tobytes() == img.tobytes(), ("the patch was written", tag)


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, **opid)
def test_norm_past_one_pass_of_the_final_workgroup(gpu_lib, bufs, op):
    dev = bufs[0]
    n = long_run_elems(op)
    assert -(-n * DT[op].itemsize // (K_DOT_ITEMS * K_DOT_BS * 16)) > K_DOT_BS * K_FINAL_PER
    rng = np.random.default_rng(50 + op)
    for _ in (1, 53 * 37, 7 * 6 * 5, 300):   # the stream test_exact_data_sets_are_order_independent checked
        gen_exact(op, _, rng)
    x = gen_exact(op, n, rng)
    dev.upload(x, LEAD)
    got = norm_dev(dev, op, ONE, LEAD, [], [n])
    assert got.tobytes() == ref_norm1_exact(op, x).tobytes(), (got, ref_norm1_exact(op, x))
    # the maximum in the last element, then in the first workgroup's first lane
    q = ref_abs(op, x)
    big = {INT: 2 ** 31 - 1, LNG: 2 ** 63 - 1}.get(op, 7.5)
    for pos in (n - 1, 0, n // 2 + 1):
        y = x.copy()
        y[pos] = np.array([complex(0, -big) if op in REAL else -big], dtype=DT[op])[0]
        dev.upload(y[pos:pos + 1], LEAD + pos * DT[op].itemsize)
        got = norm_dev(dev, op, INF, LEAD, [], [n])
        assert got.tobytes() == ref_norm_inf(op, y).tobytes() == np.array([big], dtype=q.dtype).tobytes(), (pos, got)
        dev.upload(x[pos:pos + 1], LEAD + pos * DT[op].itemsize)


def exact_norm1(op, x):
    """(the sum of the exact |x|, as Decimal; n)"""
    decimal.getcontext().prec = 60
    if op in REAL:
        vals = [(decimal.Decimal(float(r)) ** 2 + decimal.Decimal(float(i)) ** 2).sqrt() for r, i in zip(x.real, x.imag)]
    else:
        vals = [abs(decimal.Decimal(float(v))) for v in x]
    return sum(vals)


@pytest.mark.gpu
@pytest.mark.parametrize("op", [FLT, DBL, CPL, DCP], **opid)
def test_norm1_rounding_bound_and_reproducible(gpu_lib, bufs, op):
    """seeded random data: |got - exact| <= gamma * sum|x|, gamma = (n+3)u / (1 - (n+3)u): the
    any-order summation bound (n-1 additions) plus the modulus's own roundings (two products
    rounded once each before a sum, the sum, the root: at most 3u to first order on an element)"""
    dev = bufs[0]
    u = 2.0 ** -24 if real_dt(op).itemsize == 4 else 2.0 ** -53
    rng = np.random.default_rng(77 + op)
    for count, ext, off in [s for s in norm_shapes(op) if s[2] in (0, DT[op].itemsize)]:
        n = int(np.prod(count))
        x = K.gen(op, n, rng)
        stride, base, img = patch_image(op, count, ext, off, x)
        dev.upload(img)
        got = norm_dev(dev, op, ONE, base, stride, count)
        again = norm_dev(dev, op, ONE, base, stride, count)
        assert got.tobytes() == again.tobytes()
        exact = exact_norm1(op, x)
        gamma = decimal.Decimal((n + 3) * u / (1 - (n + 3) * u))
        err = abs(decimal.Decimal(float(got[0])) - exact)
        print(f"norm1 {ga_amd.OP_NAME[op]} {count} off {off}: err {float(err):.3e} bound {float(gamma * exact):.3e}")
        assert err <= gamma * exact, (count, off, float(err), float(gamma * exact))


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, **opid)
def test_norm_inf_positions_zeros_and_wrap(gpu_lib, bufs, op):
    dev = bufs[0]
    dt = DT[op]
    esz = dt.itemsize
    rng = np.random.default_rng(5 * op)
    count, ext = [53, 37], [64, 37]
    n = 53 * 37
    big = np.array([complex(-300, 400) if op in REAL else -500], dtype=dt)
    for off in (0, esz):
        for pos in (n - 1, 52, 0, 36 * 53 + 48):   # last element (last lane of a tail vector), end of row 0, first
            x = K.gen(op, n, rng, small=100)
            x[pos] = big[0]
            stride, base, img = patch_image(op, count, ext, off, x)
            dev.upload(img)
            got = norm_dev(dev, op, INF, base, stride, count)
            assert got.tobytes() == ref_norm_inf(op, x).tobytes() == np.array([500], dtype=real_dt(op)).tobytes(), (off, pos)
    if op not in UNS:
        # -0.0 only: -0.0 for the real types (GA_ABS keeps the sign), +0.0 for complex (a modulus);
        # one +0.0 among them: +0.0
        x = -np.zeros(n, dtype=dt) if op not in REAL else K._cplx(op, -np.zeros(n, REAL[op]), -np.zeros(n, REAL[op]))
        for k, y in enumerate((x, np.concatenate([x[:700], np.zeros(1, dtype=dt), x[701:]]))):
            stride, base, img = patch_image(op, count, ext, 0, y)
            dev.upload(img)
            for kind in (INF, ONE):
                got = norm_dev(dev, op, kind, base, stride, count)
                want = ref_norm_inf(op, y) if kind == INF else np.zeros(1, dtype=real_dt(op))
                assert got.tobytes() == want.tobytes(), (k, kind, got, want)
            minus = np.array([-0.0], dtype=real_dt(op)).tobytes()
            assert (ref_norm_inf(op, y).tobytes() == minus) == (k == 0 and op not in REAL)
    else:
        # INT_MIN: |INT_MIN| wraps to INT_MIN, which loses every signed comparison and adds as 2^31
        info = np.iinfo(dt)
        x = K.gen(op, n, rng, small=1000)
        x[5] = info.min
        x[1900] = info.max
        x[1901] = info.max   # the sum wraps
        stride, base, img = patch_image(op, count, ext, 0, x)
        dev.upload(img)
        assert norm_dev(dev, op, INF, base, stride, count)[0] == info.max
        got = norm_dev(dev, op, ONE, base, stride, count)
        want = (sum(abs(int(v)) for v in x) % (1 << (8 * esz)))
        assert int(got.view(UNS[op])[0]) == want and got.tobytes() == ref_norm1_exact(op, x).tobytes()
        x[:] = info.min   # INT_MIN alone is its own maximum
        stride, base, img = patch_image(op, count, ext, 0, x)
        dev.upload(img)
        assert norm_dev(dev, op, INF, base, stride, count)[0] == info.min


# ---- diagonal -------------------------------------------------------------------------
def special_values(op, x):
    """NaNs with payloads and -0.0 among x (floating-point types): GET / SET are bit copies"""
    if op in UNS:
        return x
    r = real_dt(op)
    w = x.view(r).copy()
    u = w.view(f"u{r.itemsize}")
    nan = (0x7FC12345 if r.itemsize == 4 else 0x7FF8000012345678)
    for i in range(0, w.size, 5):
        u[i] = nan + i
    w[1::7] = -0.0
    return w.view(DT[op])


# (rows, cols, ld, base offset in bytes)
def diag_geoms(op):
    esz = DT[op].itemsize
    g = [(1, 1, 1, 0), (37, 37, 37, 0), (37, 53, 53, 0), (53, 37, 37, 0), (37, 53, 64, 0), (300, 300, 301, 0),
         (37, 53, 53, esz), (300, 300, 301, 4)]
    if esz == 16:
        g.append((37, 37, 37, 8))   # a 16-byte element on a base that is 8-byte but not 16-byte aligned
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("fn", FNS, ids=lambda f: FN_NAME[f])
@pytest.mark.parametrize("op", OPS, **opid)
def test_diagonal_bit_exact(gpu_lib, bufs, op, fn):
    da, dv = bufs
    dt = DT[op]
    esz = dt.itemsize
    rng = np.random.default_rng(1000 * op + fn)
    for rows, cols, ld, off in diag_geoms(op):
        n = min(rows, cols)
        tag = (ga_amd.OP_NAME[op], FN_NAME[fn], rows, cols, ld, off)
        base = LEAD + off
        nbytes = base + ((rows - 1) * ld + cols) * esz + 64
        img = K.make_buf(op, nbytes, base, rng)
        idx = base + np.arange(n, dtype=np.int64) * (ld + 1) * esz
        a = K.take(img, idx, dt)
        v = K.gen(op, n, rng)
        if fn in (GET, SET):
            a, v = special_values(op, a), special_values(op, v[::-1].copy())[::-1].copy()
            K.put(img, idx, a)
        vbase = 256 + (off % 16)
        vimg = K.make_buf(op, vbase + n * esz + 256, vbase, rng)
        K.put(vimg, vbase + np.arange(n, dtype=np.int64) * esz, v)
        da.upload(img)
        dv.upload(vimg)
        rc = ga_amd.diag(op, fn, n, da.ptr + base, (ld + 1) * esz, dv.ptr + vbase if fn in (GET, SET, ADD) else None,
                         esz, scalar=SHIFT_C[op] if fn == SHIFT else None)
        assert rc == 0, (tag, rc)
        want_a, want_v = img.copy(), vimg.copy()
        if fn == GET:
            K.put(want_v, vbase + np.arange(n, dtype=np.int64) * esz, a)
        elif fn == SET:
            K.put(want_a, idx, v)
        elif fn == ADD:
            K.put(want_a, idx, ref_diag_add(op, a, v))
        elif fn == SHIFT:
            K.put(want_a, idx, ref_diag_add(op, a, K.scalar(op, SHIFT_C[op])))
        else:
            K.put(want_a, idx, np.zeros(n, dtype=dt))
        got_a, got_v = back(da, img.size), back(dv, vimg.size)
        assert got_a.tobytes() == want_a.tobytes(), (tag, "matrix image", np.flatnonzero(got_a != want_a)[:8])
        assert got_v.tobytes() == want_v.tobytes(), (tag, "vector image", np.flatnonzero(got_v != want_v)[:8])
        if fn in (ADD, SHIFT) and op in REAL:   # part by part
            got = K.take(got_a, idx, dt)
            other = v if fn == ADD else K.scalar(op, SHIFT_C[op])
            assert (got.real == a.real + other.real).all() and (got.imag == a.imag + other.imag).all()


# ---- scale rows / cols ----------------------------------------------------------------
SCALE_GEOMS = [(1, 1, 1, 0), (37, 53, 53, 0), (37, 53, 64, 0), (53, 37, 37, 0), (37, 53, 53, 4), (37, 53, 64, 8),
               (70001, 3, 3, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("rows_call", [True, False], ids=["rows", "cols"])
@pytest.mark.parametrize("op", OPS, **opid)
def test_scale_rows_cols_bit_exact(gpu_lib, bufs, op, rows_call):
    da, dv = bufs
    dt = DT[op]
    esz = dt.itemsize
    rng = np.random.default_rng(2000 * op + rows_call)
    for rows, cols, ld, off in SCALE_GEOMS:
        tag = (ga_amd.OP_NAME[op], "rows" if rows_call else "cols", rows, cols, ld, off)
        base = LEAD + off
        img = K.make_buf(op, base + ((rows - 1) * ld + cols) * esz + 64, base, rng)
        offs = K.offsets(esz, base, [cols, rows], [ld * esz])
        a = K.take(img, offs, dt).reshape(rows, cols)
        nv = rows if rows_call else cols
        v = K.gen(op, nv, rng)   # complex: imaginary parts differ from the real ones
        if op in REAL:
            assert (v.real != v.imag).all()
        vbase = 256 + (off % 16)
        vimg = K.make_buf(op, vbase + nv * esz + 256, vbase, rng)
        K.put(vimg, vbase + np.arange(nv, dtype=np.int64) * esz, v)
        da.upload(img)
        dv.upload(vimg)
        call = ga_amd.scale_rows if rows_call else ga_amd.scale_cols
        assert call(op, rows, cols, da.ptr + base, ld, dv.ptr + vbase) == 0, tag
        want = img.copy()
        ref = ref_scale(op, a, v, rows_call)
        K.put(want, offs, ref.reshape(-1))
        got = back(da, img.size)
        assert got.tobytes() == want.tobytes(), (tag, np.flatnonzero(got != want)[:8])   # padding and canaries too
        assert back(dv, vimg.size).tobytes() == vimg.tobytes(), (tag, "v was written")
        if op in REAL and rows > 1:   # a complex product would differ
            m = v[:, None] if rows_call else v[None, :]
            assert ref.tobytes() != (a * m).astype(dt).tobytes()
        elif op not in UNS and op not in REAL:
            assert ref.tobytes() == (a * (v[:, None] if rows_call else v[None, :])).tobytes()


# ---- offsets past 2^32 bytes ------------------------------------------------------------
# One allocation that is never filled or copied whole: only the touched elements are uploaded
# and compared, plus canaries where an offset truncated to 32 bits (offset mod 2^32) or taken as
# a signed 32-bit number (offset - 2^31 is where bit 31 alone would land) would have written.
G = 1 << 30
FAR_LD = 32768                     # f64: row r of the far matrix at r * 256 KiB
FAR_N = 16385                      # the last diagonal element at 16384 * 32769 * 8 = 4 GiB + 128 KiB
FAR_V = 4 * G + (1 << 20)          # v: behind the matrix's span
FAR_ALLOC = 4 * G + (2 << 20)
CANARY = 64


@pytest.fixture(scope="module")
def far(gpu_lib):
    dev = ga_amd.DeviceBuffer(FAR_ALLOC)
    yield dev
    dev.free()


def far_canaries(dev, offs, seed):
    """known bytes where truncated offsets would land; returns [(offset, bytes)]"""
    rng = np.random.default_rng(seed)
    out = []
    for o in offs:
        for c in (o % (1 << 32), o - (1 << 31)):
            if 0 <= c < FAR_ALLOC - CANARY and c != o:
                b = rng.integers(0, 256, CANARY, dtype=np.uint8)
                dev.upload(b, c)
                out.append((c, b))
    return out


def check_canaries(dev, canaries, skip=()):
    for c, b in canaries:
        got = dev.download(np.uint8, CANARY, c)
        keep = np.ones(CANARY, dtype=bool)
        for lo, hi in skip:   # bytes the call legitimately owns
            keep[max(0, lo - c):max(0, hi - c)] = False
        assert (got[keep] == b[keep]).all(), f"canary at {c:#x} was written"


@pytest.mark.gpu
def test_diagonal_far(gpu_lib, far):
    rng = np.random.default_rng(1)
    step = (FAR_LD + 1) * 8
    idx = [0, 1, 8191, 8192, 8193, FAR_N - 2, FAR_N - 1]   # 8192: the element at 2^31 + 64 KiB
    assert (FAR_N - 1) * step > (1 << 32) and 8192 * step > (1 << 31)
    canaries = far_canaries(far, [i * step for i in idx[2:]], 3)
    a = K.gen(DBL, len(idx), rng)
    v = K.gen(DBL, FAR_N, rng)
    for i, x in zip(idx, a):
        far.upload(np.array([x]), i * step)
    far.upload(v, FAR_V)
    assert ga_amd.diag(DBL, ADD, FAR_N, far.ptr, step, far.ptr + FAR_V, 8) == 0
    ga_amd.sync()
    for i, x in zip(idx, a):
        got = far.download(np.float64, 1, i * step)
        assert got.tobytes() == (np.array([x]) + v[i:i + 1]).tobytes(), i
    # GET back into a compact vector: the far side is the source
    assert ga_amd.diag(DBL, GET, FAR_N, far.ptr, step, far.ptr + FAR_V, 8) == 0
    ga_amd.sync()
    got = far.download(np.float64, FAR_N, FAR_V)
    for i, x in zip(idx, a):
        assert got[i:i + 1].tobytes() == (np.array([x]) + v[i:i + 1]).tobytes(), i
    check_canaries(far, canaries)


FAR_ROWS, FAR_COLS, FAR_ROW_LD = 5, 3, (G + 128) // 8   # row 4 at 4 GiB + 512, row 2 at 2 GiB + 256


@pytest.mark.gpu
def test_scale_rows_and_norm_far(gpu_lib, far):
    rng = np.random.default_rng(2)
    rowoff = [r * FAR_ROW_LD * 8 for r in range(FAR_ROWS)]
    assert rowoff[-1] > (1 << 32) and rowoff[2] > (1 << 31)
    canaries = far_canaries(far, rowoff[2:], 4)
    a = (rng.integers(-8, 9, (FAR_ROWS, FAR_COLS)) / 8).astype(np.float64)
    a[4, 2] = -9.5   # the maximum lies in the far row
    v = K.gen(DBL, FAR_ROWS, rng)
    for r in range(FAR_ROWS):
        far.upload(a[r], rowoff[r])
    q1 = norm_dev(far, DBL, ONE, 0, [FAR_ROW_LD * 8], [FAR_COLS, FAR_ROWS])
    qi = norm_dev(far, DBL, INF, 0, [FAR_ROW_LD * 8], [FAR_COLS, FAR_ROWS])
    assert q1.tobytes() == ref_norm1_exact(DBL, a.reshape(-1)).tobytes() and qi[0] == 9.5
    vat = 4 * G + (1 << 20)
    far.upload(v, vat)
    assert ga_amd.scale_rows(DBL, FAR_ROWS, FAR_COLS, far.ptr, FAR_ROW_LD, far.ptr + vat) == 0
    ga_amd.sync()
    want = ref_scale(DBL, a, v, True)
    for r in range(FAR_ROWS):
        assert far.download(np.float64, FAR_COLS, rowoff[r]).tobytes() == want[r].tobytes(), r
    check_canaries(far, canaries)
