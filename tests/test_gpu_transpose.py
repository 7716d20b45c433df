"""GPU, one rank, kernel level: gaamd_transpose and gaamd_transpose_acc
(ga_amd/csrc/gaamd_transpose.hip), the LDS-tiled kernels under GA_Transpose / GA_Symmetrize.

The tile side T comes from gaamd_transpose_plan, so the shapes follow the kernel: rows and
cols each run over {1, T-1, T, T+1, 2T+3}.

  transpose  4-, 8- and 16-byte elements of random BIT PATTERNS (NaN payloads, -0 included),
             compared as raw bits with numpy's transpose
  acc        c = alpha * (c + b^T) for f64 / f32, alpha in {0.5, -3.0}: bit-exact against
             numpy (one add, then one multiply: nothing for an FMA to contract); with
             alpha = 0.5 and b a copy of a square c the result equals its own transpose
  layouts    tight: ld = row, bases on a 16-byte boundary; pad3: both ld = row + 3;
             shift: both bases one element past a 16-byte boundary (the 16-byte vector path
             has to fall back); vec: ld rounded up to 16 bytes past the row, so the vector
             path runs with ragged edges
  guards     the destination is pre-filled with a sentinel and has guard elements before and
             after; everything but the cols x rows elements -- the ld padding too -- is
             unchanged afterwards
  position   a sub-rectangle transposed alone (offset bases, the same ld) has the bits it
             has in the whole

Spans past 2 GiB and 4 GiB, where the 64-bit offsets matter (rows spread over 9 GiB, only
the rows touched): tests/test_gpu_far_offsets.py.
"""
import numpy as np
import pytest

import ga_amd

INT, DBL, FLT, DCP = ga_amd.COMEX_ACC_INT, ga_amd.COMEX_ACC_DBL, ga_amd.COMEX_ACC_FLT, ga_amd.COMEX_ACC_DCP
ESZ = {INT: 4, DBL: 8, FLT: 4, DCP: 16}
LAYOUTS = ["tight", "pad3", "shift", "vec"]
GUARD = 8            # guard elements before and after; 8 elements are a multiple of 16 bytes
SENTINEL = 0xA5C3F00D


def tile(op):
    rc, p = ga_amd.transpose_plan(op, 1, 1, 1 << 40, 1, 2 << 40, 1)
    assert rc == 0 and p["tile_rows"] == p["tile_cols"]
    return p["tile_rows"]


def sweep(t):
    return [1, t - 1, t, t + 1, 2 * t + 3]


def ld_of(row, esz, layout):
    if layout == "pad3":
        return row + 3
    if layout == "vec":
        per = 16 // esz
        return -(-row // per) * per + per
    return row


class Mat:
    """rows x cols elements of w uint32 words each in a device buffer: GUARD elements, then
    rows * ld, then GUARD; shift: the base lies one element past a 16-byte boundary"""

    def __init__(self, dev, rows, cols, w, layout, fill):
        self.rows, self.cols, self.w = rows, cols, w
        self.ld = ld_of(cols, 4 * w, layout)
        self.first = GUARD + (1 if layout == "shift" else 0)
        self.img = np.empty((self.first + rows * self.ld + GUARD, w), dtype=np.uint32)
        self.img[:] = fill(self.img.shape)
        self.dev = dev
        assert self.img.nbytes <= dev.nbytes and dev.ptr % 16 == 0
        self.ptr = dev.ptr + self.first * 4 * w
        # (a 16-byte element is its own vector: shifted by one it is still on a boundary)
        assert (self.ptr % 16 == 0) == (layout != "shift" or w == 4)

    def view(self, img=None):
        img = self.img if img is None else img
        return img[self.first:self.first + self.rows * self.ld].reshape(self.rows, self.ld, self.w)[:, :self.cols]

    def at(self, i, j):
        return self.ptr + (i * self.ld + j) * 4 * self.w

    def upload(self):
        self.dev.upload(self.img)

    def download(self):
        return self.dev.download(np.uint32, self.img.size).reshape(self.img.shape)


@pytest.fixture(scope="module")
def bufs(gpu_lib):
    big = 2 * 64 + 3 + 8
    b = [ga_amd.DeviceBuffer(16 * (2 * GUARD + 2 + big * big)) for _ in range(3)]
    yield b
    for x in b:
        x.free()


def sentinel(shape):
    return np.full(shape, SENTINEL, dtype=np.uint32)


def words(vals):
    """an array of f64 / f32 as (rows, cols, w) uint32 words"""
    v = np.ascontiguousarray(vals)
    return v.view(np.uint32).reshape(v.shape[0], v.shape[1], v.dtype.itemsize // 4)


def unchanged_but(mat, out):
    """the downloaded image with the matrix's elements put back is the uploaded image"""
    got = mat.view(out).copy()
    mat.view(out)[:] = mat.view()
    assert out.tobytes() == mat.img.tobytes(), "guard or padding elements of the destination changed"
    return got


def do_transpose(op, rows, cols, layout, bufs, rng):
    w = ESZ[op] // 4
    src = Mat(bufs[0], rows, cols, w, layout, lambda s: rng.integers(0, 1 << 32, s, dtype=np.uint32))
    dst = Mat(bufs[1], cols, rows, w, layout, sentinel)
    src.upload()
    dst.upload()
    rc = ga_amd.transpose(op, rows, cols, src.ptr, src.ld, dst.ptr, dst.ld)
    assert rc == 0, rc
    ga_amd.sync()
    got = unchanged_but(dst, dst.download())
    want = src.view().transpose(1, 0, 2)
    assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (op, rows, cols, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("op", [INT, DBL, DCP], ids=["4B", "8B", "16B"])
def test_transpose_bits(op, layout, bufs):
    rng = np.random.default_rng(1000 * op + LAYOUTS.index(layout))
    t = tile(op)
    for rows in sweep(t):
        for cols in sweep(t):
            do_transpose(op, rows, cols, layout, bufs, rng)


@pytest.mark.gpu
def test_transpose_keeps_nan_payloads_and_minus_zero(bufs):
    """named values, beside the random patterns: a signalling-NaN pattern with a payload,
    -0, a denormal and -inf come out as the bits that went in (the kernel moves integers)"""
    pat = np.array([0x7FF0000000000001, 0x8000000000000000, 0x0000000000000001, 0xFFF0000000000000,
                    0x7FF8DEADBEEF0001, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    vals = np.resize(pat, (5, 7))
    src = Mat(bufs[0], 5, 7, 2, "tight", sentinel)
    src.view()[:] = words(vals)
    dst = Mat(bufs[1], 7, 5, 2, "tight", sentinel)
    src.upload()
    dst.upload()
    assert ga_amd.transpose(DBL, 5, 7, src.ptr, src.ld, dst.ptr, dst.ld) == 0
    ga_amd.sync()
    got = unchanged_but(dst, dst.download())
    assert got.tobytes() == np.ascontiguousarray(vals.T).tobytes()


def do_acc(op, m, n, alpha, layout, bufs, rng, b_is_c=False):
    dt = ga_amd.OP_DTYPE[op]
    w = dt.itemsize // 4
    cv = (rng.standard_normal((m, n)) * 10.0 ** rng.integers(-3, 4, (m, n))).astype(dt)
    bv = cv.copy() if b_is_c else (rng.standard_normal((n, m)) * 10.0 ** rng.integers(-3, 4, (n, m))).astype(dt)
    b = Mat(bufs[0], n, m, w, layout, sentinel)
    c = Mat(bufs[1], m, n, w, layout, sentinel)
    b.view()[:] = words(bv)
    c.view()[:] = words(cv)
    b.upload()
    c.upload()
    rc = ga_amd.transpose_acc(op, m, n, alpha, b.ptr, b.ld, c.ptr, c.ld)
    assert rc == 0, rc
    ga_amd.sync()
    got = unchanged_but(c, c.download())
    want = dt.type(alpha) * (cv + bv.T)        # stays in dt: one add, one multiply
    assert want.dtype == dt
    assert got.tobytes() == words(want).tobytes(), (op, m, n, alpha, layout)
    return np.ascontiguousarray(got).view(dt).reshape(m, n)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("op", [DBL, FLT], ids=["f64", "f32"])
def test_transpose_acc_bits(op, layout, bufs):
    rng = np.random.default_rng(7000 + 10 * op + LAYOUTS.index(layout))
    t = tile(op)
    for m in sweep(t):
        for n in sweep(t):
            for alpha in (0.5, -3.0):
                do_acc(op, m, n, alpha, layout, bufs, rng)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("op", [DBL, FLT], ids=["f64", "f32"])
def test_symmetrized_square_equals_its_transpose(op, layout, bufs):
    """alpha = 0.5, b a copy of c: 0.5 * (a_ij + a_ji) is the same number on both sides
    of the diagonal, because addition commutes"""
    rng = np.random.default_rng(4242 + op)
    n = 2 * tile(op) + 3
    got = do_acc(op, n, n, 0.5, layout, bufs, rng, b_is_c=True)
    assert got.tobytes() == np.ascontiguousarray(got.T).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("op", [INT, DBL, DCP], ids=["4B", "8B", "16B"])
def test_transpose_position_independence(op, bufs):
    rng = np.random.default_rng(99 + op)
    t = tile(op)
    w = ESZ[op] // 4
    rows, cols = 2 * t + 3, t + 9
    src = Mat(bufs[0], rows, cols, w, "pad3", lambda s: rng.integers(0, 1 << 32, s, dtype=np.uint32))
    whole = Mat(bufs[1], cols, rows, w, "pad3", sentinel)
    part = Mat(bufs[2], cols, rows, w, "pad3", sentinel)
    for x in (src, whole, part):
        x.upload()
    assert ga_amd.transpose(op, rows, cols, src.ptr, src.ld, whole.ptr, whole.ld) == 0
    # rows r0 .. r0 + nr, columns c0 .. c0 + nc of src alone, to the same place of `part`
    r0, c0, nr, nc = 17, 5, t + 11, t - 3
    assert ga_amd.transpose(op, nr, nc, src.at(r0, c0), src.ld, part.at(c0, r0), part.ld) == 0
    ga_amd.sync()
    wv, pv = whole.view(whole.download()), part.view(part.download())
    assert wv.tobytes() == np.ascontiguousarray(src.view().transpose(1, 0, 2)).tobytes()
    assert pv[c0:c0 + nc, r0:r0 + nr].tobytes() == wv[c0:c0 + nc, r0:r0 + nr].tobytes()
    pv = pv.copy()
    pv[c0:c0 + nc, r0:r0 + nr] = SENTINEL
    assert (pv == SENTINEL).all(), "the partial transpose wrote outside its rectangle"


@pytest.mark.gpu
@pytest.mark.parametrize("op", [DBL, FLT], ids=["f64", "f32"])
def test_transpose_acc_position_independence(op, bufs):
    rng = np.random.default_rng(314 + op)
    dt = ga_amd.OP_DTYPE[op]
    t = tile(op)
    w = dt.itemsize // 4
    m, n = t + 9, 2 * t + 3
    cv = rng.standard_normal((m, n)).astype(dt)
    bv = rng.standard_normal((n, m)).astype(dt)
    b = Mat(bufs[0], n, m, w, "pad3", sentinel)
    b.view()[:] = words(bv)
    b.upload()
    outs = []
    i0, j0, mi, nj = 5, 17, t - 3, t + 11
    for sub in (False, True):
        c = Mat(bufs[1 + sub], m, n, w, "pad3", sentinel)
        c.view()[:] = words(cv)
        c.upload()
        if sub:
            rc = ga_amd.transpose_acc(op, mi, nj, -3.0, b.at(j0, i0), b.ld, c.at(i0, j0), c.ld)
        else:
            rc = ga_amd.transpose_acc(op, m, n, -3.0, b.ptr, b.ld, c.ptr, c.ld)
        assert rc == 0
        ga_amd.sync()
        outs.append(c.view(c.download()).copy())
    whole, part = outs
    assert part[i0:i0 + mi, j0:j0 + nj].tobytes() == whole[i0:i0 + mi, j0:j0 + nj].tobytes()
    part[i0:i0 + mi, j0:j0 + nj] = words(cv)[i0:i0 + mi, j0:j0 + nj]
    assert part.tobytes() == words(cv).tobytes(), "the partial call changed c outside its rectangle"
