"""GPU, one rank, kernel level: gaamd_spmv, gaamd_sprs_diag, gaamd_sprs_scale_left and
gaamd_sprs_scale_right against a numpy restatement of the contract in include/ga_amd.h, compared
as raw bits.  The restatement (ref_assemble / build_csr -> block CSR, ref_spmv with lane-strided
partials and the butterfly, ref_diag_get / ref_diag_shift, mul) is checked on the CPU against plain
Python loops written from the contract (tests/test_sprs_abi.py) and is what the GA-level worker
(tests/ga_sprs_worker.py) models the whole matrix with.

  owner        index i of a dimension of dim belongs to min((i * nproc) / dim, nproc - 1)
  assembly     the owner of a row holds its elements by source rank, then insertion order, and
               stable-sorts them by (column block, row, column)
  product      a * x in the element's type; integers unsigned; complex
               re = a.re*x.re - a.im*x.im, im = a.re*x.im + a.im*x.re, each operation rounded
  row sum      the row's entries over the blocks in ascending order are e_0 .. e_{c-1}; lane L of W
               sums e_L, e_{L+W}, ... from +0; then p[l] = p[l] + p[l ^ s] for s = 1, 2, .. W / 2
"""
import numpy as np
import pytest

import ga_amd
import test_gpu_ga_math as K

INT, LNG, FLT, DBL, CPL, DCP = K.INT, K.LNG, K.FLT, K.DBL, K.CPL, K.DCP
OPS = K.OPS
DT, UNS, REAL = K.DT, K.UNS, K.REAL
GET, SHIFT = ga_amd.GAAMD_DIAG_GET, ga_amd.GAAMD_DIAG_SHIFT
TEAMS = [1, 2, 4, 8, 16, 32, 64]   # every value gaamd_spmv_team can return
SHIFT_C = {INT: 0x7FFFFFF0, LNG: -0x7FFFFFFFFFFFFFF0, FLT: 0.7, DBL: -1.0 / 3.0, CPL: complex(0.7, -0.3),
           DCP: complex(-1.0 / 3.0, 0.3)}
LEAD = 64
opid = dict(ids=lambda o: ga_amd.OP_NAME[o])


# ---- the contract restated ----------------------------------------------------------
def owner(i, dim, nproc):
    """the rank (column block) of index i; i a Python int or an integer array"""
    if isinstance(i, np.ndarray):
        return np.minimum((i.astype(np.int64) * nproc) // dim, nproc - 1)
    return min((int(i) * nproc) // dim, nproc - 1)


def own_range(dim, nproc, p):
    """[lo, hi] of the indices owner() gives to p; hi = lo - 1 when there are none"""
    first = lambda q: dim if q >= nproc else -((-q * dim) // nproc)   # noqa: E731  (the ceiling)
    return first(p), first(p + 1) - 1


def build_csr(i, j, v, ilo, nrows, jdim, ncut, keep_empty=False):
    """the block CSR of the elements (i, j, v), given in source-rank then insertion order, for the
    rows [ilo, ilo + nrows) and ncut column blocks: a stable sort by (block, row, column)"""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    blk = owner(j, jdim, ncut) if len(j) else np.zeros(0, dtype=np.int64)
    order = np.lexsort((j, i, blk))   # stable; the last key is the primary one
    i, j, v, blk = i[order], j[order], v[order], blk[order]
    blocks = list(range(ncut)) if keep_empty else sorted(set(blk.tolist()))
    offs = np.zeros((len(blocks), nrows + 1), dtype=np.int32)
    start = np.zeros(len(blocks), dtype=np.int64)
    for b, ident in enumerate(blocks):
        sel = blk == ident
        start[b] = np.searchsorted(blk, ident, "left")   # an empty block starts where the next one does
        offs[b, 1:] = np.cumsum(np.bincount(i[sel] - ilo, minlength=nrows))
    return dict(ilo=ilo, nrows=nrows, blocks=blocks, start=start, offs=offs, jdx=j.astype(np.int32),
                val=np.ascontiguousarray(v))


def ref_assemble(parts, idim, jdim, nproc, rank):
    """parts[r] = (i, j, v): what rank r added, in insertion order.  What `rank` holds afterwards."""
    ilo, ihi = own_range(idim, nproc, rank)
    ii, jj, vv = [], [], []
    for i, j, v in parts:
        mine = owner(np.asarray(i, dtype=np.int64), idim, nproc) == rank if len(i) else np.zeros(0, dtype=bool)
        ii.append(np.asarray(i)[mine])
        jj.append(np.asarray(j)[mine])
        vv.append(np.asarray(v)[mine])
    return build_csr(np.concatenate(ii), np.concatenate(jj), np.concatenate(vv), ilo, ihi - ilo + 1, jdim, nproc)


def mul(op, a, x):
    if op in UNS:
        return (a.view(UNS[op]) * x.view(UNS[op])).view(DT[op])
    if op in REAL:
        ar, ai, xr, xi = a.real.copy(), a.imag.copy(), x.real.copy(), x.imag.copy()
        return K._cplx(op, ar * xr - ai * xi, ar * xi + ai * xr)
    return a * x


def add(op, a, b):
    if op in UNS:
        return (a.view(UNS[op]) + b.view(UNS[op])).view(DT[op])
    if op in REAL:
        return K._cplx(op, a.real + b.real, a.imag + b.imag)
    return a + b


def entry_rows(csr):
    """the local row of every entry, in storage order"""
    if not len(csr["blocks"]):
        return np.zeros(0, dtype=np.int64)
    return np.concatenate([np.repeat(np.arange(csr["nrows"], dtype=np.int64), np.diff(o)) for o in csr["offs"]])


def ref_spmv(op, csr, x, x_first, W, gathered=None):
    """y of the contract; gathered: x[jdx - x_first] per entry in storage order, instead of x"""
    dt, nrows = DT[op], csr["nrows"]
    rows_all = entry_rows(csr)
    order = np.argsort(rows_all, kind="stable")   # by row, the blocks ascending within a row
    rows = rows_all[order]
    xs = gathered if gathered is not None else x[csr["jdx"].astype(np.int64) - x_first]
    prod = mul(op, csr["val"][order], xs[order])
    counts = np.bincount(rows, minlength=nrows)
    pos = np.arange(len(rows)) - (np.cumsum(counts) - counts)[rows]
    lane, step = pos % W, pos // W
    by_step = np.argsort(step, kind="stable")
    cut = np.searchsorted(step[by_step], np.arange(int(step.max()) + 2 if len(step) else 1))
    P = np.zeros((nrows, W), dtype=dt)
    for s in range(len(cut) - 1):
        m = by_step[cut[s]:cut[s + 1]]
        P[rows[m], lane[m]] = add(op, P[rows[m], lane[m]], prod[m])
    s = 1
    while s < W:
        P = add(op, P, P[:, np.arange(W) ^ s])
        s *= 2
    return np.ascontiguousarray(P[:, 0])


def ref_diag_get(csr, b, out):
    """out[r] = the last entry of row r in block b, in storage order, on the diagonal"""
    o, s = csr["offs"][b], int(csr["start"][b])
    for r in range(csr["nrows"]):
        for k in range(s + o[r], s + o[r + 1]):
            if csr["jdx"][k] == csr["ilo"] + r:
                out[r] = csr["val"][k]
    return out


def ref_diag_shift(op, csr, shift):
    """every stored (i, i) += shift, part by part"""
    on = csr["jdx"].astype(np.int64) == csr["ilo"] + entry_rows(csr)
    val = csr["val"].copy()
    val[on] = add(op, val[on], np.full(int(on.sum()), K.scalar(op, shift)[0], dtype=DT[op]))
    return val


# ---- data ----------------------------------------------------------------------------
def row_columns(rng, count, lo, hi, banned=()):
    """`count` distinct columns of [lo, hi) outside the banned (lo, hi) ranges"""
    ok = np.ones(hi - lo, dtype=bool)
    for a, b in banned:
        ok[max(a, lo) - lo:max(min(b, hi), lo) - lo] = False
    return lo + rng.choice(np.flatnonzero(ok), count, replace=False)


def mixed_matrix(op, W, ncut, rng, jdim=2000):
    """rows of 0, 1, W-1, W, W+1, 63, 64, 65 and 1000 entries, 3W+5 too; with 8 cuts the blocks 2 and 5
    stay empty; the last row's entries lie in the last block only; row 4 carries duplicates"""
    counts = [0, 1, max(W - 1, 0), W, W + 1, 63, 64, 65, 1000, 3 * W + 5, 0, 7]
    banned = [own_range(jdim, ncut, b) for b in (2, 5)] if ncut == 8 else []
    banned = [(a, b + 1) for a, b in banned]
    ii, jj = [], []
    for r, c in enumerate(counts):
        lo = own_range(jdim, ncut, ncut - 1)[0] if r == len(counts) - 1 else 0
        cols = row_columns(rng, c, lo, jdim, banned)
        ii += [r] * c
        jj += cols.tolist()
    dup = [k for k, r in enumerate(ii) if r == 4][:2]   # two (i, j) of row 4 once more, later in insertion order
    ii += [4] * len(dup) + [4] * len(dup)
    jj += [jj[k] for k in dup] * 2
    perm = rng.permutation(len(ii))
    i, j = np.array(ii)[perm], np.array(jj)[perm]
    return i, j, K.gen(op, len(i), rng), len(counts), jdim


def poison_untouched(op, x, touched):
    """NaN and -0.0 at the columns no entry names (floating point); integers: left as they are"""
    if op in UNS:
        return x
    free = np.setdiff1d(np.arange(len(x)), touched)
    x[free[0::2]] = np.nan
    x[free[1::2]] = -0.0
    return x


def bound_ok(op, csr, x, x_first, got):
    """|got - exact| <= (c + 2) * eps * sum |a||x| per row and part, exact in long double: any order of
    the c roundings of the sum, one or (complex) two roundings per product; eps = 2u leaves a factor of two"""
    if op in UNS:
        return True
    ld = np.longdouble
    rows, n = entry_rows(csr), csr["nrows"]
    xs = x[csr["jdx"].astype(np.int64) - x_first]
    a = csr["val"]
    eps = np.finfo(REAL.get(op, DT[op])).eps
    c = np.bincount(rows, minlength=n)
    if op in REAL:
        ar, ai, xr, xi = (t.astype(ld) for t in (a.real, a.imag, xs.real, xs.imag))
        terms = [(ar * xr, -(ai * xi), got.real.astype(ld)), (ar * xi, ai * xr, got.imag.astype(ld))]
    else:
        terms = [(a.astype(ld) * xs.astype(ld), np.zeros(len(a), ld), got.astype(ld))]
    for p, q, g in terms:
        exact, mag = np.zeros(n, ld), np.zeros(n, ld)
        np.add.at(exact, rows, p + q)
        np.add.at(mag, rows, np.abs(p) + np.abs(q))
        if not (np.abs(g - exact) <= (c + 2) * eps * mag).all():
            return False
    return True


# ---- device side ----------------------------------------------------------------------
class Held:
    """device copies of host arrays, freed together"""

    def __init__(self):
        self.bufs = []

    def up(self, a, lead=0, tail=0, fill=None):
        a = np.ascontiguousarray(a)
        img = np.zeros(lead + a.nbytes + tail, dtype=np.uint8) if fill is None else fill(lead + a.nbytes + tail)
        img[lead:lead + a.nbytes] = a.view(np.uint8).reshape(-1)
        b = ga_amd.DeviceBuffer(max(img.nbytes, 16))
        b.upload(img)
        self.bufs.append(b)
        return b, img

    def free(self):
        for b in self.bufs:
            b.free()


def csr_up(h, csr):
    """(offs, start, jdx, val) device addresses; 0 where the matrix has no block"""
    if not len(csr["blocks"]):
        return 0, 0, 0, 0
    return tuple(h.up(csr[k])[0].ptr for k in ("offs", "start", "jdx", "val"))


def spmv_dev(op, csr, x, x_first, W):
    """gaamd_spmv on uploaded copies; y lies between canary bytes, which must stay"""
    dt = DT[op]
    rng = np.random.default_rng(5)
    h = Held()
    try:
        offs, start, jdx, val = csr_up(h, csr)
        xb, _ = h.up(x)
        yb, yimg = h.up(np.zeros(csr["nrows"], dtype=dt), LEAD, LEAD, lambda n: rng.integers(1, 255, n).astype(np.uint8))
        rc = ga_amd.spmv(op, csr["nrows"], len(csr["blocks"]), offs, start, jdx, val, xb.ptr, x_first, yb.ptr + LEAD, W)
        assert rc == 0, rc
        ga_amd.sync()
        got = yb.download(np.uint8, yimg.nbytes)
        nb = csr["nrows"] * dt.itemsize
        assert got[:LEAD].tobytes() == yimg[:LEAD].tobytes() and got[LEAD + nb:].tobytes() == yimg[LEAD + nb:].tobytes(), "canary"
        return got[LEAD:LEAD + nb].view(dt).copy()
    finally:
        h.free()


# ---- gaamd_spmv ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W", TEAMS)
@pytest.mark.parametrize("op", OPS, **opid)
def test_spmv_bit_exact_every_team(gpu_lib, op, W):
    """rows of every length around the team width, 1, 2, 3 and 8 column blocks (empty ones among the 8), a
    row living in the last block only, duplicates, inexact random data, NaN / -0.0 at unused columns of x"""
    for ncut in (1, 2, 3, 8):
        rng = np.random.default_rng(100 * op + 10 * W + ncut)
        i, j, v, nrows, jdim = mixed_matrix(op, W, ncut, rng)
        csr = build_csr(i, j, v, 0, nrows, jdim, ncut, keep_empty=True)
        assert len(csr["blocks"]) == ncut and (ncut != 8 or csr["offs"][2, -1] == 0 == csr["offs"][5, -1])
        assert csr["offs"][:-1, nrows].sum() == csr["offs"][:-1, nrows - 1].sum() or ncut == 1   # the last row: last block only
        x = poison_untouched(op, K.gen(op, jdim, rng), j)
        got = spmv_dev(op, csr, x, 0, W)
        want = ref_spmv(op, csr, x, 0, W)
        assert got.tobytes() == want.tobytes(), (ga_amd.OP_NAME[op], W, ncut, np.flatnonzero(got != want)[:8])
        assert bound_ok(op, csr, x, 0, got)
        # the same list cut differently gives the same bits (duplicates share a column, hence a block)
        assert ref_spmv(op, build_csr(i, j, v, 0, nrows, jdim, 1), x, 0, W).tobytes() == want.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("op", [DBL, INT, CPL], **opid)
def test_spmv_many_short_rows(gpu_lib, op):
    """70 001 rows of at most 2 entries (more than 65 535 rows), teams 1, 2 and 64"""
    nrows, jdim = 70001, 5000
    rng = np.random.default_rng(7 + op)
    c = rng.integers(0, 3, nrows)
    i = np.repeat(np.arange(nrows), c)
    j = rng.integers(0, jdim, len(i))
    v = K.gen(op, len(i), rng)
    x = K.gen(op, jdim, rng)
    assert ga_amd.spmv_team(len(i), nrows) == 1
    for W, ncut in ((1, 1), (2, 3), (64, 2)):
        csr = build_csr(i, j, v, 0, nrows, jdim, ncut)
        got = spmv_dev(op, csr, x, 0, W)
        assert got.tobytes() == ref_spmv(op, csr, x, 0, W).tobytes(), (W, ncut)


@pytest.mark.gpu
@pytest.mark.parametrize("op", [FLT, DBL, DCP, LNG], **opid)
def test_spmv_non_square_and_offset_x(gpu_lib, op):
    """3001 x 2500 at about 40 000 entries with the library's team; then only the columns 700..1899 in use
    and x starting at column 700 (x_first)"""
    idim, jdim = 3001, 2500
    rng = np.random.default_rng(11 + op)
    flat = rng.choice(idim * jdim, 40000, replace=False)
    i, j = flat // jdim, flat % jdim
    v, x = K.gen(op, len(i), rng), K.gen(op, jdim, rng)
    W = ga_amd.spmv_team(len(i), idim)
    assert W == 8
    csr = build_csr(i, j, v, 0, idim, jdim, 3)
    got = spmv_dev(op, csr, x, 0, W)
    assert got.tobytes() == ref_spmv(op, csr, x, 0, W).tobytes()
    assert bound_ok(op, csr, x, 0, got)
    mid = (j >= 700) & (j < 1900)
    csr = build_csr(i[mid], j[mid], v[mid], 0, idim, jdim, 3)
    got = spmv_dev(op, csr, x[700:1900].copy(), 700, W)
    assert got.tobytes() == ref_spmv(op, csr, x, 0, W).tobytes()


@pytest.mark.gpu
def test_spmv_one_row_no_rows_no_blocks(gpu_lib):
    op = DBL
    rng = np.random.default_rng(3)
    j = np.array([5, 1, 9])
    csr = build_csr(np.zeros(3, dtype=int), j, K.gen(op, 3, rng), 0, 1, 10, 2)
    x = K.gen(op, 10, rng)
    for W in (1, 4, 64):
        assert spmv_dev(op, csr, x, 0, W).tobytes() == ref_spmv(op, csr, x, 0, W).tobytes()
    # no block: every row is +0, and x is not needed
    none = build_csr(np.zeros(0, dtype=int), np.zeros(0, dtype=int), K.gen(op, 0, rng), 0, 37, 10, 2)
    got = spmv_dev(op, none, x, 0, 8)
    assert got.tobytes() == np.zeros(37).tobytes()
    # no row: nothing is launched, nothing is read -- the addresses are not even device memory
    y = ga_amd.DeviceBuffer(64)
    y.upload(np.full(64, 0x5A, dtype=np.uint8))
    assert ga_amd.spmv(op, 0, 2, 8, 8, 8, 8, 8, 0, y.ptr, 8) == 0
    ga_amd.sync()
    assert (y.download(np.uint8, 64) == 0x5A).all()
    y.free()


@pytest.mark.gpu
def test_spmv_far_x_offsets(gpu_lib):
    """C_DCPL, columns whose byte offset into x lies beyond 2^32: x is allocated, only the gathered elements
    are written; about 100 entries; bit-exact"""
    op, dt = DCP, DT[DCP]
    far = (1 << 28) + 12345   # 16-byte elements: byte offset 2^32 + ...
    rng = np.random.default_rng(2)
    cols = np.concatenate([rng.choice(1000, 40, replace=False), far + rng.choice(5000, 60, replace=False)])
    jdim = far + 5000
    i = rng.integers(0, 9, len(cols))
    v, xs = K.gen(op, len(cols), rng), K.gen(op, len(cols), rng)
    csr = build_csr(i, cols, v, 0, 9, jdim, 2)
    xs_sorted = {int(c): xs[k] for k, c in enumerate(cols)}
    gathered = np.array([xs_sorted[int(c)] for c in csr["jdx"].astype(np.int64)], dtype=dt)
    assert int(csr["jdx"].max()) * 16 > 1 << 32
    xb = ga_amd.DeviceBuffer(jdim * 16)
    h = Held()
    try:
        for c, val in xs_sorted.items():
            xb.upload(np.array([val], dtype=dt), offset=c * 16)
        offs, start, jdx, val = csr_up(h, csr)
        yb, _ = h.up(np.zeros(9, dtype=dt))
        for W in (1, 16):
            assert ga_amd.spmv(op, 9, len(csr["blocks"]), offs, start, jdx, val, xb.ptr, 0, yb.ptr, W) == 0
            ga_amd.sync()
            got = yb.download(dt, 9)
            assert got.tobytes() == ref_spmv(op, csr, None, 0, W, gathered=gathered).tobytes(), W
    finally:
        h.free()
        xb.free()


# ---- gaamd_sprs_diag, gaamd_sprs_scale_left / _right ----------------------------------------
def diag_block(op, rng, nrows=300, first=100, jdim=600):
    """one column block of a row block starting at global row `first`: random entries, the diagonal in two
    rows of three, duplicated (three copies) in every seventh row"""
    ii, jj = [], []
    for r in range(nrows):
        cols = row_columns(rng, int(rng.integers(0, 9)), 0, jdim, [(first + r, first + r + 1)]).tolist()
        if r % 3:
            cols += [first + r] * (3 if r % 7 == 0 else 1)
        ii += [r + first] * len(cols)
        jj += cols
    perm = rng.permutation(len(ii))
    i, j = np.array(ii)[perm], np.array(jj)[perm]
    return build_csr(i, j, K.gen(op, len(i), rng), first, nrows, jdim, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [1, 8, 64])
@pytest.mark.parametrize("op", OPS, **opid)
def test_sprs_diag_get_and_shift(gpu_lib, op, W):
    dt = DT[op]
    rng = np.random.default_rng(50 * op + W)
    csr = diag_block(op, rng)
    n = csr["nrows"]
    h = Held()
    try:
        offs, start, jdx, val = csr_up(h, csr)
        before = K.gen(op, n, rng)
        ob, _ = h.up(before)
        assert ga_amd.sprs_diag(op, GET, n, offs, jdx, val, csr["ilo"], ob.ptr, W) == 0
        ga_amd.sync()
        want = ref_diag_get(csr, 0, before.copy())
        got = ob.download(dt, n)
        assert got.tobytes() == want.tobytes() and (want != before).any() and (want == before).any()
        assert ga_amd.sprs_diag(op, SHIFT, n, offs, jdx, val, csr["ilo"], 0, W, shift=SHIFT_C[op]) == 0
        ga_amd.sync()
        got = h.bufs[3].download(dt, len(csr["val"]))
        want = ref_diag_shift(op, csr, SHIFT_C[op])
        assert got.tobytes() == want.tobytes()
        on = csr["jdx"].astype(np.int64) == csr["ilo"] + entry_rows(csr)
        assert on.sum() > n // 2 and (got[~on].tobytes() == csr["val"][~on].tobytes())
        if op in REAL:   # part by part
            c = K.scalar(op, SHIFT_C[op])[0]
            assert (got[on].real == csr["val"][on].real + c.real).all() and (got[on].imag == csr["val"][on].imag + c.imag).all()
        if op in UNS:    # wraps
            assert (got[on].astype(object) != csr["val"][on].astype(object) + SHIFT_C[op]).any()
        # a row block whose diagonal block is empty: nothing is written
        zeros = h.up(np.zeros(6, dtype=np.int32))[0]
        ob.upload(before)
        assert ga_amd.sprs_diag(op, GET, 5, zeros.ptr, jdx, val, csr["ilo"], ob.ptr, W) == 0
        ga_amd.sync()
        assert ob.download(dt, n).tobytes() == before.tobytes()
    finally:
        h.free()


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, **opid)
def test_sprs_scale_left_and_right(gpu_lib, op):
    dt = DT[op]
    rng = np.random.default_rng(60 + op)
    csr = diag_block(op, rng)
    n, first, jdim = csr["nrows"], csr["ilo"], 600
    rows = entry_rows(csr)
    h = Held()
    try:
        offs, start, jdx, val = csr_up(h, csr)
        d_rows, d_cols = K.gen(op, n, rng), K.gen(op, jdim - 50, rng)   # the columns 50 .. jdim - 1 only
        db = h.up(d_rows)[0]
        for W in (1, 4, 64):
            h.bufs[3].upload(csr["val"])
            assert ga_amd.sprs_scale_left(op, n, offs, val, db.ptr, W) == 0
            ga_amd.sync()
            got = h.bufs[3].download(dt, len(rows))
            want = mul(op, d_rows[rows], csr["val"])
            assert got.tobytes() == want.tobytes(), W
        keep = csr["jdx"] >= 50
        sub = dict(jdx=csr["jdx"][keep], val=csr["val"][keep])
        jb, vb, cb = h.up(sub["jdx"])[0], h.up(sub["val"])[0], h.up(d_cols)[0]
        assert ga_amd.sprs_scale_right(op, int(keep.sum()), jb.ptr, vb.ptr, cb.ptr, 50) == 0
        ga_amd.sync()
        got = vb.download(dt, int(keep.sum()))
        want = mul(op, d_cols[sub["jdx"].astype(np.int64) - 50], sub["val"])
        assert got.tobytes() == want.tobytes()
        if op in REAL:   # the true complex product, each operation rounded on its own
            d, a = d_cols[sub["jdx"].astype(np.int64) - 50], sub["val"]
            assert (got.real == d.real * a.real - d.imag * a.imag).all()
            assert (got.imag == d.real * a.imag + d.imag * a.real).all()
        if op in UNS:
            wide = d_cols[sub["jdx"].astype(np.int64) - 50].astype(object) * sub["val"].astype(object)
            assert (got.astype(object) != wide).any()   # wrapped
    finally:
        h.free()


# ---- the matrices of the GA-level tests (tests/ga_sprs_worker.py) and of the host-side checks ------
def ga_matrix(name, size):
    """(idim, jdim, i, j, src): the elements in one global order and the rank that adds each (a rank adds
    its elements in that order).  No duplicates except in "dups"."""
    rng = np.random.default_rng({"rand": 1, "ladder": 2, "rank0": 3, "idle": 4, "tiny": 5, "gap": 6, "dups": 7}[name])
    if name in ("rand", "idle"):       # 3001 x 2500, about 40 000 entries
        idim, jdim = 3001, 2500
        flat = rng.choice(idim * jdim, 40000, replace=False)
        i, j = flat // jdim, flat % jdim
    elif name in ("ladder", "rank0"):  # 257 x 257: the diagonal, its neighbours and two rungs 16 away
        idim = jdim = 257
        r = np.arange(idim)
        i = np.concatenate([r, r[1:], r[:-1], r[16:], r[:-16]])
        j = np.concatenate([r, r[:-1], r[1:], r[:-16], r[16:]])
    elif name == "tiny":               # 2 x 5: on 3 ranks one owns no row, the column blocks hold 1 or 2 columns
        idim, jdim = 2, 5
        i, j = np.array([0, 0, 0, 1, 1, 1, 1]), np.array([4, 0, 2, 1, 3, 4, 0])
    elif name == "gap":                # 90 x 70 with no entry in the rows 30 .. 59: on 3 ranks rank 1's row block
        idim, jdim = 90, 70
        flat = rng.choice(idim * jdim, 900, replace=False)
        i, j = flat // jdim, flat % jdim
        keep = (i < 30) | (i >= 60)
        i, j = i[keep], j[keep]
    else:                              # dups: 64 x 64, every third element twice more, from other ranks too
        idim = jdim = 64
        flat = rng.choice(idim * jdim, 600, replace=False)
        i, j = flat // jdim, flat % jdim
        i, j = np.concatenate([i, i[::3], i[::3]]), np.concatenate([j, j[::3], j[::3]])
    perm = rng.permutation(len(i))
    i, j = i[perm], j[perm]
    src = rng.integers(0, size, len(i))
    if name == "rank0":
        src[:] = 0
    if name == "idle":                 # the last rank adds none
        src = rng.integers(0, max(size - 1, 1), len(i))
    return idim, jdim, i, j, src


GA_MATRICES = ("rand", "ladder", "rank0", "idle", "tiny", "gap", "dups")


def ga_values(op, name, i, j):
    """inexact random values; the diagonal made dominant for the floating-point types"""
    v = K.gen(op, len(i), np.random.default_rng(1000 + op + len(name)))
    if op not in UNS:
        v[i == j] += 8
    return v


def ga_parts(i, j, v, src, size):
    return [(i[src == r], j[src == r], v[src == r]) for r in range(size)]
