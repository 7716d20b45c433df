"""GPU, one rank, kernel level: gaamd_spmm, gaamd_dense_row_counts, gaamd_dense_to_csr and
gaamd_csr_to_dense against a numpy restatement of the contract in include/ga_amd.h, compared as raw
bits.  The restatement is the reference's sequential loop: every c[r][j] starts from +0 and takes,
entry by entry in the order of the row's one list, acc = acc + a * b[jdx][j] as two separately
rounded numpy operations (mul / add of tests/test_gpu_sprs.py: complex the true product part by
part, integers wrapping).  tests/test_spmm_abi.py checks on the CPU that the data used here tells
that sum from the fused and from the reversed one.
"""
import numpy as np
import pytest

import ga_amd
import test_gpu_sprs as S

K = S.K
INT, LNG, FLT, DBL, CPL, DCP = S.INT, S.LNG, S.FLT, S.DBL, S.CPL, S.DCP
OPS, DT, UNS, REAL = S.OPS, S.DT, S.UNS, S.REAL
opid = S.opid
WIDTHS = [1, 3, 17, 64, 65, 130]   # several rows per wave, no power of two, one wave, one past it, two column tiles
LEAD = 64


# ---- the contract restated ----------------------------------------------------------
def ref_spmm(op, csr, b, b_first, n, step=None, reverse=False, gathered=None):
    """c of the contract.  b: 2-D, row k is global row b_first + k (columns past n are ignored);
    gathered: the row of b per entry in storage order instead.  step(acc, a, brow) replaces the
    unfused acc + a * brow; reverse sums every row's list backwards."""
    nrows = csr["nrows"]
    rows_all = S.entry_rows(csr)
    order = np.argsort(rows_all, kind="stable")   # by row, the blocks ascending within a row
    rows = rows_all[order]
    counts = np.bincount(rows, minlength=nrows)
    pos = np.arange(len(rows)) - (np.cumsum(counts) - counts)[rows]
    if reverse:
        pos = counts[rows] - 1 - pos
    val = csr["val"][order]
    jj = csr["jdx"].astype(np.int64)[order] - b_first
    acc = np.zeros((nrows, n), dtype=DT[op])
    by = np.argsort(pos, kind="stable")
    cut = np.searchsorted(pos[by], np.arange(int(pos.max()) + 2 if len(pos) else 1))
    for s in range(len(cut) - 1):   # the s-th entry of every row that has one
        m = by[cut[s]:cut[s + 1]]
        brow = np.ascontiguousarray(b[jj[m], :n] if gathered is None else gathered[order[m], :n])
        a = np.repeat(val[m][:, None], n, axis=1)
        if step is not None:
            acc[rows[m]] = step(acc[rows[m]], a, brow)
        else:
            acc[rows[m]] = S.add(op, np.ascontiguousarray(acc[rows[m]]), S.mul(op, a, brow))
    return acc


def ref_keep(op, a, row_first, col_first):
    """the elements create_from_dense keeps: != 0 (not -0.0, but NaN; complex: either part) or on the diagonal"""
    r, c = np.indices(a.shape)
    return (a != 0) | (row_first + r == col_first + c)


def ref_dense_to_csr(op, a, row_first, col_first):
    keep = ref_keep(op, a, row_first, col_first)
    counts = keep.sum(axis=1).astype(np.int32)
    r, c = np.nonzero(keep)   # row-major: ascending columns within a row
    return counts, (col_first + c).astype(np.int32), np.ascontiguousarray(a[r, c])


# ---- data ----------------------------------------------------------------------------
def values(op, shape, rng):
    """inexact (seeded normal) floating-point data; integers over the whole range, so sums wrap"""
    if op in UNS:
        return K.gen(op, int(np.prod(shape)), rng).reshape(shape)
    if op in REAL:
        return K._cplx(op, rng.standard_normal(shape).astype(REAL[op]), rng.standard_normal(shape).astype(REAL[op]))
    return rng.standard_normal(shape).astype(DT[op])


def spmm_case(op, ncut, n, ldb, seed=0):
    """(csr, b, named): mixed_matrix's rows of 0, 1, 2, 7, 8, 63, 64, 65 and 1000 entries with duplicates in row
    4, the last row in the last block only; b is jdim x ldb with the rows no entry names, and the columns
    past n, poisoned (NaN / -0.0) for the floating-point types"""
    rng = np.random.default_rng(1000 * seed + 100 * op + 10 * ncut + n)
    i, j, _, nrows, jdim = S.mixed_matrix(op, 1, ncut, rng)
    csr = S.build_csr(i, j, values(op, len(i), rng), 0, nrows, jdim, ncut)
    b = values(op, (jdim, ldb), rng)
    named = np.unique(j)
    if op not in UNS:
        free = np.setdiff1d(np.arange(jdim), named)
        b[free[0::2]] = np.nan
        b[free[1::2]] = -0.0
        b[:, n:] = np.nan
    return csr, b, named


def c_fill(op):
    """what an unwritten byte of C looks like: NaN patterns, 0x5a for integers"""
    return 0x5A if op in UNS else 0xFF


def spmm_dev(op, csr, b, b_first, n, ldc, lead, nrows=None):
    """gaamd_spmm on uploaded copies; returns (c, intact): c the nrows x n result, intact whether every byte
    of C's buffer outside it -- lead, the gaps ldc - n, the tail -- is unchanged"""
    dt, esz = DT[op], DT[op].itemsize
    nrows = csr["nrows"] if nrows is None else nrows
    h = S.Held()
    try:
        offs, start, jdx, val = S.csr_up(h, csr)
        bb, _ = h.up(b, lead)
        cb, cimg = h.up(np.zeros(0, dtype=dt), 0, lead + nrows * ldc * esz + LEAD,
                        lambda k: np.full(k, c_fill(op), dtype=np.uint8))
        rc = ga_amd.spmm(op, nrows, len(csr["blocks"]), offs, start, jdx, val, bb.ptr + lead, b.shape[1], b_first, n,
                         cb.ptr + lead, ldc)
        assert rc == 0, rc
        ga_amd.sync()
        got = cb.download(np.uint8, cimg.nbytes)
        body = got[lead:lead + nrows * ldc * esz].view(dt).reshape(nrows, ldc)
        c = np.ascontiguousarray(body[:, :n])
        back = body.copy()
        back[:, :n] = cimg[lead:lead + nrows * ldc * esz].view(dt).reshape(nrows, ldc)[:, :n]
        rest = got.copy()
        rest[lead:lead + nrows * ldc * esz] = back.view(np.uint8).reshape(-1)
        return c, rest.tobytes() == cimg.tobytes()
    finally:
        h.free()


# ---- gaamd_spmm ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("op", OPS, **opid)
def test_spmm_bit_exact(gpu_lib, op, n):
    """1 and 3 column blocks; ld = n on 16-byte-aligned bases (the 16-byte path where n allows it) and
    ldb = n + 3, ldc = n + 5 on bases one element past alignment (one element per lane), C's gaps canaries"""
    esz = DT[op].itemsize
    for ncut in (1, 3):
        for ldb, ldc, lead in ((n, n, LEAD), (n + 3, n + 5, LEAD + esz)):
            csr, b, _ = spmm_case(op, ncut, n, ldb)
            assert len(csr["blocks"]) == ncut
            assert ncut == 1 or csr["offs"][:-1, -1].sum() == csr["offs"][:-1, -2].sum()   # blocks empty for the last row
            want = ref_spmm(op, csr, b, 0, n)
            got, intact = spmm_dev(op, csr, b, 0, n, ldc, lead)
            assert got.tobytes() == want.tobytes(), (ga_amd.OP_NAME[op], n, ncut, ldb, np.argwhere(got != want)[:4])
            assert intact, "bytes of C's buffer outside the nrows x n elements changed"
            if op not in UNS:
                assert not np.isnan(got.view(REAL.get(op, DT[op]))).any()   # no poisoned row of B was read
            # the same list cut differently gives the same bits
            one = S.build_csr(*csr_elements(csr), 0, csr["nrows"], b.shape[0], 1)
            assert ref_spmm(op, one, b, 0, n).tobytes() == want.tobytes()


def csr_elements(csr):
    """(i, j, v) in storage order"""
    return S.entry_rows(csr), csr["jdx"].astype(np.int64), csr["val"]


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, **opid)
def test_spmm_n1_is_spmv_team_1(gpu_lib, op):
    for ncut in (1, 3):
        csr, b, _ = spmm_case(op, ncut, 1, 1)
        got, intact = spmm_dev(op, csr, b, 0, 1, 1, LEAD)
        y = S.spmv_dev(op, csr, np.ascontiguousarray(b[:, 0]), 0, 1)
        assert intact and got[:, 0].tobytes() == y.tobytes()


@pytest.mark.gpu
def test_spmm_offset_b_one_row_and_nothing_to_do(gpu_lib):
    op, n = DBL, 5
    rng = np.random.default_rng(3)
    # b starts at global row 700: only the columns 700 .. 1899 are in use
    i, j, _, nrows, jdim = S.mixed_matrix(op, 1, 3, rng)
    mid = (j >= 700) & (j < 1900)
    csr = S.build_csr(i[mid], j[mid], values(op, int(mid.sum()), rng), 0, nrows, jdim, 3)
    b = values(op, (jdim, n), rng)
    got, intact = spmm_dev(op, csr, np.ascontiguousarray(b[700:1900]), 700, n, n, LEAD)
    assert intact and got.tobytes() == ref_spmm(op, csr, b, 0, n).tobytes()
    # one row
    one = S.build_csr(np.zeros(3, dtype=int), np.array([5, 1, 9]), values(op, 3, rng), 0, 1, 10, 2)
    b = values(op, (10, 7), rng)
    for n1 in (1, 4, 7):
        got, intact = spmm_dev(op, one, b, 0, n1, 7, LEAD)
        assert intact and got.tobytes() == ref_spmm(op, one, b, 0, n1).tobytes()
    # no block: every element of C becomes +0, and b is not needed
    none = S.build_csr(np.zeros(0, dtype=int), np.zeros(0, dtype=int), values(op, 0, rng), 0, 37, 10, 2)
    got, intact = spmm_dev(op, none, b, 0, 6, 9, LEAD + 8)
    assert intact and got.tobytes() == np.zeros((37, 6)).tobytes()
    # no row, no column: nothing is launched, nothing is read -- the addresses are not even device memory
    c = ga_amd.DeviceBuffer(64)
    c.upload(np.full(64, 0x5A, dtype=np.uint8))
    assert ga_amd.spmm(op, 0, 2, 8, 8, 8, 8, 8, 4, 0, 4, c.ptr, 4) == 0
    assert ga_amd.spmm(op, 3, 2, 8, 8, 8, 8, 8, 4, 0, 0, c.ptr, 4) == 0
    ga_amd.sync()
    assert (c.download(np.uint8, 64) == 0x5A).all()
    c.free()


@pytest.mark.gpu
def test_spmm_far_offsets(gpu_lib):
    """f64.  (1) ldb = 8192 and entries naming rows of B near 70 000 from b_first: element offsets beyond 2^29,
    byte offsets beyond 2^32; B is allocated, only the named rows and NaN rows around them are written.
    (2) ldc beyond 2^26, so C's last row lies beyond 2^32 bytes from its base; C is allocated, and only
    canaries around every row's n elements are written and checked."""
    op, dt, n = DBL, DT[DBL], 6
    rng = np.random.default_rng(2)
    far, ldb = 70000, 8192
    cols = np.concatenate([rng.choice(1000, 40, replace=False), far + 2 * rng.choice(2000, 60, replace=False)])
    i = rng.integers(0, 9, len(cols))
    csr = S.build_csr(i, cols, values(op, len(cols), rng), 0, 9, far + 4001, 2)
    brows = {int(c): values(op, n, rng) for c in cols}
    gathered = np.stack([brows[int(c)] for c in csr["jdx"]])
    want = ref_spmm(op, csr, None, 0, n, gathered=gathered)
    assert int(csr["jdx"].max()) * ldb > 1 << 29 and int(csr["jdx"].max()) * ldb * 8 > 1 << 32
    bb = ga_amd.DeviceBuffer((far + 4001) * ldb * 8)
    h = S.Held()
    try:
        nan_row = np.full(n, np.nan)
        for c in brows:   # the neighbours first: a named row may be a neighbour of another
            for nb in (c - 1, c + 1):
                if nb >= 0 and nb not in brows:
                    bb.upload(nan_row, offset=nb * ldb * 8)
        for c, row in brows.items():
            bb.upload(row, offset=c * ldb * 8)
            bb.upload(nan_row[:2], offset=(c * ldb + n) * 8)   # the columns past n
        offs, start, jdx, val = S.csr_up(h, csr)
        cb, _ = h.up(np.full(9 * n, np.nan))
        assert ga_amd.spmm(op, 9, len(csr["blocks"]), offs, start, jdx, val, bb.ptr, ldb, 0, n, cb.ptr, n) == 0
        ga_amd.sync()
        got = cb.download(dt, 9 * n).reshape(9, n)
        assert got.tobytes() == want.tobytes()
        # (2) the same product into a C whose rows are 2^26 + 8 elements apart
        ldc = (1 << 26) + 8
        assert 8 * ldc * 8 > 1 << 32
        big = ga_amd.DeviceBuffer((8 * ldc + n + 2) * 8 + 16)
        try:
            canary = np.array([0x5A5A5A5A5A5A5A5A], dtype=np.uint64)
            for r in range(9):
                big.upload(canary, offset=16 + (r * ldc - 1) * 8)
                big.upload(canary, offset=16 + (r * ldc + n) * 8)
            assert ga_amd.spmm(op, 9, len(csr["blocks"]), offs, start, jdx, val, bb.ptr, ldb, 0, n, big.ptr + 16, ldc) == 0
            ga_amd.sync()
            for r in range(9):
                row = big.download(np.uint64, n + 2, offset=16 + (r * ldc - 1) * 8)
                assert row[0] == canary[0] == row[-1], r
                assert row[1:-1].tobytes() == want[r].tobytes(), r
        finally:
            big.free()
    finally:
        h.free()
        bb.free()


# ---- gaamd_dense_row_counts, gaamd_dense_to_csr ---------------------------------------------
SHAPES = [(1, 1), (1, 200), (67, 129), (300, 5)]


def dense_block(op, rows, cols, density, rng):
    """density 0: all zero; 1: every element non-zero; else about 1 in 16; with -0.0, NaN and an element whose
    imaginary part alone is set planted where the block has room (floating point)"""
    a = values(op, (rows, cols), rng)
    if op in UNS:
        a[a == 0] = 1
    if density == 0:
        a[:] = 0
    elif density < 1:
        a[rng.random((rows, cols)) >= density] = 0
    if op not in UNS and rows * cols >= 200:
        flat = a.reshape(-1)
        flat[3] = -0.0
        flat[70] = np.nan
        if op in REAL:
            flat[5] = complex(-0.0, -0.0)
            flat[130] = complex(0.0, 1.5)
            flat[131] = complex(np.nan, 0.0)
    return a


def dense_to_csr_dev(op, a, lda, row_first, col_first):
    """(counts, jdx, val) of the two kernels; canaries after counts, jdx and val must stay"""
    dt, esz = DT[op], DT[op].itemsize
    rows, cols = a.shape
    rng = np.random.default_rng(9)
    junk = lambda k: rng.integers(1, 255, k).astype(np.uint8)   # noqa: E731
    h = S.Held()
    try:
        img = np.zeros((rows, lda), dtype=dt)
        img[:, :cols] = a
        if op not in UNS:
            img[:, cols:] = np.nan   # the gap lda - cols is not part of the block
        else:
            img[:, cols:] = 7
        ab, _ = h.up(img)
        cb, cimg = h.up(np.zeros(rows, dtype=np.int32), 0, LEAD, junk)
        assert ga_amd.dense_row_counts(op, rows, cols, ab.ptr, lda, row_first, col_first, cb.ptr) == 0
        ga_amd.sync()
        got = cb.download(np.uint8, cimg.nbytes)
        assert got[rows * 4:].tobytes() == cimg[rows * 4:].tobytes(), "canary after counts"
        counts = got[:rows * 4].view(np.int32).copy()
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        nnz = int(offs[-1])
        ob, _ = h.up(offs)
        jb, jimg = h.up(np.zeros(nnz, dtype=np.int32), 0, LEAD, junk)
        vb, vimg = h.up(np.zeros(nnz, dtype=dt), 0, LEAD, junk)
        assert ga_amd.dense_to_csr(op, rows, cols, ab.ptr, lda, row_first, col_first, ob.ptr, jb.ptr, vb.ptr) == 0
        ga_amd.sync()
        gj, gv = jb.download(np.uint8, jimg.nbytes), vb.download(np.uint8, vimg.nbytes)
        assert gj[nnz * 4:].tobytes() == jimg[nnz * 4:].tobytes(), "canary after jdx"
        assert gv[nnz * esz:].tobytes() == vimg[nnz * esz:].tobytes(), "canary after val"
        assert ab.download(np.uint8, img.nbytes).tobytes() == img.tobytes(), "the block changed"
        return counts, gj[:nnz * 4].view(np.int32).copy(), gv[:nnz * esz].view(dt).copy()
    finally:
        h.free()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("op", OPS, **opid)
def test_dense_to_csr(gpu_lib, op, shape):
    """the diagonal inside the block, outside it, and crossing its top right corner; densities 0, 1/16 and 1"""
    rows, cols = shape
    places = {"inside": (5, 5), "outside": (0, 10000), "corner": (1000 + max(cols - 2, 0), 1000)}
    for where, (row_first, col_first) in places.items():
        for density in (0, 1.0 / 16, 1):
            rng = np.random.default_rng(17 * op + rows + int(16 * density))
            a = dense_block(op, rows, cols, density, rng)
            wc, wj, wv = ref_dense_to_csr(op, a, row_first, col_first)
            on = int((row_first + np.arange(rows)[:, None] == col_first + np.arange(cols)[None, :]).sum())
            assert (on > 0) == (where != "outside") and (where != "corner" or on == min(rows, 2, cols))
            if density == 0:
                assert on <= wc.sum() <= on + 3   # the zeros of the diagonal are kept; else only the planted NaNs / imaginary part
            counts, jdx, val = dense_to_csr_dev(op, a, cols + 3, row_first, col_first)
            key = (ga_amd.OP_NAME[op], shape, where, density)
            assert counts.tobytes() == wc.tobytes(), key
            assert jdx.tobytes() == wj.tobytes(), key
            assert val.tobytes() == wv.tobytes(), key


# ---- gaamd_csr_to_dense ---------------------------------------------------------------
def csr_to_dense_dev(op, nrows, cols, offs, jdx, val, col_first, ldo):
    """one column block scattered into zeros; the gap ldo - cols holds 0x5a bytes, which must stay"""
    dt = DT[op]
    h = S.Held()
    try:
        img = np.zeros((nrows, ldo), dtype=dt)
        img.view(np.uint8).reshape(nrows, -1)[:, cols * dt.itemsize:] = 0x5A
        ob, _ = h.up(img)
        bufs = [h.up(x if len(x) else np.zeros(1, dtype=x.dtype))[0] for x in (offs, jdx, val)]
        assert ga_amd.csr_to_dense(op, nrows, cols, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, col_first, ob.ptr, ldo) == 0
        ga_amd.sync()
        got = ob.download(dt, nrows * ldo).reshape(nrows, ldo)
        assert got[:, cols:].tobytes() == img[:, cols:].tobytes(), "the gap changed"
        return np.ascontiguousarray(got[:, :cols])
    finally:
        h.free()


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, **opid)
def test_csr_to_dense(gpu_lib, op):
    """every column block of mixed_matrix (row 4 carries duplicates, of which the last wins; the blocks
    1 and 2 do not start at column 0), ldo above the width"""
    rng = np.random.default_rng(40 + op)
    i, j, _, nrows, jdim = S.mixed_matrix(op, 1, 3, rng)
    csr = S.build_csr(i, j, values(op, len(i), rng), 0, nrows, jdim, 3)
    dups = 0
    for b in range(3):
        lo, hi = S.own_range(jdim, 3, b)
        o, s = csr["offs"][b], int(csr["start"][b])
        jdx, val = csr["jdx"][s:s + o[-1]], csr["val"][s:s + o[-1]]
        want = np.zeros((nrows, hi - lo + 1), dtype=DT[op])
        for r in range(nrows):   # the reference's sequential copy
            for k in range(o[r], o[r + 1]):
                want[r, jdx[k] - lo] = val[k]
            dups += (o[r + 1] - o[r]) - len(set(jdx[o[r]:o[r + 1]].tolist()))
        got = csr_to_dense_dev(op, nrows, hi - lo + 1, o, jdx, val, lo, hi - lo + 4)
        assert got.tobytes() == want.tobytes(), (ga_amd.OP_NAME[op], b)
    assert dups == 4


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, **opid)
def test_csr_dense_round_trip(gpu_lib, op):
    """a duplicate-free, zero-free matrix: dense -> CSR of csr -> dense gives its jdx / val back"""
    idim, jdim, first = 130, 77, 40
    rng = np.random.default_rng(50 + op)
    flat = rng.choice(idim * jdim, 900, replace=False)
    v = values(op, 900, rng)
    v[v == 0] = 1
    csr = S.build_csr(flat // jdim, first + flat % jdim, v, 0, idim, 3 * (first + jdim), 1)
    dense = csr_to_dense_dev(op, idim, jdim, csr["offs"][0], csr["jdx"], csr["val"], first, jdim + 2)
    counts, jdx, val = dense_to_csr_dev(op, dense, jdim, 10 ** 6, first)   # the diagonal far outside
    assert counts.tobytes() == np.diff(csr["offs"][0]).astype(np.int32).tobytes()
    assert jdx.tobytes() == csr["jdx"].tobytes() and val.tobytes() == csr["val"].tobytes()
