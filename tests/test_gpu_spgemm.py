"""GPU, one rank, kernel level: gaamd_csr_rows, gaamd_spgemm_count and gaamd_spgemm_fill against a numpy
restatement of the contract in include/ga_amd.h, compared as raw bits.  The restatement is sequential per
(i, j): c_ij starts from +0 and takes acc = acc + a * b as two separately rounded numpy operations (mul /
add of tests/test_gpu_sprs.py) for A's row-i list in order and, per A entry with column k, B's row-k list
in order restricted to column j.  An entry exists where a pair (a_ik, b_kj) is stored, whatever the
values.  The expected layout is build_csr(keep_empty=True) of the restatement's triples.
tests/test_spgemm_abi.py checks on the CPU that the data used here tells that sum from the fused, the
reversed and the assign-first one.
"""
import numpy as np
import pytest

import ga_amd
import test_gpu_spmm as M
import test_gpu_sprs as S

K = S.K
INT, LNG, FLT, DBL, CPL, DCP = S.INT, S.LNG, S.FLT, S.DBL, S.CPL, S.DCP
OPS, DT, UNS, REAL = S.OPS, S.DT, S.UNS, S.REAL
opid = S.opid
LEAD = 64
CAP = 1024          # gaamd_spgemm_lds_cap(), asserted on the device and in test_spgemm_abi.py
JDIM_C = 5000       # columns of B and C
BROWS = 120         # rows of B = columns of A
B_FIRST = 1         # the row CSR handed to the kernels starts at B's global row 1: A never names row 0
NCUTS = [1, 3, 8]


# ---- the contract restated ----------------------------------------------------------
def ref_rows(csr):
    """the row CSR of a block CSR: (roffs int64, rjdx, rval), every row's one list contiguous, the blocks ascending"""
    rows = S.entry_rows(csr)
    order = np.argsort(rows, kind="stable")
    roffs = np.zeros(csr["nrows"] + 1, dtype=np.int64)
    roffs[1:] = np.cumsum(np.bincount(rows, minlength=csr["nrows"]))
    return roffs, np.ascontiguousarray(csr["jdx"][order]), np.ascontiguousarray(csr["val"][order])


def ref_spgemm(op, csr, rows_b, b_first, step=None, reverse=False):
    """(i, j, v, U) of C = A B: the triples by row, ascending column within a row, and the product bound per row.
    step(acc, a, b, s) replaces the unfused acc + a * b for the s-th product of an entry; reverse sums backwards."""
    roffs, rjdx, rval = rows_b
    rows_all = S.entry_rows(csr)
    order = np.argsort(rows_all, kind="stable")   # by row, the blocks ascending within a row
    rows = rows_all[order]
    ii, jj, vv, U = [], [], [], np.zeros(csr["nrows"], dtype=np.int64)
    for r in range(csr["nrows"]):
        a_idx, b_idx = [], []
        for k in order[rows == r]:                # A's row list in order
            kb = int(csr["jdx"][k]) - b_first
            span = np.arange(roffs[kb], roffs[kb + 1])   # B's row list in order
            a_idx.append(np.full(len(span), k, dtype=np.int64))
            b_idx.append(span)
        if not a_idx:
            continue
        a_idx, b_idx = np.concatenate(a_idx), np.concatenate(b_idx)
        U[r] = len(b_idx)
        if not len(b_idx):
            continue
        if reverse:
            a_idx, b_idx = a_idx[::-1], b_idx[::-1]
        uniq, inv = np.unique(rjdx[b_idx], return_inverse=True)
        by = np.argsort(inv, kind="stable")
        cnt = np.bincount(inv)
        occ = np.empty(len(inv), dtype=np.int64)   # a product's number among those of its column, in order
        occ[by] = np.arange(len(inv)) - (np.cumsum(cnt) - cnt)[inv[by]]
        a, b = csr["val"][a_idx], rval[b_idx]
        acc = np.zeros(len(uniq), dtype=DT[op])
        for s in range(int(occ.max()) + 1):
            m = np.flatnonzero(occ == s)
            am, bm, cur = np.ascontiguousarray(a[m]), np.ascontiguousarray(b[m]), np.ascontiguousarray(acc[inv[m]])
            acc[inv[m]] = step(cur, am, bm, s) if step is not None else S.add(op, cur, S.mul(op, am, bm))
        ii.append(np.full(len(uniq), r, dtype=np.int64))
        jj.append(uniq.astype(np.int64))
        vv.append(acc)
    if not ii:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=DT[op]), U
    return np.concatenate(ii), np.concatenate(jj), np.concatenate(vv), U


# ---- data ----------------------------------------------------------------------------
def allowed_columns():
    """the columns outside the blocks 2 and 5 of 8: those blocks of C stay empty"""
    ok = np.ones(JDIM_C, dtype=bool)
    for b in (2, 5):
        lo, hi = S.own_range(JDIM_C, 8, b)
        ok[lo:hi + 1] = False
    return np.flatnonzero(ok)


def b_matrix(op, rng):
    """B, BROWS x JDIM_C, as (k, j, v) in insertion order.  Rows: 0 never named; 1, 2, 3 empty; 10 of CAP - 1 entries,
    11 and 12 of one; 13, 14, 15 of CAP - 1 each on disjoint columns; 16 one column in every non-empty block of 3
    and of 8 cuts; 17 in the last block of 8 only; 18 of 72 entries with one column at the sorted positions 63 and
    64 (and one three times at 5, 6, 7), a NaN among its values; 20 .. 84 the same three columns each; 90, 91, 92
    the one column 7 with the value 1; the others a few random columns"""
    ok = allowed_columns()
    perm = ok[rng.permutation(len(ok))]
    kk, jj = [], []

    def row(k, cols):
        kk.extend([k] * len(cols))
        jj.extend(int(c) for c in cols)

    row(10, perm[:CAP - 1])
    row(11, [perm[CAP - 1]])
    row(12, [perm[CAP]])
    for q, k in enumerate((13, 14, 15)):
        row(k, perm[q * (CAP - 1):(q + 1) * (CAP - 1)])
    row(16, [S.own_range(JDIM_C, 8, b)[0] + 3 for b in (0, 1, 3, 4, 6, 7)])   # they hit the 3 blocks of 3 cuts too
    last = S.own_range(JDIM_C, 8, 7)
    row(17, rng.choice(np.arange(last[0], last[1] + 1), 9, replace=False))
    c18 = np.sort(rng.choice(ok, 69, replace=False))
    row(18, list(c18) + [c18[61], c18[5], c18[5]])   # sorted: 5, 6, 7 one column, which moves c18[61] to 63 and 64
    for k in range(20, 85):
        row(k, [40, 41, 3000])
    for k in (90, 91, 92):
        row(k, [7])
    for k in list(range(4, 10)) + list(range(93, BROWS)):
        row(k, rng.choice(ok, 5, replace=False))
    k, j = np.array(kk), np.array(jj)
    v = M.values(op, len(k), rng)
    if op in UNS:
        v[v == 0] = 1
    one = K.scalar(op, 1)[0]
    v[np.isin(k, (11, 90, 91, 92))] = one
    if op not in UNS:
        v[np.flatnonzero(k == 18)[10]] = np.nan
    return k, j, v


def a_matrix(op, rng):
    """A, 13 x BROWS, as (i, k, v, rows) in insertion order: rows without entries (0, 10), naming only empty rows of
    B (1), of one product with the value -0.0 (2), 65 entries onto three columns (3), duplicates (4), U = CAP - 1, CAP,
    CAP + 1 and 3 (CAP - 1) (5 .. 8), over every cut (9), x, -x and 0 onto one column (11), the last block only (12)"""
    rows = {0: [], 1: [1, 2], 2: [11], 3: list(range(20, 85)), 4: [18, 5, 6, 18, 5], 5: [10], 6: [10, 11], 7: [10, 11, 12],
            8: [13, 14, 15], 9: [16, 3], 10: [], 11: [90, 91, 92], 12: [17]}
    ii, kk = [], []
    for r, ks in rows.items():
        ii += [r] * len(ks)
        kk += ks
    i, k = np.array(ii), np.array(kk)
    v = M.values(op, len(i), rng)
    if op in UNS:
        v[v == 0] = 1
    r11 = np.flatnonzero(i == 11)
    x = v[r11[:1]]
    v[r11[1]] = (np.negative(x.view(UNS[op])).view(DT[op]) if op in UNS else -x)[0]   # x * 1 + (-x) * 1 cancels
    v[r11[2]] = 0                                                                      # 0 * 1: the entry is kept
    if op not in UNS:
        v[np.flatnonzero(i == 2)[0]] = -0.0                                         # a lone -0.0 product
    perm = rng.permutation(len(i))   # row 4's duplicates stay apart in insertion order
    return i[perm], k[perm], v[perm], len(rows)


_cases = {}


def spgemm_case(op):
    """A's block CSR on 3 cuts, B's row CSR from global row B_FIRST (built on 2 cuts), and the restatement's
    (i, j, v, U); computed once per type and shared"""
    if op not in _cases:
        rng = np.random.default_rng(190 + op)
        bk, bj, bv = b_matrix(op, rng)
        ai, ak, av, nrows = a_matrix(op, rng)
        csr_b = S.build_csr(bk, bj, bv, 0, BROWS, JDIM_C, 2)
        roffs, rjdx, rval = ref_rows(csr_b)
        rows_b = (np.ascontiguousarray(roffs[B_FIRST:] - roffs[B_FIRST]), rjdx[roffs[B_FIRST]:], rval[roffs[B_FIRST]:])
        csr_a = S.build_csr(ai, ak, av, 0, nrows, BROWS, 3)
        _cases[op] = (csr_a, rows_b, ref_spgemm(op, csr_a, rows_b, B_FIRST))
    return _cases[op]


def layout(op, case, ncut):
    """the block CSR of C with every one of the ncut blocks kept"""
    csr_a, _, (i, j, v, _) = case
    return S.build_csr(i, j, v, 0, csr_a["nrows"], JDIM_C, ncut, keep_empty=True)


def test_case_has_the_rows_the_kernels_branch_on():
    csr_a, rows_b, (i, j, v, U) = spgemm_case(FLT)
    roffs, rjdx, rval = rows_b
    assert U.tolist()[:3] == [0, 0, 1] and U[3] == 195 and U[10] == 0
    assert U[5:9].tolist() == [CAP - 1, CAP, CAP + 1, 3 * (CAP - 1)]
    assert np.bincount(i, minlength=13)[[0, 1, 2, 3, 8, 10, 11]].tolist() == [0, 0, 1, 3, 3 * (CAP - 1), 0, 1]
    r18 = rjdx[roffs[18 - B_FIRST]:roffs[19 - B_FIRST]]
    assert len(r18) == 72 and r18[63] == r18[64] and r18[5] == r18[6] == r18[7] and r18[62] < r18[63] < r18[65]
    assert (np.diff(r18) >= 0).all()
    c8 = layout(FLT, spgemm_case(FLT), 8)
    per_block = np.diff(c8["offs"], axis=1).sum(axis=1)
    assert per_block[2] == per_block[5] == 0 and (per_block[[0, 1, 3, 4, 6, 7]] > 0).all()
    assert np.diff(c8["offs"], axis=1)[:7, 12].sum() == 0 and np.diff(c8["offs"], axis=1)[7, 12] == 9
    for ncut in (3, 8):   # row 9 has an entry in every non-empty block
        cb = layout(FLT, spgemm_case(FLT), ncut)
        assert (np.diff(cb["offs"], axis=1)[:, 9] > 0).tolist() == [b not in (2, 5) or ncut == 3 for b in range(ncut)]
    row11 = v[i == 11]
    assert len(row11) == 1 and row11[0] == 0 and not np.signbit(row11[0])     # x - x and 0 * 1: kept, +0
    assert v[i == 2][0] == 0 and not np.signbit(v[i == 2][0])                  # +0 + (-0.0) = +0
    assert np.isnan(v[i == 4]).any()


# ---- device side ----------------------------------------------------------------------
def canary(n):
    return np.random.default_rng(11).integers(1, 255, n).astype(np.uint8)


def out_buf(h, nbytes):
    return h.up(np.zeros(0, dtype=np.uint8), 0, LEAD + nbytes + LEAD, canary)


def body(buf, img, nbytes):
    """the nbytes after the lead; asserts the bytes around them are the canaries still"""
    got = buf.download(np.uint8, img.nbytes)
    assert got[:LEAD].tobytes() == img[:LEAD].tobytes() and got[LEAD + nbytes:].tobytes() == img[LEAD + nbytes:].tobytes(), "canary"
    return got[LEAD:LEAD + nbytes].copy()


def spgemm_dev(op, csr_a, rows_b, b_first, jdim_c, ncut):
    """(counts [ncut][nrows], U, cjdx, cval) of the two kernels; the offsets between them are the prefix sums of the
    device's counts, as the GA layer forms them"""
    dt, nrows = DT[op], csr_a["nrows"]
    roffs, rjdx, rval = rows_b
    h = S.Held()
    try:
        offs, start, jdx, val = S.csr_up(h, csr_a)
        ro, rj, rv = (h.up(x)[0].ptr for x in (roffs, rjdx, rval))
        cb, cimg = out_buf(h, ncut * nrows * 4)
        ub, uimg = out_buf(h, nrows * 8)
        nblk, brows = len(csr_a["blocks"]), len(roffs) - 1
        rc = ga_amd.spgemm_count(nrows, nblk, offs, start, jdx, b_first, brows, ro, rj, jdim_c, ncut, cb.ptr + LEAD, ub.ptr + LEAD)
        assert rc == 0, rc
        ga_amd.sync()
        counts = body(cb, cimg, ncut * nrows * 4).view(np.int32).reshape(ncut, nrows)
        U = body(ub, uimg, nrows * 8).view(np.int64)
        coffs = np.zeros((ncut, nrows + 1), dtype=np.int32)
        coffs[:, 1:] = np.cumsum(counts, axis=1)
        cstart = np.concatenate([[0], np.cumsum(coffs[:, -1])[:-1]]).astype(np.int64)
        nnz = int(coffs[:, -1].sum())
        co, cs = h.up(coffs)[0].ptr, h.up(cstart)[0].ptr
        jb, jimg = out_buf(h, nnz * 4)
        vb, vimg = out_buf(h, nnz * dt.itemsize)
        rc = ga_amd.spgemm_fill(op, nrows, nblk, offs, start, jdx, val, b_first, brows, ro, rj, rv, jdim_c, ncut, co, cs,
                                jb.ptr + LEAD, vb.ptr + LEAD)
        assert rc == 0, rc
        ga_amd.sync()
        return counts, U, body(jb, jimg, nnz * 4).view(np.int32), body(vb, vimg, nnz * dt.itemsize).view(dt)
    finally:
        h.free()


@pytest.mark.gpu
@pytest.mark.parametrize("ncut", NCUTS)
@pytest.mark.parametrize("op", OPS, **opid)
def test_spgemm_bit_exact(gpu_lib, op, ncut):
    """rows without entries, naming only empty rows of B, of one product, 65 entries onto three columns, duplicates in
    A's row 4 and in B's row 18 across a 64-lane chunk, U = cap - 1, cap, cap + 1 and 3 (cap - 1) (the last two take
    the fallback), a cancelling pair and a 0 * y product kept, a NaN, a lone -0.0 product, a row over every cut, the
    last row in the last block, blocks 2 and 5 of 8 empty, b_first = 1; canaries around every output"""
    assert ga_amd.spgemm_lds_cap() == CAP
    case = spgemm_case(op)
    csr_a, rows_b, (_, _, _, U) = case
    want = layout(op, case, ncut)
    counts, gotU, cjdx, cval = spgemm_dev(op, csr_a, rows_b, B_FIRST, JDIM_C, ncut)
    assert gotU.tolist() == U.tolist()
    assert counts.tolist() == np.diff(want["offs"], axis=1).tolist()
    assert cjdx.tobytes() == want["jdx"].tobytes()
    assert cval.tobytes() == want["val"].tobytes(), (ga_amd.OP_NAME[op], ncut, np.flatnonzero(cval.view(np.uint8) != want["val"].view(np.uint8))[:4])


@pytest.mark.gpu
def test_spgemm_nothing_to_do(gpu_lib):
    """an A without entries gives zero counts and bounds and writes nothing in fill; no row: no launch"""
    op, nrows, ncut = DBL, 9, 3
    none = S.build_csr(np.zeros(0, dtype=int), np.zeros(0, dtype=int), M.values(op, 0, np.random.default_rng(1)), 0, nrows, 10, 2)
    rows_b = (np.zeros(11, dtype=np.int64), np.zeros(4, dtype=np.int32), np.zeros(4, dtype=DT[op]))
    counts, U, cjdx, cval = spgemm_dev(op, none, rows_b, 0, 50, ncut)
    assert not counts.any() and not U.any() and len(cjdx) == 0 and len(cval) == 0
    c = ga_amd.DeviceBuffer(64)
    c.upload(np.full(64, 0x5A, dtype=np.uint8))
    assert ga_amd.spgemm_count(0, 2, 8, 8, 8, 0, 4, 8, 8, 50, 3, c.ptr, c.ptr + 32) == 0
    assert ga_amd.csr_rows(op, 0, 2, 8, 8, 8, 8, c.ptr, c.ptr + 16, c.ptr + 32) == 0
    ga_amd.sync()
    assert (c.download(np.uint8, 64) == 0x5A).all()
    c.free()


# ---- gaamd_csr_rows --------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, **opid)
def test_csr_rows(gpu_lib, op):
    """mixed_matrix's rows of 0 to 1000 entries with duplicates, on 1, 3 and 8 cuts (empty blocks among the 8), and a
    matrix without entries: offsets, columns and values of the model, canaries intact"""
    dt = DT[op]
    for ncut in NCUTS:
        rng = np.random.default_rng(40 + op + ncut)
        i, j, v, nrows, jdim = S.mixed_matrix(op, 1, ncut, rng)
        csr = S.build_csr(i, j, v, 0, nrows, jdim, ncut)
        roffs, rjdx, rval = ref_rows(csr)
        h = S.Held()
        try:
            offs, start, jdx, val = S.csr_up(h, csr)
            ob, oimg = out_buf(h, (nrows + 1) * 8)
            jb, jimg = out_buf(h, len(rjdx) * 4)
            vb, vimg = out_buf(h, len(rjdx) * dt.itemsize)
            assert ga_amd.csr_rows(op, nrows, len(csr["blocks"]), offs, start, jdx, val, ob.ptr + LEAD, jb.ptr + LEAD, vb.ptr + LEAD) == 0
            ga_amd.sync()
            assert body(ob, oimg, (nrows + 1) * 8).tobytes() == roffs.tobytes()
            assert body(jb, jimg, len(rjdx) * 4).tobytes() == rjdx.tobytes()
            assert body(vb, vimg, len(rjdx) * dt.itemsize).tobytes() == rval.tobytes()
            ob, oimg = out_buf(h, (nrows + 1) * 8)
            assert ga_amd.csr_rows(op, nrows, 0, 0, 0, 0, 0, ob.ptr + LEAD, 0, 0) == 0
            ga_amd.sync()
            assert not body(ob, oimg, (nrows + 1) * 8).any()
        finally:
            h.free()


@pytest.mark.gpu
def test_csr_rows_more_rows_than_the_scan_has_threads(gpu_lib):
    """3001 rows of 0 to 3 entries: every thread of the one-workgroup prefix sum has several rows, the last fewer"""
    op, nrows, jdim = FLT, 3001, 97
    rng = np.random.default_rng(8)
    i = np.repeat(np.arange(nrows), rng.integers(0, 4, nrows))
    j = rng.integers(0, jdim, len(i))
    csr = S.build_csr(i, j, M.values(op, len(i), rng), 0, nrows, jdim, 3)
    roffs, rjdx, rval = ref_rows(csr)
    h = S.Held()
    try:
        offs, start, jdx, val = S.csr_up(h, csr)
        ob, oimg = out_buf(h, (nrows + 1) * 8)
        jb, jimg = out_buf(h, len(rjdx) * 4)
        vb, vimg = out_buf(h, len(rjdx) * 4)
        assert ga_amd.csr_rows(op, nrows, 3, offs, start, jdx, val, ob.ptr + LEAD, jb.ptr + LEAD, vb.ptr + LEAD) == 0
        ga_amd.sync()
        assert body(ob, oimg, (nrows + 1) * 8).tobytes() == roffs.tobytes()
        assert body(jb, jimg, len(rjdx) * 4).tobytes() == rjdx.tobytes()
        assert body(vb, vimg, len(rjdx) * 4).tobytes() == rval.tobytes()
    finally:
        h.free()


# ---- the fallback over several windows of one column block -----------------------------
WIN = 32768          # columns of a window of the fallback's bitmap (ga_amd.h)
JDIM_W = 300000      # 10 windows on 1 cut; on 3 cuts blocks of 100 000: windows of 32768, 32768, 32768 and 1696


def wide_case(op):
    """a 4 x 8 A and an 8 x JDIM_W B.  The columns of B lie, within [0, 100 000) and again within [200 000, 300 000),
    in the windows 0, 2 and 3 of a block of 3 cuts, window 1 and the whole block [100 000, 200 000) staying empty, the
    edges 0, 32767, 65536, 98303, 98304 and 99999 among them; on 1 cut those are the windows 0, 2, 3, 6, 8 and 9, whose
    starts are no block starts.  Row 0 of A names the rows 0 .. 5 of B and row 2 twice (U about 1800, the fallback, a
    duplicate run in B's row 2 on an edge column); row 1 names row 6 five times (U = 1500 on 300 columns); row 2 one row
    (the LDS path); row 3 nothing"""
    if ("wide", op) in _cases:
        return _cases[("wide", op)]
    rng = np.random.default_rng(900 + op)
    edges = np.array([0, WIN - 1, 2 * WIN, 3 * WIN - 1, 3 * WIN, 99999])
    inner = np.concatenate([np.arange(1, WIN - 1), np.arange(2 * WIN + 1, 3 * WIN - 1), np.arange(3 * WIN + 1, 99999)])
    pool = np.concatenate([inner, inner + 200000])
    kk, jj = [], []
    for k in range(6):
        cols = np.concatenate([rng.choice(pool, 250, replace=False), edges, edges + 200000] if k in (0, 2) else
                              [rng.choice(pool, 250, replace=False)])
        if k == 2:
            cols = np.concatenate([cols, [2 * WIN, 2 * WIN, cols[7], 200000 + 3 * WIN]])   # duplicate runs, two on edges
        kk += [k] * len(cols)
        jj += cols.tolist()
    c6 = rng.choice(pool, 300, replace=False)
    kk += [6] * 300 + [7] * 20
    jj += c6.tolist() + rng.choice(pool, 20, replace=False).tolist()
    bk, bj = np.array(kk), np.array(jj)
    perm = rng.permutation(len(bk))
    bk, bj = bk[perm], bj[perm]
    csr_b = S.build_csr(bk, bj, M.values(op, len(bk), rng), 0, 8, JDIM_W, 2)
    ai = np.array([0] * 7 + [1] * 5 + [2])
    ak = np.array([0, 1, 2, 3, 4, 5, 2] + [6] * 5 + [7])
    csr_a = S.build_csr(ai, ak, M.values(op, len(ai), rng), 0, 4, 8, 2)
    rows_b = ref_rows(csr_b)
    _cases[("wide", op)] = (csr_a, rows_b, ref_spgemm(op, csr_a, rows_b, 0))
    return _cases[("wide", op)]


def test_wide_case_crosses_windows():
    csr_a, rows_b, (i, j, v, U) = wide_case(FLT)
    assert U.tolist()[1:] == [1500, 20, 0] and U[0] > CAP
    for r, least in ((0, CAP), (1, 0)):   # both fallback rows: three windows of block 0 of 3 cuts with an empty one between
        win = set((j[i == r] // WIN).tolist())
        assert {0, 2, 3, 6, 9} <= win and 1 not in win and 4 not in win and 5 not in win and len(j[i == r]) > least // 2
        blk = j[i == r] // 100000
        assert set(blk.tolist()) == {0, 2}
        w3 = set((((j[i == r])[blk == 2] - 200000) // WIN).tolist())
        assert w3 == {0, 2, 3}
    roffs, rjdx, _ = rows_b
    r2 = rjdx[roffs[2]:roffs[3]]
    assert np.count_nonzero(r2 == 2 * WIN) == 3 and np.count_nonzero(r2 == 200000 + 3 * WIN) == 2
    assert {0, WIN - 1, 2 * WIN, 3 * WIN - 1, 3 * WIN, 99999, 200000, 299999} <= set(j[i == 0].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("ncut", [1, 3])
@pytest.mark.parametrize("op", OPS, **opid)
def test_spgemm_fallback_over_several_windows(gpu_lib, op, ncut):
    """rows above the LDS capacity whose columns lie in several windows of one column block, with empty windows and an
    empty block between them, columns on the windows' edges and duplicate runs: counts, columns and values bit for bit"""
    case = wide_case(op)
    csr_a, rows_b, (ci, cj, cv, U) = case
    want = S.build_csr(ci, cj, cv, 0, csr_a["nrows"], JDIM_W, ncut, keep_empty=True)
    counts, gotU, cjdx, cval = spgemm_dev(op, csr_a, rows_b, 0, JDIM_W, ncut)
    assert gotU.tolist() == U.tolist()
    assert counts.tolist() == np.diff(want["offs"], axis=1).tolist()
    assert cjdx.tobytes() == want["jdx"].tobytes()
    assert cval.tobytes() == want["val"].tobytes(), (ga_amd.OP_NAME[op], ncut)
