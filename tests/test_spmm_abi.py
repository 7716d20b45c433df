"""No GPU: the exported names of sparse x dense and the dense / sparse conversions, the codes their
kernel entry points return before any launch (include/ga_amd.h states codes and order), and that
the data of tests/test_gpu_spmm.py has teeth: the sequential unfused sum of the contract differs
from the fused one and from the reversed one.
"""
import numpy as np

import ga_amd
import test_gpu_spmm as M
import test_sprs_abi as A0
from ga_amd._lib import GA_LIB_PATH, LIB_PATH

S = M.S
NEW_CORE = ["gaamd_spmm", "gaamd_dense_row_counts", "gaamd_dense_to_csr", "gaamd_csr_to_dense"]
NEW_GA = ["NGA_Sprs_array_sprsdns_multiply", "NGA_Sprs_array_create_from_dense", "NGA_Sprs_array_create_from_sparse",
          "gaamd_ga_spmm_route_counts"]
A = 0x7F0000000000   # address-shaped numbers; never read
E_COUNT, E_OP, E_SCALAR, E_STRIDE, E_RANGE, E_ALIGN, E_OVERLAP = -3, -4, -5, -6, -7, -8, -11


def test_exported_names():
    core, ga = A0.exported(LIB_PATH), A0.exported(GA_LIB_PATH)
    assert not [n for n in NEW_CORE if n not in core]
    assert not [n for n in NEW_CORE if n in ga]
    assert not [n for n in NEW_GA if n not in ga]
    assert not [n for n in core if n.startswith(("GA_", "NGA_", "gaamd_ga_"))]


def in_order(call, bad):
    """bad: [(code, overrides)] in the order of the contract; each code alone, and every earlier fault
    wins over every later one when both are present"""
    for k, (code, over) in enumerate(bad):
        assert call(**over) == code, (code, over)
        for later, over2 in bad[k + 1:]:
            if set(over) & set(over2):
                continue
            assert call(**{**over2, **over}) == code, (code, over, over2)


def test_spmm_codes():
    spmm = lambda **k: ga_amd.spmm(**{**dict(op=S.DBL, nrows=5, nblk=1, offs=A, start=A, jdx=A, val=A, b=A + (1 << 30),  # noqa: E731
                                             ldb=8, b_first=0, n=8, c=A + (2 << 30), ldc=8), **k})
    assert spmm(nrows=-1) == spmm(nblk=-1) == spmm(n=-1) == E_COUNT
    assert spmm(op=36) == spmm(op=0) == E_OP
    assert spmm(nrows=0) == spmm(n=0) == spmm(nrows=0, c=0) == spmm(n=0, ldc=-4, c=3) == 0   # before the pointers
    for miss in ("offs", "start", "jdx", "val", "b", "c"):
        assert spmm(**{miss: 0}) == E_SCALAR, miss
    assert spmm(nblk=0, offs=0, start=0, jdx=0, val=0, b=0, c=0) == E_SCALAR   # c is still needed
    assert spmm(ldc=7) == spmm(ldb=7) == E_STRIDE
    assert spmm(nrows=(1 << 40) + 1) == spmm(n=1 << 31, ldb=1 << 31, ldc=1 << 31) == E_RANGE
    assert spmm(c=A + (2 << 30) + 4) == spmm(b=A + (1 << 30) + 4) == spmm(val=A + 4) == spmm(start=A + 4) == E_ALIGN
    assert spmm(offs=A + 2) == spmm(jdx=A + 2) == spmm(op=S.DCP, c=A + (2 << 30) + 8) == E_ALIGN
    assert spmm(c=A + (1 << 30)) == spmm(c=A + (1 << 30) - 8 * 8 * 4) == spmm(b=A + (2 << 30) + 8 * 36) == E_OVERLAP
    in_order(spmm, [(E_COUNT, dict(nrows=-1)), (E_OP, dict(op=36)), (E_SCALAR, dict(val=0)), (E_STRIDE, dict(ldc=7)),
                    (E_RANGE, dict(nrows=(1 << 40) + 1)), (E_ALIGN, dict(jdx=A + 2)), (E_OVERLAP, dict(c=A + (1 << 30)))])
    assert spmm(n=0, op=36) == E_OP and spmm(nrows=0, nblk=-1) == E_COUNT   # zero counts come third


def test_dense_to_csr_codes():
    cnt = lambda **k: ga_amd.dense_row_counts(**{**dict(op=S.FLT, rows=6, cols=9, a=A, lda=12, row_first=0, col_first=3,  # noqa: E731
                                                         counts=A + (1 << 30)), **k})
    sto = lambda **k: ga_amd.dense_to_csr(**{**dict(op=S.FLT, rows=6, cols=9, a=A, lda=12, row_first=0, col_first=3,  # noqa: E731
                                                     offs=A + (1 << 30), jdx=A + (2 << 30), val=A + (3 << 30)), **k})
    for f, outs in ((cnt, ("counts",)), (sto, ("offs", "jdx", "val"))):
        assert f(rows=-1) == f(cols=-1) == E_COUNT and f(op=36) == E_OP
        assert f(rows=0) == f(cols=0) == f(rows=0, a=0) == 0
        for miss in ("a",) + outs:
            assert f(**{miss: 0}) == E_SCALAR, miss
        assert f(lda=8) == E_STRIDE
        assert f(rows=(1 << 40) + 1) == f(col_first=(1 << 31) - 8) == f(col_first=-1) == f(row_first=-1) == E_RANGE
        assert f(a=A + 2) == E_ALIGN
        assert f(**{outs[-1]: A + 12 * 4}) == E_OVERLAP
        in_order(f, [(E_COUNT, dict(rows=-1)), (E_OP, dict(op=36)), (E_SCALAR, dict(a=0)), (E_STRIDE, dict(lda=8)),
                     (E_RANGE, dict(row_first=-1))])
    assert sto(jdx=A + (2 << 30) + 2) == sto(offs=A + (1 << 30) + 2) == cnt(counts=A + (1 << 30) + 2) == E_ALIGN
    assert sto(op=S.DCP, val=A + (3 << 30) + 8) == E_ALIGN and sto(jdx=A + 8) == E_OVERLAP


def test_csr_to_dense_codes():
    f = lambda **k: ga_amd.csr_to_dense(**{**dict(op=S.LNG, nrows=6, cols=9, offs=A, jdx=A + (1 << 30), val=A + (2 << 30),  # noqa: E731
                                                   col_first=100, out=A + (3 << 30), ldo=9), **k})
    assert f(nrows=-1) == f(cols=-1) == E_COUNT and f(op=1) == E_OP
    assert f(nrows=0) == f(cols=0) == f(nrows=0, out=0) == 0
    for miss in ("offs", "jdx", "val", "out"):
        assert f(**{miss: 0}) == E_SCALAR, miss
    assert f(ldo=8) == E_STRIDE and f(nrows=(1 << 40) + 1) == E_RANGE
    assert f(out=A + (3 << 30) + 4) == f(val=A + (2 << 30) + 4) == f(jdx=A + (1 << 30) + 2) == f(offs=A + 2) == E_ALIGN
    assert f(out=A + 8) == f(out=A + (1 << 30) - 8) == f(out=A + (2 << 30)) == E_OVERLAP
    in_order(f, [(E_COUNT, dict(nrows=-1)), (E_OP, dict(op=1)), (E_SCALAR, dict(val=0)), (E_STRIDE, dict(ldo=8)),
                 (E_RANGE, dict(nrows=(1 << 40) + 1)), (E_ALIGN, dict(jdx=A + (1 << 30) + 2)),
                 (E_OVERLAP, dict(out=A + 8))])


# ---- the data of the GPU test has teeth ---------------------------------------------------
def test_f32_data_tells_fused_and_reversed_from_the_contract():
    op, n = S.FLT, 17
    csr, b, _ = M.spmm_case(op, ncut=3, n=n, ldb=n)
    want = M.ref_spmm(op, csr, b, 0, n)
    f32, f64 = np.float32, np.float64
    fused = M.ref_spmm(op, csr, b, 0, n, step=lambda acc, a, brow: f32(f64(a) * brow.astype(f64) + acc.astype(f64)))
    rev = M.ref_spmm(op, csr, b, 0, n, reverse=True)
    assert (fused.view(np.uint32) != want.view(np.uint32)).any()
    assert (rev.view(np.uint32) != want.view(np.uint32)).any()
    # and the restatement is the plain loop of the contract
    rows = S.entry_rows(csr)
    order = np.argsort(rows, kind="stable")
    loop = np.zeros((csr["nrows"], n), dtype=f32)
    for k in order:
        r = rows[k]
        for j in range(n):
            p = f32(csr["val"][k] * b[csr["jdx"][k], j])
            loop[r, j] = f32(loop[r, j] + p)
    assert loop.tobytes() == want.tobytes()


def test_restatement_n1_is_the_matvec_of_team_1():
    for op in S.OPS:
        csr, b, _ = M.spmm_case(op, ncut=3, n=1, ldb=1)
        assert M.ref_spmm(op, csr, b, 0, 1)[:, 0].tobytes() == S.ref_spmv(op, csr, np.ascontiguousarray(b[:, 0]), 0, 1).tobytes()


def test_dense_filter_rule():
    """-0.0 is not kept, a NaN is, an imaginary part alone is, a zero on the diagonal is"""
    a = np.zeros((3, 4), dtype=np.complex64)
    a[0, 1] = complex(-0.0, 0.0)
    a[0, 2] = complex(0.0, 2.0)
    a[1, 3] = complex(np.nan, 0.0)
    keep = M.ref_keep(S.CPL, a, row_first=10, col_first=10)
    assert keep.tolist() == [[True, False, True, False], [False, True, False, True], [False, False, True, False]]
