"""No GPU: the exported names of sparse x sparse, the codes its kernel entry points return before any launch
(include/ga_amd.h states codes and order), and that the data of tests/test_gpu_spgemm.py has teeth: the
contract's sum differs from the fused, the reversed and the assign-first one.
"""
import numpy as np

import ga_amd
import test_gpu_spgemm as G
import test_spmm_abi as A1
import test_sprs_abi as A0
from ga_amd._lib import GA_LIB_PATH, LIB_PATH

S = G.S
NEW_CORE = ["gaamd_csr_rows", "gaamd_spgemm_count", "gaamd_spgemm_fill", "gaamd_spgemm_lds_cap"]
NEW_GA = ["NGA_Sprs_array_matmat_multiply", "gaamd_ga_spgemm_route_counts"]
A = 0x7F0000000000   # address-shaped numbers; never read
G1 = 1 << 30
E_COUNT, E_OP, E_SCALAR, E_RANGE, E_ALIGN, E_OVERLAP = -3, -4, -5, -7, -8, -11
in_order = A1.in_order


def test_exported_names():
    core, ga = A0.exported(LIB_PATH), A0.exported(GA_LIB_PATH)
    assert not [n for n in NEW_CORE if n not in core]
    assert not [n for n in NEW_CORE if n in ga]
    assert not [n for n in NEW_GA if n not in ga]
    assert ga_amd.spgemm_lds_cap() == G.CAP   # host only


def test_csr_rows_codes():
    f = lambda **k: ga_amd.csr_rows(**{**dict(op=S.DBL, nrows=5, nblk=2, offs=A, start=A + G1, jdx=A + 2 * G1, val=A + 3 * G1,  # noqa: E731
                                              roffs=A + 4 * G1, rjdx=A + 5 * G1, rval=A + 6 * G1), **k})
    assert f(nrows=-1) == f(nblk=-1) == E_COUNT and f(op=36) == f(op=0) == E_OP
    assert f(nrows=0) == f(nrows=0, roffs=0) == 0
    for miss in ("offs", "start", "jdx", "val", "roffs", "rjdx", "rval"):
        assert f(**{miss: 0}) == E_SCALAR, miss
    assert f(nblk=0, offs=0, start=0, jdx=0, val=0, rjdx=0, rval=0, roffs=0) == E_SCALAR   # roffs is still needed
    assert f(nrows=(1 << 40) + 1) == E_RANGE
    assert f(roffs=A + 4 * G1 + 4) == f(start=A + G1 + 4) == f(val=A + 3 * G1 + 4) == f(rval=A + 6 * G1 + 4) == E_ALIGN
    assert f(offs=A + 2) == f(jdx=A + 2 * G1 + 2) == f(rjdx=A + 5 * G1 + 2) == f(op=S.DCP, rval=A + 6 * G1 + 8) == E_ALIGN
    assert f(roffs=A + 8) == f(roffs=A - 40) == f(rjdx=A + 44) == f(rval=A + 3 * G1) == f(rjdx=A + 2 * G1) == E_OVERLAP
    in_order(f, [(E_COUNT, dict(nrows=-1)), (E_OP, dict(op=36)), (E_SCALAR, dict(val=0)), (E_RANGE, dict(nrows=(1 << 40) + 1)),
                 (E_ALIGN, dict(jdx=A + 2 * G1 + 2)), (E_OVERLAP, dict(roffs=A + 8))])
    assert f(nrows=0, op=36) == E_OP and f(nrows=0, nblk=-1) == E_COUNT   # a zero count comes third


def test_spgemm_codes():
    base = dict(nrows=5, nblk=2, offs=A, start=A + G1, jdx=A + 2 * G1, b_first=0, brows=9, roffs=A + 4 * G1, rjdx=A + 5 * G1,
                jdim_c=100, ncut=3)
    cnt = lambda **k: ga_amd.spgemm_count(**{**base, **dict(counts=A + 7 * G1, bound=A + 8 * G1), **k})   # noqa: E731
    fil = lambda **k: ga_amd.spgemm_fill(**{**base, **dict(op=S.FLT, val=A + 3 * G1, rval=A + 6 * G1, coffs=A + 9 * G1,  # noqa: E731
                                                           cstart=A + 10 * G1, cjdx=A + 11 * G1, cval=A + 12 * G1), **k})
    for f, outs in ((cnt, ("counts", "bound")), (fil, ("coffs", "cstart", "cjdx", "cval"))):
        assert f(nrows=-1) == f(nblk=-1) == f(brows=-1) == f(jdim_c=-1) == f(ncut=-1) == E_COUNT
        assert f(nrows=0) == f(ncut=0) == f(nrows=0, **{outs[0]: 0}) == 0
        for miss in ("offs", "start", "jdx", "roffs", "rjdx") + outs:
            assert f(**{miss: 0}) == E_SCALAR, miss
        assert f(nblk=0, offs=0, start=0, jdx=0, roffs=0, rjdx=0, **{outs[-1]: 0}) == E_SCALAR   # the outputs are still needed
        assert f(nrows=(1 << 40) + 1) == f(brows=(1 << 40) + 1) == f(jdim_c=1 << 31) == f(jdim_c=0) == E_RANGE
        assert f(b_first=-1) == E_RANGE
        assert f(start=A + G1 + 4) == f(roffs=A + 4 * G1 + 4) == f(offs=A + 2) == f(jdx=A + 2 * G1 + 2) == E_ALIGN
        assert f(rjdx=A + 5 * G1 + 2) == f(**{outs[0]: base["offs"] + 7 * G1 + 2}) == E_ALIGN
        assert f(**{outs[-1]: A + 16}) == f(**{outs[-1]: A + 4 * G1 + 8 * 9}) == f(**{outs[-1]: A + 5 * G1}) == E_OVERLAP
        in_order(f, [(E_COUNT, dict(nrows=-1)), (E_SCALAR, dict(jdx=0)), (E_RANGE, dict(jdim_c=0)),
                     (E_ALIGN, dict(offs=A + 2)), (E_OVERLAP, dict(**{outs[-1]: A + 16}))])
        assert f(nrows=0, nblk=-1) == E_COUNT   # a zero count comes after the negative ones
    assert cnt(bound=A + 8 * G1 + 4) == E_ALIGN
    assert fil(op=36) == fil(op=0) == fil(nrows=0, op=36) == E_OP and fil(op=36, nrows=-1) == E_COUNT
    assert fil(val=0) == fil(rval=0) == E_SCALAR
    assert fil(op=S.DCP, cval=A + 12 * G1 + 8) == fil(val=A + 3 * G1 + 2) == fil(cstart=A + 10 * G1 + 4) == E_ALIGN
    assert fil(cjdx=A + 9 * G1 + 4 * 17) == fil(cval=A + 3 * G1) == E_OVERLAP
    assert fil(nblk=0, offs=0, start=0, jdx=0, val=0, roffs=0, rjdx=0, rval=0) == 0   # nothing to store


# ---- the data of the GPU test has teeth ---------------------------------------------------
def test_f32_data_tells_fused_reversed_and_assign_first_from_the_contract():
    op = S.FLT
    csr_a, rows_b, (i, j, want, _) = G.spgemm_case(op)
    f32, f64 = np.float32, np.float64
    fused = G.ref_spgemm(op, csr_a, rows_b, G.B_FIRST, step=lambda acc, a, b, s: (a.astype(f64) * b.astype(f64) + acc.astype(f64)).astype(f32))
    rev = G.ref_spgemm(op, csr_a, rows_b, G.B_FIRST, reverse=True)
    first = G.ref_spgemm(op, csr_a, rows_b, G.B_FIRST, step=lambda acc, a, b, s: a * b if s == 0 else acc + a * b)
    for other in (fused, rev, first):
        assert other[0].tolist() == i.tolist() and other[1].tolist() == j.tolist()   # the structure is the same
    bits = lambda x: x.view(np.uint32)   # noqa: E731
    assert (bits(fused[2]) != bits(want)).any()
    assert (bits(rev[2]) != bits(want)).any()
    differ = np.flatnonzero(bits(first[2]) != bits(want))
    assert differ.tolist() == np.flatnonzero(i == 2).tolist()   # the lone -0.0 product alone: the stated departure
    assert bits(first[2])[differ[0]] == 0x80000000 and bits(want)[differ[0]] == 0
    # and the restatement is the plain loop of the contract
    roffs, rjdx, rval = rows_b
    rows = S.entry_rows(csr_a)
    loop = {}
    for k in np.argsort(rows, kind="stable"):
        kb = int(csr_a["jdx"][k]) - G.B_FIRST
        for q in range(roffs[kb], roffs[kb + 1]):
            key = (int(rows[k]), int(rjdx[q]))
            loop[key] = f32(loop.get(key, f32(0)) + f32(csr_a["val"][k] * rval[q]))
    assert sorted(loop) == list(zip(i.tolist(), j.tolist()))
    got = np.array([loop[key] for key in zip(i.tolist(), j.tolist())], dtype=f32)
    assert got.tobytes() == want.tobytes()


def test_the_dense_identity_on_the_restatements():
    """for finite data and a B without duplicates the dense copy of A B is gaamd_spmm's A times the dense copy of B"""
    import test_gpu_spmm as M
    for op in S.OPS:
        rng = np.random.default_rng(5 + op)
        bi, bj = np.nonzero(rng.random((30, 40)) < 0.2)
        csr_b = S.build_csr(bi, bj, M.values(op, len(bi), rng), 0, 30, 40, 3)
        ai = rng.integers(0, 20, 90)
        csr_a = S.build_csr(ai, rng.integers(0, 30, 90), M.values(op, 90, rng), 0, 20, 30, 2)   # duplicates in A are fine
        i, j, v, _ = G.ref_spgemm(op, csr_a, G.ref_rows(csr_b), 0)
        dense_b = np.zeros((30, 40), dtype=S.DT[op])
        dense_b[S.entry_rows(csr_b), csr_b["jdx"]] = csr_b["val"]
        dense_c = np.zeros((20, 40), dtype=S.DT[op])
        dense_c[i, j] = v
        assert dense_c.tobytes() == M.ref_spmm(op, csr_a, dense_b, 0, 40).tobytes()
