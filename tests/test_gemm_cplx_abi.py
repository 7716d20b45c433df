"""CPU: the argument checks of gaamd_gemm_cplx / gaamd_gemm_cplx_plan, the plan's tile grid
per op and the overlap rule; every code here is returned before anything is launched, so no
device is needed (the addresses are never dereferenced).  test_gemm_abi.py for the two
complex ops, plus the conjugate transpose among the trans characters.

Also here, because it needs no device: the check that the rounding bound of
test_gpu_gemm_cplx.py holds for the order contract itself -- a numpy restatement of
ga_amd.h's summation order in the element type stays within the bound on that test's seeds.
"""
import ctypes

import numpy as np
import pytest

import ga_amd

DCP, CPL = ga_amd.COMEX_ACC_DCP, ga_amd.COMEX_ACC_CPL
ESZ = {DCP: 16, CPL: 8}
BASE = 0x7F0000000000   # an address-shaped number; never read
A, B, C = BASE + (1 << 37), BASE + (2 << 37), BASE
AL, BE = 2 - 1j, -3 + 2j

# the codes of include/ga_amd.h
E_COUNT, E_OP, E_SCALAR, E_LD, E_ALIGN, E_OVERLAP = -3, -4, -5, -6, -8, -11
NINE = [(ta, tb) for ta in "NTC" for tb in "NTC"]


def both(op, ta, tb, m, n, k, lda, ldb, ldc, a=A, b=B, c=C, alpha=AL, beta=BE):
    """the plan's code; where that means no launch (an error, or 1: nothing to do) the
    entry point itself is called too and must agree.  A geometry that would launch is
    never handed to the entry point: the addresses are not memory."""
    prc, plan = ga_amd.gemm_cplx_plan(op, ta, tb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc)
    if prc != 0:
        rc = ga_amd.gemm_cplx(op, ta, tb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc)
        assert rc == (0 if prc == 1 else prc), (rc, prc)
    return prc


@pytest.mark.parametrize("op", [DCP, CPL])
@pytest.mark.parametrize("mnk", [(-1, 4, 4), (4, -1, 4), (4, 4, -1), (-5, -5, -5)])
def test_negative_extent(op, mnk):
    assert both(op, "N", "N", *mnk, 8, 8, 8) == E_COUNT


@pytest.mark.parametrize("op", [0, 1, 37, 38, 39, 42, 1006, 1007])
def test_op_other_than_cpl_dcp(op):
    L = ga_amd.lib()
    v = np.ones(2)
    vp = v.ctypes.data_as(ctypes.c_void_p)
    plan = (ctypes.c_longlong * 6)()
    args = (op, ord("N"), ord("N"), 4, 4, 4, vp, ctypes.c_void_p(A), 4, ctypes.c_void_p(B), 4, vp, ctypes.c_void_p(C), 4)
    assert L.gaamd_gemm_cplx(*args, None) == E_OP
    assert L.gaamd_gemm_cplx_plan(*args, plan) == E_OP


@pytest.mark.parametrize("op", [DCP, CPL])
def test_gaamd_gemm_still_refuses_the_complex_ops(op):
    """the real entry point is unchanged: that is why the complex one has a name of its own"""
    assert ga_amd.gemm_plan(op, "N", "N", 4, 4, 4, 1.0, A, 4, B, 4, 1.0, C, 4)[0] == E_OP


@pytest.mark.parametrize("ta,tb", [("X", "N"), ("N", "H"), ("h", "n"), (0, "N"), ("N", 1), ("*", "C")])
def test_trans_other_than_n_t_c(ta, tb):
    assert both(DCP, ta, tb, 4, 4, 4, 4, 4, 4) == E_OP


@pytest.mark.parametrize("ta", "NnTtCc")
@pytest.mark.parametrize("tb", "NnTtCc")
def test_every_spelling_of_trans_is_taken(ta, tb):
    assert ga_amd.gemm_cplx_plan(CPL, ta, tb, 4, 4, 4, AL, A, 4, B, 4, BE, C, 4)[0] == 0


def test_missing_scalar():
    for op in (DCP, CPL):
        for alpha, beta in ((None, BE), (AL, None), (None, None)):
            assert ga_amd.gemm_cplx(op, "N", "N", 4, 4, 4, alpha, A, 4, B, 4, beta, C, 4) == E_SCALAR
            assert ga_amd.gemm_cplx_plan(op, "N", "N", 4, 4, 4, alpha, A, 4, B, 4, beta, C, 4)[0] == E_SCALAR


@pytest.mark.parametrize("ta,tb", NINE, ids=lambda t: t)
def test_ld_below_the_stored_row(ta, tb):
    m, n, k = 5, 7, 9
    # as stored: A m x k or k x m, B k x n or n x k ('C' is stored as 'T'), C m x n
    la = k if ta == "N" else m
    lb = n if tb == "N" else k
    for op in (DCP, CPL):
        # m = n = 0 would end in "nothing to do" only after the checks
        assert ga_amd.gemm_cplx_plan(op, ta, tb, m, n, k, AL, A, la, B, lb, BE, C, n)[0] == 0
        assert both(op, ta, tb, m, n, k, la - 1, lb, n) == E_LD
        assert both(op, ta, tb, m, n, k, la, lb - 1, n) == E_LD
        assert both(op, ta, tb, m, n, k, la, lb, n - 1) == E_LD


def test_base_below_the_alignment_of_the_part():
    for op, off in ((DCP, 4), (DCP, 1), (DCP, 12), (CPL, 2), (CPL, 1), (CPL, 6)):
        assert both(op, "N", "N", 4, 4, 4, 4, 4, 4, a=A + off) == E_ALIGN
        assert both(op, "N", "N", 4, 4, 4, 4, 4, 4, b=B + off) == E_ALIGN
        assert both(op, "N", "N", 4, 4, 4, 4, 4, 4, c=C + off) == E_ALIGN
    # the alignment of the real part is enough: 8 for f64 complex, 4 for f32 complex
    assert both(DCP, "N", "N", 4, 4, 4, 4, 4, 4, a=A + 8) == 0
    assert both(DCP, "N", "N", 4, 4, 4, 4, 4, 4, a=A + 8, b=B + 24, c=C + 8) == 0
    assert both(CPL, "N", "N", 4, 4, 4, 4, 4, 4, a=A + 4, b=B + 12, c=C + 4) == 0


@pytest.mark.parametrize("op", [DCP, CPL])
@pytest.mark.parametrize("mnk", [(0, 5, 5), (5, 0, 5), (0, 0, 0), (0, 5, 0)])
def test_empty_c_is_success_without_a_launch(op, mnk):
    """no device here: a launch would fail, 0 shows there was none"""
    m, n, k = mnk
    assert ga_amd.gemm_cplx(op, "N", "N", m, n, k, AL, A, 8, B, 8, BE, C, 8) == 0
    assert ga_amd.gemm_cplx_plan(op, "N", "N", m, n, k, AL, A, 8, B, 8, BE, C, 8)[0] == 1


@pytest.mark.parametrize("op", [DCP, CPL])
def test_plan_gives_the_tiles_and_the_grid(op):
    rc, p0 = ga_amd.gemm_cplx_plan(op, "N", "N", 1, 1, 1, AL, A, 1, B, 1, BE, C, 1)
    assert rc == 0
    tm, tn, tk = p0["tm"], p0["tn"], p0["tk"]
    assert tm >= 16 and tn >= 16 and tk >= 4 and tm % 16 == 0 and tn % 16 == 0 and tk % 4 == 0
    assert (p0["grid_m"], p0["grid_n"], p0["ksteps"]) == (1, 1, 1)
    ceil = lambda x, t: -(-x // t)   # noqa: E731
    for m in (1, tm - 1, tm, tm + 1, 2 * tm + 3):
        for n in (1, tn - 1, tn, tn + 1, 2 * tn + 3):
            for k in (1, tk - 1, tk, tk + 1, 2 * tk + 3):
                for ta, tb in (("N", "N"), ("T", "T"), ("C", "N"), ("N", "C")):
                    big = max(m, n, k)
                    rc, p = ga_amd.gemm_cplx_plan(op, ta, tb, m, n, k, AL, A, big, B, big, BE, C, big)
                    assert rc == 0
                    assert (p["tm"], p["tn"], p["tk"]) == (tm, tn, tk)
                    assert (p["grid_m"], p["grid_n"], p["ksteps"]) == (ceil(m, tm), ceil(n, tn), ceil(k, tk)), (m, n, k)
    # k = 0 is legal: no k steps (the call scales C)
    rc, p = ga_amd.gemm_cplx_plan(op, "N", "N", 5, 5, 0, AL, A, 5, B, 5, BE, C, 5)
    assert rc == 0 and p["ksteps"] == 0


@pytest.mark.parametrize("op", [DCP, CPL])
def test_overlap_is_judged_on_byte_spans(op):
    """ga_amd.h: first stored element to last, in elements of 16 and of 8 bytes.  C exactly A
    overlaps; C inside B's ld padding (no element shared) overlaps; C beginning where A's
    last element ends does not; A and B may overlap each other freely."""
    m, n, k, es = 6, 5, 4, ESZ[op]
    assert both(op, "N", "N", m, n, k, 8, 8, 8, a=C) == E_OVERLAP
    assert both(op, "N", "N", m, n, k, 8, 8, 8, b=C) == E_OVERLAP
    # A's span is ((m - 1) * lda + k) elements: C adjacent after it, and A adjacent after C
    a_span = ((m - 1) * 8 + k) * es
    c_span = ((m - 1) * 8 + n) * es
    assert both(op, "N", "N", m, n, k, 8, 8, 8, a=C - a_span) == 0
    assert both(op, "N", "N", m, n, k, 8, 8, 8, a=C + c_span) == 0
    # one part closer on either side: the last byte of one meets the first of the other
    assert both(op, "N", "N", m, n, k, 8, 8, 8, a=C - a_span + es // 2) == E_OVERLAP
    assert both(op, "N", "N", m, n, k, 8, 8, 8, a=C + c_span - es // 2) == E_OVERLAP
    # C in the padding of B's rows: B is k x n with ld 16, C is m x 2 with ld 16, eight
    # columns to the right of B's elements -- no element shared, the spans interleave
    assert both(op, "N", "N", 3, 2, k, 8, 16, 16, b=C - 8 * es) == E_OVERLAP
    # transposed and conjugate-transposed operands: the span follows the stored shape (A is k x m)
    at_span = ((k - 1) * 8 + m) * es
    for t in "TC":
        assert both(op, t, "N", m, n, k, 8, 8, 8, a=C - at_span) == 0
        assert both(op, t, "N", m, n, k, 8, 8, 8, a=C - at_span + es) == E_OVERLAP
    # A and B are only read
    assert both(op, "N", "N", m, n, k, 8, 8, 8, a=A, b=A) == 0
    assert both(op, "N", "N", m, n, k, 8, 8, 8, a=A, b=A + es // 2) == 0


@pytest.mark.parametrize("op", [DCP, CPL])
@pytest.mark.parametrize("vec", [False, True], ids=["odd", "vec"])
def test_far_leading_dimensions_plan_like_compact_ones(op, vec):
    """the leading dimensions of tests/test_gpu_far_offsets.py (an operand's rows spread
    over 9 GiB) on each operand in turn: accepted, with the tiles and the grid of compact
    ones; the operands are 128 GiB apart, so no span meets another"""
    from test_gpu_far_offsets import far_ld, stored_shape
    es = ESZ[op]
    rc, p0 = ga_amd.gemm_cplx_plan(op, "N", "N", 1, 1, 1, AL, A, 1, B, 1, BE, C, 1)
    m, n, k = p0["tm"] + 1, p0["tn"] + 1, p0["tk"] + 1
    for ta, tb in NINE:
        sa, sb = "N" if ta == "N" else "T", "N" if tb == "N" else "T"   # 'C' is stored as 'T'
        ld = {w: stored_shape(w, sa, sb, m, n, k)[1] + 5 for w in "ABC"}
        rc, compact = ga_amd.gemm_cplx_plan(op, ta, tb, m, n, k, AL, A, ld["A"], B, ld["B"], BE, C, ld["C"])
        assert rc == 0 and (compact["grid_m"], compact["grid_n"], compact["ksteps"]) == (2, 2, 2)
        for which in "ABC":
            rows = stored_shape(which, sa, sb, m, n, k)[0]
            big = dict(ld)
            big[which] = far_ld(rows, es, vec)
            assert (rows - 1) * big[which] * es >= 9 << 30
            rc, p = ga_amd.gemm_cplx_plan(op, ta, tb, m, n, k, AL, A, big["A"], B, big["B"], BE, C, big["C"])
            assert rc == 0 and p == compact, (ta, tb, which, p, compact)


# ---- the GPU test's bound, checked against the order contract itself -----------------------
def contract_model(op, ta, tb, al, be, opa, opb, c0):
    """ga_amd.h's order in the element type, every operation rounded once (numpy has no FMA):
    two accumulators from +0; per group of four k, re takes a.re * b.re and then -a.im * b.im,
    im takes a.re * b.im and then a.im * b.re, the four products of an instruction added one
    by one; then t = alpha * acc, u = beta * c, c = t + u part by part.  opa, opb are op(A),
    op(B): the conjugation is exact and already in them."""
    rt = np.float64 if op == DCP else np.float32
    ar, ai = opa.real.astype(rt), opa.imag.astype(rt)
    br, bi = opb.real.astype(rt), opb.imag.astype(rt)
    nbi = -bi
    m, k = ar.shape
    n = br.shape[1]
    re, im = np.zeros((m, n), rt), np.zeros((m, n), rt)
    for k0 in range(0, k, 4):
        ks = range(k0, min(k, k0 + 4))
        for kk in ks:
            re = re + np.outer(ar[:, kk], br[kk])
        for kk in ks:
            re = re + np.outer(ai[:, kk], nbi[kk])
        for kk in ks:
            im = im + np.outer(ar[:, kk], bi[kk])
        for kk in ks:
            im = im + np.outer(ai[:, kk], br[kk])
    assert re.dtype == rt and im.dtype == rt
    alr, ali, ber, bei = rt(al.real), rt(al.imag), rt(be.real), rt(be.imag)
    cr, ci = c0.real.astype(rt), c0.imag.astype(rt)
    out_re = (alr * re - ali * im) + (ber * cr - bei * ci)
    out_im = (alr * im + ali * re) + (ber * ci + bei * cr)
    assert out_re.dtype == rt
    return out_re, out_im


@pytest.mark.parametrize("shape", [(257, 131, 1000), (64, 64, 4099)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("op", [DCP, CPL], ids=["dcp", "cpl"])
def test_order_contract_stays_within_the_gpu_tests_bound(op, shape):
    """the bound of test_gpu_gemm_cplx.py is derived (2k products per part in any order, six
    roundings of the epilogue); here the contract's own order, restated in numpy, is held
    against it on the same seeds -- so a GPU failure of that bound is the kernel's"""
    from test_gpu_gemm_cplx import random_case
    opa, opb, c0, al, be, ref, bound = random_case(op, shape)
    got_re, got_im = contract_model(op, "N", "N", al, be, opa, opb, c0)
    err_re = np.abs(got_re.astype(ref.real.dtype) - ref.real)
    err_im = np.abs(got_im.astype(ref.real.dtype) - ref.imag)
    worst = float(max(np.max(err_re / bound), np.max(err_im / bound)))
    print(f"contract model {ga_amd.OP_NAME[op]} {shape}: max |err| / bound = {worst:.4f}")
    assert np.all(err_re <= bound) and np.all(err_im <= bound), worst
