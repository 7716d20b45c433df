"""ga_amd -- MI355X-native GA/ComEx strided pack/unpack + typed accumulate.

Python mirror of the C ABI in ``include/comex.h``, ``include/armci.h`` and
``include/ga_amd.h``.  The compute path is libga_amd.so (hand-written gfx950
HIP kernels); this package only marshals arguments.  Names follow the reference
(comex/src-common/comex.h, comex/src-armci/armci.h).
"""
import ctypes

import numpy as np

from ._lib import load, ALLGATHER_FN, BARRIER_FN  # noqa: F401

# comex.h:35-43 / armci.h:183-191
COMEX_GROUP_WORLD = 0
COMEX_SUCCESS = 0
COMEX_ACC_INT = 37
COMEX_ACC_DBL = 38
COMEX_ACC_FLT = 39
COMEX_ACC_CPL = 40
COMEX_ACC_DCP = 41
COMEX_ACC_LNG = 42
COMEX_MAX_STRIDE_LEVEL = 8
GAAMD_OP_COPY = 0

# op -> numpy dtype of one element (complex: the complex numpy type)
OP_DTYPE = {
    COMEX_ACC_INT: np.dtype(np.int32),
    COMEX_ACC_DBL: np.dtype(np.float64),
    COMEX_ACC_FLT: np.dtype(np.float32),
    COMEX_ACC_CPL: np.dtype(np.complex64),
    COMEX_ACC_DCP: np.dtype(np.complex128),
    COMEX_ACC_LNG: np.dtype(np.int64),
}
OP_NAME = {COMEX_ACC_INT: "int", COMEX_ACC_DBL: "dbl", COMEX_ACC_FLT: "flt", COMEX_ACC_CPL: "cpl",
           COMEX_ACC_DCP: "dcp", COMEX_ACC_LNG: "lng"}

KIND_NAME = {0: "auto", 1: "rows", 2: "flat", 3: "serial", 4: "ordered"}


def lib():
    return load()


def build_id():
    """sha256 of the sources libga_amd.so was compiled from (gaamd_build_id)."""
    return lib().gaamd_build_id().decode()


def check_build():
    """Raise when libga_amd.so was not built from the sources beside it (a stale
    prebuilt library shipped with a newer tree); returns the build id."""
    from .provenance import tree_hash
    built, tree = build_id(), tree_hash()
    if built != tree:
        raise RuntimeError(f"libga_amd.so is stale: built from sources {built[:16]}..., the tree here is "
                           f"{tree[:16]}... -- rebuild it (make -C ga_amd/csrc)")
    return built


def int_array(vals):
    vals = list(vals) if vals is not None else []
    arr = (ctypes.c_int * max(1, len(vals)))(*vals)
    return arr


def scale_buffer(op, scale):
    """The `void *scale` argument: one element of the op's type (complex = {re, im})."""
    dt = OP_DTYPE[op]
    a = np.array([scale], dtype=dt)
    return a, a.ctypes.data_as(ctypes.c_void_p)


class DeviceBuffer:
    """HBM allocation through the library (hipMalloc); never a torch tensor."""

    def __init__(self, nbytes, host=False):
        self.nbytes = int(nbytes)
        self.host = host
        L = lib()
        p = L.gaamd_host_malloc(self.nbytes) if host else L.gaamd_dev_malloc(max(1, self.nbytes))
        if not p:
            raise MemoryError(f"allocation of {nbytes} bytes failed")
        self.ptr = p

    def upload(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= self.nbytes
        rc = lib().gaamd_memcpy(ctypes.c_void_p(self.ptr + offset), arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes)
        if rc:
            raise RuntimeError("upload failed")

    def download(self, dtype, count=None, offset=0):
        dtype = np.dtype(dtype)
        if count is None:
            count = (self.nbytes - offset) // dtype.itemsize
        out = np.empty(count, dtype=dtype)
        rc = lib().gaamd_memcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.ptr + offset), out.nbytes)
        if rc:
            raise RuntimeError("download failed")
        return out

    def free(self):
        if self.ptr:
            (lib().gaamd_host_free if self.host else lib().gaamd_dev_free)(ctypes.c_void_p(self.ptr))
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- kernel-level API (ga_amd.h section 2) ---------------------------------
def strided(op, scale, src, src_stride, dst, dst_stride, count, stride_levels, stream=None):
    """Enqueue dst (+)= op(src) over a strided patch; src/dst are device addresses (ints)."""
    if op == GAAMD_OP_COPY:
        sp = None
    else:
        keep, sp = scale_buffer(op, scale)
    rc = lib().gaamd_strided(op, sp, ctypes.c_void_p(src), int_array(src_stride), ctypes.c_void_p(dst),
                             int_array(dst_stride), int_array(count), stride_levels, stream)
    if rc:
        raise RuntimeError(f"gaamd_strided failed with {rc}")


def pack(src, src_stride, count, stride_levels, packed, stream=None):
    rc = lib().gaamd_pack(ctypes.c_void_p(src), int_array(src_stride), int_array(count), stride_levels,
                          ctypes.c_void_p(packed), stream)
    if rc:
        raise RuntimeError(f"gaamd_pack failed with {rc}")


def unpack(packed, dst, dst_stride, count, stride_levels, stream=None):
    rc = lib().gaamd_unpack(ctypes.c_void_p(packed), ctypes.c_void_p(dst), int_array(dst_stride),
                            int_array(count), stride_levels, stream)
    if rc:
        raise RuntimeError(f"gaamd_unpack failed with {rc}")


def unpack_acc(op, scale, packed, dst, dst_stride, count, stride_levels, stream=None):
    keep, sp = scale_buffer(op, scale)
    rc = lib().gaamd_unpack_acc(op, sp, ctypes.c_void_p(packed), ctypes.c_void_p(dst), int_array(dst_stride),
                                int_array(count), stride_levels, stream)
    if rc:
        raise RuntimeError(f"gaamd_unpack_acc failed with {rc}")


def ll_array(vals):
    vals = list(vals) if vals is not None else []
    return (ctypes.c_longlong * max(1, len(vals)))(*vals)


# computing on a patch where it lies (gaamd_patch_*): count in elements per dimension
# (dimension 0 contiguous), strides in bytes of dimensions 1..; the return code is
# handed back (0, or the negative codes of ga_amd.h)
def patch_fill(op, value, dst, dst_stride, count, stream=None):
    keep, vp = scale_buffer(op, value)
    return lib().gaamd_patch_fill(op, vp, ctypes.c_void_p(dst), ll_array(dst_stride), ll_array(count), len(count),
                                  stream)


def patch_scale(op, alpha, dst, dst_stride, count, stream=None):
    keep, ap = scale_buffer(op, alpha)
    return lib().gaamd_patch_scale(op, ap, ctypes.c_void_p(dst), ll_array(dst_stride), ll_array(count), len(count),
                                   stream)


def patch_add(op, alpha, a, a_stride, beta, b, b_stride, c, c_stride, count, stream=None):
    ka, ap = scale_buffer(op, alpha)
    kb, bp = scale_buffer(op, beta)
    return lib().gaamd_patch_add(op, ap, ctypes.c_void_p(a), ll_array(a_stride), bp, ctypes.c_void_p(b),
                                 ll_array(b_stride), ctypes.c_void_p(c), ll_array(c_stride), ll_array(count),
                                 len(count), stream)


def patch_dot(op, a, a_stride, b, b_stride, count, stream=None):
    """(return code, one-element numpy array of the op's type)"""
    out = np.zeros(1, dtype=OP_DTYPE[op])
    rc = lib().gaamd_patch_dot(op, ctypes.c_void_p(a), ll_array(a_stride), ctypes.c_void_p(b), ll_array(b_stride),
                               ll_array(count), len(count), out.ctypes.data_as(ctypes.c_void_p), stream)
    return rc, out


# element-wise algebra (gaamd_patch_elem1 / _elem2): fn is one of these; the return code is
# handed back (0, GAAMD_ZERO_DIVISOR, or the negative codes of ga_amd.h)
GAAMD_ELEM_ABS, GAAMD_ELEM_ADD_CONST, GAAMD_ELEM_RECIP = 1, 2, 3
GAAMD_ELEM_MUL, GAAMD_ELEM_DIV, GAAMD_ELEM_MAX, GAAMD_ELEM_MIN = 4, 5, 6, 7
GAAMD_ZERO_DIVISOR = 2


def patch_elem1(op, fn, dst, dst_stride, count, scalar=None, stream=None):
    """dst = fn(dst) in place; scalar (ADD_CONST): one element, None reaches the library as NULL"""
    keep, sp = scale_buffer(op, scalar) if scalar is not None else (None, None)
    return lib().gaamd_patch_elem1(op, fn, sp, ctypes.c_void_p(dst), ll_array(dst_stride), ll_array(count),
                                   len(count), stream)


def patch_elem2(op, fn, a, a_stride, b, b_stride, c, c_stride, count, stream=None):
    """c = fn(a, b)"""
    return lib().gaamd_patch_elem2(op, fn, ctypes.c_void_p(a), ll_array(a_stride), ctypes.c_void_p(b),
                                   ll_array(b_stride), ctypes.c_void_p(c), ll_array(c_stride), ll_array(count),
                                   len(count), stream)


def patch_select(op, want_max, a, a_stride, count, stream=None):
    """(return code, the element as a one-element numpy array of the op's type, its key as a
    one-element array -- the element's own type, complex: its real type --, its linear index)"""
    dt = OP_DTYPE[op]
    val = np.zeros(1, dtype=dt)
    key = np.zeros(1, dtype=val.real.dtype)
    idx = ctypes.c_longlong(-2)
    rc = lib().gaamd_patch_select(op, int(bool(want_max)), ctypes.c_void_p(a), ll_array(a_stride), ll_array(count),
                                  len(count), val.ctypes.data_as(ctypes.c_void_p),
                                  key.ctypes.data_as(ctypes.c_void_p), ctypes.byref(idx), stream)
    return rc, val, key, idx.value


# GA's matrix.c calls at kernel level (gaamd_patch_norm / _diagonal / _scale_rows / _scale_cols);
# the return code is handed back (0, or the negative codes of ga_amd.h)
GAAMD_NORM_ONE, GAAMD_NORM_INF = 1, 2
GAAMD_DIAG_GET, GAAMD_DIAG_SET, GAAMD_DIAG_ADD, GAAMD_DIAG_SHIFT, GAAMD_DIAG_ZERO = 1, 2, 3, 4, 5


def patch_norm(op, kind, a, a_stride, count, stream=None):
    """(return code, the norm as a one-element numpy array of the op's type, complex: its real type)"""
    out = np.zeros(1, dtype=np.zeros(1, dtype=OP_DTYPE.get(op, np.float64)).real.dtype)
    out.view(np.uint8)[:] = 0xA5   # the call has to write it, the zero of an empty patch too
    rc = lib().gaamd_patch_norm(op, kind, ctypes.c_void_p(a), ll_array(a_stride), ll_array(count), len(count),
                                out.ctypes.data_as(ctypes.c_void_p), stream)
    return rc, out


def diag(op, fn, n, a, a_step, v, v_step, scalar=None, stream=None):
    """gaamd_diagonal: n elements at a + i * a_step and v + i * v_step (bytes); v of None or 0 and
    scalar of None reach the library as NULL"""
    keep, sp = scale_buffer(op, scalar) if scalar is not None else (None, None)
    return lib().gaamd_diagonal(op, fn, n, ctypes.c_void_p(a), a_step, ctypes.c_void_p(v) if v else None, v_step,
                                sp, stream)


def scale_rows(op, rows, cols, a, lda, v, stream=None):
    """a[i][j] *= v[i] in place; lda in elements; complex part by part"""
    return lib().gaamd_scale_rows(op, rows, cols, ctypes.c_void_p(a), lda, ctypes.c_void_p(v) if v else None, stream)


def scale_cols(op, rows, cols, a, lda, v, stream=None):
    """a[i][j] *= v[j] in place; lda in elements; complex part by part"""
    return lib().gaamd_scale_cols(op, rows, cols, ctypes.c_void_p(a), lda, ctypes.c_void_p(v) if v else None, stream)


# GA's sparse.c calls at kernel level (gaamd_enum / _scan_tail / _scan / _mask_count / _mask_pack /
# _mask_unpack): contiguous 1-D device arrays, n in elements, op the value type and mop the mask
# type; the return code is handed back (0, or the negative codes of ga_amd.h).  The compaction's
# wrappers are mask_pack / mask_unpack: pack and unpack are the strided ones above.
GAAMD_SCAN_COPY, GAAMD_SCAN_ADD, GAAMD_SCAN_ADD_EXCL = 1, 2, 3


def _vp(a):
    return ctypes.c_void_p(a) if a else None


def scan_tile(op, mop):
    """elements per tile (workgroup) of the scan and compaction kernels"""
    return lib().gaamd_scan_tile(op, mop)


def scan_agg_span():
    """tile aggregates the aggregate scan's one workgroup takes per pass of its loop"""
    return lib().gaamd_scan_agg_span()


def enum(op, n, first, start, stride, dst, stream=None):
    """dst[i] = start + (T)(first + i) * stride; start / stride of None reach the library as NULL"""
    ka, ap = scale_buffer(op, start) if start is not None else (None, None)
    kb, bp = scale_buffer(op, stride) if stride is not None else (None, None)
    return lib().gaamd_enum(op, n, first, ap, bp, _vp(dst), stream)


def scan_tail(op, fn, mop, n, src, msk, stream=None):
    """(return code, has_flag, the open value at the end of the range as a one-element array)"""
    tail = np.zeros(1, dtype=OP_DTYPE.get(op, np.complex128))
    tail.view(np.uint8)[:] = 0xA5   # the call has to write it, the zero of n == 0 too
    flag = ctypes.c_int(-1)
    rc = lib().gaamd_scan_tail(op, fn, mop, n, _vp(src), _vp(msk), ctypes.byref(flag),
                               tail.ctypes.data_as(ctypes.c_void_p), stream)
    return rc, flag.value, tail


def scan(op, fn, mop, n, src, msk, dst, open=0, carry=None, stream=None):
    """the segmented scan; carry: the open segment's value so far (with open != 0)"""
    kc, cp = scale_buffer(op, carry) if carry is not None else (None, None)
    return lib().gaamd_scan(op, fn, mop, n, _vp(src), _vp(msk), _vp(dst), int(open), cp, stream)


def mask_count(mop, n, msk, stream=None):
    """(return code, the number of set elements)"""
    cnt = ctypes.c_longlong(-1)
    rc = lib().gaamd_mask_count(mop, n, _vp(msk), ctypes.byref(cnt), stream)
    return rc, cnt.value


def mask_pack(op, mop, n, src, msk, packed, stream=None):
    """packed[k] = src[f_k], f_k the k-th set element of msk"""
    return lib().gaamd_mask_pack(op, mop, n, _vp(src), _vp(msk), _vp(packed), stream)


def mask_unpack(op, mop, n, packed, msk, dst, stream=None):
    """dst[f_k] = packed[k]; the other elements of dst are not written"""
    return lib().gaamd_mask_unpack(op, mop, n, _vp(packed), _vp(msk), _vp(dst), stream)


# GA's sparse arrays at kernel level (gaamd_spmv / _sprs_diag / _sprs_scale_left / _right): a block
# CSR in HBM -- nblk tables of nrows + 1 int offsets (block b's at offs + b * (nrows + 1)) relative to
# start[b] (long long, in HBM too) in jdx (global columns) / val.  Addresses are ints, 0 or None is
# NULL; the return code is handed back.
def spmv_team(nnz_total, rows):
    """the team (lanes per row) the GA layer uses for a matrix of nnz_total entries and `rows` rows"""
    return lib().gaamd_spmv_team(nnz_total, rows)


def spmv(op, nrows, nblk, offs, start, jdx, val, x, x_first, y, team, stream=None):
    """y[r] = sum of val * x[jdx - x_first] over row r's entries, in the order contract of ga_amd.h"""
    return lib().gaamd_spmv(op, nrows, nblk, _vp(offs), _vp(start), _vp(jdx), _vp(val), _vp(x), x_first, _vp(y), team,
                            stream)


def sprs_diag(op, fn, nrows, offs, jdx, val, diag_first, out, team, shift=None, stream=None):
    """one column block: GAAMD_DIAG_GET out[r] = the last stored (r, r); GAAMD_DIAG_SHIFT every one += shift"""
    keep, sp = scale_buffer(op, shift) if shift is not None else (None, None)
    return lib().gaamd_sprs_diag(op, fn, nrows, _vp(offs), _vp(jdx), _vp(val), diag_first, _vp(out), sp, team, stream)


def sprs_scale_left(op, nrows, offs, val, d, team, stream=None):
    """one column block: val[k] = d[r] * val[k] for the entries of row r (the true complex product)"""
    return lib().gaamd_sprs_scale_left(op, nrows, _vp(offs), _vp(val), _vp(d), team, stream)


def sprs_scale_right(op, n, jdx, val, d, d_first, stream=None):
    """val[k] = d[jdx[k] - d_first] * val[k], k < n (the true complex product)"""
    return lib().gaamd_sprs_scale_right(op, n, _vp(jdx), _vp(val), _vp(d), d_first, stream)


def spmm(op, nrows, nblk, offs, start, jdx, val, b, ldb, b_first, n, c, ldc, stream=None):
    """c[r][j] = sum of val * b[jdx - b_first][j] over row r's entries, sequentially in list order; j < n"""
    return lib().gaamd_spmm(op, nrows, nblk, _vp(offs), _vp(start), _vp(jdx), _vp(val), _vp(b), ldb, b_first, n, _vp(c),
                            ldc, stream)


def dense_row_counts(op, rows, cols, a, lda, row_first, col_first, counts, stream=None):
    """counts[r] = the elements of row r that are != 0 or on the global diagonal"""
    return lib().gaamd_dense_row_counts(op, rows, cols, _vp(a), lda, row_first, col_first, _vp(counts), stream)


def dense_to_csr(op, rows, cols, a, lda, row_first, col_first, offs, jdx, val, stream=None):
    """the kept elements of row r to jdx (global columns) / val at offs[r], in ascending column order"""
    return lib().gaamd_dense_to_csr(op, rows, cols, _vp(a), lda, row_first, col_first, _vp(offs), _vp(jdx), _vp(val),
                                    stream)


def csr_to_dense(op, nrows, cols, offs, jdx, val, col_first, out, ldo, stream=None):
    """one column block: out[r][jdx - col_first] = val, of duplicates the last; the caller zeroes out"""
    return lib().gaamd_csr_to_dense(op, nrows, cols, _vp(offs), _vp(jdx), _vp(val), col_first, _vp(out), ldo, stream)


def spmm_route_counts():
    """{B in place, B through scratch, C in place, C through scratch} of NGA_Sprs_array_sprsdns_multiply so far"""
    out = (ctypes.c_longlong * 4)()
    lib().gaamd_ga_spmm_route_counts(out)
    return list(out)


# Sparse x sparse at kernel level (gaamd_csr_rows / _spgemm_count / _spgemm_fill): A a block CSR as
# above, B a row CSR -- brows + 1 long long offsets into rjdx / rval, row k being global row b_first + k.
def spgemm_lds_cap():
    """the largest product bound U of a row that takes the LDS hash-set path"""
    return lib().gaamd_spgemm_lds_cap()


def csr_rows(op, nrows, nblk, offs, start, jdx, val, roffs, rjdx, rval, stream=None):
    """the block CSR flattened: roffs (nrows + 1 long long), rjdx, rval with every row's one list contiguous"""
    return lib().gaamd_csr_rows(op, nrows, nblk, _vp(offs), _vp(start), _vp(jdx), _vp(val), _vp(roffs), _vp(rjdx),
                                _vp(rval), stream)


def spgemm_count(nrows, nblk, offs, start, jdx, b_first, brows, roffs, rjdx, jdim_c, ncut, counts, bound, stream=None):
    """counts[b * nrows + r] = the distinct columns of row r of A B in column block b of ncut; bound[r] = its products"""
    return lib().gaamd_spgemm_count(nrows, nblk, _vp(offs), _vp(start), _vp(jdx), b_first, brows, _vp(roffs), _vp(rjdx),
                                    jdim_c, ncut, _vp(counts), _vp(bound), stream)


def spgemm_fill(op, nrows, nblk, offs, start, jdx, val, b_first, brows, roffs, rjdx, rval, jdim_c, ncut, coffs, cstart,
                cjdx, cval, stream=None):
    """cjdx / cval of A B at cstart[b] + coffs[b][r], in the order contract of ga_amd.h"""
    return lib().gaamd_spgemm_fill(op, nrows, nblk, _vp(offs), _vp(start), _vp(jdx), _vp(val), b_first, brows, _vp(roffs),
                                   _vp(rjdx), _vp(rval), jdim_c, ncut, _vp(coffs), _vp(cstart), _vp(cjdx), _vp(cval), stream)


def spgemm_route_counts():
    """{B parts used in place, B parts copied} of NGA_Sprs_array_matmat_multiply so far"""
    out = (ctypes.c_longlong * 2)()
    lib().gaamd_ga_spgemm_route_counts(out)
    return list(out)


def sprs_range(dim, nproc, iproc):
    """(lo, hi) of the indices of a dimension of `dim` that rank iproc of nproc owns (host only)"""
    lo, hi = ctypes.c_long(0), ctypes.c_long(0)
    lib().gaamd_ga_sprs_range(dim, nproc, iproc, ctypes.byref(lo), ctypes.byref(hi))
    return lo.value, hi.value


def patch_add_plan(op, a, a_stride, b, b_stride, c, c_stride, count):
    """gaamd_patch_add's checks without a launch (no GPU): (code, {width, levels, rows, nvec})"""
    out = (ctypes.c_longlong * 4)()
    rc = lib().gaamd_patch_add_plan(op, ctypes.c_void_p(a), ll_array(a_stride), ctypes.c_void_p(b),
                                    ll_array(b_stride), ctypes.c_void_p(c), ll_array(c_stride), ll_array(count),
                                    len(count), out)
    return rc, {"width": out[0], "levels": out[1], "rows": out[2], "nvec": out[3]}


def _trans(t):
    return ord(t) if isinstance(t, (str, bytes)) else int(t)


# row-major GEMM on the matrix cores (gaamd_gemm): a, b, c are device addresses, ld in
# elements; scalars of None reach the library as NULL; the return code is handed back
def gemm(op, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, stream=None):
    ka, ap = scale_buffer(op, alpha) if alpha is not None else (None, None)
    kb, bp = scale_buffer(op, beta) if beta is not None else (None, None)
    return lib().gaamd_gemm(op, _trans(transa), _trans(transb), m, n, k, ap, ctypes.c_void_p(a), lda,
                            ctypes.c_void_p(b), ldb, bp, ctypes.c_void_p(c), ldc, stream)


def gemm_plan(op, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc):
    """gaamd_gemm's checks without a launch (no GPU): (code, {tm, tn, tk, grid_m, grid_n, ksteps})"""
    ka, ap = scale_buffer(op, alpha) if alpha is not None else (None, None)
    kb, bp = scale_buffer(op, beta) if beta is not None else (None, None)
    out = (ctypes.c_longlong * 6)()
    rc = lib().gaamd_gemm_plan(op, _trans(transa), _trans(transb), m, n, k, ap, ctypes.c_void_p(a), lda,
                               ctypes.c_void_p(b), ldb, bp, ctypes.c_void_p(c), ldc, out)
    return rc, {"tm": out[0], "tn": out[1], "tk": out[2], "grid_m": out[3], "grid_n": out[4], "ksteps": out[5]}


# row-major complex GEMM on the matrix cores (gaamd_gemm_cplx): op is COMEX_ACC_DCP or
# COMEX_ACC_CPL, trans one of N T C, alpha and beta Python complex (None reaches the library
# as NULL), ld in complex elements; the return code is handed back
def _cplx_scalar(op, v):
    """one complex element for the `void *` scalar: complex64 for COMEX_ACC_CPL, else complex128"""
    if v is None:
        return None, None
    a = np.array([v], dtype=np.complex64 if op == COMEX_ACC_CPL else np.complex128)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def gemm_cplx(op, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, stream=None):
    al, ap = _cplx_scalar(op, alpha)
    be, bp = _cplx_scalar(op, beta)
    return lib().gaamd_gemm_cplx(op, _trans(transa), _trans(transb), m, n, k, ap, ctypes.c_void_p(a), lda,
                                 ctypes.c_void_p(b), ldb, bp, ctypes.c_void_p(c), ldc, stream)


def gemm_cplx_plan(op, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc):
    """gaamd_gemm_cplx's checks without a launch (no GPU): (code, {tm, tn, tk, grid_m, grid_n, ksteps})"""
    al, ap = _cplx_scalar(op, alpha)
    be, bp = _cplx_scalar(op, beta)
    out = (ctypes.c_longlong * 6)()
    rc = lib().gaamd_gemm_cplx_plan(op, _trans(transa), _trans(transb), m, n, k, ap, ctypes.c_void_p(a), lda,
                                    ctypes.c_void_p(b), ldb, bp, ctypes.c_void_p(c), ldc, out)
    return rc, {"tm": out[0], "tn": out[1], "tk": out[2], "grid_m": out[3], "grid_n": out[4], "ksteps": out[5]}


# row-major transpose through LDS tiles (gaamd_transpose): src, dst are device addresses,
# ld in elements; the return code is handed back
def transpose(op, rows, cols, src, lds, dst, ldd, stream=None):
    return lib().gaamd_transpose(op, rows, cols, ctypes.c_void_p(src), lds, ctypes.c_void_p(dst), ldd, stream)


# c = alpha * (c + b^T) in place (gaamd_transpose_acc): c is m x n, b is n x m; an alpha of
# None reaches the library as NULL
def transpose_acc(op, m, n, alpha, b, ldb, c, ldc, stream=None):
    ka, ap = scale_buffer(op, alpha) if alpha is not None else (None, None)
    return lib().gaamd_transpose_acc(op, m, n, ap, ctypes.c_void_p(b), ldb, ctypes.c_void_p(c), ldc, stream)


def transpose_plan(op, rows, cols, src, lds, dst, ldd):
    """gaamd_transpose's checks without a launch (no GPU): (code, {tile_rows, tile_cols, grid_rows, grid_cols})"""
    out = (ctypes.c_longlong * 4)()
    rc = lib().gaamd_transpose_plan(op, rows, cols, ctypes.c_void_p(src), lds, ctypes.c_void_p(dst), ldd, out)
    return rc, {"tile_rows": out[0], "tile_cols": out[1], "grid_rows": out[2], "grid_cols": out[3]}


def last_launch():
    k, w, u, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    b = ctypes.c_ulonglong()
    lib().gaamd_last_launch(ctypes.byref(k), ctypes.byref(w), ctypes.byref(u), ctypes.byref(n), ctypes.byref(b))
    return {"kind": KIND_NAME.get(k.value, k.value), "width": w.value, "unroll": u.value,
            "launches": n.value, "blocks": b.value}


def plan_strided(op, src, src_stride, dst, dst_stride, count, stride_levels, row_begin=0, row_end=None):
    """The launcher's plan for a strided op (no launch, no GPU): dict or raises on an error code."""
    out = (ctypes.c_longlong * 8)()
    rc = lib().gaamd_plan_strided(op, ctypes.c_void_p(src), int_array(src_stride), ctypes.c_void_p(dst),
                                  int_array(dst_stride), int_array(count), stride_levels, row_begin,
                                  (1 << 64) - 1 if row_end is None else row_end, out)
    if rc:
        raise ValueError(f"plan error {rc}")
    return {"kind": KIND_NAME.get(out[0], out[0]), "width": out[1], "unroll": out[2], "block": out[3],
            "launches": out[4], "blocks": out[5], "levels": out[6], "aligned": bool(out[7])}


def kernel_counts():
    """launches so far by kind (this process): {'rows': n, 'flat': n, 'serial': n, 'ordered': n}"""
    c = (ctypes.c_ulonglong * 5)()
    lib().gaamd_kernel_counts(c)
    return {"rows": c[1], "flat": c[2], "serial": c[3], "ordered": c[4]}


def device_topology():
    """after comex_init: ranks on this rank's GPU (itself included), distinct GPUs among
    this node's ranks, and the peer-load mode (0 auto, 1 all peers as other GPUs, 2 off)"""
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    if lib().gaamd_device_topology(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) != 0:
        return None
    return {"ranks_on_gpu": a.value, "gpus_on_node": b.value,
            "peer_loads": {0: "auto", 1: "all", 2: "off"}.get(c.value, c.value)}


def route_counts():
    """requests this rank posted to same-node owners, by route"""
    c = (ctypes.c_ulonglong * 4)()
    lib().gaamd_route_counts(c)
    return {"packed": c[0], "direct_src": c[1], "iov": c[2], "rmw": c[3], "one_pass": lib().gaamd_one_pass_count()}


def toggle_counts():
    """operations that took the reference's PACKED / IOV / GET_SELF+SMP toggle routes"""
    c = (ctypes.c_ulonglong * 3)()
    lib().gaamd_toggle_counts(c)
    return {"rows": c[0], "pairs": c[1], "owner_gets": c[2]}


def iov_path_counts():
    """local io-vector launches with repeated-destination ordering, by path"""
    c = (ctypes.c_ulonglong * 4)()
    lib().gaamd_iov_path_counts(c)
    return {"hashed": c[0], "hashed_then_radix": c[1], "radix": c[2], "lds": c[3]}


def owner_counts():
    """requests this rank's progress thread applied, by kind"""
    c = (ctypes.c_ulonglong * 4)()
    lib().gaamd_owner_counts(c)
    return {"packed": c[0], "iov": c[1], "rmw": c[2], "direct_src": c[3]}


def set_tuning(key, value):
    return lib().gaamd_set_tuning(key.encode(), int(value))


def get_tuning(key):
    return lib().gaamd_get_tuning(key.encode())


def sync(stream=None):
    rc = lib().gaamd_sync(stream)
    if rc:
        raise RuntimeError(f"device sync failed ({rc})")


def fill(ptr, n, type_code, seed, stream=None):
    rc = lib().gaamd_fill(ctypes.c_void_p(ptr), int(n), int(type_code), int(seed), stream)
    if rc:
        raise RuntimeError("gaamd_fill failed")


# ---- io-vector descriptors (comex.h:13-18, armci.h:17-22) ------------------
def fill_const(ptr, nbytes, value, dtype="float64"):
    """Fill nbytes of device memory at ptr with a constant of an 8-byte dtype (one
    kernel; enqueued on the library's primary stream -- sync() before use)."""
    import numpy as np
    word = int(np.array([value], dtype=dtype).view(np.uint64)[0])
    assert np.dtype(dtype).itemsize == 8 and nbytes % 8 == 0
    if lib().gaamd_fill_word(ctypes.c_void_p(ptr), nbytes // 8, word, None) != 0:
        raise RuntimeError("gaamd_fill_word failed")


class GIOV(ctypes.Structure):
    _fields_ = [("src", ctypes.POINTER(ctypes.c_void_p)), ("dst", ctypes.POINTER(ctypes.c_void_p)),
                ("count", ctypes.c_int), ("bytes", ctypes.c_int)]


def make_giov(descs):
    """descs: list of (src_addrs, dst_addrs, bytes) -> (array of GIOV, keep-alive list)."""
    arr = (GIOV * len(descs))()
    keep = []
    for k, (src, dst, nbytes) in enumerate(descs):
        s = (ctypes.c_void_p * max(1, len(src)))(*src)
        d = (ctypes.c_void_p * max(1, len(dst)))(*dst)
        keep += [s, d]
        arr[k].src = ctypes.cast(s, ctypes.POINTER(ctypes.c_void_p))
        arr[k].dst = ctypes.cast(d, ctypes.POINTER(ctypes.c_void_p))
        arr[k].count = len(src)
        arr[k].bytes = nbytes
    return arr, keep


def comex_accv(op, scale, descs, proc, group=COMEX_GROUP_WORLD):
    keep_s, sp = scale_buffer(op, scale)
    arr, keep = make_giov(descs)
    return lib().comex_accv(op, sp, ctypes.cast(arr, ctypes.c_void_p), len(descs), proc, group)


def comex_putv(descs, proc, group=COMEX_GROUP_WORLD):
    arr, keep = make_giov(descs)
    return lib().comex_putv(ctypes.cast(arr, ctypes.c_void_p), len(descs), proc, group)


def comex_getv(descs, proc, group=COMEX_GROUP_WORLD):
    arr, keep = make_giov(descs)
    return lib().comex_getv(ctypes.cast(arr, ctypes.c_void_p), len(descs), proc, group)


# ---- ComEx API (comex.h) ----------------------------------------------------
def comex_init():
    return lib().comex_init()


def comex_finalize():
    return lib().comex_finalize()


def comex_accs(op, scale, src, src_stride, dst, dst_stride, count, stride_levels, proc,
               group=COMEX_GROUP_WORLD):
    keep, sp = scale_buffer(op, scale)
    return lib().comex_accs(op, sp, ctypes.c_void_p(src), int_array(src_stride), ctypes.c_void_p(dst),
                            int_array(dst_stride), int_array(count), stride_levels, proc, group)


def comex_nbaccs(op, scale, src, src_stride, dst, dst_stride, count, stride_levels, proc,
                 group=COMEX_GROUP_WORLD):
    keep, sp = scale_buffer(op, scale)
    h = ctypes.c_int(-1)
    rc = lib().comex_nbaccs(op, sp, ctypes.c_void_p(src), int_array(src_stride), ctypes.c_void_p(dst),
                            int_array(dst_stride), int_array(count), stride_levels, proc, group, ctypes.byref(h))
    return rc, h


def comex_acc(op, scale, src, dst, nbytes, proc, group=COMEX_GROUP_WORLD):
    keep, sp = scale_buffer(op, scale)
    return lib().comex_acc(op, sp, ctypes.c_void_p(src), ctypes.c_void_p(dst), int(nbytes), proc, group)


def comex_puts(src, src_stride, dst, dst_stride, count, stride_levels, proc, group=COMEX_GROUP_WORLD):
    return lib().comex_puts(ctypes.c_void_p(src), int_array(src_stride), ctypes.c_void_p(dst),
                            int_array(dst_stride), int_array(count), stride_levels, proc, group)


def comex_gets(src, src_stride, dst, dst_stride, count, stride_levels, proc, group=COMEX_GROUP_WORLD):
    return lib().comex_gets(ctypes.c_void_p(src), int_array(src_stride), ctypes.c_void_p(dst),
                            int_array(dst_stride), int_array(count), stride_levels, proc, group)


def comex_wait(h):
    return lib().comex_wait(ctypes.byref(h))


def comex_fence_all(group=COMEX_GROUP_WORLD):
    return lib().comex_fence_all(group)


def comex_barrier(group=COMEX_GROUP_WORLD):
    return lib().comex_barrier(group)


def comex_malloc(nbytes, size, group=COMEX_GROUP_WORLD):
    arr = (ctypes.c_void_p * size)()
    rc = lib().comex_malloc(arr, int(nbytes), group)
    if rc:
        raise RuntimeError("comex_malloc failed")
    return [a or 0 for a in arr]


def comex_free(ptr, group=COMEX_GROUP_WORLD):
    return lib().comex_free(ctypes.c_void_p(ptr), group)
