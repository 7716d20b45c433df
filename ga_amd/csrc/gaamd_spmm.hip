// gaamd_spmm.hip -- sparse x dense and the dense / sparse conversions of GA's sparse arrays
// (ga_amd.h gaamd_spmm, gaamd_dense_row_counts, gaamd_dense_to_csr, gaamd_csr_to_dense; ga.h
// NGA_Sprs_array_sprsdns_multiply, _create_from_dense, _create_from_sparse).  Compiled as part of
// gaamd_all.hip after gaamd_sprs.hip, whose block CSR, SprsEl, sprs_mul, type dispatch and codes
// it shares.
//
// Reference arithmetic (global/src/sparse.array.c), with the departures ga_amd.h states:
//   sprsdns   c[i][j] += a_ik * b[k][j], one product and one add per entry, in the     3517-3840
//             order of the row's one list; complex the true product of sprs_mul
//   from dense   an element is kept when it is != 0 or on the global diagonal          3234, 3263
//   from sparse  out[i][j] = a_ij, of duplicates the last in storage order             3400-3515
// Integers in unsigned arithmetic.  FP contraction is off (gaamd_sprs.hip's pragma holds to the
// end of the translation unit; it is repeated here for the reader).
//
// SPMM: the lanes of a wave run along j.  A row is computed by a group of G = 2^lg lanes, lane L
// holding the V consecutive columns j0 = (tile * G + L) * V ..; 256 / G rows per workgroup, so
// for narrow n one wave takes 64 / G rows.  V * sizeof(element) = 16 bytes where b, c, ldb, ldc
// and n allow (V = 4, 2, 1 for 4-, 8-, 16-byte elements), else V = 1.  G is the smallest power of
// two with G * V >= n, at most 64; wider n is cut into tiles of G * V columns over gridDim.y
// (strided, so any n fits), and the row's jdx / val are read once per tile.  Rows are walked by
// a 64-bit stride loop over gridDim.x.  Every lane walks the row's list itself, entry by entry
// from +0: acc = acc + a * b[jdx][j].  The lanes of a group obtain val[k] and jdx[k] by the
// SAME-ADDRESS LOAD: each issues the load of the one address, which the memory pipeline serves
// as one request per wave and row; there is no cross-lane step at all, hence no uniformity
// requirement, no LDS and no bpermute.  The loop is unrolled by four so that the four B rows
// are in flight together; the adds stay in list order.
// DENSE -> CSR: one wave per row, rows strided over the grid; a row is walked in runs of 64
// consecutive columns; a ballot of the kept lanes gives the run's count (popcount) and each
// kept lane's place (popcount of the lanes below it).  gaamd_dense_row_counts stores the row's
// count; gaamd_dense_to_csr, given the exclusive prefix sums, stores jdx / val at offs[r] + place.
// CSR -> DENSE: a team of 16 lanes per row; an entry whose successor in the row names the same
// column is skipped, so of duplicates the last is stored and no two lanes write one address.
// No atomics, no LDS, no scratch; every index into every array is 64-bit.
// Resources (hipcc -O3, gfx950; VGPRs, all with 0 bytes of scratch and of LDS):
//   k_spmm V = 1: int 67, long 48, float 43, double 48, complex float 48, complex double 62
//   k_spmm 16-byte: int x4 74, float x4 46, long x2 50, double x2 50, complex float x2 66
//   (occupancy 8 waves per SIMD, 7 for int and complex float x2, 6 for int x4)
//   k_dense_rows: counts 12 to 14, store 22 to 28;  k_csr_to_dense: 16 to 20
#pragma clang fp contract(off)

namespace gaamd {

struct SpmmDesc {
    const int32_t *offs;    // [nblk][nrows + 1]
    const int64_t *start;   // [nblk]
    const int32_t *jdx;
    const char *val;
    const char *b;
    char *c;
    int64_t b_first;        // the global row of b[0]
    int64_t ldb, ldc;       // elements between rows
    uint64_t nrows, n;
    int32_t nblk, lg;
};

template <typename T, int NP, int V>
struct alignas(sizeof(T) * NP * V) SpmmVec {
    SprsEl<T, NP> e[V];
};

template <typename T, int NP, int V>
__global__ __launch_bounds__(kSprsBS) void k_spmm(const SpmmDesc d) {
    typedef SprsEl<T, NP> E;
    typedef SpmmVec<T, NP, V> Vec;
    const uint32_t G = 1u << d.lg, lane = threadIdx.x & (G - 1);
    const uint64_t per = (uint64_t)(kSprsBS >> d.lg), step = (uint64_t)gridDim.x * per;
    const uint64_t tilew = (uint64_t)G * V, ntile = (d.n + tilew - 1) / tilew;
    const E *val = reinterpret_cast<const E *>(d.val), *B = reinterpret_cast<const E *>(d.b);
    E *C = reinterpret_cast<E *>(d.c);
    for (uint64_t tile = blockIdx.y; tile < ntile; tile += gridDim.y) {
        const uint64_t j0 = tile * tilew + (uint64_t)lane * V;
        if (j0 >= d.n) continue;   // 16-byte path: n is a multiple of V, the whole vector lies inside
        for (uint64_t row = (uint64_t)blockIdx.x * per + (threadIdx.x >> d.lg); row < d.nrows; row += step) {
            Vec acc = {};
            for (int32_t b = 0; b < d.nblk; ++b) {
                const int32_t *o = d.offs + (int64_t)b * (int64_t)(d.nrows + 1) + (int64_t)row;
                const uint32_t o0 = (uint32_t)o[0], c = (uint32_t)o[1] - o0;
                const int64_t k0 = d.start[b] + (int64_t)o0;
#pragma unroll 4
                for (uint32_t t = 0; t < c; ++t) {
                    const int64_t k = k0 + (int64_t)t;
                    const E a = val[k];
                    const Vec bv = *reinterpret_cast<const Vec *>(B + ((int64_t)d.jdx[k] - d.b_first) * d.ldb + (int64_t)j0);
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        const E p = sprs_mul<T, NP>(a, bv.e[v]);
#pragma unroll
                        for (int i = 0; i < NP; ++i) acc.e[v].t[i] = acc.e[v].t[i] + p.t[i];
                    }
                }
            }
            *reinterpret_cast<Vec *>(C + (int64_t)row * d.ldc + (int64_t)j0) = acc;
        }
    }
}

constexpr long long kSpmmMaxN = (1ll << 31) - 1;

static bool span_hit(const void *a, uint64_t abytes, const void *b, uint64_t bbytes) {
    const uint64_t alo = (uint64_t)(uintptr_t)a, blo = (uint64_t)(uintptr_t)b;
    return alo < blo + bbytes && blo < alo + abytes;
}

// the bytes of a row-major rows x cols matrix with ld elements between rows
static uint64_t dense_span(long long rows, long long cols, long long ld, int esz) {
    return ((uint64_t)(rows - 1) * (uint64_t)ld + (uint64_t)cols) * (uint64_t)esz;
}

int launch_spmm(int op, long long nrows, int nblk, const int *offs, const long long *start, const int *jdx,
                const void *val, const void *b, long long ldb, long long b_first, long long n, void *c, long long ldc,
                hipStream_t stream) {
    if (nrows < 0 || nblk < 0 || n < 0) return kPatchErrCount;
    const int esz = (op == kOpCopy) ? 0 : elem_size(op);
    if (!esz) return kPatchErrOp;
    if (nrows == 0 || n == 0) return 0;
    if (!c || (nblk > 0 && (!offs || !start || !jdx || !val || !b))) return kPatchErrScalar;
    if (ldc < n || (nblk > 0 && ldb < n)) return kPatchErrStride;
    if (nrows > kSprsMaxRows || n > kSpmmMaxN) return kPatchErrRange;
    const uintptr_t bb = nblk > 0 ? (uintptr_t)b : 0;
    if ((((uintptr_t)c | (uintptr_t)val | bb) & (uintptr_t)(esz - 1)) || ((uintptr_t)start & 7) ||
        (((uintptr_t)offs | (uintptr_t)jdx) & 3))
        return kPatchErrAlign;
    // how many rows of b the entries name is not an argument: its first row stands for it
    if (nblk > 0 && span_hit(c, dense_span(nrows, n, ldc, esz), b, (uint64_t)n * esz)) return kPatchErrOverlap;
    SpmmDesc d;
    memset(&d, 0, sizeof(d));
    d.offs = offs;
    d.start = reinterpret_cast<const int64_t *>(start);
    d.jdx = jdx;
    d.val = (const char *)val;
    d.b = (const char *)b;
    d.c = (char *)c;
    d.b_first = b_first;
    d.ldb = ldb;
    d.ldc = ldc;
    d.nrows = (uint64_t)nrows;
    d.n = (uint64_t)n;
    d.nblk = nblk;
    const int vw = 16 / esz;
    const bool wide = vw > 1 && n % vw == 0 && ldc % vw == 0 && !((uintptr_t)c & 15) &&
                      (nblk == 0 || (ldb % vw == 0 && !((uintptr_t)b & 15)));
    const uint64_t need = ((uint64_t)n + (wide ? vw : 1) - 1) / (wide ? vw : 1);
    while (d.lg < 6 && (1ull << d.lg) < need) d.lg++;
    const uint64_t tilew = (1ull << d.lg) * (wide ? vw : 1), ntile = ((uint64_t)n + tilew - 1) / tilew;
    const dim3 grid(sprs_grid(d.nrows, d.lg), (unsigned)(ntile < 65535 ? ntile : 65535));
    return rc_of(for_type(op, [&](auto t) {
        typedef decltype(t) T;
        constexpr int VW = 16 / T::elem;
        if constexpr (VW > 1) {
            if (wide) {
                hipLaunchKernelGGL((k_spmm<typename T::real, T::parts, VW>), grid, dim3(kSprsBS), 0, stream, d);
                return hipGetLastError();
            }
        }
        hipLaunchKernelGGL((k_spmm<typename T::real, T::parts, 1>), grid, dim3(kSprsBS), 0, stream, d);
        return hipGetLastError();
    }));
}

// ---------------------------------------------------------------------------
struct DenseCsrDesc {
    const char *a;
    const int32_t *offs;   // store: the rows + 1 exclusive prefix sums
    int32_t *counts;       // counts: written
    int32_t *jdx;
    char *val;
    int64_t lda, row_first, col_first;
    uint64_t rows, cols;
};

template <typename T, int NP>
__device__ __forceinline__ bool sprs_nonzero(const SprsEl<T, NP> e) {
    bool nz = false;
#pragma unroll
    for (int i = 0; i < NP; ++i) nz = nz || (e.t[i] != (T)0);   // -0.0 is not, a NaN is
    return nz;
}

template <typename T, int NP, bool STORE>
__global__ __launch_bounds__(kSprsBS) void k_dense_rows(const DenseCsrDesc d) {
    typedef SprsEl<T, NP> E;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t per = kSprsBS / 64, step = (uint64_t)gridDim.x * per;
    const E *A = reinterpret_cast<const E *>(d.a);
    for (uint64_t row = (uint64_t)blockIdx.x * per + (threadIdx.x >> 6); row < d.rows; row += step) {   // per wave
        const E *ar = A + (int64_t)row * d.lda;
        const int64_t dcol = d.row_first + (int64_t)row - d.col_first;   // the local column on the diagonal
        int64_t at = STORE ? (int64_t)d.offs[row] : 0;
        uint32_t total = 0;
        for (uint64_t c0 = 0; c0 < d.cols; c0 += 64) {   // uniform over the wave
            const uint64_t col = c0 + lane;
            E e = {};
            bool keep = false;
            if (col < d.cols) {
                e = ar[col];
                keep = sprs_nonzero<T, NP>(e) || (int64_t)col == dcol;
            }
            const uint64_t m = __ballot(keep);
            if (STORE && keep) {
                const int64_t k = at + (int64_t)__popcll(m & ((1ull << lane) - 1ull));
                d.jdx[k] = (int32_t)(d.col_first + (int64_t)col);
                reinterpret_cast<E *>(d.val)[k] = e;
            }
            const uint32_t cnt = (uint32_t)__popcll(m);
            at += cnt;
            total += cnt;
        }
        if (!STORE && lane == 0) d.counts[row] = (int32_t)total;
    }
}

static unsigned dense_grid(uint64_t rows) {
    const uint64_t nb = (rows + kSprsBS / 64 - 1) / (kSprsBS / 64);
    return (unsigned)(nb < kSprsMaxGrid ? nb : kSprsMaxGrid);
}

// counts != nullptr: the counting pass; else the storing pass
int launch_dense_csr(int op, long long rows, long long cols, const void *a, long long lda, long long row_first,
                     long long col_first, int *counts, const int *offs, int *jdx, void *val, bool store,
                     hipStream_t stream) {
    if (rows < 0 || cols < 0) return kPatchErrCount;
    const int esz = (op == kOpCopy) ? 0 : elem_size(op);
    if (!esz) return kPatchErrOp;
    if (rows == 0 || cols == 0) return 0;
    if (!a || (store ? (!offs || !jdx || !val) : !counts)) return kPatchErrScalar;
    if (lda < cols) return kPatchErrStride;
    // jdx holds global columns in an int
    if (rows > kSprsMaxRows || col_first < 0 || row_first < 0 || col_first > kSpmmMaxN + 1 - cols) return kPatchErrRange;
    if ((((uintptr_t)a | (uintptr_t)val) & (uintptr_t)(esz - 1)) ||
        (((uintptr_t)counts | (uintptr_t)offs | (uintptr_t)jdx) & 3))
        return kPatchErrAlign;
    const uint64_t ab = dense_span(rows, cols, lda, esz);
    // the length of jdx / val is offs[rows], which lies in HBM: their first element stands for them
    if (store ? (span_hit(jdx, 4, a, ab) || span_hit(val, (uint64_t)esz, a, ab)) : span_hit(counts, (uint64_t)rows * 4, a, ab))
        return kPatchErrOverlap;
    DenseCsrDesc d;
    memset(&d, 0, sizeof(d));
    d.a = (const char *)a;
    d.offs = offs;
    d.counts = counts;
    d.jdx = jdx;
    d.val = (char *)val;
    d.lda = lda;
    d.row_first = row_first;
    d.col_first = col_first;
    d.rows = (uint64_t)rows;
    d.cols = (uint64_t)cols;
    return rc_of(for_type(op, [&](auto t) {
        typedef decltype(t) T;
        if (store)
            hipLaunchKernelGGL((k_dense_rows<typename T::real, T::parts, true>), dim3(dense_grid(d.rows)), dim3(kSprsBS), 0,
                               stream, d);
        else
            hipLaunchKernelGGL((k_dense_rows<typename T::real, T::parts, false>), dim3(dense_grid(d.rows)), dim3(kSprsBS), 0,
                               stream, d);
        return hipGetLastError();
    }));
}

// ---------------------------------------------------------------------------
struct CsrDenseDesc {
    const int32_t *offs;
    const int32_t *jdx;
    const char *val;
    char *out;
    int64_t col_first, ldo;
    uint64_t nrows, cols;
};

constexpr int kCsrDenseLg = 4;   // a team of 16 lanes per row

template <typename T, int NP>
__global__ __launch_bounds__(kSprsBS) void k_csr_to_dense(const CsrDenseDesc d) {
    typedef SprsEl<T, NP> E;
    const uint32_t W = 1u << kCsrDenseLg, lane = threadIdx.x & (W - 1);
    const uint64_t per = (uint64_t)(kSprsBS >> kCsrDenseLg), step = (uint64_t)gridDim.x * per;
    const E *val = reinterpret_cast<const E *>(d.val);
    E *out = reinterpret_cast<E *>(d.out);
    for (uint64_t row = (uint64_t)blockIdx.x * per + (threadIdx.x >> kCsrDenseLg); row < d.nrows; row += step) {
        const uint32_t o0 = (uint32_t)d.offs[row], c = (uint32_t)d.offs[row + 1] - o0;
        for (uint32_t t = lane; t < c; t += W) {
            const int64_t k = (int64_t)o0 + t;
            const int32_t j = d.jdx[k];
            if (t + 1 < c && d.jdx[k + 1] == j) continue;   // a later duplicate wins
            const int64_t col = (int64_t)j - d.col_first;
            if (col < 0 || (uint64_t)col >= d.cols) continue;   // outside the window of `out`: not stored
            out[(int64_t)row * d.ldo + col] = val[k];
        }
    }
}

int launch_csr_to_dense(int op, long long nrows, long long cols, const int *offs, const int *jdx, const void *val,
                        long long col_first, void *out, long long ldo, hipStream_t stream) {
    if (nrows < 0 || cols < 0) return kPatchErrCount;
    const int esz = (op == kOpCopy) ? 0 : elem_size(op);
    if (!esz) return kPatchErrOp;
    if (nrows == 0 || cols == 0) return 0;
    if (!offs || !jdx || !val || !out) return kPatchErrScalar;
    if (ldo < cols) return kPatchErrStride;
    if (nrows > kSprsMaxRows || cols > kSpmmMaxN) return kPatchErrRange;
    if ((((uintptr_t)val | (uintptr_t)out) & (uintptr_t)(esz - 1)) || (((uintptr_t)offs | (uintptr_t)jdx) & 3))
        return kPatchErrAlign;
    const uint64_t ob = dense_span(nrows, cols, ldo, esz);
    if (span_hit(out, ob, offs, (uint64_t)(nrows + 1) * 4) || span_hit(out, ob, jdx, 4) || span_hit(out, ob, val, (uint64_t)esz))
        return kPatchErrOverlap;
    CsrDenseDesc d;
    memset(&d, 0, sizeof(d));
    d.offs = offs;
    d.jdx = jdx;
    d.val = (const char *)val;
    d.out = (char *)out;
    d.col_first = col_first;
    d.ldo = ldo;
    d.nrows = (uint64_t)nrows;
    d.cols = (uint64_t)cols;
    return rc_of(for_type(op, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((k_csr_to_dense<typename T::real, T::parts>), dim3(sprs_grid(d.nrows, kCsrDenseLg)), dim3(kSprsBS),
                           0, stream, d);
        return hipGetLastError();
    }));
}

}  // namespace gaamd
