// gaamd_spgemm.hip -- sparse x sparse of GA's sparse arrays (ga_amd.h gaamd_csr_rows, gaamd_spgemm_count,
// gaamd_spgemm_fill, gaamd_spgemm_lds_cap; ga.h NGA_Sprs_array_matmat_multiply).  Compiled as part of
// gaamd_all.hip after gaamd_spmm.hip, whose SprsEl, sprs_mul, span_hit, type dispatch and codes it shares.
//
// Reference arithmetic (global/src/sparse.array.c:2424-3103): C = A B row by row (Gustavson); an entry
// (i, j) exists where some k has a stored a_ik and a stored b_kj, whatever the values; c_ij takes one
// product and one add per contributing pair.  The departure ga_amd.h states: c_ij starts from +0, where
// the reference assigns the first product.  Integers in unsigned arithmetic.  FP contraction is off.
//
// ROW CSR: B travels as nrows + 1 64-bit offsets plus jdx / val with every row's ONE list (the blocks
// ascending) contiguous; as the blocks ascend with the columns, a row is in ascending column order and
// duplicates of one (k, j) lie side by side in storage order.  k_csr_row_len stores the row lengths,
// k_scan_i64 (one workgroup of 1024) turns them into offsets, k_csr_row_copy copies with a team of 16
// lanes per row.
// COUNT and FILL: one workgroup of ONE wave per row, rows strided over the grid, so every barrier is a
// wave's own and costs a wait only.  The wave first sums the row's product bound U = sum len(B row k),
// lanes along A's entries.
//   U <= kSpgCap (the LDS path): the lanes run along B's row k, A's entries one after the other, and
//   insert the columns into an LDS hash set of 2 * kSpgCap slots (integer compare-and-swap on the key,
//   linear probing; at most half full).  The set is compacted in place with a ballot, padded to a power
//   of two and bitonic-sorted ascending.  The cuts of C's column blocks are found in it by binary search:
//   COUNT stores the differences; FILL stores jdx, val = +0 and, in the upper half of the LDS array, the
//   final place of every column.
//   U > kSpgCap (the fallback): C's column blocks are taken one after the other in windows of kSpgWin
//   columns; a window's columns are marked in an LDS bitmap (integer or), a prefix count per word gives
//   every set bit its rank, so the window is sorted as it stands.  The row's products are walked once
//   per window.  No HBM scratch; same bits, not fast.
//   FILL then walks A's row list sequentially (uniform over the wave) with the lanes along B's row k.  A
//   lane whose predecessor in B's row names the same column does nothing; the others are the heads of
//   their runs: a head finds its column's place (binary search in the sorted list, or the bitmap rank)
//   and does val[p] = val[p] + a * b for the members of its run in order, as plain loads and stores.
//   So a place has one writer per A entry, and the wave's barrier between A entries gives program order.
// No floating-point atomics.  Every index into every array is 64-bit.
// Resources (hipcc -O3, gfx950): 8 KiB of LDS per workgroup of 64, which sets the occupancy: 5 waves per
// SIMD, 20 per CU; k_spgemm_count 55 VGPRs; k_spgemm_fill 51 (int) to 64 (complex double); k_csr_row_len 14,
// k_csr_row_copy 20 to 24; k_scan_i64 16 and 8 KiB of LDS; no kernel of this file uses scratch memory.
#pragma clang fp contract(off)

namespace gaamd {

constexpr int kSpgBS = 64;                          // one wave
constexpr int kSpgLog = 11;
constexpr int kSpgSlots = 1 << kSpgLog;             // of the hash set: 8 KiB
constexpr int kSpgCap = kSpgSlots / 2;              // the largest U of the LDS path
constexpr int kSpgWinWords = kSpgSlots / 2;         // the fallback's bitmap; the other half its prefix counts
constexpr int64_t kSpgWin = (int64_t)kSpgWinWords * 32;
constexpr uint32_t kSpgMaxGrid = 20480;             // 256 CUs x 20 resident waves x 4

int spgemm_lds_cap() { return kSpgCap; }

struct SpgDesc {
    const int32_t *offs;     // A: [nblk][nrows + 1]
    const int64_t *start;
    const int32_t *jdx;
    const char *val;
    const int64_t *roffs;    // B: the row CSR of the global rows b_first ..
    const int32_t *rjdx;
    const char *rval;
    int32_t *counts;         // count: [ncut][nrows]
    int64_t *bound;          // count: U[nrows]
    const int32_t *coffs;    // fill: [ncut][nrows + 1]
    const int64_t *cstart;   // fill: [ncut]
    int32_t *cjdx;
    char *cval;
    int64_t b_first, jdim_c;
    uint64_t nrows;
    int32_t nblk, ncut;
};

// the first column of C's column block b (sprs_build.hpp range)
__device__ __forceinline__ int64_t spg_cut(int64_t b, int64_t jdim, int64_t ncut) {
    return b >= ncut ? jdim : (b * jdim + ncut - 1) / ncut;
}

// f(place of the A entry, first entry of B's row, its length) for the entries of A's row in list order; uniform
template <typename F>
__device__ __forceinline__ void spg_walk(const SpgDesc &d, uint64_t row, F f) {
    for (int32_t b = 0; b < d.nblk; ++b) {
        const int32_t *o = d.offs + (int64_t)b * (int64_t)(d.nrows + 1) + (int64_t)row;
        const uint32_t o0 = (uint32_t)o[0], c = (uint32_t)o[1] - o0;
        const int64_t k0 = d.start[b] + (int64_t)o0;
        for (uint32_t t = 0; t < c; ++t) {
            const int64_t k = (int64_t)d.jdx[k0 + (int64_t)t] - d.b_first;
            const int64_t rs = d.roffs[k];
            f(k0 + (int64_t)t, rs, (uint32_t)(d.roffs[k + 1] - rs));
        }
    }
}

// U of the row, the same on every lane
__device__ __forceinline__ int64_t spg_bound(const SpgDesc &d, uint64_t row, uint32_t lane) {
    int64_t u = 0;
    for (int32_t b = 0; b < d.nblk; ++b) {
        const int32_t *o = d.offs + (int64_t)b * (int64_t)(d.nrows + 1) + (int64_t)row;
        const uint32_t o0 = (uint32_t)o[0], c = (uint32_t)o[1] - o0;
        const int64_t k0 = d.start[b] + (int64_t)o0;
        for (uint32_t t = lane; t < c; t += 64) {
            const int64_t k = (int64_t)d.jdx[k0 + (int64_t)t] - d.b_first;
            u += d.roffs[k + 1] - d.roffs[k];
        }
    }
    for (int s = 32; s > 0; s >>= 1) u += __shfl_xor(u, s, 64);
    return u;
}

// the first index of the ascending list[0 .. n) whose element is >= key
__device__ __forceinline__ int32_t spg_lower(const int32_t *list, int32_t n, int64_t key) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if ((int64_t)list[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// LDS path: tbl[0 .. D) = the distinct columns of the row's products, ascending; returns D <= kSpgCap
__device__ __forceinline__ int32_t spg_row_set(const SpgDesc &d, uint64_t row, uint32_t lane, int32_t *tbl) {
    __syncthreads();   // the row before is done with tbl
    for (uint32_t i = lane; i < (uint32_t)kSpgSlots; i += 64) tbl[i] = -1;
    __syncthreads();
    spg_walk(d, row, [&](int64_t, int64_t rs, uint32_t len) {
        for (uint32_t t = lane; t < len; t += 64) {
            const int32_t col = d.rjdx[rs + (int64_t)t];
            uint32_t s = ((uint32_t)col * 2654435761u) >> (32 - kSpgLog);
            for (;;) {
                const int32_t old = atomicCAS(tbl + s, -1, col);
                if (old == -1 || old == col) break;
                s = (s + 1) & (uint32_t)(kSpgSlots - 1);
            }
        }
    });
    __syncthreads();
    // compact in place: a chunk's survivors go to places at or below their own, all read before any is written
    int32_t D = 0;
    for (uint32_t base = 0; base < (uint32_t)kSpgSlots; base += 64) {
        const int32_t v = tbl[base + lane];
        const uint64_t m = __ballot(v != -1);
        __syncthreads();
        if (v != -1) tbl[D + __popcll(m & ((1ull << lane) - 1ull))] = v;
        D += __popcll(m);
        __syncthreads();
    }
    uint32_t P = 64;
    while (P < (uint32_t)D) P <<= 1;
    for (uint32_t i = (uint32_t)D + lane; i < P; i += 64) tbl[i] = INT32_MAX;   // no column: jdim_c <= 2^31 - 1
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = lane; i < P; i += 64) {
                const uint32_t x = i ^ j;
                if (x > i) {
                    const int32_t a = tbl[i], b = tbl[x];
                    if ((a > b) == ((i & k) == 0)) {
                        tbl[i] = b;
                        tbl[x] = a;
                    }
                }
            }
            __syncthreads();
        }
    return D;
}

// fallback: the distinct columns of the row's products inside [w0, w1), w1 - w0 <= kSpgWin: bit c - w0 of the
// bitmap tbl[0 .. kSpgWinWords), and in tbl[kSpgWinWords ..) the set bits before each word; returns their count
__device__ __forceinline__ int32_t spg_row_window(const SpgDesc &d, uint64_t row, uint32_t lane, int32_t *tbl, int64_t w0,
                                                  int64_t w1) {
    uint32_t *bm = reinterpret_cast<uint32_t *>(tbl), *pre = bm + kSpgWinWords;
    __syncthreads();   // the window before is done with tbl
    for (uint32_t i = lane; i < (uint32_t)kSpgWinWords; i += 64) bm[i] = 0;
    __syncthreads();
    spg_walk(d, row, [&](int64_t, int64_t rs, uint32_t len) {
        for (uint32_t t = lane; t < len; t += 64) {
            const int64_t col = (int64_t)d.rjdx[rs + (int64_t)t];
            if (col >= w0 && col < w1) {
                const uint32_t c = (uint32_t)(col - w0);
                atomicOr(bm + (c >> 5), 1u << (c & 31u));
            }
        }
    });
    __syncthreads();
    constexpr uint32_t per = kSpgWinWords / 64;   // consecutive words of a lane
    uint32_t sum = 0;
    for (uint32_t q = 0; q < per; ++q) sum += (uint32_t)__popc(bm[lane * per + q]);
    uint32_t incl = sum;
    for (uint32_t s = 1; s < 64; s <<= 1) {
        const uint32_t o = __shfl_up(incl, s, 64);
        if (lane >= s) incl += o;
    }
    uint32_t run = incl - sum;
    for (uint32_t q = 0; q < per; ++q) {
        pre[lane * per + q] = run;
        run += (uint32_t)__popc(bm[lane * per + q]);
    }
    const int32_t total = (int32_t)__shfl(incl, 63, 64);
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(kSpgBS) void k_spgemm_count(const SpgDesc d) {
    __shared__ int32_t tbl[kSpgSlots];
    const uint32_t lane = threadIdx.x;
    for (uint64_t row = blockIdx.x; row < d.nrows; row += gridDim.x) {   // uniform
        const int64_t U = spg_bound(d, row, lane);
        if (lane == 0) d.bound[row] = U;
        if (U == 0) {
            for (int32_t b = (int32_t)lane; b < d.ncut; b += 64) d.counts[(int64_t)b * (int64_t)d.nrows + (int64_t)row] = 0;
        } else if (U <= (int64_t)kSpgCap) {
            const int32_t D = spg_row_set(d, row, lane, tbl);
            for (int32_t b = (int32_t)lane; b < d.ncut; b += 64) {
                const int32_t lo = spg_lower(tbl, D, spg_cut(b, d.jdim_c, d.ncut));
                const int32_t hi = spg_lower(tbl, D, spg_cut((int64_t)b + 1, d.jdim_c, d.ncut));
                d.counts[(int64_t)b * (int64_t)d.nrows + (int64_t)row] = hi - lo;
            }
        } else {
            for (int32_t b = 0; b < d.ncut; ++b) {
                const int64_t c0 = spg_cut(b, d.jdim_c, d.ncut), c1 = spg_cut((int64_t)b + 1, d.jdim_c, d.ncut);
                int32_t n = 0;
                for (int64_t w0 = c0; w0 < c1; w0 += kSpgWin)
                    n += spg_row_window(d, row, lane, tbl, w0, w0 + kSpgWin < c1 ? w0 + kSpgWin : c1);
                if (lane == 0) d.counts[(int64_t)b * (int64_t)d.nrows + (int64_t)row] = n;
            }
        }
    }
}

// the products of the row, A's entries one after the other: the head of every run of one column in B's row
// adds the run's products, in order, onto the value at place_of(column); place_of < 0: not now
template <typename T, int NP, typename F>
__device__ __forceinline__ void spg_add_products(const SpgDesc &d, uint64_t row, uint32_t lane, F place_of) {
    typedef SprsEl<T, NP> E;
    const E *aval = reinterpret_cast<const E *>(d.val), *bval = reinterpret_cast<const E *>(d.rval);
    E *cval = reinterpret_cast<E *>(d.cval);
    spg_walk(d, row, [&](int64_t ka, int64_t rs, uint32_t len) {
        const E a = aval[ka];
        for (uint32_t t0 = 0; t0 < len; t0 += 64) {   // uniform
            const uint32_t t = t0 + lane;
            if (t < len) {
                const int32_t col = d.rjdx[rs + (int64_t)t];
                if (t == 0 || d.rjdx[rs + (int64_t)t - 1] != col) {
                    const int64_t p = place_of(col);
                    if (p >= 0) {
                        E acc = cval[p];
                        for (uint32_t u = t; u < len && d.rjdx[rs + (int64_t)u] == col; ++u) {
                            const E pr = sprs_mul<T, NP>(a, bval[rs + (int64_t)u]);
#pragma unroll
                            for (int i = 0; i < NP; ++i) acc.t[i] = acc.t[i] + pr.t[i];
                        }
                        cval[p] = acc;
                    }
                }
            }
            __syncthreads();   // the next A entry, or chunk, may name the same place
        }
    });
}

template <typename T, int NP>
__global__ __launch_bounds__(kSpgBS) void k_spgemm_fill(const SpgDesc d) {
    typedef SprsEl<T, NP> E;
    __shared__ int32_t tbl[kSpgSlots];
    const uint32_t lane = threadIdx.x;
    E *cval = reinterpret_cast<E *>(d.cval);
    for (uint64_t row = blockIdx.x; row < d.nrows; row += gridDim.x) {   // uniform
        const int64_t U = spg_bound(d, row, lane);
        if (U == 0) continue;
        if (U <= (int64_t)kSpgCap) {
            const int32_t D = spg_row_set(d, row, lane, tbl);
            int32_t *place = tbl + kSpgCap;   // D <= kSpgCap: the sorted list ends below
            for (int32_t b = 0; b < d.ncut; ++b) {
                const int32_t lo = spg_lower(tbl, D, spg_cut(b, d.jdim_c, d.ncut));
                const int32_t hi = spg_lower(tbl, D, spg_cut((int64_t)b + 1, d.jdim_c, d.ncut));
                const int64_t base = d.cstart[b] + (int64_t)d.coffs[(int64_t)b * (int64_t)(d.nrows + 1) + (int64_t)row];
                for (int32_t i = lo + (int32_t)lane; i < hi; i += 64) {
                    const int64_t p = base + (int64_t)(i - lo);
                    place[i] = (int32_t)p;   // below 2^31: ga_amd.h
                    d.cjdx[p] = tbl[i];
                    cval[p] = E{};
                }
            }
            __syncthreads();
            spg_add_products<T, NP>(d, row, lane, [&](int32_t col) { return (int64_t)place[spg_lower(tbl, D, col)]; });
        } else {
            const uint32_t *bm = reinterpret_cast<const uint32_t *>(tbl), *pre = bm + kSpgWinWords;
            for (int32_t b = 0; b < d.ncut; ++b) {
                const int64_t c0 = spg_cut(b, d.jdim_c, d.ncut), c1 = spg_cut((int64_t)b + 1, d.jdim_c, d.ncut);
                int64_t base = d.cstart[b] + (int64_t)d.coffs[(int64_t)b * (int64_t)(d.nrows + 1) + (int64_t)row];
                for (int64_t w0 = c0; w0 < c1; w0 += kSpgWin) {
                    const int64_t w1 = w0 + kSpgWin < c1 ? w0 + kSpgWin : c1;
                    const int32_t n = spg_row_window(d, row, lane, tbl, w0, w1);
                    if (n == 0) continue;   // uniform
                    for (uint32_t w = lane; w < (uint32_t)kSpgWinWords; w += 64) {
                        uint32_t bits = bm[w];
                        int64_t p = base + (int64_t)pre[w];
                        while (bits) {
                            d.cjdx[p] = (int32_t)(w0 + (int64_t)w * 32 + (int64_t)(__ffs(bits) - 1));
                            cval[p] = E{};
                            bits &= bits - 1;
                            ++p;
                        }
                    }
                    __syncthreads();
                    spg_add_products<T, NP>(d, row, lane, [&](int32_t col) -> int64_t {
                        if ((int64_t)col < w0 || (int64_t)col >= w1) return -1;
                        const uint32_t c = (uint32_t)((int64_t)col - w0);
                        return base + (int64_t)(pre[c >> 5] + (uint32_t)__popc(bm[c >> 5] & ((1u << (c & 31u)) - 1u)));
                    });
                    base += n;
                }
            }
        }
    }
}

static unsigned spg_grid(uint64_t nrows) { return (unsigned)(nrows < kSpgMaxGrid ? nrows : kSpgMaxGrid); }

// the checks count and fill share; fill: coffs != nullptr or cjdx != nullptr ...
static int spg_check(bool fill, int esz, long long nrows, int nblk, const int *offs, const long long *start, const int *jdx,
                     const void *val, long long b_first, long long brows, const long long *roffs, const int *rjdx,
                     const void *rval, long long jdim_c, int ncut, const void *out1, uint64_t out1_bytes, const void *out2,
                     uint64_t out2_bytes, const int *coffs, const long long *cstart) {
    if (!out1 || !out2 || (fill && (!coffs || !cstart))) return kPatchErrScalar;
    if (nblk > 0 && (!offs || !start || !jdx || !roffs || !rjdx || (fill && (!val || !rval)))) return kPatchErrScalar;
    if (nrows > kSprsMaxRows || brows > kSprsMaxRows || jdim_c > kSpmmMaxN || jdim_c < 1 || b_first < 0)
        return kPatchErrRange;
    if ((((uintptr_t)start | (uintptr_t)roffs | (uintptr_t)cstart) & 7) ||
        (((uintptr_t)offs | (uintptr_t)jdx | (uintptr_t)rjdx | (uintptr_t)coffs) & 3))
        return kPatchErrAlign;
    if (fill && (((uintptr_t)val | (uintptr_t)rval | (uintptr_t)out2) & (uintptr_t)(esz - 1))) return kPatchErrAlign;
    if (((uintptr_t)out1 & 3) || (!fill && ((uintptr_t)out2 & 7))) return kPatchErrAlign;
    // the lengths of jdx / val, rjdx / rval are no arguments: their first entry stands for them
    const struct { const void *p; uint64_t n; } in[] = {
        {offs, (uint64_t)nblk * (uint64_t)(nrows + 1) * 4}, {start, (uint64_t)nblk * 8}, {jdx, 4}, {val, (uint64_t)esz},
        {roffs, (uint64_t)(brows + 1) * 8}, {rjdx, 4}, {rval, (uint64_t)esz},
        {coffs, (uint64_t)ncut * (uint64_t)(nrows + 1) * 4}, {cstart, (uint64_t)ncut * 8}};
    for (const auto &s : in)
        if (s.p && nblk > 0 && (span_hit(out1, out1_bytes, s.p, s.n) || span_hit(out2, out2_bytes, s.p, s.n)))
            return kPatchErrOverlap;
    return 0;
}

static void spg_desc(SpgDesc &d, long long nrows, int nblk, const int *offs, const long long *start, const int *jdx,
                     const void *val, long long b_first, const long long *roffs, const int *rjdx, const void *rval,
                     long long jdim_c, int ncut) {
    memset(&d, 0, sizeof(d));
    d.offs = offs;
    d.start = reinterpret_cast<const int64_t *>(start);
    d.jdx = jdx;
    d.val = (const char *)val;
    d.roffs = reinterpret_cast<const int64_t *>(roffs);
    d.rjdx = rjdx;
    d.rval = (const char *)rval;
    d.b_first = b_first;
    d.jdim_c = jdim_c;
    d.nrows = (uint64_t)nrows;
    d.nblk = nblk;
    d.ncut = ncut;
}

int launch_spgemm_count(long long nrows, int nblk, const int *offs, const long long *start, const int *jdx,
                        long long b_first, long long brows, const long long *roffs, const int *rjdx, long long jdim_c,
                        int ncut, int *counts, long long *bound, hipStream_t stream) {
    if (nrows < 0 || nblk < 0 || brows < 0 || jdim_c < 0 || ncut < 0) return kPatchErrCount;
    if (nrows == 0 || ncut == 0) return 0;
    const int rc = spg_check(false, 1, nrows, nblk, offs, start, jdx, nullptr, b_first, brows, roffs, rjdx, nullptr, jdim_c,
                             ncut, counts, (uint64_t)ncut * (uint64_t)nrows * 4, bound, (uint64_t)nrows * 8, nullptr, nullptr);
    if (rc) return rc;
    SpgDesc d;
    spg_desc(d, nrows, nblk, offs, start, jdx, nullptr, b_first, roffs, rjdx, nullptr, jdim_c, ncut);
    d.counts = counts;
    d.bound = reinterpret_cast<int64_t *>(bound);
    hipLaunchKernelGGL(k_spgemm_count, dim3(spg_grid(d.nrows)), dim3(kSpgBS), 0, stream, d);
    return rc_of(hipGetLastError());
}

int launch_spgemm_fill(int op, long long nrows, int nblk, const int *offs, const long long *start, const int *jdx,
                       const void *val, long long b_first, long long brows, const long long *roffs, const int *rjdx,
                       const void *rval, long long jdim_c, int ncut, const int *coffs, const long long *cstart, int *cjdx,
                       void *cval, hipStream_t stream) {
    if (nrows < 0 || nblk < 0 || brows < 0 || jdim_c < 0 || ncut < 0) return kPatchErrCount;
    const int esz = (op == kOpCopy) ? 0 : elem_size(op);
    if (!esz) return kPatchErrOp;
    if (nrows == 0 || ncut == 0) return 0;
    const int rc = spg_check(true, esz, nrows, nblk, offs, start, jdx, val, b_first, brows, roffs, rjdx, rval, jdim_c, ncut,
                             cjdx, 4, cval, (uint64_t)esz, coffs, cstart);
    if (rc) return rc;
    if (nblk == 0) return 0;   // no entry of A: no entry of C
    SpgDesc d;
    spg_desc(d, nrows, nblk, offs, start, jdx, val, b_first, roffs, rjdx, rval, jdim_c, ncut);
    d.coffs = coffs;
    d.cstart = reinterpret_cast<const int64_t *>(cstart);
    d.cjdx = cjdx;
    d.cval = (char *)cval;
    return rc_of(for_type(op, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((k_spgemm_fill<typename T::real, T::parts>), dim3(spg_grid(d.nrows)), dim3(kSpgBS), 0, stream, d);
        return hipGetLastError();
    }));
}

// ---------------------------------------------------------------------------
struct CsrRowsDesc {
    const int32_t *offs;
    const int64_t *start;
    const int32_t *jdx;
    const char *val;
    int64_t *roffs;
    int32_t *rjdx;
    char *rval;
    uint64_t nrows;
    int32_t nblk;
};

// roffs[r + 1] = the length of row r's list, roffs[0] = 0
__global__ __launch_bounds__(kSprsBS) void k_csr_row_len(const CsrRowsDesc d) {
    const uint64_t step = (uint64_t)gridDim.x * kSprsBS;
    for (uint64_t row = (uint64_t)blockIdx.x * kSprsBS + threadIdx.x; row < d.nrows; row += step) {
        int64_t n = 0;
        for (int32_t b = 0; b < d.nblk; ++b) {
            const int32_t *o = d.offs + (int64_t)b * (int64_t)(d.nrows + 1) + (int64_t)row;
            n += (int64_t)((uint32_t)o[1] - (uint32_t)o[0]);
        }
        d.roffs[row + 1] = n;
        if (row == 0) d.roffs[0] = 0;
    }
}

constexpr int kSpgScanBS = 1024;

// x[i] = x[0] + .. + x[i], in place, by ONE workgroup: a thread sums its consecutive share, the shares' sums are
// scanned in LDS, the thread then stores its share's running sums
__global__ __launch_bounds__(kSpgScanBS) void k_scan_i64(int64_t *x, uint64_t n) {
    __shared__ int64_t part[kSpgScanBS];
    const uint64_t per = (n + kSpgScanBS - 1) / kSpgScanBS, lo = (uint64_t)threadIdx.x * per;
    const uint64_t hi = lo + per < n ? lo + per : n;
    int64_t sum = 0;
    for (uint64_t i = lo; i < hi; ++i) sum += x[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t s = 1; s < (uint32_t)kSpgScanBS; s <<= 1) {
        const int64_t o = threadIdx.x >= s ? part[threadIdx.x - s] : 0;
        __syncthreads();
        part[threadIdx.x] += o;
        __syncthreads();
    }
    int64_t run = part[threadIdx.x] - sum;
    for (uint64_t i = lo; i < hi; ++i) {
        run += x[i];
        x[i] = run;
    }
}

constexpr int kCsrRowsLg = 4;   // a team of 16 lanes per row

template <typename T, int NP>
__global__ __launch_bounds__(kSprsBS) void k_csr_row_copy(const CsrRowsDesc d) {
    typedef SprsEl<T, NP> E;
    const uint32_t W = 1u << kCsrRowsLg, lane = threadIdx.x & (W - 1);
    const uint64_t per = (uint64_t)(kSprsBS >> kCsrRowsLg), step = (uint64_t)gridDim.x * per;
    const E *val = reinterpret_cast<const E *>(d.val);
    E *rval = reinterpret_cast<E *>(d.rval);
    for (uint64_t row = (uint64_t)blockIdx.x * per + (threadIdx.x >> kCsrRowsLg); row < d.nrows; row += step) {
        int64_t to = d.roffs[row];
        for (int32_t b = 0; b < d.nblk; ++b) {
            const int32_t *o = d.offs + (int64_t)b * (int64_t)(d.nrows + 1) + (int64_t)row;
            const uint32_t o0 = (uint32_t)o[0], c = (uint32_t)o[1] - o0;
            const int64_t k0 = d.start[b] + (int64_t)o0;
            for (uint32_t t = lane; t < c; t += W) {
                d.rjdx[to + (int64_t)t] = d.jdx[k0 + (int64_t)t];
                rval[to + (int64_t)t] = val[k0 + (int64_t)t];
            }
            to += (int64_t)c;
        }
    }
}

int launch_csr_rows(int op, long long nrows, int nblk, const int *offs, const long long *start, const int *jdx,
                    const void *val, long long *roffs, int *rjdx, void *rval, hipStream_t stream) {
    if (nrows < 0 || nblk < 0) return kPatchErrCount;
    const int esz = (op == kOpCopy) ? 0 : elem_size(op);
    if (!esz) return kPatchErrOp;
    if (nrows == 0) return 0;
    if (!roffs || (nblk > 0 && (!offs || !start || !jdx || !val || !rjdx || !rval))) return kPatchErrScalar;
    if (nrows > kSprsMaxRows) return kPatchErrRange;
    if ((((uintptr_t)val | (uintptr_t)rval) & (uintptr_t)(esz - 1)) || (((uintptr_t)start | (uintptr_t)roffs) & 7) ||
        (((uintptr_t)offs | (uintptr_t)jdx | (uintptr_t)rjdx) & 3))
        return kPatchErrAlign;
    if (nblk > 0) {
        const uint64_t ob = (uint64_t)nblk * (uint64_t)(nrows + 1) * 4, rb = (uint64_t)(nrows + 1) * 8;
        const struct { const void *p; uint64_t n; } in[] = {{offs, ob}, {start, (uint64_t)nblk * 8}, {jdx, 4}, {val, (uint64_t)esz}};
        for (const auto &s : in)
            if (span_hit(roffs, rb, s.p, s.n) || span_hit(rjdx, 4, s.p, s.n) || span_hit(rval, (uint64_t)esz, s.p, s.n))
                return kPatchErrOverlap;
    }
    CsrRowsDesc d;
    memset(&d, 0, sizeof(d));
    d.offs = offs;
    d.start = reinterpret_cast<const int64_t *>(start);
    d.jdx = jdx;
    d.val = (const char *)val;
    d.roffs = reinterpret_cast<int64_t *>(roffs);
    d.rjdx = rjdx;
    d.rval = (char *)rval;
    d.nrows = (uint64_t)nrows;
    d.nblk = nblk;
    hipLaunchKernelGGL(k_csr_row_len, dim3(sprs_grid(d.nrows, 0)), dim3(kSprsBS), 0, stream, d);
    if (hipError_t e = hipGetLastError()) return rc_of(e);
    hipLaunchKernelGGL(k_scan_i64, dim3(1), dim3(kSpgScanBS), 0, stream, d.roffs + 1, d.nrows);
    if (hipError_t e = hipGetLastError()) return rc_of(e);
    if (nblk == 0) return 0;
    return rc_of(for_type(op, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((k_csr_row_copy<typename T::real, T::parts>), dim3(sprs_grid(d.nrows, kCsrRowsLg)), dim3(kSprsBS),
                           0, stream, d);
        return hipGetLastError();
    }));
}

}  // namespace gaamd
