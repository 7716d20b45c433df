// gaamd_transpose.hip -- row-major transpose through LDS (ga_amd.h gaamd_transpose,
// gaamd_transpose_acc): the kernels under GA_Transpose and GA_Symmetrize (ga.cpp).
//   transpose:      dst[j][i] = src[i][j]                  a bit copy of 4-, 8- or 16-byte elements
//   transpose_acc:  c[i][j]   = alpha * (c[i][j] + b[j][i])  f64 / f32, ga_symmetr.c:41's expression
// The reference's pnga_transpose (global.nalg.c:954) and pnga_symmetrize (ga_symmetr.c:49)
// move blocks through host buffers and loop over them there; here every block is in HBM.
//
// One workgroup of 256 threads moves one TS x TS tile of the source (TS = 64 for 4- and
// 8-byte elements, 32 for 16-byte ones): it loads the tile along source rows, keeps it in
// LDS as tile[r][c] with a row pitch of TS + 1 elements, and after one barrier reads it
// down the columns to store along destination rows.  Both global sides are contiguous
// runs of TS elements (256 B, 512 B, 512 B); a side whose base and ld are multiples of 16
// bytes moves 16-byte vectors (decided per launch and per side), any other side single
// elements.  The LDS accesses are always single elements; with the odd pitch neither the
// row-wise store nor the column-wise load is more than 2-way conflicted under the bank
// rule (the arithmetic is in DESIGN.md).  Edge tiles are predicated: nothing outside
// rows x cols is read, nothing outside cols x rows is written.  All offsets are 64-bit.
#include "gaamd_device.hpp"
#include <string.h>

#pragma clang fp contract(off)

namespace gaamd {

typedef Vec<16>::T TrE16;   // a 16-byte element (COMEX_ACC_DCP), moved whole

template <typename E> union TrVec {
    Vec<16>::T v;
    E e[16 / sizeof(E)];
};

// vs / vd: the source / destination side moves 16-byte vectors.  ACC: dst is c, src is b
// and the stored value is alpha * (c + b^T): one add, then one multiply.
template <typename E, int TS, bool ACC>
__global__ __launch_bounds__(256) void k_transpose(const E *__restrict__ src, E *__restrict__ dst, int64_t rows,
                                                    int64_t cols, int64_t ld_s, int64_t ld_d, uint32_t tiles_c,
                                                    E alpha, int vs, int vd) {
    constexpr int V = 16 / (int)sizeof(E);   // elements per 16-byte vector
    __shared__ E tile[TS][TS + 1];
    const int t = threadIdx.x;
    // blocks that run together lie on a diagonal of the tile grid: their loads and their
    // stores then differ in row and in column, where a row or a column of tiles would put
    // one side's runs a whole number of (power-of-two) leading dimensions apart
    const uint32_t by = blockIdx.x / tiles_c, bx = blockIdx.x % tiles_c, tiles_r = gridDim.x / tiles_c;
    const int64_t r0 = (int64_t)((by + bx) % tiles_r) * TS, c0 = (int64_t)bx * TS;
    const int rrem = (int)(rows - r0 < TS ? rows - r0 : TS), crem = (int)(cols - c0 < TS ? cols - c0 : TS);
    const E *s = src + r0 * ld_s + c0;   // the tile's corner in the source ...
    E *d = dst + c0 * ld_d + r0;         // ... and of its transpose in the destination

    // global -> LDS along source rows
    if (V > 1 && vs) {
        constexpr int NVR = TS / V, IT = TS * NVR / 256;   // vectors per tile row, per thread
        TrVec<E> u[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int idx = t + 256 * it, r = idx / NVR, c = (idx % NVR) * V;
            const E *p = s + (int64_t)r * ld_s + c;
            if (r < rrem && c + V <= crem) {
                u[it].v = *reinterpret_cast<const Vec<16>::T *>(p);
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k) u[it].e[k] = (r < rrem && c + k < crem) ? p[k] : E{};
            }
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int idx = t + 256 * it, r = idx / NVR, c = (idx % NVR) * V;
#pragma unroll
            for (int k = 0; k < V; ++k) tile[r][c + k] = u[it].e[k];
        }
    } else {
        constexpr int IT = TS * TS / 256;
        E u[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int idx = t + 256 * it, r = idx / TS, c = idx % TS;
            u[it] = (r < rrem && c < crem) ? s[(int64_t)r * ld_s + c] : E{};
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int idx = t + 256 * it;
            tile[idx / TS][idx % TS] = u[it];
        }
    }
    __syncthreads();

    // LDS -> global along destination rows: destination row j is source column j
    if (V > 1 && vd) {
        constexpr int NVR = TS / V, IT = TS * NVR / 256;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int idx = t + 256 * it, j = idx / NVR, i = (idx % NVR) * V;
            TrVec<E> u;
#pragma unroll
            for (int k = 0; k < V; ++k) u.e[k] = tile[i + k][j];
            E *p = d + (int64_t)j * ld_d + i;
            if (j < crem && i + V <= rrem) {
                if constexpr (ACC) {
                    TrVec<E> c;
                    c.v = *reinterpret_cast<const Vec<16>::T *>(p);
#pragma unroll
                    for (int k = 0; k < V; ++k) u.e[k] = alpha * (c.e[k] + u.e[k]);
                }
                *reinterpret_cast<Vec<16>::T *>(p) = u.v;
            } else if (j < crem) {
#pragma unroll
                for (int k = 0; k < V; ++k)
                    if (i + k < rrem) {
                        if constexpr (ACC) p[k] = alpha * (p[k] + u.e[k]);
                        else p[k] = u.e[k];
                    }
            }
        }
    } else {
        constexpr int IT = TS * TS / 256;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int idx = t + 256 * it, j = idx / TS, i = idx % TS;
            const E v = tile[i][j];
            if (j < crem && i < rrem) {
                E *p = d + (int64_t)j * ld_d + i;
                if constexpr (ACC) *p = alpha * (*p + v);
                else *p = v;
            }
        }
    }
}

// bytes per element of a COMEX_ACC_* code, 0 for anything else
static int transpose_esz(int op) {
    switch (op) {
    case COMEX_ACC_INT: case COMEX_ACC_FLT: return 4;
    case COMEX_ACC_DBL: case COMEX_ACC_CPL: case COMEX_ACC_LNG: return 8;
    case COMEX_ACC_DCP: return 16;
    }
    return 0;
}

// [lo, hi) in bytes from the first element of a rows x len matrix to the end of its last
static void transpose_span(const void *base, long long rows, long long len, long long ld, int esz, uint64_t &lo,
                           uint64_t &hi) {
    lo = hi = (uint64_t)(uintptr_t)base;
    if (rows > 0 && len > 0) hi = lo + ((uint64_t)(rows - 1) * (uint64_t)ld + (uint64_t)len) * (uint64_t)esz;
}

// the checks both entry points share; esz: bytes per element, 0 = an op the call does not take
static int transpose_check(int esz, long long rows, long long cols, bool scalar_missing, const void *src,
                           long long lds, const void *dst, long long ldd, long long plan[4]) {
    if (rows < 0 || cols < 0) return kPatchErrCount;
    if (!esz) return kPatchErrOp;
    if (scalar_missing) return kPatchErrScalar;
    if (lds < cols || ldd < rows) return kPatchErrStride;
    if ((uintptr_t)src % (unsigned)esz || (uintptr_t)dst % (unsigned)esz) return kPatchErrAlign;
    uint64_t slo, shi, dlo, dhi;
    transpose_span(src, rows, cols, lds, esz, slo, shi);
    transpose_span(dst, cols, rows, ldd, esz, dlo, dhi);
    if (dlo < shi && slo < dhi) return kPatchErrOverlap;
    const long long ts = esz == 16 ? kTransposeTile16 : kTransposeTile;
    const long long tr = (rows + ts - 1) / ts, tc = (cols + ts - 1) / ts;
    if (tr > 0 && tc > 0x7fffffffll / tr) return kPatchErrRange;
    if (plan) {
        plan[0] = ts;
        plan[1] = ts;
        plan[2] = tr;
        plan[3] = tc;
    }
    return (rows == 0 || cols == 0) ? 1 : 0;
}

int plan_transpose(int op, long long rows, long long cols, const void *src, long long lds, const void *dst,
                   long long ldd, long long plan[4]) {
    return transpose_check(transpose_esz(op), rows, cols, false, src, lds, dst, ldd, plan);
}

static bool transpose_vec(const void *base, long long ld, int esz) {
    return (uintptr_t)base % 16 == 0 && ((uint64_t)ld * (unsigned)esz) % 16 == 0;
}

template <typename E, int TS, bool ACC>
static int go_transpose(long long rows, long long cols, const void *alpha, const void *src, long long lds, void *dst,
                        long long ldd, const long long *plan, hipStream_t st) {
    E al{};
    if (ACC) memcpy(&al, alpha, sizeof(E));
    hipLaunchKernelGGL((k_transpose<E, TS, ACC>), dim3((unsigned)(plan[2] * plan[3])), dim3(256), 0, st, (const E *)src,
                       (E *)dst, (int64_t)rows, (int64_t)cols, (int64_t)lds, (int64_t)ldd, (uint32_t)plan[3], al,
                       transpose_vec(src, lds, sizeof(E)) ? 1 : 0, transpose_vec(dst, ldd, sizeof(E)) ? 1 : 0);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -100 - (int)e;
}

int launch_transpose(int op, long long rows, long long cols, const void *src, long long lds, void *dst, long long ldd,
                     hipStream_t stream) {
    long long plan[4];
    const int esz = transpose_esz(op);
    const int rc = transpose_check(esz, rows, cols, false, src, lds, dst, ldd, plan);
    if (rc) return rc < 0 ? rc : 0;
    if (esz == 4)
        return go_transpose<uint32_t, kTransposeTile, false>(rows, cols, nullptr, src, lds, dst, ldd, plan, stream);
    if (esz == 8)
        return go_transpose<uint64_t, kTransposeTile, false>(rows, cols, nullptr, src, lds, dst, ldd, plan, stream);
    return go_transpose<TrE16, kTransposeTile16, false>(rows, cols, nullptr, src, lds, dst, ldd, plan, stream);
}

int launch_transpose_acc(int op, long long m, long long n, const void *alpha, const void *b, long long ldb, void *c,
                         long long ldc, hipStream_t stream) {
    // c is m x n and the destination, b is n x m and the source: rows = n, cols = m
    long long plan[4];
    const int esz = op == COMEX_ACC_DBL ? 8 : op == COMEX_ACC_FLT ? 4 : 0;
    const int rc = transpose_check(esz, n, m, !alpha, b, ldb, c, ldc, plan);
    if (rc) return rc < 0 ? rc : 0;
    if (esz == 8) return go_transpose<double, kTransposeTile, true>(n, m, alpha, b, ldb, c, ldc, plan, stream);
    return go_transpose<float, kTransposeTile, true>(n, m, alpha, b, ldb, c, ldc, plan, stream);
}

}  // namespace gaamd
