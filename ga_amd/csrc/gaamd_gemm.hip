// gaamd_gemm.hip -- row-major GEMM on the gfx950 matrix cores (ga_amd.h gaamd_gemm):
//   C[i][j] = alpha * sum_k op(A)[i][k] * op(B)[k][j] + beta * C[i][j]
// for COMEX_ACC_DBL (v_mfma_f64_16x16x4_f64) and COMEX_ACC_FLT (v_mfma_f32_16x16x4_f32).
// Where the reference's pnga_matmul (global/src/matmul.c) fetches chunks to host
// buffers and calls a host BLAS, GA_Dgemm / GA_Sgemm (ga.cpp) call this on HBM.
//
// One workgroup of 256 threads (4 waves, 2 x 2) computes a 128 x 128 tile of C; a wave
// owns 64 x 64 of it as 4 x 4 MFMA tiles of 16 x 16 -- 16 independent accumulators, so
// the 40-cycle dependent latency of the 16x16x4 form never shows.  k advances 16 at a
// time: the operands of a k-tile go global -> registers -> LDS, and the loads of the
// next k-tile are in flight while the matrix cores work on this one.
//
// LDS holds both operands k-major, As[k][i] and Bs[k][j], whatever the transposes: the
// global -> LDS copy does the transposition, so the four (transa, transb) cases share
// the inner loop.  A lane's MFMA operand is A[i = lane & 15][k = lane >> 4] (B alike),
// i.e. 16 consecutive elements of one LDS row per quarter-wave; rows are 128 + 16
// elements apart, which puts the four quarter-waves of a read on different banks.
//
// Order (the contract of ga_amd.h): every element of C has one accumulator that starts
// at +0 and takes its products in increasing k, four per instruction; nothing about it
// depends on the element's place in the tile or the grid, or on m and n.  Edge tiles
// are zero-filled by predication (a +0 * +0 product leaves a sum that started at +0
// unchanged, bit for bit), and no load or store leaves the operands.
#include "gaamd_kernels.h"
#include <string.h>

namespace gaamd {

constexpr int kGemmLd = kGemmTM + 16;   // LDS row pitch in elements (kGemmTM == kGemmTN)
static_assert(kGemmTM == 128 && kGemmTN == 128 && kGemmTK == 16, "the thread maps below are written for 128x128x16");

typedef double gemm_d4 __attribute__((ext_vector_type(4)));
typedef float gemm_f4 __attribute__((ext_vector_type(4)));

template <typename T> struct GemmMfma;
template <> struct GemmMfma<double> {
    typedef gemm_d4 acc_t;
    static __device__ __forceinline__ acc_t mfma(double a, double b, acc_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    // C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 * reg
    static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) + 4 * reg; }
};
template <> struct GemmMfma<float> {
    typedef gemm_f4 acc_t;
    static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    // C/D of the f32 form: col = lane & 15, row = 4 * (lane >> 4) + reg
    static __device__ __forceinline__ int row(int lane, int reg) { return 4 * (lane >> 4) + reg; }
};

// One operand's share of a k-tile, 8 elements per thread.  Element (kk, x) of the tile,
// x < 128 along m (A) or n (B), is p0[x * sx + kk * sk] with p0 the tile's corner.  kc: the
// operand is contiguous along k in memory (sk == 1), so consecutive lanes take consecutive
// k and a thread's 8 elements are 16 x apart; otherwise consecutive lanes take consecutive
// x and its elements are 2 k apart.  p is the thread's first element, step the distance
// to its next; xrem / krem: the x and k left in range from the tile's corner.
template <typename T>
static __device__ __forceinline__ void gemm_load(T (&r)[8], const T *__restrict__ p, int64_t step, bool kc, int xrem,
                                                 int krem, int t) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int kk = kc ? (t & 15) : (t >> 7) + 2 * i;
        const int x = kc ? (t >> 4) + 16 * i : (t & 127);
        r[i] = (x < xrem && kk < krem) ? p[i * step] : T(0);
    }
}

template <typename T>
static __device__ __forceinline__ void gemm_store(T (*s)[kGemmLd], const T (&r)[8], bool kc, int t) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int kk = kc ? (t & 15) : (t >> 7) + 2 * i;
        const int x = kc ? (t >> 4) + 16 * i : (t & 127);
        s[kk][x] = r[i];
    }
}

template <typename T>
__global__ __launch_bounds__(256, 2) void k_gemm(const T *__restrict__ A, const T *__restrict__ B, T *__restrict__ C,
                                              int64_t m, int64_t n, int64_t k, int64_t a_sm, int64_t a_sk,
                                              int64_t b_sn, int64_t b_sk, int64_t ldc, uint32_t tiles_n, T alpha, T beta,
                                              int a_kc, int b_kc, int read_c) {
    typedef GemmMfma<T> M;
    __shared__ T As[kGemmTK][kGemmLd];
    __shared__ T Bs[kGemmTK][kGemmLd];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t m0 = (int64_t)(blockIdx.x / tiles_n) * kGemmTM, n0 = (int64_t)(blockIdx.x % tiles_n) * kGemmTN;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int l15 = lane & 15, lq = lane >> 4;

    typename M::acc_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (typename M::acc_t)(T(0));

    // this thread's first element of each operand's k-tile, and the way to its next
    const int a_kk = a_kc ? (t & 15) : (t >> 7), a_x = a_kc ? (t >> 4) : (t & 127);
    const int b_kk = b_kc ? (t & 15) : (t >> 7), b_x = b_kc ? (t >> 4) : (t & 127);
    const T *pa = A + (m0 + a_x) * a_sm + a_kk * a_sk;
    const T *pb = B + (n0 + b_x) * b_sn + b_kk * b_sk;
    const int64_t a_step = a_kc ? 16 * a_sm : 2 * a_sk, b_step = b_kc ? 16 * b_sn : 2 * b_sk;
    const int mrem = (int)(m - m0 < kGemmTM ? m - m0 : kGemmTM), nrem = (int)(n - n0 < kGemmTN ? n - n0 : kGemmTN);

    T ra[8], rb[8];
    {
        const int krem = (int)(k < kGemmTK ? k : kGemmTK);
        gemm_load(ra, pa, a_step, a_kc != 0, mrem, krem, t);
        gemm_load(rb, pb, b_step, b_kc != 0, nrem, krem, t);
    }
    for (int64_t k0 = 0; k0 < k; k0 += kGemmTK) {
        gemm_store(As, ra, a_kc != 0, t);
        gemm_store(Bs, rb, b_kc != 0, t);
        __syncthreads();
        if (k0 + kGemmTK < k) {   // the next k-tile's loads fly while this one is multiplied
            const int64_t left = k - k0 - kGemmTK;
            const int krem = (int)(left < kGemmTK ? left : kGemmTK);
            pa += kGemmTK * a_sk;
            pb += kGemmTK * b_sk;
            gemm_load(ra, pa, a_step, a_kc != 0, mrem, krem, t);
            gemm_load(rb, pb, b_step, b_kc != 0, nrem, krem, t);
        }
#pragma unroll
        for (int ks = 0; ks < kGemmTK; ks += 4) {   // increasing k: the order contract
            T a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = As[ks + lq][wm + 16 * i + l15];
                b[i] = Bs[ks + lq][wn + 16 * i + l15];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = M::mfma(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }

    // alpha * acc + beta * c: two products and one sum (no FMA: -ffp-contract=off);
    // beta == 0 never reads C
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t gm = m0 + wm + 16 * i + M::row(lane, r), gn = n0 + wn + 16 * j + l15;
                if (gm < m && gn < n) {
                    T *p = C + gm * ldc + gn;
                    T v = alpha * acc[i][j][r];
                    if (read_c) v = v + beta * *p;
                    *p = v;
                }
            }
}

static int gemm_trans(int c) {
    if (c == 'N' || c == 'n') return 0;
    if (c == 'T' || c == 't') return 1;
    return -1;
}

// [lo, hi) in bytes from the first element of a rows x len matrix to the end of its last
static void gemm_span(const void *base, long long rows, long long len, long long ld, int esz, uint64_t &lo,
                      uint64_t &hi) {
    lo = hi = (uint64_t)(uintptr_t)base;
    if (rows > 0 && len > 0) hi = lo + ((uint64_t)(rows - 1) * (uint64_t)ld + (uint64_t)len) * (uint64_t)esz;
}

int plan_gemm(int op, int transa, int transb, long long m, long long n, long long k, const void *alpha,
              const void *a, long long lda, const void *b, long long ldb, const void *beta, const void *c,
              long long ldc, long long plan[6]) {
    const int esz = op == COMEX_ACC_DBL ? 8 : op == COMEX_ACC_FLT ? 4 : 0;
    const int ta = gemm_trans(transa), tb = gemm_trans(transb);
    if (!esz || ta < 0 || tb < 0) return kPatchErrOp;
    if (m < 0 || n < 0 || k < 0) return kPatchErrCount;
    if (!alpha || !beta) return kPatchErrScalar;
    // as stored: A is m x k ('N') or k x m ('T'), B is k x n ('N') or n x k ('T')
    const long long a_rows = ta ? k : m, a_len = ta ? m : k, b_rows = tb ? n : k, b_len = tb ? k : n;
    if (lda < a_len || ldb < b_len || ldc < n) return kPatchErrStride;
    if ((uintptr_t)a % (unsigned)esz || (uintptr_t)b % (unsigned)esz || (uintptr_t)c % (unsigned)esz) return kPatchErrAlign;
    uint64_t alo, ahi, blo, bhi, clo, chi;
    gemm_span(a, a_rows, a_len, lda, esz, alo, ahi);
    gemm_span(b, b_rows, b_len, ldb, esz, blo, bhi);
    gemm_span(c, m, n, ldc, esz, clo, chi);
    if ((clo < ahi && alo < chi) || (clo < bhi && blo < chi)) return kPatchErrOverlap;
    const long long tm = (m + kGemmTM - 1) / kGemmTM, tn = (n + kGemmTN - 1) / kGemmTN;
    if (tm > 0 && tn > 0x7fffffffll / tm) return kPatchErrRange;
    if (plan) {
        plan[0] = kGemmTM;
        plan[1] = kGemmTN;
        plan[2] = kGemmTK;
        plan[3] = tm;
        plan[4] = tn;
        plan[5] = (k + kGemmTK - 1) / kGemmTK;
    }
    return (m == 0 || n == 0) ? 1 : 0;
}

template <typename T>
static hipError_t go_gemm(int ta, int tb, long long m, long long n, long long k, const void *alpha, const void *a,
                          long long lda, const void *b, long long ldb, const void *beta, void *c, long long ldc,
                          const long long *plan, hipStream_t st) {
    T al, be;
    memcpy(&al, alpha, sizeof(T));
    memcpy(&be, beta, sizeof(T));
    // element (i, kk) of op(A) at a[i * a_sm + kk * a_sk]; (kk, j) of op(B) at b[j * b_sn + kk * b_sk]
    const int64_t a_sm = ta ? 1 : lda, a_sk = ta ? lda : 1, b_sn = tb ? ldb : 1, b_sk = tb ? 1 : ldb;
    hipLaunchKernelGGL(k_gemm<T>, dim3((unsigned)(plan[3] * plan[4])), dim3(256), 0, st, (const T *)a, (const T *)b,
                       (T *)c, (int64_t)m, (int64_t)n, (int64_t)k, a_sm, a_sk, b_sn, b_sk, (int64_t)ldc,
                       (uint32_t)plan[4], al, be, ta ? 0 : 1, tb ? 1 : 0, be != T(0) ? 1 : 0);
    return hipGetLastError();
}

int launch_gemm(int op, int transa, int transb, long long m, long long n, long long k, const void *alpha,
                const void *a, long long lda, const void *b, long long ldb, const void *beta, void *c, long long ldc,
                hipStream_t stream) {
    long long plan[6];
    const int rc = plan_gemm(op, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, plan);
    if (rc) return rc < 0 ? rc : 0;
    bool alpha0, beta0;
    if (op == COMEX_ACC_DBL) {
        double al, be;
        memcpy(&al, alpha, 8);
        memcpy(&be, beta, 8);
        alpha0 = al == 0.0;
        beta0 = be == 0.0;
    } else {
        float al, be;
        memcpy(&al, alpha, 4);
        memcpy(&be, beta, 4);
        alpha0 = al == 0.0f;
        beta0 = be == 0.0f;
    }
    if (alpha0 || k == 0) {
        // A and B are not read: C = beta * C, by the patch kernels (beta == 0: C = 0, not read)
        const long long count[2] = {n, m}, stride[1] = {ldc * (op == COMEX_ACC_DBL ? 8 : 4)};
        const double zero = 0.0;
        return beta0 ? launch_patch_fill(op, &zero, c, stride, count, 2, stream)
                     : launch_patch_scale(op, beta, c, stride, count, 2, stream);
    }
    const int ta = gemm_trans(transa), tb = gemm_trans(transb);
    const hipError_t e = op == COMEX_ACC_DBL ? go_gemm<double>(ta, tb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, plan, stream)
                                  : go_gemm<float>(ta, tb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, plan, stream);
    return e == hipSuccess ? 0 : -100 - (int)e;
}

}  // namespace gaamd
