// gaamd_gemm_cplx.hip -- row-major complex GEMM on the gfx950 matrix cores (ga_amd.h
// gaamd_gemm_cplx):
//   C[i][j] = alpha * sum_k op(A)[i][k] * op(B)[k][j] + beta * C[i][j]
// for COMEX_ACC_DCP (v_mfma_f64_16x16x4_f64 on the parts) and COMEX_ACC_CPL
// (v_mfma_f32_16x16x4_f32), elements interleaved (re, im); op(X) is X, its transpose or its
// conjugate transpose.  Where the reference's pnga_matmul hands these types to a host
// zgemm / cgemm, GA_Zgemm / GA_Cgemm (ga.cpp) call this on HBM.
//
// k_gemm's shape (gaamd_gemm.hip, included before this file: GemmMfma and gemm_span are its),
// with two accumulators per element of C.  A complex product is four real matrix-core
// products: re += a.re * b.re, re += a.im * (-b.im), im += a.re * b.im, im += a.im * b.re.
// One workgroup of 256 threads is 2 x 2 waves; a wave owns 4 x WN MFMA tiles of 16 x 16:
//   f64 complex  WN = 2: the wave 64 x 32, the workgroup 128 x 64;  8 tiles x 2 parts x 8
//                registers = 128 accumulator registers, what k_gemm<double> has
//   f32 complex  WN = 4: the wave 64 x 64, the workgroup 128 x 128; 16 x 2 x 4 = 128
// (64 x 64 of f64 complex would be 256 registers of accumulators alone: the whole budget of
// a lane at two workgroups per CU.)
//
// LDS holds the re and the im plane of both operands apart, k-major: As[part][k][i],
// Bs[part][k][j].  The global -> LDS copy splits the parts, does the transposition and, for
// trans 'C', negates the imaginary part -- exactly, a flip of the sign bit -- so the nine (transa,
// transb) cases share the inner loop.  The next k-tile's loads are in flight while the
// matrix cores work on this one.
//
// Order (the contract of ga_amd.h): both accumulators of an element start at +0; for every
// group of four consecutive k, from 0 upwards, re takes the instruction over a.re * b.re,
// then the one over -a.im * b.im; im takes the one over a.re * b.im, then the one over
// a.im * b.re.  The sign is put on b.im here: (-x) * y and x * (-y) are the same bits.
// Nothing depends on the element's place in the tile or the grid, or on m and n.  Edge tiles
// are zero-filled by predication, and no load or store leaves the operands.
#include "gaamd_kernels.h"
#include <string.h>

namespace gaamd {

static_assert(kCGemmTM == 128, "the thread maps below are written for 2 x 2 waves of 64 rows");

// the conjugation: the sign bit of an imaginary part flipped (flip is the sign bit or 0).
// It is done on the way from the registers to LDS, after the wait for the loads, so that
// nothing between a load and the MFMAs it flies under needs its value.  The +0 of a
// zero-filled edge element takes the sign too.  That changes no bit of C: a product of two
// zeros is a zero of some sign, and x + (+-0) == x for every x but -0, which an accumulator
// that started at +0 never holds under round-to-nearest.
// elem: one complex element as it lies in memory, aligned to its real part only; it stays one
// value from the load to the LDS store, so a predicated load needs nothing but its own
// destination registers cleared beforehand.
template <typename T> struct CGemmBits;
template <> struct CGemmBits<double> {
    typedef unsigned long long type;
    static constexpr type sign = 1ull << 63;
    typedef double elem __attribute__((ext_vector_type(2), aligned(8)));
};
template <> struct CGemmBits<float> {
    typedef unsigned int type;
    static constexpr type sign = 1u << 31;
    typedef float elem __attribute__((ext_vector_type(2), aligned(4)));
};
template <typename T>
static __device__ __forceinline__ T cgemm_flip(T v, typename CGemmBits<T>::type flip) {
    return __builtin_bit_cast(T, __builtin_bit_cast(typename CGemmBits<T>::type, v) ^ flip);
}

// One operand's share of a k-tile: X x TK complex elements, X * TK / 256 per thread.  Element
// (kk, x) of the tile, x < X along m (A) or n (B), has its real part at p0[2 * (x * sx +
// kk * sk)] with p0 the tile's corner.  kc: the operand is contiguous along k in memory, so
// consecutive lanes take consecutive k and a thread's elements are 256 / TK x apart;
// otherwise consecutive lanes take consecutive x and its elements are 256 / X k apart.
// p is the real part of the thread's first element, step the distance to its next in
// complex elements; xrem / krem: the x and k left in range from the tile's corner.
template <typename T, int X, int TK>
static __device__ __forceinline__ void cgemm_load(typename CGemmBits<T>::elem (&r)[X * TK / 256],
                                                  const T *__restrict__ p, int64_t step, bool kc, int xrem, int krem,
                                                  int t) {
    typedef typename CGemmBits<T>::elem E;
#pragma unroll
    for (int i = 0; i < X * TK / 256; ++i) {
        const int kk = kc ? (t % TK) : (t / X) + (256 / X) * i;
        const int x = kc ? (t / TK) + (256 / TK) * i : (t % X);
        r[i] = (x < xrem && kk < krem) ? *(const E *)(p + 2 * i * step) : E(T(0));
    }
}

template <typename T, int X, int TK>
static __device__ __forceinline__ void cgemm_store(T (*sre)[X + 16], T (*sim)[X + 16],
                                                   const typename CGemmBits<T>::elem (&r)[X * TK / 256], bool kc,
                                                   bool conj, int t) {
    const typename CGemmBits<T>::type flip = conj ? CGemmBits<T>::sign : 0;
#pragma unroll
    for (int i = 0; i < X * TK / 256; ++i) {
        const int kk = kc ? (t % TK) : (t / X) + (256 / X) * i;
        const int x = kc ? (t / TK) + (256 / TK) * i : (t % X);
        sre[kk][x] = r[i].x;
        sim[kk][x] = cgemm_flip<T>(r[i].y, flip);
    }
}

enum { kCBetaZero = 0, kCBetaOne = 1, kCBetaAny = 2 };

// strides in complex elements; A, B, C point at the real part of the first element
template <typename T, int WN, int TK>
__global__ __launch_bounds__(256, 2) void k_gemm_cplx(const T *__restrict__ A, const T *__restrict__ B,
                                                   T *__restrict__ C, int64_t m, int64_t n, int64_t k, int64_t a_sm,
                                                   int64_t a_sk, int64_t b_sn, int64_t b_sk, int64_t ldc,
                                                   uint32_t tiles_n, T al_re, T al_im, T be_re, T be_im, int a_kc,
                                                   int b_kc, int a_conj, int b_conj, int beta_mode) {
    typedef GemmMfma<T> M;
    constexpr int TM = kCGemmTM, TN = 32 * WN;
    __shared__ T As[2][TK][TM + 16];
    __shared__ T Bs[2][TK][TN + 16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t m0 = (int64_t)(blockIdx.x / tiles_n) * TM, n0 = (int64_t)(blockIdx.x % tiles_n) * TN;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * (16 * WN);
    const int l15 = lane & 15, lq = lane >> 4;

    typename M::acc_t acc_re[4][WN], acc_im[4][WN];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc_re[i][j] = acc_im[i][j] = (typename M::acc_t)(T(0));

    // this thread's first element of each operand's k-tile, and the way to its next
    const int a_kk = a_kc ? (t % TK) : (t / TM), a_x = a_kc ? (t / TK) : (t % TM);
    const int b_kk = b_kc ? (t % TK) : (t / TN), b_x = b_kc ? (t / TK) : (t % TN);
    const T *pa = A + 2 * ((m0 + a_x) * a_sm + a_kk * a_sk);
    const T *pb = B + 2 * ((n0 + b_x) * b_sn + b_kk * b_sk);
    const int64_t a_step = a_kc ? (256 / TK) * a_sm : (256 / TM) * a_sk;
    const int64_t b_step = b_kc ? (256 / TK) * b_sn : (256 / TN) * b_sk;
    const int mrem = (int)(m - m0 < TM ? m - m0 : TM), nrem = (int)(n - n0 < TN ? n - n0 : TN);

    typename CGemmBits<T>::elem ra[TM * TK / 256], rb[TN * TK / 256];
    {
        const int krem = (int)(k < TK ? k : TK);
        cgemm_load<T, TM, TK>(ra, pa, a_step, a_kc != 0, mrem, krem, t);
        cgemm_load<T, TN, TK>(rb, pb, b_step, b_kc != 0, nrem, krem, t);
    }
    for (int64_t k0 = 0; k0 < k; k0 += TK) {
        cgemm_store<T, TM, TK>(As[0], As[1], ra, a_kc != 0, a_conj != 0, t);
        cgemm_store<T, TN, TK>(Bs[0], Bs[1], rb, b_kc != 0, b_conj != 0, t);
        __syncthreads();
        if (k0 + TK < k) {   // the next k-tile's loads fly while this one is multiplied
            const int64_t left = k - k0 - TK;
            const int krem = (int)(left < TK ? left : TK);
            pa += 2 * TK * a_sk;
            pb += 2 * TK * b_sk;
            cgemm_load<T, TM, TK>(ra, pa, a_step, a_kc != 0, mrem, krem, t);
            cgemm_load<T, TN, TK>(rb, pb, b_step, b_kc != 0, nrem, krem, t);
        }
#pragma unroll
        for (int ks = 0; ks < TK; ks += 4) {   // increasing k, four products per group: the order contract
            T ar[4], ai[4], br[WN], bi[WN], nbi[WN];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ar[i] = As[0][ks + lq][wm + 16 * i + l15];
                ai[i] = As[1][ks + lq][wm + 16 * i + l15];
            }
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                br[j] = Bs[0][ks + lq][wn + 16 * j + l15];
                bi[j] = Bs[1][ks + lq][wn + 16 * j + l15];
                nbi[j] = -bi[j];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) {
                    acc_re[i][j] = M::mfma(ar[i], br[j], acc_re[i][j]);
                    acc_im[i][j] = M::mfma(ar[i], bi[j], acc_im[i][j]);
                }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) {
                    acc_re[i][j] = M::mfma(ai[i], nbi[j], acc_re[i][j]);
                    acc_im[i][j] = M::mfma(ai[i], br[j], acc_im[i][j]);
                }
        }
        __syncthreads();
    }

    // t = alpha * acc and u = beta * c as four products, one difference and one sum each (no
    // FMA: -ffp-contract=off), c = t + u part by part; beta == 0 never reads C, beta == (1, 0)
    // adds C as it is
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t gm = m0 + wm + 16 * i + M::row(lane, r), gn = n0 + wn + 16 * j + l15;
                if (gm < m && gn < n) {
                    T *p = C + 2 * (gm * ldc + gn);
                    const T s_re = acc_re[i][j][r], s_im = acc_im[i][j][r];
                    T v_re = al_re * s_re - al_im * s_im;
                    T v_im = al_re * s_im + al_im * s_re;
                    if (beta_mode == kCBetaOne) {
                        v_re = v_re + p[0];
                        v_im = v_im + p[1];
                    } else if (beta_mode == kCBetaAny) {
                        const T c_re = p[0], c_im = p[1];
                        v_re = v_re + (be_re * c_re - be_im * c_im);
                        v_im = v_im + (be_re * c_im + be_im * c_re);
                    }
                    p[0] = v_re;
                    p[1] = v_im;
                }
            }
}

static int cgemm_trans(int c) {
    if (c == 'N' || c == 'n') return 0;
    if (c == 'T' || c == 't') return 1;
    if (c == 'C' || c == 'c') return 2;
    return -1;
}

int plan_gemm_cplx(int op, int transa, int transb, long long m, long long n, long long k, const void *alpha,
                   const void *a, long long lda, const void *b, long long ldb, const void *beta, const void *c,
                   long long ldc, long long plan[6]) {
    const int esz = op == COMEX_ACC_DCP ? 16 : op == COMEX_ACC_CPL ? 8 : 0;
    const int ta = cgemm_trans(transa), tb = cgemm_trans(transb);
    if (!esz || ta < 0 || tb < 0) return kPatchErrOp;
    if (m < 0 || n < 0 || k < 0) return kPatchErrCount;
    if (!alpha || !beta) return kPatchErrScalar;
    // as stored: A is m x k ('N') or k x m ('T', 'C'), B is k x n ('N') or n x k ('T', 'C')
    const long long a_rows = ta ? k : m, a_len = ta ? m : k, b_rows = tb ? n : k, b_len = tb ? k : n;
    if (lda < a_len || ldb < b_len || ldc < n) return kPatchErrStride;
    const unsigned part = (unsigned)esz / 2;   // alignment to the real part is enough
    if ((uintptr_t)a % part || (uintptr_t)b % part || (uintptr_t)c % part) return kPatchErrAlign;
    uint64_t alo, ahi, blo, bhi, clo, chi;
    gemm_span(a, a_rows, a_len, lda, esz, alo, ahi);
    gemm_span(b, b_rows, b_len, ldb, esz, blo, bhi);
    gemm_span(c, m, n, ldc, esz, clo, chi);
    if ((clo < ahi && alo < chi) || (clo < bhi && blo < chi)) return kPatchErrOverlap;
    const long long TN = op == COMEX_ACC_DCP ? kCGemmTN_DCP : kCGemmTN_CPL, TK = op == COMEX_ACC_DCP ? kCGemmTK_DCP : kCGemmTK_CPL;
    const long long tm = (m + kCGemmTM - 1) / kCGemmTM, tn = (n + TN - 1) / TN;
    if (tm > 0 && tn > 0x7fffffffll / tm) return kPatchErrRange;
    if (plan) {
        plan[0] = kCGemmTM;
        plan[1] = TN;
        plan[2] = TK;
        plan[3] = tm;
        plan[4] = tn;
        plan[5] = (k + TK - 1) / TK;
    }
    return (m == 0 || n == 0) ? 1 : 0;
}

template <typename T, int WN, int TK>
static hipError_t go_gemm_cplx(int ta, int tb, long long m, long long n, long long k, const T *al, const void *a,
                               long long lda, const void *b, long long ldb, const T *be, void *c, long long ldc,
                               const long long *plan, hipStream_t st) {
    // element (i, kk) of op(A) at a[i * a_sm + kk * a_sk]; (kk, j) of op(B) at b[j * b_sn + kk * b_sk]
    const int64_t a_sm = ta ? 1 : lda, a_sk = ta ? lda : 1, b_sn = tb ? ldb : 1, b_sk = tb ? 1 : ldb;
    const int mode = be[0] == T(0) && be[1] == T(0) ? kCBetaZero : be[0] == T(1) && be[1] == T(0) ? kCBetaOne : kCBetaAny;
    hipLaunchKernelGGL((k_gemm_cplx<T, WN, TK>), dim3((unsigned)(plan[3] * plan[4])), dim3(256), 0, st, (const T *)a,
                       (const T *)b, (T *)c, (int64_t)m, (int64_t)n, (int64_t)k, a_sm, a_sk, b_sn, b_sk, (int64_t)ldc,
                       (uint32_t)plan[4], al[0], al[1], be[0], be[1], ta ? 0 : 1, tb ? 1 : 0, ta == 2 ? 1 : 0,
                       tb == 2 ? 1 : 0, mode);
    return hipGetLastError();
}

int launch_gemm_cplx(int op, int transa, int transb, long long m, long long n, long long k, const void *alpha,
                     const void *a, long long lda, const void *b, long long ldb, const void *beta, void *c,
                     long long ldc, hipStream_t stream) {
    long long plan[6];
    const int rc = plan_gemm_cplx(op, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, plan);
    if (rc) return rc < 0 ? rc : 0;
    double ald[2], bed[2];
    float alf[2], bef[2];
    bool alpha0, beta0;
    if (op == COMEX_ACC_DCP) {
        memcpy(ald, alpha, 16);
        memcpy(bed, beta, 16);
        alpha0 = ald[0] == 0.0 && ald[1] == 0.0;
        beta0 = bed[0] == 0.0 && bed[1] == 0.0;
    } else {
        memcpy(alf, alpha, 8);
        memcpy(bef, beta, 8);
        alpha0 = alf[0] == 0.0f && alf[1] == 0.0f;
        beta0 = bef[0] == 0.0f && bef[1] == 0.0f;
    }
    if (alpha0 || k == 0) {
        // A and B are not read: C = beta * C, by the patch kernels (beta == 0: C = 0, not read)
        const long long count[2] = {n, m}, stride[1] = {ldc * (op == COMEX_ACC_DCP ? 16 : 8)};
        const double zero[2] = {0.0, 0.0};
        return beta0 ? launch_patch_fill(op, zero, c, stride, count, 2, stream)
                     : launch_patch_scale(op, beta, c, stride, count, 2, stream);
    }
    const int ta = cgemm_trans(transa), tb = cgemm_trans(transb);
    const hipError_t e =
        op == COMEX_ACC_DCP ? go_gemm_cplx<double, kCGemmTN_DCP / 32, kCGemmTK_DCP>(ta, tb, m, n, k, ald, a, lda, b, ldb, bed, c, ldc,
                                                                        plan, stream)
                 : go_gemm_cplx<float, kCGemmTN_CPL / 32, kCGemmTK_CPL>(ta, tb, m, n, k, alf, a, lda, b, ldb, bef, c, ldc,
                                                                       plan, stream);
    return e == hipSuccess ? 0 : -100 - (int)e;
}

}  // namespace gaamd
