// gaamd_patch.hip -- gfx950 kernels that compute on a patch of a global array
// where it lies (HBM): fill, scale, add and the dot product, with their host
// launchers (ga_amd.h section 2: gaamd_patch_fill/_scale/_add/_dot).
//
// Reference arithmetic (global/src/global.npatch.c), expression for expression:
//   fill           stores the value                               1528-1650
//   scale, real    x *= alpha                                     1953-1966
//   scale, complex re = x.re*al.re - x.im*al.im
//                  im = al.im*x.re + x.im*al.re                   1976-1986
//   add, real      c = alpha*a + beta*b (two products, one sum)   2520-2525
//   add, complex   c.re = x.re*a.re - x.im*a.im + y.re*b.re - y.im*b.im
//                  c.im = x.re*a.im + x.im*a.re + y.re*b.im + y.im*b.re   2537-2546
//   dot            sum += a*b; complex (no conjugate)
//                  re += a.re*b.re - b.im*a.im; im += a.im*b.re + b.im*a.re   938-1095
// and the element-wise algebra of global/src/elem_alg.c on the same map kernel
// (gaamd_patch_elem1 / _elem2: abs, add constant, reciprocal, multiply, divide, maximum,
// minimum; the operations ElAbs .. ElMaxMin below carry their line numbers).  RECIP and DIV
// leave an element whose divisor is zero unwritten and raise a flag word in mapped pinned
// memory, which their launchers read after synchronising the stream.
// Integers in unsigned arithmetic (two's-complement wraparound).  FP contraction is
// off (pragma below and -ffp-contract=off): no FMA in any of these kernels.
//
// Geometry: count[] in elements per dimension (dimension 0 contiguous), byte strides
// of dimensions 1.., all 64-bit.  The host drops count-1 dimensions and merges
// contiguous ones (a whole block becomes one long row), then:
//   * MAP kernel (fill, scale, add): grid = (chunks of a row) x (rows of this launch);
//     a block streams BS*U W-byte vectors of one row, W = 16 where every base, stride
//     and the row length allow, 8 or 4 otherwise; non-temporal loads and stores; the
//     row decode is wave-uniform.  No loop and no division by the chunk count.
//   * DOT kernel: work item = (row, chunk of kDotBS vectors); workgroup g sums the
//     fixed range of items [g*kDotItems, (g+1)*kDotItems): each lane its own vectors
//     in item order, the lanes of a wave by a shuffle tree, the waves through LDS in
//     wave order; one partial per workgroup goes to device scratch.  A second launch
//     of one workgroup adds the partials (lane t takes partials t*kFinalPer.. of every
//     pass of kDotBS*kFinalPer, then the same tree) and stores the result into mapped
//     pinned host memory.  Nothing depends on timing, the stream or the number of
//     compute units: the same input gives the same bits.  No atomics.
#pragma clang fp contract(off)

#include "gaamd_kernels.h"
#include "gaamd_device.hpp"
#include <string.h>
#include <mutex>
#include <vector>

namespace gaamd {

struct PatchDesc {
    char *p[3];                          // operand bases ([0]: the output; dot: a, b)
    int64_t str[3][kPatchMaxLevels];     // byte stride of row level j, per operand
    FastDiv cnt[kPatchMaxLevels];        // rows of level j
    int32_t levels;
    uint32_t row0;                       // first row of this launch
    uint64_t nvec;                       // W-byte vectors per row
};

// byte offsets of row r for the first NP operands.  LV == 1: at most one row level
// (2-D patches, contiguous runs): row r sits at r * stride, no digits.  LV == 0: mixed
// radix over all kPatchMaxLevels levels, level 0 fastest, without a branch -- the host
// fills the levels a patch does not have with count 1 and stride 0.
template <int NP, int LV>
__device__ __forceinline__ void patch_row(const PatchDesc &d, uint32_t r, int64_t (&off)[NP]) {
    if constexpr (LV == 1) {
#pragma unroll
        for (int k = 0; k < NP; ++k) off[k] = (int64_t)r * d.str[k][0];
    } else {
#pragma unroll
        for (int k = 0; k < NP; ++k) off[k] = 0;
#pragma unroll
        for (int j = 0; j < kPatchMaxLevels; ++j) {
            const uint32_t q = d.cnt[j].div(r);
            const uint32_t dig = r - q * d.cnt[j].d;
#pragma unroll
            for (int k = 0; k < NP; ++k) off[k] += (int64_t)dig * d.str[k][j];
            r = q;
        }
    }
}

// ---------------------------------------------------------------------------
// element operations on one W-byte vector.  kOps: operand pointers; kIn: vectors
// loaded (0: none; 1: the output itself; 2: operands 1 and 2)
struct PatchFill {
    static constexpr int kOps = 1, kIn = 0;
    Scale16 pat;   // the value repeated over 16 bytes
    template <int W>
    __device__ __forceinline__ typename Vec<W>::T apply(typename Vec<W>::T, typename Vec<W>::T) const {
        union { Scale16 s; typename Vec<W>::T v; } u;
        u.s = pat;
        return u.v;
    }
};

template <typename A>
struct PatchScaleReal {
    static constexpr int kOps = 1, kIn = 1;
    A s;
    template <int W>
    __device__ __forceinline__ typename Vec<W>::T apply(typename Vec<W>::T xv, typename Vec<W>::T) const {
        constexpr int N = W / (int)sizeof(A);
        union { typename Vec<W>::T v; A t[N]; } x;
        x.v = xv;
#pragma unroll
        for (int i = 0; i < N; ++i) x.t[i] = x.t[i] * s;
        return x.v;
    }
};

template <typename R>
struct PatchScaleCplx {
    static constexpr int kOps = 1, kIn = 1;
    R ar, ai;
    template <int W>
    __device__ __forceinline__ typename Vec<W>::T apply(typename Vec<W>::T xv, typename Vec<W>::T) const {
        constexpr int N = W / (int)(2 * sizeof(R));
        union { typename Vec<W>::T v; R t[2 * N]; } x;
        x.v = xv;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const R xr = x.t[2 * i], xi = x.t[2 * i + 1];
            R p1 = xr * ar;
            R p2 = xi * ai;
            R re = p1 - p2;
            R p3 = ai * xr;
            R p4 = xi * ar;
            R im = p3 + p4;
            x.t[2 * i] = re;
            x.t[2 * i + 1] = im;
        }
        return x.v;
    }
};

template <typename A>
struct PatchAddReal {
    static constexpr int kOps = 3, kIn = 2;
    A al, be;
    template <int W>
    __device__ __forceinline__ typename Vec<W>::T apply(typename Vec<W>::T av, typename Vec<W>::T bv) const {
        constexpr int N = W / (int)sizeof(A);
        union { typename Vec<W>::T v; A t[N]; } a, b;
        a.v = av;
        b.v = bv;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            A p1 = al * a.t[i];
            A p2 = be * b.t[i];
            a.t[i] = p1 + p2;
        }
        return a.v;
    }
};

// x = alpha, y = beta; a, b the elements (global.npatch.c:2537-2546), left to right
template <typename R>
struct PatchAddCplx {
    static constexpr int kOps = 3, kIn = 2;
    R xr, xi, yr, yi;
    template <int W>
    __device__ __forceinline__ typename Vec<W>::T apply(typename Vec<W>::T av, typename Vec<W>::T bv) const {
        constexpr int N = W / (int)(2 * sizeof(R));
        union { typename Vec<W>::T v; R t[2 * N]; } a, b;
        a.v = av;
        b.v = bv;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const R ar = a.t[2 * i], ai = a.t[2 * i + 1], br = b.t[2 * i], bi = b.t[2 * i + 1];
            R p1 = xr * ar;
            R p2 = xi * ai;
            R p3 = yr * br;
            R p4 = yi * bi;
            R re = p1 - p2;
            re = re + p3;
            re = re - p4;
            R q1 = xr * ai;
            R q2 = xi * ar;
            R q3 = yr * bi;
            R q4 = yi * br;
            R im = q1 + q2;
            im = im + q3;
            im = im + q4;
            a.t[2 * i] = re;
            a.t[2 * i + 1] = im;
        }
        return a.v;
    }
};

// ---------------------------------------------------------------------------
// element-wise algebra (global/src/elem_alg.c; GA_ABS / GA_MAX / GA_MIN globalp.h:55-57),
// expression for expression.  An operation F gives one element: real(a, b, s, r) for the
// real and integer types, cplx(ar, ai, br, bi, sr, si, re, im) for the complex ones, and
// returns false where the reference aborts on a zero divisor (nothing is stored then).
// Integers: sums and products in unsigned arithmetic, comparisons and quotients signed.
template <typename T>
__device__ __forceinline__ T el_abs(T a) {   // GA_ABS: -0.0 stays -0.0, INT_MIN wraps to itself
    if constexpr (std::is_integral<T>::value) {
        typedef typename std::make_unsigned<T>::type U;
        return a >= 0 ? a : (T)((U)0 - (U)a);
    } else {
        return a >= 0 ? a : -a;
    }
}
template <typename T> __device__ __forceinline__ T el_max(T a, T b) { return a >= b ? a : b; }
template <typename T> __device__ __forceinline__ T el_min(T a, T b) { return a <= b ? a : b; }

struct ElAbs {   // do_abs 245-336, the portable branch (no hypot)
    static constexpr bool kCheck = false;
    template <typename T> __device__ __forceinline__ static bool real(T a, T, T, T &r) {
        r = el_abs(a);
        return true;
    }
    template <typename R>
    __device__ __forceinline__ static bool cplx(R ar, R ai, R, R, R, R, R &re, R &im) {
        const R mr = el_abs(ar), mi = el_abs(ai);
        const bool first = mr >= mi;
        const R num = first ? ai : ar, den = first ? ar : ai, m = first ? mr : mi;
        const R x2 = num / den;
        R t = x2 * x2;
        t = (R)1 + t;
        R res;
        if constexpr (sizeof(R) == 4) {   // as C evaluates it: sqrt and the product in double
            const double q = (double)m * __builtin_sqrt((double)t);
            res = (R)q;
        } else {
            res = m * __builtin_sqrt(t);
        }
        re = (first && ar == (R)0) ? (R)0 : res;
        im = (R)0;
        return true;
    }
};

struct ElAddConst {   // do_add_const 524-574
    static constexpr bool kCheck = false;
    template <typename T> __device__ __forceinline__ static bool real(T a, T, T s, T &r) {
        if constexpr (std::is_integral<T>::value) {
            typedef typename std::make_unsigned<T>::type U;
            r = (T)((U)a + (U)s);
        } else {
            r = a + s;
        }
        return true;
    }
    template <typename R>
    __device__ __forceinline__ static bool cplx(R ar, R ai, R, R, R sr, R si, R &re, R &im) {
        re = ar + sr;
        im = ai + si;
        return true;
    }
};

struct ElRecip {   // do_recip 338-522
    static constexpr bool kCheck = true;
    template <typename T> __device__ __forceinline__ static bool real(T a, T, T, T &r) {
        if (a == (T)0) return false;
        if constexpr (std::is_integral<T>::value) r = a == (T)1 ? (T)1 : a == (T)-1 ? (T)-1 : (T)0;   // 1 / a
        else r = (T)1 / a;
        return true;
    }
    template <typename R>
    __device__ __forceinline__ static bool cplx(R x1, R x2, R, R, R, R, R &re, R &im) {
        const R magr = el_abs(x1), magi = el_abs(x2);
        const bool first = magr >= magi;
        if (first && !(magr != (R)0)) return false;
        const R num = first ? x2 : x1, den = first ? x1 : x2;
        const R c = num / den;
        R t = c * c;
        t = (R)1 + t;
        t = t * den;
        const R d = (R)1 / t;
        const R cd = first ? (-c) * d : c * d;
        re = first ? d : cd;
        im = first ? cd : -d;
        return true;
    }
};

struct ElMul {   // do_multiply 1068-1086, assign_mul_reg / _cpl
    static constexpr bool kCheck = false;
    template <typename T> __device__ __forceinline__ static bool real(T a, T b, T, T &r) {
        if constexpr (std::is_integral<T>::value) {
            typedef typename std::make_unsigned<T>::type U;
            r = (T)((U)a * (U)b);
        } else {
            r = a * b;
        }
        return true;
    }
    template <typename R>
    __device__ __forceinline__ static bool cplx(R ar, R ai, R br, R bi, R, R, R &re, R &im) {
        R p1 = ar * br;
        R p2 = ai * bi;
        re = p1 - p2;
        R p3 = ar * bi;
        R p4 = ai * br;
        im = p3 + p4;
        return true;
    }
};

struct ElDiv {   // do_divide 1136-1266; complex: every intermediate a double, for C_SCPL too
    static constexpr bool kCheck = true;
    template <typename T> __device__ __forceinline__ static bool real(T a, T b, T, T &r) {
        if (b == (T)0) return false;
        if constexpr (std::is_integral<T>::value) {
            typedef typename std::make_unsigned<T>::type U;
            r = b == (T)-1 ? (T)((U)0 - (U)a) : a / b;   // INT_MIN / -1 wraps to INT_MIN
        } else {
            r = a / b;
        }
        return true;
    }
    template <typename R>
    __device__ __forceinline__ static bool cplx(R ar, R ai, R br, R bi, R, R, R &re, R &im) {
        const double aReal = ar, aImag = ai, bReal = br, bImag = bi;
        const bool first = el_abs(bReal) >= el_abs(bImag);
        if (first && !(bReal != 0.0)) return false;
        const double num = first ? bImag : bReal, den = first ? bReal : bImag;
        const double x1 = num / den;
        double t = x1 * x1;
        t = 1.0 + t;
        t = den * t;
        const double x2 = 1.0 / t;
        const double u = (first ? aImag : aReal) * x1;   // aImag*x1 | aReal*x1
        const double v = (first ? aReal : aImag) * x1;   // aReal*x1 | aImag*x1
        const double nr = first ? aReal + u : u + aImag;
        const double ni = first ? aImag - v : v - aReal;
        re = (R)(nr * x2);
        im = (R)(ni * x2);
        return true;
    }
};

template <bool MAX>
struct ElMaxMin {   // do_maximum 1533-1625, do_minimum 1628-1720
    static constexpr bool kCheck = false;
    template <typename T> __device__ __forceinline__ static bool real(T a, T b, T, T &r) {
        r = MAX ? el_max(a, b) : el_min(a, b);
        return true;
    }
    template <typename R>
    __device__ __forceinline__ static bool cplx(R ar, R ai, R br, R bi, R, R, R &re, R &im) {
        double aReal = ar, aImag = ai, bReal = br, bImag = bi;
        double x1 = el_max(el_abs(aReal), el_abs(aImag));
        const double x2 = el_max(el_abs(bReal), el_abs(bImag));
        x1 = el_max(x1, x2);
        bool take_a = true;
        if (!(x1 == 0.0)) {
            x1 = 1.0 / x1;
            aReal = aReal * x1;
            aImag = aImag * x1;
            bReal = bReal * x1;
            bImag = bImag * x1;
            double p1 = aReal * aReal, p2 = aImag * aImag, p3 = bReal * bReal, p4 = bImag * bImag;
            const double temp1 = p1 + p2, temp2 = p3 + p4;
            take_a = MAX ? temp1 > temp2 : temp1 < temp2;
        }
        re = take_a ? ar : br;
        im = take_a ? ai : bi;
        return true;
    }
};

// F over the W / sizeof(T) elements of a vector.  KIN = 1: dst = F(dst) in place; KIN = 2:
// c = F(a, b).  `bad` receives bit i for element i of the vector when F refused it.
template <class F, typename T, int KIN>
struct PatchElemReal {
    static constexpr int kOps = KIN == 1 ? 1 : 3, kIn = KIN, kElem = (int)sizeof(T);
    static constexpr bool kCheck = F::kCheck;
    T s;
    uint32_t *flag;   // kCheck: mapped pinned word, set to 1 by every lane that meets a zero divisor
    template <int W>
    __device__ __forceinline__ typename Vec<W>::T apply(typename Vec<W>::T av, typename Vec<W>::T bv,
                                                        uint32_t &bad) const {
        constexpr int N = W / (int)sizeof(T);
        union { typename Vec<W>::T v; T t[N]; } a, b;
        a.v = av;
        b.v = bv;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            T r = a.t[i];
            if (!F::real(a.t[i], b.t[i], s, r)) bad |= 1u << i;
            a.t[i] = r;
        }
        return a.v;
    }
    template <int W>
    __device__ __forceinline__ typename Vec<W>::T apply(typename Vec<W>::T av, typename Vec<W>::T bv) const {
        uint32_t bad = 0;
        return apply<W>(av, bv, bad);
    }
};

template <class F, typename R, int KIN>
struct PatchElemCplx {
    static constexpr int kOps = KIN == 1 ? 1 : 3, kIn = KIN, kElem = 2 * (int)sizeof(R);
    static constexpr bool kCheck = F::kCheck;
    R sr, si;
    uint32_t *flag;
    template <int W>
    __device__ __forceinline__ typename Vec<W>::T apply(typename Vec<W>::T av, typename Vec<W>::T bv,
                                                        uint32_t &bad) const {
        constexpr int N = W / (int)(2 * sizeof(R));
        union { typename Vec<W>::T v; R t[2 * N]; } a, b;
        a.v = av;
        b.v = bv;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            R re = a.t[2 * i], im = a.t[2 * i + 1];
            if (!F::cplx(a.t[2 * i], a.t[2 * i + 1], b.t[2 * i], b.t[2 * i + 1], sr, si, re, im)) bad |= 1u << i;
            a.t[2 * i] = re;
            a.t[2 * i + 1] = im;
        }
        return a.v;
    }
    template <int W>
    __device__ __forceinline__ typename Vec<W>::T apply(typename Vec<W>::T av, typename Vec<W>::T bv) const {
        uint32_t bad = 0;
        return apply<W>(av, bv, bad);
    }
};

// an operation whose apply() may refuse elements (RECIP, DIV) declares kCheck = true
template <class OP, class = void> struct op_checks { static constexpr bool value = false; };
template <class OP> struct op_checks<OP, std::void_t<decltype(OP::kCheck)>> { static constexpr bool value = OP::kCheck; };

template <typename A> __device__ __forceinline__ void store_sys(A *p, A v);

// one result vector to memory.  A checking operation stores only the elements it computed:
// a refused element keeps its bytes (a vector of more than one element is W-aligned, so its
// elements are naturally aligned) and the lane raises the flag word.
template <class OP, int W>
__device__ __forceinline__ void map_store(char *o, const OP &op, typename Vec<W>::T a, typename Vec<W>::T b) {
    typedef typename Vec<W>::T V;
    if constexpr (op_checks<OP>::value) {
        uint32_t bad = 0;
        const V r = op.template apply<W>(a, b, bad);
        if (bad == 0) {
            vstore<W, true>(o, r);
            return;
        }
        constexpr int E = OP::kElem, N = W / E;
        if constexpr (N > 1) {
            union { V v; typename Vec<E>::T e[N]; } u;
            u.v = r;
#pragma unroll
            for (int i = 0; i < N; ++i)
                if (!((bad >> i) & 1u)) vstore<E, true>(o + i * E, u.e[i]);
        }
        store_sys(op.flag, 1u);
    } else {
        vstore<W, true>(o, op.template apply<W>(a, b));
    }
}

// ---------------------------------------------------------------------------
// MAP kernel: block (x, y) = chunk x of row row0 + y
template <class OP, int W, int U, int BS, int LV>
__global__ __launch_bounds__(BS) void k_patch_map(const PatchDesc d, const OP op) {
    typedef typename Vec<W>::T V;
    int64_t off[OP::kOps];
    patch_row<OP::kOps, LV>(d, d.row0 + blockIdx.y, off);
    const uint64_t c0 = (uint64_t)blockIdx.x * (uint64_t)(BS * U);
    const int64_t b0 = (int64_t)((c0 + threadIdx.x) * (uint64_t)W);
    char *o = d.p[0] + off[0] + b0;
    const char *i1 = o, *i2 = o;
    if constexpr (OP::kIn == 2) {
        i1 = d.p[1] + off[1] + b0;
        i2 = d.p[2] + off[2] + b0;
    }
    V x[U], y[U];
    if (c0 + (uint64_t)(BS * U) <= d.nvec) {   // wave-uniform: the whole chunk lies inside the row
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if constexpr (OP::kIn >= 1) x[k] = vload<W, true>(i1 + (int64_t)k * BS * W);
            else x[k] = V{};
            if constexpr (OP::kIn == 2) y[k] = vload<W, true>(i2 + (int64_t)k * BS * W);
            else y[k] = x[k];
        }
#pragma unroll
        for (int k = 0; k < U; ++k) map_store<OP, W>(o + (int64_t)k * BS * W, op, x[k], y[k]);
        return;
    }
    for (int k = 0; k < U; ++k) {   // row tail: one vector at a time
        if (c0 + threadIdx.x + (uint64_t)k * BS >= d.nvec) continue;
        V a = V{}, b = V{};
        if constexpr (OP::kIn >= 1) a = vload<W, true>(i1 + (int64_t)k * BS * W);
        if constexpr (OP::kIn == 2) b = vload<W, true>(i2 + (int64_t)k * BS * W);
        map_store<OP, W>(o + (int64_t)k * BS * W, op, a, b);
    }
}

// ---------------------------------------------------------------------------
// DOT kernels
constexpr int kDotBS = 256;     // threads per workgroup (4 waves)
constexpr int kDotItems = 8;    // (row, chunk) items per workgroup; a chunk is kDotBS vectors
constexpr int kFinalPer = 4;    // consecutive partials per lane and pass of the final workgroup

template <typename A>
struct PatchDotReal {
    typedef A acc_t;
    static constexpr int kAcc = 1;
    template <int W>
    __device__ __forceinline__ static void accum(A (&acc)[1], typename Vec<W>::T av, typename Vec<W>::T bv) {
        constexpr int N = W / (int)sizeof(A);
        union { typename Vec<W>::T v; A t[N]; } a, b;
        a.v = av;
        b.v = bv;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            A p = a.t[i] * b.t[i];
            acc[0] = acc[0] + p;
        }
    }
};

template <typename R>
struct PatchDotCplx {
    typedef R acc_t;
    static constexpr int kAcc = 2;
    template <int W>
    __device__ __forceinline__ static void accum(R (&acc)[2], typename Vec<W>::T av, typename Vec<W>::T bv) {
        constexpr int N = W / (int)(2 * sizeof(R));
        union { typename Vec<W>::T v; R t[2 * N]; } a, b;
        a.v = av;
        b.v = bv;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const R ar = a.t[2 * i], ai = a.t[2 * i + 1], br = b.t[2 * i], bi = b.t[2 * i + 1];
            R p1 = ar * br;
            R p2 = bi * ai;
            R re = p1 - p2;
            acc[0] = acc[0] + re;
            R p3 = ai * br;
            R p4 = bi * ar;
            R im = p3 + p4;
            acc[1] = acc[1] + im;
        }
    }
};

template <typename A>
__device__ __forceinline__ A shfl_down_any(A v, int delta) {
    union { A a; int w[sizeof(A) / 4]; } u;
    u.a = v;
#pragma unroll
    for (int i = 0; i < (int)(sizeof(A) / 4); ++i) u.w[i] = __shfl_down(u.w[i], delta, 64);
    return u.a;
}

// one word of the result into mapped pinned host memory (as k_flag does)
template <typename A>
__device__ __forceinline__ void store_sys(A *p, A v) {
    if constexpr (sizeof(A) == 4) {
        uint32_t w;
        memcpy(&w, &v, 4);
        __hip_atomic_store(reinterpret_cast<uint32_t *>(p), w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    } else {
        uint64_t w;
        memcpy(&w, &v, 8);
        __hip_atomic_store(reinterpret_cast<uint64_t *>(p), w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// the workgroup's sum in a fixed order: shuffle tree per wave, then waves 0..3 by lane 0
template <typename A, int NA, bool SYS>
__device__ __forceinline__ void block_sum_store(A (&acc)[NA], A *out) {
    __shared__ A sh[kDotBS / 64][NA];
#pragma unroll
    for (int delta = 32; delta > 0; delta >>= 1) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const A o = shfl_down_any(acc[i], delta);
            acc[i] = acc[i] + o;
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NA; ++i) sh[wave][i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            A s = sh[0][i];
#pragma unroll
            for (int w = 1; w < kDotBS / 64; ++w) s = s + sh[w][i];
            if constexpr (SYS) store_sys(out + i, s);
            else out[i] = s;
        }
    }
}

template <class OP, int W, int LV>
__global__ __launch_bounds__(kDotBS) void k_patch_dot(const PatchDesc d, const uint32_t items, const FastDiv chunk_div,
                                                      typename OP::acc_t *part) {
    typedef typename Vec<W>::T V;
    typedef typename OP::acc_t A;
    V va[kDotItems], vb[kDotItems];
    bool ok[kDotItems];
    const uint32_t i0 = blockIdx.x * (uint32_t)kDotItems;
    // every load first and without a branch, so that all are in flight together: a lane
    // without a vector in an item (past the row's end, or an item past the last) reads
    // vector 0 of a row of the patch instead and drops it below
#pragma unroll
    for (int k = 0; k < kDotItems; ++k) {
        const bool in = i0 + k < items;
        const uint32_t it = in ? i0 + k : 0u;
        const uint32_t rl = chunk_div.div(it);
        const uint32_t chunk = it - rl * chunk_div.d;
        int64_t off[2];
        patch_row<2, LV>(d, rl, off);
        const uint64_t v = (uint64_t)chunk * kDotBS + threadIdx.x;
        ok[k] = in && v < d.nvec;
        const int64_t b = ok[k] ? (int64_t)(v * W) : 0;
        va[k] = vload<W, true>(d.p[0] + off[0] + b);
        vb[k] = vload<W, true>(d.p[1] + off[1] + b);
    }
    // the sums in item order; a dropped vector adds 0 * 0 = +0, which leaves every sum as
    // it is (a sum that starts at +0 never becomes -0)
    A acc[OP::kAcc] = {};
#pragma unroll
    for (int k = 0; k < kDotItems; ++k) {
        if (!ok[k]) {
            va[k] = V{};
            vb[k] = V{};
        }
        OP::template accum<W>(acc, va[k], vb[k]);
    }
    block_sum_store<A, OP::kAcc, false>(acc, part + (size_t)blockIdx.x * OP::kAcc);
}

template <typename A, int NA>
__global__ __launch_bounds__(kDotBS) void k_patch_dot_final(const A *part, const uint32_t n, A *out) {
    A acc[NA] = {};
    for (uint32_t base = 0; base < n; base += kDotBS * kFinalPer) {
#pragma unroll
        for (int k = 0; k < kFinalPer; ++k) {
            const uint32_t i = base + threadIdx.x * kFinalPer + k;
            if (i < n) {
#pragma unroll
                for (int j = 0; j < NA; ++j) acc[j] = acc[j] + part[(size_t)i * NA + j];
            }
        }
    }
    block_sum_store<A, NA, true>(acc, out);
}

// ---------------------------------------------------------------------------
// host: checks, merging, vector width
struct PatchPlan {
    int esz = 0, W = 0, L = 0, block = 0;
    uint64_t row_bytes = 0, rows = 1;
    uint32_t cn[kPatchMaxLevels] = {};
    int64_t st[3][kPatchMaxLevels] = {};
};

// 0: launch; 1: nothing to do (a count of zero); < 0: error
static int patch_plan(int op, int nops, const void *const *base, const long long *const *stride,
                      const long long *count, int ndim, PatchPlan &p) {
    if (ndim < 1 || ndim > kPatchMaxLevels + 1) return kPatchErrNdim;
    p.esz = (op == kOpCopy) ? 0 : elem_size(op);
    if (!p.esz) return kPatchErrOp;
    if (!count) return kPatchErrCount;
    bool empty = false;
    for (int d = 0; d < ndim; ++d) {
        if (count[d] < 0) return kPatchErrCount;
        if (count[d] == 0) empty = true;
    }
    for (int k = 0; k < nops; ++k)
        if (ndim > 1 && !stride[k]) return kPatchErrStride;
    if (empty) return 1;
    if (count[0] > (long long)(INT64_MAX / 32)) return kPatchErrRange;
    p.row_bytes = (uint64_t)count[0] * (uint64_t)p.esz;
    int L = 0;
    for (int d = 1; d < ndim; ++d) {
        if (count[d] == 1) continue;
        if (count[d] >= (1ll << 31)) return kPatchErrRange;
        p.cn[L] = (uint32_t)count[d];
        for (int k = 0; k < nops; ++k) p.st[k][L] = stride[k][d - 1];
        ++L;
    }
    auto drop = [&](int j) {
        for (int i = j; i + 1 < L; ++i) {
            p.cn[i] = p.cn[i + 1];
            for (int k = 0; k < nops; ++k) p.st[k][i] = p.st[k][i + 1];
        }
        --L;
    };
    // rows back to back on every operand: one longer row
    while (L > 0) {
        bool cont = true;
        for (int k = 0; k < nops; ++k) cont = cont && p.st[k][0] == (int64_t)p.row_bytes;
        if (!cont || p.row_bytes * p.cn[0] > (uint64_t)(INT64_MAX / 2)) break;
        p.row_bytes *= p.cn[0];
        drop(0);
    }
    // level j+1 continues level j on every operand: one level
    for (int j = 0; j + 1 < L;) {
        bool cont = (uint64_t)p.cn[j] * p.cn[j + 1] < (1ull << 31);
        for (int k = 0; k < nops; ++k) cont = cont && p.st[k][j + 1] == p.st[k][j] * (int64_t)p.cn[j];
        if (cont) {
            p.cn[j] *= p.cn[j + 1];
            drop(j + 1);
        } else {
            ++j;
        }
    }
    p.L = L;
    p.rows = 1;
    for (int j = 0; j < L; ++j) p.rows *= p.cn[j];
    if (p.rows >= (1ull << 31)) return kPatchErrRange;
    // vector width: the largest power of two <= 16 dividing every base, stride and the row
    uint64_t a = p.row_bytes | 16;
    for (int k = 0; k < nops; ++k) {
        a |= (uint64_t)(uintptr_t)base[k];
        for (int j = 0; j < L; ++j) a |= (uint64_t)p.st[k][j];
    }
    int W = (int)lowbit(a);
    // elements below their natural alignment: one element per vector at dword alignment
    // (as launch_strided); below 4 bytes the launcher refuses
    if (W < p.esz) {
        if (W < 4) return kPatchErrAlign;
        W = p.esz;
    }
    p.W = W;
    // one-wave blocks when every row starts 4 KiB-aligned on every operand, else 128
    // threads (launch_strided's choice for the rows kernels)
    uint64_t al = 0;
    for (int k = 0; k < nops; ++k) {
        al |= (uint64_t)(uintptr_t)base[k];
        for (int j = 0; j < L; ++j) al |= (uint64_t)p.st[k][j];
    }
    p.block = (W == 16 && !(al & 4095)) ? 64 : 128;
    return 0;
}

// byte span [lo, hi) of operand k of a plan
static void plan_span(const PatchPlan &p, int k, const void *base, int64_t &lo, int64_t &hi) {
    lo = hi = (int64_t)(uintptr_t)base;
    for (int j = 0; j < p.L; ++j) {
        const int64_t ext = p.st[k][j] * (int64_t)(p.cn[j] - 1);
        if (ext < 0) lo += ext;
        else hi += ext;
    }
    hi += (int64_t)p.row_bytes;
}

// c may be exactly a (or b): the same base and the same strides; any other overlap of
// c with an input is refused
static bool add_overlap_ok(const PatchPlan &p, const void *const *base) {
    int64_t clo, chi;
    plan_span(p, 0, base[0], clo, chi);
    for (int k = 1; k < 3; ++k) {
        bool same = base[k] == base[0];
        for (int j = 0; j < p.L; ++j) same = same && p.st[k][j] == p.st[0][j];
        if (same) continue;
        int64_t lo, hi;
        plan_span(p, k, base[k], lo, hi);
        if (lo < chi && clo < hi) return false;
    }
    return true;
}

static void fill_desc(PatchDesc &d, const PatchPlan &p, int nops, const void *const *base) {
    memset(&d, 0, sizeof(d));
    for (int k = 0; k < nops; ++k) {
        d.p[k] = (char *)base[k];
        for (int j = 0; j < p.L; ++j) d.str[k][j] = p.st[k][j];
    }
    for (int j = 0; j < kPatchMaxLevels; ++j) d.cnt[j] = make_fastdiv(j < p.L ? p.cn[j] : 1);   // stride 0 beyond L
    d.levels = p.L;
    d.nvec = p.row_bytes / (uint64_t)p.W;
}

template <class OP, int W, int BS, int U>
static hipError_t go_map(PatchDesc d, const PatchPlan &p, const OP &op, hipStream_t st) {
    const uint64_t chunks = (d.nvec + (uint64_t)(BS * U) - 1) / (uint64_t)(BS * U);
    if (chunks > 0x7fffffffull) return hipErrorInvalidValue;
    for (uint64_t r0 = 0; r0 < p.rows; r0 += 65535) {
        const uint64_t nr = p.rows - r0 < 65535 ? p.rows - r0 : 65535;
        d.row0 = (uint32_t)r0;
        if (p.L <= 1)
            hipLaunchKernelGGL((k_patch_map<OP, W, U, BS, 1>), dim3((unsigned)chunks, (unsigned)nr), dim3(BS), 0, st, d,
                               op);
        else
            hipLaunchKernelGGL((k_patch_map<OP, W, U, BS, 0>), dim3((unsigned)chunks, (unsigned)nr), dim3(BS), 0, st, d,
                               op);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// the plan's vector width W (W >= ELEM, the bytes of one element, always) as a compile-time
// constant: f(std::integral_constant<int, W>)
template <int ELEM, class F>
static hipError_t with_width(int W, F &&f) {
    if (W == 16) return f(std::integral_constant<int, 16>());
    if constexpr (ELEM <= 8) {
        if (W == 8) return f(std::integral_constant<int, 8>());
    }
    if constexpr (ELEM <= 4) {
        if (W == 4) return f(std::integral_constant<int, 4>());
    }
    return hipErrorInvalidValue;
}

// the element type a COMEX_ACC_* code names: f(TypeTag<real type, parts>).  The families read
// integers differently: I32 / I64 are unsigned for scale, add, dot, scan, enum and the
// diagonals (wrapping arithmetic), signed for elem, norm and select (ordering, abs).
template <typename T, int NP>
struct TypeTag {
    typedef T real;
    static constexpr int parts = NP, elem = NP * (int)sizeof(T);
};
template <typename I32 = uint32_t, typename I64 = uint64_t, class F>
static hipError_t for_type(int op, F &&f) {
    switch (op) {
    case COMEX_ACC_INT: return f(TypeTag<I32, 1>());
    case COMEX_ACC_DBL: return f(TypeTag<double, 1>());
    case COMEX_ACC_FLT: return f(TypeTag<float, 1>());
    case COMEX_ACC_CPL: return f(TypeTag<float, 2>());
    case COMEX_ACC_DCP: return f(TypeTag<double, 2>());
    case COMEX_ACC_LNG: return f(TypeTag<I64, 1>());
    }
    return hipErrorInvalidValue;
}

// ELEM: bytes of one element (W >= ELEM always).  A store-only operation (fill) has no
// loads to keep in flight: 256-thread blocks of 4 vectors per lane (16 KiB at W = 16).
template <class OP, int ELEM>
static hipError_t go_map_w(const PatchDesc &d, const PatchPlan &p, const OP &op, hipStream_t st) {
    if constexpr (OP::kIn == 0) {
        return with_width<4>(p.W, [&](auto w) { return go_map<OP, decltype(w)::value, 256, 4>(d, p, op, st); });
    } else {   // 16 bytes per lane: 128 threads of 16 / W vectors, or the plan's one-wave blocks at W = 16
        return with_width<ELEM>(p.W, [&](auto w) {
            constexpr int W = decltype(w)::value;
            if (W == 16 && p.block == 64) return go_map<OP, 16, 64, 1>(d, p, op, st);
            return go_map<OP, W, 128, 16 / W>(d, p, op, st);
        });
    }
}

static int rc_of(hipError_t e) { return e == hipSuccess ? 0 : -100 - (int)e; }

template <typename T> static T rd(const void *p, int i = 0) {
    T v;
    memcpy(&v, (const char *)p + (size_t)i * sizeof(T), sizeof(T));
    return v;
}

int launch_patch_fill(int op, const void *value, void *dst, const long long *dst_stride, const long long *count,
                      int ndim, hipStream_t stream) {
    PatchPlan p;
    const void *base[1] = {dst};
    const long long *str[1] = {dst_stride};
    const int rc = patch_plan(op, 1, base, str, count, ndim, p);
    if (rc) return rc < 0 ? rc : 0;
    if (!value) return kPatchErrScalar;
    PatchDesc d;
    fill_desc(d, p, 1, base);
    PatchFill f;
    for (int i = 0; i < 16; i += p.esz) memcpy((char *)&f.pat + i, value, (size_t)p.esz);
    return rc_of(go_map_w<PatchFill, 4>(d, p, f, stream));
}

int launch_patch_scale(int op, const void *alpha, void *dst, const long long *dst_stride, const long long *count,
                       int ndim, hipStream_t stream) {
    PatchPlan p;
    const void *base[1] = {dst};
    const long long *str[1] = {dst_stride};
    const int rc = patch_plan(op, 1, base, str, count, ndim, p);
    if (rc) return rc < 0 ? rc : 0;
    if (!alpha) return kPatchErrScalar;
    PatchDesc d;
    fill_desc(d, p, 1, base);
    return rc_of(for_type(op, [&](auto t) {
        typedef typename decltype(t)::real T;
        constexpr int E = decltype(t)::elem;
        if constexpr (decltype(t)::parts == 1)
            return go_map_w<PatchScaleReal<T>, E>(d, p, PatchScaleReal<T>{rd<T>(alpha)}, stream);
        else
            return go_map_w<PatchScaleCplx<T>, E>(d, p, PatchScaleCplx<T>{rd<T>(alpha), rd<T>(alpha, 1)}, stream);
    }));
}

// the checks of launch_patch_add without a launch (no device needed); plan[0..3] =
// {vector width, row levels after merging, rows, vectors per row}
int plan_patch_add(int op, const void *a, const long long *a_stride, const void *b, const long long *b_stride,
                   const void *c, const long long *c_stride, const long long *count, int ndim, long long plan[4],
                   PatchPlan *out) {
    PatchPlan p;
    const void *base[3] = {c, a, b};
    const long long *str[3] = {c_stride, a_stride, b_stride};
    if (plan) plan[0] = plan[1] = plan[2] = plan[3] = 0;
    const int rc = patch_plan(op, 3, base, str, count, ndim, p);
    if (rc) return rc;
    if (!add_overlap_ok(p, base)) return kPatchErrOverlap;
    if (plan) {
        plan[0] = p.W;
        plan[1] = p.L;
        plan[2] = (long long)p.rows;
        plan[3] = (long long)(p.row_bytes / (uint64_t)p.W);
    }
    if (out) *out = p;
    return 0;
}

int launch_patch_add(int op, const void *alpha, const void *a, const long long *a_stride, const void *beta,
                     const void *b, const long long *b_stride, void *c, const long long *c_stride,
                     const long long *count, int ndim, hipStream_t stream) {
    PatchPlan p;
    const int rc = plan_patch_add(op, a, a_stride, b, b_stride, c, c_stride, count, ndim, nullptr, &p);
    if (rc) return rc < 0 ? rc : 0;
    if (!alpha || !beta) return kPatchErrScalar;
    const void *base[3] = {c, a, b};
    PatchDesc d;
    fill_desc(d, p, 3, base);
    return rc_of(for_type(op, [&](auto t) {
        typedef typename decltype(t)::real T;
        constexpr int E = decltype(t)::elem;
        if constexpr (decltype(t)::parts == 1)
            return go_map_w<PatchAddReal<T>, E>(d, p, PatchAddReal<T>{rd<T>(alpha), rd<T>(beta)}, stream);
        else
            return go_map_w<PatchAddCplx<T>, E>(
                d, p, PatchAddCplx<T>{rd<T>(alpha), rd<T>(alpha, 1), rd<T>(beta), rd<T>(beta, 1)}, stream);
    }));
}

// ---------------------------------------------------------------------------
// dot: per-thread scratch (the partials in HBM, the result in mapped pinned memory),
// grown on demand, freed by patch_release() at comex_finalize.  The pinned block also holds
// what select returns (gaamd_select.hip: the element at 0, its key at kResKey, its index
// at kResIndex) and the zero-divisor flag of RECIP / DIV (kResFlag).
constexpr size_t kResBytes = 128, kResKey = 16, kResIndex = 24, kResFlag = 64;
struct DotScratch {
    int dev = -1;
    void *part = nullptr;
    size_t part_bytes = 0;
    void *res_host = nullptr, *res_dev = nullptr;
};
static std::mutex g_dot_mu;
static std::vector<DotScratch *> g_dot_all;
static thread_local DotScratch *t_dot = nullptr;

static void dot_scratch_free(DotScratch &s) {
    if (s.part) (void)hipFree(s.part);
    if (s.res_host) (void)hipHostFree(s.res_host);
    s = DotScratch();
}

void patch_release() {
    std::lock_guard<std::mutex> g(g_dot_mu);
    for (DotScratch *s : g_dot_all) dot_scratch_free(*s);
}

static DotScratch *dot_scratch(size_t bytes) {
    if (!t_dot) {
        t_dot = new DotScratch();
        std::lock_guard<std::mutex> g(g_dot_mu);
        g_dot_all.push_back(t_dot);
    }
    std::lock_guard<std::mutex> g(g_dot_mu);
    DotScratch &s = *t_dot;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    if (s.dev != dev) dot_scratch_free(s);
    s.dev = dev;
    if (!s.res_host) {
        if (hipHostMalloc(&s.res_host, kResBytes, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess)
            return nullptr;
        if (hipHostGetDevicePointer(&s.res_dev, s.res_host, 0) != hipSuccess) return nullptr;
    }
    if (s.part_bytes < bytes) {
        if (s.part) (void)hipFree(s.part);
        s.part = nullptr;
        s.part_bytes = 0;
        size_t want = 1 << 16;
        while (want < bytes) want <<= 1;
        if (hipMalloc(&s.part, want) != hipSuccess) return nullptr;
        s.part_bytes = want;
    }
    return &s;
}

// The launch of a reduction over a patch (dot; norm in gaamd_matrix.hip, select in
// gaamd_select.hip): the rows in chunks of kDotBS vectors, kDotItems (row, chunk) items per
// workgroup, one partial of `part_bytes` per workgroup in the thread's scratch.
struct PatchReduce {
    PatchDesc d;
    uint32_t items = 0, nwg = 0;
    FastDiv cd;
    DotScratch *s = nullptr;
};

// 0, or the launcher's error code
static int patch_reduce(const PatchPlan &p, int nops, const void *const *base, size_t part_bytes, PatchReduce &r) {
    fill_desc(r.d, p, nops, base);
    const uint64_t chunks = (r.d.nvec + kDotBS - 1) / kDotBS;
    const uint64_t items = chunks * p.rows;
    if (chunks >= (1ull << 31) || items >= (1ull << 31)) return kPatchErrRange;
    r.items = (uint32_t)items;
    r.nwg = (uint32_t)((items + kDotItems - 1) / kDotItems);
    r.s = dot_scratch((size_t)r.nwg * part_bytes);
    if (!r.s) return -100 - (int)hipGetLastError();
    r.cd = make_fastdiv((uint32_t)chunks);
    return 0;
}

// after the launches (`e`: their error): waits for the stream; the pinned result block, or
// null with the error code in rc
static const char *patch_result(const DotScratch *s, hipError_t e, hipStream_t stream, int &rc) {
    if (e == hipSuccess) e = stream ? hipStreamSynchronize(stream) : hipDeviceSynchronize();
    rc = rc_of(e);
    return rc ? nullptr : (const char *)s->res_host;
}

template <class OP, int W>
static hipError_t go_dot(const PatchReduce &r, hipStream_t st) {
    typedef typename OP::acc_t A;
    if (r.d.levels <= 1)
        hipLaunchKernelGGL((k_patch_dot<OP, W, 1>), dim3(r.nwg), dim3(kDotBS), 0, st, r.d, r.items, r.cd, (A *)r.s->part);
    else
        hipLaunchKernelGGL((k_patch_dot<OP, W, 0>), dim3(r.nwg), dim3(kDotBS), 0, st, r.d, r.items, r.cd, (A *)r.s->part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_patch_dot_final<A, OP::kAcc>), dim3(1), dim3(kDotBS), 0, st, (const A *)r.s->part, r.nwg,
                       (A *)r.s->res_dev);
    return hipGetLastError();
}

int launch_patch_dot(int op, const void *a, const long long *a_stride, const void *b, const long long *b_stride,
                     const long long *count, int ndim, void *result, hipStream_t stream) {
    PatchPlan p;
    const void *base[2] = {a, b};
    const long long *str[2] = {a_stride, b_stride};
    const int rc = patch_plan(op, 2, base, str, count, ndim, p);
    if (rc < 0) return rc;
    if (!result) return kPatchErrScalar;
    if (rc == 1) {   // an empty patch: the sum of nothing
        memset(result, 0, (size_t)p.esz);
        return 0;
    }
    PatchReduce r;
    int err = patch_reduce(p, 2, base, 16, r);
    if (err) return err;
    const hipError_t e = for_type(op, [&](auto t) {
        typedef typename decltype(t)::real T;
        typedef std::conditional_t<decltype(t)::parts == 1, PatchDotReal<T>, PatchDotCplx<T>> OP;
        return with_width<decltype(t)::elem>(p.W, [&](auto w) { return go_dot<OP, decltype(w)::value>(r, stream); });
    });
    const char *res = patch_result(r.s, e, stream, err);
    if (res) memcpy(result, res, (size_t)p.esz);
    return err;
}

// ---------------------------------------------------------------------------
// element-wise algebra: the map kernel with the operations above
template <class F, int KIN>
static hipError_t go_elem(int op, const PatchDesc &d, const PatchPlan &p, const void *s, uint32_t *flag,
                          hipStream_t st) {
    const double zero[2] = {0.0, 0.0};
    if (!s) s = zero;
    return for_type<int32_t, int64_t>(op, [&](auto t) {
        typedef typename decltype(t)::real T;
        constexpr int E = decltype(t)::elem;
        if constexpr (decltype(t)::parts == 1)
            return go_map_w<PatchElemReal<F, T, KIN>, E>(d, p, PatchElemReal<F, T, KIN>{rd<T>(s), flag}, st);
        else
            return go_map_w<PatchElemCplx<F, T, KIN>, E>(d, p, PatchElemCplx<F, T, KIN>{rd<T>(s), rd<T>(s, 1), flag}, st);
    });
}

// RECIP and DIV: the flag word cleared before the launch, read after the stream has finished
template <class F, int KIN>
static int go_elem_checked(int op, const PatchDesc &d, const PatchPlan &p, hipStream_t stream) {
    DotScratch *s = dot_scratch(0);
    if (!s) return -100 - (int)hipGetLastError();
    volatile uint32_t *flag = (volatile uint32_t *)((char *)s->res_host + kResFlag);
    *flag = 0;
    const hipError_t e = go_elem<F, KIN>(op, d, p, nullptr, (uint32_t *)((char *)s->res_dev + kResFlag), stream);
    int rc;
    if (!patch_result(s, e, stream, rc)) return rc;
    return *flag ? kPatchZeroDivisor : 0;
}

int launch_patch_elem1(int op, int fn, const void *scalar, void *dst, const long long *dst_stride,
                       const long long *count, int ndim, hipStream_t stream) {
    PatchPlan p;
    const void *base[1] = {dst};
    const long long *str[1] = {dst_stride};
    const int rc = patch_plan(op, 1, base, str, count, ndim, p);
    if (rc < 0) return rc;
    if (fn != kElemAbs && fn != kElemAddConst && fn != kElemRecip) return kPatchErrOp;
    if (rc) return 0;
    if (fn == kElemAddConst && !scalar) return kPatchErrScalar;
    PatchDesc d;
    fill_desc(d, p, 1, base);
    switch (fn) {
    case kElemAbs: return rc_of(go_elem<ElAbs, 1>(op, d, p, nullptr, nullptr, stream));
    case kElemAddConst: return rc_of(go_elem<ElAddConst, 1>(op, d, p, scalar, nullptr, stream));
    default: return go_elem_checked<ElRecip, 1>(op, d, p, stream);
    }
}

int launch_patch_elem2(int op, int fn, const void *a, const long long *a_stride, const void *b,
                       const long long *b_stride, void *c, const long long *c_stride, const long long *count,
                       int ndim, hipStream_t stream) {
    PatchPlan p;
    const int rc = plan_patch_add(op, a, a_stride, b, b_stride, c, c_stride, count, ndim, nullptr, &p);
    if (rc < 0) return rc;
    if (fn != kElemMul && fn != kElemDiv && fn != kElemMax && fn != kElemMin) return kPatchErrOp;
    if (rc) return 0;
    const void *base[3] = {c, a, b};
    PatchDesc d;
    fill_desc(d, p, 3, base);
    switch (fn) {
    case kElemMul: return rc_of(go_elem<ElMul, 2>(op, d, p, nullptr, nullptr, stream));
    case kElemMax: return rc_of(go_elem<ElMaxMin<true>, 2>(op, d, p, nullptr, nullptr, stream));
    case kElemMin: return rc_of(go_elem<ElMaxMin<false>, 2>(op, d, p, nullptr, nullptr, stream));
    default: return go_elem_checked<ElDiv, 2>(op, d, p, stream);
    }
}

}  // namespace gaamd
