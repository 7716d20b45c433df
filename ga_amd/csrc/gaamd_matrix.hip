// gaamd_matrix.hip -- the kernels under GA's matrix.c calls (ga_amd.h gaamd_patch_norm,
// gaamd_diagonal, gaamd_scale_rows, gaamd_scale_cols; ga.h GA_Norm1 / GA_Norm_infinity, the
// diagonal calls, GA_Scale_rows / GA_Scale_cols).  Compiled as part of gaamd_all.hip after
// gaamd_patch.hip, whose descriptor, row decode, plan, reduction and per-thread scratch it
// shares.
//
// Reference arithmetic (global/src/matrix.c), expression for expression:
//   norm1      sum += GA_ABS(x); complex sum += sqrt(re*re + im*im)          1118-1171
//   norm inf   the maximum of the same per-element quantity                   801-859
//   add diag   a += v; complex real and imaginary part each                   1640-1690
//   shift diag a += c; complex real and imaginary part each                   2080-2127
//   scale      a *= v; complex re *= v.re, im *= v.im -- part by part, NOT a complex
//              product                                                         2494-2503, 2700-2710
// Integers in unsigned arithmetic (two's-complement wraparound).  FP contraction is off.
//
// NORM: k_patch_dot's work split and reduction with one operand -- item = (row, chunk of
// kDotBS vectors), kDotItems items per workgroup, every load issued first; lane, wave tree,
// waves in order, one partial per workgroup, k_patch_dot_final over the partials.  ONE adds
// in the element's own type.  INF reduces with max instead of +: its accumulator is NormMax,
// whose operator+ is the maximum, so block_sum_store and k_patch_dot_final are used as they
// are.  NormMax holds the per-element quantity q as the unsigned key bits(q) ^ signbit: for
// q >= +0, for -0.0 and for the signed integers the keys order as the values do (-0.0 and
// INT_MIN map to key 0, below +0), so the maximum does not depend on the order it is taken
// in, and key 0 -- what zero-initialisation gives -- is the identity.
// DIAGONAL: one lane per element, 64-bit byte steps on both sides.
// SCALE: the map kernel's streaming shape (grid = chunks of a row x rows of this launch,
// non-temporal loads and stores of `a`, the row decode wave-uniform) with a second vector of
// multipliers: for rows the row's own v element repeated over the vector (uniform per
// workgroup), for cols v's vector at the same position, read with an ordinary cached load
// because every row reads it again.  The product is taken part by part, which is the real
// product for the real types and the reference's expression for the complex ones.
#pragma clang fp contract(off)

namespace gaamd {

// ---------------------------------------------------------------------------
// norms
template <typename U>
struct NormMax {   // a maximum that block_sum_store / k_patch_dot_final reduce with `+`
    U key;
    __device__ __forceinline__ NormMax operator+(const NormMax o) const { return NormMax{key > o.key ? key : o.key}; }
};

template <typename T>
__device__ __forceinline__ auto norm_key(T q) {
    typedef typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type U;
    U b;
    memcpy(&b, &q, sizeof(T));
    return b ^ ((U)1 << (8 * sizeof(T) - 1));
}

// the per-element quantity: GA_ABS for the real and integer types, the modulus for complex
// (two products, one sum, the correctly rounded square root; for float through double, which
// rounds to the same float)
template <typename R> __device__ __forceinline__ R norm_modulus(R re, R im) {
    R p1 = re * re;
    R p2 = im * im;
    R s = p1 + p2;
    if constexpr (sizeof(R) == 4) return (R)__builtin_sqrt((double)s);
    else return __builtin_sqrt(s);
}

// T: the element (complex: its real type R with CPLX); A: the accumulator
template <typename T, bool CPLX, bool INF>
struct PatchNorm {
    typedef typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type U;
    typedef typename std::conditional<INF, NormMax<U>, typename std::conditional<std::is_integral<T>::value, U, T>::type>::type
        acc_t;
    static constexpr int kAcc = 1;
    __device__ __forceinline__ static void one(acc_t &acc, T q) {
        if constexpr (INF) acc = acc + acc_t{norm_key(q)};
        else acc = acc + (acc_t)q;   // integers: unsigned wraparound
    }
    template <int W>
    __device__ __forceinline__ static void accum(acc_t (&acc)[1], typename Vec<W>::T av) {
        constexpr int N = W / (int)sizeof(T);
        union { typename Vec<W>::T v; T t[N]; } a;
        a.v = av;
        if constexpr (CPLX) {
#pragma unroll
            for (int i = 0; i < N / 2; ++i) one(acc[0], norm_modulus(a.t[2 * i], a.t[2 * i + 1]));
        } else {
#pragma unroll
            for (int i = 0; i < N; ++i) one(acc[0], el_abs(a.t[i]));
        }
    }
};

template <class OP, int W, int LV>
__global__ __launch_bounds__(kDotBS) void k_patch_norm(const PatchDesc d, const uint32_t items, const FastDiv chunk_div,
                                                       typename OP::acc_t *part) {
    typedef typename Vec<W>::T V;
    typedef typename OP::acc_t A;
    V va[kDotItems];
    bool ok[kDotItems];
    const uint32_t i0 = blockIdx.x * (uint32_t)kDotItems;
    // every load first and without a branch (k_patch_dot): a lane without a vector in an item
    // reads vector 0 of a row of the patch instead and drops it below
#pragma unroll
    for (int k = 0; k < kDotItems; ++k) {
        const bool in = i0 + k < items;
        const uint32_t it = in ? i0 + k : 0u;
        const uint32_t rl = chunk_div.div(it);
        const uint32_t chunk = it - rl * chunk_div.d;
        int64_t off[1];
        patch_row<1, LV>(d, rl, off);
        const uint64_t v = (uint64_t)chunk * kDotBS + threadIdx.x;
        ok[k] = in && v < d.nvec;
        const int64_t b = ok[k] ? (int64_t)(v * W) : 0;
        va[k] = vload<W, true>(d.p[0] + off[0] + b);
    }
    A acc[1] = {};
#pragma unroll
    for (int k = 0; k < kDotItems; ++k)
        if (ok[k]) OP::template accum<W>(acc, va[k]);
    block_sum_store<A, 1, false>(acc, part + blockIdx.x);
}

template <class OP, int W>
static hipError_t go_norm(const PatchReduce &r, hipStream_t st) {
    typedef typename OP::acc_t A;
    if (r.d.levels <= 1)
        hipLaunchKernelGGL((k_patch_norm<OP, W, 1>), dim3(r.nwg), dim3(kDotBS), 0, st, r.d, r.items, r.cd, (A *)r.s->part);
    else
        hipLaunchKernelGGL((k_patch_norm<OP, W, 0>), dim3(r.nwg), dim3(kDotBS), 0, st, r.d, r.items, r.cd, (A *)r.s->part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_patch_dot_final<A, 1>), dim3(1), dim3(kDotBS), 0, st, (const A *)r.s->part, r.nwg,
                       (A *)r.s->res_dev);
    return hipGetLastError();
}

template <typename T, bool CPLX, int ELEM>
static hipError_t go_norm_w(bool inf, int W, const PatchReduce &r, hipStream_t st) {
    return with_width<ELEM>(W, [&](auto w) {
        constexpr int VW = decltype(w)::value;
        return inf ? go_norm<PatchNorm<T, CPLX, true>, VW>(r, st) : go_norm<PatchNorm<T, CPLX, false>, VW>(r, st);
    });
}

int launch_patch_norm(int op, int kind, const void *a, const long long *a_stride, const long long *count, int ndim,
                      void *result, hipStream_t stream) {
    PatchPlan p;
    const void *base[1] = {a};
    const long long *str[1] = {a_stride};
    const int rc = patch_plan(op, 1, base, str, count, ndim, p);
    if (rc < 0) return rc;
    if (kind != kNormOne && kind != kNormInf) return kPatchErrOp;
    if (!result) return kPatchErrScalar;
    const int rsz = op == COMEX_ACC_CPL ? 4 : op == COMEX_ACC_DCP ? 8 : p.esz;   // complex: the real type
    if (rc == 1) {   // an empty patch: the norm of nothing
        memset(result, 0, (size_t)rsz);
        return 0;
    }
    PatchReduce r;
    int err = patch_reduce(p, 1, base, 8, r);
    if (err) return err;
    const bool inf = kind == kNormInf;
    const hipError_t e = for_type<int32_t, int64_t>(op, [&](auto t) {
        typedef decltype(t) T;
        return go_norm_w<typename T::real, T::parts == 2, T::elem>(inf, p.W, r, stream);
    });
    const char *res = patch_result(r.s, e, stream, err);
    if (!res) return err;
    if (inf) {   // the key back to the value's bits
        if (rsz == 4) {
            const uint32_t b = rd<uint32_t>(res) ^ 0x80000000u;
            memcpy(result, &b, 4);
        } else {
            const uint64_t b = rd<uint64_t>(res) ^ 0x8000000000000000ull;
            memcpy(result, &b, 8);
        }
    } else {
        memcpy(result, res, (size_t)rsz);
    }
    return 0;
}

// ---------------------------------------------------------------------------
// diagonal: element i of the matrix side at a + i * a_step, of the vector side at
// v + i * v_step.  An element is NP parts of type P and moves in pieces of CW bytes: the
// whole element where both sides are aligned to it, its parts otherwise.
struct DiagDesc {
    char *a, *v;
    int64_t a_step, v_step;
    uint64_t n;
    int32_t fn;
    Scale16 s;   // SHIFT: the constant
};

template <typename P, int NP, int CW>
__global__ __launch_bounds__(256) void k_diagonal(const DiagDesc d) {
    constexpr int E = NP * (int)sizeof(P), NC = E / CW;
    typedef typename Vec<CW>::T C;
    union El { C c[NC]; P t[NP]; };
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= d.n) return;
    char *pa = d.a + (int64_t)i * d.a_step;
    char *pv = d.v + (int64_t)i * d.v_step;
    El x, y;
    switch (d.fn) {   // uniform
    case kDiagGet:
#pragma unroll
        for (int k = 0; k < NC; ++k) vstore<CW, false>(pv + k * CW, vload<CW, false>(pa + k * CW));
        break;
    case kDiagSet:
#pragma unroll
        for (int k = 0; k < NC; ++k) vstore<CW, false>(pa + k * CW, vload<CW, false>(pv + k * CW));
        break;
    case kDiagZero:
#pragma unroll
        for (int k = 0; k < NC; ++k) vstore<CW, false>(pa + k * CW, C{});
        break;
    default:   // ADD, SHIFT
#pragma unroll
        for (int k = 0; k < NC; ++k) x.c[k] = vload<CW, false>(pa + k * CW);
        if (d.fn == kDiagAdd) {
#pragma unroll
            for (int k = 0; k < NC; ++k) y.c[k] = vload<CW, false>(pv + k * CW);
        } else {
            union { Scale16 s; El e; } u;
            u.s = d.s;
            y = u.e;
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) x.t[k] = x.t[k] + y.t[k];
#pragma unroll
        for (int k = 0; k < NC; ++k) vstore<CW, false>(pa + k * CW, x.c[k]);
        break;
    }
}

template <typename P, int NP>
static hipError_t go_diagonal(const DiagDesc &d, bool whole, hipStream_t st) {
    const unsigned nb = (unsigned)((d.n + 255) / 256);
    constexpr int E = NP * (int)sizeof(P);
    if (whole) hipLaunchKernelGGL((k_diagonal<P, NP, E>), dim3(nb), dim3(256), 0, st, d);
    else hipLaunchKernelGGL((k_diagonal<P, NP, (int)sizeof(P)>), dim3(nb), dim3(256), 0, st, d);
    return hipGetLastError();
}

// byte span [lo, hi) of n elements of esz bytes, `step` apart
static void step_span(const void *base, int64_t step, int64_t n, int esz, int64_t &lo, int64_t &hi) {
    lo = hi = (int64_t)(uintptr_t)base;
    const int64_t ext = step * (n - 1);
    if (ext < 0) lo += ext;
    else hi += ext;
    hi += esz;
}

int launch_diagonal(int op, int fn, long long n, void *a, long long a_step, void *v, long long v_step,
                    const void *scalar, hipStream_t stream) {
    const int esz = (op == kOpCopy) ? 0 : elem_size(op);
    if (!esz || fn < kDiagGet || fn > kDiagZero) return kPatchErrOp;
    if (n < 0) return kPatchErrCount;
    if (n >= (1ll << 39)) return kPatchErrRange;   // 2^31 workgroups of 256
    const bool uses_v = fn == kDiagGet || fn == kDiagSet || fn == kDiagAdd;
    if (!a || (uses_v && !v) || (fn == kDiagShift && !scalar)) return kPatchErrScalar;
    uint64_t al = (uint64_t)(uintptr_t)a | (uint64_t)a_step;
    if (uses_v) al |= (uint64_t)(uintptr_t)v | (uint64_t)v_step;
    if (al & 3) return kPatchErrAlign;
    if (uses_v && n > 0) {
        int64_t alo, ahi, vlo, vhi;
        step_span(a, a_step, n, esz, alo, ahi);
        step_span(v, v_step, n, esz, vlo, vhi);
        if (alo < vhi && vlo < ahi) return kPatchErrOverlap;
    }
    if (n == 0) return 0;
    DiagDesc d;
    memset(&d, 0, sizeof(d));
    d.a = (char *)a;
    d.v = uses_v ? (char *)v : (char *)a;
    d.a_step = a_step;
    d.v_step = uses_v ? v_step : 0;
    d.n = (uint64_t)n;
    d.fn = fn;
    if (fn == kDiagShift) memcpy(&d.s, scalar, (size_t)esz);
    const bool whole = !(al & (uint64_t)(esz - 1));
    return rc_of(for_type(op, [&](auto t) {   // a one-part element is always moved whole
        typedef decltype(t) T;
        return go_diagonal<typename T::real, T::parts>(d, T::parts == 1 || whole, stream);
    }));
}

// ---------------------------------------------------------------------------
// scale rows / columns of a row-major matrix in place
struct ScaleRcDesc {
    char *a;
    const char *v;
    int64_t lda;       // bytes between rows
    uint64_t nvec;     // W-byte vectors per row
    uint32_t row0;     // first row of this launch
    int32_t esz;       // bytes of one element (rows: the multiplier repeats with this period)
};

template <typename P, int W>
__device__ __forceinline__ typename Vec<W>::T scale_parts(typename Vec<W>::T xv, typename Vec<W>::T mv) {
    constexpr int N = W / (int)sizeof(P);
    union { typename Vec<W>::T v; P t[N]; } x, m;
    x.v = xv;
    m.v = mv;
#pragma unroll
    for (int i = 0; i < N; ++i) x.t[i] = x.t[i] * m.t[i];
    return x.v;
}

// block (x, y) = chunk x of row row0 + y
template <typename P, int W, int U, int BS, bool COLS>
__global__ __launch_bounds__(BS) void k_scale_rc(const ScaleRcDesc d) {
    typedef typename Vec<W>::T V;
    const uint32_t row = d.row0 + blockIdx.y;
    const uint64_t c0 = (uint64_t)blockIdx.x * (uint64_t)(BS * U);
    const int64_t b0 = (int64_t)((c0 + threadIdx.x) * (uint64_t)W);
    char *o = d.a + (int64_t)row * d.lda + b0;
    const char *vc = d.v + b0;
    V mrow = V{};
    if constexpr (!COLS) {   // the row's element over the vector: uniform per workgroup
        const uint32_t *e = reinterpret_cast<const uint32_t *>(d.v + (int64_t)row * d.esz);
        union { V v; uint32_t w[W / 4]; } m;
        const int mask = d.esz / 4 - 1;
#pragma unroll
        for (int c = 0; c < W / 4; ++c) m.w[c] = e[c & mask];
        mrow = m.v;
    }
    V x[U], m[U];
    if (c0 + (uint64_t)(BS * U) <= d.nvec) {   // wave-uniform: the whole chunk lies inside the row
#pragma unroll
        for (int k = 0; k < U; ++k) {
            x[k] = vload<W, true>(o + (int64_t)k * BS * W);
            if constexpr (COLS) m[k] = vload<W, false>(vc + (int64_t)k * BS * W);
            else m[k] = mrow;
        }
#pragma unroll
        for (int k = 0; k < U; ++k) vstore<W, true>(o + (int64_t)k * BS * W, scale_parts<P, W>(x[k], m[k]));
        return;
    }
    for (int k = 0; k < U; ++k) {   // row tail: one vector at a time
        if (c0 + threadIdx.x + (uint64_t)k * BS >= d.nvec) continue;
        V mm = mrow;
        if constexpr (COLS) mm = vload<W, false>(vc + (int64_t)k * BS * W);
        vstore<W, true>(o + (int64_t)k * BS * W, scale_parts<P, W>(vload<W, true>(o + (int64_t)k * BS * W), mm));
    }
}

template <typename P, int W, int BS, int U>
static hipError_t go_scale_rc(ScaleRcDesc d, uint64_t rows, bool cols, hipStream_t st) {
    const uint64_t chunks = (d.nvec + (uint64_t)(BS * U) - 1) / (uint64_t)(BS * U);
    if (chunks > 0x7fffffffull) return hipErrorInvalidValue;
    for (uint64_t r0 = 0; r0 < rows; r0 += 65535) {   // as go_map
        const uint64_t nr = rows - r0 < 65535 ? rows - r0 : 65535;
        d.row0 = (uint32_t)r0;
        if (cols)
            hipLaunchKernelGGL((k_scale_rc<P, W, U, BS, true>), dim3((unsigned)chunks, (unsigned)nr), dim3(BS), 0, st, d);
        else
            hipLaunchKernelGGL((k_scale_rc<P, W, U, BS, false>), dim3((unsigned)chunks, (unsigned)nr), dim3(BS), 0, st, d);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// go_map_w's shapes for an operation that loads its output
template <typename P>
static hipError_t go_scale_rc_w(int W, int block, const ScaleRcDesc &d, uint64_t rows, bool cols, hipStream_t st) {
    return with_width<(int)sizeof(P)>(W, [&](auto w) {
        constexpr int VW = decltype(w)::value;
        if (VW == 16 && block == 64) return go_scale_rc<P, 16, 64, 1>(d, rows, cols, st);
        return go_scale_rc<P, VW, 128, 16 / VW>(d, rows, cols, st);
    });
}

int launch_scale_rc(int op, bool cols, long long rows, long long ncols, void *a, long long lda, const void *v,
                    hipStream_t stream) {
    const int esz = (op == kOpCopy) ? 0 : elem_size(op);
    if (!esz) return kPatchErrOp;
    if (rows < 0 || ncols < 0) return kPatchErrCount;
    if (lda < ncols) return kPatchErrStride;
    if (rows == 0 || ncols == 0) return 0;
    if (!v) return kPatchErrScalar;
    if (rows >= (1ll << 31) || ncols > (long long)(INT64_MAX / 32) || lda > (long long)(INT64_MAX / 32))
        return kPatchErrRange;
    const uint64_t row_bytes = (uint64_t)ncols * (uint64_t)esz, lda_b = (uint64_t)lda * (uint64_t)esz;
    // vector width: the largest power of two <= 16 dividing the base, the row step, the row
    // length and, for cols, v's base (its vectors are loaded beside a's)
    uint64_t al = (uint64_t)(uintptr_t)a | (rows > 1 ? lda_b : 0);
    uint64_t w = al | row_bytes | 16 | (cols ? (uint64_t)(uintptr_t)v : 0);
    int W = (int)lowbit(w);
    if (((uintptr_t)v | (uintptr_t)a) & 3) return kPatchErrAlign;
    if (W < esz) W = esz;   // elements below their natural alignment: one per vector (patch_plan)
    const int64_t alo = (int64_t)(uintptr_t)a, ahi = alo + (int64_t)((uint64_t)(rows - 1) * lda_b + row_bytes);
    const int64_t vlo = (int64_t)(uintptr_t)v, vhi = vlo + (int64_t)((uint64_t)(cols ? ncols : rows) * (uint64_t)esz);
    if (alo < vhi && vlo < ahi) return kPatchErrOverlap;
    ScaleRcDesc d;
    memset(&d, 0, sizeof(d));
    d.a = (char *)a;
    d.v = (const char *)v;
    d.lda = (int64_t)lda_b;
    d.nvec = row_bytes / (uint64_t)W;
    d.esz = esz;
    const int block = (W == 16 && !(al & 4095)) ? 64 : 128;
    return rc_of(for_type(op, [&](auto t) {   // complex part by part: only the real type matters
        return go_scale_rc_w<typename decltype(t)::real>(W, block, d, (uint64_t)rows, cols, stream);
    }));
}

}  // namespace gaamd
