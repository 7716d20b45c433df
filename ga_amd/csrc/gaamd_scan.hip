// gaamd_scan.hip -- the kernels under GA's sparse.c calls (ga_amd.h gaamd_enum, gaamd_scan_tail,
// gaamd_scan, gaamd_mask_count, gaamd_mask_pack, gaamd_mask_unpack; ga.h GA_Patch_enum,
// GA_Scan_copy, GA_Scan_add, GA_Pack, GA_Unpack).  Compiled as part of gaamd_all.hip after
// gaamd_patch.hip, whose per-thread scratch (dot_scratch) it shares.
//
// Reference arithmetic (global/src/sparse.c), expression for expression:
//   enum       offset = (off + i) * stride; a[i] = start + offset; complex part by part   59-76
//   mask test  neq_zero_reg / neq_zero_cpl of abstract_ops.h: x != 0, complex either part
//   scan copy  last = msk[i] ? src[i] : last; dst[i] = last; zero before the first set     196-206
//   scan add   a segment starts at every set element; inclusive or exclusive               361-406
//   pack       the set elements of src in order; unpack the inverse                        528-533, 590-601
// Integers in unsigned arithmetic (two's-complement wraparound).  FP contraction is off.
//
// SHAPE: reduce, then scan -- three launches, no workgroup ever waits for another, no atomics.
//   1  k_scan_reduce / k_mask_count   one workgroup per tile of kScanTile elements: the tile's
//                                     aggregate (flag, value) -- for the compaction (0, set count)
//   2  k_scan_aggs                    ONE workgroup scans the aggregates in tile order, kScanAggSpan
//                                     of them per pass of its loop, and leaves each tile's exclusive
//                                     prefix in their place (and the grand total for the host)
//   3  k_scan_write / k_mask_move     one workgroup per tile redoes its tile from its prefix and writes
// The combine is (f1, v1) (+) (f2, v2) = (f1 | f2, f2 ? v2 : v1 + v2) for ADD and
// (f1 | f2, f2 ? v2 : v1) for COPY; both are associative.  An open segment on entry is the
// pair (1, carry) in front of tile 0.
//
// SUMMATION ORDER (block_scan; the contract of ga_amd.h): a lane folds its K consecutive
// elements left to right; the 64 lanes of a wave are scanned by the Hillis-Steele steps 1, 2, 4,
// 8, 16, 32 (lane l takes lane l - step on its left); the four waves of a workgroup are taken in
// order; the tiles are scanned by the same procedure with K = kScanAggK aggregates per lane and
// the passes of the loop in order.  An element's result is
//   ((((carry-in (+) tiles before) (+) waves before) (+) lanes before) (+) elements before) (+) x.
// The identity is (0, -0.0) -- -0.0 + x has the bits of x for every x -- and 0 for integers, so
// positions past n and empty prefixes change no bit.
//
// ACCESS: a lane's K consecutive elements are K * E >= 32 contiguous bytes, moved as 16-byte
// vectors where the base is 16-byte aligned and as 8- or 4-byte ones otherwise (the width is
// the same for every lane: lowbit(base | 16)); the last, partial tile and a lane with
// unwritten elements go element by element in 4-byte words.
#pragma clang fp contract(off)

namespace gaamd {

constexpr int kScanBS = 256;                       // lanes of every workgroup here
constexpr int kScanK = 8;                          // consecutive elements per lane
constexpr int kScanTile = kScanBS * kScanK;        // 2048 elements: 8 / 16 / 32 KiB of src
constexpr int kScanAggK = 4;                       // aggregates per lane of the aggregate scan
constexpr int kScanAggSpan = kScanBS * kScanAggK;  // tiles per pass of its loop
constexpr long long kScanMaxN = 1ll << 34;         // 2^23 tiles: 160 MiB of aggregates at most

template <typename P, int NP>
struct SVal {
    P t[NP];
};

template <typename P>
__device__ __forceinline__ P scan_ident() {
    if constexpr (std::is_floating_point<P>::value) return (P)-0.0;
    else return (P)0;
}
template <typename P, int NP>
__device__ __forceinline__ SVal<P, NP> scan_ident_v() {
    SVal<P, NP> v;
#pragma unroll
    for (int k = 0; k < NP; ++k) v.t[k] = scan_ident<P>();
    return v;
}

// a = a (+) b, a the earlier
template <typename P, int NP, bool ADD>
__device__ __forceinline__ void scan_comb(uint32_t &fa, SVal<P, NP> &va, uint32_t fb, const SVal<P, NP> &vb) {
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if constexpr (ADD) {
            const P s = va.t[k] + vb.t[k];
            va.t[k] = fb ? vb.t[k] : s;
        } else {
            va.t[k] = fb ? vb.t[k] : va.t[k];
        }
    }
    fa |= fb;
}

template <typename V>
__device__ __forceinline__ V scan_shfl_up(const V &v, int step) {
    constexpr int NW = (int)sizeof(V) / 4;
    union { V v; uint32_t w[NW]; } a, b;
    a.v = v;
#pragma unroll
    for (int k = 0; k < NW; ++k) b.w[k] = (uint32_t)__shfl_up((int)a.w[k], step, 64);
    return b.v;
}

template <typename P, int NP>
struct ScanShared {
    SVal<P, NP> v[kScanBS / 64];
    uint32_t f[kScanBS / 64];
};

// The workgroup's scan of kScanBS * K pairs, lane l holding pairs l * K .. l * K + K - 1 (flag
// of pair k = bit k of flags).  (ef, ev): the combination of every pair before the lane's first;
// (tf, tv): of all pairs.  Ends with a barrier, so sh may be used again at once.
template <typename P, int NP, bool ADD, int K>
__device__ __forceinline__ void block_scan(uint32_t flags, const SVal<P, NP> (&x)[K], ScanShared<P, NP> &sh, uint32_t &ef,
                                           SVal<P, NP> &ev, uint32_t &tf, SVal<P, NP> &tv) {
    typedef SVal<P, NP> V;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t f = 0;
    V v = scan_ident_v<P, NP>();
#pragma unroll
    for (int k = 0; k < K; ++k) scan_comb<P, NP, ADD>(f, v, (flags >> k) & 1u, x[k]);
#pragma unroll
    for (int step = 1; step < 64; step <<= 1) {
        uint32_t pf = (uint32_t)__shfl_up((int)f, step, 64);
        V pv = scan_shfl_up(v, step);
        scan_comb<P, NP, ADD>(pf, pv, f, v);
        if (lane >= step) {
            f = pf;
            v = pv;
        }
    }
    if (lane == 63) {
        sh.f[wave] = f;
        sh.v[wave] = v;
    }
    __syncthreads();
    uint32_t wf = 0, af = 0;
    V wv = scan_ident_v<P, NP>(), av = wv;
#pragma unroll
    for (int w = 0; w < kScanBS / 64; ++w) {
        if (w == wave) {
            wf = af;
            wv = av;
        }
        scan_comb<P, NP, ADD>(af, av, sh.f[w], sh.v[w]);
    }
    tf = af;
    tv = av;
    const uint32_t pf = (uint32_t)__shfl_up((int)f, 1, 64);
    const V pv = scan_shfl_up(v, 1);
    ef = wf;
    ev = wv;
    if (lane > 0) scan_comb<P, NP, ADD>(ef, ev, pf, pv);
    __syncthreads();
}

// ---------------------------------------------------------------------------
// loads and stores of a lane's run
template <int BYTES>
__device__ __forceinline__ void ld_run(const char *p, int w, uint32_t (&out)[BYTES / 4]) {
    if (w == 16) {
#pragma unroll
        for (int j = 0; j < BYTES / 16; ++j) {
            union { Vec<16>::T v; uint32_t t[4]; } u;
            u.v = vload<16, false>(p + 16 * j);
#pragma unroll
            for (int c = 0; c < 4; ++c) out[4 * j + c] = u.t[c];
        }
    } else if (w == 8) {
#pragma unroll
        for (int j = 0; j < BYTES / 8; ++j) {
            union { Vec<8>::T v; uint32_t t[2]; } u;
            u.v = vload<8, false>(p + 8 * j);
            out[2 * j] = u.t[0];
            out[2 * j + 1] = u.t[1];
        }
    } else {
#pragma unroll
        for (int j = 0; j < BYTES / 4; ++j) out[j] = vload<4, false>(p + 4 * j);
    }
}

template <int BYTES>
__device__ __forceinline__ void st_run(char *p, int w, const uint32_t (&in)[BYTES / 4]) {
    if (w == 16) {
#pragma unroll
        for (int j = 0; j < BYTES / 16; ++j) {
            union { Vec<16>::T v; uint32_t t[4]; } u;
#pragma unroll
            for (int c = 0; c < 4; ++c) u.t[c] = in[4 * j + c];
            vstore<16, true>(p + 16 * j, u.v);
        }
    } else if (w == 8) {
#pragma unroll
        for (int j = 0; j < BYTES / 8; ++j) {
            union { Vec<8>::T v; uint32_t t[2]; } u;
            u.t[0] = in[2 * j];
            u.t[1] = in[2 * j + 1];
            vstore<8, true>(p + 8 * j, u.v);
        }
    } else {
#pragma unroll
        for (int j = 0; j < BYTES / 4; ++j) vstore<4, true>(p + 4 * j, in[j]);
    }
}

// K elements of E bytes from element i0 on; positions at and past n read nothing and give `fill`
template <int E, int K>
__device__ __forceinline__ void ld_elems(const char *base, uint64_t i0, uint64_t n, int w, uint32_t fill,
                                         uint32_t (&out)[K * E / 4]) {
    constexpr int NW = E / 4;
    if (i0 + K <= n) {
        ld_run<K * E>(base + (int64_t)(i0 * (uint64_t)E), w, out);
        return;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const bool in = i0 + k < n;
        const uint32_t *p = reinterpret_cast<const uint32_t *>(base + (int64_t)((in ? i0 + k : 0) * (uint64_t)E));
#pragma unroll
        for (int j = 0; j < NW; ++j) out[k * NW + j] = in ? p[j] : fill;
    }
}

struct ScanDesc {
    const char *src, *msk;
    char *dst;
    uint64_t n;
    int32_t sw, mw, dw;   // vector width of the src / msk / dst runs
    int32_t me;           // bytes of a mask element
    uint32_t msign;       // bit j: word j of a mask element carries a sign bit, which the test ignores
    int32_t fn;
};

// bit k: mask element i0 + k is set (x != 0; -0.0 is not, a NaN is; complex: either part)
template <int ME, int K>
__device__ __forceinline__ uint32_t mask_flags_e(const ScanDesc &d, uint64_t i0) {
    constexpr int NW = ME / 4;
    uint32_t w[K * NW];
    ld_elems<ME, K>(d.msk, i0, d.n, d.mw, 0u, w);
    uint32_t flags = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        uint32_t any = 0;
#pragma unroll
        for (int j = 0; j < NW; ++j) any |= w[k * NW + j] & (((d.msign >> j) & 1u) ? 0x7fffffffu : 0xffffffffu);
        flags |= (any ? 1u : 0u) << k;
    }
    return flags;
}

template <int K>
__device__ __forceinline__ uint32_t mask_flags(const ScanDesc &d, uint64_t i0) {
    if (i0 >= d.n) return 0;
    switch (d.me) {   // uniform
    case 4: return mask_flags_e<4, K>(d, i0);
    case 8: return mask_flags_e<8, K>(d, i0);
    default: return mask_flags_e<16, K>(d, i0);
    }
}

template <typename P, int NP, int K>
__device__ __forceinline__ void ld_vals(const ScanDesc &d, uint64_t i0, SVal<P, NP> (&x)[K]) {
    constexpr int E = NP * (int)sizeof(P);
    union { uint32_t w[K * E / 4]; SVal<P, NP> v[K]; } u;
    if (i0 + K <= d.n) {
        ld_run<K * E>(d.src + (int64_t)(i0 * (uint64_t)E), d.sw, u.w);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (i0 + k < d.n) {
                const uint32_t *p = reinterpret_cast<const uint32_t *>(d.src + (int64_t)((i0 + k) * (uint64_t)E));
#pragma unroll
                for (int j = 0; j < E / 4; ++j) u.w[k * (E / 4) + j] = p[j];
            } else {
                u.v[k] = scan_ident_v<P, NP>();
            }
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = u.v[k];
}

// ---------------------------------------------------------------------------
// 1: a tile's aggregate
template <typename P, int NP, bool ADD>
__global__ __launch_bounds__(kScanBS) void k_scan_reduce(const ScanDesc d, uint32_t *aggf, SVal<P, NP> *aggv) {
    __shared__ ScanShared<P, NP> sh;
    const uint64_t i0 = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanK;
    const uint32_t flags = mask_flags<kScanK>(d, i0);
    SVal<P, NP> x[kScanK];
    ld_vals<P, NP, kScanK>(d, i0, x);
    uint32_t ef, tf;
    SVal<P, NP> ev, tv;
    block_scan<P, NP, ADD, kScanK>(flags, x, sh, ef, ev, tf, tv);
    if (threadIdx.x == 0) {
        aggf[blockIdx.x] = tf;
        aggv[blockIdx.x] = tv;
    }
}

// 2: one workgroup; every aggregate replaced by the combination of (open, carry) and the
// aggregates before it (write_prefix), the combination of everything to outf / outv (if given)
template <typename P, int NP, bool ADD>
__global__ __launch_bounds__(kScanBS) void k_scan_aggs(uint32_t *aggf, SVal<P, NP> *aggv, const uint32_t ntiles,
                                                       const uint32_t open, const SVal<P, NP> carry,
                                                       const int write_prefix, uint32_t *outf, SVal<P, NP> *outv) {
    typedef SVal<P, NP> V;
    __shared__ ScanShared<P, NP> sh;
    uint32_t rf = open ? 1u : 0u;
    V rv = open ? carry : scan_ident_v<P, NP>();
    for (uint32_t base = 0; base < ntiles; base += (uint32_t)kScanAggSpan) {
        const uint32_t j0 = base + threadIdx.x * (uint32_t)kScanAggK;
        uint32_t flags = 0;
        V x[kScanAggK];
#pragma unroll
        for (int k = 0; k < kScanAggK; ++k) {
            const bool in = j0 + k < ntiles;
            x[k] = in ? aggv[j0 + k] : scan_ident_v<P, NP>();
            flags |= (in ? (aggf[j0 + k] & 1u) : 0u) << k;
        }
        uint32_t ef, tf;
        V ev, tv;
        block_scan<P, NP, ADD, kScanAggK>(flags, x, sh, ef, ev, tf, tv);
        uint32_t pf = rf;
        V pv = rv;
        scan_comb<P, NP, ADD>(pf, pv, ef, ev);
        if (write_prefix) {
#pragma unroll
            for (int k = 0; k < kScanAggK; ++k) {
                if (j0 + k < ntiles) {
                    aggf[j0 + k] = pf;
                    aggv[j0 + k] = pv;
                }
                scan_comb<P, NP, ADD>(pf, pv, (flags >> k) & 1u, x[k]);
            }
        }
        scan_comb<P, NP, ADD>(rf, rv, tf, tv);
    }
    if (threadIdx.x == 0 && outf) {
        *outf = rf;
        *outv = rv;
    }
}

// 3: the tile again, from its prefix.  ADD writes an element only once a segment is open
// (the prefix's flag or a set element at or before it); COPY writes every element.
template <typename P, int NP, bool ADD>
__global__ __launch_bounds__(kScanBS) void k_scan_write(const ScanDesc d, const uint32_t *aggf, const SVal<P, NP> *aggv) {
    typedef SVal<P, NP> V;
    constexpr int E = NP * (int)sizeof(P);
    __shared__ ScanShared<P, NP> sh;
    const uint64_t i0 = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanK;
    const uint32_t flags = mask_flags<kScanK>(d, i0);
    V x[kScanK];
    ld_vals<P, NP, kScanK>(d, i0, x);
    uint32_t ef, tf;
    V ev, tv;
    block_scan<P, NP, ADD, kScanK>(flags, x, sh, ef, ev, tf, tv);
    uint32_t cf = aggf[blockIdx.x];
    V cv = aggv[blockIdx.x];
    scan_comb<P, NP, ADD>(cf, cv, ef, ev);
    union { uint32_t w[kScanK * E / 4]; V v[kScanK]; } o;
    uint32_t written = 0;
    const bool excl = d.fn == kScanAddExcl;   // uniform
#pragma unroll
    for (int k = 0; k < kScanK; ++k) {
        const uint32_t fk = (flags >> k) & 1u;
        if (excl) {
            V z;
#pragma unroll
            for (int c = 0; c < NP; ++c) z.t[c] = fk ? (P)0 : cv.t[c];
            o.v[k] = z;
            written |= (cf | fk) << k;
            scan_comb<P, NP, ADD>(cf, cv, fk, x[k]);
        } else {
            scan_comb<P, NP, ADD>(cf, cv, fk, x[k]);
            o.v[k] = cv;
            written |= (ADD ? cf : 1u) << k;
        }
    }
    if (i0 >= d.n) return;
    char *q = d.dst + (int64_t)(i0 * (uint64_t)E);
    if (i0 + kScanK <= d.n && written == (1u << kScanK) - 1u) {
        st_run<kScanK * E>(q, d.dw, o.w);
        return;
    }
#pragma unroll
    for (int k = 0; k < kScanK; ++k) {
        if (i0 + k < d.n && ((written >> k) & 1u)) {
#pragma unroll
            for (int j = 0; j < E / 4; ++j) reinterpret_cast<uint32_t *>(q + k * E)[j] = o.w[k * (E / 4) + j];
        }
    }
}

// ---------------------------------------------------------------------------
// compaction.  The counts go through k_scan_aggs<uint64_t, 1, true> as (0, count) pairs with
// (1, 0) in front: what it leaves in aggv[tile] is the tile's first position in `packed`.
__device__ __forceinline__ void block_excl_u32(uint32_t c, uint32_t *sh, uint32_t &excl, uint32_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t s = c;
#pragma unroll
    for (int step = 1; step < 64; step <<= 1) {
        const uint32_t p = (uint32_t)__shfl_up((int)s, step, 64);
        if (lane >= step) s += p;
    }
    if (lane == 63) sh[wave] = s;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kScanBS / 64; ++w) {
        if (w == wave) before = all;
        all += sh[w];
    }
    excl = before + s - c;
    total = all;
}

__global__ __launch_bounds__(kScanBS) void k_mask_count(const ScanDesc d, uint32_t *aggf, SVal<uint64_t, 1> *aggv) {
    __shared__ uint32_t sh[kScanBS / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanK;
    const uint32_t flags = mask_flags<kScanK>(d, i0);
    uint32_t excl, total;
    block_excl_u32((uint32_t)__popc(flags), sh, excl, total);
    if (threadIdx.x == 0) {
        aggf[blockIdx.x] = 0;
        aggv[blockIdx.x].t[0] = total;
    }
}

// one element of E bytes in pieces of w bytes (w <= E, uniform)
template <int E>
__device__ __forceinline__ void copy_elem(char *q, const char *p, int w) {
    if constexpr (E >= 16) {
        if (w == 16) {
            vstore<16, false>(q, vload<16, false>(p));
            return;
        }
    }
    if constexpr (E >= 8) {
        if (w >= 8) {
#pragma unroll
            for (int j = 0; j < E / 8; ++j) vstore<8, false>(q + 8 * j, vload<8, false>(p + 8 * j));
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < E / 4; ++j) vstore<4, false>(q + 4 * j, vload<4, false>(p + 4 * j));
}

// PACK: d.dst[pos] = d.src[i] for the set i in order; UNPACK: d.dst[i] = d.src[pos]
template <int E, bool UNPACK>
__global__ __launch_bounds__(kScanBS) void k_mask_move(const ScanDesc d, const SVal<uint64_t, 1> *aggv) {
    __shared__ uint32_t sh[kScanBS / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanK;
    const uint32_t flags = mask_flags<kScanK>(d, i0);
    uint32_t excl, total;
    block_excl_u32((uint32_t)__popc(flags), sh, excl, total);
    uint64_t pos = aggv[blockIdx.x].t[0] + excl;
    if (!flags) return;
#pragma unroll
    for (int k = 0; k < kScanK; ++k) {
        if ((flags >> k) & 1u) {
            const int64_t bi = (int64_t)((i0 + k) * (uint64_t)E), bp = (int64_t)(pos * (uint64_t)E);
            if constexpr (UNPACK) copy_elem<E>(d.dst + bi, d.src + bp, d.dw);
            else copy_elem<E>(d.dst + bp, d.src + bi, d.dw);
            ++pos;
        }
    }
}

// ---------------------------------------------------------------------------
// enum: a lane computes the elements of 16 bytes of dst
template <typename P, int NP>
__global__ __launch_bounds__(kScanBS) void k_enum(char *dst, const uint64_t n, const uint64_t first,
                                                  const SVal<P, NP> start, const SVal<P, NP> stride, const int w) {
    constexpr int E = NP * (int)sizeof(P), NE = 16 / E;
    const uint64_t i0 = ((uint64_t)blockIdx.x * kScanBS + threadIdx.x) * (uint64_t)NE;
    if (i0 >= n) return;
    union { uint32_t w[4]; SVal<P, NP> v[NE]; } o;
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        const uint64_t g = first + i0 + k;
#pragma unroll
        for (int c = 0; c < NP; ++c) {
            P m;
            if constexpr (std::is_floating_point<P>::value) m = (P)(int64_t)g;
            else m = (P)g;
            const P off = m * stride.t[c];
            o.v[k].t[c] = start.t[c] + off;
        }
    }
    char *q = dst + (int64_t)(i0 * (uint64_t)E);
    if (i0 + NE <= n) {
        st_run<16>(q, w, o.w);
        return;
    }
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        if (i0 + k < n) {
#pragma unroll
            for (int j = 0; j < E / 4; ++j) reinterpret_cast<uint32_t *>(q + k * E)[j] = o.w[k * (E / 4) + j];
        }
    }
}

// ---------------------------------------------------------------------------
// host side
static int scan_width(const void *p) { return (int)lowbit((uint64_t)(uintptr_t)p | 16); }

static bool scan_type_ok(int op) { return op >= COMEX_ACC_INT && op <= COMEX_ACC_LNG; }

// which 4-byte words of a mask element hold a sign bit
static uint32_t mask_sign_words(int mop) {
    switch (mop) {
    case COMEX_ACC_FLT: return 1u;    // float
    case COMEX_ACC_DBL: return 2u;    // double: the high word
    case COMEX_ACC_CPL: return 3u;    // float complex
    case COMEX_ACC_DCP: return 10u;   // double complex: words 1 and 3
    }
    return 0u;
}

static bool spans_overlap(const void *a, uint64_t abytes, const void *b, uint64_t bbytes) {
    const uint64_t alo = (uint64_t)(uintptr_t)a, blo = (uint64_t)(uintptr_t)b;
    return alo < blo + bbytes && blo < alo + abytes;
}

struct ScanScratch {
    DotScratch *s;
    void *aggv;
    uint32_t *aggf;
};

static bool scan_scratch(uint32_t ntiles, ScanScratch &o) {
    o.s = dot_scratch((size_t)ntiles * 20);
    if (!o.s) return false;
    o.aggv = o.s->part;
    o.aggf = (uint32_t *)((char *)o.s->part + (size_t)ntiles * 16);
    return true;
}

static void scan_desc(ScanDesc &d, int mop, long long n, const void *src, const void *msk, void *dst, int fn) {
    memset(&d, 0, sizeof(d));
    d.src = (const char *)src;
    d.msk = (const char *)msk;
    d.dst = (char *)dst;
    d.n = (uint64_t)n;
    d.sw = scan_width(src);
    d.mw = scan_width(msk);
    d.dw = scan_width(dst);
    d.me = elem_size(mop);
    d.msign = mask_sign_words(mop);
    d.fn = fn;
}

// tail != 0: launches 1 and 2 with the total to the pinned result; else all three
template <typename P, int NP, bool ADD>
static hipError_t go_scan(bool tail, const ScanDesc &d, uint32_t ntiles, const ScanScratch &sc, int open, const void *carry,
                          hipStream_t st) {
    typedef SVal<P, NP> V;
    V c;
    memset(&c, 0, sizeof(c));
    if (open && carry) memcpy(&c, carry, sizeof(c));
    hipLaunchKernelGGL((k_scan_reduce<P, NP, ADD>), dim3(ntiles), dim3(kScanBS), 0, st, d, sc.aggf, (V *)sc.aggv);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    uint32_t *outf = tail ? (uint32_t *)((char *)sc.s->res_dev + kResFlag) : nullptr;
    V *outv = tail ? (V *)sc.s->res_dev : nullptr;
    hipLaunchKernelGGL((k_scan_aggs<P, NP, ADD>), dim3(1), dim3(kScanBS), 0, st, sc.aggf, (V *)sc.aggv, ntiles,
                       (uint32_t)(open != 0), c, tail ? 0 : 1, outf, outv);
    e = hipGetLastError();
    if (e != hipSuccess || tail) return e;
    hipLaunchKernelGGL((k_scan_write<P, NP, ADD>), dim3(ntiles), dim3(kScanBS), 0, st, d, (const uint32_t *)sc.aggf,
                       (const V *)sc.aggv);
    return hipGetLastError();
}

static hipError_t go_scan_op(int op, int fn, bool tail, const ScanDesc &d, uint32_t ntiles, const ScanScratch &sc, int open,
                             const void *carry, hipStream_t st) {
    if (fn == kScanCopy) {   // by element size
        switch (elem_size(op)) {
        case 4: return go_scan<uint32_t, 1, false>(tail, d, ntiles, sc, open, carry, st);
        case 8: return go_scan<uint64_t, 1, false>(tail, d, ntiles, sc, open, carry, st);
        case 16: return go_scan<uint64_t, 2, false>(tail, d, ntiles, sc, open, carry, st);
        }
        return hipErrorInvalidValue;
    }
    return for_type(op, [&](auto t) {
        typedef decltype(t) T;
        return go_scan<typename T::real, T::parts, true>(tail, d, ntiles, sc, open, carry, st);
    });
}

static bool scan_fn_ok(int fn) { return fn == kScanCopy || fn == kScanAdd || fn == kScanAddExcl; }

int scan_tile(int op, int mop) { return scan_type_ok(op) && scan_type_ok(mop) ? kScanTile : kPatchErrOp; }
int scan_agg_span() { return kScanAggSpan; }

int launch_scan_tail(int op, int fn, int mop, long long n, const void *src, const void *msk, int *has_flag, void *tail,
                     hipStream_t stream) {
    if (n < 0) return kPatchErrCount;
    if (!scan_type_ok(op) || !scan_type_ok(mop) || !scan_fn_ok(fn)) return kPatchErrOp;
    if (!src || !msk || !has_flag || !tail) return kPatchErrScalar;
    if (n > kScanMaxN) return kPatchErrRange;
    if (((uintptr_t)src | (uintptr_t)msk) & 3) return kPatchErrAlign;
    const int esz = elem_size(op);
    *has_flag = 0;
    memset(tail, 0, (size_t)esz);
    if (n == 0) return 0;
    const uint32_t ntiles = (uint32_t)(((uint64_t)n + kScanTile - 1) / kScanTile);
    ScanScratch sc;
    if (!scan_scratch(ntiles, sc)) return -100 - (int)hipGetLastError();
    ScanDesc d;
    scan_desc(d, mop, n, src, msk, nullptr, fn);
    int rc;
    const char *res = patch_result(sc.s, go_scan_op(op, fn, true, d, ntiles, sc, 0, nullptr, stream), stream, rc);
    if (!res) return rc;
    *has_flag = rd<uint32_t>(res + kResFlag) ? 1 : 0;
    memcpy(tail, res, (size_t)esz);
    return 0;
}

int launch_scan(int op, int fn, int mop, long long n, const void *src, const void *msk, void *dst, int open,
                const void *carry, hipStream_t stream) {
    if (n < 0) return kPatchErrCount;
    if (!scan_type_ok(op) || !scan_type_ok(mop) || !scan_fn_ok(fn)) return kPatchErrOp;
    if (!src || !msk || !dst || (open && !carry)) return kPatchErrScalar;
    if (n > kScanMaxN) return kPatchErrRange;
    if (((uintptr_t)src | (uintptr_t)msk | (uintptr_t)dst) & 3) return kPatchErrAlign;
    const uint64_t vb = (uint64_t)n * (uint64_t)elem_size(op), mb = (uint64_t)n * (uint64_t)elem_size(mop);
    if (n > 0 && (spans_overlap(dst, vb, src, vb) || spans_overlap(dst, vb, msk, mb))) return kPatchErrOverlap;
    if (n == 0) return 0;
    const uint32_t ntiles = (uint32_t)(((uint64_t)n + kScanTile - 1) / kScanTile);
    ScanScratch sc;
    if (!scan_scratch(ntiles, sc)) return -100 - (int)hipGetLastError();
    ScanDesc d;
    scan_desc(d, mop, n, src, msk, dst, fn);
    return rc_of(go_scan_op(op, fn, false, d, ntiles, sc, open, carry, stream));
}

// launches 1 and 2 of the compaction; total: only the count, to the pinned result
static hipError_t go_mask_offsets(const ScanDesc &d, uint32_t ntiles, const ScanScratch &sc, bool total, hipStream_t st) {
    typedef SVal<uint64_t, 1> V;
    hipLaunchKernelGGL(k_mask_count, dim3(ntiles), dim3(kScanBS), 0, st, d, sc.aggf, (V *)sc.aggv);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    V zero;
    zero.t[0] = 0;
    hipLaunchKernelGGL((k_scan_aggs<uint64_t, 1, true>), dim3(1), dim3(kScanBS), 0, st, sc.aggf, (V *)sc.aggv, ntiles, 1u,
                       zero, total ? 0 : 1, total ? (uint32_t *)((char *)sc.s->res_dev + kResFlag) : nullptr,
                       total ? (V *)sc.s->res_dev : nullptr);
    return hipGetLastError();
}

int launch_mask_count(int mop, long long n, const void *msk, long long *count, hipStream_t stream) {
    if (n < 0) return kPatchErrCount;
    if (!scan_type_ok(mop)) return kPatchErrOp;
    if (!msk || !count) return kPatchErrScalar;
    if (n > kScanMaxN) return kPatchErrRange;
    if ((uintptr_t)msk & 3) return kPatchErrAlign;
    *count = 0;
    if (n == 0) return 0;
    const uint32_t ntiles = (uint32_t)(((uint64_t)n + kScanTile - 1) / kScanTile);
    ScanScratch sc;
    if (!scan_scratch(ntiles, sc)) return -100 - (int)hipGetLastError();
    ScanDesc d;
    scan_desc(d, mop, n, nullptr, msk, nullptr, 0);
    int rc;
    const char *res = patch_result(sc.s, go_mask_offsets(d, ntiles, sc, true, stream), stream, rc);
    if (res) *count = (long long)rd<uint64_t>(res);
    return rc;
}

// unpack == false: `other` is packed (written), `arr` is src; true: `other` is packed (read), `arr` is dst
int launch_mask_move(bool unpack, int op, int mop, long long n, const void *arr, const void *msk, const void *other,
                     hipStream_t stream) {
    if (n < 0) return kPatchErrCount;
    if (!scan_type_ok(op) || !scan_type_ok(mop)) return kPatchErrOp;
    if (!arr || !msk || !other) return kPatchErrScalar;
    if (n > kScanMaxN) return kPatchErrRange;
    if (((uintptr_t)arr | (uintptr_t)msk | (uintptr_t)other) & 3) return kPatchErrAlign;
    const int esz = elem_size(op);
    const uint64_t vb = (uint64_t)n * (uint64_t)esz, mb = (uint64_t)n * (uint64_t)elem_size(mop);
    // the written side against both read sides; `packed` judged at its largest, n elements
    const void *wr = unpack ? arr : other, *rdv = unpack ? other : arr;
    if (n > 0 && (spans_overlap(wr, vb, rdv, vb) || spans_overlap(wr, vb, msk, mb))) return kPatchErrOverlap;
    if (n == 0) return 0;
    const uint32_t ntiles = (uint32_t)(((uint64_t)n + kScanTile - 1) / kScanTile);
    ScanScratch sc;
    if (!scan_scratch(ntiles, sc)) return -100 - (int)hipGetLastError();
    ScanDesc d;
    scan_desc(d, mop, n, rdv, msk, (void *)wr, 0);
    int w = (int)lowbit((uint64_t)(uintptr_t)arr | (uint64_t)(uintptr_t)other | 16);
    d.dw = w < esz ? w : esz;   // the piece an element moves in
    hipError_t e = go_mask_offsets(d, ntiles, sc, false, stream);
    if (e != hipSuccess) return rc_of(e);
    typedef SVal<uint64_t, 1> V;
    const V *av = (const V *)sc.aggv;
    switch (esz) {
    case 4:
        if (unpack) hipLaunchKernelGGL((k_mask_move<4, true>), dim3(ntiles), dim3(kScanBS), 0, stream, d, av);
        else hipLaunchKernelGGL((k_mask_move<4, false>), dim3(ntiles), dim3(kScanBS), 0, stream, d, av);
        break;
    case 8:
        if (unpack) hipLaunchKernelGGL((k_mask_move<8, true>), dim3(ntiles), dim3(kScanBS), 0, stream, d, av);
        else hipLaunchKernelGGL((k_mask_move<8, false>), dim3(ntiles), dim3(kScanBS), 0, stream, d, av);
        break;
    default:
        if (unpack) hipLaunchKernelGGL((k_mask_move<16, true>), dim3(ntiles), dim3(kScanBS), 0, stream, d, av);
        else hipLaunchKernelGGL((k_mask_move<16, false>), dim3(ntiles), dim3(kScanBS), 0, stream, d, av);
        break;
    }
    return rc_of(hipGetLastError());
}

template <typename P, int NP>
static hipError_t go_enum(long long n, long long first, const void *start, const void *stride, void *dst, hipStream_t st) {
    typedef SVal<P, NP> V;
    constexpr int NE = 16 / (NP * (int)sizeof(P));
    V a, s;
    memcpy(&a, start, sizeof(V));
    memcpy(&s, stride, sizeof(V));
    const uint64_t lanes = ((uint64_t)n + NE - 1) / NE;
    const unsigned nb = (unsigned)((lanes + kScanBS - 1) / kScanBS);
    hipLaunchKernelGGL((k_enum<P, NP>), dim3(nb), dim3(kScanBS), 0, st, (char *)dst, (uint64_t)n, (uint64_t)first, a, s,
                       scan_width(dst));
    return hipGetLastError();
}

int launch_enum(int op, long long n, long long first, const void *start, const void *stride, void *dst, hipStream_t stream) {
    if (n < 0) return kPatchErrCount;
    if (!scan_type_ok(op)) return kPatchErrOp;
    if (!start || !stride || !dst) return kPatchErrScalar;
    if (n > kScanMaxN) return kPatchErrRange;
    if ((uintptr_t)dst & 3) return kPatchErrAlign;
    if (n == 0) return 0;
    return rc_of(for_type(op, [&](auto t) {
        typedef decltype(t) T;
        return go_enum<typename T::real, T::parts>(n, first, start, stride, dst, stream);
    }));
}

}  // namespace gaamd
