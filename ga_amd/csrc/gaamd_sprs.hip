// gaamd_sprs.hip -- the kernels under GA's sparse arrays (ga_amd.h gaamd_spmv, gaamd_sprs_diag,
// gaamd_sprs_scale_left, gaamd_sprs_scale_right; ga.h NGA_Sprs_array_*).  Compiled as part of
// gaamd_all.hip after gaamd_patch.hip, whose type dispatch (for_type) and codes it shares.
//
// The matrix is a block CSR: the rows of one rank, cut into column blocks.  Block b has a table
// of nrows + 1 row offsets (offs + b * (nrows + 1)), relative to the place start[b] where the
// block begins in jdx / val; jdx holds global column indices.  The entries of a row, over the
// blocks in ascending order, form one list e_0 .. e_{c-1}.
//
// Reference arithmetic (global/src/sparse.array.c), with the departures ga_amd.h states:
//   matvec       y_i = sum a_ij * x_j: one product, one add per entry; complex the true product
//                re = a.re*x.re - a.im*x.im, im = a.re*x.im + a.im*x.re, summed part by part
//   get diag     d_i = a_ii, the last (i, i) in storage order                       1646-1693
//   shift diag   a_ii += shift on every stored (i, i), complex part by part         1995-2023
//   left/right   a_ij = d * a_ij, complex re = d.re*a.re - d.im*a.im,
//                im = d.re*a.im + d.im*a.re                                        1742-1770, 1871-1900
// Integers in unsigned arithmetic (two's-complement wraparound).  FP contraction is off.
//
// SPMV, DIAG, SCALE_LEFT: one team of W = 2^lg lanes per row, 256 / W rows per workgroup, teams
// packed into wave64; a workgroup walks rows base, base + gridDim.x * 256 / W, ... with `base`
// uniform, so every lane reaches every cross-lane step.  Lane L of a team takes e_L, e_{L+W}, ...
// in that order from +0: in block b, whose entries are e_P .. e_{P+c_b-1}, that is the local
// entries t = (L - P) mod W, t + W, ..., so for W >= 2 consecutive lanes read consecutive jdx /
// val (rotated by P).  The W partials are combined by the butterfly v = v + v[lane ^ s],
// s = 1, 2, .. W / 2: addition commutes bit for bit, so after it every lane of the team holds the
// same bits; lane 0 stores.  Lanes past a row's end, and teams past the last row, hold +0.
// The cross-lane move is ds_bpermute_b32 (one per 32 bits of the value): it needs no LDS
// allocation and takes any s, where DPP row operations stop at 16 lanes.  No atomics, no LDS.
// Every index into offs, jdx, val, x and y is 64-bit.
// SCALE_RIGHT: one lane per entry.
// Resources (hipcc -O3, gfx950): k_spmv 22 to 24 VGPRs, 30 for complex double; the other
// kernels at most 24; occupancy 8 waves per SIMD; no kernel of this file uses scratch or LDS.
#pragma clang fp contract(off)

namespace gaamd {

int spmv_team(long long nnz_total, long long rows) {
    if (rows < 1 || nnz_total < 1) return 1;
    // the smallest power of two W with 2 * W * rows >= nnz_total, at most 64: a lane of the
    // average row takes about two entries
    const long long q = nnz_total / rows, r = nnz_total % rows;
    int w = 1;
    while (w < 64 && (q > 2ll * w || (q == 2ll * w && r > 0))) w *= 2;
    return w;
}

template <typename T, int NP>
struct alignas(sizeof(T) * NP) SprsEl {
    T t[NP];
};

// r = a * b: the product of the real types, the true complex product
template <typename T, int NP>
__device__ __forceinline__ SprsEl<T, NP> sprs_mul(const SprsEl<T, NP> a, const SprsEl<T, NP> b) {
    SprsEl<T, NP> r;
    if constexpr (NP == 1) {
        r.t[0] = a.t[0] * b.t[0];
    } else {
        const T p1 = a.t[0] * b.t[0];
        const T p2 = a.t[1] * b.t[1];
        const T p3 = a.t[0] * b.t[1];
        const T p4 = a.t[1] * b.t[0];
        r.t[0] = p1 - p2;
        r.t[1] = p3 + p4;
    }
    return r;
}

// the value of lane (lane ^ s) of the wave
template <typename T>
__device__ __forceinline__ T lane_xor(T v, uint32_t s) {
    const int addr = (int)(((threadIdx.x & 63u) ^ s) << 2);
    int w[sizeof(T) / 4];
    memcpy(w, &v, sizeof(T));
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) / 4); ++k) w[k] = __builtin_amdgcn_ds_bpermute(addr, w[k]);
    memcpy(&v, w, sizeof(T));
    return v;
}

constexpr int kSprsBS = 256;
constexpr uint32_t kSprsMaxGrid = 1u << 22;

struct SpmvDesc {
    const int32_t *offs;    // [nblk][nrows + 1]
    const int64_t *start;   // [nblk]
    const int32_t *jdx;
    const char *val;
    const char *x;
    char *y;
    int64_t x_first;        // the global column of x[0]
    uint64_t nrows;
    int32_t nblk, lg;
};

template <typename T, int NP>
__global__ __launch_bounds__(kSprsBS) void k_spmv(const SpmvDesc d) {
    typedef SprsEl<T, NP> E;
    const uint32_t W = 1u << d.lg, lane = threadIdx.x & (W - 1);
    const uint64_t per = (uint64_t)(kSprsBS >> d.lg), step = (uint64_t)gridDim.x * per;
    const E *val = reinterpret_cast<const E *>(d.val), *x = reinterpret_cast<const E *>(d.x);
    for (uint64_t base = (uint64_t)blockIdx.x * per; base < d.nrows; base += step) {   // uniform
        const uint64_t row = base + (threadIdx.x >> d.lg);
        E acc = {};
        if (row < d.nrows) {
            uint32_t P = 0;   // entries of the row in the blocks before b
            for (int32_t b = 0; b < d.nblk; ++b) {
                const int32_t *o = d.offs + (int64_t)b * (int64_t)(d.nrows + 1) + (int64_t)row;
                const uint32_t o0 = (uint32_t)o[0], c = (uint32_t)o[1] - o0;
                const int64_t k0 = d.start[b] + (int64_t)o0;
                for (uint32_t t = (lane - P) & (W - 1); t < c; t += W) {
                    const int64_t k = k0 + (int64_t)t;
                    const E p = sprs_mul<T, NP>(val[k], x[(int64_t)d.jdx[k] - d.x_first]);
#pragma unroll
                    for (int i = 0; i < NP; ++i) acc.t[i] = acc.t[i] + p.t[i];
                }
                P += c;
            }
        }
        for (uint32_t s = 1; s < W; s <<= 1) {
#pragma unroll
            for (int i = 0; i < NP; ++i) acc.t[i] = acc.t[i] + lane_xor(acc.t[i], s);
        }
        if (row < d.nrows && lane == 0) reinterpret_cast<E *>(d.y)[row] = acc;
    }
}

static int sprs_lg(int team) {
    for (int lg = 0; lg <= 6; ++lg)
        if (team == (1 << lg)) return lg;
    return -1;
}

static unsigned sprs_grid(uint64_t nrows, int lg) {
    const uint64_t per = (uint64_t)(kSprsBS >> lg), nb = (nrows + per - 1) / per;
    return (unsigned)(nb < kSprsMaxGrid ? nb : kSprsMaxGrid);
}

constexpr long long kSprsMaxRows = 1ll << 40;

int launch_spmv(int op, long long nrows, int nblk, const int *offs, const long long *start, const int *jdx,
                const void *val, const void *x, long long x_first, void *y, int team, hipStream_t stream) {
    if (nrows < 0 || nblk < 0) return kPatchErrCount;
    const int esz = (op == kOpCopy) ? 0 : elem_size(op), lg = sprs_lg(team);
    if (!esz || lg < 0) return kPatchErrOp;
    if (nrows == 0) return 0;
    if (!y || (nblk > 0 && (!offs || !start || !jdx || !val || !x))) return kPatchErrScalar;
    if (nrows > kSprsMaxRows) return kPatchErrRange;
    if ((((uintptr_t)y | (uintptr_t)val | (uintptr_t)x) & (uintptr_t)(esz - 1)) || ((uintptr_t)start & 7) ||
        (((uintptr_t)offs | (uintptr_t)jdx) & 3))
        return kPatchErrAlign;
    SpmvDesc d;
    memset(&d, 0, sizeof(d));
    d.offs = offs;
    d.start = reinterpret_cast<const int64_t *>(start);
    d.jdx = jdx;
    d.val = (const char *)val;
    d.x = (const char *)x;
    d.y = (char *)y;
    d.x_first = x_first;
    d.nrows = (uint64_t)nrows;
    d.nblk = nblk;
    d.lg = lg;
    return rc_of(for_type(op, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((k_spmv<typename T::real, T::parts>), dim3(sprs_grid(d.nrows, lg)), dim3(kSprsBS), 0, stream, d);
        return hipGetLastError();
    }));
}

// ---------------------------------------------------------------------------
// one column block: offs its nrows + 1 offsets, jdx / val from the block's start
struct SprsBlockDesc {
    const int32_t *offs;
    const int32_t *jdx;
    char *val;
    char *v;              // diag GET: the dense run written; scale_left: the multipliers
    int64_t diag_first;   // the global index of row 0
    uint64_t nrows;
    int32_t fn, lg;
    Scale16 s;            // SHIFT: the constant
};

template <typename T, int NP>
__global__ __launch_bounds__(kSprsBS) void k_sprs_diag(const SprsBlockDesc d) {
    typedef SprsEl<T, NP> E;
    const uint32_t W = 1u << d.lg, lane = threadIdx.x & (W - 1);
    const uint64_t per = (uint64_t)(kSprsBS >> d.lg), step = (uint64_t)gridDim.x * per;
    E *val = reinterpret_cast<E *>(d.val);
    union { Scale16 s; E e; } sh;
    sh.s = d.s;
    for (uint64_t base = (uint64_t)blockIdx.x * per; base < d.nrows; base += step) {
        const uint64_t row = base + (threadIdx.x >> d.lg);
        int32_t best = -1;   // GET: the last local entry on the diagonal
        int64_t k0 = 0;
        if (row < d.nrows) {
            const uint32_t o0 = (uint32_t)d.offs[row], c = (uint32_t)d.offs[row + 1] - o0;
            const int64_t want = d.diag_first + (int64_t)row;
            k0 = (int64_t)o0;
            for (uint32_t t = lane; t < c; t += W) {
                if ((int64_t)d.jdx[k0 + t] != want) continue;
                if (d.fn == kDiagGet) {
                    best = (int32_t)t;
                } else {
                    E a = val[k0 + t];
#pragma unroll
                    for (int i = 0; i < NP; ++i) a.t[i] = a.t[i] + sh.e.t[i];
                    val[k0 + t] = a;
                }
            }
        }
        if (d.fn != kDiagGet) continue;   // uniform
        for (uint32_t s = 1; s < W; s <<= 1) {
            const int32_t o = lane_xor(best, s);
            best = o > best ? o : best;
        }
        if (row < d.nrows && lane == 0 && best >= 0) reinterpret_cast<E *>(d.v)[row] = val[k0 + best];
    }
}

template <typename T, int NP>
__global__ __launch_bounds__(kSprsBS) void k_sprs_scale_left(const SprsBlockDesc d) {
    typedef SprsEl<T, NP> E;
    const uint32_t W = 1u << d.lg, lane = threadIdx.x & (W - 1);
    const uint64_t per = (uint64_t)(kSprsBS >> d.lg), step = (uint64_t)gridDim.x * per;
    E *val = reinterpret_cast<E *>(d.val);
    for (uint64_t row = (uint64_t)blockIdx.x * per + (threadIdx.x >> d.lg); row < d.nrows; row += step) {
        const uint32_t o0 = (uint32_t)d.offs[row], c = (uint32_t)d.offs[row + 1] - o0;
        const E m = reinterpret_cast<const E *>(d.v)[row];
        for (uint32_t t = lane; t < c; t += W) val[(int64_t)o0 + t] = sprs_mul<T, NP>(m, val[(int64_t)o0 + t]);
    }
}

struct SprsRightDesc {
    const int32_t *jdx;
    char *val;
    const char *v;
    int64_t first;   // the global column of v[0]
    uint64_t n;
};

template <typename T, int NP>
__global__ __launch_bounds__(kSprsBS) void k_sprs_scale_right(const SprsRightDesc d) {
    typedef SprsEl<T, NP> E;
    const uint64_t k = (uint64_t)blockIdx.x * kSprsBS + threadIdx.x;
    if (k >= d.n) return;
    E *val = reinterpret_cast<E *>(d.val);
    val[k] = sprs_mul<T, NP>(reinterpret_cast<const E *>(d.v)[(int64_t)d.jdx[k] - d.first], val[k]);
}

int launch_sprs_diag(int op, int fn, long long nrows, const int *offs, const int *jdx, void *val, long long diag_first,
                     void *out, const void *shift, int team, hipStream_t stream) {
    if (nrows < 0) return kPatchErrCount;
    const int esz = (op == kOpCopy) ? 0 : elem_size(op), lg = sprs_lg(team);
    if (!esz || lg < 0 || (fn != kDiagGet && fn != kDiagShift)) return kPatchErrOp;
    if (nrows == 0) return 0;
    if (!offs || !jdx || !val || (fn == kDiagGet ? !out : !shift)) return kPatchErrScalar;
    if (nrows > kSprsMaxRows) return kPatchErrRange;
    if ((((uintptr_t)val | (uintptr_t)out) & (uintptr_t)(esz - 1)) || (((uintptr_t)offs | (uintptr_t)jdx) & 3))
        return kPatchErrAlign;
    SprsBlockDesc d;
    memset(&d, 0, sizeof(d));
    d.offs = offs;
    d.jdx = jdx;
    d.val = (char *)val;
    d.v = (char *)out;
    d.diag_first = diag_first;
    d.nrows = (uint64_t)nrows;
    d.fn = fn;
    d.lg = lg;
    if (fn == kDiagShift) memcpy(&d.s, shift, (size_t)esz);
    return rc_of(for_type(op, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((k_sprs_diag<typename T::real, T::parts>), dim3(sprs_grid(d.nrows, lg)), dim3(kSprsBS), 0, stream,
                           d);
        return hipGetLastError();
    }));
}

int launch_sprs_scale_left(int op, long long nrows, const int *offs, void *val, const void *dv, int team,
                           hipStream_t stream) {
    if (nrows < 0) return kPatchErrCount;
    const int esz = (op == kOpCopy) ? 0 : elem_size(op), lg = sprs_lg(team);
    if (!esz || lg < 0) return kPatchErrOp;
    if (nrows == 0) return 0;
    if (!offs || !val || !dv) return kPatchErrScalar;
    if (nrows > kSprsMaxRows) return kPatchErrRange;
    if ((((uintptr_t)val | (uintptr_t)dv) & (uintptr_t)(esz - 1)) || ((uintptr_t)offs & 3)) return kPatchErrAlign;
    SprsBlockDesc d;
    memset(&d, 0, sizeof(d));
    d.offs = offs;
    d.val = (char *)val;
    d.v = (char *)const_cast<void *>(dv);
    d.nrows = (uint64_t)nrows;
    d.lg = lg;
    return rc_of(for_type(op, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((k_sprs_scale_left<typename T::real, T::parts>), dim3(sprs_grid(d.nrows, lg)), dim3(kSprsBS), 0,
                           stream, d);
        return hipGetLastError();
    }));
}

int launch_sprs_scale_right(int op, long long n, const int *jdx, void *val, const void *dv, long long d_first,
                            hipStream_t stream) {
    if (n < 0) return kPatchErrCount;
    const int esz = (op == kOpCopy) ? 0 : elem_size(op);
    if (!esz) return kPatchErrOp;
    if (n == 0) return 0;
    if (!jdx || !val || !dv) return kPatchErrScalar;
    if (n >= (1ll << 39)) return kPatchErrRange;   // 2^31 workgroups of 256
    if ((((uintptr_t)val | (uintptr_t)dv) & (uintptr_t)(esz - 1)) || ((uintptr_t)jdx & 3)) return kPatchErrAlign;
    SprsRightDesc d;
    d.jdx = jdx;
    d.val = (char *)val;
    d.v = (const char *)dv;
    d.first = d_first;
    d.n = (uint64_t)n;
    const unsigned nb = (unsigned)((d.n + kSprsBS - 1) / kSprsBS);
    return rc_of(for_type(op, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((k_sprs_scale_right<typename T::real, T::parts>), dim3(nb), dim3(kSprsBS), 0, stream, d);
        return hipGetLastError();
    }));
}

}  // namespace gaamd
