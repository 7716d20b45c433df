// gaamd_select.hip -- the minimum or maximum element of a patch and where it lies
// (ga_amd.h gaamd_patch_select; the kernel under NGA_Select_elem).  Compiled as part of
// gaamd_all.hip after gaamd_patch.hip, whose descriptor, row decode, plan and per-thread
// scratch it shares.
//
// Reference (global/src/select.c:143-250): a scan from the first element that replaces
// its candidate only by a strictly better key, so among equal keys the first occurrence
// wins.  Key: the element itself; complex re*re + im*im in the element's own real type
// (two products, one sum, no FMA; 169-197).
//
// A candidate is (key, index), index = row * row_elements + position in the row, 64-bit,
// which is the element's linear index in the patch with count[0] fastest (merging joins
// only contiguous dimensions).  Candidates are combined by
//     better(x, y) = x.key < y.key || (x.key == y.key && x.idx < y.idx)     (min; max: >)
// everywhere -- a lane over its vectors, the lanes of a wave by a shuffle tree, the waves
// through LDS, the workgroups' partials in a second launch of one workgroup.  For NaN-free
// input `better` is a total order on candidates, so the combine is associative and
// commutative: the result does not depend on the grid or on timing and equals the
// reference's first-occurrence scan.  A patch holding a NaN returns an unspecified element.
// The work split is k_patch_dot's: item = (row, chunk of kDotBS vectors), kDotItems items
// per workgroup, every load issued before the first compare.  No atomics.
#pragma clang fp contract(off)

namespace gaamd {

template <typename K>
struct SelCand {
    K key;
    int64_t idx;   // < 0: no candidate
};

struct SelPart {   // a workgroup's candidate in device scratch
    int64_t idx;
    uint64_t key;
};

template <bool MAX, typename K>
__device__ __forceinline__ SelCand<K> sel_pick(const SelCand<K> x, const SelCand<K> y) {
    const bool y_key = MAX ? y.key > x.key : y.key < x.key;
    const bool take_y = x.idx < 0 || (y.idx >= 0 && (y_key || (y.key == x.key && y.idx < x.idx)));
    return take_y ? y : x;
}

template <typename T>
struct SelReal {
    typedef T key_t;
    static constexpr int kElem = (int)sizeof(T);
    template <bool MAX, int W>
    __device__ __forceinline__ static void scan(SelCand<T> &c, typename Vec<W>::T v, int64_t idx0) {
        constexpr int N = W / (int)sizeof(T);
        union { typename Vec<W>::T v; T t[N]; } a;
        a.v = v;
#pragma unroll
        for (int i = 0; i < N; ++i) c = sel_pick<MAX>(c, SelCand<T>{a.t[i], idx0 + i});
    }
};

template <typename R>
struct SelCplx {
    typedef R key_t;
    static constexpr int kElem = 2 * (int)sizeof(R);
    template <bool MAX, int W>
    __device__ __forceinline__ static void scan(SelCand<R> &c, typename Vec<W>::T v, int64_t idx0) {
        constexpr int N = W / (int)(2 * sizeof(R));
        union { typename Vec<W>::T v; R t[2 * N]; } a;
        a.v = v;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            R p1 = a.t[2 * i] * a.t[2 * i];
            R p2 = a.t[2 * i + 1] * a.t[2 * i + 1];
            R k = p1 + p2;
            c = sel_pick<MAX>(c, SelCand<R>{k, idx0 + i});
        }
    }
};

// the workgroup's candidate, valid in thread 0: shuffle tree per wave, then the waves by lane 0
template <bool MAX, typename K>
__device__ __forceinline__ SelCand<K> sel_block(SelCand<K> c) {
    __shared__ K sh_key[kDotBS / 64];
    __shared__ int64_t sh_idx[kDotBS / 64];
#pragma unroll
    for (int delta = 32; delta > 0; delta >>= 1) {
        SelCand<K> o;
        o.key = shfl_down_any(c.key, delta);
        o.idx = shfl_down_any(c.idx, delta);
        c = sel_pick<MAX>(c, o);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        sh_key[wave] = c.key;
        sh_idx[wave] = c.idx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kDotBS / 64; ++w) c = sel_pick<MAX>(c, SelCand<K>{sh_key[w], sh_idx[w]});
    }
    return c;
}

template <class OP, bool MAX, int W, int LV>
__global__ __launch_bounds__(kDotBS) void k_patch_select(const PatchDesc d, const uint32_t items,
                                                         const FastDiv chunk_div, const int64_t row_elems,
                                                         SelPart *part) {
    typedef typename Vec<W>::T V;
    typedef typename OP::key_t K;
    V va[kDotItems];
    int64_t idx0[kDotItems];
    const uint32_t i0 = blockIdx.x * (uint32_t)kDotItems;
    // every load first and without a branch (k_patch_dot): a lane without a vector in an
    // item reads vector 0 of a row of the patch instead and drops it below (idx0 < 0)
#pragma unroll
    for (int k = 0; k < kDotItems; ++k) {
        const bool in = i0 + k < items;
        const uint32_t it = in ? i0 + k : 0u;
        const uint32_t rl = chunk_div.div(it);
        const uint32_t chunk = it - rl * chunk_div.d;
        int64_t off[1];
        patch_row<1, LV>(d, rl, off);
        const uint64_t v = (uint64_t)chunk * kDotBS + threadIdx.x;
        const bool ok = in && v < d.nvec;
        const int64_t b = ok ? (int64_t)(v * W) : 0;
        va[k] = vload<W, true>(d.p[0] + off[0] + b);
        idx0[k] = ok ? (int64_t)rl * row_elems + (int64_t)(v * (uint64_t)(W / OP::kElem)) : (int64_t)-1;
    }
    SelCand<K> c{K(), -1};
#pragma unroll
    for (int k = 0; k < kDotItems; ++k)
        if (idx0[k] >= 0) OP::template scan<MAX, W>(c, va[k], idx0[k]);
    c = sel_block<MAX>(c);
    if (threadIdx.x == 0) {
        SelPart o;
        o.idx = c.idx;
        o.key = 0;
        memcpy(&o.key, &c.key, sizeof(K));
        part[blockIdx.x] = o;
    }
}

// one workgroup over the partials (k_patch_dot_final's passes), then thread 0 reads the
// winning element and stores it, its key and its index into mapped pinned host memory
template <class OP, bool MAX, int LV>
__global__ __launch_bounds__(kDotBS) void k_patch_select_final(const PatchDesc d, const SelPart *part,
                                                               const uint32_t n, const int64_t row_elems,
                                                               char *out) {
    typedef typename OP::key_t K;
    SelCand<K> c{K(), -1};
    for (uint32_t base = 0; base < n; base += kDotBS * kFinalPer) {
#pragma unroll
        for (int k = 0; k < kFinalPer; ++k) {
            const uint32_t i = base + threadIdx.x * kFinalPer + k;
            if (i < n) {
                const SelPart o = part[i];
                SelCand<K> y;
                memcpy(&y.key, &o.key, sizeof(K));
                y.idx = o.idx;
                c = sel_pick<MAX>(c, y);
            }
        }
    }
    c = sel_block<MAX>(c);
    if (threadIdx.x != 0) return;
    if (c.idx >= 0) {
        const int64_t row = c.idx / row_elems, pos = c.idx - row * row_elems;
        int64_t off[1];
        patch_row<1, LV>(d, (uint32_t)row, off);
        const uint32_t *e = reinterpret_cast<const uint32_t *>(d.p[0] + off[0] + pos * OP::kElem);
#pragma unroll
        for (int w = 0; w < OP::kElem / 4; ++w) store_sys(reinterpret_cast<uint32_t *>(out) + w, e[w]);
        store_sys(reinterpret_cast<K *>(out + kResKey), c.key);
    }
    store_sys(reinterpret_cast<int64_t *>(out + kResIndex), c.idx);
}

template <class OP, bool MAX, int W>
static hipError_t go_select(const PatchReduce &r, int64_t row_elems, hipStream_t st) {
    SelPart *part = (SelPart *)r.s->part;
    if (r.d.levels <= 1) {
        hipLaunchKernelGGL((k_patch_select<OP, MAX, W, 1>), dim3(r.nwg), dim3(kDotBS), 0, st, r.d, r.items, r.cd, row_elems,
                           part);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((k_patch_select_final<OP, MAX, 1>), dim3(1), dim3(kDotBS), 0, st, r.d, (const SelPart *)part,
                           r.nwg, row_elems, (char *)r.s->res_dev);
    } else {
        hipLaunchKernelGGL((k_patch_select<OP, MAX, W, 0>), dim3(r.nwg), dim3(kDotBS), 0, st, r.d, r.items, r.cd, row_elems,
                           part);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((k_patch_select_final<OP, MAX, 0>), dim3(1), dim3(kDotBS), 0, st, r.d, (const SelPart *)part,
                           r.nwg, row_elems, (char *)r.s->res_dev);
    }
    return hipGetLastError();
}

template <class OP, int ELEM>
static hipError_t go_select_w(bool want_max, int W, const PatchReduce &r, int64_t row_elems, hipStream_t st) {
    return with_width<ELEM>(W, [&](auto w) {
        constexpr int VW = decltype(w)::value;
        return want_max ? go_select<OP, true, VW>(r, row_elems, st) : go_select<OP, false, VW>(r, row_elems, st);
    });
}

int launch_patch_select(int op, int want_max, const void *a, const long long *a_stride, const long long *count,
                        int ndim, void *value, void *key, long long *index, hipStream_t stream) {
    PatchPlan p;
    const void *base[1] = {a};
    const long long *str[1] = {a_stride};
    const int rc = patch_plan(op, 1, base, str, count, ndim, p);
    if (rc < 0) return rc;
    if (!value || !index) return kPatchErrScalar;
    if (rc == 1) {   // an empty patch has no element
        *index = -1;
        return 1;
    }
    PatchReduce r;
    int err = patch_reduce(p, 1, base, sizeof(SelPart), r);
    if (err) return err;
    const int64_t row_elems = (int64_t)(p.row_bytes / (uint64_t)p.esz);
    const bool mx = want_max != 0;
    int ksz = 0;   // the key: the element itself, for complex a value of its real type
    const hipError_t e = for_type<int32_t, int64_t>(op, [&](auto t) {
        typedef typename decltype(t)::real T;
        typedef std::conditional_t<decltype(t)::parts == 1, SelReal<T>, SelCplx<T>> OP;
        ksz = (int)sizeof(T);
        return go_select_w<OP, decltype(t)::elem>(mx, p.W, r, row_elems, stream);
    });
    const char *res = patch_result(r.s, e, stream, err);
    if (!res) return err;
    memcpy(value, res, (size_t)p.esz);
    if (key) memcpy(key, res + kResKey, (size_t)ksz);
    memcpy(index, res + kResIndex, 8);
    return 0;
}

}  // namespace gaamd
