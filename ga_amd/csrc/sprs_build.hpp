// sprs_build.hpp -- the host-only part of the sparse-array assembly (ga.cpp NGA_Sprs_array_assemble;
// ga.h states the contract): who owns a row or a column, and the owner's stable sort of the
// elements it received into a block CSR.  No GPU, no runtime: it is also compiled into a
// stand-alone program under the sanitizers (tests/c/sprs_build_main.cpp).
#ifndef GAAMD_SPRS_BUILD_HPP
#define GAAMD_SPRS_BUILD_HPP
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

namespace gaamd_sprs {

// one element as it travels to its owner: global row, global column, the value's bytes
struct Elem {
    int32_t i, j;
    unsigned char v[16];
};

// index i of a dimension of `dim` belongs to min((i * nproc) / dim, nproc - 1) (sparse.array.c:326, 524)
inline int owner(long long i, long long dim, int nproc) {
    const long long o = (i * (long long)nproc) / dim;
    return (int)std::min<long long>(o, nproc - 1);
}

// the indices that formula gives to iproc: [lo, hi], hi = lo - 1 when there are none.  The first
// index of p is the smallest i with i * nproc >= p * dim.
inline void range(long long dim, int nproc, int iproc, long long *lo, long long *hi) {
    auto first = [&](long long p) { return p >= nproc ? dim : (p * dim + nproc - 1) / nproc; };
    *lo = first(iproc);
    *hi = first((long long)iproc + 1) - 1;
}

struct BlockCsr {
    std::vector<int> blocks;            // the non-empty column blocks, ascending
    std::vector<long long> start;       // where each begins in jdx / val
    std::vector<int32_t> offs;          // [blocks][nrows + 1], relative to the block's start
    std::vector<int32_t> jdx;           // global columns
    std::vector<unsigned char> val;     // esz bytes per entry
};

// elems: what the owner of rows [ilo, ilo + nrows) received, ordered by source rank, then by
// insertion.  Stable sort by (column block, row, column): duplicates of one (i, j) keep that order.
inline void build(std::vector<Elem> &elems, long long ilo, long long nrows, long long jdim, int nproc, int esz,
                  BlockCsr &out) {
    std::stable_sort(elems.begin(), elems.end(), [&](const Elem &a, const Elem &b) {
        const int ba = owner(a.j, jdim, nproc), bb = owner(b.j, jdim, nproc);
        if (ba != bb) return ba < bb;
        if (a.i != b.i) return a.i < b.i;
        return a.j < b.j;
    });
    const size_t n = elems.size();
    out = BlockCsr();
    out.jdx.resize(n);
    out.val.resize(n * (size_t)esz);
    for (size_t k = 0; k < n;) {
        const int blk = owner(elems[k].j, jdim, nproc);
        size_t e = k;
        while (e < n && owner(elems[e].j, jdim, nproc) == blk) ++e;
        out.blocks.push_back(blk);
        out.start.push_back((long long)k);
        const size_t t0 = out.offs.size();
        out.offs.resize(t0 + (size_t)nrows + 1, 0);
        int32_t *offs = out.offs.data() + t0;
        for (size_t q = k; q < e; ++q) offs[elems[q].i - ilo + 1]++;
        for (long long r = 0; r < nrows; ++r) offs[r + 1] += offs[r];
        k = e;
    }
    for (size_t k = 0; k < n; ++k) {
        out.jdx[k] = elems[k].j;
        memcpy(out.val.data() + k * (size_t)esz, elems[k].v, (size_t)esz);
    }
}

}  // namespace gaamd_sprs

#endif
