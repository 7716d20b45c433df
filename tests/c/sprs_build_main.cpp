// The host part of NGA_Sprs_array_assemble (ga_amd/csrc/sprs_build.hpp: ownership, the owner's
// stable sort and the block CSR build) as a stand-alone program, built by tests/test_sprs_abi.py
// with -fsanitize=address,undefined.  Input (stdin): "idim jdim nproc n", then n lines
// "i j value" in source-rank then insertion order (the order the owners receive them in), values
// as unsigned 64-bit integers.  Output: for every rank its rows, blocks, starts, offsets, columns
// and values, which the test compares with its numpy restatement.
#include <stdio.h>
#include <stdlib.h>
#include "../../ga_amd/csrc/sprs_build.hpp"

int main() {
    long long idim, jdim, n;
    int nproc;
    if (scanf("%lld %lld %d %lld", &idim, &jdim, &nproc, &n) != 4) return 2;
    std::vector<gaamd_sprs::Elem> all((size_t)n);
    for (long long k = 0; k < n; k++) {
        long long i, j;
        unsigned long long v;
        if (scanf("%lld %lld %llu", &i, &j, &v) != 3) return 2;
        memset(&all[(size_t)k], 0, sizeof(gaamd_sprs::Elem));
        all[(size_t)k].i = (int32_t)i;
        all[(size_t)k].j = (int32_t)j;
        memcpy(all[(size_t)k].v, &v, 8);
    }
    for (int p = 0; p < nproc; p++) {
        long long lo, hi;
        gaamd_sprs::range(idim, nproc, p, &lo, &hi);
        std::vector<gaamd_sprs::Elem> mine;
        for (const gaamd_sprs::Elem &e : all)
            if (gaamd_sprs::owner(e.i, idim, nproc) == p) mine.push_back(e);
        gaamd_sprs::BlockCsr c;
        gaamd_sprs::build(mine, lo, hi - lo + 1, jdim, nproc, 8, c);
        printf("rank %d rows %lld %lld\nblocks", p, lo, hi);
        for (int b : c.blocks) printf(" %d", b);
        printf("\nstart");
        for (long long s : c.start) printf(" %lld", s);
        printf("\noffs");
        for (int32_t o : c.offs) printf(" %d", o);
        printf("\njdx");
        for (int32_t j : c.jdx) printf(" %d", j);
        printf("\nval");
        for (size_t k = 0; k < c.jdx.size(); k++) {
            unsigned long long v;
            memcpy(&v, c.val.data() + 8 * k, 8);
            printf(" %llu", v);
        }
        printf("\n");
    }
    return 0;
}
