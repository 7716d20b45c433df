// ga.cpp -- the Global Arrays caller of the accumulate path (SURVEY.md §8(a)
// row a15) over the MI355X ARMCI/ComEx runtime.
//
// Reference (paths in the GA tree):
//   NGA_Create / NGA_Create_irreg / NGA_Acc ...  global/src/capi.c:164-265, 2079-2089
//     (C order, 0-based  ->  Fortran order, 1-based: COPYC2F/COPYINDEX_C2F capi.c:54-61)
//   process grid            ddb, ddb_h2, ddb_ex, dd_ev, dd_su  global/src/decomp.c:125-758
//   block map               pnga_allocate  global/src/base.c:2550-2630
//   owner iteration         gai_iterator_*  global/src/iterator.c:188-771 (REGULAR)
//   ngai_acc_common         global/src/onesided.c:1334-1453: per owner
//       pbuf = buf + size*gam_ComputePatchIndex (onesided.c:330-337)
//       count = gam_ComputeCount, count[0] *= size (base.h:341-344)
//       stride_loc/stride_rem = gam_setstride (base.h:322-331)
//       remote owners first, then SMP-local; ARMCI_NbAccS for all but the last
//   statistics              GAstat.numacc, GAbytes.acctot/accloc (onesided.c:1372-1419)
// Each rank's block is column-major with the block's extents as leading
// dimensions (no ghosts), in one comex_malloc segment per array (HBM).
//
// This file is its own library, libga_amd_ga.so, linked against libga_amd.so
// and calling it only through the public C ABI (comex.h, armci.h, ga_amd.h) --
// the same position global/src has over libarmci.  libga_amd.so itself exports
// only comex_*/ARMCI_*/armci_*/gaamd_* names (as libarmci does, capi.c:14-27),
// so a real GA, which defines NGA_*/GA_* itself (global/src/capi.c:2079-2089),
// links against it without a second definition of its own entry points.
// built with -fvisibility=hidden: only the names the headers declare are exported
#pragma GCC visibility push(default)
#include "../../include/ga.h"
#include "../../include/armci.h"
#include "../../include/message.h"
#include "../../include/comex.h"
#include "../../include/ga_amd.h"
#pragma GCC visibility pop
#include "sprs_build.hpp"
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <limits>
#include <thread>
#include <string>
#include <vector>

namespace gaamd_ga {

// GA_Error / pnga_error: message, then abort through the runtime (comex_error ->
// the reference's MPI_Abort, comex_impl.h:52-76)
[[noreturn]] static void fatal(const char *fmt, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    char msg[800];
    snprintf(msg, sizeof(msg), "ga_amd GA: %s", buf);
    comex_error(msg, 1);
    abort();   // comex_error does not return
}

static int my_rank() {
    int me = 0;
    comex_group_rank(COMEX_GROUP_WORLD, &me);
    return me;
}

static int world_size() {
    int n = 1;
    comex_group_size(COMEX_GROUP_WORLD, &n);
    return n;
}

struct GArray {
    bool live = false;
    int type = 0, ndim = 0, elemsize = 0, optype = 0;
    std::string name;
    long dims[GA_MAX_DIM] = {0};        // Fortran order
    int nblock[GA_MAX_DIM] = {0};       // blocks (processes) per dimension
    std::vector<long> map[GA_MAX_DIM];  // 1-based first index of every block
    std::vector<void *> ptr;            // each rank's block (owner's address space)
    int nproc_grid = 0;
};

static std::vector<GArray> g_arrays;
static struct {
    long numacc = 0, numput = 0, numget = 0, numsca = 0, numgat = 0;
    double acctot = 0, accloc = 0, scatot = 0, scaloc = 0, gattot = 0, gatloc = 0;
    // calls that compute on the arrays where they lie, and the bytes this rank's kernels moved
    long numfill = 0, numscale = 0, numadd = 0, numcopy = 0, numdot = 0, numgemm = 0;
    long numtranspose = 0, numsymm = 0;
    long numelem[8] = {0};   // by GAAMD_ELEM_* code
    long numselect = 0;
    long numdiag = 0, numscalerows = 0, numscalecols = 0, numnorm1 = 0, numnorminf = 0;
    long numenum = 0, numscancopy = 0, numscanadd = 0, numpack = 0, numunpack = 0;
    long numsprs[7] = {0};   // by SprsCall
    double mathloc = 0;
} g_stat;

static GArray &arr(int g_a) {
    if (g_a < 1 || g_a > (int)g_arrays.size() || !g_arrays[g_a - 1].live) fatal("invalid global array handle %d", g_a);
    return g_arrays[g_a - 1];
}

static int type_size(int type, int *optype) {
    switch (type) {   // onesided.c:1362-1368
    case C_DBL: *optype = COMEX_ACC_DBL; return 8;
    case C_FLOAT: *optype = COMEX_ACC_FLT; return 4;
    case C_DCPL: *optype = COMEX_ACC_DCP; return 16;
    case C_SCPL: *optype = COMEX_ACC_CPL; return 8;
    case C_INT: *optype = COMEX_ACC_INT; return 4;
    case C_LONG: *optype = COMEX_ACC_LNG; return 8;
    }
    fatal("type %d not supported", type);
}

// ---- process grid: decomp.c restated ---------------------------------------
// dd_ev (decomp.c:711-722): load-balance ratio of a grid
static double dd_ev(int ndims, const long *ardims, const long *pedims) {
    double t = 1.0;
    for (int k = 0; k < ndims; k++) {
        const double q = (double)((ardims[k] / pedims[k]) * pedims[k]);
        t = t * (q / (double)ardims[k]);
    }
    return t;
}

// dd_su (decomp.c:730-738)
static void dd_su(int ndims, const long *ardims, const long *pedims, long *blk) {
    for (int i = 0; i < ndims; i++) {
        blk[i] = ardims[i] / pedims[i];
        if (blk[i] < 1) blk[i] = 1;
    }
}

// ddb_ex (decomp.c:213-333): exhaustive search over factorisations of npes,
// best load balance first, then least communication volume
static void ddb_ex(int ndims, const long *ardims, long npes, double threshold, long *blk, long *pedims) {
    if (ndims == 1) {
        pedims[0] = npes;
        dd_su(1, ardims, pedims, blk);
        return;
    }
    std::vector<long> tard(ndims), tdims(ndims, 0), stack(ndims, 0);
    for (int i = 0; i < ndims; i++) if (blk[i] < 1) blk[i] = 1;
    for (int i = 0; i < ndims; i++) tard[i] = ardims[i] / blk[i];
    for (int i = 0; i < ndims; i++) if (tard[i] < 1) { tard[i] = 1; blk[i] = ardims[i]; }
    double blb = -1.0;
    long bev = 1;
    for (int i = 0; i < ndims; i++) bev *= tard[i];
    pedims[0] = npes;
    for (int i = 1; i < ndims; i++) pedims[i] = 1;
    tdims[0] = 0;
    stack[0] = npes;
    int pc = 0;
    bool done = false;
    do {
        if (pc == ndims - 1) {
            tdims[pc] = stack[pc];
            const double clb = dd_ev(ndims, tard.data(), tdims.data());
            long cev = 0;
            for (int k = 0; k < ndims; k++) {
                long r = 1;
                for (int j = 0; j < ndims; j++) if (j != k) r = r * (tard[j] / tdims[j]);
                cev = cev + r;
            }
            if (clb > blb || (clb == blb && cev < bev)) {
                for (int j = 0; j < ndims; j++) pedims[j] = tdims[j];
                blb = clb;
                bev = cev;
            }
            if (blb > threshold) break;
            tdims[pc] = 0;
            pc -= 1;
        } else {
            if (tdims[pc] == stack[pc]) {
                done = (pc == 0);
                tdims[pc] = 0;
                pc -= 1;
            } else {
                for (tdims[pc] += 1; stack[pc] % tdims[pc] != 0; tdims[pc] += 1) {}
                pc += 1;
                stack[pc] = npes;
                for (int i = 0; i < pc; i++) stack[pc] /= tdims[i];
                tdims[pc] = 0;
            }
        }
    } while (!done);
    dd_su(ndims, ardims, pedims, blk);
}

// ddb_h2 (decomp.c:611-703): deal the prime factors of npes to the axes
static void ddb_h2(int ndims, const long *ardims, long npes, double threshold, long bias, long *blk, long *pedims) {
    std::vector<long> tard(ndims);
    for (int i = 0; i < ndims; i++) if (blk[i] < 1) blk[i] = 1;
    for (int i = 0; i < ndims; i++) tard[i] = (ardims[i] + blk[i] - 1) / blk[i];
    for (int i = 0; i < ndims; i++) if (tard[i] < 1) { tard[i] = 1; blk[i] = ardims[i]; }
    std::vector<long> pdivs;
    for (long i = 1; i <= npes; i++) if (npes % i == 0) pdivs.push_back(i);
    long npdivs = (long)pdivs.size();
    if (npdivs > 1) {   // prime divisors with repetition
        long k = 1;
        do {
            long h = k + 1;
            for (long j = h; j < npdivs; j++)
                if (pdivs[j] % pdivs[k] == 0) pdivs[h++] = pdivs[j] / pdivs[k];
            npdivs = h;
            k = k + 1;
        } while (k < npdivs);
    }
    long istep = 1, istart = 0;
    if (bias > 0) { istep = -1; istart = ndims - 1; }
    for (int j = 0; j < ndims; j++) pedims[j] = 1;
    for (long k = npdivs - 1; k >= 1; k--) {
        const long p0 = pdivs[k];
        long h = istart;
        double q = (tard[istart] < p0 * pedims[istart]) ? 1.1
                   : (double)(tard[istart] % (p0 * pedims[istart])) / (double)tard[istart];
        for (int j = 1; j < ndims; j++) {
            const long ilook = (istart + istep * j) % ndims;
            const double w = (tard[ilook] < p0 * pedims[ilook]) ? 1.1
                             : (double)(tard[ilook] % (p0 * pedims[ilook])) / (double)tard[ilook];
            if (w < q) { q = w; h = ilook; }
        }
        pedims[h] *= p0;
        if (bias == 0) istart = (istart + 1) % ndims;
    }
    const double ub = dd_ev(ndims, tard.data(), pedims);
    if (ub < threshold) ddb_ex(ndims, tard.data(), npes, threshold, blk, pedims);
    dd_su(ndims, ardims, pedims, blk);
    for (int i = 0; i < ndims; i++) {
        if (pedims[i] <= 0) fatal("process dimension is zero: ddb_h2");
        blk[i] = (tard[i] + pedims[i] - 1) / pedims[i];
    }
}

// ddb (decomp.c:125-199): user-chunked axes first, ddb_h2 on the rest
static void ddb(int ndims, const long *ardims, long npes, long *blk, long *pedims) {
    const double threshold = 0.1;
    long tp = npes, count = 0;
    for (int i = ndims - 1; i >= 0; i--) {
        if (blk[i] <= 0) {
            pedims[i] = -1;
            count += 1;
        } else {
            long sp = (ardims[i] + blk[i] - 1) / blk[i];
            if (sp > tp) {
                sp = tp;
                tp = 1;
                pedims[i] = sp;
            } else {
                long j;
                for (j = sp; j < tp && (tp % j != 0); j++) {}
                pedims[i] = j;
                tp = tp / j;
            }
        }
    }
    if (count > 0) {
        std::vector<long> tardim, tblk(count, 1), tpedim(count, 0);
        for (int j = 0; j < ndims; j++) if (pedims[j] < 0) tardim.push_back(ardims[j]);
        ddb_h2((int)count, tardim.data(), tp, threshold, 0, tblk.data(), tpedim.data());
        for (int i = 0, j = 0; j < ndims; j++)
            if (pedims[j] < 0) { blk[j] = (tardim[i] + tpedim[i] - 1) / tpedim[i]; i++; }
        for (int i = 0, j = 0; j < ndims; j++) if (pedims[j] < 0) pedims[j] = tpedim[i++];
    }
}

// ---- allocation --------------------------------------------------------------
static long block_elems(const GArray &a, int proc, long *lo, long *hi) {
    // ga_ownsM_no_handle (base.h:153-180): proc -> block coordinates, dim 0 fastest
    long n = 1;
    int idx = proc;
    for (int d = 0; d < a.ndim; d++) {
        const int loc = idx % a.nblock[d];
        idx /= a.nblock[d];
        lo[d] = a.map[d][loc];
        hi[d] = (loc + 1 < a.nblock[d]) ? a.map[d][loc + 1] - 1 : a.dims[d];
        n *= std::max(0L, hi[d] - lo[d] + 1);
    }
    if (proc >= a.nproc_grid) {
        for (int d = 0; d < a.ndim; d++) { lo[d] = 0; hi[d] = -1; }
        return 0;
    }
    return n;
}

// a rank's own block: HBM is zeroed on the device; a host segment (COMEX_AMD_SEGMENT=host)
// the way pnga_zero does it, memset through the host pointer (global.nalg.c:94-129)
static void zero_block(void *p, size_t bytes) {
    if (!bytes) return;
    if (gaamd_segment_kind(p) == 2) memset(p, 0, bytes);
    else if (gaamd_memset(p, 0, bytes) != 0) fatal("zeroing a %zu-byte block failed", bytes);
}

static int allocate(GArray &a) {
    const int me = my_rank(), np = world_size();
    long lo[GA_MAX_DIM], hi[GA_MAX_DIM];
    a.nproc_grid = 1;
    for (int d = 0; d < a.ndim; d++) a.nproc_grid *= a.nblock[d];
    if (a.nproc_grid > np) fatal("distribution needs %d processes, have %d", a.nproc_grid, np);
    const long n = block_elems(a, me, lo, hi);
    a.ptr.assign(np, nullptr);
    if (comex_malloc(a.ptr.data(), (size_t)n * a.elemsize, COMEX_GROUP_WORLD) != COMEX_SUCCESS) return 0;
    zero_block(a.ptr[me], (size_t)n * a.elemsize);
    comex_barrier(COMEX_GROUP_WORLD);
    a.live = true;
    g_arrays.push_back(a);
    return (int)g_arrays.size();
}

// ---- owner iteration + the per-owner ARMCI call (ngai_*_common) ---------------
enum GaOp { GA_ACC, GA_PUT, GA_GET };

// skip != nullptr: the strided (every skip[d]-th element) variants,
// pnga_strided_acc/put/get (onesided.c:4225-4470).  nb != nullptr: the
// non-blocking variants (pnga_nbacc/nbput/nbget, onesided.c:685, 1300, 1481):
// every owner's transfer is non-blocking and its handle is returned.
static void patch_op(GaOp kind, int g_a, const long *lo, const long *hi, void *buf, const long *ld, void *alpha,
                     const long *skip = nullptr, std::vector<armci_hdl_t> *nb = nullptr) {
    GArray &a = arr(g_a);
    const int me = my_rank();
    const int nd = a.ndim, size = a.elemsize;
    for (int d = 0; d < nd; d++)
        if (lo[d] < 1 || hi[d] > a.dims[d] || lo[d] > hi[d]) fatal("patch out of range in dim %d", d);
    // blocks of every dimension that intersect [lo, hi] (pnga_locate_region)
    int b0[GA_MAX_DIM], b1[GA_MAX_DIM];
    for (int d = 0; d < nd; d++) {
        const std::vector<long> &m = a.map[d];
        b0[d] = (int)(std::upper_bound(m.begin(), m.end(), lo[d]) - m.begin()) - 1;
        b1[d] = (int)(std::upper_bound(m.begin(), m.end(), hi[d]) - m.begin()) - 1;
    }
    long elems = 1;
    for (int d = 0; d < nd; d++) elems *= hi[d] - lo[d] + 1;
    if (kind == GA_ACC) { g_stat.numacc++; g_stat.acctot += (double)size * elems; }
    else if (kind == GA_PUT) g_stat.numput++;
    else g_stat.numget++;

    struct Owner { int proc; long plo[GA_MAX_DIM], phi[GA_MAX_DIM], ldrem[GA_MAX_DIM], blo[GA_MAX_DIM]; };
    std::vector<Owner> owners;
    int bi[GA_MAX_DIM];
    for (int d = 0; d < nd; d++) bi[d] = b0[d];
    for (;;) {
        Owner o;
        int proc = 0, mul = 1;
        for (int d = 0; d < nd; d++) { proc += bi[d] * mul; mul *= a.nblock[d]; }
        long blo[GA_MAX_DIM], bhi[GA_MAX_DIM];
        block_elems(a, proc, blo, bhi);
        o.proc = proc;
        for (int d = 0; d < nd; d++) {
            o.plo[d] = std::max(lo[d], blo[d]);
            o.phi[d] = std::min(hi[d], bhi[d]);
            o.ldrem[d] = bhi[d] - blo[d] + 1;
            o.blo[d] = blo[d];
        }
        owners.push_back(o);
        int d = 0;
        while (d < nd && ++bi[d] > b1[d]) { bi[d] = b0[d]; ++d; }
        if (d == nd) break;
    }
    // remote owners first, then the local one (onesided.c:1387-1400); the
    // strided variants keep the iterator's order (gai_iterator_next)
    if (!skip)
        std::stable_partition(owners.begin(), owners.end(), [&](const Owner &o) { return o.proc != me; });
    std::vector<armci_hdl_t> hdl;
    for (size_t k = 0; k < owners.size(); ++k) {
        Owner &o = owners[k];
        int count[2 * GA_MAX_DIM], stride_rem[2 * GA_MAX_DIM], stride_loc[2 * GA_MAX_DIM];
        int levels = nd - 1;
        char *pbuf, *prem;
        if (skip) {
            // gai_correct_strided_patch (onesided.c:4051-4070): first/last selected element
            bool empty = false;
            for (int d = 0; d < nd; d++) {
                long delta = o.plo[d] - lo[d];
                if (delta % skip[d]) o.plo[d] = o.plo[d] - delta % skip[d] + skip[d];
                delta = o.phi[d] - lo[d];
                if (delta % skip[d]) o.phi[d] -= delta % skip[d];
                if (o.phi[d] < o.plo[d]) empty = true;
            }
            if (empty) continue;
            // gai_FindOffset(blo, plo, ldrem) (4204-4216): remote offset of plo
            long roff = 0, rf = 1;
            for (int d = 0; d < nd; d++) { roff += (o.plo[d] - o.blo[d]) * rf; if (d < nd - 1) rf *= o.ldrem[d]; }
            prem = (char *)a.ptr[o.proc] + (long)size * roff;
            // gai_ComputePatchIndexWithSkip (4178-4202): the local buffer holds only
            // the selected elements
            long idx = (o.plo[0] - lo[0]) / skip[0];
            for (int d = 0; d < nd - 1; d++) idx += ld[d] * ((o.plo[d + 1] - lo[d + 1]) / skip[d + 1]);
            pbuf = (char *)buf + (long)size * idx;
            // gai_ComputeCountWithSkip (4077-4100, the "#if 1" form): one element per
            // run, then the selected elements of every dimension as stride levels
            count[0] = size;
            for (int d = 0; d < nd; d++) count[d + 1] = (int)((o.phi[d] - o.plo[d]) / skip[d] + 1);
            levels = nd;
            // gai_SetStrideWithSkip (4135-4150, "#if 1"); the reference also reads
            // ld[ndim-1], past the ndim-1 given, for a stride it never passes on
            stride_rem[0] = stride_loc[0] = size;
            for (int d = 0; d < nd; d++) {
                stride_rem[d + 1] = stride_rem[d];
                stride_rem[d] *= (int)skip[d];
                stride_rem[d + 1] *= (int)o.ldrem[d];
                stride_loc[d + 1] = stride_loc[d];
                if (d < nd - 1) stride_loc[d + 1] *= (int)ld[d];
            }
        } else {
            // gam_ComputePatchIndex (onesided.c:330-337)
            long idx = o.plo[0] - lo[0], factor = 1;
            for (int d = 0; d < nd - 1; d++) { factor *= ld[d]; idx += factor * (o.plo[d + 1] - lo[d + 1]); }
            pbuf = (char *)buf + (long)size * idx;
            // remote address: owner's block base + offset of plo in its column-major block
            long roff = 0, rf = 1;
            for (int d = 0; d < nd; d++) { roff += (o.plo[d] - o.blo[d]) * rf; rf *= o.ldrem[d]; }
            prem = (char *)a.ptr[o.proc] + (long)size * roff;
            for (int d = 0; d < nd; d++) count[d] = (int)(o.phi[d] - o.plo[d] + 1);   // gam_ComputeCount
            count[0] *= size;
            stride_rem[0] = stride_loc[0] = size;                                       // gam_setstride
            for (int d = 0; d < nd - 1; d++) {
                stride_rem[d] *= (int)o.ldrem[d];
                stride_loc[d] *= (int)ld[d];
                stride_rem[d + 1] = stride_rem[d];
                stride_loc[d + 1] = stride_loc[d];
            }
        }
        if (kind == GA_ACC && o.proc == me) {
            long e = 1;
            for (int d = 0; d < nd; d++) e *= (o.phi[d] - o.plo[d]) / (skip ? skip[d] : 1) + 1;
            g_stat.accloc += (double)size * e;
        }
        const bool last = !nb && (skip || k + 1 == owners.size());
        armci_hdl_t h = -1;
        if (kind == GA_ACC) {
            if (last) ARMCI_AccS(a.optype, alpha, pbuf, stride_loc, prem, stride_rem, count, levels, o.proc);
            else ARMCI_NbAccS(a.optype, alpha, pbuf, stride_loc, prem, stride_rem, count, levels, o.proc, &h);
        } else if (kind == GA_PUT) {
            if (last) ARMCI_PutS(pbuf, stride_loc, prem, stride_rem, count, levels, o.proc);
            else ARMCI_NbPutS(pbuf, stride_loc, prem, stride_rem, count, levels, o.proc, &h);
        } else {
            if (last) ARMCI_GetS(prem, stride_rem, pbuf, stride_loc, count, levels, o.proc);
            else ARMCI_NbGetS(prem, stride_rem, pbuf, stride_loc, count, levels, o.proc, &h);
        }
        if (h >= 0) hdl.push_back(h);
    }
    if (nb) {
        nb->insert(nb->end(), hdl.begin(), hdl.end());
        return;
    }
    for (armci_hdl_t &h : hdl) ARMCI_Wait(&h);   // nga_wait_internal
    if (kind == GA_GET) comex_fence_all(COMEX_GROUP_WORLD);   // data is in `buf` on return
}

// ---- gather / scatter / scatter-accumulate --------------------------------
// gai_gatscat (onesided.c:2747-3370, the default build: USE_GATSCAT_NEW is not
// defined): locate the owner of every subscript (pnga_locate), group the
// elements by owner -- owners in ascending rank order, elements in input order
// within an owner -- and issue ONE ARMCI_GetV / PutV / AccV per owner with
// `bytes = elemsize` and the (local, remote) address pairs (gam_Loc_ptr).
// Repeated subscripts of a scatter-accumulate are applied in that order (the
// io-vector path applies the pairs of a repeated destination in input order).
enum GatScat { GS_GATHER, GS_SCATTER, GS_SCATTER_ACC };


// per-call buffers kept across calls: a scatter of millions of elements would
// otherwise page-fault its way through fresh arrays every call
template <class T> static T *grow(std::vector<T> &v, size_t n) {
    if (v.size() < n) v.resize(n);
    return v.data();
}

// Subscripts arrive in C order (capi.c:3026-3160: row-major, 0-based, as an
// array of pointers or one flat array); they are read in place, reversed and
// made 1-based per element rather than copied into a Fortran array first.
// Locating owners and grouping the pairs is a stable counting sort by owner,
// split over host threads for large calls: every thread locates a contiguous
// range of elements and counts per owner, the counts are prefix-summed owner
// by owner in thread order, and every thread locates its range again and writes
// the pairs at its own offsets -- owners ascending, input order within an owner,
// as with one thread.  Locating twice (a few integer operations per element) is
// cheaper than storing each element's owner and offset between the passes: the
// call is bound by host memory traffic, 32 bytes per element this way against 48
// (NGA_Scatter_acc_flat of 4 Mi elements: profiles/r05/scatter2, scatter3).
// host threads that locate owners and group pairs (one per 128 Ki elements, up to 8;
// the former COMEX_AMD_GS_THREADS knob, settled: the box's host share is 16 cores)
static int gs_threads() { return 8; }

struct GsCtx {
    const GArray *a;
    int *const *csubs;
    const int *cflat;
    const long *blo, *ext;   // every owner's block: first index and extents
    char *v;
    int size;
};

static inline void gs_locate(const GsCtx &c, long k, int *pr_out, long *off_out) {
    const GArray &a = *c.a;
    const int nd = a.ndim;
    const int *cs = c.csubs ? c.csubs[k] : c.cflat + k * nd;
    long sub[GA_MAX_DIM];
    int pr = 0, mul = 1;
    for (int d = 0; d < nd; d++) {   // locate(): the owner's block along each dimension
        sub[d] = (long)cs[nd - 1 - d] + 1;
        if (sub[d] < 1 || sub[d] > a.dims[d]) fatal("gather/scatter: invalid subscript of element %ld", k);
        if (a.nblock[d] > 1) {
            const std::vector<long> &m = a.map[d];
            pr += (int)(std::upper_bound(m.begin(), m.end(), sub[d]) - m.begin() - 1) * mul;
        }
        mul *= a.nblock[d];
    }
    long o = 0, f = 1;
    const long *bl = c.blo + (size_t)pr * nd, *ex = c.ext + (size_t)pr * nd;
    for (int d = 0; d < nd; d++) { o += (sub[d] - bl[d]) * f; f *= ex[d]; }
    *pr_out = pr;
    *off_out = o;
}

static void gatscat(GatScat op, int g_a, void *v, int *const *csubs, const int *cflat, long nv, void *alpha) {
    if (nv < 1) return;   // pnga_gather / pnga_scatter: nv < 1 returns
    GArray &a = arr(g_a);
    const int me = my_rank(), np = world_size();
    const int size = a.elemsize, nd = a.ndim;
    static std::vector<void *> s_loc, s_rem;
    std::vector<long> blo((size_t)a.nproc_grid * nd), ext((size_t)a.nproc_grid * nd);
    for (int p = 0; p < a.nproc_grid; ++p) {
        long lo[GA_MAX_DIM], hi[GA_MAX_DIM];
        block_elems(a, p, lo, hi);
        for (int d = 0; d < nd; ++d) {
            blo[(size_t)p * nd + d] = lo[d];
            ext[(size_t)p * nd + d] = hi[d] - lo[d] + 1;
        }
    }
    const GsCtx c{&a, csubs, cflat, blo.data(), ext.data(), (char *)v, size};
    void **loc = grow(s_loc, (size_t)nv), **rem = grow(s_rem, (size_t)nv);
    const int P = np;
    // one thread per 128 Ki elements, at most gs_threads() (COMEX_AMD_GS_THREADS, default 8)
    const int T = (int)std::max(1L, std::min<long>(gs_threads(), nv >> 17));
    std::vector<long> cnt((size_t)T * P, 0);   // cnt[t*P + p]: elements of thread t owned by p
    auto range = [&](int t, long *k0, long *k1) { *k0 = nv * t / T; *k1 = nv * (t + 1) / T; };
    auto locate = [&](int t) {
        long k0, k1;
        range(t, &k0, &k1);
        std::vector<long> ct(P, 0);   // thread-local: neighbours' counters share cache lines
        for (long k = k0; k < k1; k++) {
            int pr;
            long o;
            gs_locate(c, k, &pr, &o);
            ct[pr]++;
        }
        std::copy(ct.begin(), ct.end(), &cnt[(size_t)t * P]);
    };
    std::vector<long> pos((size_t)T * P);      // pos[t*P + p]: next slot of thread t's owner-p pairs
    auto place = [&](int t) {
        long k0, k1;
        range(t, &k0, &k1);
        std::vector<long> pt(&pos[(size_t)t * P], &pos[(size_t)t * P] + P);
        for (long k = k0; k < k1; k++) {
            int pr;
            long o;
            gs_locate(c, k, &pr, &o);
            const long j = pt[pr]++;
            loc[j] = c.v + (long)size * k;
            rem[j] = (char *)a.ptr[pr] + (long)size * o;
        }
    };
    auto run = [&](const std::function<void(int)> &fn) {   // on libga_amd's host worker pool
        if (T == 1) { fn(0); return; }
        if (gaamd_host_parallel(T, [](int t, void *f) { (*(const std::function<void(int)> *)f)(t); },
                                (void *)&fn))
            fatal("gather/scatter: host pool refused %d threads", T);
    };
    if (a.nproc_grid == 1) {
        // one block: every element is its owner's (rank 0 of the grid) -- no counting pass
        // (the placing pass still checks every subscript)
        for (int t = 0; t < T; ++t) {
            long k0, k1;
            range(t, &k0, &k1);
            cnt[(size_t)t * P] = k1 - k0;
        }
    } else {
        run(locate);
    }
    std::vector<long> nelem(P, 0), first(P, 0);
    long acc = 0;
    for (int p = 0; p < P; p++) {
        first[p] = acc;
        for (int t = 0; t < T; t++) {
            pos[(size_t)t * P + p] = acc;
            acc += cnt[(size_t)t * P + p];
        }
        nelem[p] = acc - first[p];
    }
    run(place);
    double &tot = op == GS_GATHER ? g_stat.gattot : g_stat.scatot;
    double &lcl = op == GS_GATHER ? g_stat.gatloc : g_stat.scaloc;
    (op == GS_GATHER ? g_stat.numgat : g_stat.numsca)++;
    tot += (double)size * nv;
    lcl += (double)size * nelem[me];
    for (int p = 0; p < np; p++) {
        if (!nelem[p]) continue;
        armci_giov_t desc;
        desc.bytes = size;
        desc.ptr_array_len = (int)nelem[p];
        int rc;
        if (op == GS_GATHER) {
            desc.src_ptr_array = &rem[first[p]];
            desc.dst_ptr_array = &loc[first[p]];
            rc = ARMCI_GetV(&desc, 1, p);
        } else {
            desc.src_ptr_array = &loc[first[p]];
            desc.dst_ptr_array = &rem[first[p]];
            rc = op == GS_SCATTER ? ARMCI_PutV(&desc, 1, p) : ARMCI_AccV(a.optype, alpha, &desc, 1, p);
        }
        if (rc) fatal("gather/scatter failed in armci (%d)", rc);
    }
    if (op == GS_GATHER) comex_fence_all(COMEX_GROUP_WORLD);   // data is in `v` on return
}

// C (row-major, 0-based) -> Fortran (column-major, 1-based): capi.c:54-61
static void c2f_index(int nd, const int *c, long *f) { for (int i = 0; i < nd; i++) f[nd - i - 1] = (long)c[i] + 1; }
static void c2f(int nd, const int *c, long *f) { for (int i = 0; i < nd; i++) f[nd - i - 1] = c[i]; }

// a patch in internal order (Fortran order, 1-based, inclusive), from the C subscripts of
// a call; without subscripts (clo == nullptr) the whole array
struct Patch {
    long lo[GA_MAX_DIM], hi[GA_MAX_DIM];
    Patch() {}
    Patch(const GArray &a, const int *clo, const int *chi) {
        if (clo) {
            c2f_index(a.ndim, clo, lo);
            c2f_index(a.ndim, chi, hi);
        } else {
            for (int d = 0; d < a.ndim; d++) { lo[d] = 1; hi[d] = a.dims[d]; }
        }
    }
    Patch(long lo0, long hi0) { lo[0] = lo0; hi[0] = hi0; }   // elements [lo0, hi0] of a 1-D array
};

// NGA_Put's (lo, hi, ld) in internal order
struct PatchLd {
    Patch p;
    long ld[GA_MAX_DIM] = {0};
    PatchLd(const GArray &a, const int *clo, const int *chi, const int *cld) : p(a, clo, chi) {
        if (a.ndim > 1) c2f(a.ndim - 1, cld, ld);
    }
};

// pnga_allocate (base.c:2550-2630): the block sizes and the process grid ddb picks for
// `npes` processes from dims and chunk (Fortran order; chunk[0] == 0: no chunk given)
static void proc_grid(int ndim, const long *fdims, const long *fchunk, long npes, long *blk, long *pe) {
    if (fchunk[0] != 0)
        for (int d = 0; d < ndim; d++) blk[d] = std::min(fchunk[d], fdims[d]);
    else
        for (int d = 0; d < ndim; d++) blk[d] = -1;
    for (int d = 0; d < ndim; d++) if (fdims[d] == 1) blk[d] = 1;
    ddb(ndim, fdims, npes, blk, pe);
}

// Which armci_msg_?gop carries which GA type: the one on the type's real component type.
// f(buf as a pointer to that type, the gop) -- the caller passes its count (2 for the parts
// of a complex value) and operator, and reads the typed result.
template <class F>
static void gop_by_type(int type, void *buf, F &&f) {
    switch (type) {
    case C_INT: f((int *)buf, armci_msg_igop); break;
    case C_LONG: f((long *)buf, armci_msg_lgop); break;
    case C_FLOAT:
    case C_SCPL: f((float *)buf, armci_msg_fgop); break;
    default: f((double *)buf, armci_msg_dgop); break;
    }
}

}  // namespace gaamd_ga

using namespace gaamd_ga;

extern "C" {

int GA_Initialize(void) { return ARMCI_Init(); }
static void destroy(int g_a) {
    GArray &a = arr(g_a);
    comex_free(a.ptr[my_rank()], COMEX_GROUP_WORLD);
    a.live = false;
    a.ptr.clear();
}

static void sprs_release_all();   // the HBM of sparse arrays still alive (below)

void GA_Terminate(void) {
    sprs_release_all();
    for (size_t i = 0; i < g_arrays.size(); ++i)
        if (g_arrays[i].live) destroy((int)i + 1);
    ARMCI_Finalize();
}
int GA_Nodeid(void) { return my_rank(); }
int GA_Nnodes(void) { return world_size(); }
void GA_Sync(void) { comex_barrier(COMEX_GROUP_WORLD); }
void GA_Error(char *msg, int code) { comex_error(msg, code); }

int NGA_Create(int type, int ndim, int dims[], char *name, int chunk[]) {
    if (ndim < 1 || ndim > GA_MAX_DIM) return 0;
    GArray a;
    a.type = type;
    a.ndim = ndim;
    a.name = name ? name : "";
    a.elemsize = type_size(type, &a.optype);
    long fdims[GA_MAX_DIM], fchunk[GA_MAX_DIM] = {0};
    c2f(ndim, dims, fdims);
    if (chunk) c2f(ndim, chunk, fchunk);
    for (int d = 0; d < ndim; d++) {
        if (fdims[d] < 1) fatal("NGA_Create: dimension %d is %ld", d, fdims[d]);
        a.dims[d] = fdims[d];
    }
    // pnga_allocate (base.c:2550-2630)
    long blk[GA_MAX_DIM], pe[GA_MAX_DIM];
    proc_grid(ndim, fdims, fchunk, world_size(), blk, pe);
    for (int d = 0; d < ndim; d++) {
        long pcut;
        if (fchunk[d] > 1) {
            const long ddim = (fdims[d] - 1) / std::min(fchunk[d], fdims[d]) + 1;
            pcut = ddim - (blk[d] - 1) * pe[d];
        } else {
            pcut = fdims[d] - (blk[d] - 1) * pe[d];
        }
        long i = 0, nblock = 0;
        for (long p = 0; p < pe[d] && i < fdims[d]; p++, nblock++) {
            long b = blk[d];
            if (p >= pcut) b = b - 1;
            a.map[d].push_back(i + 1);
            if (fchunk[d] > 1) b *= std::min(fchunk[d], fdims[d]);
            i += b;
        }
        a.nblock[d] = (int)std::min(pe[d], nblock);
        a.map[d].resize(a.nblock[d]);
    }
    return allocate(a);
}

int NGA_Create_irreg(int type, int ndim, int dims[], char *name, int block[], int map[]) {
    if (ndim < 1 || ndim > GA_MAX_DIM) return 0;
    GArray a;
    a.type = type;
    a.ndim = ndim;
    a.name = name ? name : "";
    a.elemsize = type_size(type, &a.optype);
    long fdims[GA_MAX_DIM];
    c2f(ndim, dims, fdims);
    for (int d = 0; d < ndim; d++) a.dims[d] = fdims[d];
    // copy_map (capi.c): C dimension i's block starts follow those of i-1 in `map`
    int off[GA_MAX_DIM];
    for (int i = 0, o = 0; i < ndim; i++) { off[i] = o; o += block[i]; }
    for (int i = 0; i < ndim; i++) {
        const int fd = ndim - 1 - i;
        a.nblock[fd] = block[i];
        for (int k = 0; k < block[i]; k++) a.map[fd].push_back((long)map[off[i] + k] + 1);
    }
    return allocate(a);
}

void GA_Destroy(int g_a) { destroy(g_a); }

void GA_Zero(int g_a) {
    GArray &a = arr(g_a);
    const int me = my_rank();
    long lo[GA_MAX_DIM], hi[GA_MAX_DIM];
    const long n = block_elems(a, me, lo, hi);
    // pnga_zero (global.nalg.c:60-90) is collective and syncs first: no rank may
    // zero its block while another still reads or writes it
    comex_barrier(COMEX_GROUP_WORLD);
    zero_block(a.ptr[me], (size_t)n * a.elemsize);
    comex_barrier(COMEX_GROUP_WORLD);   // fences (syncs every library stream) + barrier
}

void NGA_Distribution(int g_a, int iproc, int lo[], int hi[]) {
    GArray &a = arr(g_a);
    long flo[GA_MAX_DIM], fhi[GA_MAX_DIM];
    block_elems(a, iproc, flo, fhi);
    for (int i = 0; i < a.ndim; i++) {   // COPYINDEX_F2C
        lo[a.ndim - i - 1] = (int)flo[i] - 1;
        hi[a.ndim - i - 1] = (int)fhi[i] - 1;
    }
}

// pnga_locate_num_blocks (base.c:5591-5627): the region is bounds-checked, and the
// count is only defined for block-cyclic distributions; an array with a map
// (NGA_Create's regular blocks or NGA_Create_irreg's) is GA's REGULAR type, for which
// the reference returns -1 -- so does this.
int NGA_Locate_num_blocks(int g_a, int lo[], int hi[]) {
    GArray &a = arr(g_a);
    const Patch p(a, lo, hi);
    for (int d = 0; d < a.ndim; d++)
        if (p.lo[d] < 1 || p.hi[d] > a.dims[d] || p.lo[d] > p.hi[d]) fatal("Requested region out of bounds");
    return -1;
}

static void c_patch(GaOp kind, int g_a, int lo[], int hi[], void *buf, int ld[], void *alpha) {
    const PatchLd f(arr(g_a), lo, hi, ld);
    patch_op(kind, g_a, f.p.lo, f.p.hi, buf, f.ld, alpha);
}

// ---- strided (skip) and non-blocking variants: capi.c:1990-2060, 2103-2190 ----
static void c_strided(GaOp kind, int g_a, int lo[], int hi[], int skip[], void *buf, int ld[], void *alpha) {
    GArray &a = arr(g_a);
    const PatchLd f(a, lo, hi, ld);
    long fskip[GA_MAX_DIM];
    c2f(a.ndim, skip, fskip);   // COPYC2F: reversed, no +1
    for (int d = 0; d < a.ndim; d++)
        if (fskip[d] < 1) fatal("nga_strided: invalid skip %ld along coordinate %d", fskip[d], d);
    patch_op(kind, g_a, f.p.lo, f.p.hi, buf, f.ld, alpha, fskip);
}

void NGA_Strided_acc(int g_a, int lo[], int hi[], int skip[], void *buf, int ld[], void *alpha) {
    c_strided(GA_ACC, g_a, lo, hi, skip, buf, ld, alpha);
}
void NGA_Strided_put(int g_a, int lo[], int hi[], int skip[], void *buf, int ld[]) {
    c_strided(GA_PUT, g_a, lo, hi, skip, buf, ld, nullptr);
}
void NGA_Strided_get(int g_a, int lo[], int hi[], int skip[], void *buf, int ld[]) {
    c_strided(GA_GET, g_a, lo, hi, skip, buf, ld, nullptr);
    comex_fence_all(COMEX_GROUP_WORLD);
}

// GA non-blocking handle -> the ARMCI handles of its owners (the reference's
// gai_nbhdl agg lists, onesided.c:120-300); value = slot + 1, 0 = done
struct GaNb { bool used = false; bool get = false; std::vector<armci_hdl_t> h; };
static std::vector<GaNb> g_ga_nb;

static void c_nb(GaOp kind, int g_a, int lo[], int hi[], void *buf, int ld[], void *alpha, ga_nbhdl_t *nbhandle) {
    const PatchLd f(arr(g_a), lo, hi, ld);
    size_t slot = 0;
    while (slot < g_ga_nb.size() && g_ga_nb[slot].used) ++slot;
    if (slot == g_ga_nb.size()) g_ga_nb.emplace_back();
    GaNb &n = g_ga_nb[slot];
    n.used = true;
    n.get = kind == GA_GET;
    n.h.clear();
    patch_op(kind, g_a, f.p.lo, f.p.hi, buf, f.ld, alpha, nullptr, &n.h);
    *nbhandle = (ga_nbhdl_t)(slot + 1);
}

void NGA_NbAcc(int g_a, int lo[], int hi[], void *buf, int ld[], void *alpha, ga_nbhdl_t *nbhandle) {
    c_nb(GA_ACC, g_a, lo, hi, buf, ld, alpha, nbhandle);
}
void NGA_NbPut(int g_a, int lo[], int hi[], void *buf, int ld[], ga_nbhdl_t *nbhandle) {
    c_nb(GA_PUT, g_a, lo, hi, buf, ld, nullptr, nbhandle);
}
void NGA_NbGet(int g_a, int lo[], int hi[], void *buf, int ld[], ga_nbhdl_t *nbhandle) {
    c_nb(GA_GET, g_a, lo, hi, buf, ld, nullptr, nbhandle);
}
void NGA_NbWait(ga_nbhdl_t *nbhandle) {   // pnga_nbwait -> nga_wait_internal (onesided.c:368)
    if (!nbhandle || *nbhandle <= 0 || (size_t)*nbhandle > g_ga_nb.size()) return;
    GaNb &n = g_ga_nb[(size_t)*nbhandle - 1];
    if (!n.used) return;
    for (armci_hdl_t &h : n.h) ARMCI_Wait(&h);
    if (n.get) comex_fence_all(COMEX_GROUP_WORLD);   // data is in `buf` on return
    n.h.clear();
    n.used = false;
    *nbhandle = 0;
}

void NGA_Acc(int g_a, int lo[], int hi[], void *buf, int ld[], void *alpha) { c_patch(GA_ACC, g_a, lo, hi, buf, ld, alpha); }
void NGA_Put(int g_a, int lo[], int hi[], void *buf, int ld[]) { c_patch(GA_PUT, g_a, lo, hi, buf, ld, nullptr); }
void NGA_Get(int g_a, int lo[], int hi[], void *buf, int ld[]) { c_patch(GA_GET, g_a, lo, hi, buf, ld, nullptr); }

void NGA_Access(int g_a, int lo[], int hi[], void *ptr, int ld[]) {
    GArray &a = arr(g_a);
    const int me = my_rank();
    long blo[GA_MAX_DIM], bhi[GA_MAX_DIM];
    block_elems(a, me, blo, bhi);
    const Patch p(a, lo, hi);
    long off = 0, f = 1;
    for (int d = 0; d < a.ndim; d++) {
        if (p.lo[d] < blo[d] || p.hi[d] > bhi[d]) fatal("NGA_Access: patch not local");
        off += (p.lo[d] - blo[d]) * f;
        f *= bhi[d] - blo[d] + 1;
    }
    comex_fence_all(COMEX_GROUP_WORLD);   // pending writes land before the caller reads
    *(char **)ptr = (char *)a.ptr[me] + off * a.elemsize;
    for (int i = 0; i < a.ndim - 1; i++) ld[a.ndim - 2 - i] = (int)(bhi[i] - blo[i] + 1);
}

void NGA_Release(int g_a, int lo[], int hi[]) { (void)arr(g_a); (void)lo; (void)hi; }
void NGA_Release_update(int g_a, int lo[], int hi[]) { (void)arr(g_a); (void)lo; (void)hi; }

// capi.c:3026-3160 (NGA_Scatter*, NGA_Gather*): C subscripts, converted per element in gatscat
void NGA_Scatter(int g_a, void *v, int *subsArray[], int n) {
    gatscat(GS_SCATTER, g_a, v, subsArray, nullptr, n, nullptr);
}
void NGA_Scatter_flat(int g_a, void *v, int subsArray[], int n) {
    gatscat(GS_SCATTER, g_a, v, nullptr, subsArray, n, nullptr);
}
void NGA_Scatter_acc(int g_a, void *v, int *subsArray[], int n, void *alpha) {
    gatscat(GS_SCATTER_ACC, g_a, v, subsArray, nullptr, n, alpha);
}
void NGA_Scatter_acc_flat(int g_a, void *v, int subsArray[], int n, void *alpha) {
    gatscat(GS_SCATTER_ACC, g_a, v, nullptr, subsArray, n, alpha);
}
void NGA_Gather(int g_a, void *v, int *subsArray[], int n) {
    gatscat(GS_GATHER, g_a, v, subsArray, nullptr, n, nullptr);
}
void NGA_Gather_flat(int g_a, void *v, int subsArray[], int n) {
    gatscat(GS_GATHER, g_a, v, nullptr, subsArray, n, nullptr);
}

void GA_Get_proc_grid(int g_a, int dims[]) {
    GArray &a = arr(g_a);
    for (int i = 0; i < a.ndim; i++) dims[a.ndim - 1 - i] = a.nblock[i];
}

// The process grid NGA_Create picks for `npes` processes (C order), without
// allocating anything: host-only, used by the CPU tests of the restated ddb.
int gaamd_ga_proc_grid(int ndim, const int *dims, const int *chunk, int npes, int *grid) {
    if (ndim < 1 || ndim > GA_MAX_DIM || npes < 1) return -1;
    long fdims[GA_MAX_DIM], fchunk[GA_MAX_DIM] = {0}, blk[GA_MAX_DIM], pe[GA_MAX_DIM];
    c2f(ndim, dims, fdims);
    if (chunk) c2f(ndim, chunk, fchunk);
    proc_grid(ndim, fdims, fchunk, npes, blk, pe);
    for (int i = 0; i < ndim; i++) grid[ndim - 1 - i] = (int)pe[i];
    return 0;
}

// ---- computing on arrays where they lie ------------------------------------------
// GA_Fill / GA_Scale / GA_Add / GA_Copy / GA_?dot and their patch forms
// (global/src/global.npatch.c, global.nalg.c; capi.c names and argument orders).
// Every block is in HBM, so each rank runs one gfx950 kernel on its own part of the
// patch (ga_amd.h gaamd_patch_*) where the reference runs a host loop.  All are
// collective with the reference's sync discipline: GA_Sync on entry, the local work
// on gaamd_stream(), a stream sync, GA_Sync on exit; the dot products end in the sum
// over ranks (armci_msg_?gop "+", as pnga_gop) instead of the exit sync.
//   fast path ("compatible", npatch.c:2698-2737, 1207-1247): equal block maps and
//     equal patches -- every rank's operands share its block's leading dimensions;
//   general path: the odd operand is copied into a GA_Duplicate of the output (of
//     g_a for dot) with NGA_Copy_patch first, as the reference does.
// Transposes, reshapes and arrays in a host segment abort: nothing here computes on
// the host.

// this rank's part of a patch: its address in the block, the counts and the byte
// strides the block's extents give
struct Sub {
    bool any = false;
    char *p = nullptr;
    long plo[GA_MAX_DIM], phi[GA_MAX_DIM], ext[GA_MAX_DIM];
    long long count[GA_MAX_DIM], stride[GA_MAX_DIM];
    double bytes = 0;
};

static Sub own_sub(const GArray &a, const Patch &p) {
    Sub s;
    long blo[GA_MAX_DIM], bhi[GA_MAX_DIM];
    if (block_elems(a, my_rank(), blo, bhi) == 0) return s;
    for (int d = 0; d < a.ndim; d++) {
        s.plo[d] = std::max(p.lo[d], blo[d]);
        s.phi[d] = std::min(p.hi[d], bhi[d]);
        if (s.plo[d] > s.phi[d]) return s;
    }
    long long off = 0, f = 1;
    s.bytes = a.elemsize;
    for (int d = 0; d < a.ndim; d++) {
        s.ext[d] = bhi[d] - blo[d] + 1;
        off += (s.plo[d] - blo[d]) * f;
        f *= s.ext[d];
        s.count[d] = s.phi[d] - s.plo[d] + 1;
        s.stride[d] = f * a.elemsize;   // byte stride of dimension d + 1
        s.bytes *= (double)s.count[d];
    }
    s.p = (char *)a.ptr[my_rank()] + off * a.elemsize;
    s.any = true;
    return s;
}

static void need_hbm(const GArray &a, const char *what) {
    void *p = a.ptr[my_rank()];
    if (p && gaamd_segment_kind(p) == 2)
        fatal("%s: array '%s' lives in a host segment (COMEX_AMD_SEGMENT=host); "
              "computing on host-segment arrays is not supported", what, a.name.c_str());
}

static void check_patch(const GArray &a, const Patch &p, const char *what) {
    for (int d = 0; d < a.ndim; d++)
        if (p.lo[d] < 1 || p.hi[d] > a.dims[d] || p.lo[d] > p.hi[d]) fatal("%s: patch out of range in dim %d", what, d);
}

// pnga_compare_distr (base.c): equal shapes and equal block maps
static bool same_distr(const GArray &a, const GArray &b) {
    if (a.ndim != b.ndim) return false;
    for (int d = 0; d < a.ndim; d++)
        if (a.dims[d] != b.dims[d] || a.nblock[d] != b.nblock[d] || a.map[d] != b.map[d]) return false;
    return true;
}

static bool same_patch(int nd, const Patch &a, const Patch &b) {
    for (int d = 0; d < nd; d++)
        if (a.lo[d] != b.lo[d] || a.hi[d] != b.hi[d]) return false;
    return true;
}

// patches of equal rank and extents (anything else is a reshape)
static void need_same_shape(const GArray &a, const Patch &pa, const GArray &b, const Patch &pb, const char *what) {
    bool same = a.ndim == b.ndim;
    for (int d = 0; same && d < a.ndim; d++) same = pa.hi[d] - pa.lo[d] == pb.hi[d] - pb.lo[d];
    if (!same)
        fatal("%s: patches of different rank or extents (a reshape) are not supported", what);
}

static void need_no_trans(char t, const char *what) {
    if (t != 'n' && t != 'N') fatal("%s: transposed patches (trans '%c') are not supported", what, t);
}

// how a launcher's return code ends a collective call.  zero_ok: GAAMD_ZERO_DIVISOR (the
// element-wise calls) is not an error here -- returns 1 for the caller to combine over ranks
static int launched(int rc, const char *what, bool zero_ok = false) {
    if (zero_ok && rc == GAAMD_ZERO_DIVISOR) return 1;
    if (rc) fatal("%s: kernel launch failed (%d)", what, rc);
    return 0;
}

static void stream_wait(const char *what) {
    if (gaamd_sync(gaamd_stream()) != 0) fatal("%s: the stream failed", what);
}

static void math_end(const char *what) {
    stream_wait(what);
    comex_barrier(COMEX_GROUP_WORLD);
}

// HBM scratch of one call, freed when it goes out of scope (or by free(), earlier)
struct Scratch {
    void *p = nullptr;
    Scratch() {}
    Scratch(Scratch &&o) : p(o.p) { o.p = nullptr; }
    Scratch &operator=(Scratch &&o) {
        std::swap(p, o.p);
        return *this;
    }
    ~Scratch() { free(); }
    void *alloc(size_t bytes) { return p = gaamd_dev_malloc(bytes); }   // null: the caller aborts with its message
    void free() {
        if (p) gaamd_dev_free(p);
        p = nullptr;
    }
};

int GA_Duplicate(int g_a, char *array_name) {
    GArray n = arr(g_a);   // type, shape and block map (pnga_duplicate, base.c)
    n.name = array_name ? array_name : "";
    n.live = false;
    n.ptr.clear();
    return allocate(n);
}

int GA_Compare_distr(int g_a, int g_b) { return same_distr(arr(g_a), arr(g_b)) ? 0 : 1; }   // capi.c:2375: 0 = same

void NGA_Inquire(int g_a, int *type, int *ndim, int dims[]) {
    GArray &a = arr(g_a);
    *type = a.type;
    *ndim = a.ndim;
    for (int i = 0; i < a.ndim; i++) dims[a.ndim - 1 - i] = (int)a.dims[i];
}

int gaamd_ga_live_arrays(void) {
    int n = 0;
    for (const GArray &a : g_arrays) n += a.live ? 1 : 0;
    return n;
}

enum MapKind { M_FILL, M_SCALE };
static void map_patch(MapKind kind, int g_a, const Patch &p, const void *val, const char *what) {
    GArray &a = arr(g_a);
    need_hbm(a, what);
    check_patch(a, p, what);
    comex_barrier(COMEX_GROUP_WORLD);   // fences every pending one-sided operation, then syncs
    const Sub s = own_sub(a, p);
    (kind == M_FILL ? g_stat.numfill : g_stat.numscale)++;
    if (s.any) {
        launched(kind == M_FILL ? gaamd_patch_fill(a.optype, val, s.p, s.stride, s.count, a.ndim, gaamd_stream())
                                : gaamd_patch_scale(a.optype, val, s.p, s.stride, s.count, a.ndim, gaamd_stream()),
                 what);
        g_stat.mathloc += s.bytes * (kind == M_FILL ? 1 : 2);
    }
    math_end(what);
}

// a block-local copy of any size through gaamd_strided's int geometry: contiguous
// dimensions merged, a 1-D run in pieces of 1 GiB
static void local_copy(const Sub &s, const Sub &t, int nd, int esz, const char *what) {
    long long cnt[GA_MAX_DIM] = {0}, ss[GA_MAX_DIM] = {0}, ds[GA_MAX_DIM] = {0};
    int n = nd;
    for (int d = 0; d < nd; d++) { cnt[d] = s.count[d]; ss[d] = s.stride[d]; ds[d] = t.stride[d]; }
    cnt[0] *= esz;   // bytes
    while (n > 1 && ss[0] == cnt[0] && ds[0] == cnt[0]) {
        cnt[0] *= cnt[1];
        for (int d = 1; d + 1 < n; d++) { cnt[d] = cnt[d + 1]; ss[d - 1] = ss[d]; ds[d - 1] = ds[d]; }
        --n;
    }
    const long long piece = 1ll << 30;
    if (n == 1) {
        for (long long o = 0; o < cnt[0]; o += piece) {
            int c = (int)std::min(piece, cnt[0] - o);
            if (gaamd_strided(GAAMD_OP_COPY, nullptr, s.p + o, nullptr, t.p + o, nullptr, &c, 0, gaamd_stream()))
                fatal("%s: copy kernel failed", what);
        }
        return;
    }
    int ic[GA_MAX_DIM], is[GA_MAX_DIM], id[GA_MAX_DIM];
    for (int d = 0; d < n; d++) {
        if (cnt[d] >= (1ll << 31) || (d < n - 1 && (ss[d] >= (1ll << 31) || ds[d] >= (1ll << 31))))
            fatal("%s: a strided block-local copy past 2 GiB is not supported", what);
        ic[d] = (int)cnt[d];
        is[d] = (int)ss[d];
        id[d] = (int)ds[d];
    }
    if (gaamd_strided(GAAMD_OP_COPY, nullptr, s.p, is, t.p, id, ic, n - 1, gaamd_stream()))
        fatal("%s: copy kernel failed", what);
}

// pnga_copy_patch (global.npatch.c:560-935), trans 'N', equal rank and extents: each
// rank cuts the source patch by its own block and puts that part, from HBM, into g_b
// at the shifted position; where both blocks coincide it is one local copy kernel
static void copy_patch(int g_a, const Patch &pa, int g_b, const Patch &pb, const char *what) {
    GArray &a = arr(g_a), &b = arr(g_b);
    if (a.type != b.type) fatal("%s: types of '%s' and '%s' differ", what, a.name.c_str(), b.name.c_str());
    need_hbm(a, what);
    need_hbm(b, what);
    if (a.ndim != b.ndim) fatal("%s: arrays of different rank (a reshape) are not supported", what);
    check_patch(a, pa, what);
    check_patch(b, pb, what);
    need_same_shape(a, pa, b, pb, what);
    const int nd = a.ndim;
    if (g_a == g_b && !same_patch(nd, pa, pb)) {
        bool meet = true;
        for (int d = 0; d < nd; d++) meet = meet && pa.lo[d] <= pb.hi[d] && pb.lo[d] <= pa.hi[d];
        if (meet) fatal("%s: overlapping patches of one array", what);   // npatch.c: "arrays overlap"
    }
    comex_barrier(COMEX_GROUP_WORLD);
    g_stat.numcopy++;
    const Sub s = own_sub(a, pa);
    if (s.any && !(g_a == g_b && same_patch(nd, pa, pb))) {
        Patch dst;
        long ld[GA_MAX_DIM];
        bool here = same_distr(a, b);
        for (int d = 0; d < nd; d++) {
            dst.lo[d] = pb.lo[d] + (s.plo[d] - pa.lo[d]);
            dst.hi[d] = dst.lo[d] + (s.phi[d] - s.plo[d]);
            ld[d] = s.ext[d];
            here = here && dst.lo[d] == s.plo[d];
        }
        if (here) {
            const Sub t = own_sub(b, dst);
            local_copy(s, t, nd, a.elemsize, what);
        } else {
            patch_op(GA_PUT, g_b, dst.lo, dst.hi, s.p, ld, nullptr);
        }
        g_stat.mathloc += 2 * s.bytes;
    }
    math_end(what);
}

// RECIP / DIV: after the kernel has completed and math_end's barrier, the ranks combine
// their zero-divisor flags; if any is set every rank ends here, none waits in a barrier
static void zero_divisor_end(int flag, const char *what) {
    char mx[] = "max";
    armci_msg_igop(&flag, 1, mx);
    if (flag)
        fatal("%s: zero divisor (the reference aborts at the first one; here those elements were left unwritten)",
              what);
}

// An input that does not lie on the target's block map and patch is first copied into a
// GA_Duplicate of the target, as the reference does (npatch.c:2698-2737, 1207-1247).  The
// temporaries of one call are destroyed, in the order they were made, when `Temps` goes
// out of scope.
struct Temps {
    std::vector<int> made;
    ~Temps() { for (int g : made) destroy(g); }
};

// the handle to compute with: g itself, or a temporary holding p at the target's patch
static int on_map_of(int g, const Patch &p, int g_to, const Patch &pto, const char *tmp_name, Temps &temps,
                     const char *what) {
    if (same_distr(arr(g), arr(g_to)) && same_patch(arr(g_to).ndim, p, pto)) return g;
    const int tmp = GA_Duplicate(g_to, const_cast<char *>(tmp_name));
    temps.made.push_back(tmp);
    copy_patch(g, p, tmp, pto, what);
    return tmp;
}

// c = kernel(a, b) over patches of equal shape: GA_Add's structure (npatch.c) and
// ngai_elem2_patch_'s (elem_alg.c:1851-1990), temporaries included.  `kernel` launches on
// this rank's parts and returns its zero-divisor flag; combine_zero: the ranks combine it.
typedef std::function<int(const GArray &c, const Sub &sa, const Sub &sb, const Sub &sc)> BinaryKernel;
static void binary_patch(int g_a, const Patch &pa, int g_b, const Patch &pb, int g_c, const Patch &pc, long &counter,
                         const char *tmp_name, bool combine_zero, const char *what, const BinaryKernel &kernel) {
    const int g[3] = {g_a, g_b, g_c};
    const Patch *p[3] = {&pa, &pb, &pc};
    if (arr(g_a).type != arr(g_c).type || arr(g_b).type != arr(g_c).type) fatal("%s: types of the arrays differ", what);
    for (int k = 0; k < 3; k++) need_hbm(arr(g[k]), what);
    for (int k = 0; k < 3; k++) check_patch(arr(g[k]), *p[k], what);
    for (int k = 0; k < 2; k++) need_same_shape(arr(g[k]), *p[k], arr(g_c), pc, what);
    comex_barrier(COMEX_GROUP_WORLD);
    counter++;
    int zero = 0;
    {
        Temps temps;
        int use[2];
        for (int k = 0; k < 2; k++) use[k] = on_map_of(g[k], *p[k], g_c, pc, tmp_name, temps, what);
        GArray &c = arr(g_c);
        const Sub sc = own_sub(c, pc);
        if (sc.any) {
            zero = kernel(c, own_sub(arr(use[0]), pc), own_sub(arr(use[1]), pc), sc);
            g_stat.mathloc += 3 * sc.bytes;
        }
        math_end(what);
    }
    if (combine_zero) zero_divisor_end(zero, what);
}

// every rank returns the same bits: the local sums are combined by armci_msg_?gop
static void dot_patch(int type, int g_a, char t_a, const Patch &pa, int g_b, char t_b, const Patch &pb, void *result,
                      const char *what) {
    {
        GArray &a = arr(g_a), &b = arr(g_b);
        if (a.type != type || b.type != type)
            fatal("%s: type mismatch: arrays of type %d and %d in a call for type %d", what, a.type, b.type, type);
        need_no_trans(t_a, what);
        need_no_trans(t_b, what);
        need_hbm(a, what);
        need_hbm(b, what);
        check_patch(a, pa, what);
        check_patch(b, pb, what);
        need_same_shape(a, pa, b, pb, what);
    }
    comex_barrier(COMEX_GROUP_WORLD);
    g_stat.numdot++;
    Temps temps;
    const int use_b = on_map_of(g_b, pb, g_a, pa, "ga_amd dot temporary", temps, what);
    GArray &a = arr(g_a);
    double res[2] = {0.0, 0.0};   // 16 zero bytes: the zero of every type
    const Sub sa = own_sub(a, pa);
    if (sa.any) {
        const Sub sb = own_sub(arr(use_b), pa);
        launched(gaamd_patch_dot(a.optype, sa.p, sa.stride, sb.p, sb.stride, sa.count, a.ndim, res, gaamd_stream()), what);
        g_stat.mathloc += 2 * sa.bytes;
    }
    char plus[] = "+";
    const int parts = type == C_SCPL || type == C_DCPL ? 2 : 1;
    gop_by_type(type, res, [&](auto *r, auto gop) { gop(r, parts, plus); });
    memcpy(result, res, (size_t)a.elemsize);
}

void NGA_Fill_patch(int g_a, int lo[], int hi[], void *val) {
    map_patch(M_FILL, g_a, Patch(arr(g_a), lo, hi), val, "NGA_Fill_patch");
}
void NGA_Zero_patch(int g_a, int lo[], int hi[]) {
    const double zero[2] = {0.0, 0.0};
    map_patch(M_FILL, g_a, Patch(arr(g_a), lo, hi), zero, "NGA_Zero_patch");
}
void NGA_Scale_patch(int g_a, int lo[], int hi[], void *alpha) {
    map_patch(M_SCALE, g_a, Patch(arr(g_a), lo, hi), alpha, "NGA_Scale_patch");
}
void GA_Fill(int g_a, void *value) { map_patch(M_FILL, g_a, Patch(arr(g_a), nullptr, nullptr), value, "GA_Fill"); }
void GA_Scale(int g_a, void *value) { map_patch(M_SCALE, g_a, Patch(arr(g_a), nullptr, nullptr), value, "GA_Scale"); }

void NGA_Copy_patch(char trans, int g_a, int alo[], int ahi[], int g_b, int blo[], int bhi[]) {
    need_no_trans(trans, "NGA_Copy_patch");
    const Patch pa(arr(g_a), alo, ahi), pb(arr(g_b), blo, bhi);
    copy_patch(g_a, pa, g_b, pb, "NGA_Copy_patch");
}
void GA_Copy(int g_a, int g_b) {
    const Patch pa(arr(g_a), nullptr, nullptr), pb(arr(g_b), nullptr, nullptr);
    copy_patch(g_a, pa, g_b, pb, "GA_Copy");
}

// alo == nullptr: the whole arrays (GA_Add)
static void c_add(void *alpha, int g_a, int *alo, int *ahi, void *beta, int g_b, int *blo, int *bhi, int g_c, int *clo,
                  int *chi, const char *what) {
    const Patch pa(arr(g_a), alo, ahi), pb(arr(g_b), blo, bhi), pc(arr(g_c), clo, chi);
    binary_patch(g_a, pa, g_b, pb, g_c, pc, g_stat.numadd, "ga_amd add temporary", false, what,
                 [&](const GArray &c, const Sub &sa, const Sub &sb, const Sub &sc) {
                     return launched(gaamd_patch_add(c.optype, alpha, sa.p, sa.stride, beta, sb.p, sb.stride, sc.p,
                                                     sc.stride, sc.count, c.ndim, gaamd_stream()),
                                     what);
                 });
}
void NGA_Add_patch(void *alpha, int g_a, int alo[], int ahi[], void *beta, int g_b, int blo[], int bhi[], int g_c,
                   int clo[], int chi[]) {
    c_add(alpha, g_a, alo, ahi, beta, g_b, blo, bhi, g_c, clo, chi, "NGA_Add_patch");
}
void GA_Add(void *alpha, int g_a, void *beta, int g_b, int g_c) {
    c_add(alpha, g_a, nullptr, nullptr, beta, g_b, nullptr, nullptr, g_c, nullptr, nullptr, "GA_Add");
}

// alo == nullptr: the whole arrays (GA_?dot)
static void c_dot_patch(int type, int g_a, char t_a, int *alo, int *ahi, int g_b, char t_b, int *blo, int *bhi,
                        void *res, const char *what) {
    const Patch pa(arr(g_a), alo, ahi), pb(arr(g_b), blo, bhi);
    dot_patch(type, g_a, t_a, pa, g_b, t_b, pb, res, what);
}

#define GAAMD_DOT(T, NAME, CODE)                                                                          \
    T GA_##NAME(int g_a, int g_b) {                                                                        \
        T v;                                                                                               \
        c_dot_patch(CODE, g_a, 'n', nullptr, nullptr, g_b, 'n', nullptr, nullptr, &v, "GA_" #NAME);        \
        return v;                                                                                          \
    }                                                                                                      \
    T NGA_##NAME##_patch(int g_a, char t_a, int alo[], int ahi[], int g_b, char t_b, int blo[], int bhi[]) { \
        T v;                                                                                               \
        c_dot_patch(CODE, g_a, t_a, alo, ahi, g_b, t_b, blo, bhi, &v, "NGA_" #NAME "_patch");              \
        return v;                                                                                          \
    }
GAAMD_DOT(int, Idot, C_INT)
GAAMD_DOT(long, Ldot, C_LONG)
GAAMD_DOT(float, Fdot, C_FLOAT)
GAAMD_DOT(double, Ddot, C_DBL)
GAAMD_DOT(SingleComplex, Cdot, C_SCPL)
GAAMD_DOT(DoubleComplex, Zdot, C_DCPL)
#undef GAAMD_DOT

// ---- element-wise algebra and NGA_Select_elem ------------------------------------------
// pnga_abs_value ... pnga_elem_minimum_patch (global/src/elem_alg.c) loop over the local
// block on the host; here each rank runs gaamd_patch_elem1 / _elem2 on its part in HBM.

static void elem1_patch(int fn, int g_a, const Patch &p, const void *alpha, const char *what) {
    GArray &a = arr(g_a);
    need_hbm(a, what);
    check_patch(a, p, what);
    if (fn == GAAMD_ELEM_ADD_CONST && !alpha) fatal("%s: alpha is missing", what);
    comex_barrier(COMEX_GROUP_WORLD);   // fences every pending one-sided operation, then syncs
    const Sub s = own_sub(a, p);
    g_stat.numelem[fn]++;
    int zero = 0;
    if (s.any) {
        zero = launched(gaamd_patch_elem1(a.optype, fn, alpha, s.p, s.stride, s.count, a.ndim, gaamd_stream()), what, true);
        g_stat.mathloc += 2 * s.bytes;
    }
    math_end(what);
    if (fn == GAAMD_ELEM_RECIP) zero_divisor_end(zero, what);
}

// lo == nullptr: the whole array
static void c_elem1(int fn, int g_a, int *lo, int *hi, const void *alpha, const char *what) {
    elem1_patch(fn, g_a, Patch(arr(g_a), lo, hi), alpha, what);
}

static void c_elem2(int fn, int g_a, int *alo, int *ahi, int g_b, int *blo, int *bhi, int g_c, int *clo, int *chi,
                    const char *what) {
    const Patch pa(arr(g_a), alo, ahi), pb(arr(g_b), blo, bhi), pc(arr(g_c), clo, chi);
    binary_patch(g_a, pa, g_b, pb, g_c, pc, g_stat.numelem[fn], "ga_amd elem temporary", fn == GAAMD_ELEM_DIV, what,
                 [&](const GArray &c, const Sub &sa, const Sub &sb, const Sub &sc) {
                     return launched(gaamd_patch_elem2(c.optype, fn, sa.p, sa.stride, sb.p, sb.stride, sc.p, sc.stride,
                                                       sc.count, c.ndim, gaamd_stream()),
                                     what, true);
                 });
}

void GA_Abs_value(int g_a) { c_elem1(GAAMD_ELEM_ABS, g_a, nullptr, nullptr, nullptr, "GA_Abs_value"); }
void GA_Abs_value_patch(int g_a, int *lo, int *hi) {
    c_elem1(GAAMD_ELEM_ABS, g_a, lo, hi, nullptr, "GA_Abs_value_patch");
}
void GA_Add_constant(int g_a, void *alpha) {
    c_elem1(GAAMD_ELEM_ADD_CONST, g_a, nullptr, nullptr, alpha, "GA_Add_constant");
}
void GA_Add_constant_patch(int g_a, int *lo, int *hi, void *alpha) {
    c_elem1(GAAMD_ELEM_ADD_CONST, g_a, lo, hi, alpha, "GA_Add_constant_patch");
}
void GA_Recip(int g_a) { c_elem1(GAAMD_ELEM_RECIP, g_a, nullptr, nullptr, nullptr, "GA_Recip"); }
void GA_Recip_patch(int g_a, int *lo, int *hi) { c_elem1(GAAMD_ELEM_RECIP, g_a, lo, hi, nullptr, "GA_Recip_patch"); }

#define GAAMD_ELEM2(NAME, FN)                                                                              \
    void GA_Elem_##NAME(int g_a, int g_b, int g_c) {                                                       \
        c_elem2(FN, g_a, nullptr, nullptr, g_b, nullptr, nullptr, g_c, nullptr, nullptr, "GA_Elem_" #NAME); \
    }                                                                                                      \
    void GA_Elem_##NAME##_patch(int g_a, int *alo, int *ahi, int g_b, int *blo, int *bhi, int g_c, int *clo, \
                                int *chi) {                                                                \
        c_elem2(FN, g_a, alo, ahi, g_b, blo, bhi, g_c, clo, chi, "GA_Elem_" #NAME "_patch");               \
    }
GAAMD_ELEM2(multiply, GAAMD_ELEM_MUL)
GAAMD_ELEM2(divide, GAAMD_ELEM_DIV)
GAAMD_ELEM2(maximum, GAAMD_ELEM_MAX)
GAAMD_ELEM2(minimum, GAAMD_ELEM_MIN)
#undef GAAMD_ELEM2

// pnga_select_elem (select.c:255-470): each rank with a block selects on it, then the ranks
// agree by gops -- the best key, the lowest row-major linear index among its holders, and
// that element's bits summed as integers (every other rank adds zeros, so -0.0 survives).
// armci_msg_sel_scope would break ties by rank; this rule does not depend on the block map.
void NGA_Select_elem(int g_a, char *op, void *val, int *index) {
    const char *what = "NGA_Select_elem";
    GArray &a = arr(g_a);
    if (!op || (strncmp(op, "min", 3) != 0 && strncmp(op, "max", 3) != 0))
        fatal("%s: operator '%s' not recognized (\"min\" or \"max\")", what, op ? op : "(null)");
    need_hbm(a, what);
    const bool mx = strncmp(op, "max", 3) == 0;
    comex_barrier(COMEX_GROUP_WORLD);
    g_stat.numselect++;
    const Sub s = own_sub(a, Patch(a, nullptr, nullptr));
    int bits[4] = {0, 0, 0, 0};
    union { int i; long l; float f; double d; } key;
    memset(&key, 0, sizeof(key));
    long lin = 0;
    if (s.any) {
        long long li = -1;
        launched(gaamd_patch_select(a.optype, mx ? 1 : 0, s.p, s.stride, s.count, a.ndim, bits, &key, &li, gaamd_stream()),
                 what);
        long mult = 1;
        for (int d = 0; d < a.ndim; d++) {   // block-local, dimension 0 fastest -> whole array
            lin += (s.plo[d] - 1 + (long)(li % s.count[d])) * mult;
            li /= s.count[d];
            mult *= a.dims[d];
        }
        g_stat.mathloc += s.bytes;
    }
    // the best key; a rank without a block contributes the operation's identity
    char opname[4];
    snprintf(opname, sizeof(opname), "%s", mx ? "max" : "min");
    bool holder = s.any;
    gop_by_type(a.type, &key, [&](auto *k, auto gop) {
        typedef std::numeric_limits<std::remove_pointer_t<decltype(k)>> L;   // identity: the type's end, or infinity
        auto best = s.any ? *k : mx ? (L::has_infinity ? -L::infinity() : L::lowest())
                                    : (L::has_infinity ? L::infinity() : L::max());
        gop(&best, 1, opname);
        holder = holder && *k == best;
    });
    char mn[] = "min", plus[] = "+";
    long first = holder ? lin : LONG_MAX;
    armci_msg_lgop(&first, 1, mn);
    if (!(holder && lin == first)) memset(bits, 0, sizeof(bits));
    armci_msg_igop(bits, 4, plus);
    if (first == LONG_MAX) first = 0;   // only NaN keys: unspecified
    memcpy(val, bits, (size_t)a.elemsize);
    for (int d = 0; d < a.ndim; d++) {
        index[a.ndim - 1 - d] = (int)(first % a.dims[d]);
        first /= a.dims[d];
    }
}

// ---- GA_Dgemm / GA_Sgemm / GA_Zgemm / GA_Cgemm / NGA_Matmul_patch -------------------
// pnga_matmul (global/src/matmul.c) gets chunks of A and B to host buffers, multiplies
// them with a host BLAS and accumulates the products into C.  Here every block is in HBM
// and the owner computes: a rank cuts the C patch by its own block and, for every panel of
// kGemmPanel values of k -- counted from the start of the patch's k range, never from a
// block boundary -- gets the rows of op(A) and the columns of op(B) that part needs into
// two HBM scratch buffers (NGA_Get's path: one strided copy kernel per owner, peers read
// through their mappings) and runs gaamd_gemm into its block in place: the caller's beta
// on the first panel, beta = 1 on the later ones.  The panels and the kernel's summation
// order depend on neither the block maps nor the rank count, so neither do the bits of C.
// C_DCPL and C_SCPL arrays (which the reference hands to a host zgemm / cgemm) go the same
// way through gaamd_gemm_cplx, whose beta == (1,0) adds C exactly; for them alone trans may
// be 'C' 'c', the conjugate transpose, its patch stored as for 'T'.
constexpr long kGemmPanel = 1024;

static bool is_trans(char t, const char *what, bool cplx) {
    if (t == 'n' || t == 'N') return false;
    if (t == 't' || t == 'T') return true;
    if (cplx && (t == 'c' || t == 'C')) return true;
    if (cplx) fatal("%s: trans '%c' is not one of N n T t C c", what, t);
    fatal("%s: trans '%c' is not one of N n T t", what, t);
}

static bool patches_meet(const Patch &a, const Patch &b) {
    return a.lo[0] <= b.hi[0] && b.lo[0] <= a.hi[0] && a.lo[1] <= b.hi[1] && b.lo[1] <= a.hi[1];
}

// patches in Fortran order, 1-based: index 0 runs along a stored row (the C column
// subscript), index 1 down the rows.  type: the array type the call is for, 0 = either.
static void matmul_patch(int type, char transa, char transb, const void *alpha, const void *beta, int g_a,
                         const Patch &pa, int g_b, const Patch &pb, int g_c, const Patch &pc, const char *what) {
    GArray &a = arr(g_a), &b = arr(g_b), &c = arr(g_c);
    const bool cplx = c.type == C_DCPL || c.type == C_SCPL;
    const bool ta = is_trans(transa, what, cplx), tb = is_trans(transb, what, cplx);
    if (c.type != C_DBL && c.type != C_FLOAT && !cplx)
        fatal("%s: type %d is none of C_DBL, C_FLOAT, C_DCPL, C_SCPL", what, c.type);
    if (a.type != c.type || b.type != c.type) fatal("%s: types of the arrays differ", what);
    if (type && c.type != type)
        fatal("%s: type mismatch: arrays of type %d in a call for type %d", what, c.type, type);
    if (a.ndim != 2 || b.ndim != 2 || c.ndim != 2) fatal("%s: arrays of rank other than 2 are not supported", what);
    if (!alpha || !beta) fatal("%s: alpha or beta is missing", what);
    const GArray *const abc[3] = {&a, &b, &c};
    const Patch *const pabc[3] = {&pa, &pb, &pc};
    for (int i = 0; i < 3; i++) need_hbm(*abc[i], what);
    for (int i = 0; i < 3; i++) check_patch(*abc[i], *pabc[i], what);
    // op(A) is m x k, op(B) is k x n, C is m x n (matmul.c:1376-1381)
    const long arows = pa.hi[1] - pa.lo[1] + 1, acols = pa.hi[0] - pa.lo[0] + 1;
    const long brows = pb.hi[1] - pb.lo[1] + 1, bcols = pb.hi[0] - pb.lo[0] + 1;
    const long m = ta ? acols : arows, k = ta ? arows : acols, kb = tb ? bcols : brows, n = tb ? brows : bcols;
    if (kb != k || pc.hi[1] - pc.lo[1] + 1 != m || pc.hi[0] - pc.lo[0] + 1 != n)
        fatal("%s: patch extents do not agree: op(A) is %ld x %ld, op(B) %ld x %ld, C %ld x %ld", what, m, k, kb, n,
              pc.hi[1] - pc.lo[1] + 1, pc.hi[0] - pc.lo[0] + 1);
    // every owner writes its part of C while others still read A and B
    if ((g_c == g_a && patches_meet(pc, pa)) || (g_c == g_b && patches_meet(pc, pb)))
        fatal("%s: the C patch overlaps an input patch of the same array", what);
    comex_barrier(COMEX_GROUP_WORLD);
    g_stat.numgemm++;
    const Sub sc = own_sub(c, pc);
    if (sc.any) {
        const long mi = (long)sc.count[1], nj = (long)sc.count[0];       // this rank's rows and columns of C
        const long i0 = sc.plo[1] - pc.lo[1], j0 = sc.plo[0] - pc.lo[0];     // ... from the patch's corner
        const long kmax = std::min(k, kGemmPanel);
        Scratch bufa, bufb;
        bufa.alloc((size_t)mi * kmax * c.elemsize);
        bufb.alloc((size_t)kmax * nj * c.elemsize);
        if (!bufa.p || !bufb.p) fatal("%s: no device memory for the panel buffers", what);
        const double one_d[2] = {1.0, 0.0};   // 1, or (1,0) for the complex types
        const float one_f[2] = {1.0f, 0.0f};
        const void *one = c.type == C_DBL || c.type == C_DCPL ? (const void *)one_d : (const void *)one_f;
        for (long kp = 0; kp < k; kp += kGemmPanel) {
            const long kl = std::min(kGemmPanel, k - kp);
            long lo[2], hi[2], ld[1];
            // rows i0 .. i0 + mi of op(A), columns kp .. kp + kl: stored mi x kl, or kl x mi for 'T'
            lo[0] = pa.lo[0] + (ta ? i0 : kp);
            hi[0] = lo[0] + (ta ? mi : kl) - 1;
            lo[1] = pa.lo[1] + (ta ? kp : i0);
            hi[1] = lo[1] + (ta ? kl : mi) - 1;
            const long lda = ld[0] = hi[0] - lo[0] + 1;
            patch_op(GA_GET, g_a, lo, hi, bufa.p, ld, nullptr);
            // rows kp .. kp + kl of op(B), columns j0 .. j0 + nj: stored kl x nj, or nj x kl for 'T'
            lo[0] = pb.lo[0] + (tb ? kp : j0);
            hi[0] = lo[0] + (tb ? kl : nj) - 1;
            lo[1] = pb.lo[1] + (tb ? j0 : kp);
            hi[1] = lo[1] + (tb ? nj : kl) - 1;
            const long ldb = ld[0] = hi[0] - lo[0] + 1;
            patch_op(GA_GET, g_b, lo, hi, bufb.p, ld, nullptr);
            launched((cplx ? gaamd_gemm_cplx : gaamd_gemm)(c.optype, transa, transb, mi, nj, kl, alpha, bufa.p, lda, bufb.p,
                                                           ldb, kp ? one : beta, sc.p, sc.ext[0], gaamd_stream()),
                     what);
            stream_wait(what);   // the next panel's gets overwrite the buffers
            g_stat.mathloc += (double)c.elemsize * ((double)mi * kl + (double)kl * nj + 2.0 * mi * nj);
        }
    }
    math_end(what);
}

static void c_gemm(int type, char ta, char tb, int m, int n, int k, const void *alpha, int g_a, int g_b,
                   const void *beta, int g_c, const char *what) {
    // the leading corners, as stored: A m x k (k x m for 'T'), B k x n (n x k), C m x n
    const bool cplx = type == C_DCPL || type == C_SCPL;
    const bool tra = is_trans(ta, what, cplx), trb = is_trans(tb, what, cplx);
    const auto corner = [](long cols, long rows) {
        Patch p;
        p.lo[0] = p.lo[1] = 1;
        p.hi[0] = cols;
        p.hi[1] = rows;
        return p;
    };
    matmul_patch(type, ta, tb, alpha, beta, g_a, corner(tra ? m : k, tra ? k : m), g_b, corner(trb ? k : n, trb ? n : k),
                 g_c, corner(n, m), what);
}

void GA_Dgemm(char ta, char tb, int m, int n, int k, double alpha, int g_a, int g_b, double beta, int g_c) {
    c_gemm(C_DBL, ta, tb, m, n, k, &alpha, g_a, g_b, &beta, g_c, "GA_Dgemm");
}
void GA_Sgemm(char ta, char tb, int m, int n, int k, float alpha, int g_a, int g_b, float beta, int g_c) {
    c_gemm(C_FLOAT, ta, tb, m, n, k, &alpha, g_a, g_b, &beta, g_c, "GA_Sgemm");
}
void GA_Zgemm(char ta, char tb, int m, int n, int k, DoubleComplex alpha, int g_a, int g_b, DoubleComplex beta,
              int g_c) {
    c_gemm(C_DCPL, ta, tb, m, n, k, &alpha, g_a, g_b, &beta, g_c, "GA_Zgemm");
}
void GA_Cgemm(char ta, char tb, int m, int n, int k, SingleComplex alpha, int g_a, int g_b, SingleComplex beta,
              int g_c) {
    c_gemm(C_SCPL, ta, tb, m, n, k, &alpha, g_a, g_b, &beta, g_c, "GA_Cgemm");
}
void NGA_Matmul_patch(char transa, char transb, void *alpha, void *beta, int g_a, int alo[], int ahi[], int g_b,
                      int blo[], int bhi[], int g_c, int clo[], int chi[]) {
    const int g[3] = {g_a, g_b, g_c};
    int *lo[3] = {alo, blo, clo}, *hi[3] = {ahi, bhi, chi};
    Patch p[3];
    for (int i = 0; i < 3; i++) {
        if (arr(g[i]).ndim != 2) fatal("NGA_Matmul_patch: arrays of rank other than 2 are not supported");
        p[i] = Patch(arr(g[i]), lo[i], hi[i]);
    }
    matmul_patch(0, transa, transb, alpha, beta, g_a, p[0], g_b, p[1], g_c, p[2], "NGA_Matmul_patch");
}
int gaamd_ga_gemm_panel(void) { return (int)kGemmPanel; }

// ---- a patch of another array as an operand of this rank's kernel ---------------------
// The owner-computes calls below (transposes, matrix.c, pack / unpack, sparse arrays) each need
// a patch of a 1-D or 2-D array that the caller's block map need not agree with.  A Part is
// that patch for one kernel: the rank's own block in place where it holds the whole patch,
// HBM scratch otherwise -- filled through NGA_Get's path for V_READ, stored back through
// NGA_Put's path by part_done for V_WRITE.  Patches are internal (Fortran order, 1-based):
// index 0 runs along a stored row.
enum PartUse { V_NONE, V_READ, V_WRITE };
enum PartPlace { P_AUTO, P_OWN, P_SCRATCH };   // P_AUTO: in place where own_holds() says so

struct Part {
    char *p = nullptr;
    long long ld = 0;   // elements between stored rows (2-D): the block's in place, the patch's width in scratch
    Scratch scratch;
    int g = 0;          // what part_done stores back: the array, the patch and the use
    long lo[2] = {0, 0}, hi[2] = {0, 0};
    PartUse use = V_NONE;
};

// the 0-based inclusive ranges of the sparse code as a patch: index 0 (elements of a vector,
// columns of a matrix), then index 1 (rows of a matrix)
static Patch patch0(long long lo0, long long hi0, long long lo1 = 0, long long hi1 = 0) {
    Patch p;
    p.lo[0] = (long)lo0 + 1;
    p.hi[0] = (long)hi0 + 1;
    p.lo[1] = (long)lo1 + 1;
    p.hi[1] = (long)hi1 + 1;
    return p;
}

// this rank's own block holds the whole patch
static bool own_holds(const GArray &a, const Patch &p) {
    const Sub s = own_sub(a, p);
    if (!s.any) return false;
    for (int d = 0; d < a.ndim; d++)
        if (s.count[d] != p.hi[d] - p.lo[d] + 1) return false;
    return true;
}

// `cap` (1-D): the kernel may touch cap elements from p.lo[0] although only the patch holds data --
// in place only where all of them stay inside the block, else scratch of cap elements.
// `block`: the scratch is a whole block's mirror, and a failed allocation says so.
static Part part(int g, const Patch &p, PartUse use, const char *what, PartPlace place = P_AUTO, long cap = 0,
                 bool block = false) {
    Part r;
    GArray &a = arr(g);
    r.g = g;
    r.use = use;
    for (int d = 0; d < a.ndim; d++) { r.lo[d] = p.lo[d]; r.hi[d] = p.hi[d]; }
    if (place == P_AUTO) {
        Patch room = p;
        if (cap) room.hi[0] = p.lo[0] + cap - 1;
        place = own_holds(a, room) ? P_OWN : P_SCRATCH;
    }
    if (place == P_OWN) {
        const Sub s = own_sub(a, p);
        r.p = s.p;
        r.ld = a.ndim > 1 ? s.ext[0] : 0;
        return r;
    }
    const long long n = cap ? cap : p.hi[0] - p.lo[0] + 1, rows = a.ndim > 1 ? p.hi[1] - p.lo[1] + 1 : 1;
    r.ld = a.ndim > 1 ? n : 0;
    r.p = (char *)r.scratch.alloc((size_t)rows * (size_t)n * a.elemsize);
    if (!r.p) {
        if (a.ndim == 1) fatal("%s: no device memory for %ld elements of scratch", what, (long)n);
        fatal(block ? "%s: no device memory for the %lld x %lld scratch block"
                    : "%s: no device memory for %lld x %lld elements of scratch", what, rows, n);
    }
    const long ld[1] = {(long)r.ld};
    if (use == V_READ) patch_op(GA_GET, g, r.lo, r.hi, r.p, ld, nullptr);
    return r;
}

// the kernel that used the part is waited for; scratch it has written is stored into the array
// and complete at its owner; scratch is freed
static void part_done(Part &r, const char *what) {
    stream_wait(what);
    if (!r.scratch.p) return;
    if (r.use == V_WRITE) {
        const long ld[1] = {(long)r.ld};
        patch_op(GA_PUT, r.g, r.lo, r.hi, r.scratch.p, ld, nullptr);
        comex_fence_all(COMEX_GROUP_WORLD);
    }
    r.scratch.free();
}

// a vector for a computing call: rank 1, `len` elements, of `type`, in HBM.  `of`: the name of the
// dense array whose type that is, null for a sparse array
static void need_vector(int g_v, int type, const char *of, long len, const char *what) {
    const GArray &v = arr(g_v);
    if (v.ndim != 1) fatal("%s: '%s' has rank %d, a vector of rank 1 is needed", what, v.name.c_str(), v.ndim);
    if (v.type != type && of) fatal("%s: types of '%s' and '%s' differ", what, of, v.name.c_str());
    if (v.type != type) fatal("%s: the type of '%s' differs from the sparse array's", what, v.name.c_str());
    if (v.dims[0] != len) fatal("%s: '%s' has %ld elements, %ld are needed", what, v.name.c_str(), v.dims[0], len);
    need_hbm(v, what);
}

// ---- GA_Transpose / GA_Symmetrize ----------------------------------------------------
// pnga_transpose (global.nalg.c:954) transposes a rank's block of A in a host buffer and
// puts it into B; pnga_symmetrize (ga_symmetr.c:49) gets the mirror of a rank's block into
// a host buffer and adds it there.  Here the destination's owner computes, as matmul_patch
// does: a rank takes its own block of the destination -- rows r0..r1, columns c0..c1 as
// stored -- takes the mirror patch of the source (rows c0..c1, columns r0..r1) as a Part, and
// runs the LDS-tiled kernel from it into its block in place.  The block maps of source and
// destination need not agree.

// the mirror of this rank's part `s` of a 2-D array: count[0] rows of count[1]
static Patch mirror_of(const Sub &s) {
    Patch m;
    for (int d = 0; d < 2; d++) { m.lo[d] = s.plo[1 - d]; m.hi[d] = s.phi[1 - d]; }
    return m;
}

void GA_Transpose(int g_a, int g_b) {
    const char *what = "GA_Transpose";
    if (g_a == g_b) fatal("%s: the arrays have to be different", what);
    GArray &a = arr(g_a), &b = arr(g_b);
    if (a.ndim != 2 || b.ndim != 2) fatal("%s: arrays of rank other than 2 are not supported", what);
    if (a.type != b.type) fatal("%s: types of the arrays differ", what);
    if (a.dims[0] != b.dims[1] || a.dims[1] != b.dims[0])
        fatal("%s: dims of the arrays do not agree: A is %ld x %ld, B is %ld x %ld", what, a.dims[1], a.dims[0],
              b.dims[1], b.dims[0]);
    need_hbm(a, what);
    need_hbm(b, what);
    comex_barrier(COMEX_GROUP_WORLD);
    g_stat.numtranspose++;
    const Sub s = own_sub(b, Patch(b, nullptr, nullptr));
    if (s.any) {
        // the block is count[1] rows of count[0]; its mirror in A is count[0] rows of count[1].
        // A mirror that lies wholly in this rank's own block of A is read there, without a get.
        Part src = part(g_a, mirror_of(s), V_READ, what, P_AUTO, 0, true);
        launched(gaamd_transpose(b.optype, s.count[0], s.count[1], src.p, src.ld, s.p, s.ext[0], gaamd_stream()), what);
        part_done(src, what);
        g_stat.mathloc += 2 * s.bytes;
    }
    math_end(what);
}

void GA_Symmetrize(int g_a) {
    const char *what = "GA_Symmetrize";
    GArray &a = arr(g_a);
    if (a.ndim != 2) fatal("%s: arrays of rank other than 2 are not supported", what);
    if (a.dims[0] != a.dims[1]) fatal("%s: the array is not square: %ld x %ld", what, a.dims[1], a.dims[0]);
    if (a.type != C_DBL && a.type != C_FLOAT) fatal("%s: type %d is neither C_DBL nor C_FLOAT", what, a.type);
    need_hbm(a, what);
    comex_barrier(COMEX_GROUP_WORLD);
    g_stat.numsymm++;
    const Sub s = own_sub(a, Patch(a, nullptr, nullptr));
    // always through the scratch copy, on one rank too: in place, a block on the diagonal
    // would read what it is writing
    Part buf;
    if (s.any) buf = part(g_a, mirror_of(s), V_READ, what, P_SCRATCH, 0, true);
    stream_wait(what);
    comex_barrier(COMEX_GROUP_WORLD);   // every rank has read before any rank writes (ga_symmetr.c:105)
    if (s.any) {
        const double half_d = 0.5;
        const float half_f = 0.5f;
        const void *half = a.type == C_DBL ? (const void *)&half_d : (const void *)&half_f;
        launched(gaamd_transpose_acc(a.optype, s.count[1], s.count[0], half, buf.p, buf.ld, s.p, s.ext[0],
                                     gaamd_stream()),
                 what);
        part_done(buf, what);
        g_stat.mathloc += 3 * s.bytes;
    }
    math_end(what);
}

// ---- diagonals, row / column scaling, norms (global/src/matrix.c) ------------------------
// The reference fetches the part of g_v a rank's block needs into a host buffer and loops over
// the block on the host.  Here the owner of g_a computes in HBM, and the elements of g_v its
// block needs are a Part (above).
// Internally (Fortran order) index 0 runs along a stored row: C subscript j is index 0, C
// subscript i is index 1; a block is count[1] rows of count[0] with ext[0] between rows.
static void diagonal_call(int fn, int g_a, int g_v, const void *c, const char *what) {
    GArray &a = arr(g_a);
    if (a.ndim != 2) fatal("%s: arrays of rank other than 2 are not supported", what);
    need_hbm(a, what);
    const PartUse use = fn == GAAMD_DIAG_GET ? V_WRITE : (fn == GAAMD_DIAG_SET || fn == GAAMD_DIAG_ADD) ? V_READ : V_NONE;
    if (use != V_NONE) need_vector(g_v, a.type, a.name.c_str(), std::min(a.dims[0], a.dims[1]), what);
    if (fn == GAAMD_DIAG_SHIFT && !c) fatal("%s: the constant is missing", what);
    comex_barrier(COMEX_GROUP_WORLD);
    g_stat.numdiag++;
    const Sub s = own_sub(a, Patch(a, nullptr, nullptr));
    // rows plo[1]..phi[1], columns plo[0]..phi[0]: the diagonal elements d0..d1 (1-based)
    const long d0 = s.any ? std::max(s.plo[0], s.plo[1]) : 1, d1 = s.any ? std::min(s.phi[0], s.phi[1]) : 0;
    if (d0 <= d1) {
        const long n = d1 - d0 + 1;
        char *p = s.p + ((d0 - s.plo[1]) * s.ext[0] + (d0 - s.plo[0])) * a.elemsize;
        Part v;
        if (use != V_NONE) v = part(g_v, Patch(d0, d1), use, what);
        launched(gaamd_diagonal(a.optype, fn, n, p, (long long)(s.ext[0] + 1) * a.elemsize, v.p, a.elemsize, c,
                                gaamd_stream()),
                 what);
        part_done(v, what);
        g_stat.mathloc += (double)n * a.elemsize * (use == V_NONE && fn == GAAMD_DIAG_ZERO ? 1 : 2);
    }
    math_end(what);
}

static void scale_rc_call(bool rows, int g_a, int g_v, const char *what) {
    GArray &a = arr(g_a);
    if (a.ndim != 2) fatal("%s: arrays of rank other than 2 are not supported", what);
    need_hbm(a, what);
    // C subscript i (rows) is internal index 1, j (columns) internal index 0
    const int dim = rows ? 1 : 0;
    need_vector(g_v, a.type, a.name.c_str(), a.dims[dim], what);
    comex_barrier(COMEX_GROUP_WORLD);
    (rows ? g_stat.numscalerows : g_stat.numscalecols)++;
    const Sub s = own_sub(a, Patch(a, nullptr, nullptr));
    if (s.any) {
        Part v = part(g_v, Patch(s.plo[dim], s.phi[dim]), V_READ, what);
        launched(rows ? gaamd_scale_rows(a.optype, s.count[1], s.count[0], s.p, s.ext[0], v.p, gaamd_stream())
                      : gaamd_scale_cols(a.optype, s.count[1], s.count[0], s.p, s.ext[0], v.p, gaamd_stream()),
                 what);
        part_done(v, what);
        g_stat.mathloc += 2 * s.bytes;
    }
    math_end(what);
}

// pnga_norm1 / pnga_norm_infinity: each rank's norm of its block, then the gop in the element's
// type ("+" / "max"); every rank returns the same bits
static void norm_call(int kind, int g_a, double *nm, const char *what) {
    GArray &a = arr(g_a);
    if (a.ndim != 1 && a.ndim != 2) fatal("%s: arrays of rank other than 1 or 2 are not supported", what);
    if (!nm) fatal("%s: the result is missing", what);
    need_hbm(a, what);
    comex_barrier(COMEX_GROUP_WORLD);
    (kind == GAAMD_NORM_ONE ? g_stat.numnorm1 : g_stat.numnorminf)++;
    const Sub s = own_sub(a, Patch(a, nullptr, nullptr));
    union { int i; long l; float f; double d; } res;
    memset(&res, 0, sizeof(res));   // a rank owning nothing contributes 0
    if (s.any) {
        launched(gaamd_patch_norm(a.optype, kind, s.p, s.stride, s.count, a.ndim, &res, gaamd_stream()), what);
        g_stat.mathloc += s.bytes;
    }
    char opname[4];
    snprintf(opname, sizeof(opname), "%s", kind == GAAMD_NORM_ONE ? "+" : "max");
    gop_by_type(a.type, &res, [&](auto *r, auto gop) {
        gop(r, 1, opname);
        *nm = (double)*r;
    });
    comex_barrier(COMEX_GROUP_WORLD);
}

void GA_Shift_diagonal(int g_a, void *c) { diagonal_call(GAAMD_DIAG_SHIFT, g_a, 0, c, "GA_Shift_diagonal"); }
void GA_Set_diagonal(int g_a, int g_v) { diagonal_call(GAAMD_DIAG_SET, g_a, g_v, nullptr, "GA_Set_diagonal"); }
void GA_Zero_diagonal(int g_a) { diagonal_call(GAAMD_DIAG_ZERO, g_a, 0, nullptr, "GA_Zero_diagonal"); }
void GA_Add_diagonal(int g_a, int g_v) { diagonal_call(GAAMD_DIAG_ADD, g_a, g_v, nullptr, "GA_Add_diagonal"); }
void GA_Get_diag(int g_a, int g_v) { diagonal_call(GAAMD_DIAG_GET, g_a, g_v, nullptr, "GA_Get_diag"); }
void GA_Scale_rows(int g_a, int g_v) { scale_rc_call(true, g_a, g_v, "GA_Scale_rows"); }
void GA_Scale_cols(int g_a, int g_v) { scale_rc_call(false, g_a, g_v, "GA_Scale_cols"); }
void GA_Norm1(int g_a, double *nm) { norm_call(GAAMD_NORM_ONE, g_a, nm, "GA_Norm1"); }
void GA_Norm_infinity(int g_a, double *nm) { norm_call(GAAMD_NORM_INF, g_a, nm, "GA_Norm_infinity"); }

// ---- enumerate, segmented scans, pack / unpack (global/src/sparse.c) ------------------------
// 1-D arrays.  Each rank runs the kernels of ga_amd.h (gaamd_enum, gaamd_scan_tail / gaamd_scan,
// gaamd_mask_count / gaamd_mask_pack / gaamd_mask_unpack) on its part of [lo, hi] where it lies;
// what crosses ranks is one small host exchange per call.  For a 1-D array rank r owns block r,
// so rank order is block order.
static void need_1d(const GArray &a, const char *what) {
    if (a.ndim != 1) fatal("%s: '%s' has rank %d, applicable to 1-dim arrays", what, a.name.c_str(), a.ndim);
    need_hbm(a, what);
}

static void need_range(const GArray &a, long lo, long hi, const char *what) {
    if (lo > hi || lo < 1 || hi > a.dims[0])
        fatal("%s: range [%ld, %ld] outside '%s' of %ld elements", what, lo - 1, hi - 1, a.name.c_str(), a.dims[0]);
}

// one slot of `per` longs per rank in a zeroed array, combined with the integer "+" gop: every
// slot has one writer, so the bits arrive as they were (x + 0), as sparse.c does with lim[]
static void exchange_slots(std::vector<long> &slots) {
    char op[2] = "+";
    armci_msg_lgop(slots.data(), (int)slots.size(), op);
}

// a = a + b in the array's type on the host: complex part by part, integers unsigned
static void host_add(int type, void *a, const void *b) {
    switch (type) {
    case C_INT: { uint32_t x, y; memcpy(&x, a, 4); memcpy(&y, b, 4); x += y; memcpy(a, &x, 4); break; }
    case C_LONG: { uint64_t x, y; memcpy(&x, a, 8); memcpy(&y, b, 8); x += y; memcpy(a, &x, 8); break; }
    case C_FLOAT:
    case C_SCPL: {
        float x[2], y[2];
        const int np = type == C_SCPL ? 2 : 1;
        memcpy(x, a, 4 * np); memcpy(y, b, 4 * np);
        for (int k = 0; k < np; k++) x[k] = x[k] + y[k];
        memcpy(a, x, 4 * np);
        break;
    }
    default: {
        double x[2], y[2];
        const int np = type == C_DCPL ? 2 : 1;
        memcpy(x, a, 8 * np); memcpy(y, b, 8 * np);
        for (int k = 0; k < np; k++) x[k] = x[k] + y[k];
        memcpy(a, x, 8 * np);
        break;
    }
    }
}

static void enum_call(int g_a, long lo, long hi, const void *start, const void *inc) {
    const char *what = "GA_Patch_enum";
    GArray &a = arr(g_a);
    need_1d(a, what);
    need_range(a, lo, hi, what);
    if (!start || !inc) fatal("%s: the start or the increment is missing", what);
    comex_barrier(COMEX_GROUP_WORLD);
    g_stat.numenum++;
    const Sub s = own_sub(a, Patch(lo, hi));
    if (s.any) {
        launched(gaamd_enum(a.optype, s.count[0], s.plo[0] - lo, start, inc, s.p, gaamd_stream()), what);
        g_stat.mathloc += s.bytes;
    }
    math_end(what);
}

static void scan_call(int fn, int g_src, int g_dst, int g_msk, long lo, long hi, const char *what) {
    GArray &src = arr(g_src), &dst = arr(g_dst), &msk = arr(g_msk);
    need_1d(src, what);
    need_1d(dst, what);
    need_1d(msk, what);
    if (g_src == g_dst) fatal("%s: src and dst must be different arrays", what);
    if (src.type != dst.type) fatal("%s: src and dst arrays must be same type", what);
    if (!same_distr(src, msk)) fatal("%s: different distribution src", what);
    if (!same_distr(dst, msk)) fatal("%s: different distribution dst", what);
    need_range(msk, lo, hi, what);
    comex_barrier(COMEX_GROUP_WORLD);
    (fn == GAAMD_SCAN_COPY ? g_stat.numscancopy : g_stat.numscanadd)++;
    const int me = my_rank(), np = world_size();
    const Patch range(lo, hi);
    const Sub ss = own_sub(src, range), sd = own_sub(dst, range), sm = own_sub(msk, range);
    // slot r: {1 rank r has a part of the range | 2 it holds a set element, its tail (16 bytes)}
    std::vector<long> slots((size_t)np * 3, 0);
    if (sm.any) {
        int flag = 0;
        long tail[2] = {0, 0};
        launched(gaamd_scan_tail(src.optype, fn, msk.optype, sm.count[0], ss.p, sm.p, &flag, tail, gaamd_stream()), what);
        slots[(size_t)me * 3] = 1 | (flag ? 2 : 0);
        slots[(size_t)me * 3 + 1] = tail[0];
        slots[(size_t)me * 3 + 2] = tail[1];
    }
    exchange_slots(slots);
    if (sm.any) {
        // the carry: the tail of the nearest rank before this one that holds a set element, plus
        // (ADD) the tails of the ranks between, in ascending order
        int from = me - 1;
        while (from >= 0 && !(slots[(size_t)from * 3] & 2)) from--;
        long carry[2] = {0, 0};
        if (from >= 0) {
            memcpy(carry, &slots[(size_t)from * 3 + 1], 16);
            if (fn != GAAMD_SCAN_COPY)
                for (int r = from + 1; r < me; r++)
                    if (slots[(size_t)r * 3] & 1) host_add(src.type, carry, &slots[(size_t)r * 3 + 1]);
        }
        launched(gaamd_scan(src.optype, fn, msk.optype, sm.count[0], ss.p, sm.p, sd.p, from >= 0 ? 1 : 0, carry,
                            gaamd_stream()),
                 what);
        g_stat.mathloc += 3 * ss.bytes + 2 * sm.bytes;   // src twice and dst, msk twice
    }
    math_end(what);
}

static void pack_call(bool unpack, int g_src, int g_dst, int g_msk, long lo, long hi, int *icount) {
    const char *what = unpack ? "GA_Unpack" : "GA_Pack";
    GArray &src = arr(g_src), &dst = arr(g_dst), &msk = arr(g_msk);
    need_1d(src, what);
    need_1d(dst, what);
    need_1d(msk, what);
    if (g_src == g_dst) fatal("%s: src and dst must be different arrays", what);
    if (src.type != dst.type) fatal("%s: src and dst must be same type", what);
    // `full` lies beside the mask element for element, `thin` is the packed side (any block map)
    const int g_full = unpack ? g_dst : g_src, g_thin = unpack ? g_src : g_dst;
    GArray &full = arr(g_full), &thin = arr(g_thin);
    if (!same_distr(full, msk)) fatal("%s: %s and msk distributions differ", what, unpack ? "dst" : "src");
    need_range(msk, lo, hi, what);
    if (!icount) fatal("%s: icount is missing", what);
    comex_barrier(COMEX_GROUP_WORLD);
    (unpack ? g_stat.numunpack : g_stat.numpack)++;
    const int me = my_rank(), np = world_size();
    const Sub sf = own_sub(full, Patch(lo, hi)), sm = own_sub(msk, Patch(lo, hi));
    std::vector<long> counts((size_t)np, 0);
    if (sm.any) {
        long long c = 0;
        launched(gaamd_mask_count(msk.optype, sm.count[0], sm.p, &c, gaamd_stream()), what);
        counts[(size_t)me] = (long)c;
    }
    exchange_slots(counts);
    long place = 0, total = 0;
    for (int r = 0; r < np; r++) {
        if (r < me) place += counts[(size_t)r];
        total += counts[(size_t)r];
    }
    *icount = (int)total;
    if (total > thin.dims[0])   // every rank knows the total: all end here, nothing was moved
        fatal("%s: %ld set elements do not fit the packed array '%s' of %ld elements", what, total, thin.name.c_str(),
              thin.dims[0]);
    const long cnt = counts[(size_t)me];
    if (cnt > 0) {
        const long n = sm.count[0];
        // the packed side: cnt elements from `place` on.  The kernel judges overlap with it at n
        // elements, so the part has room for n
        Part v = part(g_thin, patch0(place, place + cnt - 1), unpack ? V_READ : V_WRITE, what, P_AUTO, n);
        launched(unpack ? gaamd_mask_unpack(full.optype, msk.optype, n, v.p, sm.p, sf.p, gaamd_stream())
                        : gaamd_mask_pack(full.optype, msk.optype, n, sf.p, sm.p, v.p, gaamd_stream()),
                 what);
        part_done(v, what);
        g_stat.mathloc += 3.0 * sm.bytes + 2.0 * cnt * full.elemsize;   // msk three times, cnt elements in and out
    }
    math_end(what);
}

// capi.c:2261-2373: C subscripts, inclusive
void GA_Patch_enum(int g_a, int lo, int hi, void *start, void *inc) { enum_call(g_a, (long)lo + 1, (long)hi + 1, start, inc); }
void GA_Scan_copy(int g_src, int g_dst, int g_msk, int lo, int hi) {
    scan_call(GAAMD_SCAN_COPY, g_src, g_dst, g_msk, (long)lo + 1, (long)hi + 1, "GA_Scan_copy");
}
void GA_Scan_add(int g_src, int g_dst, int g_msk, int lo, int hi, int excl) {
    scan_call(excl ? GAAMD_SCAN_ADD_EXCL : GAAMD_SCAN_ADD, g_src, g_dst, g_msk, (long)lo + 1, (long)hi + 1, "GA_Scan_add");
}
void GA_Pack(int g_src, int g_dst, int g_msk, int lo, int hi, int *icount) {
    pack_call(false, g_src, g_dst, g_msk, (long)lo + 1, (long)hi + 1, icount);
}
void GA_Unpack(int g_src, int g_dst, int g_msk, int lo, int hi, int *icount) {
    pack_call(true, g_src, g_dst, g_msk, (long)lo + 1, (long)hi + 1, icount);
}

// ---- sparse arrays (global/src/sparse.array.c; ga.h states the contract) -------------------
// A handle names a matrix whose rows are dealt to the ranks by gaamd_sprs::owner.  Until
// NGA_Sprs_array_assemble the elements a rank added wait on its host; assemble moves every
// element to the owner of its row (a table of counts through exchange_slots, then one comex_put
// per owner into a segment of the incoming size), and the owner sorts on the host
// (sprs_build.hpp) and uploads the block CSR into plain HBM allocations once.  The computing
// calls run the kernels of ga_amd.h on that CSR where it lies; the vectors are Parts, as in
// the matrix.c calls.
enum SprsCall { SP_ASSEMBLE, SP_MATVEC, SP_GET_DIAG, SP_SHIFT_DIAG, SP_SCALE, SP_DIAG_LEFT, SP_DIAG_RIGHT };

struct SprsArray {
    bool live = false, assembled = false;
    int type = 0, elemsize = 0, optype = 0;
    long idim = 0, jdim = 0;
    std::vector<gaamd_sprs::Elem> pending;   // added here, not yet assembled
    long long ilo = 0, nrows = 0;            // this rank's rows
    long long nnz = 0, nnz_total = 0;        // entries here, entries on all ranks
    int team = 1;                            // gaamd_spmv_team(nnz_total, idim)
    std::vector<int> blocks;                 // the non-empty column blocks, ascending
    std::vector<long long> start;            // where each begins in jdx / val
    int *offs = nullptr;                     // HBM: [blocks][nrows + 1]
    long long *dstart = nullptr;             // HBM: `start`
    int *jdx = nullptr;                      // HBM: global columns
    char *val = nullptr;                     // HBM: values
};
static std::vector<SprsArray> g_sprs;
static long long g_sprs_routes[4] = {0, 0, 0, 0};   // x in place, x through scratch, y in place, y through scratch

static SprsArray &sprs(int s_a, const char *what) {
    if (s_a < 1 || s_a > (int)g_sprs.size() || !g_sprs[s_a - 1].live)
        fatal("%s: invalid sparse array handle %d", what, s_a);
    return g_sprs[s_a - 1];
}

static SprsArray &sprs_assembled(int s_a, const char *what) {
    SprsArray &s = sprs(s_a, what);
    if (!s.assembled) fatal("%s: the sparse array has not been assembled", what);
    return s;
}

static void *sprs_dev_alloc(size_t bytes, const char *what) {
    void *p = gaamd_dev_malloc(bytes);
    if (!p) fatal("%s: no device memory for %zu bytes", what, bytes);
    return p;
}

static void *sprs_upload(const void *host, size_t bytes, const char *what) {
    void *p = sprs_dev_alloc(bytes, what);
    if (gaamd_memcpy(p, host, bytes) != 0) fatal("%s: copying %zu bytes failed", what, bytes);
    return p;
}

static void sprs_release(SprsArray &s) {
    for (void *p : {(void *)s.offs, (void *)s.dstart, (void *)s.jdx, (void *)s.val})
        if (p) gaamd_dev_free(p);
    s.offs = nullptr;
    s.dstart = nullptr;
    s.jdx = nullptr;
    s.val = nullptr;
}

static void sprs_release_all() {
    for (SprsArray &s : g_sprs) {
        sprs_release(s);
        s = SprsArray();
    }
}

// block b of the CSR: its offsets, and its place in jdx / val
static const int *sprs_offs(const SprsArray &s, size_t b) { return s.offs + b * (size_t)(s.nrows + 1); }
static char *sprs_val(const SprsArray &s, size_t b) { return s.val + s.start[b] * s.elemsize; }

// the columns this rank's entries can name: first column of its first non-empty block to the
// last column of its last one (0-based, inclusive); false when it has no entry
static bool sprs_col_span(const SprsArray &s, long long *lo, long long *hi) {
    if (s.blocks.empty()) return false;
    long long unused;
    gaamd_sprs::range(s.jdim, world_size(), s.blocks.front(), lo, &unused);
    gaamd_sprs::range(s.jdim, world_size(), s.blocks.back(), &unused, hi);
    return true;
}

static void sprs_matvec(int s_a, int g_a, int g_v) {
    const char *what = "NGA_Sprs_array_matvec_multiply";
    SprsArray &s = sprs_assembled(s_a, what);
    need_vector(g_a, s.type, nullptr, s.jdim, what);
    need_vector(g_v, s.type, nullptr, s.idim, what);
    if (g_a == g_v) fatal("%s: the vector and the product must be different arrays", what);
    comex_barrier(COMEX_GROUP_WORLD);
    g_stat.numsprs[SP_MATVEC]++;
    if (s.nrows > 0) {
        long long c0 = 0, c1 = -1;
        Part x;
        if (sprs_col_span(s, &c0, &c1)) {
            x = part(g_a, patch0(c0, c1), V_READ, what);
            g_sprs_routes[x.scratch.p ? 1 : 0]++;
        }
        Part y = part(g_v, patch0(s.ilo, s.ilo + s.nrows - 1), V_WRITE, what);
        g_sprs_routes[y.scratch.p ? 3 : 2]++;
        launched(gaamd_spmv(s.optype, s.nrows, (int)s.blocks.size(), s.offs, s.dstart, s.jdx, s.val, x.p, c0, y.p, s.team,
                            gaamd_stream()),
                 what);
        part_done(x, what);
        part_done(y, what);
        g_stat.mathloc += (double)s.nnz * (2.0 * s.elemsize + 4) + (double)s.nrows * s.elemsize;
    }
    math_end(what);
}

// diag(d) S (left) or S diag(d) (right) on the values in place
static void sprs_diag_multiply(bool left, int s_a, int g_d) {
    const char *what = left ? "NGA_Sprs_array_diag_left_multiply" : "NGA_Sprs_array_diag_right_multiply";
    SprsArray &s = sprs_assembled(s_a, what);
    need_vector(g_d, s.type, nullptr, left ? s.idim : s.jdim, what);
    comex_barrier(COMEX_GROUP_WORLD);
    g_stat.numsprs[left ? SP_DIAG_LEFT : SP_DIAG_RIGHT]++;
    long long lo = s.ilo, hi = s.ilo + s.nrows - 1;
    if (s.nnz > 0 && (left || sprs_col_span(s, &lo, &hi))) {
        Part d = part(g_d, patch0(lo, hi), V_READ, what);
        if (left) {
            for (size_t b = 0; b < s.blocks.size(); b++)
                launched(gaamd_sprs_scale_left(s.optype, s.nrows, sprs_offs(s, b), sprs_val(s, b), d.p, s.team,
                                               gaamd_stream()),
                         what);
        } else {
            launched(gaamd_sprs_scale_right(s.optype, s.nnz, s.jdx, s.val, d.p, lo, gaamd_stream()), what);
        }
        part_done(d, what);
        g_stat.mathloc += (double)s.nnz * (3.0 * s.elemsize + (left ? 0 : 4));
    }
    math_end(what);
}

int NGA_Sprs_array_create(int idim, int jdim, int type) {
    const char *what = "NGA_Sprs_array_create";
    if (idim <= 0 || jdim <= 0) fatal("%s: dimensions %d x %d", what, idim, jdim);
    SprsArray s;
    s.type = type;
    s.elemsize = type_size(type, &s.optype);
    s.idim = idim;
    s.jdim = jdim;
    s.live = true;
    g_sprs.push_back(s);
    return (int)g_sprs.size();
}

void NGA_Sprs_array_add_element(int s_a, int idx, int jdx, void *val) {
    const char *what = "NGA_Sprs_array_add_element";
    SprsArray &s = sprs(s_a, what);
    if (s.assembled) fatal("%s: the sparse array has been assembled already", what);
    if (idx < 0 || idx >= s.idim || jdx < 0 || jdx >= s.jdim)
        fatal("%s: element (%d, %d) outside the %ld x %ld array", what, idx, jdx, s.idim, s.jdim);
    if (!val) fatal("%s: the value is missing", what);
    gaamd_sprs::Elem e;
    memset(&e, 0, sizeof(e));
    e.i = idx;
    e.j = jdx;
    memcpy(e.v, val, (size_t)s.elemsize);
    s.pending.push_back(e);
}

int NGA_Sprs_array_assemble(int s_a) {
    const char *what = "NGA_Sprs_array_assemble";
    SprsArray &s = sprs(s_a, what);
    if (s.assembled) fatal("%s: the sparse array has been assembled already", what);
    const int me = my_rank(), np = world_size();
    typedef gaamd_sprs::Elem Elem;
    // the np x np table of counts: row r holds what rank r sends to every owner
    std::vector<long> table((size_t)np * np, 0);
    for (const Elem &e : s.pending) table[(size_t)me * np + gaamd_sprs::owner(e.i, s.idim, np)]++;
    exchange_slots(table);
    std::vector<long long> total(np, 0);
    s.nnz_total = 0;
    for (int p = 0; p < np; p++) {
        for (int r = 0; r < np; r++) total[p] += table[(size_t)r * np + p];
        s.nnz_total += total[p];
    }
    for (int p = 0; p < np; p++)   // every rank holds the table: all end here
        if (total[p] >= (1ll << 31)) fatal("%s: rank %d would hold %lld entries, 2^31 or more", what, p, total[p]);
    // this rank's elements grouped by owner, insertion order kept
    std::vector<size_t> pos(np, 0);
    for (int p = 1; p < np; p++) pos[p] = pos[p - 1] + (size_t)table[(size_t)me * np + p - 1];
    const std::vector<size_t> first = pos;
    std::vector<Elem> out(s.pending.size());
    for (const Elem &e : s.pending) out[pos[gaamd_sprs::owner(e.i, s.idim, np)]++] = e;
    std::vector<Elem>().swap(s.pending);
    // rank r's elements for owner p go after those of the ranks before r
    std::vector<void *> seg(np, nullptr);
    if (comex_malloc(seg.data(), (size_t)total[me] * sizeof(Elem), COMEX_GROUP_WORLD) != COMEX_SUCCESS)
        fatal("%s: no segment for %lld incoming elements", what, total[me]);
    comex_barrier(COMEX_GROUP_WORLD);
    for (int p = 0; p < np; p++) {
        const size_t n = (size_t)table[(size_t)me * np + p];
        size_t before = 0;
        for (int r = 0; r < me; r++) before += (size_t)table[(size_t)r * np + p];
        const size_t piece = (1u << 30) / sizeof(Elem);   // comex_put counts bytes in an int
        for (size_t k = 0; k < n; k += piece) {
            const size_t c = std::min(piece, n - k);
            if (comex_put(out.data() + first[p] + k, (char *)seg[p] + (before + k) * sizeof(Elem), (int)(c * sizeof(Elem)), p,
                          COMEX_GROUP_WORLD) != COMEX_SUCCESS)
                fatal("%s: sending %zu elements to rank %d failed", what, c, p);
        }
    }
    comex_barrier(COMEX_GROUP_WORLD);   // fences: every element lies at its owner
    std::vector<Elem> in((size_t)total[me]);
    if (!in.empty()) {
        if (gaamd_segment_kind(seg[me]) == 2) memcpy(in.data(), seg[me], in.size() * sizeof(Elem));
        else if (gaamd_memcpy(in.data(), seg[me], in.size() * sizeof(Elem)) != 0) fatal("%s: reading the segment failed", what);
    }
    comex_free(seg[me], COMEX_GROUP_WORLD);
    long long ihi;
    gaamd_sprs::range(s.idim, np, me, &s.ilo, &ihi);
    s.nrows = ihi - s.ilo + 1;
    gaamd_sprs::BlockCsr csr;
    gaamd_sprs::build(in, s.ilo, s.nrows, s.jdim, np, s.elemsize, csr);
    s.nnz = (long long)in.size();
    s.blocks = csr.blocks;
    s.start = csr.start;
    s.team = gaamd_spmv_team(s.nnz_total, s.idim);
    if (s.nnz > 0) {
        s.offs = (int *)sprs_upload(csr.offs.data(), csr.offs.size() * sizeof(int), what);
        s.dstart = (long long *)sprs_upload(csr.start.data(), csr.start.size() * sizeof(long long), what);
        s.jdx = (int *)sprs_upload(csr.jdx.data(), csr.jdx.size() * sizeof(int), what);
        s.val = (char *)sprs_upload(csr.val.data(), csr.val.size(), what);
    }
    s.assembled = true;
    g_stat.numsprs[SP_ASSEMBLE]++;
    comex_barrier(COMEX_GROUP_WORLD);
    return 1;
}

int NGA_Sprs_array_destroy(int s_a) {
    SprsArray &s = sprs(s_a, "NGA_Sprs_array_destroy");
    comex_barrier(COMEX_GROUP_WORLD);
    sprs_release(s);
    s = SprsArray();
    return 1;
}

int NGA_Sprs_array_duplicate(int s_a) {
    const char *what = "NGA_Sprs_array_duplicate";
    (void)sprs(s_a, what);
    comex_barrier(COMEX_GROUP_WORLD);   // no rank is still writing the values
    SprsArray n = sprs(s_a, what);
    if (n.assembled && n.nnz > 0) {
        const size_t bytes[4] = {n.blocks.size() * (size_t)(n.nrows + 1) * sizeof(int), n.blocks.size() * sizeof(long long),
                                 (size_t)n.nnz * sizeof(int), (size_t)n.nnz * (size_t)n.elemsize};
        void *from[4] = {n.offs, n.dstart, n.jdx, n.val}, *to[4];
        for (int k = 0; k < 4; k++) {
            to[k] = sprs_dev_alloc(bytes[k], what);
            if (gaamd_memcpy(to[k], from[k], bytes[k]) != 0) fatal("%s: copying %zu bytes failed", what, bytes[k]);
        }
        n.offs = (int *)to[0];
        n.dstart = (long long *)to[1];
        n.jdx = (int *)to[2];
        n.val = (char *)to[3];
    }
    g_sprs.push_back(n);
    return (int)g_sprs.size();
}

void gaamd_ga_sprs_range(long dim, int nproc, int iproc, long *lo, long *hi) {
    long long l = 0, h = -1;
    if (dim > 0 && nproc > 0 && iproc >= 0 && iproc < nproc) gaamd_sprs::range(dim, nproc, iproc, &l, &h);
    *lo = (long)l;
    *hi = (long)h;
}

void gaamd_ga_sprs_route_counts(long long counts[4]) { memcpy(counts, g_sprs_routes, sizeof(g_sprs_routes)); }

static void sprs_distribution(long dim, int iproc, int *lo, int *hi, const char *what) {
    if (iproc < 0 || iproc >= world_size()) fatal("%s: no rank %d", what, iproc);
    long long l, h;
    gaamd_sprs::range(dim, world_size(), iproc, &l, &h);
    *lo = (int)l;
    *hi = (int)h;
}

void NGA_Sprs_array_row_distribution(int s_a, int iproc, int *lo, int *hi) {
    const char *what = "NGA_Sprs_array_row_distribution";
    sprs_distribution(sprs(s_a, what).idim, iproc, lo, hi, what);
}

void NGA_Sprs_array_column_distribution(int s_a, int iproc, int *lo, int *hi) {
    const char *what = "NGA_Sprs_array_column_distribution";
    sprs_distribution(sprs(s_a, what).jdim, iproc, lo, hi, what);
}

void NGA_Sprs_array_col_block_list(int s_a, int **idx, int *n) {
    const SprsArray &s = sprs_assembled(s_a, "NGA_Sprs_array_col_block_list");
    *n = (int)s.blocks.size();
    *idx = (int *)malloc(std::max<size_t>(1, s.blocks.size()) * sizeof(int));
    std::copy(s.blocks.begin(), s.blocks.end(), *idx);
}

void NGA_Sprs_array_access_col_block(int s_a, int icol, int **idx, int **jdx, void **val) {
    const char *what = "NGA_Sprs_array_access_col_block";
    const SprsArray &s = sprs_assembled(s_a, what);
    if (icol < 0 || icol >= world_size()) fatal("%s: no column block %d", what, icol);
    *idx = nullptr;
    *jdx = nullptr;
    *val = nullptr;
    const auto it = std::lower_bound(s.blocks.begin(), s.blocks.end(), icol);
    if (it == s.blocks.end() || *it != icol) return;
    const size_t b = (size_t)(it - s.blocks.begin());
    *idx = const_cast<int *>(sprs_offs(s, b));
    *jdx = s.jdx + s.start[b];
    *val = sprs_val(s, b);
}

void NGA_Sprs_array_matvec_multiply(int s_a, int g_a, int g_v) { sprs_matvec(s_a, g_a, g_v); }

void NGA_Sprs_array_get_diag(int s_a, int *g_d) {
    const char *what = "NGA_Sprs_array_get_diag";
    if (!g_d) fatal("%s: g_d is missing", what);
    const int me = my_rank(), np = world_size();
    GArray d;   // idim elements on the row cuts; allocate() zeroes it and syncs
    {
        const SprsArray &s = sprs_assembled(s_a, what);
        d.type = s.type;
        d.ndim = 1;
        d.name = "sprs_diag";
        d.elemsize = s.elemsize;
        d.optype = s.optype;
        d.dims[0] = s.idim;
        d.nblock[0] = np;
        for (int p = 0; p < np; p++) {
            long long lo, hi;
            gaamd_sprs::range(s.idim, np, p, &lo, &hi);
            d.map[0].push_back((long)lo + 1);
        }
    }
    comex_barrier(COMEX_GROUP_WORLD);
    *g_d = allocate(d);
    if (*g_d == 0) fatal("%s: no memory for the diagonal", what);
    const SprsArray &s = sprs_assembled(s_a, what);
    g_stat.numsprs[SP_GET_DIAG]++;
    const auto it = std::lower_bound(s.blocks.begin(), s.blocks.end(), me);
    if (s.nrows > 0 && it != s.blocks.end() && *it == me) {   // the rank's own diagonal column block only
        const size_t b = (size_t)(it - s.blocks.begin());
        launched(gaamd_sprs_diag(s.optype, GAAMD_DIAG_GET, s.nrows, sprs_offs(s, b), s.jdx + s.start[b], sprs_val(s, b),
                                 s.ilo, arr(*g_d).ptr[me], nullptr, s.team, gaamd_stream()),
                 what);
        g_stat.mathloc += (double)s.nrows * (s.elemsize + 8);
    }
    math_end(what);
}

void NGA_Sprs_array_shift_diag(int s_a, void *shift) {
    const char *what = "NGA_Sprs_array_shift_diag";
    const SprsArray &s = sprs_assembled(s_a, what);
    if (!shift) fatal("%s: the shift is missing", what);
    comex_barrier(COMEX_GROUP_WORLD);
    g_stat.numsprs[SP_SHIFT_DIAG]++;
    for (size_t b = 0; s.nrows > 0 && b < s.blocks.size(); b++)
        launched(gaamd_sprs_diag(s.optype, GAAMD_DIAG_SHIFT, s.nrows, sprs_offs(s, b), s.jdx + s.start[b], sprs_val(s, b),
                                 s.ilo, nullptr, shift, s.team, gaamd_stream()),
                 what);
    math_end(what);
}

void NGA_Sprs_array_scale(int s_a, void *scale) {
    const char *what = "NGA_Sprs_array_scale";
    const SprsArray &s = sprs_assembled(s_a, what);
    if (!scale) fatal("%s: the factor is missing", what);
    comex_barrier(COMEX_GROUP_WORLD);
    g_stat.numsprs[SP_SCALE]++;
    if (s.nnz > 0) {
        const long long count[1] = {s.nnz};
        launched(gaamd_patch_scale(s.optype, scale, s.val, nullptr, count, 1, gaamd_stream()), what);
        g_stat.mathloc += 2.0 * s.nnz * s.elemsize;
    }
    math_end(what);
}

void NGA_Sprs_array_diag_left_multiply(int s_a, int g_d) { sprs_diag_multiply(true, s_a, g_d); }
void NGA_Sprs_array_diag_right_multiply(int s_a, int g_d) { sprs_diag_multiply(false, s_a, g_d); }

// ---- sparse x dense, dense -> sparse, sparse -> dense (sparse.array.c:3222-3840) ----------------
enum SpmmCall { SM_SPRSDNS, SM_FROM_DENSE, SM_FROM_SPARSE };
static long g_spmm_calls[3] = {0, 0, 0};
static long long g_spmm_routes[4] = {0, 0, 0, 0};   // B in place, B through scratch, C in place, C through scratch
constexpr size_t kSpmmPanelBytes = (size_t)1 << 28;   // the most one scratch side of a panel holds

void gaamd_ga_spmm_route_counts(long long counts[4]) { memcpy(counts, g_spmm_routes, sizeof(g_spmm_routes)); }

// a dense idim x ncols array on the sparse array's row cuts: one block of full rows per rank that
// owns rows (sparse.array.c:3669-3696), so block k lies on rank k; not yet allocated
static GArray sprs_row_array(const SprsArray &s, long ncols, const char *name) {
    GArray d;
    d.type = s.type;
    d.ndim = 2;
    d.name = name;
    d.elemsize = s.elemsize;
    d.optype = s.optype;
    d.dims[0] = ncols;
    d.dims[1] = s.idim;
    d.nblock[0] = 1;
    d.map[0].push_back(1);
    for (int p = 0; p < world_size(); p++) {
        long long lo, hi;
        gaamd_sprs::range(s.idim, world_size(), p, &lo, &hi);
        if (hi >= lo) d.map[1].push_back((long)lo + 1);
    }
    d.nblock[1] = (int)d.map[1].size();
    return d;
}

// this rank's own block of the 2-D array g holds rows [r0, r1] (0-based) at ALL columns: panels of those
// rows are used in place.  Asked once per call, so every panel goes the same way
static bool own_holds_rows(int g, long long r0, long long r1) {
    const GArray &a = arr(g);
    return own_holds(a, patch0(0, a.dims[0] - 1, r0, r1));
}

int NGA_Sprs_array_sprsdns_multiply(int s_a, int g_b) {
    const char *what = "NGA_Sprs_array_sprsdns_multiply";
    SprsArray &s = sprs_assembled(s_a, what);
    long n;
    {
        const GArray &b = arr(g_b);
        if (b.ndim != 2) fatal("%s: '%s' has rank %d, a matrix of rank 2 is needed", what, b.name.c_str(), b.ndim);
        if (b.type != s.type) fatal("%s: the type of '%s' differs from the sparse array's", what, b.name.c_str());
        if (b.dims[1] != s.jdim) fatal("%s: '%s' has %ld rows, %ld are needed", what, b.name.c_str(), b.dims[1], s.jdim);
        need_hbm(b, what);
        n = b.dims[0];
    }
    GArray c = sprs_row_array(s, n, "sprs_dns_product");
    comex_barrier(COMEX_GROUP_WORLD);
    const int g_c = allocate(c);   // zeroes and syncs
    if (g_c == 0) fatal("%s: no memory for the product", what);
    g_spmm_calls[SM_SPRSDNS]++;
    if (s.nrows > 0) {
        const long long r0 = s.ilo, r1 = s.ilo + s.nrows - 1;
        long long c0 = 0, c1 = -1;
        const bool has_b = sprs_col_span(s, &c0, &c1);
        const bool b_own = has_b && own_holds_rows(g_b, c0, c1), c_own = own_holds_rows(g_c, r0, r1);
        if (has_b) g_spmm_routes[b_own ? 0 : 1]++;
        g_spmm_routes[c_own ? 2 : 3]++;
        // panels of columns bound each scratch side by kSpmmPanelBytes (one column at the least)
        long long rows_max = 0;
        if (has_b && !b_own) rows_max = c1 - c0 + 1;
        if (!c_own) rows_max = std::max(rows_max, s.nrows);
        long long pw = n;
        if (rows_max > 0) pw = std::max<long long>(1, std::min<long long>(n, (long long)(kSpmmPanelBytes / s.elemsize) / rows_max));
        for (long long j0 = 0; j0 < n; j0 += pw) {
            const long long j1 = std::min<long long>(n, j0 + pw) - 1;
            Part bp;
            if (has_b) bp = part(g_b, patch0(j0, j1, c0, c1), V_READ, what, b_own ? P_OWN : P_SCRATCH);
            Part cp = part(g_c, patch0(j0, j1, r0, r1), V_WRITE, what, c_own ? P_OWN : P_SCRATCH);
            launched(gaamd_spmm(s.optype, s.nrows, (int)s.blocks.size(), s.offs, s.dstart, s.jdx, s.val, bp.p, bp.ld, c0,
                                j1 - j0 + 1, cp.p, cp.ld, gaamd_stream()),
                     what);
            part_done(cp, what);
            part_done(bp, what);
        }
        g_stat.mathloc += (double)s.nnz * (s.elemsize + 4) + ((double)s.nnz + (double)s.nrows) * (double)n * s.elemsize;
    }
    math_end(what);
    return g_c;
}

int NGA_Sprs_array_create_from_dense(int g_a) {
    const char *what = "NGA_Sprs_array_create_from_dense";
    const int me = my_rank(), np = world_size();
    int type, optype, esz;
    long idim, jdim;
    {
        const GArray &a = arr(g_a);
        if (a.ndim != 2) fatal("%s: '%s' has rank %d, a matrix of rank 2 is needed", what, a.name.c_str(), a.ndim);
        need_hbm(a, what);
        if (a.dims[0] >= (1l << 31) || a.dims[1] >= (1l << 31)) fatal("%s: a dimension of 2^31 or more", what);
        type = a.type;
        optype = a.optype;
        esz = a.elemsize;
        idim = a.dims[1];
        jdim = a.dims[0];
    }
    comex_barrier(COMEX_GROUP_WORLD);   // no rank is still writing g_a
    g_spmm_calls[SM_FROM_DENSE]++;
    const Sub sa = own_sub(arr(g_a), Patch(arr(g_a), nullptr, nullptr));
    const long long rows = sa.any ? sa.count[1] : 0, cols = sa.any ? sa.count[0] : 0;
    std::vector<int> offs((size_t)rows + 1, 0);
    Scratch d_offs;
    long long kept = 0;
    if (rows > 0) {
        if (!d_offs.alloc(offs.size() * sizeof(int))) fatal("%s: no device memory for %lld row counts", what, rows);
        launched(gaamd_dense_row_counts(optype, rows, cols, sa.p, sa.ext[0], sa.plo[1] - 1, sa.plo[0] - 1, (int *)d_offs.p,
                                        gaamd_stream()),
                 what);
        stream_wait(what);
        if (gaamd_memcpy(offs.data() + 1, d_offs.p, (size_t)rows * sizeof(int)) != 0) fatal("%s: reading the counts failed", what);
        for (long long r = 0; r < rows; r++) {   // the exclusive prefix sums, in 64 bits
            const long long c = offs[(size_t)r + 1];
            offs[(size_t)r] = (int)std::min<long long>(kept, INT32_MAX);
            kept += c;
        }
        offs[(size_t)rows] = (int)std::min<long long>(kept, INT32_MAX);
        g_stat.mathloc += sa.bytes;
    }
    std::vector<long> totals((size_t)np, 0);
    totals[(size_t)me] = (long)kept;
    exchange_slots(totals);
    for (int p = 0; p < np; p++)   // every rank holds the totals: all end here, before any is stored
        if (totals[(size_t)p] >= (1l << 31)) fatal("%s: rank %d would keep %ld entries, 2^31 or more", what, p, totals[(size_t)p]);
    const int s_new = NGA_Sprs_array_create((int)idim, (int)jdim, type);
    if (kept > 0) {
        Scratch d_jdx, d_val;
        if (!d_jdx.alloc((size_t)kept * sizeof(int)) || !d_val.alloc((size_t)kept * (size_t)esz))
            fatal("%s: no device memory for %lld kept elements", what, kept);
        if (gaamd_memcpy(d_offs.p, offs.data(), offs.size() * sizeof(int)) != 0) fatal("%s: copying the offsets failed", what);
        launched(gaamd_dense_to_csr(optype, rows, cols, sa.p, sa.ext[0], sa.plo[1] - 1, sa.plo[0] - 1, (const int *)d_offs.p,
                                    (int *)d_jdx.p, d_val.p, gaamd_stream()),
                 what);
        stream_wait(what);
        std::vector<int> jdx((size_t)kept);
        std::vector<unsigned char> val((size_t)kept * (size_t)esz);
        if (gaamd_memcpy(jdx.data(), d_jdx.p, jdx.size() * sizeof(int)) != 0 || gaamd_memcpy(val.data(), d_val.p, val.size()) != 0)
            fatal("%s: reading the kept elements failed", what);
        g_stat.mathloc += sa.bytes + (double)kept * (esz + 4);
        std::vector<gaamd_sprs::Elem> &pending = g_sprs[(size_t)s_new - 1].pending;
        pending.resize((size_t)kept);
        for (long long r = 0; r < rows; r++)
            for (int k = offs[(size_t)r]; k < offs[(size_t)r + 1]; k++) {
                gaamd_sprs::Elem &e = pending[(size_t)k];
                memset(&e, 0, sizeof(e));
                e.i = (int32_t)(sa.plo[1] - 1 + r);
                e.j = jdx[(size_t)k];
                memcpy(e.v, val.data() + (size_t)k * (size_t)esz, (size_t)esz);
            }
    }
    NGA_Sprs_array_assemble(s_new);   // syncs; counted as an assemble too
    return s_new;
}

int NGA_Sprs_array_create_from_sparse(int s_a) {
    const char *what = "NGA_Sprs_array_create_from_sparse";
    SprsArray &s = sprs_assembled(s_a, what);
    GArray d = sprs_row_array(s, s.jdim, "sprs_dense");
    comex_barrier(COMEX_GROUP_WORLD);
    const int g_d = allocate(d);   // zeroes and syncs
    if (g_d == 0) fatal("%s: no memory for the dense array", what);
    g_spmm_calls[SM_FROM_SPARSE]++;
    if (s.nrows > 0 && s.nnz > 0) {
        const long long r0 = s.ilo, r1 = s.ilo + s.nrows - 1;
        const bool own = own_holds_rows(g_d, r0, r1);
        // rows that lie in another rank's block: full-width panels of rows, zeroed, scattered and put
        const long long rows_max = own ? s.nrows : std::max<long long>(1, (long long)(kSpmmPanelBytes / s.elemsize) / s.jdim);
        for (long long q0 = 0; q0 < s.nrows; q0 += rows_max) {
            const long long q1 = std::min<long long>(s.nrows, q0 + rows_max) - 1;
            Part out = part(g_d, patch0(0, s.jdim - 1, r0 + q0, r0 + q1), V_WRITE, what, own ? P_OWN : P_SCRATCH);
            if (!own && gaamd_memset(out.p, 0, (size_t)(q1 - q0 + 1) * (size_t)s.jdim * s.elemsize) != 0)
                fatal("%s: zeroing the scratch failed", what);
            for (size_t b = 0; b < s.blocks.size(); b++)
                launched(gaamd_csr_to_dense(s.optype, q1 - q0 + 1, s.jdim, sprs_offs(s, b) + q0, s.jdx + s.start[b],
                                            sprs_val(s, b), 0, out.p, out.ld, gaamd_stream()),
                         what);
            part_done(out, what);
        }
        g_stat.mathloc += (double)s.nnz * (2.0 * s.elemsize + 4);
    }
    math_end(what);
    return g_d;
}

// ---- sparse x sparse (sparse.array.c:2424-3103) ---------------------------------------------------
// Rank l's row block of B is A's column block l: the cut rule is the same and B.idim == A.jdim.  Every
// rank flattens its B into a row CSR (gaamd_csr_rows) inside a comex_malloc segment that lives for the
// length of the call; a rank reads the parts its non-empty column blocks of A name with comex_get into
// HBM scratch and runs gaamd_spgemm_count / _fill on its own rows.  No global array is created.
static long g_spgemm_calls = 0;
static long long g_spgemm_routes[2] = {0, 0};   // B parts used in place, B parts copied

void gaamd_ga_spgemm_route_counts(long long counts[2]) { memcpy(counts, g_spgemm_routes, sizeof(g_spgemm_routes)); }

// where rank p's part of B lies in its segment: (rows + 1) offsets, then jdx, then val from a 16-byte boundary
struct SpgPart {
    long long rows = 0, nnz = 0;
    size_t jdx_at = 0, val_at = 0, bytes = 0;
    SpgPart() {}
    SpgPart(long long rows_, long long nnz_, int esz) : rows(rows_), nnz(nnz_) {
        if (nnz == 0) return;   // nothing is published
        jdx_at = (size_t)(rows + 1) * sizeof(long long);
        val_at = (jdx_at + (size_t)nnz * sizeof(int) + 15) & ~(size_t)15;
        bytes = val_at + (size_t)nnz * (size_t)esz;
    }
};

// comex_get counts bytes in an int; the rank's own part is a local copy out of its segment
static void spg_fetch(void *remote, void *local, size_t bytes, int proc, const char *what) {
    if (proc == my_rank()) {
        if (bytes && gaamd_memcpy(local, remote, bytes) != 0) fatal("%s: copying %zu bytes of this rank's part of B failed", what, bytes);
        return;
    }
    const size_t piece = (size_t)1 << 30;
    for (size_t k = 0; k < bytes; k += piece)
        if (comex_get((char *)remote + k, (char *)local + k, (int)std::min(piece, bytes - k), proc, COMEX_GROUP_WORLD) !=
            COMEX_SUCCESS)
            fatal("%s: reading %zu bytes of rank %d's part of B failed", what, bytes, proc);
}

int NGA_Sprs_array_matmat_multiply(int s_a, int s_b) {
    const char *what = "NGA_Sprs_array_matmat_multiply";
    const int me = my_rank(), np = world_size();
    SprsArray c;
    {
        const SprsArray &a = sprs_assembled(s_a, what), &b = sprs_assembled(s_b, what);
        if (a.type != b.type) fatal("%s: the types of the two sparse arrays differ", what);
        if (a.jdim != b.idim) fatal("%s: A has %ld columns, B has %ld rows", what, a.jdim, b.idim);
        c.type = a.type;
        c.elemsize = a.elemsize;
        c.optype = a.optype;
        c.idim = a.idim;
        c.jdim = b.jdim;
        c.ilo = a.ilo;
        c.nrows = a.nrows;
    }
    const int esz = c.elemsize;
    comex_barrier(COMEX_GROUP_WORLD);
    g_spgemm_calls++;
    // what every rank publishes
    std::vector<long> nnzs((size_t)np, 0);
    nnzs[(size_t)me] = (long)g_sprs[(size_t)s_b - 1].nnz;
    exchange_slots(nnzs);
    std::vector<SpgPart> parts((size_t)np);
    std::vector<long long> row0((size_t)np + 1, 0);   // the first row of B of every rank
    for (int p = 0; p < np; p++) {
        long long lo, hi;
        gaamd_sprs::range(g_sprs[(size_t)s_b - 1].idim, np, p, &lo, &hi);
        row0[(size_t)p] = lo;
        parts[(size_t)p] = SpgPart(hi - lo + 1, nnzs[(size_t)p], esz);
    }
    row0[(size_t)np] = g_sprs[(size_t)s_b - 1].idim;
    std::vector<void *> seg((size_t)np, nullptr);
    if (comex_malloc(seg.data(), parts[(size_t)me].bytes, COMEX_GROUP_WORLD) != COMEX_SUCCESS)
        fatal("%s: no segment for %zu bytes of B", what, parts[(size_t)me].bytes);
    const SpgPart &mine = parts[(size_t)me];
    if (mine.bytes) {
        const SprsArray &b = g_sprs[(size_t)s_b - 1];
        if (gaamd_segment_kind(seg[(size_t)me]) == 2)
            fatal("%s: segments live on the host (COMEX_AMD_SEGMENT=host); not supported", what);
        char *sp = (char *)seg[(size_t)me];
        launched(gaamd_csr_rows(b.optype, b.nrows, (int)b.blocks.size(), b.offs, b.dstart, b.jdx, b.val, (long long *)sp,
                                (int *)(sp + mine.jdx_at), sp + mine.val_at, gaamd_stream()),
                 what);
        stream_wait(what);
        g_stat.mathloc += 2.0 * (double)b.nnz * (esz + 4);
    }
    comex_barrier(COMEX_GROUP_WORLD);   // every part is published

    const SprsArray a = g_sprs[(size_t)s_a - 1];   // the pointers are A's still: nothing is released here
    std::vector<int> counts;   // [np][nrows]
    Scratch g_offs, g_jdx, g_val, d_coffs, d_cstart;
    const long long *roffs = nullptr;
    const int *rjdx = nullptr;
    const char *rval = nullptr;
    long long b_first = 0, brows = 0;
    if (a.nrows > 0 && !a.blocks.empty()) {
        const int l0 = a.blocks.front(), l1 = a.blocks.back();
        b_first = row0[(size_t)l0];
        brows = (l1 + 1 < np ? row0[(size_t)l1 + 1] : row0[(size_t)np]) - b_first;
        if (l0 == me && l1 == me && mine.bytes) {   // its own part alone: in place
            const char *sp = (const char *)seg[(size_t)me];
            roffs = (const long long *)sp;
            rjdx = (const int *)(sp + mine.jdx_at);
            rval = sp + mine.val_at;
            g_spgemm_routes[0]++;
        } else {   // one row CSR over the span; the blocks A does not name, and the parts without entries, give empty rows
            long long total = 0;
            for (int l : a.blocks) total += parts[(size_t)l].nnz;
            std::vector<long long> offs((size_t)brows + 1, 0);
            if (!g_offs.alloc(offs.size() * sizeof(long long)) || !g_jdx.alloc(std::max<size_t>(16, (size_t)total * sizeof(int))) ||
                !g_val.alloc(std::max<size_t>(16, (size_t)total * (size_t)esz)))
                fatal("%s: no device memory for %lld gathered entries of B", what, total);
            long long at = 0;
            size_t r = 0;
            for (int l = l0; l <= l1; l++) {
                const SpgPart &p = parts[(size_t)l];
                const bool named = std::binary_search(a.blocks.begin(), a.blocks.end(), l) && p.nnz > 0;
                if (named) {
                    std::vector<long long> theirs((size_t)p.rows + 1);
                    spg_fetch(seg[(size_t)l], theirs.data(), theirs.size() * sizeof(long long), l, what);
                    for (long long q = 0; q < p.rows; q++) offs[r + (size_t)q] = at + theirs[(size_t)q];
                    spg_fetch((char *)seg[(size_t)l] + p.jdx_at, (int *)g_jdx.p + at, (size_t)p.nnz * sizeof(int), l, what);
                    spg_fetch((char *)seg[(size_t)l] + p.val_at, (char *)g_val.p + at * esz, (size_t)p.nnz * (size_t)esz, l, what);
                    at += p.nnz;
                    g_spgemm_routes[1]++;
                } else {
                    for (long long q = 0; q < p.rows; q++) offs[r + (size_t)q] = at;
                }
                r += (size_t)p.rows;
            }
            offs[(size_t)brows] = at;
            if (gaamd_memcpy(g_offs.p, offs.data(), offs.size() * sizeof(long long)) != 0) fatal("%s: copying the offsets failed", what);
            roffs = (const long long *)g_offs.p;
            rjdx = (const int *)g_jdx.p;
            rval = (const char *)g_val.p;
            g_stat.mathloc += (double)total * (esz + 4);
        }
        // the counting phase
        Scratch d_counts, d_bound;
        counts.resize((size_t)np * (size_t)a.nrows);
        if (!d_counts.alloc(counts.size() * sizeof(int)) || !d_bound.alloc((size_t)a.nrows * sizeof(long long)))
            fatal("%s: no device memory for the counts of %lld rows", what, a.nrows);
        launched(gaamd_spgemm_count(a.nrows, (int)a.blocks.size(), a.offs, a.dstart, a.jdx, b_first, brows, roffs, rjdx, c.jdim,
                                    np, (int *)d_counts.p, (long long *)d_bound.p, gaamd_stream()),
                 what);
        stream_wait(what);
        if (gaamd_memcpy(counts.data(), d_counts.p, counts.size() * sizeof(int)) != 0) fatal("%s: reading the counts failed", what);
    }
    // per block: the offsets of the rows and the total; the 2^31 check on the table of all ranks
    std::vector<int> coffs((size_t)np * (size_t)(c.nrows + 1), 0);
    std::vector<long long> cstart((size_t)np, 0);
    long long held = 0;
    for (int b = 0; b < np; b++) {
        cstart[(size_t)b] = held;
        long long run = 0;
        int *o = coffs.data() + (size_t)b * (size_t)(c.nrows + 1);
        for (long long r = 0; r < c.nrows; r++) {
            o[r] = (int)std::min<long long>(run, INT32_MAX);
            if (!counts.empty()) run += counts[(size_t)b * (size_t)c.nrows + (size_t)r];
        }
        o[c.nrows] = (int)std::min<long long>(run, INT32_MAX);
        held += run;
    }
    std::vector<long> totals((size_t)np, 0);
    totals[(size_t)me] = (long)held;
    exchange_slots(totals);
    for (int p = 0; p < np; p++) {   // every rank holds the totals: all end here, before anything is stored
        if (totals[(size_t)p] >= (1l << 31)) fatal("%s: rank %d would hold %ld entries, 2^31 or more", what, p, totals[(size_t)p]);
        c.nnz_total += totals[(size_t)p];
    }
    c.nnz = held;
    c.team = gaamd_spmv_team(c.nnz_total, c.idim);
    if (held > 0) {
        c.jdx = (int *)sprs_dev_alloc((size_t)held * sizeof(int), what);
        c.val = (char *)sprs_dev_alloc((size_t)held * (size_t)esz, what);
        if (!d_coffs.alloc(coffs.size() * sizeof(int)) || !d_cstart.alloc(cstart.size() * sizeof(long long)))
            fatal("%s: no device memory for the offsets of %lld rows", what, c.nrows);
        if (gaamd_memcpy(d_coffs.p, coffs.data(), coffs.size() * sizeof(int)) != 0 ||
            gaamd_memcpy(d_cstart.p, cstart.data(), cstart.size() * sizeof(long long)) != 0)
            fatal("%s: copying the offsets failed", what);
        launched(gaamd_spgemm_fill(a.optype, a.nrows, (int)a.blocks.size(), a.offs, a.dstart, a.jdx, a.val, b_first, brows, roffs,
                                   rjdx, rval, c.jdim, np, (const int *)d_coffs.p, (const long long *)d_cstart.p, c.jdx, c.val,
                                   gaamd_stream()),
                 what);
        // the empty blocks are dropped: what stays is assemble's layout
        std::vector<int> offs;
        for (int b = 0; b < np; b++) {
            const int *o = coffs.data() + (size_t)b * (size_t)(c.nrows + 1);
            if (o[c.nrows] == 0) continue;
            c.blocks.push_back(b);
            c.start.push_back(cstart[(size_t)b]);
            offs.insert(offs.end(), o, o + c.nrows + 1);
        }
        c.offs = (int *)sprs_upload(offs.data(), offs.size() * sizeof(int), what);
        c.dstart = (long long *)sprs_upload(c.start.data(), c.start.size() * sizeof(long long), what);
        g_stat.mathloc += (double)held * (esz + 4) + (double)a.nnz * (esz + 4);
    }
    c.live = true;
    c.assembled = true;
    math_end(what);   // every rank is done reading the parts
    comex_free(seg[(size_t)me], COMEX_GROUP_WORLD);
    g_sprs.push_back(c);
    return (int)g_sprs.size();
}

void GA_Print_stats(void) {
    printf("[%d] GA on-device calls: fill %ld, scale %ld, add %ld, copy %ld, dot %ld; local bytes moved %.0f; "
           "gemm %ld\n",
           my_rank(), g_stat.numfill, g_stat.numscale, g_stat.numadd, g_stat.numcopy, g_stat.numdot,
           g_stat.mathloc, g_stat.numgemm);
    printf("[%d] GA statistics: acc calls %ld, put calls %ld, get calls %ld, scatter calls %ld, gather calls %ld\n",
           my_rank(), g_stat.numacc, g_stat.numput, g_stat.numget, g_stat.numsca, g_stat.numgat);
    printf("[%d] accumulate bytes total %.0f, local %.0f (%.1f%%)\n", my_rank(), g_stat.acctot, g_stat.accloc,
           g_stat.acctot > 0 ? 100.0 * g_stat.accloc / g_stat.acctot : 0.0);
    printf("[%d] GA transposes: transpose %ld, symmetrize %ld\n", my_rank(), g_stat.numtranspose, g_stat.numsymm);
    printf("[%d] GA element-wise calls: abs %ld, add_constant %ld, recip %ld, multiply %ld, divide %ld, maximum %ld, "
           "minimum %ld; select %ld\n",
           my_rank(), g_stat.numelem[GAAMD_ELEM_ABS], g_stat.numelem[GAAMD_ELEM_ADD_CONST],
           g_stat.numelem[GAAMD_ELEM_RECIP], g_stat.numelem[GAAMD_ELEM_MUL], g_stat.numelem[GAAMD_ELEM_DIV],
           g_stat.numelem[GAAMD_ELEM_MAX], g_stat.numelem[GAAMD_ELEM_MIN], g_stat.numselect);
    printf("[%d] GA matrix calls: diagonal %ld, scale_rows %ld, scale_cols %ld, norm1 %ld, norm_infinity %ld\n",
           my_rank(), g_stat.numdiag, g_stat.numscalerows, g_stat.numscalecols, g_stat.numnorm1, g_stat.numnorminf);
    printf("[%d] GA sparse calls: enum %ld, scan_copy %ld, scan_add %ld, pack %ld, unpack %ld\n", my_rank(),
           g_stat.numenum, g_stat.numscancopy, g_stat.numscanadd, g_stat.numpack, g_stat.numunpack);
    printf("[%d] GA sparse-array calls: assemble %ld, matvec %ld, get_diag %ld, shift_diag %ld, scale %ld, diag_left %ld, "
           "diag_right %ld\n",
           my_rank(), g_stat.numsprs[SP_ASSEMBLE], g_stat.numsprs[SP_MATVEC], g_stat.numsprs[SP_GET_DIAG],
           g_stat.numsprs[SP_SHIFT_DIAG], g_stat.numsprs[SP_SCALE], g_stat.numsprs[SP_DIAG_LEFT],
           g_stat.numsprs[SP_DIAG_RIGHT]);
    printf("[%d] GA sparse-product calls: sprsdns %ld, from_dense %ld, from_sparse %ld\n", my_rank(),
           g_spmm_calls[SM_SPRSDNS], g_spmm_calls[SM_FROM_DENSE], g_spmm_calls[SM_FROM_SPARSE]);
    if (g_spgemm_calls > 0) printf("[%d] GA sparse-sparse calls: matmat %ld\n", my_rank(), g_spgemm_calls);
}

}  // extern "C"
