/*
 * ga_amd.h -- framework-level C ABI of libga_amd.so beyond comex.h/armci.h.
 *
 *  1. Bootstrap hooks.  The reference exchanges segment registrations and
 *     semaphore names with MPI_Allgather (comex/src-mpi-pr/comex.c:2461, 2874)
 *     and synchronises with MPI_Barrier (comex.c:1231).  Here the host program
 *     may hand in its own allgather/barrier (torch.distributed, MPI, ...);
 *     without hooks comex_init() uses RANK/WORLD_SIZE/LOCAL_RANK (or the
 *     OMPI_/PMI_ equivalents) and a node-local shared-memory rendezvous.
 *  2. Kernel-level entry points: the gfx950 kernels that comex_accs/puts/gets
 *     enqueue, callable directly on device pointers with an explicit stream.
 *     They replace, element for element:
 *       gaamd_strided(op=COMEX_ACC_*) : nb_accs per-row _acc  comex.c:6890-6962,
 *                                       acc.h:106-154
 *       gaamd_strided(op=GAAMD_OP_COPY): nb_puts/nb_gets       comex.c:6342-6427, 6617-6696
 *       gaamd_pack                     : pack                   comex.c:1267-1328
 *       gaamd_unpack                   : unpack                 comex.c:1331-1384
 *       gaamd_unpack_acc               : _acc_packed_handler    comex.c:4238-4268
 *  3. Device plumbing used by tests and bench.py (allocation, copies,
 *     synthetic inputs, HIP-event timing, tuning knobs).
 *
 * All functions return 0 on success and a negative code on failure unless
 * stated otherwise; `stream` arguments are hipStream_t passed as void*
 * (NULL = the library's own stream).
 */
#ifndef GA_AMD_H
#define GA_AMD_H

#include <stddef.h>

#if defined(__cplusplus)
extern "C" {
#endif

#define GAAMD_OP_COPY 0

/* ---- 1. bootstrap ------------------------------------------------------ */
typedef int (*gaamd_allgather_fn)(const void *send, void *recv, size_t bytes, void *ctx);
typedef int (*gaamd_barrier_fn)(void *ctx);
int gaamd_set_bootstrap(int rank, int size, int local_rank,
                        gaamd_allgather_fn allgather, gaamd_barrier_fn barrier, void *ctx);
#ifdef MPI_VERSION
/* hooks over an MPI communicator (the bootstrap half of comex_init_comm, no GPU) */
int gaamd_set_bootstrap_comm(MPI_Comm comm);
#endif
/* exercise the bootstrap alone (no GPU): allgather of ranks + barriers */
int gaamd_bootstrap_selftest(int rounds);
int gaamd_rank(void);
int gaamd_size(void);
/* HIP device of this rank after comex_init (COMEX_AMD_DEVICE or local rank mod devices) */
int gaamd_device(void);
/* after comex_init: ranks (this one included) whose HIP device is this rank's physical
   GPU (PCI bus id), distinct GPUs among the ranks of this node, and the peer-load mode
   (COMEX_AMD_PEER_LOADS: 0 auto -- peers on other GPUs read with system-scope loads,
   1 all -- every peer treated as another GPU, 2 off).  Lets a caller say whether its
   remote traffic crossed xGMI. */
int gaamd_device_topology(int *ranks_on_gpu, int *gpus_on_node, int *peer_loads);
/* nodes: ranks sharing a host (or the same COMEX_AMD_NODE value) map each other's
   HBM; ranks on different nodes exchange the MPI-PR messages over TCP (wire.cpp).
   After bootstrap: this rank's node index, the node count, ranks on this node. */
int gaamd_node_info(int *node, int *nnodes, int *node_size);
/* exercise the cross-node transport alone (no GPU): PING frames between all ranks */
int gaamd_wire_selftest(int rounds);

/* ---- 2. kernels -------------------------------------------------------- */
int gaamd_strided(int op, const void *scale, const void *src, const int *src_stride,
                  void *dst, const int *dst_stride, const int *count, int stride_levels,
                  void *stream);
/* Computing on a patch where it lies (HBM): the loops of global/src/global.npatch.c
 * (fill 1528-1650, scale 1953-1986, add 2520-2546, dot 938-1095), expression for
 * expression, no FMA, integers in unsigned arithmetic.
 * element type by COMEX_ACC_* code; count[] in ELEMENTS per dimension (dim 0 contiguous),
 * *_stride[j] = byte stride of dimension j+1, ndim 1..7, all 64-bit.
 * Negative codes, nothing launched: -2 ndim outside 1..7, -3 a negative count, -4 an
 * unknown op, -5 a missing scalar or result, -6 missing strides, -7 2^31 rows or more
 * after merging, -8 a base or stride below 4-byte alignment, -11 (add) c overlaps a or b
 * without being exactly it (same base, same strides).  A count of zero: 0, no launch.
 * gaamd_patch_dot synchronises its stream and writes one element to `result` (host
 * memory); the same input gives the same bits on every run. */
int gaamd_patch_fill (int op, const void *value, void *dst, const long long *dst_stride,
                      const long long *count, int ndim, void *stream);
int gaamd_patch_scale(int op, const void *alpha, void *dst, const long long *dst_stride,
                      const long long *count, int ndim, void *stream);
int gaamd_patch_add  (int op, const void *alpha, const void *a, const long long *a_stride,
                      const void *beta,  const void *b, const long long *b_stride,
                      void *c, const long long *c_stride, const long long *count, int ndim, void *stream);
int gaamd_patch_dot  (int op, const void *a, const long long *a_stride, const void *b,
                      const long long *b_stride, const long long *count, int ndim,
                      void *result /* host, one element of the type */, void *stream);
/* gaamd_patch_add's checks without a launch (no GPU needed): 0 it would launch, 1 nothing
 * to do, or its error code; plan[0..3] = {vector width, row levels after merging, rows,
 * vectors per row} */
int gaamd_patch_add_plan(int op, const void *a, const long long *a_stride, const void *b,
                         const long long *b_stride, const void *c, const long long *c_stride,
                         const long long *count, int ndim, long long plan[4]);
/* Element-wise algebra on a patch where it lies: the loops of global/src/elem_alg.c (GA_ABS /
 * GA_MAX / GA_MIN of globalp.h:55-57), expression for expression, no FMA, on gaamd_patch_add's
 * map kernel.  Geometry, checks and negative codes are those of gaamd_patch_scale (elem1, in
 * place on dst) and gaamd_patch_add (elem2, c = fn(a, b); c may be exactly a and/or b, any other
 * overlap is -11); an unknown fn is -4, a missing scalar for ADD_CONST -5; a count of zero: 0,
 * no launch.  All six types; integer sums and products in unsigned (wraparound) arithmetic.
 *   ABS        x >= 0 ? x : -x (not fabs: -0.0 stays -0.0, INT_MIN / LONG_MIN wrap to
 *              themselves).  Complex: the reference's portable branch (do_abs without
 *              HAVE_HYPOT, 270-288 / 297-315), the larger part times sqrt(1 + ratio^2), imag = 0
 *              -- NOT hypot: the host's and the device's hypot are different functions, only
 *              this branch has the same bits everywhere.  C_SCPL as C evaluates it: ratio and
 *              1 + ratio^2 in float, sqrt and the product in double, one rounding on the store.
 *   ADD_CONST  x += *scalar; complex: real and imaginary part each              524-574
 *   RECIP      1 / x; complex: the scaled form 399-425 (C_SCPL entirely in float, 454-480)
 *   MUL        a * b; complex re = a.re*b.re - a.im*b.im, im = a.re*b.im + a.im*b.re
 *   DIV        a / b (INT_MIN / -1, undefined in C, is the wrapped INT_MIN); complex: the
 *              scaled form 1177-1194, for C_SCPL with every intermediate a double   1136-1266
 *   MAX, MIN   a >= b ? a : b, a <= b ? a : b (with a NaN: b; +0 against -0: a).  Complex:
 *              squared moduli after scaling by 1 / max|parts|, in double; MAX takes a only if
 *              |a|^2 > |b|^2, MIN only if <, a tie gives b, both zero gives a      1533-1720
 * Zero divisors (RECIP: x == 0, so -0.0 too, complex both parts zero; DIV: b == 0, complex
 * b.re == 0 where |b.re| >= |b.im|): the reference aborts at the first one.  Here that element
 * is left unwritten, every other element is written, and the call returns GAAMD_ZERO_DIVISOR.
 * RECIP and DIV therefore synchronise their stream before they return; the other five return
 * with the kernel in flight, like gaamd_patch_add. */
#define GAAMD_ELEM_ABS 1         /* fn of gaamd_patch_elem1 */
#define GAAMD_ELEM_ADD_CONST 2
#define GAAMD_ELEM_RECIP 3
#define GAAMD_ELEM_MUL 4         /* fn of gaamd_patch_elem2 */
#define GAAMD_ELEM_DIV 5
#define GAAMD_ELEM_MAX 6
#define GAAMD_ELEM_MIN 7
#define GAAMD_ZERO_DIVISOR 2
int gaamd_patch_elem1(int op, int fn, const void *scalar /* ADD_CONST only */, void *dst,
                      const long long *dst_stride, const long long *count, int ndim, void *stream);
int gaamd_patch_elem2(int op, int fn, const void *a, const long long *a_stride, const void *b,
                      const long long *b_stride, void *c, const long long *c_stride,
                      const long long *count, int ndim, void *stream);
/* The minimum (want_max != 0: maximum) element of a patch and its position; the kernel under
 * NGA_Select_elem (select.c:143-250).  Key: the element itself; complex re*re + im*im in the
 * element's own real type (two products, one sum).  `value` receives the element's bits (for
 * complex the element, not the key), `key` (may be NULL) the compared quantity, `index` the
 * element's linear index in the patch with count[0] fastest.  Among equal keys the lowest index
 * wins (the reference's first occurrence; of +0 and -0 the one that comes first), whatever the
 * grid: two launches, partials in device scratch, no atomics; the same input gives the same
 * answer on every run.  A patch that holds a NaN returns an unspecified element (the
 * reference's answer depends on where the NaN lies).  Synchronises its stream, like
 * gaamd_patch_dot, whose geometry, checks and codes it has (-5: value or index missing).
 * A count of zero: returns 1 and *index = -1, nothing launched. */
int gaamd_patch_select(int op, int want_max, const void *a, const long long *a_stride,
                       const long long *count, int ndim, void *value /* host, one element */,
                       void *key /* host, may be NULL: the compared quantity */,
                       long long *index /* host */, void *stream);
/* The kernels under GA's matrix.c calls (ga.h: GA_Norm1 / GA_Norm_infinity, the diagonal calls,
 * GA_Scale_rows / GA_Scale_cols), global/src/matrix.c expression for expression, no FMA, all six
 * types, integers in unsigned (wraparound) arithmetic, every offset 64-bit.
 *
 * gaamd_patch_norm: a one-operand reduction over a patch with gaamd_patch_dot's geometry, checks
 * and negative codes (-4 also for an unknown kind, -5 a missing result).  The per-element
 * quantity q is GA_ABS(x) = x >= 0 ? x : -x for the real and integer types (INT_MIN / LONG_MIN
 * wrap to themselves, -0.0 stays -0.0) and sqrt(re*re + im*im) for the complex ones: two
 * products and one sum in the real type, then the correctly rounded square root (for C_SCPL the
 * float one; the reference's (float)sqrt((double)x) is the same number).
 *   GAAMD_NORM_ONE  the sum of q in the element's own type (complex: its real type; integers wrap),
 *                   matrix.c:1118-1171.  The reduction has gaamd_patch_dot's fixed shape -- lane,
 *                   wave tree, waves in order, one partial per workgroup, one final workgroup, no
 *                   atomics -- so the same input gives the same bits on every run.
 *   GAAMD_NORM_INF  the maximum of q, matrix.c:801-859.  It does not depend on the order it is
 *                   taken in, so it is exact on any grid.  Signed zeros: -0.0 only if every q is
 *                   -0.0, else +0.0 before -0.0.  Integers compare signed, so a wrapped INT_MIN
 *                   loses to every other value.  A patch holding a NaN gives an unspecified
 *                   result, as for gaamd_patch_select.
 * It synchronises its stream and writes `result` (host): one value of the element's type, for
 * complex of its real type.  A count of zero: 0, the type's zero written, nothing launched.
 *
 * gaamd_diagonal: n elements, element i of the matrix side at a + i * a_step BYTES and of the
 * vector side at v + i * v_step bytes (for the diagonal of a row-major matrix a_step =
 * (ld + 1) * elemsize; steps may be negative).  One lane per element; a 16-byte element moves
 * as one 16-byte access where bases and steps are 16-byte aligned, an 8-byte complex one as one
 * 8-byte access where they are 8-byte aligned, and as its parts otherwise.  Returns with the
 * kernel in flight.
 *   GAAMD_DIAG_GET    v_i = a_i, a bit copy (NaN payloads and -0.0 survive)
 *   GAAMD_DIAG_SET    a_i = v_i, a bit copy
 *   GAAMD_DIAG_ADD    a_i += v_i, complex real and imaginary part each      matrix.c:1640-1690
 *   GAAMD_DIAG_SHIFT  a_i += *scalar, complex part by part (v is not used)  2080-2127
 *   GAAMD_DIAG_ZERO   a_i = 0 (v is not used)
 * Negative codes, all before any launch: -4 an unknown op or fn, -3 a negative n, -7 n of 2^39 or
 * more, -5 a missing a, a missing scalar for SHIFT or a missing v for GET / SET / ADD, -8 a base
 * or step below 4-byte alignment, -11 the byte spans of the a side and the v side (first element
 * to last) overlap.  n == 0: 0, nothing launched.
 * (The name gaamd_diag is the library's diagnostic entry point, last section.)
 *
 * gaamd_scale_rows: a[i][j] *= v[i];  gaamd_scale_cols: a[i][j] *= v[j];  i < rows, j < cols, in
 * place on a row-major matrix with lda in ELEMENTS between rows; v is contiguous (rows, resp.
 * cols elements).  Real types: one product.  Complex is PART BY PART, re *= v.re and im *= v.im
 * (matrix.c:2494-2503, 2700-2710): the reference's expression, NOT a complex product.  On the
 * map kernel's streaming shape: 16-byte vectors where the base, lda, the row length (and for
 * cols v's base) allow, 8 or 4 bytes otherwise; non-temporal accesses to a; more than 65535 rows
 * in several launches.  rows: the multiplier is uniform per workgroup; cols: v's vector is
 * loaded beside a's with a cached load (every row reads it again).  Nothing outside the rows x
 * cols elements is written.  Return with the kernel in flight.  Codes as gaamd_patch_scale:
 * -3 a negative extent, -4 an unknown op, -5 v missing, -6 lda below cols, -7 2^31 rows or more,
 * -8 a base below 4-byte alignment, and -11 v's bytes overlap a's span (first stored element to
 * last).  A zero extent: 0, no launch. */
#define GAAMD_NORM_ONE 1
#define GAAMD_NORM_INF 2
#define GAAMD_DIAG_GET 1
#define GAAMD_DIAG_SET 2
#define GAAMD_DIAG_ADD 3
#define GAAMD_DIAG_SHIFT 4
#define GAAMD_DIAG_ZERO 5
int gaamd_patch_norm(int op, int kind, const void *a, const long long *a_stride,
                     const long long *count, int ndim,
                     void *result /* host, one value of the element's (complex: real) type */, void *stream);
int gaamd_diagonal(int op, int fn, long long n, void *a, long long a_step, void *v, long long v_step,
                   const void *scalar /* SHIFT only */, void *stream);
int gaamd_scale_rows(int op, long long rows, long long cols, void *a, long long lda, const void *v, void *stream);
int gaamd_scale_cols(int op, long long rows, long long cols, void *a, long long lda, const void *v, void *stream);
/* The kernels under GA's sparse.c calls (ga.h: GA_Patch_enum, GA_Scan_copy, GA_Scan_add, GA_Pack,
 * GA_Unpack), global/src/sparse.c expression for expression, no FMA: enumerate, the segmented
 * scans, and stream compaction by a mask.  Arrays are contiguous and 1-D, n is in elements, every
 * index and byte offset is 64-bit.  op is the value type and mop the mask type, both COMEX_ACC_*
 * codes; all six types on both sides, in any combination.  Integers in unsigned (wraparound)
 * arithmetic; complex part by part.
 * A mask element is SET when it is non-zero (neq_zero_reg / neq_zero_cpl of abstract_ops.h): for
 * complex when either part is; -0.0 is not set, a NaN is, a denormal is.
 * (The names gaamd_pack / gaamd_unpack are the strided pack and unpack of section 2; the
 * compaction is gaamd_mask_pack / gaamd_mask_unpack.)
 *
 * gaamd_enum: dst[i] = start + (T)(first + i) * stride, i < n (sparse.c:59-76): first + i is a
 * 64-bit integer converted to the element type (integers: truncated), one product, one sum;
 * complex re = start.re + (R)(first + i) * stride.re and im likewise.  start and stride are one
 * host element each.  Returns with the kernel in flight.
 *
 * The segmented scans.  A segment starts at every set element.  fn:
 *   GAAMD_SCAN_COPY      dst[i] = src[s], s the last set index at or before i: a bit copy (NaN
 *                        payloads and -0.0 survive).  Elements before the first set one are
 *                        written ZERO (sparse.c:196-206).
 *   GAAMD_SCAN_ADD       dst[i] = src[s] + ... + src[i] (inclusive).  Elements before the first set
 *                        one are NOT WRITTEN (sparse.c:361-365, scan_addc.c:116-134).
 *   GAAMD_SCAN_ADD_EXCL  dst[i] = src[s] + ... + src[i-1]; +0 at i == s.  (The reference's loop
 *                        starts the sum from that zero: the two differ only where every term is
 *                        -0.0, which comes out as -0.0 here.)
 * open != 0: a segment is open on entry and *carry (host, one element) is its value so far --
 * the leftmost term of every sum up to the first set element, for COPY the value copied there.
 * gaamd_scan returns with its kernels in flight.  dst must not overlap src or msk.
 * gaamd_scan_tail is the reduction half, for the ranks of a distributed scan: *has_flag = 1 when
 * any element is set; *tail = the open value at the end of the range -- ADD (either): the sum
 * of src from the last set element to n - 1, of the whole range when none is set; COPY: the bits
 * of src at the last set element, zero when none is set.  One pass over src and msk.  It
 * synchronises its stream and writes both host outputs.  The next range's gaamd_scan takes
 * (open = has_flag or an earlier range's, carry = tail combined on the host).
 *
 * The compaction.  With f_k the k-th set element: gaamd_mask_count writes their number to *count
 * (host) after synchronising; gaamd_mask_pack packed[k] = src[f_k]; gaamd_mask_unpack
 * dst[f_k] = packed[k], the unset elements of dst are not written, nor is packed past the count.
 * Bit copies of 4-, 8- or 16-byte elements.  Both return with their kernels in flight.  The written
 * side must not overlap the other two (packed judged at n elements).
 *
 * Shape: reduce, then scan -- three launches, and no workgroup ever waits for another (no
 * look-back, no grid barrier), no atomics.  (1) one workgroup per tile of gaamd_scan_tile()
 * elements computes the tile's aggregate: (a set element present, the open value at the tile's
 * end), or the tile's set count; (2) ONE workgroup scans the aggregates in tile order,
 * gaamd_scan_agg_span() of them per pass of its loop; (3) one workgroup per tile redoes its tile
 * from its prefix and writes.  The aggregates live in the calling thread's device scratch
 * (gaamd_patch_dot's, recycled call to call, freed at comex_finalize): calls of one thread that
 * are in flight together must be on one stream.
 *
 * SUMMATION ORDER, a contract.  The combine (f1, v1) (+) (f2, v2) = (f1 | f2, f2 ? v2 : v1 + v2)
 * is associative, so integer results are exact in any tree.  For float, double and the complex
 * types the tree is fixed: a lane folds its 8 consecutive elements left to right; the 64 lanes of
 * a wave are combined by the scan steps 1, 2, 4, 8, 16, 32 (at each step lane l takes the value
 * of lane l - step on its left); the 4 waves of a workgroup in order; the tiles by the same
 * procedure with 4 aggregates per lane, the passes in order; an element's result is
 *   ((((carry (+) tiles before) (+) waves before) (+) lanes before) (+) elements before) (+) x.
 * The same input therefore gives the same bits on every run.  Exactly summable data (every
 * partial sum representable) give the sequential loop's bits; inexact data need not, and stay
 * within the error bound of any summation order.  The identity is -0.0 (-0.0 + x has the bits of
 * x), so empty prefixes and positions past n change no bit.
 *
 * Access: a lane's 8 consecutive elements move as 16-byte vectors where the base is 16-byte
 * aligned, as 8- or 4-byte ones otherwise; bases need 4-byte alignment only.
 * Negative codes, all before any launch or allocation, in this order: -3 a negative n; -4 an
 * unknown op, mop or fn; -5 a missing pointer or host output (carry with open != 0); -7 n above
 * GAAMD_SCAN_MAX_N; -8 a base below 4-byte alignment; -11 a forbidden overlap.  n == 0: 0 and no
 * launch, the host outputs written (count 0, has_flag 0, tail zero).  gaamd_scan_tile: -4 for an
 * unknown type. */
#define GAAMD_SCAN_COPY 1
#define GAAMD_SCAN_ADD 2
#define GAAMD_SCAN_ADD_EXCL 3
#define GAAMD_SCAN_MAX_N (1ll << 34)
int gaamd_scan_tile(int op, int mop);   /* elements per tile (workgroup) */
int gaamd_scan_agg_span(void);          /* tile aggregates per pass of launch (2)'s loop */
int gaamd_enum(int op, long long n, long long first, const void *start, const void *stride, void *dst, void *stream);
int gaamd_scan_tail(int op, int fn, int mop, long long n, const void *src, const void *msk,
                    int *has_flag /* host */, void *tail /* host, one element */, void *stream);
int gaamd_scan(int op, int fn, int mop, long long n, const void *src, const void *msk, void *dst, int open,
               const void *carry /* host, one element; open != 0 only */, void *stream);
int gaamd_mask_count(int mop, long long n, const void *msk, long long *count /* host */, void *stream);
int gaamd_mask_pack(int op, int mop, long long n, const void *src, const void *msk, void *packed, void *stream);
int gaamd_mask_unpack(int op, int mop, long long n, const void *packed, const void *msk, void *dst, void *stream);
/* GA's sparse arrays (global/src/sparse.array.c) as kernels on a block CSR in HBM; the kernels
 * under NGA_Sprs_array_matvec_multiply, _get_diag, _shift_diag, _diag_left_multiply and
 * _diag_right_multiply (ga.h).  op = COMEX_ACC_* names the element type, all six.
 * Layout: the rows of one rank, cut into nblk column blocks.  Block b has a table of nrows + 1
 * row offsets (int) at offs + b * (nrows + 1); they are relative to start[b], the place where the
 * block begins in jdx (int, GLOBAL column indices) and val (elements).  offs, start (long long,
 * nblk of them), jdx, val, x, y and d are HBM addresses.  The entries of a row, over the blocks in
 * ascending order, form one list e_0 .. e_{c-1}.
 *   gaamd_spmv   y[r] = sum over the row's list of val * x[jdx - x_first], r < nrows; x_first is
 *                the global column of x[0].  y is overwritten; a row without entries gives +0.
 * Arithmetic and order (a contract): per entry one product, then one add, never fused.  Integers
 * wrap (unsigned arithmetic).  A complex product is re = a.re*x.re - a.im*x.im,
 * im = a.re*x.im + a.im*x.re, and the sum is taken part by part.  A team of W = `team` lanes
 * computes a row: lane L sums e_L, e_{L+W}, ... sequentially from +0, and the W partials p are
 * combined by the butterfly p[l] = p[l] + p[l ^ s] for s = 1, 2, .. W / 2 (lanes past the row's
 * end hold +0).  The same arrays and team therefore give the same bits on every call, however the
 * list is cut into blocks.  Nothing of x is read but the elements the entries name.
 *   gaamd_spmv_team(nnz_total, rows)   the team the GA layer uses: the smallest power of two W
 *                with 2 * W * rows >= nnz_total, 1 <= W <= 64 (1 when either count is < 1); it grows
 *                with nnz_total and shrinks with rows, and knows nothing of ranks.
 *   gaamd_sprs_diag   ONE column block (offs its table, jdx / val from its start), row r being
 *                global row diag_first + r:  fn = GAAMD_DIAG_GET: out[r] = the value of the last
 *                entry of row r, in storage order, whose column is diag_first + r; out[r] is left
 *                alone where there is none.  fn = GAAMD_DIAG_SHIFT: every such entry += *shift
 *                (host, one element), complex part by part; no entry is created.
 *   gaamd_sprs_scale_left    one column block: val[k] = d[r] * val[k] for the entries k of row r
 *   gaamd_sprs_scale_right   n entries: val[k] = d[jdx[k] - d_first] * val[k]
 *                both the true complex product, re = d.re*v.re - d.im*v.im, im = d.re*v.im + d.im*v.re
 *                (sparse.array.c:1754-1770), unlike gaamd_scale_rows.
 * One team per row, 256 / W rows per workgroup, teams packed into wave64; rows are walked with a
 * 64-bit stride loop, and every offset into offs, jdx, val, x, y is 64-bit.  For W >= 2 consecutive
 * lanes read consecutive jdx / val.  The cross-lane step is ds_bpermute_b32; no atomics, no LDS,
 * no scratch (k_spmv: at most 30 VGPRs).
 * Negative codes, all before any launch, in this order: -3 a negative nrows, nblk or n; -4 an
 * unknown op or fn, or a team that is no power of two in 1..64; then nrows == 0 (n == 0): 0 and
 * no launch; -5 a missing pointer (gaamd_spmv with nblk == 0 needs y only); -7 nrows above 2^40
 * (n from 2^39); -8 val, x, y, d or out below the element's alignment, start below 8, offs or jdx
 * below 4. */
int gaamd_spmv_team(long long nnz_total, long long rows);
int gaamd_spmv(int op, long long nrows, int nblk, const int *offs, const long long *start, const int *jdx,
               const void *val, const void *x, long long x_first, void *y, int team, void *stream);
int gaamd_sprs_diag(int op, int fn, long long nrows, const int *offs, const int *jdx, void *val, long long diag_first,
                    void *out, const void *shift /* host, one element */, int team, void *stream);
int gaamd_sprs_scale_left(int op, long long nrows, const int *offs, void *val, const void *d, int team, void *stream);
int gaamd_sprs_scale_right(int op, long long n, const int *jdx, void *val, const void *d, long long d_first,
                           void *stream);
/* Sparse x dense, and the conversions between a dense block and the block CSR; the kernels under
 * NGA_Sprs_array_sprsdns_multiply, _create_from_dense and _create_from_sparse (ga.h).  All six
 * types.  The dense sides are row-major with ld ELEMENTS between rows, all HBM.
 *   gaamd_spmm   c[r][j] = sum over row r's list of val * b[jdx - b_first][j], r < nrows, j < n; the
 *                block CSR is gaamd_spmv's; b[0] is global row b_first of B; c is nrows x n.
 * Arithmetic and order (a contract): c[r][j] starts from +0 and takes, per entry, one product and
 * then one add, never fused, the entries in the order of the row's ONE list over the column
 * blocks ascending: acc = acc + val * b.  Integers wrap.  A complex product is the true product
 * re = a.re*b.re - a.im*b.im, im = a.re*b.im + a.im*b.re, added part by part.  A row without
 * entries gives +0; c is OVERWRITTEN.  Of b nothing is read but the rows the entries name; the gap
 * ldc - n of c is not written.  Each (r, j) being one sequential sum, the bits do not depend on
 * the grid, the tiling, the vector width or on how the list is cut into blocks; column 0 of an
 * n = 1 product is gaamd_spmv with team 1, bit for bit.
 * Shape: the lanes of a wave run along j; a row is taken by a group of G = 2^k lanes, each holding
 * V consecutive columns, 256 / G rows per workgroup (so 64 / G rows per wave for narrow n).  V is
 * 16 bytes' worth where b, c are 16-byte aligned and ldb, ldc, n are multiples of V, else 1.  G is
 * the smallest power of two with G * V >= n, at most 64; wider n is cut into tiles of G * V
 * columns over the grid's second dimension, the row's jdx / val being read once per tile.  The lanes
 * of a group read val[k] / jdx[k] by the same-address load.  Rows: a 64-bit stride loop.
 *   gaamd_dense_row_counts   counts[r] = the kept elements of row r of the rows x cols block a,
 *                whose element (0, 0) is global (row_first, col_first).  KEPT: the value != 0 (so
 *                -0.0 is not kept, a NaN is; complex: either part) or the element lies on the global
 *                diagonal, row_first + r == col_first + c (sparse.array.c:3234, 3263).
 *   gaamd_dense_to_csr   offs = the rows + 1 exclusive prefix sums of those counts (HBM): the kept
 *                elements of row r go to jdx / val at offs[r] .., in ascending column order, jdx the
 *                GLOBAL column col_first + c, val the bits unchanged.
 *                Both walk a row in runs of 64 consecutive columns, one wave per row; a ballot and a
 *                count of the lanes below give each kept lane its place.
 *   gaamd_csr_to_dense   ONE column block (as gaamd_sprs_diag takes it) into the nrows x cols window
 *                `out` whose column 0 is global column col_first: out[r][jdx - col_first] = val.
 *                The caller zeroes `out`; nothing else of it is written.  Of duplicates of one (r, j),
 *                which lie side by side, the last in storage order is stored: an entry whose successor
 *                in the row names the same column is skipped, so no address has two writers.  An
 *                entry outside the window is not stored.
 * No atomics, no LDS, no scratch; every index into every array is 64-bit (k_spmm: 43 to 74 VGPRs).
 * Negative codes, all before any launch, in this order: -3 a negative count (nrows, nblk, n, rows,
 * cols); -4 an unknown op; then a zero nrows, n, rows or cols: 0 and no launch; -5 a missing
 * pointer (gaamd_spmm with nblk == 0 needs c only); -6 an ld below the stored row length (ldb with
 * nblk > 0, ldc, lda, ldo); -7 nrows or rows above 2^40, n or cols above 2^31 - 1, a negative
 * row_first or col_first, col_first + cols above 2^31; -8 a, b, c, val or out below the element's
 * alignment, start below 8, offs, counts or jdx below 4; -11 the byte span of the output (c;
 * counts; jdx / val; out) overlaps that of a dense input or of offs.  Where a length is not an
 * argument -- the rows of b the entries name, the offs[rows] entries of jdx / val -- the first
 * row of b, the first entry of jdx / val stands for the span. */
int gaamd_spmm(int op, long long nrows, int nblk, const int *offs, const long long *start, const int *jdx,
               const void *val, const void *b, long long ldb, long long b_first, long long n, void *c, long long ldc,
               void *stream);
int gaamd_dense_row_counts(int op, long long rows, long long cols, const void *a, long long lda, long long row_first,
                           long long col_first, int *counts, void *stream);
int gaamd_dense_to_csr(int op, long long rows, long long cols, const void *a, long long lda, long long row_first,
                       long long col_first, const int *offs, int *jdx, void *val, void *stream);
int gaamd_csr_to_dense(int op, long long nrows, long long cols, const int *offs, const int *jdx, const void *val,
                       long long col_first, void *out, long long ldo, void *stream);
/* Sparse x sparse, C = A B with all three sparse (sparse.array.c:2424-3103); the kernels under
 * NGA_Sprs_array_matmat_multiply (ga.h).  All six types, all addresses HBM.  A is the block CSR of
 * gaamd_spmv.  B is a ROW CSR: brows + 1 offsets (long long) into rjdx (int, global columns) / rval,
 * row k of it being global row b_first + k of B, each row's entries its ONE list; the entries of A
 * name rows in [b_first, b_first + brows).  Offsets are 64-bit because a gathered B may exceed 2^31
 * entries although no rank's part does.
 * REQUIRED of the caller of gaamd_spgemm_count and gaamd_spgemm_fill, and checked by neither (the
 * arrays lie in HBM): (1) every row of the row CSR is in ascending column order, so that duplicates
 * of one (k, j) lie side by side -- what gaamd_csr_rows gives from an assembled block CSR; otherwise
 * two lanes add onto one value at once and the result is undefined; (2) every jdx of A lies in
 * [b_first, b_first + brows); otherwise roffs is read out of bounds; (3) coffs / cstart are the
 * prefix sums of the counts gaamd_spgemm_count gave for the same operands.
 *   gaamd_csr_rows   flattens a block CSR into the row CSR of the same nrows rows: roffs (nrows + 1),
 *                rjdx and rval (as many entries as the block CSR holds), every row's one list
 *                contiguous, the blocks ascending, storage order kept: row lengths over the blocks,
 *                a prefix sum, a copy.  With nblk == 0, roffs becomes nrows + 1 zeros.
 *   gaamd_spgemm_count   counts[b * nrows + r] = the DISTINCT columns j of row r of C that lie in
 *                column block b of ncut, a column j of jdim_c belonging to block
 *                min(j * ncut / jdim_c, ncut - 1); every one of the ncut blocks has its nrows counts,
 *                an empty one zeros.  bound[r] = U[r] = the sum of the lengths of the rows of B that
 *                row r's entries name, duplicates counted: the products of the row.
 *   gaamd_spgemm_fill    given coffs, the [ncut][nrows + 1] exclusive prefix sums of those counts per
 *                block, and cstart[ncut], where each block begins in cjdx / cval (both HBM): the
 *                columns of row r in block b go to cjdx at cstart[b] + coffs[b][r] .., ascending,
 *                their values to cval.  cstart[b] + coffs[b][nrows] is below 2^31 for every b.
 * Structure: C holds exactly one entry per (r, j) for which some k has a stored a_rk and a stored
 * b_kj; existence only is tested, never a value, so a product of 0 or a sum that cancels keeps its
 * entry.
 * Arithmetic and order (a contract, as gaamd_spmm's): c_rj starts from +0 and takes one product and
 * then one add per contributing pair, never fused.  The order: A's row-r list as ONE list over its
 * column blocks ascending, duplicates in storage order; for each A entry with column k, B's row-k
 * list in storage order, restricted to column j.  A complex product is the true product, part by
 * part; integers wrap.  One stated departure: the reference ASSIGNS the first product where this
 * ADDS it to +0; the two differ only for a lone -0.0 product.  With that start, for finite data
 * and a B without duplicates, the dense copy of C equals gaamd_spmm of A with the dense copy of B
 * bit for bit.  The bits depend neither on the grid nor on the path a row takes.
 * Shape: one wave per row.  A row with U <= gaamd_spgemm_lds_cap() (1024) collects its columns in
 * an LDS hash set (integer compare-and-swap on the key only), compacts and bitonic-sorts it; the
 * cuts are found by binary search.  A larger row takes its column blocks in windows of 32768
 * columns marked in an LDS bitmap, walking its products once per window: the same bits, not fast.
 * Fill walks A's row list sequentially with the lanes along B's row; duplicates (k, j) lie side by
 * side in B's row, only the head of a run acts and adds its run in order, so a place has one writer
 * per A entry: plain loads and stores, no floating-point atomics.  8 KiB of LDS per wave (20 waves
 * per CU), no scratch memory, no HBM scratch; every index into every array is 64-bit.
 * Negative codes, all before any launch, in this order: -3 a negative nrows, nblk, brows, jdim_c or
 * ncut; -4 an unknown op (csr_rows, fill); then nrows == 0 (count, fill: or ncut == 0): 0 and no
 * launch; -5 a missing pointer (with nblk == 0 the outputs only -- roffs; counts and bound; coffs,
 * cstart, cjdx, cval); -7 nrows or brows above 2^40, jdim_c outside 1 .. 2^31 - 1, a negative
 * b_first (ncut may exceed jdim_c: blocks without columns stay empty); -8 val, rval or cval below
 * the element's alignment, start, roffs, cstart or bound below 8, offs, jdx, rjdx, coffs, counts or
 * cjdx below 4; -11 an output overlaps an input (a length that is no argument is stood for by the
 * first entry). */
int gaamd_spgemm_lds_cap(void);
int gaamd_csr_rows(int op, long long nrows, int nblk, const int *offs, const long long *start, const int *jdx,
                   const void *val, long long *roffs, int *rjdx, void *rval, void *stream);
int gaamd_spgemm_count(long long nrows, int nblk, const int *offs, const long long *start, const int *jdx,
                       long long b_first, long long brows, const long long *roffs, const int *rjdx, long long jdim_c,
                       int ncut, int *counts, long long *bound, void *stream);
int gaamd_spgemm_fill(int op, long long nrows, int nblk, const int *offs, const long long *start, const int *jdx,
                      const void *val, long long b_first, long long brows, const long long *roffs, const int *rjdx,
                      const void *rval, long long jdim_c, int ncut, const int *coffs, const long long *cstart, int *cjdx,
                      void *cval, void *stream);
/* Row-major GEMM on the gfx950 matrix cores, for op = COMEX_ACC_DBL (v_mfma_f64_16x16x4_f64)
 * and COMEX_ACC_FLT (v_mfma_f32_16x16x4_f32); the kernel under GA_Dgemm / GA_Sgemm (ga.h):
 *   C[i][j] = alpha * sum_k op(A)[i][k] * op(B)[k][j] + beta * C[i][j],  i < m, j < n, kk < k
 * op(X) = X for trans 'N'/'n', its transpose for 'T'/'t'.  As stored, row-major with ld in
 * ELEMENTS between rows: A is m x k ('N') or k x m ('T'), B is k x n or n x k, C is m x n.
 * Any m, n, k >= 0, any ld >= the stored row length, bases aligned to the element; all
 * offsets are 64-bit.  Nothing outside the m x n elements of C is written, nothing outside
 * the stored elements of A and B is read.
 * Summation order (a contract): every element of C has one accumulator, which starts at
 * +0 and takes its k products in increasing k -- four consecutive k per matrix-core
 * instruction, each instruction adding onto the result of the one before (for f32 this is
 * bit for bit the fmaf chain over k; for f64 the instruction's own fixed order within its
 * four).  The order does not depend on where the element lies in C or in the launch grid,
 * nor on m and n: a sub-rectangle of C computed alone (offset base pointers, the same ld
 * and k) has the bits it has in the whole product, and so has every repeat of a call.
 * Then C = alpha * acc + beta * C as two products and one sum, no FMA (gaamd_patch_add's
 * expression).  beta == 0: C is not read (a NaN there does not propagate) and
 * C = alpha * acc.  alpha == 0 or k == 0: A and B are not read and C = beta * C
 * (gaamd_patch_scale; all zeros when beta == 0 too).  m == 0 or n == 0: 0, no launch.
 * Negative codes, nothing launched: -3 a negative extent, -4 an op other than DBL / FLT or
 * a trans other than N n T t, -5 alpha or beta missing, -6 an ld below the stored row
 * length, -7 2^31 tiles of C or more, -8 a base below element alignment, -11 C overlaps A
 * or B.  Overlap is judged on byte spans, first stored element to last: C being exactly A
 * overlaps, and so does a C that lies between the rows of B (inside B's ld padding, sharing
 * no element with it); a C that begins where A's last element ends does not. */
int gaamd_gemm(int op, int transa, int transb, long long m, long long n, long long k,
               const void *alpha, const void *a, long long lda, const void *b, long long ldb,
               const void *beta, void *c, long long ldc, void *stream);
/* gaamd_gemm's checks without a launch (no GPU needed): 0 it would launch, 1 nothing to do
 * (m or n is 0), or its error code; plan[0..5] = {tile M, tile N, tile K (the workgroup's
 * tile of C and its k step), tiles along m = ceil(m / tile M), tiles along n, k steps} */
int gaamd_gemm_plan(int op, int transa, int transb, long long m, long long n, long long k,
                    const void *alpha, const void *a, long long lda, const void *b, long long ldb,
                    const void *beta, const void *c, long long ldc, long long plan[6]);
/* Row-major complex GEMM on the gfx950 matrix cores, for op = COMEX_ACC_DCP
 * (v_mfma_f64_16x16x4_f64 on the parts) and COMEX_ACC_CPL (v_mfma_f32_16x16x4_f32); the kernel
 * under GA_Zgemm / GA_Cgemm (ga.h).  gaamd_gemm's argument list, expression and storage rules,
 * with elements interleaved (re, im), alpha and beta pointing at one complex element and ld in
 * COMPLEX ELEMENTS.  op(X) = X for trans 'N'/'n', its transpose for 'T'/'t', its conjugate
 * transpose for 'C'/'c' (stored as for 'T').  Bases aligned to the element's real part (8 / 4
 * bytes) are enough; all offsets are 64-bit.
 * Summation order (a contract): trans 'C' negates the imaginary part first, exactly.  Every
 * element of C has two accumulators, re and im, both starting at +0.  For each group of four
 * consecutive k, counted from 0 in increasing order, re takes the matrix-core instruction over
 * a.re * b.re, then the one over -a.im * b.im; im takes the one over a.re * b.im, then the one
 * over a.im * b.re -- four real products per complex product, never three.  Nothing depends
 * on where the element lies in C or in the launch grid, nor on m and n: a sub-rectangle of C
 * computed alone has the bits it has in the whole product, and so has every repeat of a call.
 * Then, with s the accumulators and no FMA: t.re = al.re * s.re - al.im * s.im,
 * t.im = al.re * s.im + al.im * s.re; u = beta * c formed the same way; c = t + u part by
 * part.  beta == (0,0): C is not read and c = t.  beta exactly (1,0): c = t + c with no
 * products on C -- exact, so a -0 or an infinity there is not turned into something else by a
 * multiplication.  alpha == (0,0) or k == 0: A and B are not read and C = beta * C
 * (gaamd_patch_scale for that op; all zeros when beta == (0,0) too).  m == 0 or n == 0: 0, no
 * launch.
 * Negative codes and the overlap rule are gaamd_gemm's: -4 is an op other than DCP / CPL or a
 * trans other than N n T t C c, -8 a base below the alignment of the real part.
 * gaamd_gemm_cplx_plan: gaamd_gemm_plan's answers; the tile constants differ between the two
 * ops and from gaamd_gemm's. */
int gaamd_gemm_cplx(int op, int transa, int transb, long long m, long long n, long long k,
                    const void *alpha, const void *a, long long lda, const void *b, long long ldb,
                    const void *beta, void *c, long long ldc, void *stream);
int gaamd_gemm_cplx_plan(int op, int transa, int transb, long long m, long long n, long long k,
                         const void *alpha, const void *a, long long lda, const void *b, long long ldb,
                         const void *beta, const void *c, long long ldc, long long plan[6]);
/* Row-major transpose through LDS tiles; the kernels under GA_Transpose / GA_Symmetrize (ga.h).
 *   gaamd_transpose:      dst[j][i] = src[i][j],  i < rows, j < cols
 *     src is rows x cols, dst is cols x rows.  A pure bit copy: op is any COMEX_ACC_* code and
 *     only gives the element size (INT FLT 4, DBL CPL LNG 8, DCP 16 bytes); NaN payloads and
 *     -0 survive.
 *   gaamd_transpose_acc:  c[i][j] = alpha * (c[i][j] + b[j][i]),  i < m, j < n
 *     c is m x n, in place; b is n x m.  op = COMEX_ACC_DBL or COMEX_ACC_FLT.  The reference's
 *     expression (ga_symmetr.c:41): one add, then one multiply -- not alpha*c + alpha*b, no FMA.
 * Row-major with ld in ELEMENTS between rows; any extents >= 0, any ld >= the stored row
 * length, bases aligned to the element; all offsets are 64-bit.  A side whose base and ld are
 * multiples of 16 bytes moves 16-byte vectors, any other side single elements (decided per
 * launch).  Nothing outside the source's elements is read, nothing outside the destination's
 * elements -- its ld padding included -- is written.  A zero extent: 0, no launch.
 * Negative codes, nothing launched, with gaamd_gemm's meanings: -3 a negative extent, -4 an
 * unknown op (for _acc: anything but DBL / FLT), -5 alpha missing, -6 an ld below the stored
 * row length, -7 2^31 tiles or more, -8 a base below element alignment, -11 the byte spans of
 * source and destination (first stored element to last) overlap: dst equal to src overlaps,
 * and so does a dst inside src's ld padding; a dst that begins where src's last element ends
 * does not. */
int gaamd_transpose(int op, long long rows, long long cols,
                    const void *src, long long lds, void *dst, long long ldd, void *stream);
int gaamd_transpose_acc(int op, long long m, long long n, const void *alpha,
                        const void *b, long long ldb, void *c, long long ldc, void *stream);
/* gaamd_transpose's checks without a launch (no GPU needed): 0 it would launch, 1 nothing to
 * do (rows or cols is 0), or its error code; plan[0..3] = {tile rows, tile cols (of src, in
 * elements), tiles along rows = ceil(rows / tile rows), tiles along cols} */
int gaamd_transpose_plan(int op, long long rows, long long cols, const void *src,
                         long long lds, const void *dst, long long ldd, long long plan[4]);
long gaamd_packed_size(const int *count, int stride_levels);
int gaamd_pack(const void *src, const int *src_stride, const int *count, int stride_levels,
               void *packed, void *stream);
int gaamd_unpack(const void *packed, void *dst, const int *dst_stride, const int *count,
                 int stride_levels, void *stream);
int gaamd_unpack_acc(int op, const void *scale, const void *packed, void *dst,
                     const int *dst_stride, const int *count, int stride_levels, void *stream);
/* The launch plan of a strided operation without launching anything (no GPU
 * needed): plan[0..7] = {kind (1 rows, 2 flat, 3 serial, 4 ordered), vector width, unroll
 * (for kind 4: 0 one workgroup, 1 column slices with src prefetch, 2 column slices in
 * place), threads per block, launches, blocks, stride levels after merging, chunk grid
 * aligned}; row_end = ~0 for all rows.  Returns 0 or the launcher's error code. */
int gaamd_plan_strided(int op, const void *src, const int *src_stride, const void *dst, const int *dst_stride,
                       const int *count, int stride_levels, unsigned long long row_begin,
                       unsigned long long row_end, long long plan[8]);
/* kind / vector width / unroll / launches / blocks of the last kernel-level call */
int gaamd_last_launch(int *kind, int *width, int *unroll, int *launches,
                      unsigned long long *blocks);
/* kernel launches since start, by kind: counts[0..4] = {unused, rows, flat,
 * serial, ordered}, every caller of this process (user calls, progress thread, wire) */
int gaamd_kernel_counts(unsigned long long counts[5]);
/* requests this rank posted to same-node owners, by route: counts[0..3] =
 * {packed chunks (pack -> staging -> owner unpack), direct-source (owner reads
 * our segment), io-vector, rmw} */
int gaamd_route_counts(unsigned long long counts[4]);
/* Operations that took the reference's route toggles beyond SELF/SMP, since init:
 * [0] strided operations split row by row (COMEX_ENABLE_{ACC,PUT,GET}_PACKED=0),
 * [1] io-vector descriptors split pair by pair (COMEX_ENABLE_{ACC,PUT,GET}_IOV=0),
 * [2] gets through the owner (COMEX_ENABLE_GET_SELF/SMP=0). */
int gaamd_toggle_counts(unsigned long long counts[3]);
/* Local io-vector launches whose destinations may repeat (>= 2048 pairs, or fewer
 * with a repeat), by path: [0] hashed (only pairs sharing a destination sorted, in
 * LDS), [1] hashed, then the radix path for the pairs it could not order (more than
 * 8192 such pairs), [2] the radix path (above the other paths' range, or for the
 * partitions [3] deferred), [3] ordered in LDS: one workgroup below 1 Ki pairs, hash
 * partitions up to 4 Mi pairs (tuning iov_lds=0 routes to [0]-[2] instead). */
int gaamd_iov_path_counts(unsigned long long counts[4]);
/* runs fn(t, ctx) for t = 0 .. T-1 (1 <= T <= 16) on the library's persistent host worker
 * pool, t = 0 on the calling thread, and returns when all have; -1 on bad arguments.
 * One job at a time (concurrent callers wait); fn must not call back into this function. */
int gaamd_host_parallel(int T, void (*fn)(int t, void *ctx), void *ctx);
/* one-pass accumulates this rank applied into the segment of a rank on the same GPU */
unsigned long long gaamd_one_pass_count(void);
/* comex_malloc calls served by a freed segment block kept for reuse (with its IPC export) */
unsigned long long gaamd_segment_cache_reuse(void);
/* segments this rank replaced because a peer's fresh IPC mapping did not read their tags */
unsigned long long gaamd_segment_remaps(void);
/* times the freed-segment cache was given back under device-memory pressure */
unsigned long long gaamd_segment_cache_trims(void);
/* the kind of this rank's segment holding p: 0 none, 1 HBM, 2 host (node shm,
   COMEX_AMD_SEGMENT=host: the host may read and write it directly) */
int gaamd_segment_kind(const void *p);
/* vmm segment allocator: hipMemSetAccess refusals retried at a fresh range (diagnostic) */
unsigned long long gaamd_vmm_access_retries(void);
/* CPU self-test of the vmm allocator's descriptor exchange over the bootstrap (no GPU):
   wrong or missing descriptors, 0 = pass */
int gaamd_vmm_exchange_selftest(int rounds);
/* same-node peers whose staging buffer this rank could not map by IPC at
 * comex_init (remote accumulates to or from them would abort); -1 before init */
int gaamd_peers_unmapped(void);
/* requests this rank's progress thread applied, by kind: packed, io-vector, rmw, direct-source */
int gaamd_owner_counts(unsigned long long counts[4]);
/* keys: "kind" (0 auto, 1 rows, 2 flat, 3 serial, 4 ordered), "block" (0 auto/64/128),
 * "flat_max_nvec", "align", "flat_line_min", "ordered_cols" (column-sliced ordered
 * kernel), "streams", "iov_lds" (1: io-vectors with repeated destinations ordered in
 * LDS up to 4 Mi pairs; 0: the hashed / radix paths); returns the previous value or -1 */
int gaamd_set_tuning(const char *key, int value);
int gaamd_get_tuning(const char *key);

/* ---- 3. device plumbing ------------------------------------------------ */
int gaamd_device_count(void);
int gaamd_set_device(int dev);
void *gaamd_stream(void);
/* library stream i (0 = gaamd_stream()), or NULL past gaamd_num_streams() */
void *gaamd_stream_at(int i);
void *gaamd_dev_malloc(size_t bytes);
int gaamd_dev_free(void *p);
void *gaamd_host_malloc(size_t bytes);   /* pinned, device-mapped */
int gaamd_host_free(void *p);
int gaamd_memcpy(void *dst, const void *src, size_t bytes);   /* any direction, synchronous */
/* a 2-D patch, any direction, synchronous: `height` rows of `width` bytes, rows
 * `spitch` / `dpitch` bytes apart (hipMemcpy2D) */
int gaamd_memcpy2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height);
int gaamd_memset(void *dst, int value, size_t bytes);
int gaamd_sync(void *stream);          /* NULL: all library streams */
/* order the primary stream (gaamd_stream()) after everything enqueued on the
 * library's other streams, and them after it (COMEX_AMD_STREAMS > 1) */
int gaamd_join(void);
int gaamd_num_streams(void);
/* synthetic inputs of SURVEY.md 8(d) generated on the device; type:
 * 0 f64, 1 f32, 2 i32, 3 i64 ; n elements from splitmix64(seed) */
int gaamd_fill(void *dst, long n, int type, unsigned long long seed, void *stream);
/* n 8-byte words of one bit pattern (8-byte aligned dst) */
int gaamd_fill_word(void *dst, long n, unsigned long long word, void *stream);
void *gaamd_stream_create(void);       /* an extra blocking HIP stream */
int gaamd_stream_destroy(void *stream);
/* HIP events on the library stream (or `stream`) */
void *gaamd_event_create(void);
int gaamd_event_destroy(void *ev);
int gaamd_event_record(void *ev, void *stream);
int gaamd_event_sync(void *ev);
float gaamd_event_elapsed_ms(void *start, void *stop);
const char *gaamd_version(void);
/* path of the HIP runtime (libamdhip64) this library's calls resolve to */
const char *gaamd_hip_runtime(void);
/* build provenance: sha256 (hex) of the sources this library was compiled from --
 * ga_amd/csrc/ and include/ (ga_amd/provenance.py) -- so a stale prebuilt library is
 * detectable against the tree beside it */
const char *gaamd_build_id(void);

/* ---- test and diagnostic hooks (not used by GA) ------------
 * One entry point; returns 0, or -1 for an unknown key.
 *   "stamps"        host stamps (CLOCK_BOOTTIME ns) of the last strided call and
 *                   the last comex_wait_all: [0] call entry, [1] route decided
 *                   (launch lock held), [2] stream picked, [3] kernel launched,
 *                   [4] call return, [5] wait entry, [6] streams about to be
 *                   synchronised, [7] synchronised.  out (nout >= 8, may be NULL)
 *                   receives them; value 1 clears them and starts stamping, 0
 *                   stops, -1 leaves it.
 *   "stale_gen"     N > 0: every peer treats its first mapping of each rank's N-th
 *                   allocation as stale, so the replace-and-repeat path of
 *                   comex_malloc runs on demand (0: off).
 *   "stale_granule" G >= 0 (with stale_gen): instead, each owner writes a foreign
 *                   tag into granule G (G * 2 MiB bytes in) of its N-th allocation
 *                   on the first exchange, and the peers' check must find it
 *                   (-1: off).
 *   "iov_host_sides" out[0] (nout >= 1): io-vector sides found wholly in pageable
 *                   host memory by one /proc/self/maps pass (value ignored).
 *   "host_range"    that pass on its own: out[0], out[1] (nout >= 2) hold [lo, hi) on
 *                   entry, value 1 asks for writable memory; out[0] is 1 when every
 *                   byte lies in readable (writable) mappings that are not device
 *                   files, else 0.  Needs no GPU.
 *   "pinned_threads" out[0] (nout >= 1): threads that hold pinned bounce buffers or
 *                   a non-blocking ring now (a thread's are freed when it ends, every
 *                   thread's at comex_finalize).
 *   "publish"       1: the conservative publication mode -- every direct-source
 *                   post, every packed-chunk post and every fence first records a
 *                   system-scope release (hipEventReleaseToSystem) on each library
 *                   stream and waits for them (the markers round 5 measured and took
 *                   out of the default path); 0: the default; -1 leaves it.  out[0]
 *                   (nout >= 1) receives the previous setting.  Used to classify a
 *                   cross-GPU mismatch as visibility (clears) or logic (persists).
 *   "drop_chunk"    N > 0: the owner's progress thread counts every N-th packed chunk
 *                   applied without running its kernel (a test hook: a logic fault);
 *                   0: off.
 *   "peer_gets"     out[0] (nout >= 1): strided gets this rank read from another GPU's
 *                   memory with system-scope loads.
 *   "vmm_window"    out[0], out[1] (nout >= 2): bytes of the vmm allocator's private
 *                   address window taken so far and bytes left.  Every mapping (this
 *                   rank's blocks and its imports of peers' blocks) takes
 *                   round_up(bytes, 2 MiB) + 2 MiB of it, never handed out again;
 *                   comex_malloc aborts with a message once it is used up. */
int gaamd_diag(const char *key, long long value, unsigned long long *out, int nout);

#if defined(__cplusplus)
}
#endif

#endif /* GA_AMD_H */
