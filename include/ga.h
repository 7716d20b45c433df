/*
 * ga.h -- the Global Arrays C API subset on the one-sided accumulate path,
 * exported by libga_amd_ga.so (the caller row a15 of SURVEY.md §8(a)), a
 * library of its own over libga_amd.so's public ABI.  libga_amd.so -- the
 * drop-in beneath global/src -- defines none of these names, so a real GA that
 * defines them itself (global/src/capi.c) links against it unchanged.
 *
 * Same names, argument order and index conventions as the reference C API
 * (global/src/capi.c, global/src/ga.h): C (row-major, 0-based) subscripts at
 * the API, converted to GA's Fortran order (column-major, 1-based) inside, as
 * capi.c:54-61 does.  Arrays use the REGULAR block distribution: the process
 * grid of ddb/ddb_h2 (global/src/decomp.c) and the block map of pnga_allocate
 * (base.c:2550-2630), or an explicit map with NGA_Create_irreg.  Each rank's
 * block lives in its GPU's HBM (one comex_malloc segment per array).
 */
#ifndef GA_AMD_GA_H
#define GA_AMD_GA_H

#if defined(__cplusplus)
extern "C" {
#endif

/* global/src/gacommon.h:14-22 (MT_BASE 1000, ma/macommon.h:11-20) */
#define C_INT 1001
#define C_LONG 1002
#define C_FLOAT 1003
#define C_DBL 1004
#define C_SCPL 1006
#define C_DCPL 1007
#define GA_MAX_DIM 7

/* complex scalars (comex/src-common/acc.h:6-15) */
#ifndef GA_AMD_COMPLEX_TYPES
#define GA_AMD_COMPLEX_TYPES
typedef struct { double real; double imag; } DoubleComplex;
typedef struct { float real; float imag; } SingleComplex;
#endif

int GA_Initialize(void);
void GA_Terminate(void);
int GA_Nodeid(void);
int GA_Nnodes(void);
void GA_Sync(void);
void GA_Error(char *msg, int code);

int NGA_Create(int type, int ndim, int dims[], char *name, int chunk[]);
int NGA_Create_irreg(int type, int ndim, int dims[], char *name, int block[], int map[]);
void GA_Destroy(int g_a);
void GA_Zero(int g_a);
void NGA_Distribution(int g_a, int iproc, int lo[], int hi[]);
int NGA_Locate_num_blocks(int g_a, int lo[], int hi[]);

/* one-sided patch operations (capi.c:2079-2089, onesided.c:1334-1471) */
void NGA_Acc(int g_a, int lo[], int hi[], void *buf, int ld[], void *alpha);
void NGA_Put(int g_a, int lo[], int hi[], void *buf, int ld[]);
void NGA_Get(int g_a, int lo[], int hi[], void *buf, int ld[]);

/* non-blocking patch operations (capi.c:2103-2190 -> pnga_nbacc/nbput/nbget,
   onesided.c:685, 1300, 1481) and their wait (pnga_nbwait, onesided.c:368);
   ga_nbhdl_t is GA's Integer (ga.h:18) */
typedef long ga_nbhdl_t;
void NGA_NbAcc(int g_a, int lo[], int hi[], void *buf, int ld[], void *alpha, ga_nbhdl_t *nbhandle);
void NGA_NbPut(int g_a, int lo[], int hi[], void *buf, int ld[], ga_nbhdl_t *nbhandle);
void NGA_NbGet(int g_a, int lo[], int hi[], void *buf, int ld[], ga_nbhdl_t *nbhandle);
void NGA_NbWait(ga_nbhdl_t *nbhandle);
/* every skip[d]-th element of the patch; buf holds only the selected elements
   (capi.c:1990-2060 -> pnga_strided_acc/put/get, onesided.c:4225-4470) */
void NGA_Strided_acc(int g_a, int lo[], int hi[], int skip[], void *buf, int ld[], void *alpha);
void NGA_Strided_put(int g_a, int lo[], int hi[], int skip[], void *buf, int ld[]);
void NGA_Strided_get(int g_a, int lo[], int hi[], int skip[], void *buf, int ld[]);
/* direct access to the local block (an HBM address) */
/* gather / scatter / scatter-accumulate of single elements: capi.c:3026-3160 ->
   gai_gatscat onesided.c:2747 (one ARMCI_GetV/PutV/AccV per owner).  subsArray[k]
   points at the ndim C subscripts of element k; *_flat takes them as one array. */
void NGA_Scatter(int g_a, void *v, int *subsArray[], int n);
void NGA_Scatter_flat(int g_a, void *v, int subsArray[], int n);
void NGA_Scatter_acc(int g_a, void *v, int *subsArray[], int n, void *alpha);
void NGA_Scatter_acc_flat(int g_a, void *v, int subsArray[], int n, void *alpha);
void NGA_Gather(int g_a, void *v, int *subsArray[], int n);
void NGA_Gather_flat(int g_a, void *v, int subsArray[], int n);

void NGA_Access(int g_a, int lo[], int hi[], void *ptr, int ld[]);
void NGA_Release(int g_a, int lo[], int hi[]);
void NGA_Release_update(int g_a, int lo[], int hi[]);

/* Computing on arrays where they lie (capi.c:1645-1880, 2375, 2748, 3574-3990,
   4163-4250 -> global/src/global.npatch.c, global.nalg.c).  Collective, with the
   reference's syncs on entry and exit; each rank runs one gfx950 kernel on its own
   part of the patch (ga_amd.h gaamd_patch_*), the reference's arithmetic expression
   for expression.  The dot products end in a sum over ranks: every rank returns the
   same bits, and the same arrays give the same bits on every call.  Arrays of equal
   block maps with equal patches are computed in place; any other combination goes
   through a GA_Duplicate temporary and NGA_Copy_patch, as in the reference.
   Transposed patches (trans / t_a / t_b other than 'N'), patches of different rank or
   extents, a type that does not match the call, and arrays in a host segment abort
   through GA_Error. */
int GA_Duplicate(int g_a, char *array_name);
int GA_Compare_distr(int g_a, int g_b);   /* 0: same shape and block maps */
void NGA_Inquire(int g_a, int *type, int *ndim, int dims[]);
void GA_Fill(int g_a, void *value);
void GA_Scale(int g_a, void *value);
void GA_Add(void *alpha, int g_a, void *beta, int g_b, int g_c);
void GA_Copy(int g_a, int g_b);
int GA_Idot(int g_a, int g_b);
long GA_Ldot(int g_a, int g_b);
float GA_Fdot(int g_a, int g_b);
double GA_Ddot(int g_a, int g_b);
SingleComplex GA_Cdot(int g_a, int g_b);
DoubleComplex GA_Zdot(int g_a, int g_b);
void NGA_Fill_patch(int g_a, int lo[], int hi[], void *val);
void NGA_Zero_patch(int g_a, int lo[], int hi[]);
void NGA_Scale_patch(int g_a, int lo[], int hi[], void *alpha);
void NGA_Add_patch(void *alpha, int g_a, int alo[], int ahi[], void *beta, int g_b, int blo[], int bhi[],
                   int g_c, int clo[], int chi[]);
void NGA_Copy_patch(char trans, int g_a, int alo[], int ahi[], int g_b, int blo[], int bhi[]);
int NGA_Idot_patch(int g_a, char t_a, int alo[], int ahi[], int g_b, char t_b, int blo[], int bhi[]);
long NGA_Ldot_patch(int g_a, char t_a, int alo[], int ahi[], int g_b, char t_b, int blo[], int bhi[]);
float NGA_Fdot_patch(int g_a, char t_a, int alo[], int ahi[], int g_b, char t_b, int blo[], int bhi[]);
double NGA_Ddot_patch(int g_a, char t_a, int alo[], int ahi[], int g_b, char t_b, int blo[], int bhi[]);
SingleComplex NGA_Cdot_patch(int g_a, char t_a, int alo[], int ahi[], int g_b, char t_b, int blo[], int bhi[]);
DoubleComplex NGA_Zdot_patch(int g_a, char t_a, int alo[], int ahi[], int g_b, char t_b, int blo[], int bhi[]);
/* Matrix multiply on the gfx950 matrix cores (capi.c GA_Dgemm, GA_Sgemm,
   NGA_Matmul_patch -> global/src/matmul.c):
     C = alpha * op(A) * op(B) + beta * C,   op(X) = X ('N' 'n') or its transpose ('T' 't')
   on 2-D arrays of C_DBL or C_FLOAT, one type for all three; REGULAR or irregular block
   maps, which need not agree.  Collective, GA_Sync on entry and exit.
   Patch subscripts: alo/ahi, blo/bhi and clo/chi are C subscripts into the arrays AS
   STORED, and op(A) is that stored patch or its transpose -- with m x k = op(A),
   k x n = op(B), m x n = the C patch.  For 'N' this is the reference's meaning.  For 'T'
   the reference's own range check (matmul.c:2105-2117) reads the same numbers as op()
   coordinates and is inconsistent on non-square arrays; the rule here is the one above.
   GA_Dgemm / GA_Sgemm are the patch form over the leading corners as stored: A's
   m x k (k x m for 'T'), B's k x n (n x k for 'T'), C's m x n.
   Owner computes: a rank cuts the C patch by its own block, fetches the rows of op(A)
   and columns of op(B) it needs in panels of gaamd_ga_gemm_panel() values of k, counted
   from the start of the patch's k range, into HBM scratch (freed before return) and runs
   gaamd_gemm (ga_amd.h) into its block in place: the caller's beta on the first panel,
   beta = 1 on the later ones.
   Rank independence: with gaamd_gemm's order contract -- per element of C one sum from
   +0 in increasing k within a panel, then alpha * sum + beta * C without FMA -- the
   result for given arrays is the same bits on any number of ranks and any block maps,
   as the dot products' is.  beta == 0 does not read C (a NaN there does not propagate).
   Aborts through GA_Error, before the first sync or launch: a type that is not C_DBL /
   C_FLOAT, differs between the arrays or does not match the call; a rank other than 2;
   a trans other than N n T t; a patch out of range; patch extents that do not agree; an
   array in a host segment; g_c equal to g_a or g_b with patches that overlap (an owner
   would read what another rank is writing).
   Complex arrays (capi.c GA_Zgemm, GA_Cgemm, which the reference hands to a host zgemm /
   cgemm): GA_Zgemm on C_DCPL, GA_Cgemm on C_SCPL and NGA_Matmul_patch on either run the
   same loop over gaamd_gemm_cplx (ga_amd.h), with beta = (1,0) on the later panels, which
   that kernel adds exactly.  For complex arrays, and only for them, trans may also be
   'C' 'c': op(X) is the conjugate transpose, the stored patch shaped as for 'T'.  Rank
   independence holds as above with gaamd_gemm_cplx's order contract: two accumulators per
   element from +0, four real products per complex product in a fixed sequence, increasing
   k within a panel, then alpha * acc + beta * C part by part without FMA.  Aborts: as
   above with C_DCPL / C_SCPL among the types; 'C' 'c' on real arrays (GA_Dgemm, GA_Sgemm
   and NGA_Matmul_patch on them answer as before); GA_Zgemm / GA_Cgemm on arrays of
   another type. */
void GA_Dgemm(char ta, char tb, int m, int n, int k, double alpha, int g_a, int g_b, double beta, int g_c);
void GA_Sgemm(char ta, char tb, int m, int n, int k, float alpha, int g_a, int g_b, float beta, int g_c);
void GA_Zgemm(char ta, char tb, int m, int n, int k, DoubleComplex alpha, int g_a, int g_b, DoubleComplex beta,
              int g_c);
void GA_Cgemm(char ta, char tb, int m, int n, int k, SingleComplex alpha, int g_a, int g_b, SingleComplex beta,
              int g_c);
void NGA_Matmul_patch(char transa, char transb, void *alpha, void *beta, int g_a, int alo[], int ahi[],
                      int g_b, int blo[], int bhi[], int g_c, int clo[], int chi[]);
/* values of k per panel of the owner-computes loop (a fixed constant, 1024) */
int gaamd_ga_gemm_panel(void);
/* Transpose and symmetrize on HBM blocks (capi.c GA_Transpose -> pnga_transpose,
   global.nalg.c:954; GA_Symmetrize -> pnga_symmetrize, ga_symmetr.c:49):
     GA_Transpose:   B = A^T          2-D arrays of one type, any of the six; B's dims are
                                      A's reversed; a bit copy (NaN payloads, -0 survive)
     GA_Symmetrize:  A = 0.5*(A+A^T)  a square 2-D array of C_DBL or C_FLOAT
   REGULAR or irregular block maps, which need not agree between A and B.  Collective,
   GA_Sync on entry and exit.
   Destination owner computes: a rank takes its own block of the destination (rows
   r0..r1, columns c0..c1 as stored), gets the mirror patch of the source (rows c0..c1,
   columns r0..r1) into HBM scratch of one block's size with NGA_Get's path, and runs
   gaamd_transpose / gaamd_transpose_acc (ga_amd.h) from the scratch into its block in
   place; the scratch is freed before return.  GA_Symmetrize always goes through the
   scratch copy, and holds a barrier between the gets and the kernels: every rank has read
   before any rank writes.  Each element is 0.5 * (a_ij + a_ji), one add and one multiply,
   so the result equals its own transpose bit for bit and is the same bits on any number of
   ranks and any block map.
   Aborts through GA_Error, before the first sync or launch: g_a == g_b, a rank other
   than 2, types that differ, B's dims not A's reversed (transpose); a rank other than 2,
   an array that is not square, a type other than C_DBL / C_FLOAT (symmetrize); an array
   in a host segment (both). */
void GA_Transpose(int g_a, int g_b);
void GA_Symmetrize(int g_a);
/* Element-wise algebra and element selection on HBM blocks (capi.c GA_Abs_value ...
   GA_Elem_minimum_patch -> global/src/elem_alg.c; NGA_Select_elem -> global/src/select.c).
   Collective, with the reference's syncs; each rank runs one gfx950 kernel on its own part
   of the patch (ga_amd.h gaamd_patch_elem1 / _elem2 / _select), the reference's arithmetic
   expression for expression (listed there).  All six types.
     GA_Abs_value       a = |a|              GA_Elem_multiply   c = a * b
     GA_Add_constant    a = a + *alpha       GA_Elem_divide     c = a / b
     GA_Recip           a = 1 / a            GA_Elem_maximum / _minimum   c = max / min(a, b)
   The unary calls work in place like NGA_Scale_patch.  The binary calls follow NGA_Add_patch:
   equal block maps with equal patches are computed in place (g_c may be g_a and / or g_b, so
   GA_Elem_multiply(g_a, g_b, g_a) is legal); any other combination goes through GA_Duplicate
   temporaries and NGA_Copy_patch (ngai_elem2_patch_, elem_alg.c:1886-1930), destroyed before
   return.
   Departure 1, complex GA_Abs_value: the reference uses hypot() where the C library has it.
   The host's and the device's hypot are different functions, so the reference's portable
   branch (the larger part times sqrt(1 + ratio^2)) is used instead: it is the only one whose
   bits can be reproduced anywhere.
   Zero divisors (GA_Recip, GA_Elem_divide): the reference aborts at the first one.  Here the
   kernel leaves such elements unwritten and writes all others; after it has completed the
   ranks combine their flags and, if any is set, EVERY rank ends through GA_Error ("zero
   divisor"), so none is left waiting in a barrier.
   NGA_Select_elem(g_a, "min" | "max", val, index): the smallest / largest element (complex:
   by re*re + im*im in the element's real type), its bits in *val and its C subscripts in
   index[].  Syncs on entry (select.c:268-270).
   Departure 2, ties: the result is the best key over all ranks and, among equal keys, the
   element of the lowest row-major (C order) linear index in the whole array -- the
   reference's first occurrence on one rank, and, unlike the reference (whose
   armci_msg_sel_scope breaks ties by rank), the same answer on any number of ranks and any
   block map, as the dot products and gemm are.  Of +0 and -0 the one that comes first is
   returned, with its sign.  An array that holds a NaN returns an unspecified element.
   Aborts through GA_Error, before the first sync or launch: types that differ, a patch out
   of range, patches of different rank or extents, an array in a host segment; an op that is
   neither "min" nor "max". */
void GA_Abs_value(int g_a);
void GA_Abs_value_patch(int g_a, int *lo, int *hi);
void GA_Add_constant(int g_a, void *alpha);
void GA_Add_constant_patch(int g_a, int *lo, int *hi, void *alpha);
void GA_Recip(int g_a);
void GA_Recip_patch(int g_a, int *lo, int *hi);
void GA_Elem_multiply(int g_a, int g_b, int g_c);
void GA_Elem_divide(int g_a, int g_b, int g_c);
void GA_Elem_maximum(int g_a, int g_b, int g_c);
void GA_Elem_minimum(int g_a, int g_b, int g_c);
void GA_Elem_multiply_patch(int g_a, int *alo, int *ahi, int g_b, int *blo, int *bhi, int g_c, int *clo, int *chi);
void GA_Elem_divide_patch(int g_a, int *alo, int *ahi, int g_b, int *blo, int *bhi, int g_c, int *clo, int *chi);
void GA_Elem_maximum_patch(int g_a, int *alo, int *ahi, int g_b, int *blo, int *bhi, int g_c, int *clo, int *chi);
void GA_Elem_minimum_patch(int g_a, int *alo, int *ahi, int g_b, int *blo, int *bhi, int g_c, int *clo, int *chi);
void NGA_Select_elem(int g_a, char *op, void *val, int *index);
/* Diagonals, row / column scaling and norms on HBM blocks (capi.c:4940-4986 -> global/src/matrix.c).
   Collective, GA_Sync on entry and exit; the reference's arithmetic expression for expression
   (ga_amd.h gaamd_diagonal / gaamd_scale_rows / gaamd_scale_cols / gaamd_patch_norm).  All six types.
     GA_Shift_diagonal(g_a, c)   a[i][i] += *c          GA_Zero_diagonal(g_a)   a[i][i] = 0
     GA_Set_diagonal(g_a, g_v)   a[i][i] = v[i]         GA_Add_diagonal(g_a, g_v)   a[i][i] += v[i]
     GA_Get_diag(g_a, g_v)       v[i] = a[i][i]
   g_a has rank 2, g_v rank 1 and min(dims[0], dims[1]) elements (matrix.c:1512).  Complex adds
   work on the real and the imaginary part each.
     GA_Scale_rows(g_a, g_v)     a[i][j] *= v[i],  v of dims[0] elements
     GA_Scale_cols(g_a, g_v)     a[i][j] *= v[j],  v of dims[1] elements
   SUBSCRIPTS ARE THE C API's: i is the first C subscript of g_a, j the second, and dims[] is what
   NGA_Create was called with.  (capi.c reverses the index order and therefore hands
   GA_Scale_rows to the Fortran-order pnga_scale_cols and the reverse; the result is the above.)
   Complex scaling is PART BY PART, re *= v.re and im *= v.im (matrix.c:2494-2503, 2700-2710):
   the reference's expression, not a complex product.
   Owner of g_a computes: a rank cuts the diagonal by its own block (rows r0..r1, columns
   c0..c1: elements max(r0,c0)..min(r1,c1)), or takes the rows / columns of its block.  Where that
   range of g_v lies wholly in the rank's own block of g_v it is used in place; otherwise it is
   fetched into HBM scratch with NGA_Get's path (GA_Get_diag: written to scratch by the kernel,
   then stored with NGA_Put's path, complete at its owner before the closing sync).  The scratch
   is freed before return.  REGULAR or irregular block maps, which need not agree between g_a
   and g_v.  A rank that owns nothing of the diagonal launches nothing and takes part in the syncs.
     GA_Norm1(g_a, nm)          *nm = sum |a|     GA_Norm_infinity(g_a, nm)   *nm = max |a|
   over ALL elements of an array of rank 1 or 2, as matrix.c:998-1018 / 1306-1325 compute them
   (not the induced matrix norms); |x| is GA_ABS, for complex sqrt(re*re + im*im).  Each rank
   reduces its block in the element's own type (complex: its real type; integers wrap), a rank
   owning nothing contributes 0, the ranks combine with armci_msg_?gop "+" / "max" in that type,
   and *nm is that value converted to double.  Every rank returns the same bits and the same
   arrays give the same bits on every call.  GA_Norm_infinity also returns the same bits on any
   number of ranks and any block map; GA_Norm1 does so for the integer types only -- for the
   floating-point types its roundings depend on how the array is cut, as the dot products' do.
   Aborts through GA_Error, before the first sync or launch: g_a not of rank 2 (diagonal and
   scale calls) or not of rank 1 or 2 (norms), g_v not of rank 1 or of the wrong length, types
   that differ, a missing c or nm, an array in a host segment. */
void GA_Shift_diagonal(int g_a, void *c);
void GA_Set_diagonal(int g_a, int g_v);
void GA_Zero_diagonal(int g_a);
void GA_Add_diagonal(int g_a, int g_v);
void GA_Get_diag(int g_a, int g_v);
void GA_Scale_rows(int g_a, int g_v);
void GA_Scale_cols(int g_a, int g_v);
void GA_Norm1(int g_a, double *nm);
void GA_Norm_infinity(int g_a, double *nm);
/* Enumerate, segmented scans, pack and unpack on HBM blocks (capi.c:2261-2373 -> global/src/sparse.c):
   the calls a GA program builds CSR offsets with, compresses a vector by a mask and expands it
   again.  Collective, GA_Sync on entry and exit; the arrays are 1-D; lo and hi are C subscripts,
   inclusive.  All six value types and all six mask types, in any combination.  A mask element is
   set when it is non-zero (complex: either part; -0.0 is not set, a NaN is).  Set mask elements
   outside [lo, hi] are ignored, and elements of g_dst outside [lo, hi] are never written.  Each rank
   runs the kernels of ga_amd.h (gaamd_enum, gaamd_scan_tail + gaamd_scan, gaamd_mask_count +
   gaamd_mask_pack / gaamd_mask_unpack) on its own part of the range; a rank that owns nothing of it
   launches nothing and takes part in the exchange and the syncs.
     GA_Patch_enum(g_a, lo, hi, start, inc)   a[i] = *start + (T)(i - lo) * *inc, lo <= i <= hi
   (complex part by part; integers wrap).
     GA_Scan_copy(g_src, g_dst, g_msk, lo, hi)        dst[i] = src at the last set element in [lo, i];
                                                      zero before the first set one
     GA_Scan_add(g_src, g_dst, g_msk, lo, hi, excl)   dst[i] = src[s] + ... + src[i], s the last set
                                                      element in [lo, i]; excl != 0: ... + src[i-1], zero
                                                      at s; elements before the first set one are NOT
                                                      written (scan_addc.c:116-134 is the meaning)
   Across ranks: each rank reduces its part (has a set element, open value at its end), the ranks
   exchange these pairs bit for bit (one slot per rank of a zeroed array, armci_msg_lgop "+"), and
   each rank forms its carry on the host: the tail of the nearest rank before it, in block order,
   that holds a set element, plus -- for the adds -- the tails of the ranks between in ascending
   order; then it scans its part with that carry.  For the integer types and for exactly summable
   data the results are the same bits on any number of ranks and any block map; for inexact
   floating-point data they are the same bits on every call for a given rank count and map, and
   depend on how the array is cut, as GA_Norm1's and the dot products' do (summation order: ga_amd.h).
   DEPARTURES from sparse.c: its second phase -- a pnga_gather of partial results from the ranks
   between and a local fix-up loop (409-434) -- and its remote pnga_get of one element of g_src in
   the exclusive case (378-382) are both replaced by the carry above; nothing is fetched from
   another rank's block.
     GA_Pack(g_src, g_dst, g_msk, lo, hi, icount)     dst[k] = src[f_k], f_k the k-th set element of
                                                      [lo, hi], k from 0; *icount = their number
     GA_Unpack(g_src, g_dst, g_msk, lo, hi, icount)   dst[f_k] = src[k]; the other elements stay
   Bit copies.  Each rank counts its set elements, the ranks exchange the counts, a rank's place is
   the sum of the counts before it in block order.  The packed side (g_dst of pack, g_src of
   unpack) may have any block map: where the rank's range of it lies in its own block the kernel
   works there in place, otherwise through HBM scratch and NGA_Put's / NGA_Get's path (a put is
   complete at its owner before the closing sync); the scratch is freed before return.  The packed
   side must hold *icount elements: otherwise every rank ends through GA_Error with a message that
   names both numbers, and nothing was moved (the reference does not check this).
   Aborts through GA_Error on every rank, before the first sync or launch: an array of rank other
   than 1; lo > hi or a range outside the array; value types that differ; g_src == g_dst; block maps
   of g_src and g_msk that differ (scans, pack) or of g_dst and g_msk (scans, unpack); an array in
   a host segment; a missing icount, start or inc.  The *64 forms are not provided. */
void GA_Patch_enum(int g_a, int lo, int hi, void *start, void *inc);
void GA_Scan_copy(int g_src, int g_dst, int g_msk, int lo, int hi);
void GA_Scan_add(int g_src, int g_dst, int g_msk, int lo, int hi, int excl);
void GA_Pack(int g_src, int g_dst, int g_msk, int lo, int hi, int *icount);
void GA_Unpack(int g_src, int g_dst, int g_msk, int lo, int hi, int *icount);
/* Sparse arrays (global/src/ga.h:355-382 -> global/src/sparse.array.c), the 32-bit-index forms: a
   distributed idim x jdim sparse matrix of any of the six types, held as a block CSR in each rank's
   HBM, and its product with a distributed vector.
   Distribution: row i belongs to rank min((i * nproc) / idim, nproc - 1), column j to column block
   min((j * nproc) / jdim, nproc - 1), in 64-bit arithmetic (sparse.array.c:326, 524).
   NGA_Sprs_array_row_distribution / _column_distribution return that set for iproc as [lo, hi],
   zero-based and inclusive; a rank that owns nothing gets hi = lo - 1.  gaamd_ga_sprs_range is the
   same rule for any dim and nproc, host-only (no GPU, no GA_Initialize).
   Handles are a name space of their own, counted from 1.  A sparse array holds NO global array
   inside: its CSR lies in plain HBM allocations of the rank, so gaamd_ga_live_arrays() does not
   change from NGA_Sprs_array_create to NGA_Sprs_array_destroy (the incoming segment of assemble is
   freed before it returns).  The array NGA_Sprs_array_get_diag returns is the caller's to destroy.
     s_a = NGA_Sprs_array_create(idim, jdim, type)        local bookkeeping, the same call on every rank
     NGA_Sprs_array_add_element(s_a, i, j, &val)          local; any rank may add any (i, j), zero-based
     NGA_Sprs_array_assemble(s_a)                         collective; returns 1
   Assembly, an order contract (the reference places elements by pnga_read_inc, in arrival order):
   the ranks exchange the nproc x nproc table of counts; rank r's elements for owner p are stored
   after those of the ranks before r, in insertion order; the owner then stable-sorts what it holds
   by column block, row and column.  Duplicates of one (i, j) stay separate entries, in source-rank
   then insertion order.  The sort runs on the host and the result is uploaded once.
   Layout, as NGA_Sprs_array_access_col_block(s_a, icol, &idx, &jdx, &val) shows it: per non-empty
   column block, idx holds the rank's row count + 1 row offsets relative to the block's start, jdx
   global zero-based column indices and val the values; entries within a row are in ascending
   column order (the reference's TODO at sparse.array.c:764).  All three are HBM ADDRESSES like
   NGA_Access's, for kernels, not for host dereference; all three are NULL for an empty block.
   NGA_Sprs_array_col_block_list(s_a, &idx, &n) returns the non-empty blocks, ascending, in a
   malloc'ed list the caller frees.  NGA_Sprs_array_duplicate copies the matrix as it stands (the
   copy outlives the original); NGA_Sprs_array_destroy frees it.  Both collective.
     NGA_Sprs_array_matvec_multiply(s_a, g_a, g_v)        v = S a
   g_a has rank 1, jdim elements and the matrix's type, g_v rank 1, idim elements and that type;
   REGULAR or irregular block maps, which need not match the matrix's cuts or each other.  The owner
   of a row block computes with gaamd_spmv (ga_amd.h).  It needs g_a over the span of its non-empty
   column blocks: used in place where that span lies in its own block of g_a, otherwise fetched into
   HBM scratch with NGA_Get's path.  It writes g_v for its rows in place where they lie in its own
   block of g_v, otherwise through scratch and NGA_Put's path, complete at the owner before the
   closing sync; the scratch is freed before return.  g_v is OVERWRITTEN (rows without entries give
   0; the reference's macro assigns per column block).  A rank without rows launches nothing and
   takes part in the syncs.  gaamd_ga_sprs_route_counts: {x in place, x through scratch, y in place,
   y through scratch} taken so far on this rank.
   Arithmetic contract: gaamd_spmv's -- per entry one product and one add, never fused; integers wrap;
   the true complex product re = a.re*x.re - a.im*x.im, im = a.re*x.im + a.im*x.re (a stated
   departure: the reference's complex macro reads the vector where it means the matrix value); the
   entries of a row over all column blocks in ascending order are ONE list, summed by a team of W
   lanes, lane L taking e_L, e_{L+W}, ... from +0 and the partials combined by a fixed butterfly.
   W = gaamd_spmv_team(entries of the whole matrix, idim) depends on global counts only.
   Consequence: for a matrix without duplicate (i, j), or whose duplicates keep their relative
   order, the product is the same bits on every call, on any number of ranks, and under any block
   maps of g_a and g_v: the column blocks change with the rank count, the concatenated list does not.
   The other calls, the reference's expressions as kernels on the block CSR in place (ga_amd.h
   gaamd_sprs_diag, gaamd_sprs_scale_left / _right, gaamd_patch_scale):
     NGA_Sprs_array_get_diag(s_a, &g_d)       a new 1-D array of idim elements on the row cuts, zeroed,
                                              then d_i = a_ii where stored -- from the rank's own
                                              diagonal column block only (sparse.array.c:1646-1693);
                                              of duplicates the last in storage order
     NGA_Sprs_array_shift_diag(s_a, &shift)   a_ii += shift on EVERY stored (i, i); none is created;
                                              complex part by part
     NGA_Sprs_array_scale(s_a, &scale)        every value *= scale, as GA_Scale
     NGA_Sprs_array_diag_left_multiply(s_a, g_d)    a_ij = d_i * a_ij, d of idim elements
     NGA_Sprs_array_diag_right_multiply(s_a, g_d)   a_ij = d_j * a_ij, d of jdim elements
   both true complex products (sparse.array.c:1754-1770), unlike GA_Scale_rows; d may have any
   block map and is obtained as g_a is.
   Aborts through GA_Error -- the collective calls on every rank, before the first sync or launch:
   idim or jdim <= 0 or an unknown type; add_element after assemble, with an index out of range or
   without a value; any computing call, access_col_block and col_block_list before assemble; a
   second assemble; a handle that is not live; a vector of the wrong rank, length or type, or in a
   host segment; g_a == g_v; a rank that would hold 2^31 entries or more; a missing shift, scale or
   g_d.
   Sparse x dense and the conversions (sparse.array.c:3222-3840), all collective:
     g_c = NGA_Sprs_array_sprsdns_multiply(s_a, g_b)      a NEW array g_c = S B
   g_b has rank 2, C dimensions jdim x n, the matrix's type, lives in HBM and may be under any block
   map.  g_c is idim x n and the caller's to destroy (gaamd_ga_live_arrays() rises by exactly one).
   It is created on the sparse array's row cuts: one block of full rows per rank that owns rows
   (sparse.array.c:3669-3696), block k on rank k.  Where every rank owns rows that is
   NGA_Sprs_array_row_distribution's set and every owner writes its rows in place; where idim <
   nproc the array has fewer blocks than ranks, and a rank whose rows lie in another rank's block
   writes them through HBM scratch and NGA_Put's path, complete at the owner before the closing
   sync.  The rule is vec_part's: in place when the rank's own block covers the patch, scratch
   otherwise.  B is needed over the rows of the rank's column span (first column of its first
   non-empty column block to the last of its last) and all n columns: used in place where that
   patch lies in the rank's own block of g_b, else fetched into HBM scratch with NGA_Get's path.
   Where a side goes through scratch the product runs in panels of columns, so that a scratch side
   never holds more than 2^28 bytes (one column at the least); the bits do not change.  A rank
   without rows launches nothing and takes part in the syncs.  gaamd_ga_spmm_route_counts: {B in
   place, B through scratch, C in place, C through scratch}, once per call, on this rank.
   Arithmetic contract: gaamd_spmm's (ga_amd.h) -- c_ij starts from +0 and takes one product and
   one add per entry, never fused, in the order of the row's ONE list over the column blocks; the
   true complex product; integers wrap.  So for a matrix whose duplicates keep their relative
   order the product is the same bits on any number of ranks and under any block map of g_b, and
   for n = 1 it is the matvec of team 1.
     s_b = NGA_Sprs_array_create_from_dense(g_a)          a NEW assembled sparse array
   g_a: rank 2, any type, HBM, any block map; unchanged.  The result has g_a's dimensions and type
   and holds the elements that are != 0 (so not -0.0, but a NaN; complex: either part) and every
   element of the diagonal, zero or not (sparse.array.c:3234, 3263).  Each rank runs
   gaamd_dense_row_counts and gaamd_dense_to_csr on its own block where it lies, copies the CSR of
   the kept elements only to the host and hands them to the assembly above: the result is bit for
   bit what create, add_element of the kept elements and assemble give.  It counts as an assemble
   in the statistics too.
     g_d = NGA_Sprs_array_create_from_sparse(s_a)         a NEW dense idim x jdim array
   on the row cuts under g_c's rule, zeroed, then every non-empty column block scattered by
   gaamd_csr_to_dense; of duplicates of one (i, j) the last in storage order (get_diag's rule).
   The three abort through GA_Error on every rank before the first sync or launch: a handle that
   is not live or not assembled; an array of rank other than 2; a type that differs; g_b with other
   than jdim rows; an array in a host segment.  A rank that would keep 2^31 entries or more ends
   create_from_dense on every rank, after the counting launch and before anything is stored.
   Sparse x sparse (sparse.array.c:2424-3103), collective:
     s_c = NGA_Sprs_array_matmat_multiply(s_a, s_b)       a NEW assembled sparse array C = A B
   of A.idim x B.jdim and the operands' type, on A's row cuts; s_a == s_b is allowed; A and B are
   unchanged; gaamd_ga_live_arrays() is the same before and after the call; C is the caller's to
   destroy.  Structure: C holds exactly one entry for every (i, j) for which some k has a stored
   A(i,k) and a stored B(k,j).  Nothing is dropped for being numerically zero: a product of 0, or a
   sum that cancels, keeps its entry (the reference tests existence, never value).  The entries of a
   row are in ascending column order, the column blocks those of owner(j, B.jdim, nproc), and the
   stored layout is bit for bit what NGA_Sprs_array_create, add_element of C's (i, j, value)
   triples and assemble give: the non-empty block list, the starts, the per-block offset tables,
   jdx, val, the entry counts and the team gaamd_spmv_team(entries of C, idim).  Every call above
   therefore works on C without knowing where it came from.
   Arithmetic contract: gaamd_spgemm_fill's (ga_amd.h) -- c_ij starts from +0 and takes one product
   and then one add per contributing pair, never fused; the order is A's row-i list as ONE list over
   its column blocks ascending, duplicates in storage order, and for each A entry with column k B's
   row-k ONE list in storage order, restricted to column j; the true complex product; integers wrap.
   So C is the same bits on every call and on any rank count whenever the operands' duplicates keep
   their relative order.  One stated departure: the reference ASSIGNS the first product where this
   ADDS it to +0; the two differ only for a lone -0.0 product.  With the +0 start, for finite data
   and a B without duplicates, create_from_sparse(A B) equals
   sprsdns_multiply(A, create_from_sparse(B)) bit for bit.
   How: rank l's row block of B is A's column block l (the same cut rule, B.idim == A.jdim).  Every
   rank flattens its B into a row CSR (gaamd_csr_rows) inside a comex_malloc segment that is freed
   before the call returns; no global array is created.  A rank gathers the parts named by its
   non-empty column blocks of A with comex_get into ONE row CSR in HBM scratch over its column span
   (blocks in between, and parts without entries, give empty rows); where the only part named is
   its own, that part is used where it lies, without a copy (in practice the one-rank route, or a
   block-diagonal A); otherwise its own part is copied into the gathered CSR device to device.
   Then gaamd_spgemm_count, the exchange
   of the ranks' totals, allocation, gaamd_spgemm_fill, and the empty blocks are dropped.  A rank
   without rows launches nothing of these and takes part in every sync.  A LIMIT: a rank may hold a
   copy of all of B (the reference's get_block loop fetches the same); B is not panelled.
   gaamd_ga_spgemm_route_counts: {B parts used in place, B parts copied into the gathered CSR} on
   this rank so far.  The call does not count as an assemble; GA_Print_stats prints the line
   "GA sparse-sparse calls: matmat N" once it has been made.
   It aborts through GA_Error on every rank before the first sync or launch: a handle that is not
   live or not assembled; types that differ; A.jdim != B.idim.  After the counting phase and before
   anything is stored, a rank that would hold 2^31 entries of C or more ends every rank.
   Not provided: the *64 forms, dnssprs_multiply, get_block, get_column (they need the CSR
   persistently remote-readable), export, count_sketch; assembly still sorts on the host. */
int NGA_Sprs_array_create(int idim, int jdim, int type);
void NGA_Sprs_array_add_element(int s_a, int idx, int jdx, void *val);
int NGA_Sprs_array_assemble(int s_a);
int NGA_Sprs_array_destroy(int s_a);
int NGA_Sprs_array_duplicate(int s_a);
void NGA_Sprs_array_row_distribution(int s_a, int iproc, int *lo, int *hi);
void NGA_Sprs_array_column_distribution(int s_a, int iproc, int *lo, int *hi);
void NGA_Sprs_array_col_block_list(int s_a, int **idx, int *n);
void NGA_Sprs_array_access_col_block(int s_a, int icol, int **idx, int **jdx, void **val);
void NGA_Sprs_array_matvec_multiply(int s_a, int g_a, int g_v);
void NGA_Sprs_array_get_diag(int s_a, int *g_d);
void NGA_Sprs_array_shift_diag(int s_a, void *shift);
void NGA_Sprs_array_scale(int s_a, void *scale);
void NGA_Sprs_array_diag_left_multiply(int s_a, int g_d);
void NGA_Sprs_array_diag_right_multiply(int s_a, int g_d);
void gaamd_ga_sprs_range(long dim, int nproc, int iproc, long *lo, long *hi);
void gaamd_ga_sprs_route_counts(long long counts[4]);
int NGA_Sprs_array_sprsdns_multiply(int s_a, int g_b);
int NGA_Sprs_array_create_from_dense(int g_a);
int NGA_Sprs_array_create_from_sparse(int s_a);
void gaamd_ga_spmm_route_counts(long long counts[4]);
int NGA_Sprs_array_matmat_multiply(int s_a, int s_b);
void gaamd_ga_spgemm_route_counts(long long counts[2]);
/* global arrays alive on this rank (temporaries of the general path are destroyed
   before their call returns) */
int gaamd_ga_live_arrays(void);

/* process grid the REGULAR distribution chose, C order (ga.h GA_Get_proc_grid) */
void GA_Get_proc_grid(int g_a, int dims[]);
/* process grid (C order) that NGA_Create picks for npes ranks (restated
 * ddb/ddb_h2 of global/src/decomp.c); host-only, no GPU */
int gaamd_ga_proc_grid(int ndim, const int *dims, const int *chunk, int npes, int *grid);
/* statistics of global/src/onesided.c:1372-1419 (GAstat.numacc, GAbytes.acctot/accloc) */
void GA_Print_stats(void);

#if defined(__cplusplus)
}
#endif

#endif /* GA_AMD_GA_H */
