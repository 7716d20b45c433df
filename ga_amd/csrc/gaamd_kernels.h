// gaamd_kernels.h -- internal interface between the host runtime and the
// gfx950 strided pack/unpack/accumulate kernels (gaamd_kernels.hip).
//
// One descriptor covers every operation on the hot path:
//   * fused strided accumulate   dst[row_d(r)] += scale * src[row_s(r)]
//       (comex_accs self/SMP path, comex.c:6890-6962 -> _acc acc.h:106-154)
//   * pack / unpack / put / get  strided byte copy with either side possibly
//       packed-contiguous (comex.c:1267-1384, 6342-6427, 6617-6696)
//   * unpack-accumulate          packed src -> strided dst with _acc
//       (_acc_packed_handler comex.c:4238-4268)
// A packed buffer is just a strided side whose strides are the running
// products count[0]*count[1]*...; see gaamd_packed_strides().
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "../../include/comex.h"   // COMEX_ACC_*: the element type codes

namespace gaamd {

constexpr int kMaxLevels = 7;       // odometer arrays are int[7] in comex.c:1273
constexpr int kOpCopy = 0;          // byte copy (put/get/pack/unpack)

// q = n / d for 0 <= n < 2^31 with one mul-hi, an add and a shift
// (round-up magic number, Granlund & Montgomery).  Shared host/device.
struct FastDiv {
    uint32_t d, m, s;
    __host__ __device__ inline uint32_t div(uint32_t n) const {
#if defined(__HIP_DEVICE_COMPILE__)
        uint32_t hi = __umulhi(n, m);
#else
        uint32_t hi = (uint32_t)(((uint64_t)n * m) >> 32);
#endif
        return (uint32_t)(((uint64_t)hi + n) >> s);
    }
};
FastDiv make_fastdiv(uint32_t d);

struct alignas(16) Scale16 { uint64_t w[2]; };

struct Desc {
    const char *src;
    char *dst;
    int64_t s_str[kMaxLevels];   // byte stride of level j+1 (stride[j])
    int64_t d_str[kMaxLevels];
    FastDiv cnt[kMaxLevels];     // count[j+1]
    int32_t levels;              // stride_levels in this launch
    uint32_t rows;               // rows covered by this launch
    uint32_t row0;               // global index of the first row
    uint32_t nvec;               // W-byte vectors per row
    FastDiv nvec_div;
    uint32_t chunks;             // row chunks per row (row kernel)
    FastDiv chunk_div;
    uint64_t items;              // work items in this launch
    uint32_t align_mask;         // 2-D rows kernel: chunk alignment of dst (0 = off)
    Scale16 scale;
};

enum KernelKind { KK_AUTO = 0, KK_ROWS = 1, KK_FLAT = 2, KK_SERIAL = 3, KK_ORDERED = 4 };
constexpr int kKinds = 5;

// Run-time knobs.  Only shipped choices remain: the variants rounds 1-2 measured
// as losing (U = 2/4 vectors per thread, 256-thread row blocks, plain instead of
// non-temporal accesses, the looping kernel where the loop-free one applies, the
// 256 x 2 flat shape, 16-byte vectors at misaligned bases -- DESIGN.md §4) are
// no longer compiled; their probes live under tools/.
struct Tuning {
    int kind = KK_AUTO;     // force a kernel family
    int block = 0;          // threads per block of the rows kernels {64, 128}; 0 = auto
    int flat_max_nvec = 127;// rows with at most this many vectors use the flat kernel
    int align = 1;          // 2-D rows kernel: start chunks on chunk-aligned dst addresses (misaligned rows)
    int flat_line_min = 40; // rows off 128 B lines on both sides with at least this many vectors: rows kernel (0 = off)
    // ordered rows sharing bytes only column-wise: 2 (default) column slices, rows loaded by
    // every wave of a workgroup and applied in order from LDS (k_ordered_cols_lds); 1 one lane
    // per column slice loading its own rows (k_ordered_cols); 0 the one-workgroup kernel
    int ordered_cols = 2;
    // io-vectors of at most kIovLdsMax pairs whose destinations may repeat: 1 (default) the
    // one-workgroup LDS kernel, 0 the hashed three-launch path (kept for A/B and fallback)
    int iov_lds = 1;
};
Tuning &tuning();

struct LaunchInfo {
    int kind;      // KernelKind actually used
    int width;     // vector width in bytes
    int unroll;
    int launches;
    uint64_t blocks;
    int block;     // threads per block (rows kernels)
    int levels;    // stride levels after dropping count-1 levels and merging contiguous ones
    int aligned;   // 1: chunk grid shifted to chunk-aligned dst addresses
    int sys;       // 1: source read with system-scope loads (a peer GPU's memory)
};

// Enqueue `op` (kOpCopy or COMEX_ACC_*) over the strided patch.  src/dst
// must be device-accessible.  Returns 0 or a negative error code; never
// touches the host copy of the data.  `info` may be null.
// `src_peer`: src lies in another GPU's HBM (IPC mapping): it is read with
// system-scope loads (gaamd_kernels.hip vload_sys); a geometry whose rows'
// order matters returns kErrPeerOrdered, and the caller packs the rows into
// local memory first.
constexpr int kErrPeerOrdered = -10;
int launch_strided(int op, const void *scale, const void *src, const int *src_stride,
                   void *dst, const int *dst_stride, const int *count, int stride_levels,
                   hipStream_t stream, LaunchInfo *info,
                   uint64_t row_begin = 0, uint64_t row_end = ~0ull, bool plan_only = false,
                   bool src_peer = false);

// byte span [lo, hi) of one side relative to its base pointer
void side_span_host(const int *stride, const int *count, int stride_levels, int64_t row_bytes,
                    int64_t *lo, int64_t *hi);

int elem_size(int op);            // bytes per element for op; 1 for copy; 0 if unknown

// ---- computing on a patch where it lies (gaamd_patch.hip) --------------------
// op = COMEX_ACC_* names the element type; count[] in elements per dimension
// (dimension 0 contiguous), stride[j] = byte stride of dimension j+1, ndim 1..7.
// A count of zero is success without a launch.
constexpr int kPatchMaxLevels = 6;     // row levels of a 7-dimensional patch
constexpr int kPatchErrNdim = -2;      // ndim outside 1..7
constexpr int kPatchErrCount = -3;     // a negative (or missing) count
constexpr int kPatchErrOp = -4;        // not a COMEX_ACC_* type
constexpr int kPatchErrScalar = -5;    // a missing value / alpha / beta / result
constexpr int kPatchErrStride = -6;    // ndim > 1 without strides
constexpr int kPatchErrRange = -7;     // 2^31 rows or more after merging
constexpr int kPatchErrAlign = -8;     // a base or stride below 4-byte alignment
constexpr int kPatchErrOverlap = -11;  // add: c overlaps an input without being exactly it
int launch_patch_fill(int op, const void *value, void *dst, const long long *dst_stride, const long long *count,
                      int ndim, hipStream_t stream);
int launch_patch_scale(int op, const void *alpha, void *dst, const long long *dst_stride, const long long *count,
                       int ndim, hipStream_t stream);
int launch_patch_add(int op, const void *alpha, const void *a, const long long *a_stride, const void *beta,
                     const void *b, const long long *b_stride, void *c, const long long *c_stride,
                     const long long *count, int ndim, hipStream_t stream);
// synchronises `stream` and writes one element to `result` (host)
int launch_patch_dot(int op, const void *a, const long long *a_stride, const void *b, const long long *b_stride,
                     const long long *count, int ndim, void *result, hipStream_t stream);
// element-wise algebra (global/src/elem_alg.c) on the map kernel; fn = GAAMD_ELEM_* (ga_amd.h).
// RECIP and DIV synchronise `stream` and return kPatchZeroDivisor when an element was left
// unwritten because its divisor is zero; the other operations return with the kernel in flight.
enum { kElemAbs = 1, kElemAddConst = 2, kElemRecip = 3, kElemMul = 4, kElemDiv = 5, kElemMax = 6, kElemMin = 7 };
constexpr int kPatchZeroDivisor = 2;
int launch_patch_elem1(int op, int fn, const void *scalar, void *dst, const long long *dst_stride,
                       const long long *count, int ndim, hipStream_t stream);
int launch_patch_elem2(int op, int fn, const void *a, const long long *a_stride, const void *b,
                       const long long *b_stride, void *c, const long long *c_stride, const long long *count,
                       int ndim, hipStream_t stream);
// the minimum (maximum) element of a patch and its linear index (gaamd_select.hip); synchronises
// `stream`; value, key (may be null) and index are host memory.  1 and *index = -1 on a count of zero.
int launch_patch_select(int op, int want_max, const void *a, const long long *a_stride, const long long *count,
                        int ndim, void *value, void *key, long long *index, hipStream_t stream);
// ---- GA's matrix.c calls (gaamd_matrix.hip; ga_amd.h gaamd_patch_norm / _diagonal / _scale_rows / _cols) ----
// the 1-norm (sum of |x|) or infinity norm (max of |x|) of a patch; launch_patch_dot's geometry,
// checks and codes; synchronises `stream`; result (host): one value of the element's type, for
// complex of its real type
enum { kNormOne = 1, kNormInf = 2 };
int launch_patch_norm(int op, int kind, const void *a, const long long *a_stride, const long long *count, int ndim,
                      void *result, hipStream_t stream);
// n elements, element i of the matrix side at a + i * a_step bytes, of the vector side at v + i * v_step
enum { kDiagGet = 1, kDiagSet = 2, kDiagAdd = 3, kDiagShift = 4, kDiagZero = 5 };
int launch_diagonal(int op, int fn, long long n, void *a, long long a_step, void *v, long long v_step,
                    const void *scalar, hipStream_t stream);
// a[i][j] *= v[i] (cols: v[j]) on a row-major rows x ncols matrix, lda in elements; complex part by part
int launch_scale_rc(int op, bool cols, long long rows, long long ncols, void *a, long long lda, const void *v,
                    hipStream_t stream);
// ---- GA's sparse.c calls (gaamd_scan.hip; ga_amd.h gaamd_enum / _scan_tail / _scan / _mask_count / _mask_pack /
// _mask_unpack): contiguous 1-D arrays, n in elements, op the value type and mop the mask type (any two
// COMEX_ACC_* types); the codes are the patch codes above (kPatchErrRange: n above 2^34) ----
enum { kScanCopy = 1, kScanAdd = 2, kScanAddExcl = 3 };
int scan_tile(int op, int mop);   // elements per tile (workgroup), or kPatchErrOp
int scan_agg_span();              // tile aggregates per pass of the aggregate scan's loop
int launch_enum(int op, long long n, long long first, const void *start, const void *stride, void *dst,
                hipStream_t stream);
// synchronises `stream`; has_flag and tail (one element) are host memory
int launch_scan_tail(int op, int fn, int mop, long long n, const void *src, const void *msk, int *has_flag, void *tail,
                     hipStream_t stream);
int launch_scan(int op, int fn, int mop, long long n, const void *src, const void *msk, void *dst, int open,
                const void *carry, hipStream_t stream);
int launch_mask_count(int mop, long long n, const void *msk, long long *count, hipStream_t stream);   // synchronises
// pack (unpack == false): arr = src, other = packed (written); unpack: arr = dst (written), other = packed
int launch_mask_move(bool unpack, int op, int mop, long long n, const void *arr, const void *msk, const void *other,
                     hipStream_t stream);
// ---- GA's sparse arrays (gaamd_sprs.hip; ga_amd.h gaamd_spmv / _sprs_diag / _sprs_scale_left / _right): a block
// CSR in HBM, nblk tables of nrows + 1 offsets (block b's at offs + b * (nrows + 1)) relative to start[b] in
// jdx / val; the codes are the patch codes above (kPatchErrOp also: a team that is no power of two in 1..64) ----
int spmv_team(long long nnz_total, long long rows);
int launch_spmv(int op, long long nrows, int nblk, const int *offs, const long long *start, const int *jdx,
                const void *val, const void *x, long long x_first, void *y, int team, hipStream_t stream);
// one column block; fn = kDiagGet (out[r] = the last stored (r, r)) or kDiagShift (every stored (r, r) += *shift)
int launch_sprs_diag(int op, int fn, long long nrows, const int *offs, const int *jdx, void *val, long long diag_first,
                     void *out, const void *shift, int team, hipStream_t stream);
int launch_sprs_scale_left(int op, long long nrows, const int *offs, void *val, const void *d, int team,
                           hipStream_t stream);
int launch_sprs_scale_right(int op, long long n, const int *jdx, void *val, const void *d, long long d_first,
                            hipStream_t stream);
// ---- sparse x dense and the dense / sparse conversions (gaamd_spmm.hip; ga_amd.h gaamd_spmm / _dense_row_counts /
// _dense_to_csr / _csr_to_dense): the block CSR above, dense sides row-major with ld in elements; the codes are the
// patch codes above (kPatchErrStride an ld below the stored row, kPatchErrOverlap an output on a dense input) ----
int launch_spmm(int op, long long nrows, int nblk, const int *offs, const long long *start, const int *jdx,
                const void *val, const void *b, long long ldb, long long b_first, long long n, void *c, long long ldc,
                hipStream_t stream);
// store == false: counts[r] = the kept elements of row r; true: jdx / val at the prefix sums offs
int launch_dense_csr(int op, long long rows, long long cols, const void *a, long long lda, long long row_first,
                     long long col_first, int *counts, const int *offs, int *jdx, void *val, bool store,
                     hipStream_t stream);
int launch_csr_to_dense(int op, long long nrows, long long cols, const int *offs, const int *jdx, const void *val,
                        long long col_first, void *out, long long ldo, hipStream_t stream);
// ---- sparse x sparse (gaamd_spgemm.hip; ga_amd.h gaamd_csr_rows / _spgemm_count / _spgemm_fill): A the block CSR
// above, B a row CSR (brows + 1 64-bit offsets, jdx, val) of the global rows b_first ..; the codes are the patch codes ----
int spgemm_lds_cap();
int launch_csr_rows(int op, long long nrows, int nblk, const int *offs, const long long *start, const int *jdx,
                    const void *val, long long *roffs, int *rjdx, void *rval, hipStream_t stream);
int launch_spgemm_count(long long nrows, int nblk, const int *offs, const long long *start, const int *jdx,
                        long long b_first, long long brows, const long long *roffs, const int *rjdx, long long jdim_c,
                        int ncut, int *counts, long long *bound, hipStream_t stream);
int launch_spgemm_fill(int op, long long nrows, int nblk, const int *offs, const long long *start, const int *jdx,
                       const void *val, long long b_first, long long brows, const long long *roffs, const int *rjdx,
                       const void *rval, long long jdim_c, int ncut, const int *coffs, const long long *cstart, int *cjdx,
                       void *cval, hipStream_t stream);
struct PatchPlan;
// launch_patch_add's checks without a launch (no device): 0 launch, 1 nothing to do, < 0 error;
// plan[0..3] = {vector width, row levels after merging, rows, vectors per row}
int plan_patch_add(int op, const void *a, const long long *a_stride, const void *b, const long long *b_stride,
                   const void *c, const long long *c_stride, const long long *count, int ndim, long long plan[4],
                   PatchPlan *out = nullptr);
void patch_release();   // comex_finalize: every thread's dot-product scratch (streams idle)

// ---- row-major GEMM on the matrix cores (gaamd_gemm.hip; ga_amd.h gaamd_gemm) ---------
// op = COMEX_ACC_DBL or COMEX_ACC_FLT; ld in elements; the codes are the patch codes above
// (kPatchErrCount a negative extent, kPatchErrOp the op or a trans, kPatchErrScalar,
// kPatchErrStride an ld below the stored row, kPatchErrAlign, kPatchErrOverlap,
// kPatchErrRange 2^31 tiles or more).
constexpr int kGemmTM = 128, kGemmTN = 128, kGemmTK = 16;   // the workgroup's tile of C and its k step
int launch_gemm(int op, int transa, int transb, long long m, long long n, long long k, const void *alpha,
                const void *a, long long lda, const void *b, long long ldb, const void *beta, void *c, long long ldc,
                hipStream_t stream);
// launch_gemm's checks without a launch (no device): 0 launch, 1 nothing to do (m or n is 0),
// < 0 error; plan[0..5] = {tile M, tile N, tile K, tiles along m, tiles along n, k steps}
int plan_gemm(int op, int transa, int transb, long long m, long long n, long long k, const void *alpha,
              const void *a, long long lda, const void *b, long long ldb, const void *beta, const void *c,
              long long ldc, long long plan[6]);

// ---- row-major complex GEMM on the matrix cores (gaamd_gemm_cplx.hip; ga_amd.h gaamd_gemm_cplx) ----
// op = COMEX_ACC_DCP or COMEX_ACC_CPL; trans N T C in either case; ld in complex elements;
// launch_gemm's codes, kPatchErrAlign below the alignment of the element's real part.
// The workgroup's tile of C and its k step, per op (the wave tile is 64 x TN / 2):
constexpr int kCGemmTM = 128;
constexpr int kCGemmTN_DCP = 64, kCGemmTK_DCP = 16;
constexpr int kCGemmTN_CPL = 128, kCGemmTK_CPL = 16;
int launch_gemm_cplx(int op, int transa, int transb, long long m, long long n, long long k, const void *alpha,
                     const void *a, long long lda, const void *b, long long ldb, const void *beta, void *c,
                     long long ldc, hipStream_t stream);
// plan[0..5] as plan_gemm's, with the op's own tile constants
int plan_gemm_cplx(int op, int transa, int transb, long long m, long long n, long long k, const void *alpha,
                   const void *a, long long lda, const void *b, long long ldb, const void *beta, const void *c,
                   long long ldc, long long plan[6]);

// ---- row-major transpose through LDS (gaamd_transpose.hip; ga_amd.h gaamd_transpose) ----
// op: any COMEX_ACC_* type (transpose, for the element size) or DBL / FLT (transpose_acc);
// ld in elements; the codes are the patch codes above, with gaamd_gemm's meanings.
constexpr int kTransposeTile = 64, kTransposeTile16 = 32;   // tile side for 4- / 8-byte and for 16-byte elements
int launch_transpose(int op, long long rows, long long cols, const void *src, long long lds, void *dst, long long ldd,
                     hipStream_t stream);
int launch_transpose_acc(int op, long long m, long long n, const void *alpha, const void *b, long long ldb, void *c,
                         long long ldc, hipStream_t stream);
// launch_transpose's checks without a launch (no device): 0 launch, 1 nothing to do, < 0 error;
// plan[0..3] = {tile rows, tile cols, tiles along rows, tiles along cols}
int plan_transpose(int op, long long rows, long long cols, const void *src, long long lds, const void *dst,
                   long long ldd, long long plan[4]);

// comex_rmw: fetch-and-add (swap == 0) or swap of one 4- or 8-byte word at
// `addr` (device-accessible); the old value lands in *out_dev (8 bytes)
int launch_rmw(int swap, void *addr, int bytes, uint64_t val, uint64_t *out_dev, hipStream_t stream);
// one lane stores v into *flag_dev (pinned host memory) after the stream's earlier work
int launch_flag(uint64_t *flag_dev, uint64_t v, hipStream_t stream);
// segment tags (segments.cpp): the tag of granule g (g * kSegGranule bytes into a
// block) for the block key `key` (granule 0's tag is the key itself)
constexpr uint64_t kSegGranule = 2ull << 20;
__host__ __device__ inline uint64_t seg_granule_tag(uint64_t key, uint32_t g) {
    return key ^ ((uint64_t)g * 0x9E3779B97F4A7C15ull);
}
// where a block's end tag lies: the last 8-byte-aligned word (an aligned 64-bit
// access even when bytes % 8 != 0, e.g. a float block of an odd count)
__host__ __device__ inline uint64_t seg_end_tag_off(uint64_t bytes) { return (bytes - 8) & ~7ull; }
// granule tags of a block of `bytes` (>= 16): every granule whose 8-byte tag ends at
// or before the end tag, so no two tags share a byte (a block of 2 MiB + 12 bytes has
// one granule tag, at 0, and its end tag at 2 MiB)
__host__ __device__ inline uint32_t seg_granule_count(uint64_t bytes) {
    return (uint32_t)((seg_end_tag_off(bytes) - 8) / kSegGranule + 1);
}
// write every granule's tag and the end tag (key_end, at seg_end_tag_off) of a block
int launch_seg_tags(void *p, uint64_t bytes, uint64_t key, uint64_t key_end, hipStream_t stream);
// check them through a mapping (system-scope loads); out_dev[2] (device memory,
// preset {0, ~0u}): mismatches, and the first bad granule (granule count = the end tag)
int launch_seg_check(const void *p, uint64_t bytes, uint64_t key, uint64_t key_end, uint32_t *out_dev,
                     hipStream_t stream);
LaunchInfo *last_launch_info();   // most recent launch_strided (any caller)
unsigned long long kernel_count(int kind);   // launch_strided launches so far, by KernelKind (< kKinds)

// I/O-vector descriptor: n pairs of `bytes`; a side is a device array of n
// addresses (list) or, when the list is null, base + i*bytes (packed)
struct IovDesc {
    const uint64_t *src_list;
    const uint64_t *dst_list;
    const char *src_base;
    char *dst_base;
    int32_t bytes;
    uint32_t n;
    uint32_t nvec, items;   // filled by launch_iov
    FastDiv nvec_div;
    const uint32_t *run_key;   // launch_iov_runs: destinations sorted ((dst - dlo) / bytes)
    const uint32_t *run_perm;  //   and the pair index of each sorted position
};
// `align_or` = OR of every listed address (the launcher cannot read device lists);
// `serial` applies the pairs one by one in order (overlapping destinations)
// `src_peer`: the sources lie in a peer GPU's memory (byte copy only: getv)
int launch_iov(int op, const void *scale, IovDesc d, uint64_t align_or, bool serial, hipStream_t stream,
               bool src_peer = false);
// Pairs whose destinations may repeat (GA scatter-accumulate with repeated
// subscripts), without a host-side overlap check: the destinations are sorted on
// the GPU (stable radix sort of (dst - dlo) / bytes, so equal destinations keep
// their input order) and one lane per distinct destination applies its pairs in
// input order -- the reference's pair order wherever it matters.  Requires a
// device dst list, every dst - dlo a multiple of d.bytes, iov_units_ok(units),
// d.bytes <= kIovRunsMaxBytes, and no source inside a destination.
constexpr int kIovRunsMaxBytes = 256;
// `units` of every GPU-ordered launcher: the slots of d.bytes from dlo up to the end of
// the highest destination, so the 32-bit sort keys (dst - dlo) / bytes are 0 .. units - 1.
// The key 0xffffffff is kIovRunSkip, the mark of the masked passes for "this pair was
// applied already", and k_iov_runs skips it on every route: units < kIovRunSkip is the
// one limit, the same for the classification (iov.cpp, the requester and the owner in
// remote.cpp) and for launch_iov_runs / _hashed / _lds, masked or not.  From 0xffffffff
// units up the callers take the host-checked plain or serial kernel.
constexpr uint32_t kIovRunSkip = 0xffffffffu;
// dend: one past the last byte of the highest destination
inline uint64_t iov_units(uint64_t dlo, uint64_t dend, int bytes) { return (dend - dlo) / (uint64_t)bytes; }
inline bool iov_units_ok(uint64_t units) { return units < (uint64_t)kIovRunSkip; }
size_t iov_runs_work_bytes(uint32_t n);
struct IovPartState;   // the partitioned path's deferred overflow (below)
struct IovHash;   // the hashed path's table (one per calling thread; kept across calls)
// mask: the table of a hashed launch whose conflicts overflowed (iov_hash_overflowed):
// the pairs it applied already are skipped
int launch_iov_runs(int op, const void *scale, IovDesc d, uint64_t align_or, uint64_t dlo, uint64_t units,
                    void *work, size_t work_bytes, hipStream_t stream, bool src_peer = false,
                    const IovHash *mask = nullptr, const IovPartState *pmask = nullptr);
// The same contract as launch_iov_runs without the sort for up to 2^19 pairs: a
// hash table finds the destinations with more than one pair; pairs alone on
// theirs are applied at once, the rest (up to 8192) sorted by (destination,
// index) in one workgroup's LDS and applied in index order.  Returns 1 when n is
// outside its range (use launch_iov_runs).  After the stream has completed the
// launch, iov_hash_overflowed(h) true means more conflicting pairs than the LDS
// holds: none of those was applied -- run launch_iov_runs(..., mask = h) next.
// The caller serialises its launches on one IovHash (the table is reused).
// dst_in / src_in (optional, device-mapped pinned memory): the lists not yet in HBM --
// the first kernel copies them to d.dst_list / d.src_list on its way (no upload launch);
// when this returns 1 nothing was launched and the caller uploads them itself.
IovHash *iov_hash_create();
int launch_iov_hashed(IovHash *h, int op, const void *scale, IovDesc d, uint64_t align_or, uint64_t dlo,
                      uint64_t units, hipStream_t stream, bool src_peer = false, const uint64_t *dst_in = nullptr,
                      const uint64_t *src_in = nullptr);
bool iov_hash_overflowed(const IovHash *h);
// The same contract with the ordering held in LDS; d.dst_list / d.src_list may point
// into mapped pinned memory (read once).  Below kIovLdsRoute pairs, or without scratch,
// ONE launch of one workgroup (k_iov_lds, up to kIovLdsMax pairs); from kIovLdsRoute
// to kIovPartMax pairs with `scratch` (HBM, iov_lds_scratch_bytes(n)), two launches:
// the keys into hash-partition buckets (k_iov_keyof), then one workgroup per partition
// orders and applies its pairs (k_iov_part).  Returns 1 when n is outside its range.
// Calls from one thread must be ordered (each completes before the next starts): the
// partition counters are per thread and zero between calls.
// A partition of more than its bucket's pairs (heavy repeats) is done in windows of the
// input by its workgroup: n / 1024 windows, so only up to kIovPartWindowMax pairs.  Larger
// calls pass `defer` with a mapped pinned flag: such partitions are then left untouched
// (counters kept), the flag raised, and after the stream completed the caller applies
// them with launch_iov_runs(..., pmask = defer) (which zeroes the counters again).
struct IovPartState {
    uint32_t *flag_dev = nullptr;   // in: device view of a zeroed mapped pinned word
    uint32_t *counts = nullptr;     // out: the call's partition counters
    uint32_t lg = 0;                // out: log2 of its partitions
};
constexpr uint32_t kIovPartWindowMax = 1u << 16;
void iov_part_release();   // comex_finalize: the partition counters (streams idle)
constexpr uint32_t kIovLdsMax = 16384;
constexpr uint32_t kIovLdsRoute = 1024;
constexpr uint32_t kIovPartMax = 1u << 22;
size_t iov_lds_scratch_bytes(uint32_t n);   // keys and partition buckets (~68 B a pair)
int launch_iov_lds(int op, const void *scale, IovDesc d, uint64_t align_or, uint64_t dlo, uint64_t units,
                   hipStream_t stream, bool src_peer = false, void *scratch = nullptr,
                   IovPartState *defer = nullptr);

}  // namespace gaamd
