"""One rank, kernel level: every kernel family at byte offsets past 2^31 and 2^32 from its
base (and, for 4-byte elements, at element indices past 2^31), bit-exact.

The rest of the suite checks the same kernels inside buffers of a few MiB, where a 32-bit
offset and a 64-bit one are the same number.  Here one operand at a time is FAR: its rows
lie up to 9 GiB from its base (io-vector destinations up to 16 GiB), the other operands
are compact.  Nothing of that size is ever copied: a `Sparse` image keeps the extents a
case touches -- the rows, and canaries that must come back unchanged:

  * 256 bytes before and after every row;
  * for every row piece past 2^32 from its base the same bytes at (offset mod 2^32), and
    for every piece past 2^31 those at (offset - 2^31): where a kernel that narrowed an
    offset to 32 or 31 bits would read or write instead.  They hold random bytes of their
    own, so a wrapped read changes the result and a wrapped write is reported as "canary
    at wrapped offset ... changed" and not only as wrong data;

and uploads, downloads and compares exactly those.  All of it lies in ONE allocation of
16 GiB + 1 MiB (module scope): the far operand from +4096, the compact operands from
12 GiB on, in disjoint spans.

test_checker_flags_truncated_offsets (no GPU) runs a numpy model kernel through the same
checker over every geometry the GPU tests use -- with 64-bit offsets (must pass), with
offsets truncated to uint32 and to int32 (both must be flagged; an int32 offset that falls
before the buffer is a dropped access) -- so the file shows that it would catch the bug
without a broken kernel on a GPU.

References: the oracle on the same rows at a compact stride (strided, pack / unpack,
io-vectors: the same row or pair order, so the same bits); the ref_* restatements of
test_gpu_ga_math.py (patch kernels); the int64 product (gemm, integer data); numpy
(transposes).  No tolerance anywhere.
"""
import bisect
import ctypes

import numpy as np
import pytest

import cases as C
import ga_amd
from helpers import _giov
from test_gpu_ga_math import ALPHA, BETA, VALUE, gen, ref_add, ref_dot_exact, ref_fill, ref_scale
from test_gpu_iov_fuzz import (HASH_CAP, HASH_MAX_PAIRS, PART_CAP, PART_MAX, PART_WINDOW_MAX, PATHS, RUNS_MIN,
                               part_lg, part_of)

INT, DBL, FLT, DCP, LNG = C.INT, C.DBL, C.FLT, C.DCP, C.LNG
COPY = ga_amd.GAAMD_OP_COPY
DT = ga_amd.OP_DTYPE
G = 1 << 30
B31, B32 = 1 << 31, 1 << 32
ALLOC = 16 * G + (1 << 20)      # the one allocation: the most this file holds at a time
FAR = 4096                      # the far operand's region starts here (+0, +4 or +8)
COMPACT = (12 * G, 13 * G, 14 * G)   # the compact operands' regions
IOV_SRC = 16 * G + (64 << 10)   # io-vector sources: after the 16 GiB + 64 KiB of destinations
CANARY = 256
UNITS_LIMIT = 0xFFFFFFFF        # kIovRunSkip: the GPU-ordered routes take units < this


# ---------------------------------------------------------------------------------------
# the sparse image
def pieces_at_boundaries(off, n):
    """[off, off + n) cut at the multiples of 2^31"""
    out, a = [], off
    while a < off + n:
        b = min(off + n, (a // B31 + 1) * B31)
        out.append((a, b - a))
        a = b
    return out


class Sparse:
    """The extents of one (far) allocation that a case touches: what was uploaded, what is
    expected afterwards, and a comparison that downloads exactly those extents.
    `dev` has upload(arr, offset) / download(dtype, count, offset) / nbytes."""

    def __init__(self, dev, seed):
        self.dev = dev
        self.rng = np.random.default_rng(seed)
        self.items = []          # [offset, uploaded bytes, expected bytes, label]
        self.asks = []           # canaries wanted around the rows: (offset, n, label)
        self.wrapped = []        # and at the wrapped offsets: these get their bytes first
        self.starts, self.ends = [], []
        self.chunks = None

    def rows(self, base, offs, data, label):
        """rows of data.shape[1] bytes at base + offs[i]; returns a handle for expect()"""
        data = np.ascontiguousarray(data).view(np.uint8).reshape(len(offs), -1)
        n = data.shape[1]
        first = len(self.items)
        for o, d in zip(offs, data):
            o = int(o)
            self.items.append([base + o, d.copy(), d.copy(), f"row of {label}"])
            self.asks.append((base + o - CANARY, CANARY, f"canary before a row of {label}"))
            self.asks.append((base + o + n, CANARY, f"canary after a row of {label}"))
            for a, m in pieces_at_boundaries(o, n):
                if a >= B32:
                    self.wrapped.append((base + a % B32, m, f"canary at wrapped offset (mod 2^32) of {label}"))
                if a >= B31:
                    self.wrapped.append((base + a - B31, m, f"canary at wrapped offset (- 2^31) of {label}"))
        return range(first, len(self.items))

    def expect(self, handle, want):
        want = np.ascontiguousarray(want).view(np.uint8).reshape(len(handle), -1)
        for i, w in zip(handle, want):
            assert w.size == self.items[i][1].size
            self.items[i][2] = w.copy()

    def _uncovered(self, a, b):
        out = []
        i = bisect.bisect_right(self.starts, a) - 1
        if i >= 0 and self.ends[i] > a:
            a = self.ends[i]
        i += 1
        while a < b and i < len(self.starts) and self.starts[i] < b:
            if self.starts[i] > a:
                out.append((a, self.starts[i]))
            a = max(a, self.ends[i])
            i += 1
        if a < b:
            out.append((a, b))
        return out

    def _cover(self, a, b):
        i = bisect.bisect_left(self.starts, a)
        self.starts.insert(i, a)
        self.ends.insert(i, b)

    def seal(self):
        """the rows are all known: the canaries take what the rows left free (clipped to the
        allocation), then everything goes up, contiguous extents in one copy"""
        for off, d, _, label in self.items:
            assert 0 <= off and off + d.size <= self.dev.nbytes, (label, off)
            assert self._uncovered(off, off + d.size) == [(off, off + d.size)], f"{label} at {off:#x} overlaps another"
            self._cover(off, off + d.size)
        first = len(self.items)
        for off, n, label in self.wrapped + self.asks:
            for a, b in self._uncovered(max(0, off), min(self.dev.nbytes, off + n)):
                self.items.append([a, b - a, None, label])
                self._cover(a, b)
        junk = self.rng.integers(0, 256, sum(it[1] for it in self.items[first:]), dtype=np.uint8)
        p = 0
        for it in self.items[first:]:
            it[1] = it[2] = junk[p:p + it[1]]
            p += it[1].size
        order = sorted(range(len(self.items)), key=lambda i: self.items[i][0])
        self.chunks = []
        for i in order:
            off, d = self.items[i][0], self.items[i][1]
            if self.chunks and self.chunks[-1][0] + self.chunks[-1][1] == off:
                self.chunks[-1][1] += d.size
                self.chunks[-1][2].append(i)
            else:
                self.chunks.append([off, d.size, [i]])
        for off, n, idx in self.chunks:
            self.dev.upload(np.concatenate([self.items[i][1] for i in idx]), offset=off)
        return self

    def check(self):
        """downloads exactly the extents; the list of what differs (empty: all as expected)"""
        bad = []
        for off, n, idx in self.chunks:
            got = self.dev.download(np.uint8, n, offset=off)
            p = 0
            for i in idx:
                o, d, want, label = self.items[i]
                if not np.array_equal(got[p:p + d.size], want):
                    bad.append(f"{label} at offset {o:#x} " + ("holds wrong data" if label.startswith("row") else "changed"))
                p += d.size
        return bad


def assert_clean(img, what):
    bad = img.check()
    assert not bad, (what, len(bad), bad[:6])


# ---------------------------------------------------------------------------------------
# geometries: the far operand's rows, shared by the GPU tests and the checker's self-test
class Geo:
    def __init__(self, name, offs, row, base=FAR, compact=COMPACT[0]):
        self.name, self.offs, self.row, self.base = name, [int(o) for o in offs], int(row), base
        self.compact = compact      # where the self-test's model puts the other operand


def level_offsets(strides, counts):
    """row offsets of a strided patch in the reference's odometer order (level 1 fastest)"""
    offs = [0]
    for s, c in zip(strides, counts):
        offs = [o + j * s for j in range(c) for o in offs]
    return offs


STRIDED_LEVELS = (([G + 64], [5]), ([G + 64, B31 - 16], [3, 3]))
ROW_FLAT, ROW_ROWS = 48, (40 << 10) + 16
COLRED_ROW = (4 << 10) + 16


def strided_geos():
    """(geo, strides, counts): one and two levels; 48-byte rows everywhere, 40 KiB + 16 rows
    on one level (on two, rows of that length at these strides would overlap each other)"""
    out = []
    for strides, counts in STRIDED_LEVELS:
        for row in (ROW_FLAT, ROW_ROWS) if len(counts) == 1 else (ROW_FLAT,):
            for off in (0, 8):
                g = Geo(f"strided{len(counts)}-row{row}+{off}", level_offsets(strides, counts), row, FAR + off)
                out.append((g, strides, counts))
    return out


def colred_geos():
    return [Geo(f"colred+{off}", level_offsets([G + 64], [5]), COLRED_ROW, FAR + off) for off in (0, 8)]


PATCH_SHAPES = (([17, 3], [B31 + 48]), ([17, 2, 3], [G + 16, B31 + 48]))
PATCH_OPS = (DBL, FLT, DCP)


def patch_geos(op):
    out = []
    for count, stride in PATCH_SHAPES:
        for off in ((0, 4) if op == FLT else (0,)):
            g = Geo(f"patch-{C.NAMES[op]}-{len(count)}d+{off}", level_offsets(stride, count[1:]),
                    count[0] * C.ESZ[op], FAR + off)
            out.append((g, count, stride))
    return out


FAR_SPAN = 9 * G                # two of 17 rows past byte 2^33, element 2^31 of a 4-byte type


def far_ld(rows, esz, vec):
    """a leading dimension (elements) that spreads `rows` rows over FAR_SPAN: odd, or a
    multiple of 16 bytes"""
    ld = -(-FAR_SPAN // ((rows - 1) * esz))
    if vec:
        per = max(1, 16 // esz)
        return -(-ld // per) * per
    return ld | 1


def mat_geo(name, rows, cols, esz, vec, base=FAR):
    ld = far_ld(rows, esz, vec)
    g = Geo(f"{name}-{rows}x{cols}x{esz}B-{'vec' if vec else 'odd'}", [i * ld * esz for i in range(rows)], cols * esz, base)
    g.ld = ld
    return g


def gemm_tiles():
    rc, p = ga_amd.gemm_plan(DBL, "N", "N", 1, 1, 1, 1.0, 1 << 40, 1, 2 << 40, 1, 1.0, 3 << 40, 1)
    assert rc == 0
    return p["tm"], p["tn"], p["tk"]


def transpose_tile(op):
    rc, p = ga_amd.transpose_plan(op, 1, 1, 1 << 40, 1, 2 << 40, 1)
    assert rc == 0 and p["tile_rows"] == p["tile_cols"]
    return p["tile_rows"]


def stored_shape(which, ta, tb, m, n, k):
    """rows x cols of an operand as it lies in memory"""
    if which == "A":
        return (m, k) if ta == "N" else (k, m)
    if which == "B":
        return (k, n) if tb == "N" else (n, k)
    return (m, n)


def gemm_geos():
    tm, tn, tk = gemm_tiles()
    m, n, k = tm + 1, tn + 1, tk + 1
    out = {}
    for esz in (8, 4):
        for shape in {(m, k), (k, m), (k, n), (n, k), (m, n)}:
            for vec in (False, True):
                out[(esz,) + shape + (vec,)] = mat_geo("gemm", shape[0], shape[1], esz, vec)
    return out


def transpose_geos():
    out = {}
    for op in (INT, DBL, DCP, FLT):
        t = transpose_tile(op)
        for vec in (False, True):
            out[(C.ESZ[op], t + 1, vec)] = mat_geo("transpose", t + 1, t + 1, C.ESZ[op], vec)
    return out


def iov_keys(case):
    """the destination keys (slots of the pair size from the lowest destination) of one
    io-vector case, in pair order; both end destinations are repeated"""
    kind, n, units, seed = case
    rng = np.random.default_rng(seed)
    last = units - 1
    if kind == "deferred":                      # 65537 pairs on 400 slots + 1500 on the last
        slots = np.concatenate([[0, last], rng.integers(1, last, 398, dtype=np.uint64)]).astype(np.uint64)
        keys = np.concatenate([slots, slots[rng.integers(0, 400, 65537 - 400)], np.full(1500, last, dtype=np.uint64)])
    else:
        mid = np.unique(rng.integers(1, last, 150, dtype=np.uint64))   # many pairs a destination
        keys = np.concatenate([mid, mid[rng.integers(0, mid.size, n - 6 - mid.size)],
                               np.zeros(3, dtype=np.uint64), np.full(3, last, dtype=np.uint64)])
    keys = keys[rng.permutation(keys.size)].astype(np.uint64)
    assert keys.size == n and int(keys.min()) == 0 and int(keys.max()) == last
    return keys


# (name, op, n pairs, units, seed)
IOV_SMALL = [("small", INT, 1000, 2 * G + 12345, 1), ("small", DBL, 1000, G + 999, 2)]
IOV_UNITS = [("units", INT, n, u, 10 + i) for i, (n, u) in enumerate(
    (n, u) for n in (2048, 4096) for u in (UNITS_LIMIT - 1, UNITS_LIMIT, B32))]
IOV_DEFERRED = [("deferred", INT, 65537 + 1500, UNITS_LIMIT - 1, 20)]
IOV_BIT31 = [("bit31", DBL, 2048, B31, 21)]
IOV_CASES = IOV_SMALL + IOV_UNITS + IOV_DEFERRED + IOV_BIT31


def iov_id(c):
    return f"{c[0]}-{C.NAMES[c[1]]}-{c[2]}-{c[3]:#x}"


def iov_geo(case):
    name, op, n, units, seed = case
    keys = iov_keys((name, n, units, seed))
    uniq, inv = np.unique(keys, return_inverse=True)
    g = Geo("iov-" + iov_id(case), [int(u) * C.ESZ[op] for u in uniq], C.ESZ[op], base=0, compact=IOV_SRC)
    g.keys, g.inv = keys, inv
    return g


def all_geos():
    out = [g for g, _, _ in strided_geos()] + colred_geos()
    for op in PATCH_OPS:
        out += [g for g, _, _ in patch_geos(op)]
    out += list(gemm_geos().values()) + list(transpose_geos().values())
    out += [iov_geo(c) for c in IOV_CASES]
    return out


# ---------------------------------------------------------------------------------------
# the checker's self-test (no GPU)
class FakeDevice:
    """a sparse stand-in for the allocation: pages made on first touch, holding junk that
    depends on the page alone (a read of untouched memory returns some other data)"""
    PAGE = 1 << 12

    def __init__(self, nbytes):
        self.nbytes, self.ptr, self.pages = nbytes, 0, {}

    def _spans(self, off, n):
        while n > 0:
            p, o = divmod(off, self.PAGE)
            if p not in self.pages:
                self.pages[p] = np.random.default_rng(p).integers(0, 256, self.PAGE, dtype=np.uint8)
            m = min(n, self.PAGE - o)
            yield self.pages[p], o, m
            off, n = off + m, n - m

    def upload(self, arr, offset=0):
        b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        assert 0 <= offset and offset + b.size <= self.nbytes
        p = 0
        for page, o, m in self._spans(offset, b.size):
            page[o:o + m] = b[p:p + m]
            p += m

    def download(self, dtype, count, offset=0):
        n = np.dtype(dtype).itemsize * count
        assert 0 <= offset and offset + n <= self.nbytes
        return np.concatenate([page[o:o + m] for page, o, m in self._spans(offset, n)]).view(dtype)


def as_u64(o):
    return o


def as_u32(o):
    return o & 0xFFFFFFFF


def as_i32(o):
    return ((o & 0xFFFFFFFF) ^ B31) - B31


def model_kernel(dev, sbase, soffs, dbase, doffs, row, narrow):
    """dst row i = src row i ^ 0x5A, every row offset through `narrow` first; an access that
    falls before the allocation is dropped"""
    for so, do in zip(soffs, doffs):
        s, d = sbase + narrow(so), dbase + narrow(do)
        if s < 0 or d < 0:
            continue
        dev.upload(dev.download(np.uint8, row, offset=s) ^ np.uint8(0x5A), offset=d)


def model_case(geo, far_is_dst, narrow, seed=0):
    dev = FakeDevice(ALLOC)
    img = Sparse(dev, seed)
    rng = np.random.default_rng(seed + 1)
    n = len(geo.offs)
    coffs = [i * (geo.row + 16) for i in range(n)]
    far = img.rows(geo.base, geo.offs, rng.integers(0, 256, (n, geo.row), dtype=np.uint8), "the far operand")
    src = rng.integers(0, 256, (n, geo.row), dtype=np.uint8)
    com = img.rows(geo.compact, coffs, src, "the compact operand")
    if far_is_dst:
        img.expect(far, src ^ np.uint8(0x5A))
    else:
        img.expect(com, np.stack([img.items[i][1] for i in far]) ^ np.uint8(0x5A))
    img.seal()
    if far_is_dst:
        model_kernel(dev, geo.compact, coffs, geo.base, geo.offs, geo.row, narrow)
    else:
        model_kernel(dev, geo.base, geo.offs, geo.compact, coffs, geo.row, narrow)
    return img.check()


def test_geometries_cross_the_boundaries_mid_patch():
    """every geometry has rows on both sides of byte 2^31 and of byte 2^32 -- where the
    leading dimension or the destinations are this file's choice, more than the last row
    past each -- and the 4-byte gemm and transpose operands pass element 2^31"""
    for g in all_geos():
        o = sorted(g.offs)
        assert o[0] < B31, g.name
        for edge in (B31, B32):
            past = [x for x in o if x + g.row > edge]
            chosen = g.name.startswith(("gemm", "transpose", "iov"))   # the rest: strides the issue fixed
            assert (2 if chosen else 1) <= len(past) < len(o), (g.name, edge)
        if g.name.startswith(("gemm", "transpose")) and "x4B" in g.name:
            assert sum(x >= (1 << 33) for x in o) >= 2, g.name
        assert g.base + o[-1] + g.row + CANARY <= (COMPACT[0] if g.base else IOV_SRC), g.name


FAMILIES = {"strided": 6, "colred": 2, "patch": 8, "gemm": 12, "transpose": 6, "iov": len(IOV_CASES)}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_checker_flags_truncated_offsets(family):
    geos = [g for g in all_geos() if g.name.startswith(family)]
    assert len(geos) == FAMILIES[family]
    for g in geos:
        for far_is_dst in (True, False):
            what = (g.name, "far dst" if far_is_dst else "far src")
            assert model_case(g, far_is_dst, as_u64) == [], what
            bad32 = model_case(g, far_is_dst, as_u32)
            assert bad32, (what, "offsets truncated to uint32 went unnoticed")
            if far_is_dst:
                assert any("canary at wrapped offset (mod 2^32)" in b for b in bad32), (what, bad32[:4])
            assert model_case(g, far_is_dst, as_i32), (what, "offsets truncated to int32 went unnoticed")


# ---------------------------------------------------------------------------------------
# GPU
@pytest.fixture(scope="module")
def far(gpu_lib):
    """the one allocation; a failure to get it is a failure of the test"""
    dev = ga_amd.DeviceBuffer(ALLOC)
    assert dev.ptr % 256 == 0
    yield dev
    dev.free()


def typed_rows(op, n, row, seed):
    """n rows of valid elements of op's type (no NaN by construction)"""
    return np.stack([C.fill_bytes(op if op != COPY else DBL, row, seed + i) for i in range(n)])


def compact_offs(n, row):
    return [i * row for i in range(n)]


class Knob:
    def __init__(self, key, val):
        self.key, self.val = key, val

    def __enter__(self):
        self.old = ga_amd.set_tuning(self.key, self.val)

    def __exit__(self, *exc):
        ga_amd.set_tuning(self.key, self.old)


def strided_case(far, oracle, geo, strides, counts, op, far_dst, kind, seed):
    n, row = len(geo.offs), geo.row
    img = Sparse(far, seed)
    off = geo.base - FAR
    cbase = COMPACT[0] + off
    fdata, cdata = typed_rows(op, n, row, seed), typed_rows(op, n, row, seed + 100)
    fh = img.rows(geo.base, geo.offs, fdata, "the far side")
    ch = img.rows(cbase, compact_offs(n, row), cdata, "the compact side")
    src, dst = (cdata, fdata) if far_dst else (fdata, cdata)
    want = dst.copy()
    if op == COPY:
        want[:] = src
    else:
        oracle.accs(op, C.SCALE[op], np.ascontiguousarray(src), 0, [row], want, 0, [row], [row, n], 1)
    img.expect(fh if far_dst else ch, want)
    img.seal()
    cstr = [row * int(np.prod(counts[:j], dtype=np.int64)) for j in range(len(counts))]
    sp, ss, dp, ds = ((far.ptr + cbase, cstr, far.ptr + geo.base, strides) if far_dst
                      else (far.ptr + geo.base, strides, far.ptr + cbase, cstr))
    with Knob("kind", kind):
        ga_amd.strided(op, C.SCALE.get(op), sp, ss, dp, ds, [row] + list(counts), len(counts))
        launched = ga_amd.last_launch()["kind"]
    ga_amd.sync()
    assert_clean(img, (geo.name, C.NAMES.get(op, "copy"), "far dst" if far_dst else "far src", launched))
    return launched


@pytest.mark.gpu
@pytest.mark.parametrize("far_dst", [True, False], ids=["far-dst", "far-src"])
@pytest.mark.parametrize("op", [INT, DBL, DCP, COPY], ids=["int", "dbl", "dcp", "copy"])
def test_strided_far(gpu_lib, oracle, far, op, far_dst):
    seen = set()
    for i, (geo, strides, counts) in enumerate(strided_geos()):
        # the launcher's own choice (FLAT for 48-byte rows, ROWS for 40 KiB + 16), then both forced
        for kind in (0, 1, 2):
            launched = strided_case(far, oracle, geo, strides, counts, op, far_dst, kind, 1000 * op + 10 * i + kind)
            seen.add((len(counts), launched))
            if kind:
                assert launched == ga_amd.KIND_NAME[kind], (geo.name, kind, launched)
    assert {(1, "flat"), (1, "rows"), (2, "flat"), (2, "rows")} <= seen, seen


@pytest.mark.gpu
@pytest.mark.parametrize("op,off,width", [(LNG, 0, 16), (LNG, 8, 8), (DBL, 0, 8)],
                         ids=["lng-sum-atomic", "lng-rows-atomic", "dbl-lds"])
def test_column_reduction_of_far_rows(gpu_lib, oracle, far, op, off, width):
    """a zero dst stride: 5 far rows of 4 KiB + 16 summed into one compact row.  int64 into
    a destination in HBM adds partial sums atomically: 16-byte columns summed in LDS first
    when the source rows lie on 16 bytes (k_cols_sum), elements (k_cols_atomic) at base + 8;
    f64 keeps the reference's order a column, rows staged through LDS.  The vector width
    of the launch tells the first two apart."""
    geo = colred_geos()[off // 8]
    n, row = len(geo.offs), geo.row
    img = Sparse(far, 77 + op)
    src = typed_rows(op, n, row, 300 + op)
    dst = typed_rows(op, 1, row, 400 + op)
    img.rows(geo.base, geo.offs, src, "the far source rows")
    dh = img.rows(COMPACT[0], [0], dst, "the destination row")
    want = dst.copy()
    oracle.accs(op, C.SCALE[op], np.ascontiguousarray(src), 0, [row], want, 0, [0], [row, n], 1)
    img.expect(dh, want)
    img.seal()
    ga_amd.strided(op, C.SCALE[op], far.ptr + geo.base, [G + 64], far.ptr + COMPACT[0], [0], [row, n], 1)
    info = ga_amd.last_launch()
    assert info["kind"] == "ordered" and info["width"] == width, info
    ga_amd.sync()
    assert_clean(img, (geo.name, C.NAMES[op]))


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["pack", "unpack", "unpack_acc"])
def test_pack_unpack_far(gpu_lib, oracle, far, what):
    op = DBL
    for i, (geo, strides, counts) in enumerate(strided_geos()):
        n, row = len(geo.offs), geo.row
        img = Sparse(far, 500 + i)
        fdata = typed_rows(op, n, row, 600 + 10 * i)
        packed = typed_rows(op, 1, n * row, 700 + i)
        fh = img.rows(geo.base, geo.offs, fdata, "the strided side")
        ph = img.rows(COMPACT[0], [0], packed, "the packed side")
        count = [row] + list(counts)
        if what == "pack":
            img.expect(ph, fdata.reshape(1, -1))
        elif what == "unpack":
            img.expect(fh, packed.reshape(n, row))
        else:
            want = np.ascontiguousarray(fdata)
            oracle.unpack_acc(op, C.SCALE[op], np.ascontiguousarray(packed.reshape(-1)), want, 0, [row], [row, n], 1)
            img.expect(fh, want)
        img.seal()
        if what == "pack":
            ga_amd.pack(far.ptr + geo.base, strides, count, len(counts), far.ptr + COMPACT[0])
        elif what == "unpack":
            ga_amd.unpack(far.ptr + COMPACT[0], far.ptr + geo.base, strides, count, len(counts))
        else:
            ga_amd.unpack_acc(op, C.SCALE[op], far.ptr + COMPACT[0], far.ptr + geo.base, strides, count, len(counts))
        ga_amd.sync()
        assert_clean(img, (what, geo.name))


# ---- gaamd_patch_* ---------------------------------------------------------------------
def patch_operands(far, geo, count, stride, op, which_far, names, rng, seed, small=None):
    """operands `names`, the one named which_far on the far geometry, the others compact with
    tight strides; returns (image, {name: (pointer, strides, handle, values (rows, count[0]))})"""
    n, per = len(geo.offs), count[0]
    esz = C.ESZ[op]
    img = Sparse(far, seed)
    tight = [per * esz * int(np.prod(count[1:d], dtype=np.int64)) for d in range(1, len(count))]
    out = {}
    zone = iter(COMPACT)
    for name in names:
        vals = gen(op, n * per, rng, small).reshape(n, per)
        if name == which_far:
            base, offs, st = geo.base, geo.offs, stride
        else:
            base, offs, st = next(zone) + (geo.base - FAR), compact_offs(n, per * esz), tight
        h = img.rows(base, offs, vals, f"operand {name}" + (" (far)" if name == which_far else ""))
        out[name] = (far.ptr + base, st, h, vals)
    return img, out


@pytest.mark.gpu
@pytest.mark.parametrize("op", PATCH_OPS, ids=lambda o: C.NAMES[o])
def test_patch_fill_scale_far(gpu_lib, far, op):
    rng = np.random.default_rng(31 + op)
    for i, (geo, count, stride) in enumerate(patch_geos(op)):
        for kernel in ("fill", "scale"):
            img, ops = patch_operands(far, geo, count, stride, op, "c", "c", rng, 40 + i)
            p, st, h, vals = ops["c"]
            if kernel == "fill":
                img.expect(h, ref_fill(op, vals.size, VALUE[op]))
            else:
                img.expect(h, ref_scale(op, vals.reshape(-1), ALPHA[op]))
            img.seal()
            if kernel == "fill":
                assert ga_amd.patch_fill(op, VALUE[op], p, st, count) == 0
            else:
                assert ga_amd.patch_scale(op, ALPHA[op], p, st, count) == 0
            ga_amd.sync()
            assert_clean(img, (kernel, geo.name))


@pytest.mark.gpu
@pytest.mark.parametrize("which_far", ["a", "b", "c"])
@pytest.mark.parametrize("op", PATCH_OPS, ids=lambda o: C.NAMES[o])
def test_patch_add_far(gpu_lib, far, op, which_far):
    rng = np.random.default_rng(53 + op)
    for i, (geo, count, stride) in enumerate(patch_geos(op)):
        img, ops = patch_operands(far, geo, count, stride, op, which_far, "abc", rng, 60 + i)
        (pa, sa, _, a), (pb, sb, _, b), (pc, sc, hc, _) = ops["a"], ops["b"], ops["c"]
        img.expect(hc, ref_add(op, ALPHA[op], a.reshape(-1), BETA[op], b.reshape(-1)))
        img.seal()
        assert ga_amd.patch_add(op, ALPHA[op], pa, sa, BETA[op], pb, sb, pc, sc, count) == 0
        ga_amd.sync()
        assert_clean(img, ("add", which_far, geo.name))


@pytest.mark.gpu
@pytest.mark.parametrize("which_far", ["a", "b"])
@pytest.mark.parametrize("op", PATCH_OPS, ids=lambda o: C.NAMES[o])
def test_patch_dot_far(gpu_lib, far, op, which_far):
    """integer-valued data: every order of the sum gives the same bits"""
    rng = np.random.default_rng(71 + op)
    for i, (geo, count, stride) in enumerate(patch_geos(op)):
        img, ops = patch_operands(far, geo, count, stride, op, which_far, "ab", rng, 80 + i, small=4)
        (pa, sa, _, a), (pb, sb, _, b) = ops["a"], ops["b"]
        img.seal()
        rc, got = ga_amd.patch_dot(op, pa, sa, pb, sb, count)
        assert rc == 0
        want = ref_dot_exact(op, a.reshape(-1), b.reshape(-1))
        assert got.tobytes() == want.tobytes(), ("dot", which_far, geo.name, got, want)
        assert_clean(img, ("dot", which_far, geo.name))


# ---- gaamd_gemm ------------------------------------------------------------------------
def place_matrix(img, far, vals, geo, zone, label):
    """the matrix on the far geometry, or compact in `zone` with ld = cols + 5; (pointer, ld, handle)"""
    rows, cols = vals.shape
    esz = vals.dtype.itemsize
    if geo is not None:
        assert len(geo.offs) == rows and geo.row == cols * esz
        return far.ptr + geo.base, geo.ld, img.rows(geo.base, geo.offs, vals, label + " (far)")
    ld = cols + 5
    return far.ptr + zone, ld, img.rows(zone, [i * ld * esz for i in range(rows)], vals, label)


@pytest.mark.gpu
@pytest.mark.parametrize("which_far", ["A", "B", "C"])
@pytest.mark.parametrize("ta,tb", [("N", "N"), ("N", "T"), ("T", "N"), ("T", "T")], ids=lambda t: t)
@pytest.mark.parametrize("op", [DBL, FLT], ids=["dbl", "flt"])
def test_gemm_far(gpu_lib, far, op, ta, tb, which_far):
    tm, tn, tk = gemm_tiles()
    m, n, k = tm + 1, tn + 1, tk + 1
    dt = DT[op]
    geos = gemm_geos()
    rng = np.random.default_rng(100 * op + 10 * ord(ta) + ord(tb) + ord(which_far))
    for vec in (False, True):
        opa, opb, c0 = rng.integers(-8, 9, (m, k)), rng.integers(-8, 9, (k, n)), rng.integers(-8, 9, (m, n))
        stored = {"A": opa if ta == "N" else opa.T, "B": opb if tb == "N" else opb.T, "C": c0}
        img = Sparse(far, 900 + vec)
        placed = {}
        for name, zone in zip("ABC", COMPACT):
            vals = np.ascontiguousarray(stored[name]).astype(dt)
            geo = geos[(dt.itemsize,) + vals.shape + (vec,)] if name == which_far else None
            placed[name] = place_matrix(img, far, vals, geo, zone, f"matrix {name}")
        want = (2 * (opa.astype(np.int64) @ opb.astype(np.int64)) - 3 * c0).astype(dt)
        img.expect(placed["C"][2], want)
        img.seal()
        (pa, lda, _), (pb, ldb, _), (pc, ldc, _) = placed["A"], placed["B"], placed["C"]
        rc = ga_amd.gemm(op, ta, tb, m, n, k, 2.0, pa, lda, pb, ldb, -3.0, pc, ldc)
        assert rc == 0, rc
        ga_amd.sync()
        assert_clean(img, ("gemm", C.NAMES[op], ta + tb, "far " + which_far, "vec" if vec else "odd"))


# ---- gaamd_transpose / gaamd_transpose_acc ---------------------------------------------
def compact_ld(t, esz, vec):
    """the compact side's leading dimension: a multiple of 16 bytes past the row, or odd"""
    per = max(1, 16 // esz)
    return -(-t // per) * per + per if vec else (t + 3) | 1


@pytest.mark.gpu
@pytest.mark.parametrize("far_dst", [False, True], ids=["far-src", "far-dst"])
@pytest.mark.parametrize("op", [INT, DBL, DCP], ids=["4B", "8B", "16B"])
def test_transpose_far(gpu_lib, far, op, far_dst):
    """random bit patterns moved as they are; the vector path (bases and ld * esz multiples
    of 16) and the scalar one (odd ld)"""
    esz = C.ESZ[op]
    t = transpose_tile(op) + 1
    geos = transpose_geos()
    rng = np.random.default_rng(17 + op + far_dst)
    for vec in (False, True):
        img = Sparse(far, 1100 + vec)
        src = rng.integers(0, 256, (t, t, esz), dtype=np.uint8)
        old = rng.integers(0, 256, (t, t, esz), dtype=np.uint8)
        geo = geos[(esz, t, vec)]
        cld = compact_ld(t, esz, vec)
        coffs = [i * cld * esz for i in range(t)]
        if far_dst:
            ps, lds, _ = far.ptr + COMPACT[0], cld, img.rows(COMPACT[0], coffs, src.reshape(t, -1), "the source")
            pd, ldd, hd = far.ptr + geo.base, geo.ld, img.rows(geo.base, geo.offs, old.reshape(t, -1), "the far destination")
        else:
            ps, lds, _ = far.ptr + geo.base, geo.ld, img.rows(geo.base, geo.offs, src.reshape(t, -1), "the far source")
            pd, ldd, hd = far.ptr + COMPACT[0], cld, img.rows(COMPACT[0], coffs, old.reshape(t, -1), "the destination")
        img.expect(hd, np.ascontiguousarray(src.transpose(1, 0, 2)).reshape(t, -1))
        img.seal()
        assert ga_amd.transpose(op, t, t, ps, lds, pd, ldd) == 0
        ga_amd.sync()
        assert_clean(img, ("transpose", esz, "far dst" if far_dst else "far src", "vec" if vec else "odd"))


@pytest.mark.gpu
@pytest.mark.parametrize("far_c", [False, True], ids=["far-b", "far-c"])
@pytest.mark.parametrize("op", [DBL, FLT], ids=["f64", "f32"])
def test_transpose_acc_far(gpu_lib, far, op, far_c):
    """c = alpha * (c + b^T): one add, one multiply, bit-exact against numpy"""
    dt = DT[op]
    esz = dt.itemsize
    t = transpose_tile(op) + 1
    geos = transpose_geos()
    rng = np.random.default_rng(23 + op + far_c)
    for vec in (False, True):
        img = Sparse(far, 1200 + vec)
        cv = (rng.standard_normal((t, t)) * 10.0 ** rng.integers(-3, 4, (t, t))).astype(dt)
        bv = (rng.standard_normal((t, t)) * 10.0 ** rng.integers(-3, 4, (t, t))).astype(dt)
        geo = geos[(esz, t, vec)]
        cld = compact_ld(t, esz, vec)
        coffs = [i * cld * esz for i in range(t)]
        fargs = (geo.base, geo.offs)
        cargs = (COMPACT[0], coffs)
        img.rows(*(cargs if far_c else fargs), bv, "b" if far_c else "b (far)")
        hc = img.rows(*(fargs if far_c else cargs), cv, "c (far)" if far_c else "c")
        pb, ldb = (far.ptr + COMPACT[0], cld) if far_c else (far.ptr + geo.base, geo.ld)
        pc, ldc = (far.ptr + geo.base, geo.ld) if far_c else (far.ptr + COMPACT[0], cld)
        want = dt.type(-3.0) * (cv + bv.T)
        assert want.dtype == dt
        img.expect(hc, want)
        img.seal()
        assert ga_amd.transpose_acc(op, t, t, -3.0, pb, ldb, pc, ldc) == 0
        ga_amd.sync()
        assert_clean(img, ("transpose_acc", C.NAMES[op], "far c" if far_c else "far b", "vec" if vec else "odd"))


# ---- io-vectors ------------------------------------------------------------------------
def predict_far(n, keys, iov_lds):
    """test_gpu_iov_fuzz.predict for congruent destinations of at most 256 bytes, with the
    rule on units: from 0xffffffff units up no GPU-ordered route"""
    out = dict.fromkeys(PATHS, 0)
    if int(keys.max()) + 1 >= UNITS_LIMIT:
        return out
    if n < RUNS_MIN and np.unique(keys).size == n:
        return out
    if iov_lds:
        assert n <= PART_MAX
        out["lds"] = 1
        if n > PART_WINDOW_MAX:
            lg = part_lg(n)
            counts = np.bincount(part_of(keys.astype(np.uint32), lg), minlength=1 << lg)
            if counts.max() > PART_CAP:
                out["radix"] = 1
    else:
        assert n <= HASH_MAX_PAIRS
        _, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
        out["hashed" if int((cnt[inv] > 1).sum()) <= HASH_CAP else "hashed_then_radix"] = 1
    return out


def iov_case(L, oracle, far, case, kind, iov_lds):
    name, op, n, units, seed = case
    geo = iov_geo(case)
    nb = C.ESZ[op]
    keys, inv = geo.keys, geo.inv
    nu = len(geo.offs)
    img = Sparse(far, seed)
    dst = typed_rows(op, 1, nu * nb, 2000 + seed).reshape(nu, nb)
    src = typed_rows(op, 1, n * nb, 3000 + seed).reshape(n, nb)
    dh = img.rows(0, geo.offs, dst, "an io-vector destination")
    img.rows(IOV_SRC, [0], src.reshape(1, -1), "the io-vector sources")
    # the reference: the oracle's pair-by-pair loop on the destinations compacted
    want = np.ascontiguousarray(dst)
    src_c = np.ascontiguousarray(src)
    sa = np.uint64(src_c.ctypes.data) + np.arange(n, dtype=np.uint64) * np.uint64(nb)
    da = np.uint64(want.ctypes.data) + inv.astype(np.uint64) * np.uint64(nb)
    if kind == "acc":
        oracle.accv(op, C.SCALE[op], sa, da, nb)
    else:
        oracle.copyv(sa, da, nb)
    img.expect(dh, want)
    img.seal()
    g = _giov(np.uint64(far.ptr + IOV_SRC) + np.arange(n, dtype=np.uint64) * np.uint64(nb),
              np.uint64(far.ptr) + keys * np.uint64(nb), nb)
    expect = predict_far(n, keys, iov_lds)
    with Knob("iov_lds", iov_lds):
        p0 = ga_amd.iov_path_counts()
        if kind == "acc":
            keep, sp = ga_amd.scale_buffer(op, C.SCALE[op])
            rc = L.comex_accv(op, sp, ctypes.byref(g), 1, 0, 0)
        else:
            rc = L.comex_putv(ctypes.byref(g), 1, 0, 0)
        assert rc == 0
        ga_amd.comex_fence_all()
        p1 = ga_amd.iov_path_counts()
    delta = {k: int(p1[k] - p0[k]) for k in PATHS}
    what = (iov_id(case), kind, "iov_lds", iov_lds)
    assert delta == expect, (what, "path counters", delta, expect)
    assert_clean(img, what)
    return delta


@pytest.mark.gpu
@pytest.mark.parametrize("case", IOV_SMALL, ids=iov_id)
def test_iov_far_one_workgroup(gpu_lib, oracle, far, case):
    """fewer than 1024 pairs, destinations over more than 8 GiB, both ends three times"""
    assert case[3] * C.ESZ[case[1]] > 8 * G
    for kind in ("acc", "put"):
        assert iov_case(gpu_lib, oracle, far, case, kind, 1)["lds"] == 1
        assert iov_case(gpu_lib, oracle, far, case, kind, 0)["hashed"] == 1


@pytest.mark.gpu
def test_iov_far_getv_sources(gpu_lib, far):
    """getv: the far side is the source list (1000 sources over more than 8 GiB)"""
    case = IOV_SMALL[0]
    geo = iov_geo(case)
    n, nb = case[2], 4
    img = Sparse(far, 4)
    rng = np.random.default_rng(5)
    vals = rng.integers(0, 256, (len(geo.offs), nb), dtype=np.uint8)
    img.rows(0, geo.offs, vals, "an io-vector source")
    dh = img.rows(COMPACT[1], [0], np.zeros((1, n * nb), dtype=np.uint8), "the getv destinations")
    img.expect(dh, vals[geo.inv].reshape(1, -1))
    img.seal()
    g = _giov(np.uint64(far.ptr) + geo.keys * np.uint64(nb),
              np.uint64(far.ptr + COMPACT[1]) + np.arange(n, dtype=np.uint64) * np.uint64(nb), nb)
    p0 = ga_amd.iov_path_counts()
    assert gpu_lib.comex_getv(ctypes.byref(g), 1, 0, 0) == 0
    ga_amd.comex_fence_all()
    assert ga_amd.iov_path_counts() == p0, "one contiguous vector of destinations: no GPU ordering"
    assert_clean(img, "getv")


@pytest.mark.gpu
@pytest.mark.parametrize("case", IOV_UNITS, ids=iov_id)
def test_iov_far_units_limit(gpu_lib, oracle, far, case):
    """units either side of the limit: at 0xfffffffe the GPU orders the pairs and applies
    the top key; from 0xffffffff no GPU-ordered counter moves and the bytes still match"""
    for iov_lds in (1, 0):
        delta = iov_case(gpu_lib, oracle, far, case, "acc", iov_lds)
        if case[3] < UNITS_LIMIT:
            assert delta["lds" if iov_lds else "hashed"] == 1, delta
        else:
            assert not any(delta.values()), delta


@pytest.mark.gpu
def test_iov_far_deferred_partition_at_largest_key(gpu_lib, oracle, far):
    """more than 65536 pairs, 1500 of them on the last destination of 0xfffffffe units: its
    partition overflows and goes to the masked radix pass with the largest admitted key"""
    delta = iov_case(gpu_lib, oracle, far, IOV_DEFERRED[0], "acc", 1)
    assert delta["lds"] == 1 and delta["radix"] == 1, delta


@pytest.mark.gpu
def test_iov_far_key_bit_31(gpu_lib, oracle, far):
    """8-byte pairs over the whole 16 GiB: 2^31 units, the top key has bit 31 set"""
    for iov_lds in (1, 0):
        delta = iov_case(gpu_lib, oracle, far, IOV_BIT31[0], "acc", iov_lds)
        assert delta["lds" if iov_lds else "hashed"] == 1, delta
