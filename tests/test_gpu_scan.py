"""GPU, one rank, kernel level: gaamd_enum, gaamd_scan_tail, gaamd_scan, gaamd_mask_count,
gaamd_mask_pack and gaamd_mask_unpack against a numpy restatement of the reference loops
(global/src/sparse.c), compared as raw bits.  The restatement (ref_* below) is checked on the
CPU against plain Python loops written from sparse.c and scan_addc.c (tests/test_scan_abi.py).

  set        msk[i] != 0; complex: either part; -0.0 is not set, a NaN is (neq_zero_reg / _cpl)
  enum       a[i] = start + (T)(first + i) * stride, complex part by part            59-76
  scan copy  dst[i] = src at the last set element at or before i; zero before the first 196-206
  scan add   dst[i] = src[s] + ... + src[i] (exclusive: ... + src[i-1], zero at s), s the last set
             element at or before i; elements before the first set one are NOT written  361-406
  pack       packed[k] = src[f_k], f_k the k-th set element; unpack dst[f_k] = packed[k]
  open/carry a segment open on entry: carry is the leftmost term (copy: the value copied)
Integers in unsigned arithmetic (wraparound).  The sums of the restatement are sequential
(np.add.accumulate); the kernel's tree is another order, so floating-point ADD is compared bit
for bit only on exactly summable data and within the any-order bound otherwise.

T (elements per tile) and the aggregate scan's span come from the library (gaamd_scan_tile,
gaamd_scan_agg_span).

The far-offset case is checked on the device with the library's own kernels (gaamd_enum for
the expected values, gaamd_patch_add and gaamd_patch_norm for the difference), not with torch:
torch's wheel carries a HIP runtime of its own and its allocations are not this runtime's
(tests/test_abi.py, test_torch_runtime_first_*).
"""
import math

import numpy as np
import pytest

import ga_amd
import test_gpu_ga_math as K

INT, LNG, FLT, DBL, CPL, DCP = K.INT, K.LNG, K.FLT, K.DBL, K.CPL, K.DCP
OPS = K.OPS
DT, UNS, REAL = K.DT, K.UNS, K.REAL
COPY, ADD, EXCL = ga_amd.GAAMD_SCAN_COPY, ga_amd.GAAMD_SCAN_ADD, ga_amd.GAAMD_SCAN_ADD_EXCL
FNS = [COPY, ADD, EXCL]
FN_NAME = {COPY: "copy", ADD: "add", EXCL: "excl"}
opid = dict(ids=lambda o: ga_amd.OP_NAME[o])
CANARY = 0xA5


# ---- the reference restated --------------------------------------------------------
def ref_set(m):
    """which mask elements are set"""
    return m != 0


def ref_enum(op, n, first, start, stride):
    g = first + np.arange(n, dtype=np.int64)
    a, s = K.scalar(op, start), K.scalar(op, stride)
    if op in UNS:
        u = UNS[op]
        return (a.view(u) + g.astype(u) * s.view(u)).view(DT[op])
    if op in REAL:
        r = g.astype(REAL[op])
        return K._cplx(op, a.real + r * s.real, a.imag + r * s.imag)
    return a + g.astype(DT[op]) * s


def _acc(op, x):
    """the running sums of x, left to right, in the element's type (complex part by part)"""
    if op in UNS:
        return np.add.accumulate(x.view(UNS[op]), dtype=UNS[op]).view(DT[op])
    return np.add.accumulate(x, dtype=DT[op])


def ref_scan_add(op, x, st, excl, open_=0, carry=None):
    """(dst, written): written False where the call leaves dst alone"""
    n = len(x)
    out = np.zeros(n, dtype=DT[op])
    written = np.zeros(n, dtype=bool)
    starts = list(np.flatnonzero(st))
    first = starts[0] if starts else n
    if open_ and first > 0:
        run = _acc(op, np.concatenate([K.scalar(op, carry), x[:first]]))
        out[:first] = run[:-1] if excl else run[1:]
        written[:first] = True
    for s, e in zip(starts, starts[1:] + [n]):
        run = _acc(op, x[s:e])
        if excl:
            out[s] = 0
            out[s + 1:e] = run[:-1]
        else:
            out[s:e] = run
        written[s:e] = True
    return out, written


def ref_scan_copy(op, x, st, open_=0, carry=None):
    n = len(x)
    last = np.maximum.accumulate(np.where(st, np.arange(n), -1))
    out = x[np.maximum(last, 0)].copy()
    out[last < 0] = K.scalar(op, carry)[0] if open_ else np.zeros(1, dtype=DT[op])[0]
    return out, np.ones(n, dtype=bool)


def ref_scan(op, fn, x, st, open_=0, carry=None):
    if fn == COPY:
        return ref_scan_copy(op, x, st, open_, carry)
    return ref_scan_add(op, x, st, fn == EXCL, open_, carry)


def ref_scan_tail(op, fn, x, st):
    """(has_flag, tail)"""
    idx = np.flatnonzero(st)
    if fn == COPY:
        return int(len(idx) > 0), (x[idx[-1]:idx[-1] + 1].copy() if len(idx) else np.zeros(1, dtype=DT[op]))
    if len(x) == 0:
        return 0, np.zeros(1, dtype=DT[op])
    return int(len(idx) > 0), _acc(op, x[idx[-1] if len(idx) else 0:])[-1:].copy()


def ref_pack(x, st):
    return x[st].copy()


def ref_unpack(packed, st, dst):
    out = dst.copy()
    out[st] = packed[:int(st.sum())]
    return out


# ---- data ---------------------------------------------------------------------------
def gen_bits(op, n, rng):
    """any bit pattern: NaNs with payloads, -0.0, denormals, infinities (copy, pack, unpack)"""
    x = rng.integers(0, 256, n * DT[op].itemsize, dtype=np.uint8).view(DT[op]).copy()
    if n > 2 and op not in UNS:
        x[1] = np.array([-0.0], dtype=DT[op])[0]
        x.view(np.uint8)[2 * DT[op].itemsize:3 * DT[op].itemsize] = 0xFF   # a NaN with a full payload
    return x


def gen_exact(op, n, rng):
    """ADD data: integers of the full range (wraparound); floats integer-valued in [-100, 100],
    so n * max|x| < 2^24 up to n = 167772 and every partial sum in any order is exact"""
    if op in UNS:
        return K.gen(op, n, rng)
    return K.gen(op, n, rng, small=100)


def exact_in_range(op, x):
    """the restatement's own check of gen_exact: the sum of |x| stays below 2^24 / 2^53"""
    if op in UNS:
        return True
    parts = [x.real, x.imag] if op in REAL else [x]
    lim = 2.0 ** (24 if REAL.get(op, DT[op]).itemsize == 4 else 53)
    return all(float(np.abs(p.astype(np.float64)).sum()) < lim and np.all(p == np.rint(p)) for p in parts)


MASK_OPS = [INT, DBL, CPL, LNG, FLT, DCP]


def make_mask(mop, st, rng):
    """a mask of type mop with exactly the elements st set: set ones from odd non-zero values (a
    NaN, a denormal, INT_MIN, a word of zeros beside a word of ones), the others +0 or -0.0"""
    n = len(st)
    dt = DT[mop]
    pick = rng.integers(0, 4, n)
    if mop in UNS:
        vals = np.array({INT: [1, -1, -2 ** 31, 7], LNG: [1, 1 << 32, -2 ** 63, 0xFFFFFFFF]}[mop], dtype=dt)
        return np.where(st, vals[pick], 0).astype(dt)
    rdt = REAL.get(mop, dt)
    tiny = np.finfo(rdt).smallest_subnormal
    nz = np.array([1.0, np.nan, tiny, -2.5], dtype=rdt)
    zs = np.array([0.0, -0.0], dtype=rdt)
    z1, z2 = zs[rng.integers(0, 2, n)], zs[rng.integers(0, 2, n)]
    if mop in REAL:
        which = rng.integers(0, 3, n)   # re only, im only, both
        re = np.where(st & (which != 1), nz[pick], z1)
        im = np.where(st & (which != 0), nz[(pick + 1) % 4], z2)
        return K._cplx(mop, re, im)
    return np.where(st, nz[pick], z1).astype(dt)


def patterns(n, T, rng):
    """(name, set) for every mask pattern the length admits"""
    idx = np.arange(n)
    out = [("none", np.zeros(n, dtype=bool)), ("all", np.ones(n, dtype=bool)), ("first", idx == 0),
           ("last", idx == n - 1), ("tile_last", idx % T == T - 1), ("tile_first", idx % T == 0)]
    if n >= 3 * T:   # two whole tiles with nothing set between two set elements
        out.append(("carry_through", (idx == T - 3) | (idx == 3 * T + 5)))
    for d in (2, 64, 4096):
        out.append((f"random_1/{d}", rng.integers(0, d, n) == 0))
    return out


def lengths(T):
    return [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]


# ---- device plumbing ----------------------------------------------------------------
LEAD = 256
SLOT = 1 << 20    # room for 3 T + 17 elements of 16 bytes, the canaries and the alignment offsets
# (src, msk, dst) byte offsets below 16: every vector width on every side
ALIGNS = [(0, 0, 0), (4, 8, 12), (8, 4, 0), (12, 0, 8), (0, 12, 4)]


@pytest.fixture(scope="module")
def dev(gpu_lib):
    b = ga_amd.DeviceBuffer(4 * SLOT)
    yield b
    b.free()


class Img:
    """an array inside canaries at byte offset `off` of slot `slot`"""

    def __init__(self, dev, slot, off, arr):
        self.dev, self.base, self.nbytes = dev, slot * SLOT + LEAD + off, arr.nbytes
        assert LEAD + off + arr.nbytes + LEAD <= SLOT
        self.img = np.full(LEAD + off + arr.nbytes + LEAD, CANARY, dtype=np.uint8)
        self.img[LEAD + off:LEAD + off + arr.nbytes] = arr.view(np.uint8).reshape(-1)
        dev.upload(self.img, slot * SLOT)
        self.slot, self.off = slot, off

    @property
    def ptr(self):
        return self.dev.ptr + self.base

    def expect(self, arr, written=None):
        """the image with `arr` where `written` (all by default)"""
        e = self.img.copy()
        body = e[LEAD + self.off:LEAD + self.off + self.nbytes].view(arr.dtype)
        if written is None:
            body[:] = arr
        else:
            body[written] = arr[written]
        return e

    def back(self):
        ga_amd.sync()
        return self.dev.download(np.uint8, self.img.size, self.slot * SLOT)


def canary_arr(op, n):
    return np.full(n * DT[op].itemsize, CANARY, dtype=np.uint8).view(DT[op])


CARRY = {INT: -123456789, LNG: -0x123456789ABCDEF, FLT: 37.0, DBL: -41.0, CPL: complex(5.0, -9.0), DCP: complex(-3.0, 8.0)}


def check_scan(dev, op, fn, mop, x, st, rng, al, open_=0, tag=None):
    m = make_mask(mop, st, rng)
    assert np.array_equal(ref_set(m), st), tag
    n = len(x)
    src, msk = Img(dev, 0, al[0], x), Img(dev, 1, al[1], m)
    dst = Img(dev, 2, al[2], canary_arr(op, n))
    carry = CARRY[op] if open_ else None
    assert ga_amd.scan(op, fn, mop, n, src.ptr, msk.ptr, dst.ptr, open_, carry) == 0, tag
    want, written = ref_scan(op, fn, x, st, open_, carry)
    got = dst.back()
    assert got.tobytes() == dst.expect(want, written).tobytes(), tag
    if not open_:
        rc, flag, tail = ga_amd.scan_tail(op, fn, mop, n, src.ptr, msk.ptr)
        rf, rt = ref_scan_tail(op, fn, x, st)
        assert rc == 0 and flag == rf and tail.tobytes() == rt.tobytes(), (tag, flag, rf, tail, rt)
    assert src.back().tobytes() == src.img.tobytes() and msk.back().tobytes() == msk.img.tobytes(), tag


# ---- tests --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, **opid)
def test_scan_bit_exact_on_lengths_and_patterns(gpu_lib, dev, op):
    """every length x every mask pattern x copy / add / exclusive add, the mask type, the base
    alignments and open/carry rotating; ADD on exactly summable data, COPY on any bits"""
    T = ga_amd.scan_tile(op, INT)
    rng = np.random.default_rng(100 + op)
    case = 0
    for n in lengths(T):
        xa, xc = gen_exact(op, n, rng), gen_bits(op, n, rng)
        assert exact_in_range(op, np.concatenate([xa, K.scalar(op, CARRY[op])]))
        for name, st in patterns(n, T, rng):
            for fn in FNS:
                mop = MASK_OPS[case % len(MASK_OPS)]
                al = ALIGNS[case % len(ALIGNS)]
                open_ = (case // 3) % 2
                case += 1
                check_scan(dev, op, fn, mop, xc if fn == COPY else xa, st, rng, al, open_,
                           (ga_amd.OP_NAME[op], FN_NAME[fn], ga_amd.OP_NAME[mop], n, name, al, open_))


@pytest.mark.gpu
@pytest.mark.parametrize("mop", MASK_OPS, **opid)
def test_every_mask_type_against_every_element_size(gpu_lib, dev, mop):
    """the mask loader per type (NaN, -0.0, denormals, half-zero words) under 4-, 8- and 16-byte
    values, with open and closed entry for every fn"""
    T = ga_amd.scan_tile(INT, mop)
    rng = np.random.default_rng(200 + mop)
    n = T + 65
    for op in (INT, DBL, DCP):
        for k, (fn, open_) in enumerate([(f, o) for f in FNS for o in (0, 1)]):
            st = rng.integers(0, 3, n) == 0
            st[:5] = False
            x = gen_bits(op, n, rng) if fn == COPY else gen_exact(op, n, rng)
            check_scan(dev, op, fn, mop, x, st, rng, ALIGNS[k % len(ALIGNS)], open_,
                       (ga_amd.OP_NAME[op], FN_NAME[fn], ga_amd.OP_NAME[mop], open_))


@pytest.mark.gpu
def test_more_tiles_than_one_pass_of_the_aggregate_scan(gpu_lib):
    """the aggregate scan's loop runs twice: a carry that crosses the pass boundary, a set
    element in the first and in the last tile of each pass"""
    T, span = ga_amd.scan_tile(INT, INT), ga_amd.scan_agg_span()
    n = T * (span + 3) + 11
    assert -(-n // T) > span
    rng = np.random.default_rng(5)
    x = gen_exact(INT, n, rng)
    st = np.zeros(n, dtype=bool)
    st[[7, T * (span - 1) + 1, T * span + T - 1, n - 2]] = True
    m = make_mask(INT, st, rng)
    bufs = [ga_amd.DeviceBuffer(n * 4 + 2 * LEAD) for _ in range(3)]
    try:
        bufs[0].upload(x, LEAD)
        bufs[1].upload(m, LEAD)
        for fn, open_ in ((ADD, 0), (EXCL, 1), (COPY, 0)):
            img = np.full(n * 4 + 2 * LEAD, CANARY, dtype=np.uint8)
            bufs[2].upload(img)
            carry = CARRY[INT] if open_ else None
            assert ga_amd.scan(INT, fn, INT, n, bufs[0].ptr + LEAD, bufs[1].ptr + LEAD, bufs[2].ptr + LEAD, open_,
                               carry) == 0
            want, written = ref_scan(INT, fn, x, st, open_, carry)
            body = img[LEAD:LEAD + 4 * n].view(np.int32)
            body[written] = want[written]
            ga_amd.sync()
            assert bufs[2].download(np.uint8).tobytes() == img.tobytes(), FN_NAME[fn]
        rc, flag, tail = ga_amd.scan_tail(INT, ADD, INT, n, bufs[0].ptr + LEAD, bufs[1].ptr + LEAD)
        assert (rc, flag) == (0, 1) and tail.tobytes() == ref_scan_tail(INT, ADD, x, st)[1].tobytes()
        # the compaction's offsets cross the pass boundary too
        st2 = rng.integers(0, 64, n) == 0
        st2[[T * span - 1, T * span]] = True
        bufs[1].upload(make_mask(INT, st2, rng), LEAD)
        rc, cnt = ga_amd.mask_count(INT, n, bufs[1].ptr + LEAD)
        assert (rc, cnt) == (0, int(st2.sum()))
        img = np.full(n * 4 + 2 * LEAD, CANARY, dtype=np.uint8)
        bufs[2].upload(img)
        assert ga_amd.mask_pack(INT, INT, n, bufs[0].ptr + LEAD, bufs[1].ptr + LEAD, bufs[2].ptr + LEAD) == 0
        img[LEAD:LEAD + 4 * cnt] = ref_pack(x, st2).view(np.uint8)
        ga_amd.sync()
        assert bufs[2].download(np.uint8).tobytes() == img.tobytes()
    finally:
        for b in bufs:
            b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, **opid)
def test_count_pack_unpack_bit_exact(gpu_lib, dev, op):
    """every length x every pattern: the count, packed[0 .. count) and nothing past it, unpack
    into a dst whose unset elements stay; any bit pattern survives"""
    T = ga_amd.scan_tile(op, INT)
    rng = np.random.default_rng(300 + op)
    case = 0
    for n in lengths(T):
        x = gen_bits(op, n, rng)
        for name, st in patterns(n, T, rng):
            mop = MASK_OPS[case % len(MASK_OPS)]
            al = ALIGNS[case % len(ALIGNS)]
            case += 1
            tag = (ga_amd.OP_NAME[op], ga_amd.OP_NAME[mop], n, name, al)
            m = make_mask(mop, st, rng)
            src, msk = Img(dev, 0, al[0], x), Img(dev, 1, al[1], m)
            packed = Img(dev, 2, al[2], canary_arr(op, n))
            rc, cnt = ga_amd.mask_count(mop, n, msk.ptr)
            assert (rc, cnt) == (0, int(st.sum())), tag
            assert ga_amd.mask_pack(op, mop, n, src.ptr, msk.ptr, packed.ptr) == 0, tag
            want = ref_pack(x, st)
            full = canary_arr(op, n).copy()
            full[:cnt] = want
            assert packed.back().tobytes() == packed.expect(full).tobytes(), tag
            # unpack what was packed, reversed in order, into a dst of other bits
            y = gen_bits(op, n, rng)
            rev = Img(dev, 0, al[0], want[::-1].copy() if cnt else canary_arr(op, 1))
            dst = Img(dev, 3, al[2], y)
            assert ga_amd.mask_unpack(op, mop, n, rev.ptr, msk.ptr, dst.ptr) == 0, tag
            assert dst.back().tobytes() == dst.expect(ref_unpack(want[::-1], st, y)).tobytes(), tag
            assert rev.back().tobytes() == rev.img.tobytes() and msk.back().tobytes() == msk.img.tobytes(), tag


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS, **opid)
def test_enum_bit_exact(gpu_lib, dev, op):
    """all six types, integer wraparound, a first far above 2^32, every base alignment"""
    T = ga_amd.scan_tile(op, INT)
    start = {INT: 2 ** 31 - 5, LNG: 2 ** 63 - 9, FLT: 0.1, DBL: -1.0 / 3.0, CPL: complex(0.1, -7.5),
             DCP: complex(1.0 / 3.0, 2.0)}[op]
    stride = {INT: 0x10001, LNG: 0x100000001, FLT: 0.7, DBL: 1.0 / 7.0, CPL: complex(-0.3, 0.7),
              DCP: complex(1.0 / 7.0, -3.0)}[op]
    case = 0
    for n in lengths(T) + [2, 3, 5]:
        for first in (0, 17, (1 << 33) + 12345):
            al = ALIGNS[case % len(ALIGNS)]
            case += 1
            dst = Img(dev, 2, al[2], canary_arr(op, n))
            assert ga_amd.enum(op, n, first, start, stride, dst.ptr) == 0
            want = ref_enum(op, n, first, start, stride)
            assert dst.back().tobytes() == dst.expect(want).tobytes(), (ga_amd.OP_NAME[op], n, first, al)


def _seg_bound(op, x, st, excl, open_, carry):
    """2 gamma_L sum|x_j| per element and part, in float64 with math.fsum; L counts the terms"""
    rdt = REAL.get(op, DT[op])
    u = 2.0 ** -24 if rdt.itemsize == 4 else 2.0 ** -53
    parts = [x.real, x.imag] if op in REAL else [x]
    cs = [K.scalar(op, carry).real[0], K.scalar(op, carry).imag[0]] if open_ else [0.0, 0.0]
    n = len(x)
    out = np.zeros((len(parts), n))
    for pi, p in enumerate(parts):
        a = np.abs(p.astype(np.float64))
        terms = [abs(float(cs[pi]))] if open_ else []
        for i in range(n):
            if st[i]:
                terms = []
            if not excl:
                terms.append(a[i])
            L = len(terms)
            g = L * u / (1 - L * u)
            out[pi, i] = 2 * g * math.fsum(terms)
            if excl:
                terms.append(a[i])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("op", [FLT, DBL, CPL, DCP], **opid)
def test_inexact_add_reproducible_and_within_the_any_order_bound(gpu_lib, dev, op):
    """random normal data of mixed sign: two runs give the same bits; against the sequential
    restatement every element lies within 2 gamma_L sum|x_j| over its segment so far (the
    standard bound of any summation order, applied to both sides), gamma_L = L u / (1 - L u)"""
    T = ga_amd.scan_tile(op, INT)
    rng = np.random.default_rng(400 + op)
    n = 3 * T + 17
    rdt = REAL.get(op, DT[op])
    x = K._cplx(op, rng.standard_normal(n).astype(rdt), rng.standard_normal(n).astype(rdt)) if op in REAL \
        else rng.standard_normal(n).astype(rdt)
    for (name, st), fn, open_ in zip([p for p in patterns(n, T, rng) if p[0] in ("none", "carry_through", "random_1/64")],
                                     (ADD, EXCL, ADD), (1, 0, 1)):
        carry = CARRY[op] if open_ else None
        m = make_mask(INT, st, rng)
        src, msk = Img(dev, 0, 8, x), Img(dev, 1, 4, m)
        runs = []
        for _ in range(2):
            dst = Img(dev, 2, 0, canary_arr(op, n))
            assert ga_amd.scan(op, fn, INT, n, src.ptr, msk.ptr, dst.ptr, open_, carry) == 0
            runs.append(dst.back())
        assert runs[0].tobytes() == runs[1].tobytes(), name
        want, written = ref_scan(op, fn, x, st, open_, carry)
        got = runs[0][LEAD:LEAD + x.nbytes].view(DT[op])
        assert runs[0].tobytes() == dst.expect(got, written).tobytes(), ("an unwritten element was written", name)
        bound = _seg_bound(op, x, st, fn == EXCL, open_, carry)
        gp = [got.real, got.imag] if op in REAL else [got]
        wp = [want.real, want.imag] if op in REAL else [want]
        for pi in range(len(gp)):
            err = np.abs(gp[pi].astype(np.float64) - wp[pi].astype(np.float64))[written]
            assert np.all(err <= bound[pi][written]), (name, float(err.max()))


@pytest.mark.gpu
def test_zero_length_and_host_outputs(gpu_lib, dev):
    rc, flag, tail = ga_amd.scan_tail(DCP, ADD, INT, 0, dev.ptr, dev.ptr + SLOT)
    assert (rc, flag) == (0, 0) and tail.tobytes() == bytes(16)
    assert ga_amd.mask_count(CPL, 0, dev.ptr) == (0, 0)
    assert ga_amd.scan(DBL, ADD, INT, 0, dev.ptr, dev.ptr + SLOT, dev.ptr + 2 * SLOT) == 0
    assert ga_amd.mask_pack(DBL, INT, 0, dev.ptr, dev.ptr + SLOT, dev.ptr + 2 * SLOT) == 0
    assert ga_amd.mask_unpack(DBL, INT, 0, dev.ptr, dev.ptr + SLOT, dev.ptr + 2 * SLOT) == 0
    assert ga_amd.enum(DBL, 0, 0, 1.0, 1.0, dev.ptr) == 0


@pytest.mark.gpu
def test_far_offsets_int_inclusive_add(gpu_lib):
    """C_INT, n = 2^30 + T + 3, src all ones, set at 0 and at 2^30 + 1: byte offsets pass 2^32.
    dst[i] = i + 1 up to 2^30, then i - 2^30.  Checked on the device (see the module docstring):
    expected values by gaamd_enum, dst - expected by gaamd_patch_add, its infinity norm must be 0;
    the head, the 64 elements around 2^30 + 1 and the tail are fetched and compared here."""
    T = ga_amd.scan_tile(INT, INT)
    n, cut = 2 ** 30 + T + 3, 2 ** 30 + 1
    src, msk, dst, exp = (ga_amd.DeviceBuffer(4 * n + 512) for _ in range(4))
    L = gpu_lib
    try:
        assert ga_amd.patch_fill(INT, 1, src.ptr, [], [n]) == 0
        assert L.gaamd_memset(msk.ptr, 0, 4 * n) == 0
        assert L.gaamd_memset(dst.ptr, CANARY, 4 * n + 512) == 0
        one = np.ones(1, dtype=np.int32)
        ga_amd.sync()
        msk.upload(one, 0)
        msk.upload(one, 4 * cut)
        assert ga_amd.scan(INT, ADD, INT, n, src.ptr, msk.ptr, dst.ptr) == 0
        assert ga_amd.enum(INT, cut, 0, 1, 1, exp.ptr) == 0
        assert ga_amd.enum(INT, n - cut, 0, 1, 1, exp.ptr + 4 * cut) == 0
        assert ga_amd.patch_add(INT, 1, dst.ptr, [], -1, exp.ptr, [], exp.ptr, [], [n]) == 0
        rc, worst = ga_amd.patch_norm(INT, ga_amd.GAAMD_NORM_INF, exp.ptr, [], [n])
        assert rc == 0 and int(worst[0]) == 0, worst
        assert np.array_equal(dst.download(np.int32, 64, 0), np.arange(1, 65, dtype=np.int32))
        around = dst.download(np.int32, 64, 4 * (cut - 32))
        assert np.array_equal(around, np.concatenate([np.arange(cut - 31, cut + 1), np.arange(1, 33)]).astype(np.int32))
        tail = dst.download(np.int32, 64, 4 * (n - 64))
        assert np.array_equal(tail, np.arange(n - 64 - cut + 1, n - cut + 1, dtype=np.int32))
        assert dst.download(np.uint8, 512, 4 * n).tobytes() == bytes([CANARY]) * 512
        rc, flag, t = ga_amd.scan_tail(INT, ADD, INT, n, src.ptr, msk.ptr)
        assert (rc, flag, int(t[0])) == (0, 1, n - cut)
    finally:
        for b in (src, msk, dst, exp):
            b.free()
