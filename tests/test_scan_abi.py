"""CPU: the argument checks of gaamd_enum / gaamd_scan_tail / gaamd_scan / gaamd_mask_count /
gaamd_mask_pack / gaamd_mask_unpack, the exported names, and the numpy restatement of sparse.c
(the ref_* functions of test_gpu_scan.py) against plain Python loops written from sparse.c and
scan_addc.c.  Every code here is returned before anything is launched or allocated, so no device
is needed (the addresses are never dereferenced)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ga_amd
import test_gpu_scan as S
from ga_amd._lib import GA_LIB_PATH, LIB_PATH

INT, LNG, FLT, DBL, CPL, DCP = S.INT, S.LNG, S.FLT, S.DBL, S.CPL, S.DCP
OPS = sorted(ga_amd.OP_DTYPE)
DT, UNS, REAL = S.DT, S.UNS, S.REAL
COPY, ADD, EXCL = S.COPY, S.ADD, S.EXCL
BASE = 0x7F0000000000   # address-shaped numbers; never read
MSK = BASE + (1 << 40)
OUT = BASE + (1 << 41)
E_COUNT, E_OP, E_SCALAR, E_RANGE, E_ALIGN, E_OVERLAP = -3, -4, -5, -7, -8, -11
NEW_CORE = ["gaamd_enum", "gaamd_scan_tail", "gaamd_scan", "gaamd_mask_count", "gaamd_mask_pack", "gaamd_mask_unpack",
            "gaamd_scan_tile", "gaamd_scan_agg_span"]
NEW_GA = ["GA_Patch_enum", "GA_Scan_copy", "GA_Scan_add", "GA_Pack", "GA_Unpack"]
LIMIT = 1 << 34   # the documented limit of n (ga_amd.h); the issue asks for at least 2^33
opid = dict(ids=lambda o: ga_amd.OP_NAME[o])


def test_constants_match_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ga_amd.h")).read()
    for name in ("GAAMD_SCAN_COPY", "GAAMD_SCAN_ADD", "GAAMD_SCAN_ADD_EXCL"):
        m = re.search(rf"#define {name} (\d+)", hdr)
        assert m and int(m.group(1)) == getattr(ga_amd, name), name
    assert len({COPY, ADD, EXCL}) == 3
    m = re.search(r"#define GAAMD_SCAN_MAX_N \(1ll << (\d+)\)", hdr)
    assert m and (1 << int(m.group(1))) == LIMIT >= 1 << 33


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3}


def test_exported_names():
    """the kernel library exports the new entry points and still no GA name; the GA library the
    five calls.  gaamd_pack / gaamd_unpack stay the strided pack and unpack: the compaction is
    gaamd_mask_pack / gaamd_mask_unpack"""
    core, ga = exported(LIB_PATH), exported(GA_LIB_PATH)
    for n in NEW_CORE + ["gaamd_pack", "gaamd_unpack"]:
        assert n in core, n
    assert not [n for n in core if n.startswith(("GA_", "NGA_"))]
    assert not [n for n in NEW_GA if n not in ga]
    assert len(ga_amd.lib().gaamd_pack.argtypes) == 6 and len(ga_amd.lib().gaamd_mask_pack.argtypes) == 7


def test_tile_query():
    for op in OPS:
        for mop in OPS:
            T = ga_amd.scan_tile(op, mop)
            assert T > 0 and T % 64 == 0 and (T * 4) % 16 == 0
    assert ga_amd.scan_tile(36, INT) == E_OP and ga_amd.scan_tile(INT, 43) == E_OP and ga_amd.scan_tile(0, INT) == E_OP
    assert ga_amd.scan_agg_span() >= 64


# ---- the negative codes, every entry point ------------------------------------------------
ALL = ("enum", "scan_tail", "scan", "mask_count", "mask_pack", "mask_unpack")


def calls(names=ALL, op=DBL, mop=INT, fn=ADD, n=100, src=BASE, msk=MSK, out=OUT, host=True, open_=0):
    """the named entry points with the same arguments: {name: return code}.  Only calls that
    fail a check (or have n == 0) may be asked for: there is no device here."""
    L = ga_amd.lib()
    vp = lambda a: ctypes.c_void_p(a) if a else None   # noqa: E731
    flag, cnt = ctypes.c_int(-7), ctypes.c_longlong(-7)
    tail = (ctypes.c_char * 16)()
    one = np.ones(2, dtype=np.float64).ctypes.data_as(ctypes.c_void_p) if host else None
    fns = {
        "enum": lambda: L.gaamd_enum(op, n, 0, one, one, vp(out), None),
        "scan_tail": lambda: L.gaamd_scan_tail(op, fn, mop, n, vp(src), vp(msk), ctypes.byref(flag) if host else None,
                                               tail if host else None, None),
        "scan": lambda: L.gaamd_scan(op, fn, mop, n, vp(src), vp(msk), vp(out), open_, None, None),
        "mask_count": lambda: L.gaamd_mask_count(mop, n, vp(msk), ctypes.byref(cnt) if host else None, None),
        "mask_pack": lambda: L.gaamd_mask_pack(op, mop, n, vp(src), vp(msk), vp(out), None),
        "mask_unpack": lambda: L.gaamd_mask_unpack(op, mop, n, vp(src), vp(msk), vp(out), None),
    }
    return {k: fns[k]() for k in names}


USES_OP = ("enum", "scan_tail", "scan", "mask_pack", "mask_unpack")
USES_MOP = ("scan_tail", "scan", "mask_count", "mask_pack", "mask_unpack")
USES_SRC = ("scan_tail", "scan", "mask_pack", "mask_unpack")
USES_OUT = ("enum", "scan", "mask_pack", "mask_unpack")


def test_negative_n():
    assert set(calls(n=-1).values()) == {E_COUNT}


def test_unknown_types_and_fn():
    for bad in (0, 36, 43, -1):
        assert set(calls(USES_OP, op=bad).values()) == {E_OP}, bad
        assert set(calls(USES_MOP, mop=bad).values()) == {E_OP}, bad
    for bad in (0, 4, -1):
        assert set(calls(("scan", "scan_tail"), fn=bad).values()) == {E_OP}, bad
    # a negative n comes first, an unknown type before a missing pointer
    assert set(calls(USES_OP, op=36, n=-1).values()) == {E_COUNT}
    assert set(calls(USES_SRC, op=36, src=0).values()) == {E_OP}


def test_missing_pointers_and_host_outputs():
    assert set(calls(USES_SRC, src=0).values()) == {E_SCALAR}
    assert set(calls(USES_MOP, msk=0).values()) == {E_SCALAR}
    assert set(calls(USES_OUT, out=0).values()) == {E_SCALAR}
    assert set(calls(("enum", "scan_tail", "mask_count"), host=False).values()) == {E_SCALAR}
    L = ga_amd.lib()
    one = np.ones(2).ctypes.data_as(ctypes.c_void_p)
    assert L.gaamd_enum(DBL, 5, 0, one, None, ctypes.c_void_p(OUT), None) == E_SCALAR
    assert L.gaamd_enum(DBL, 5, 0, None, one, ctypes.c_void_p(OUT), None) == E_SCALAR
    flag = ctypes.c_int()
    assert L.gaamd_scan_tail(DBL, ADD, INT, 5, ctypes.c_void_p(BASE), ctypes.c_void_p(MSK), ctypes.byref(flag), None,
                             None) == E_SCALAR
    # an open segment needs its carry; n == 0 does not excuse a missing pointer
    assert calls(("scan",), open_=1)["scan"] == E_SCALAR
    assert set(calls(USES_MOP, n=0, msk=0).values()) == {E_SCALAR}


def test_n_above_the_limit():
    assert set(calls(n=LIMIT + 1, out=BASE + (1 << 45)).values()) == {E_RANGE}
    # the limit itself passes this check: the next one answers (here the alignment)
    assert set(calls(n=LIMIT, src=BASE + 2, msk=MSK + 2, out=OUT + 2).values()) == {E_ALIGN}


def test_alignment_below_four_bytes():
    for off in (1, 2, 3):
        assert set(calls(USES_SRC, src=BASE + off).values()) == {E_ALIGN}
        assert set(calls(USES_MOP, msk=MSK + off).values()) == {E_ALIGN}
        assert set(calls(USES_OUT, out=OUT + off).values()) == {E_ALIGN}


def test_forbidden_overlaps():
    n = 100
    # dst / packed inside src, touching its last element; inside msk; exactly src
    for out in (BASE + 8 * (n - 1), MSK + 4 * (n - 1), BASE, BASE - 8 * (n - 1)):
        assert set(calls(("scan", "mask_pack"), n=n, out=out).values()) == {E_OVERLAP}, hex(out)
    # unpack's arguments are (packed, msk, dst): dst against packed and against msk
    for out in (BASE + 8 * (n - 1), MSK - 8 * (n - 1)):
        assert calls(("mask_unpack",), n=n, out=out)["mask_unpack"] == E_OVERLAP, hex(out)
    # an n of zero overlaps nothing
    assert set(calls(("scan", "mask_pack", "mask_unpack"), n=0, out=BASE).values()) == {0}


def test_zero_length_writes_the_host_outputs():
    rc, flag, tail = ga_amd.scan_tail(DCP, ADD, CPL, 0, BASE, MSK)
    assert (rc, flag) == (0, 0) and tail.tobytes() == bytes(16)
    assert ga_amd.mask_count(DCP, 0, MSK) == (0, 0)
    r = calls(n=0)
    assert set(r.values()) == {0}, r


# ---- plain loops written from sparse.c / scan_addc.c ---------------------------------------
def loop_set(m):
    out = []
    for v in m:
        if np.iscomplexobj(m):
            out.append(bool(v.real != 0 or v.imag != 0))   # neq_zero_cpl
        else:
            out.append(bool(v != 0))                       # neq_zero_reg
    return np.array(out, dtype=bool)


def _wrap(op, v):
    bits = 8 * DT[op].itemsize
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def add(op, a, b):
    """assign_add_reg / _cpl in the element's type"""
    if op in UNS:
        return _wrap(op, int(a) + int(b))
    if op in REAL:
        r = REAL[op].type
        return complex(r(a.real) + r(b.real), r(a.imag) + r(b.imag))
    return DT[op].type(a) + DT[op].type(b)


def loop_enum(op, n, first, start, stride):
    out = np.zeros(n, dtype=DT[op])
    for i in range(n):
        if op in UNS:
            out[i] = _wrap(op, int(start) + (first + i) * int(stride))
        elif op in REAL:
            r = REAL[op].type
            out[i] = complex(r(start.real) + r(first + i) * r(stride.real), r(start.imag) + r(first + i) * r(stride.imag))
        else:
            t = DT[op].type
            out[i] = t(start) + t(first + i) * t(stride)
    return out


def loop_scan_add(op, x, st, excl, open_, carry):
    """scan_addc.c:116-134 with the open segment of gaamd_scan in front"""
    n = len(x)
    out = np.zeros(n, dtype=DT[op])
    written = np.zeros(n, dtype=bool)
    have = bool(open_)
    run = K_scalar(op, carry) if open_ else None   # the segment's value so far, before element i
    for i in range(n):
        if st[i]:
            have = True
            run = None
        if not have:
            continue
        if excl:
            out[i] = 0 if run is None else run
            run = x[i] if run is None else add(op, run, x[i])
        else:
            run = x[i] if run is None else add(op, run, x[i])
            out[i] = run
        written[i] = True
    return out, written


def K_scalar(op, v):
    return np.array([v], dtype=DT[op])[0]


def loop_scan_copy(op, x, st, open_, carry):
    """sparse.c:196-206"""
    out = np.zeros(len(x), dtype=DT[op])
    last = K_scalar(op, carry) if open_ else np.zeros(1, dtype=DT[op])[0]
    for i in range(len(x)):
        if st[i]:
            last = x[i]
        out[i] = last
    return out


def loop_pack(x, st):
    return np.array([x[i] for i in range(len(x)) if st[i]], dtype=x.dtype)


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_restated_mask_test_against_loops():
    """six mask types (three required, a complex one among them); -0.0 is not set, a NaN is"""
    rng = np.random.default_rng(1)
    for mop in S.MASK_OPS:
        st = rng.integers(0, 3, 400) == 0
        m = S.make_mask(mop, st, rng)
        assert np.array_equal(S.ref_set(m), loop_set(m)) and np.array_equal(loop_set(m), st), mop
    for dt in (np.float32, np.float64):
        m = np.array([0.0, -0.0, np.nan, np.finfo(dt).smallest_subnormal, -1.0], dtype=dt)
        assert list(S.ref_set(m)) == list(loop_set(m)) == [False, False, True, True, True]
    for dt in (np.complex64, np.complex128):
        m = np.array([complex(0.0, -0.0), complex(-0.0, 0.0), complex(np.nan, 0), complex(0, 1), complex(-0.0, np.nan)],
                     dtype=dt)
        assert list(S.ref_set(m)) == list(loop_set(m)) == [False, False, True, True, True]


@pytest.mark.parametrize("op", OPS, **opid)
def test_restated_enum_against_loops(op):
    start = {INT: 2 ** 31 - 5, LNG: 2 ** 63 - 9, FLT: 0.1, DBL: -1.0 / 3.0, CPL: complex(0.1, -7.5),
             DCP: complex(1.0 / 3.0, 2.0)}[op]
    stride = {INT: 0x10001, LNG: 0x100000001, FLT: 0.7, DBL: 1.0 / 7.0, CPL: complex(-0.3, 0.7),
              DCP: complex(1.0 / 7.0, -3.0)}[op]
    for first in (0, 17, (1 << 33) + 12345):
        want = loop_enum(op, 50, first, K_scalar(op, start), K_scalar(op, stride))
        assert same_bits(S.ref_enum(op, 50, first, start, stride), want), (op, first)
    if op in UNS:   # the integers did wrap
        assert np.any(np.diff(S.ref_enum(op, 50, 0, start, stride).astype(object)) < 0)


@pytest.mark.parametrize("op", OPS, **opid)
def test_restated_scans_pack_unpack_against_loops(op):
    rng = np.random.default_rng(10 + op)
    n = 300
    for k, (name, st) in enumerate(S.patterns(n, 100, rng)):
        xa, xc = S.gen_exact(op, n, rng), S.gen_bits(op, n, rng)
        assert S.exact_in_range(op, xa)
        for open_ in (0, 1):
            carry = S.CARRY[op] if open_ else None
            for excl in (False, True):
                got, gw = S.ref_scan_add(op, xa, st, excl, open_, carry)
                want, ww = loop_scan_add(op, xa, st, excl, open_, carry)
                assert np.array_equal(gw, ww) and same_bits(got[gw], want[ww]), (name, open_, excl)
            got, gw = S.ref_scan_copy(op, xc, st, open_, carry)
            assert gw.all() and same_bits(got, loop_scan_copy(op, xc, st, open_, carry)), (name, open_)
        # the tails: what a following range would take as its carry
        for fn in (ADD, COPY):
            x = xa if fn == ADD else xc
            flag, tail = S.ref_scan_tail(op, fn, x, st)
            assert flag == int(st.any())
            more, ms = x[:7], np.zeros(7, dtype=bool)
            whole, _ = S.ref_scan(op, fn, np.concatenate([x, more]), np.concatenate([st, ms]))
            if st.any() or fn == COPY:
                part, _ = S.ref_scan(op, fn, more, ms, 1 if st.any() else 0, tail[0] if st.any() else None)
                assert same_bits(part, whole[n:]), (name, fn)
        assert same_bits(S.ref_pack(xc, st), loop_pack(xc, st))
        y = S.gen_bits(op, n, rng)
        want = y.copy()
        j = 0
        for i in range(n):   # sparse.c:590-601
            if st[i]:
                want[i] = xc[j]
                j += 1
        assert same_bits(S.ref_unpack(xc, st, y), want)
    if op in UNS:   # the integer sums did wrap
        full, _ = S.ref_scan_add(op, S.gen_exact(op, n, rng), np.arange(n) == 0, False)
        assert np.any(np.diff(full.astype(object)) < 0) and np.any(np.diff(full.astype(object)) > 0)


def test_exact_data_stays_in_range_and_the_check_can_fail():
    rng = np.random.default_rng(3)
    T = ga_amd.scan_tile(FLT, INT)
    for op in OPS:
        assert S.exact_in_range(op, S.gen_exact(op, 3 * T + 17, rng))
    assert not S.exact_in_range(FLT, np.full(200000, 100.0, dtype=np.float32))
    assert not S.exact_in_range(DBL, np.array([0.5]))
