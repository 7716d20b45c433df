"""Comparison helpers and case builders shared by the parity and fuzz tests."""
import ctypes

import numpy as np

import cases as C


def random_alpha(rng, op):
    if op in (C.INT, C.LNG):
        return int(rng.integers(-5, 6))
    if op in (C.FLT, C.DBL):
        return float(rng.uniform(-2, 2))
    return complex(rng.uniform(-2, 2), rng.uniform(-2, 2))


def phased_fill(op, nbytes, off, seed):
    """fill values laid out from byte `off % esz` on, so that the elements a side
    reads at an offset below the natural alignment are the generator's values, not
    bit patterns straddling two of them (which include NaNs: the sign and payload of
    a NaN that arithmetic produces are not pinned, so they would differ in the bytes)"""
    ph = off % C.ESZ[op]
    out = np.zeros(nbytes, dtype=np.uint8)
    out[ph:] = C.fill_bytes(op, nbytes - ph, seed)
    return out


def _giov(src_addrs, dst_addrs, nbytes):
    """one comex_giov_t over numpy uint64 address arrays (kept alive by the descriptor)"""
    import ga_amd
    src_addrs = np.ascontiguousarray(src_addrs, dtype=np.uint64)
    dst_addrs = np.ascontiguousarray(dst_addrs, dtype=np.uint64)
    g = ga_amd.GIOV()
    g._keep = (src_addrs, dst_addrs)
    g.src = ctypes.cast(ctypes.c_void_p(src_addrs.ctypes.data), ctypes.POINTER(ctypes.c_void_p))
    g.dst = ctypes.cast(ctypes.c_void_p(dst_addrs.ctypes.data), ctypes.POINTER(ctypes.c_void_p))
    g.count, g.bytes = len(src_addrs), nbytes
    return g


def same_bits_nan_aware(a, b, op):
    """Byte equality, except that a NaN element matches any NaN (payload bits of a
    NaN produced by arithmetic are not pinned by the reference or IEEE)."""
    if np.array_equal(a, b):
        return True
    rt = np.dtype(C.REAL[op])
    if rt.kind != "f":
        return False
    n = (a.size // rt.itemsize) * rt.itemsize
    if not np.array_equal(a[n:], b[n:]):
        return False
    x, y = a[:n].view(rt), b[:n].view(rt)
    xn, yn = np.isnan(x), np.isnan(y)
    if not np.array_equal(xn, yn):
        return False
    it = np.int64 if rt.itemsize == 8 else np.int32
    return np.array_equal(x[~xn].view(it), y[~yn].view(it))


def first_mismatch(a, b, op):
    rt = np.dtype(C.REAL[op])
    n = (min(a.size, b.size) // rt.itemsize) * rt.itemsize
    x, y = a[:n].view(rt), b[:n].view(rt)
    bad = np.nonzero(~((x == y) | (np.isnan(x) & np.isnan(y)) if rt.kind == "f" else (x == y)))[0]
    if bad.size == 0:
        return "tail bytes differ"
    i = bad[0]
    return f"{bad.size} elements differ, first at {i}: got {x[i]!r} want {y[i]!r}"
