"""One rank of the GA_Patch_enum / GA_Scan_copy / GA_Scan_add / GA_Pack / GA_Unpack tests
(test_gpu_ga_scan_mp.py starts 1, 2 or 3 of these on one GPU).

Modes:
  all          the cases of scan_addc.c, packc.c, unpackc.c and patch_enumc.c restated at 3001
               elements on REGULAR and irregular block maps, and the corner cases -- each section
               prints "SECTION <name> OK"
  abort-short  GA_Pack into a g_dst one element too short: every rank must end through GA_Error;
               prints "ABORT EXPECTED" just before it and "NOT REACHED" if it returns
Expected values: the numpy restatement of sparse.c in test_gpu_scan.py, compared as raw bits by
every rank.  Floating-point data are exactly summable, so the results do not depend on how the
array is cut: every result is printed as "DIGEST <case> <sha1>", which the launcher compares
across ranks and rank counts.  Prints "RANK <r> OK" on success.
"""
import ctypes
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import ga_amd  # noqa: E402
import test_gpu_ga_math as K  # noqa: E402
import test_gpu_scan as S  # noqa: E402
from ga_worker import C_DBL, C_DCPL, C_FLOAT, C_INT, C_LONG, C_SCPL, GA, OP_OF, blocks_of, run, vp  # noqa: E402

NELEM = 3001
VALUE_TYPES = (C_INT, C_LONG, C_FLOAT, C_DBL, C_DCPL)
MASK_TYPES = (C_INT, C_DBL, C_SCPL)
# scan_addc.c:226-235
SCAN_CASES = [(0, NELEM - 1, 0), (0, NELEM - 1, 1), (1, NELEM - 1, 0), (1, NELEM - 1, 1), (0, NELEM - 2, 0),
              (0, NELEM - 2, 1), (NELEM // 4, NELEM // 2, 0), (NELEM // 4, NELEM // 2, 1),
              (NELEM // 3, NELEM // 3 + 10, 0), (NELEM // 3, NELEM // 3 + 10, 1)]
# packc.c / unpackc.c:213-217
PACK_CASES = [(0, NELEM - 1), (1, NELEM - 1), (0, NELEM - 2), (NELEM // 4, NELEM // 2), (NELEM // 3, NELEM // 3 + 10)]
DENSITY = (1, 2, 3, 64)   # one element in q set; scan_addc.c runs q = 1, 2, 3


def cuts(n, size, shift):
    """`size` block starts over n elements, the interior ones moved by `shift`"""
    return [0] + [min(n - 1, max(1, n * k // size + shift)) for k in range(1, size)]


def array(L, t, n, size, irreg, name=b"x", shift=37):
    if not irreg:
        return GA(L, t, [n], name)
    nb = min(size, n)
    return GA(L, t, [n], name, irreg=([nb], cuts(n, nb, shift)))


def live_unchanged(L, live, what):
    assert L.gaamd_ga_live_arrays() == live, f"{what}: a temporary is still alive"


def call(L, name, *args):
    live = L.gaamd_ga_live_arrays()
    getattr(L, name)(*args)
    live_unchanged(L, live, name)


def digest(case, arr):
    print(f"DIGEST {case} {hashlib.sha1(np.ascontiguousarray(arr).tobytes()).hexdigest()}", flush=True)


def mask_for(mop, n, q, rng, lo, hi):
    """one element in q set, and the elements just outside [lo, hi] set too: they are ignored"""
    st = rng.integers(0, q, n) == 0
    for i in (lo - 1, hi + 1):
        if 0 <= i < n:
            st[i] = True
    return st


def scan_model(dst, fn, src, st, lo, hi):
    """what the call leaves in dst: [lo, hi] from the restatement, the rest alone"""
    want, written = S.ref_scan(dst.op, fn, src.model[lo:hi + 1], st[lo:hi + 1])
    part = dst.model[lo:hi + 1]
    part[written] = want[written]


def trio(L, t, mt, n, size, irreg, shift=37):
    return (array(L, t, n, size, irreg, b"src", shift), array(L, t, n, size, irreg, b"dst", shift),
            array(L, mt, n, size, irreg, b"msk", shift))


# ---- sections ---------------------------------------------------------------------
def scans(L, rank, size):
    live = L.gaamd_ga_live_arrays()
    for t in VALUE_TYPES:
        for mt in MASK_TYPES:
            for irreg in (False, True):
                src, dst, msk = trio(L, t, mt, NELEM, size, irreg)
                op, mop = src.op, msk.op
                rng = np.random.default_rng(1000 * op + mop)
                tag = f"{ga_amd.OP_NAME[op]}-{ga_amd.OP_NAME[mop]}"
                src.put(S.gen_exact(op, NELEM, rng), rank)
                assert S.exact_in_range(op, src.model)
                dst.put(K.gen(op, NELEM, rng), rank)
                for k, (lo, hi, excl) in enumerate(SCAN_CASES):
                    st = mask_for(mop, NELEM, DENSITY[k % len(DENSITY)], rng, lo, hi)
                    msk.put(S.make_mask(mop, st, rng), rank)
                    call(L, "GA_Scan_add", src.g, dst.g, msk.g, lo, hi, excl)
                    scan_model(dst, S.EXCL if excl else S.ADD, src, st, lo, hi)
                    dst.check(f"GA_Scan_add {tag} irreg={irreg} lo={lo} hi={hi} excl={excl}")
                    digest(f"scan_add-{tag}-{lo}-{hi}-{excl}", dst.model)
                    if excl:   # the same mask and range through the copy
                        call(L, "GA_Scan_copy", src.g, dst.g, msk.g, lo, hi)
                        scan_model(dst, S.COPY, src, st, lo, hi)
                        dst.check(f"GA_Scan_copy {tag} irreg={irreg} lo={lo} hi={hi}")
                        digest(f"scan_copy-{tag}-{lo}-{hi}", dst.model)
                src.check(f"the scans left src alone {tag}")
                for a in (src, dst, msk):
                    a.destroy()
    live_unchanged(L, live, "scans")


def packs(L, rank, size):
    live = L.gaamd_ga_live_arrays()
    for t in VALUE_TYPES:
        for mt in MASK_TYPES:
            for irreg in (False, True):
                src, dst, msk = trio(L, t, mt, NELEM, size, irreg)
                # the packed side under another map than the mask's
                other = array(L, t, NELEM, size, not irreg, b"packed", -91)
                op, mop = src.op, msk.op
                rng = np.random.default_rng(2000 * op + mop)
                tag = f"{ga_amd.OP_NAME[op]}-{ga_amd.OP_NAME[mop]}"
                src.put(S.gen_bits(op, NELEM, rng), rank)
                for k, (lo, hi) in enumerate(PACK_CASES):
                    st = mask_for(mop, NELEM, DENSITY[k % len(DENSITY)], rng, lo, hi)
                    msk.put(S.make_mask(mop, st, rng), rank)
                    inside = np.zeros(NELEM, dtype=bool)
                    inside[lo:hi + 1] = st[lo:hi + 1]
                    cnt = int(inside.sum())
                    for packed in (dst, other):   # the mask's own map, then another
                        packed.put(S.gen_bits(op, NELEM, rng), rank)
                        ic = ctypes.c_int(-1)
                        call(L, "GA_Pack", src.g, packed.g, msk.g, lo, hi, ctypes.byref(ic))
                        assert ic.value == cnt, (tag, lo, hi, ic.value, cnt)
                        packed.model[:cnt] = S.ref_pack(src.model, inside)
                        packed.check(f"GA_Pack {tag} irreg={irreg} lo={lo} hi={hi}")
                        digest(f"pack-{tag}-{lo}-{hi}", packed.model[:cnt])
                    # unpack `other` into dst: the set elements of [lo, hi] return, the rest stay
                    dst.put(S.gen_bits(op, NELEM, rng), rank)
                    ic = ctypes.c_int(-1)
                    call(L, "GA_Unpack", other.g, dst.g, msk.g, lo, hi, ctypes.byref(ic))
                    assert ic.value == cnt
                    dst.model = S.ref_unpack(other.model, inside, dst.model)
                    assert dst.model[inside].tobytes() == src.model[inside].tobytes()   # the round trip
                    dst.check(f"GA_Unpack {tag} irreg={irreg} lo={lo} hi={hi}")
                    other.check(f"GA_Unpack left the packed side alone {tag}")
                    digest(f"unpack-{tag}-{lo}-{hi}", dst.model)
                src.check(f"pack and unpack left src alone {tag}")
                for a in (src, dst, msk, other):
                    a.destroy()
    live_unchanged(L, live, "packs")


def enums(L, rank, size):
    """patch_enumc.c: start = inc = 1 over the whole array (complex (1, 1)); then a range that
    cuts inside blocks with a start and an increment that make the integers wrap"""
    live = L.gaamd_ga_live_arrays()
    start = {K.INT: 2 ** 31 - 5, K.LNG: 2 ** 63 - 9, K.FLT: 0.5, K.DBL: -1.0 / 3.0, K.DCP: complex(1.0 / 3.0, 2.0)}
    inc = {K.INT: 0x10001, K.LNG: 0x100000001, K.FLT: 0.25, K.DBL: 1.0 / 7.0, K.DCP: complex(1.0 / 7.0, -3.0)}
    for t in VALUE_TYPES:
        for irreg in (False, True):
            a = array(L, t, NELEM, size, irreg, b"enum")
            op = a.op
            rng = np.random.default_rng(3000 + op)
            one = complex(1, 1) if op in K.REAL else 1
            for lo, hi, s0, s1 in ((0, NELEM - 1, one, one), (NELEM // 4, NELEM // 2, start[op], inc[op])):
                a.put(K.gen(op, NELEM, rng), rank)
                call(L, "GA_Patch_enum", a.g, lo, hi, vp(K.scalar(op, s0)), vp(K.scalar(op, s1)))
                a.model[lo:hi + 1] = S.ref_enum(op, hi - lo + 1, 0, s0, s1)
                a.check(f"GA_Patch_enum {ga_amd.OP_NAME[op]} irreg={irreg} lo={lo} hi={hi}")
                digest(f"enum-{ga_amd.OP_NAME[op]}-{lo}-{hi}", a.model)
            a.destroy()
    live_unchanged(L, live, "enums")


def corners(L, rank, size):
    live = L.gaamd_ga_live_arrays()
    rng = np.random.default_rng(77)
    for t, mt in ((C_DBL, C_INT), (C_INT, C_SCPL), (C_DCPL, C_DBL)):
        op, mop = OP_OF[t], OP_OF[mt]
        tag = f"{ga_amd.OP_NAME[op]}-{ga_amd.OP_NAME[mop]}"
        # an array of 2 elements: on 3 ranks one rank owns nothing
        src, dst, msk = trio(L, t, mt, 2, size, False)
        if size == 3:
            owners = sum(all(h >= l for l, h in zip(lo, hi)) for lo, hi in blocks_of(L, msk.g, 1, size))
            assert owners < size
        src.put(S.gen_exact(op, 2, rng), rank)
        for st in (np.array([True, False]), np.array([False, True]), np.array([False, False])):
            msk.put(S.make_mask(mop, st, rng), rank)
            for fn, excl in ((S.ADD, 0), (S.EXCL, 1), (S.COPY, 0)):
                dst.put(K.gen(op, 2, rng), rank)
                if fn == S.COPY:
                    call(L, "GA_Scan_copy", src.g, dst.g, msk.g, 0, 1)
                else:
                    call(L, "GA_Scan_add", src.g, dst.g, msk.g, 0, 1, excl)
                scan_model(dst, fn, src, st, 0, 1)
                dst.check(f"2 elements {tag} {S.FN_NAME[fn]} {st}")
                digest(f"two-{tag}-{S.FN_NAME[fn]}-{st.tolist()}", dst.model)
            ic = ctypes.c_int(-1)
            dst.put(K.gen(op, 2, rng), rank)
            call(L, "GA_Pack", src.g, dst.g, msk.g, 0, 1, ctypes.byref(ic))
            assert ic.value == int(st.sum())
            dst.model[:ic.value] = S.ref_pack(src.model, st)
            dst.check(f"2 elements pack {tag} {st}")
        for a in (src, dst, msk):
            a.destroy()
        # a middle rank whose whole block holds no set element (the carry crosses it), a range
        # that excludes the last rank's block, a mask with none set, and g_dst of GA_Pack under
        # another map and exactly icount long
        # (these cases follow the block map, so they print no digest and draw from a stream of their own)
        n = 2400
        rng2, rng = rng, np.random.default_rng(78 + op)
        src, dst, msk = trio(L, t, mt, n, size, True, shift=11)
        blocks = blocks_of(L, msk.g, 1, size)
        src.put(S.gen_exact(op, n, rng), rank)
        st = rng.integers(0, 5, n) == 0
        if size == 3:
            st[blocks[1][0][0]:blocks[1][1][0] + 1] = False
            st[blocks[0][0][0] + 3] = True
        hi_cut = blocks[-1][0][0] - 1 if size > 1 else n - 7   # ends where the last rank's block begins
        for lo, hi, sset in ((0, n - 1, st), (5, hi_cut, st), (0, n - 1, np.zeros(n, dtype=bool))):
            msk.put(S.make_mask(mop, sset, rng), rank)
            for fn, excl in ((S.ADD, 0), (S.EXCL, 1), (S.COPY, 0)):
                dst.put(K.gen(op, n, rng), rank)
                if fn == S.COPY:
                    call(L, "GA_Scan_copy", src.g, dst.g, msk.g, lo, hi)
                else:
                    call(L, "GA_Scan_add", src.g, dst.g, msk.g, lo, hi, excl)
                scan_model(dst, fn, src, sset, lo, hi)
                dst.check(f"crossing {tag} {S.FN_NAME[fn]} lo={lo} hi={hi} set={int(sset.sum())}")
            inside = np.zeros(n, dtype=bool)
            inside[lo:hi + 1] = sset[lo:hi + 1]
            cnt = int(inside.sum())
            exact = array(L, t, max(cnt, 1), size, False, b"exact")
            exact.put(K.gen(op, max(cnt, 1), rng), rank)
            ic = ctypes.c_int(-1)
            call(L, "GA_Pack", src.g, exact.g, msk.g, lo, hi, ctypes.byref(ic))
            assert ic.value == cnt
            exact.model[:cnt] = S.ref_pack(src.model, inside)
            exact.check(f"GA_Pack into exactly icount elements {tag} lo={lo} hi={hi} count={cnt}")
            dst.put(K.gen(op, n, rng), rank)
            call(L, "GA_Unpack", exact.g, dst.g, msk.g, lo, hi, ctypes.byref(ic))
            assert ic.value == cnt
            dst.model = S.ref_unpack(exact.model, inside, dst.model)
            dst.check(f"GA_Unpack from exactly icount elements {tag} lo={lo} hi={hi}")
            exact.destroy()
        for a in (src, dst, msk):
            a.destroy()
        rng = rng2
    live_unchanged(L, live, "corners")


def aborts(L, rank, size, mode):
    src, dst, msk = GA(L, C_DBL, [100], b"src"), GA(L, C_DBL, [39], b"short"), GA(L, C_INT, [100], b"msk")
    st = np.zeros(100, dtype=bool)
    st[::3] = True
    st[[1, 2, 4, 5, 7, 8]] = True   # 40 set elements for a g_dst of 39
    assert int(st.sum()) == 40
    src.put(np.arange(100.0), rank)
    msk.put(st.astype(np.int32), rank)
    ic = ctypes.c_int(-1)
    print("ABORT EXPECTED", flush=True)
    L.GA_Pack(src.g, dst.g, msk.g, 0, 99, ctypes.byref(ic))
    print("NOT REACHED", flush=True)


if __name__ == "__main__":
    run([("enums", enums), ("scans", scans), ("packs", packs), ("corners", corners)], aborts)
