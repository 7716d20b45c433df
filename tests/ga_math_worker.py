"""One rank of the GA_Fill / GA_Scale / GA_Add / GA_Copy / GA_?dot tests
(test_gpu_ga_math_mp.py starts 1, 2 or 3 of these on one GPU).

Modes:
  all         whole-array calls, patch forms, the general path, ordering against a
              pending NGA_NbAcc -- each section prints "SECTION <name> OK"
  big         a 1-D C_DBL array of 2**29 + 3 elements: 64-bit offsets
  tall        C_DBL and C_FLOAT arrays of [70001 * ranks + 1, 3]: every rank's part of the
              patch has more than 65535 rows, so the map kernels take a second launch
  abort-type / abort-trans / abort-host
              a call that must end the process through GA_Error; prints
              "ABORT EXPECTED" just before it and "NOT REACHED" if it returns
Expected values: the numpy restatement of global.npatch.c in test_gpu_ga_math.py.
Prints "RANK <r> OK" on success and "DOT <case> <hex>" for every dot product, which
the launcher compares across ranks.
"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import ga_amd  # noqa: E402
import test_gpu_ga_math as K  # noqa: E402

from ga_worker import (C_DBL, C_DCPL, C_FLOAT, C_INT, C_LONG, C_SCPL, DOT_OF, GA, OP_OF, blocks_of, flat, ia, run,  # noqa: E402
                       sl, vp)


def dot_call(L, t, ga, gb, patch=None):
    """GA_?dot or NGA_?dot_patch as a one-element numpy array of the type"""
    dt = K.DT[OP_OF[t]]
    if patch is None:
        v = getattr(L, f"GA_{DOT_OF[t]}dot")(ga, gb)
    else:
        alo, ahi, blo, bhi = patch
        v = getattr(L, f"NGA_{DOT_OF[t]}dot_patch")(ga, b"N", ia(alo), ia(ahi), gb, b"N", ia(blo), ia(bhi))
    if t in (C_SCPL, C_DCPL):
        return np.array([complex(v.real, v.imag)], dtype=dt)
    return np.array([v], dtype=dt)


def say_dot(case, v):
    print(f"DOT {case} {v.tobytes().hex()}", flush=True)


# ---- sections ---------------------------------------------------------------------
def whole_array(L, rank, size):
    for dims in ([67, 45], [9, 10, 11]):
        n = int(np.prod(dims))
        for t in (C_INT, C_LONG, C_FLOAT, C_DBL, C_SCPL, C_DCPL):
            op = OP_OF[t]
            rng = np.random.default_rng(100 * t + len(dims))
            a, b, c = (GA(L, t, dims, nm) for nm in (b"a", b"b", b"c"))
            a.put(K.gen(op, n, rng), rank)
            b.put(K.gen(op, n, rng), rank)
            tag = f"{ga_amd.OP_NAME[op]} {dims}"
            val, al, be = K.scalar(op, K.VALUE[op]), K.scalar(op, K.ALPHA[op]), K.scalar(op, K.BETA[op])
            L.GA_Fill(c.g, vp(val))
            c.model = K.ref_fill(op, n, K.VALUE[op]).reshape(dims)
            c.check(f"GA_Fill {tag}")
            L.GA_Scale(a.g, vp(al))
            a.model = K.ref_scale(op, flat(a.model), K.ALPHA[op]).reshape(dims)
            a.check(f"GA_Scale {tag}")
            L.GA_Add(vp(al), a.g, vp(be), b.g, c.g)
            c.model = K.ref_add(op, K.ALPHA[op], flat(a.model), K.BETA[op], flat(b.model)).reshape(dims)
            c.check(f"GA_Add {tag}")
            a.check(f"GA_Add left a alone {tag}")
            L.GA_Add(vp(al), a.g, vp(be), b.g, a.g)   # g_c == g_a
            a.model = c.model.copy()
            a.check(f"GA_Add in place {tag}")
            b.check(f"GA_Add left b alone {tag}")
            L.GA_Zero(c.g)
            L.GA_Copy(a.g, c.g)
            c.model = a.model.copy()
            c.check(f"GA_Copy {tag}")
            # dot: exact data (integers wrap; floats hold small integers) against numpy, then
            # random data, which only has to be the same bits on every rank
            small = None if op in K.UNS else 5
            a.put(K.gen(op, n, rng, small), rank)
            b.put(K.gen(op, n, rng, small), rank)
            got = dot_call(L, t, a.g, b.g)
            want = K.ref_dot_exact(op, flat(a.model), flat(b.model))
            assert got.tobytes() == want.tobytes(), (f"GA_{DOT_OF[t]}dot {tag}", got, want)
            a.put(K.gen(op, n, rng), rank)
            say_dot(f"whole-{ga_amd.OP_NAME[op]}-{len(dims)}d", dot_call(L, t, a.g, b.g))
            for x in (a, b, c):
                x.destroy()


def patch_forms(L, rank, size):
    dims = [67, 45]
    n = dims[0] * dims[1]
    for t in (C_DBL, C_SCPL, C_INT):
        op = OP_OF[t]
        rng = np.random.default_rng(7 * t)
        a, b, c = (GA(L, t, dims, nm) for nm in (b"a", b"b", b"c"))
        blk = blocks_of(L, a.g, 2, size)
        b0lo, b0hi = blk[0]
        assert all(h - l >= 2 for l, h in zip(b0lo, b0hi)), blk
        # the bounding box of every rank's block but the last one's, one element in
        some_lo = [min(blk[q][0][d] for q in range(max(1, size - 1))) + 1 for d in range(2)]
        some_hi = [max(blk[q][1][d] for q in range(max(1, size - 1))) - 1 for d in range(2)]
        patches = {
            "inside one block": ([x + 1 for x in b0lo], [x - 1 for x in b0hi]),
            "all blocks": ([1, 1], [65, 43]),
            "some blocks": (some_lo, some_hi),
            "one element": ([33, 22], [33, 22]),
        }
        if size > 1:
            touched = [all(some_lo[d] <= blk[q][1][d] and blk[q][0][d] <= some_hi[d] for d in range(2))
                       for q in range(size)]
            assert any(touched) and not all(touched), (blk, some_lo, some_hi)
        val, al, be = K.scalar(op, K.VALUE[op]), K.scalar(op, K.ALPHA[op]), K.scalar(op, K.BETA[op])
        for name, (lo, hi) in patches.items():
            tag = f"{ga_amd.OP_NAME[op]} {name} {lo}..{hi}"
            s = sl(lo, hi)
            shape = a.model[s].shape
            a.put(K.gen(op, n, rng), rank)
            b.put(K.gen(op, n, rng), rank)
            c.put(K.gen(op, n, rng), rank)
            L.NGA_Fill_patch(c.g, ia(lo), ia(hi), vp(val))
            c.model[s] = K.scalar(op, K.VALUE[op])[0]
            c.check(f"NGA_Fill_patch {tag}")
            L.NGA_Scale_patch(a.g, ia(lo), ia(hi), vp(al))
            a.model[s] = K.ref_scale(op, flat(a.model[s]), K.ALPHA[op]).reshape(shape)
            a.check(f"NGA_Scale_patch {tag}")
            L.NGA_Add_patch(vp(al), a.g, ia(lo), ia(hi), vp(be), b.g, ia(lo), ia(hi), c.g, ia(lo), ia(hi))
            c.model[s] = K.ref_add(op, K.ALPHA[op], flat(a.model[s]), K.BETA[op], flat(b.model[s])).reshape(shape)
            c.check(f"NGA_Add_patch {tag}")
            L.NGA_Copy_patch(b"N", c.g, ia(lo), ia(hi), b.g, ia(lo), ia(hi))
            b.model[s] = c.model[s]
            b.check(f"NGA_Copy_patch {tag}")
            L.NGA_Zero_patch(a.g, ia(lo), ia(hi))
            a.model[s] = 0
            a.check(f"NGA_Zero_patch {tag}")
            small = None if op in K.UNS else 5
            a.put(K.gen(op, n, rng, small), rank)
            b.put(K.gen(op, n, rng, small), rank)
            got = dot_call(L, t, a.g, b.g, (lo, hi, lo, hi))
            want = K.ref_dot_exact(op, flat(a.model[s]), flat(b.model[s]))
            assert got.tobytes() == want.tobytes(), (f"dot_patch {tag}", got, want)
        for x in (a, b, c):
            x.destroy()


def general_path(L, rank, size):
    dims = [67, 45]
    n = dims[0] * dims[1]
    t, op = C_DBL, K.DBL
    rng = np.random.default_rng(99)
    live0 = L.gaamd_ga_live_arrays()
    a, c = GA(L, t, dims, b"a"), GA(L, t, dims, b"c")
    starts = [0, 10, 50][:size]
    b = GA(L, t, dims, b"irreg", irreg=([size, 1], starts + [0]))
    assert (L.GA_Compare_distr(a.g, c.g) == 0) and (size == 1 or L.GA_Compare_distr(a.g, b.g) == 1)
    ty, nd, dd = ctypes.c_int(), ctypes.c_int(), (ctypes.c_int * 7)()
    L.NGA_Inquire(b.g, ctypes.byref(ty), ctypes.byref(nd), dd)
    assert (ty.value, nd.value, list(dd)[:2]) == (t, 2, dims)
    live = L.gaamd_ga_live_arrays()
    assert live == live0 + 3
    al, be = K.scalar(op, 1.5), K.scalar(op, -0.25)
    a.put(K.gen(op, n, rng), rank)
    b.put(K.gen(op, n, rng), rank)
    c.put(K.gen(op, n, rng), rank)
    # g_b on another block map
    L.GA_Add(vp(al), a.g, vp(be), b.g, c.g)
    c.model = K.ref_add(op, 1.5, flat(a.model), -0.25, flat(b.model)).reshape(dims)
    c.check("GA_Add with g_b on another map")
    a.check("a unchanged")
    b.check("b unchanged")
    L.GA_Copy(b.g, a.g)
    a.model = b.model.copy()
    a.check("GA_Copy from another map")
    a.put(K.gen(op, n, rng, 6), rank)
    b.put(K.gen(op, n, rng, 6), rank)
    got = dot_call(L, t, a.g, b.g)
    assert got.tobytes() == K.ref_dot_exact(op, flat(a.model), flat(b.model)).tobytes(), ("GA_Ddot other map", got)
    # the a patch shifted against c (b on c's patch, on the regular map this time)
    b.destroy()
    b = GA(L, t, dims, b"b")
    a.put(K.gen(op, n, rng), rank)
    b.put(K.gen(op, n, rng), rank)
    c.put(K.gen(op, n, rng), rank)
    alo, ahi, clo, chi = [2, 3], [40, 30], [20, 5], [58, 32]
    L.NGA_Add_patch(vp(al), a.g, ia(alo), ia(ahi), vp(be), b.g, ia(clo), ia(chi), c.g, ia(clo), ia(chi))
    sa, sc = sl(alo, ahi), sl(clo, chi)
    c.model[sc] = K.ref_add(op, 1.5, flat(a.model[sa]), -0.25, flat(b.model[sc])).reshape(c.model[sc].shape)
    c.check("NGA_Add_patch with a shifted")
    a.check("a unchanged by the shifted add")
    b.check("b unchanged by the shifted add")
    # in place on a shifted patch of the same array: c = 1.5 * c[shifted] - 0.25 * b
    L.NGA_Add_patch(vp(al), c.g, ia(alo), ia(ahi), vp(be), b.g, ia(clo), ia(chi), c.g, ia(clo), ia(chi))
    c.model[sc] = K.ref_add(op, 1.5, flat(c.model[sa].copy()), -0.25, flat(b.model[sc])).reshape(c.model[sc].shape)
    c.check("NGA_Add_patch of a shifted patch of c itself")
    # copy to a shifted position
    L.NGA_Copy_patch(b"N", a.g, ia(alo), ia(ahi), b.g, ia(clo), ia(chi))
    b.model[sc] = a.model[sa]
    b.check("NGA_Copy_patch shifted")
    # dot of shifted patches
    a.put(K.gen(op, n, rng, 6), rank)
    b.put(K.gen(op, n, rng, 6), rank)
    got = dot_call(L, t, a.g, b.g, (alo, ahi, clo, chi))
    want = K.ref_dot_exact(op, flat(a.model[sa]), flat(b.model[sc]))
    assert got.tobytes() == want.tobytes(), ("NGA_Ddot_patch shifted", got, want)
    a.put(K.gen(op, n, rng), rank)
    say_dot("shifted-dbl", dot_call(L, t, a.g, b.g, (alo, ahi, clo, chi)))
    a.check("a unchanged by the dot")
    b.check("b unchanged by the dot")
    assert L.gaamd_ga_live_arrays() == live, "a temporary of the general path is still alive"
    for x in (a, b, c):
        x.destroy()
    assert L.gaamd_ga_live_arrays() == live0


def ordering(L, rank, size):
    """an NGA_NbAcc still pending when GA_Scale is called: acc-then-scale"""
    dims = [67, 45]
    a = GA(L, C_DBL, dims, b"a")
    a.put(np.arange(67 * 45, dtype=np.float64), rank)
    blk = blocks_of(L, a.g, 2, size)
    lo, hi = blk[(rank + 1) % size]
    shape = [h - l + 1 for l, h in zip(lo, hi)]
    buf = np.full(shape, float(rank + 1))
    one, three = np.array([1.0]), np.array([3.0])
    h = ctypes.c_long(0)
    L.NGA_NbAcc(a.g, ia(lo), ia(hi), vp(buf), ia(shape[1:]), vp(one), ctypes.byref(h))
    L.GA_Scale(a.g, vp(three))   # no wait before it
    L.NGA_NbWait(ctypes.byref(h))
    for q in range(size):
        qlo, qhi = blk[(q + 1) % size]
        a.model[sl(qlo, qhi)] += float(q + 1)
    a.model = a.model * 3.0
    a.check("NGA_NbAcc then GA_Scale")
    a.destroy()


def big(L, rank, size):
    n = (1 << 29) + 3
    g = L.NGA_Create(C_DBL, 1, ia([n]), b"big", None)
    assert g > 0
    one = np.array([1.0])
    L.GA_Fill(g, vp(one))
    d = L.GA_Ddot(g, g)
    assert d == float(n), d
    for first in (n - 3, (1 << 29) - 1):   # the last three; three straddling byte offset 2**32
        out = np.zeros(3)
        L.NGA_Get(g, ia([first]), ia([first + 2]), vp(out), ia([1]))
        assert out.tolist() == [1.0, 1.0, 1.0], (first, out)
    two = np.array([2.0])
    L.GA_Scale(g, vp(two))
    assert L.GA_Ddot(g, g) == 4.0 * n
    L.GA_Destroy(g)


def tall(L, rank, size):
    """a patch of two of the three columns without the first and the last row: rows of two
    elements, more than 65535 of them on every rank (go_map's second launch, row0 != 0)"""
    rows = 70001 * size + 1
    dims = [rows, 3]
    n = rows * 3
    lo, hi = [1, 0], [rows - 2, 1]
    s = sl(lo, hi)
    for t in (C_DBL, C_FLOAT):
        op = OP_OF[t]
        rng = np.random.default_rng(31 * t)
        a, b, c = (GA(L, t, dims, nm) for nm in (b"a", b"b", b"c"))
        mylo, myhi = blocks_of(L, a.g, 2, size)[rank]
        own = min(myhi[0], hi[0]) - max(mylo[0], lo[0]) + 1
        assert own > 65535 and mylo[1] <= lo[1] and myhi[1] >= hi[1], (mylo, myhi, own)
        tag = f"{ga_amd.OP_NAME[op]} {dims} {lo}..{hi}"
        shape = a.model[s].shape
        val, al, be = K.scalar(op, K.VALUE[op]), K.scalar(op, K.ALPHA[op]), K.scalar(op, K.BETA[op])
        a.put(K.gen(op, n, rng), rank)
        b.put(K.gen(op, n, rng), rank)
        c.put(K.gen(op, n, rng), rank)
        L.NGA_Fill_patch(c.g, ia(lo), ia(hi), vp(val))
        c.model[s] = K.scalar(op, K.VALUE[op])[0]
        c.check(f"NGA_Fill_patch {tag}")
        L.NGA_Scale_patch(a.g, ia(lo), ia(hi), vp(al))
        a.model[s] = K.ref_scale(op, flat(a.model[s]), K.ALPHA[op]).reshape(shape)
        a.check(f"NGA_Scale_patch {tag}")
        L.NGA_Add_patch(vp(al), a.g, ia(lo), ia(hi), vp(be), b.g, ia(lo), ia(hi), c.g, ia(lo), ia(hi))
        c.model[s] = K.ref_add(op, K.ALPHA[op], flat(a.model[s]), K.BETA[op], flat(b.model[s])).reshape(shape)
        c.check(f"NGA_Add_patch {tag}")
        a.check(f"NGA_Add_patch left a alone {tag}")
        b.check(f"NGA_Add_patch left b alone {tag}")
        a.put(K.gen(op, n, rng, 5), rank)   # f32: 25 * 2 * (rows - 2) < 2**24, every sum exact
        b.put(K.gen(op, n, rng, 5), rank)
        got = dot_call(L, t, a.g, b.g, (lo, hi, lo, hi))
        want = K.ref_dot_exact(op, flat(a.model[s]), flat(b.model[s]))
        assert got.tobytes() == want.tobytes(), (f"NGA_{DOT_OF[t]}dot_patch {tag}", got, want)
        say_dot(f"tall-{ga_amd.OP_NAME[op]}", got)
        L.GA_Fill(c.g, vp(val))
        c.model = K.ref_fill(op, n, K.VALUE[op]).reshape(dims)
        c.check(f"GA_Fill {tag}")
        for x in (a, b, c):
            x.destroy()


def aborts(L, rank, size, mode):
    dims = [20, 30]
    if mode == "abort-type":
        f = GA(L, C_FLOAT, dims, b"f")
        print("ABORT EXPECTED", flush=True)
        L.GA_Ddot(f.g, f.g)
    elif mode == "abort-trans":
        a, b = GA(L, C_DBL, dims, b"a"), GA(L, C_DBL, dims, b"b")
        print("ABORT EXPECTED", flush=True)
        L.NGA_Copy_patch(b"T", a.g, ia([0, 0]), ia([9, 9]), b.g, ia([0, 0]), ia([9, 9]))
    elif mode == "abort-host":
        a = GA(L, C_DBL, dims, b"hostseg")
        one = np.array([1.0])
        print("ABORT EXPECTED", flush=True)
        L.GA_Fill(a.g, vp(one))
    print("NOT REACHED", flush=True)


if __name__ == "__main__":
    run([("whole", whole_array), ("patch", patch_forms), ("general", general_path), ("order", ordering)], aborts,
        bare={"big": big, "tall": tall})
