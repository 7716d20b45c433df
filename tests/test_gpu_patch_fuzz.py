"""Seeded random patch geometry through the kernels that compute on arrays in place
(ga_amd/csrc/gaamd_patch.hip, gaamd_select.hip, gaamd_transpose.hip), bit-exact against the
numpy restatements of test_gpu_ga_math.py and test_gpu_ga_elem.py.

Those files pin the arithmetic on a short list of shapes; this one draws the geometry, so that
every launch route of the shared host planner (patch_plan) and row decoder (patch_row) runs:
  * the vector width W = 16, 8 or 4 bytes, with at most one row level (LV == 1) and with the
    mixed-radix decode (LV == 0), on rows with a full chunk, with a tail, and with both;
  * the 64-thread block of the map kernels (W = 16 and every base and stride on 4 KiB);
  * more than 65535 rows: go_map launches once per 65535 rows and passes row0;
  * fill's chunk of 1024 vectors (rows of 1023, 1024, 1025 and 2 * 1024 + 1 vectors);
  * dot and select: a last workgroup with fewer than 8 items, more than 1024 workgroups;
  * the transposes with the 16-byte-vector path decided differently on the two sides.

A case is {op, count, geo, alias, name}: op the element type, count[] in elements with
dimension 0 contiguous, geo[k] = (buffer, bytes of the base past a 4 KiB boundary, byte strides
of dimensions 1..) for the operands c, a, b.  Bases are placed from dev.ptr, so the route of a
case does not depend on where the allocator put the buffer, and the route predictor (route())
needs no GPU: it takes ga_amd.patch_add_plan and the constants of go_map_w / launch_patch_dot.
The plan does not tell the block size, so the generator draws two classes in which it is known:
"aligned" (every base and stride a multiple of 4096: 64 threads exactly when W = 16) and
"unaligned" (the output's base off the 4 KiB boundary: 128 threads).

Everything is compared as raw bits over the whole downloaded buffer: the bytes before, between
and after the rows are the canary.  GAAMD_FUZZ_SEED shifts every seed; 0 is the suite's.
"""
import functools
import math
import os

import numpy as np
import pytest

import ga_amd
import test_gpu_ga_elem as E
import test_gpu_ga_math as K
import test_gpu_transpose as T
from test_gpu_ga_math import CPL, DBL, DCP, DT, FLT, INT, LNG, OPS, REAL, UNS

SEED = int(os.environ.get("GAAMD_FUZZ_SEED", "0")) * 100003
N_RANDOM = 240         # random cases per family, beside the directed ones
TR_DRAWS = 6           # shapes per pair of layouts and element size

PAGE = 4096
LIMIT = 4 << 20        # no operand spans more
TRAIL = 64             # canary bytes after the last element
BUF = LIMIT + 4 * PAGE
GRID_ROWS = 65535      # rows per launch of go_map
FILL_CHUNK = 1024      # vectors per block of k_patch_map<PatchFill>: 256 threads x 4
DOT_BS, DOT_ITEMS, FINAL_PASS = 256, 8, 1024
# bytes of a base past a 4 KiB boundary: 0, 4, 8, 16 and 48 bytes past a 16-byte boundary that
# is not a 4 KiB one, and the 4 KiB boundary itself
OFFS = [64, 68, 72, 80, 112, 0]
FAKE_PTRS = [0x7E0000000100 + (k << 32) for k in range(3)]   # the CPU tests' "allocations"

MAP_FNS = ["fill", "scale", "add", "abs", "add_const", "recip", "mul", "div", "max", "min"]
ARITY = {"fill": 1, "scale": 1, "abs": 1, "add_const": 1, "recip": 1, "select": 1, "dot": 2,
         "add": 3, "mul": 3, "div": 3, "max": 3, "min": 3}
ELEM_FN = {"abs": E.ABS, "add_const": E.ADD_CONST, "recip": E.RECIP, "mul": E.MUL, "div": E.DIV, "max": E.MAX,
           "min": E.MIN}


def widths(op):
    return [w for w in (4, 8, 16) if w >= DT[op].itemsize]


def map_chunk(fn, W, block):
    """vectors per block (go_map_w): fill 256 x 4; else 64 or 128 x 1, 128 x 2, 128 x 4"""
    return FILL_CHUNK if fn == "fill" else {16: block, 8: 256, 4: 512}[W]


# ---- cases --------------------------------------------------------------------------
def lead(ptr):
    """bytes from the allocation to the 4 KiB boundary the bases are counted from (at least
    one page of canary before it)"""
    return PAGE + (-ptr) % PAGE


def base_off(ptrs, g):
    return lead(ptrs[g[0]]) + g[1]


def span(esz, count, stride):
    return sum(s * (c - 1) for s, c in zip(stride, count[1:])) + count[0] * esz


def make_case(op, count, geo, alias="none", name=""):
    """alias: c is exactly a, b or both (the same base and strides, as gaamd_patch_add allows)"""
    geo = [(k, int(off), [int(s) for s in st]) for k, (off, st) in enumerate(geo)]
    if alias in ("a", "both"):
        geo[1] = geo[0]
    if alias in ("b", "both"):
        geo[2] = geo[0]
    esz = DT[op].itemsize
    for _, off, st in geo:
        assert len(st) == len(count) - 1 and span(esz, count, st) <= LIMIT and off in OFFS and all(s > 0 for s in st)
    return dict(op=op, count=[int(c) for c in count], geo=geo, alias=alias, name=name)


def draw_row(rng, esz, max_bytes):
    """elements of a row: log-uniform up to max_bytes, extra mass +-1 vector around 64 .. 1024"""
    if rng.random() < 0.35:
        w = int(rng.choice([x for x in (4, 8, 16) if x >= esz]))
        b = (int(rng.choice([64, 128, 256, 512, 1024])) + int(rng.integers(-1, 2))) * w
        if b <= max_bytes:
            return b // esz
    return max(1, int(np.exp(rng.uniform(0, np.log(max_bytes // esz)))))


def draw_strides(rng, esz, count, aligned, cont, tall=False):
    """cont[j]: level j continues the one before it exactly (mergeable); else it is padded
    (tall: by less than 16 bytes, which keeps 100000 rows under 4 MiB)"""
    st, unit = [], count[0] * esz
    for j, c in enumerate(count[1:]):
        if aligned:   # continuing needs unit % 4096 == 0: every level above a padded one can
            s = -(-unit // PAGE) * PAGE + (0 if cont[j] else PAGE * int(rng.integers(1, 3)))
        elif cont[j]:
            s = unit
        elif tall:
            s = unit + esz * int(rng.integers(1, max(2, 16 // esz)))
        else:
            s = unit + (16 * int(rng.integers(1, 5)) if rng.random() < 0.5 else esz * int(rng.integers(1, 6)))
        st.append(s)
        unit = s * c
    return st


def draw_case(rng, family, op, k):
    """family "map": rows up to 3 chunks of fill (the widest route), aliasing drawn from
    none / a / b / both; "red" (dot, select): rows up to 3 chunks of 256 vectors"""
    esz = DT[op].itemsize
    if rng.random() < 0.06:   # tall: rows of at most 16 bytes, 65536 .. 100000 of them in 1 .. 4 levels
        n0 = int(rng.integers(1, 16 // esz + 1))
        nd = int(rng.integers(2, 6))
        count = [int(c) for c in rng.choice([1, 2, 3, 5, 7], nd - 2)]
        count.append(-(-int(rng.integers(65536, 100001)) // int(np.prod(count))))
        count = [n0] + [int(c) for c in rng.permutation(count)]
        aligned, tall = False, True
    else:
        tall = False
        n0 = draw_row(rng, esz, 3 * (FILL_CHUNK if family == "map" else DOT_BS) * 16)
        nd = int(rng.integers(1, 8))
        rows_left = max(1, (256 << 10) // (n0 * esz))
        count = [n0]
        for _ in range(nd - 1):
            c = min(int(rng.choice([1, 1, 2, 2, 3, 4, 5, 7, 9, 16, 33])), rows_left)
            rows_left = max(1, rows_left // c)
            count.append(c)
        aligned = rng.random() < 0.25
    alias = str(rng.choice(["none", "none", "a", "b", "both"])) if family == "map" else "none"
    while True:
        if rng.random() < 0.12:       # every operand fully contiguous
            cont = [[True] * (nd - 1)] * 3
        else:
            shared = rng.random(nd - 1) < 0.3   # a level that continues on every operand merges
            cont = [[bool(shared[j] or rng.random() < 0.25) for j in range(nd - 1)] for _ in range(3)]
        strides = [draw_strides(rng, esz, count, aligned, cont[i], tall) for i in range(3)]
        if all(span(esz, count, st) <= LIMIT for st in strides):
            break
        j = int(np.argmax(count[1:])) + 1   # too large (4 KiB strides, tall patches): fewer rows
        count[j] = max(1, count[j] // 2)
    if aligned:
        offs = [0, 0, 0]
    else:   # the output's base is off the 4 KiB boundary; 4 and 8 put 8- and 16-byte elements
        offs = [int(rng.choice(OFFS[:5]))] + [int(rng.choice(OFFS)) for _ in range(2)]   # below their alignment
    return make_case(op, count, list(zip(offs, strides)), alias, f"{family}-rnd{k}-{ga_amd.OP_NAME[op]}")


def rows_case(op, W, lv, nvec, aligned=False, off=None, name=""):
    """rows of nvec W-byte vectors, padded differently on every operand: LV == 1 as 5 rows,
    LV == 0 as 3 x 2 rows in two levels that do not merge"""
    esz = DT[op].itemsize
    assert (nvec * W) % esz == 0
    rb = nvec * W
    geo = []
    for k in range(3):
        if aligned:
            s1 = -(-rb // PAGE) * PAGE + PAGE * (1 + k % 2)
            s2 = 3 * s1 + PAGE
            o = 0
        else:
            s1 = rb + (3 + k) * W
            s2 = 3 * s1 + (5 - k) * W
            o = 64 + {16: 0, 8: 8, 4: 4}[W] if off is None else off
        geo.append((o, [s1] if lv == 1 else [s1, s2]))
    count = [rb // esz, 5] if lv == 1 else [rb // esz, 3, 2]
    return make_case(op, count, geo, "none", name or f"rows-{ga_amd.OP_NAME[op]}-W{W}-LV{lv}-{nvec}v")


def tall_cases():
    """[k, rows] patches past the 65535 rows of one launch: rows of one 16-byte vector at stride
    32 (LV == 1), and row counts factored into two levels with a padded inner stride
    (LV == 0).  65537 and 2 * 65535 + 1 are primes, so the LV == 0 cases take the products next
    above them: 257 x 256 (a second launch of 257 rows) and 362 x 363 (three launches; rows of
    two 8-byte vectors at stride 24, which keeps the operand under 4 MiB)"""
    out = []
    for op, rows in zip((DCP, DBL, FLT, INT), (65535, 65536, 65537, 2 * 65535 + 1)):
        per = 16 // DT[op].itemsize
        sb = 48 if rows * 48 <= LIMIT else 32   # b with its own stride where it fits
        out.append(make_case(op, [per, rows], [(64, [32]), (64, [32]), (64, [sb])], "none",
                             f"tall-LV1-{rows}-{ga_amd.OP_NAME[op]}"))
    for op, (c1, c2), s0 in zip((LNG, CPL, DBL, FLT), ((255, 257), (256, 256), (257, 256), (362, 363)), (32, 32, 32, 24)):
        per = 16 // DT[op].itemsize
        geo = [(64, [s0, s0 * c1 + s0])] * 3
        out.append(make_case(op, [per, c1, c2], geo, "none", f"tall-LV0-{c1}x{c2}-{ga_amd.OP_NAME[op]}"))
    return out


def directed_cases(family):
    out = []
    chunks = (lambda W: (map_chunk("add", W, 128) + 1, FILL_CHUNK + 1)) if family == "map" else (lambda W: (257, 513))
    for op in OPS:
        for W in widths(op):
            for lv in (1, 0):
                for nvec in chunks(W):   # one vector past a chunk: a full chunk and a tail
                    out.append(rows_case(op, W, lv, nvec))
        if DT[op].itemsize >= 8:   # elements below their natural alignment: W = the element
            for off in ((68,) if DT[op].itemsize == 8 else (68, 72)):
                for lv in (1, 0):
                    out.append(rows_case(op, DT[op].itemsize, lv, 130, off=off,
                                         name=f"subnatural-{ga_amd.OP_NAME[op]}-off{off - 64}-LV{lv}"))
    if family == "map":
        # fill's chunk at every width: below it, exactly it, one past it, two chunks and one
        for W in (4, 8, 16):
            for i, nvec in enumerate((1023, 1024, 1025, 2 * 1024 + 1)):
                ops = [o for o in OPS if W in widths(o)]
                out.append(rows_case(ops[i % len(ops)], W, i % 2, nvec))
        # the 64-thread block: W = 16, every base and stride on 4 KiB
        for i, nvec in enumerate((63, 64, 65, 129)):
            for lv in (1, 0):
                out.append(rows_case(OPS[(2 * i + lv) % 6], 16, lv, nvec, aligned=True,
                                     name=f"block64-LV{lv}-{nvec}v"))
        out.append(make_case(DBL, [2 * 129], [(0, [])] * 3, "a", "block64-contiguous"))
    return out + tall_cases()


@functools.lru_cache(maxsize=None)
def cases(family):
    rng = np.random.default_rng({"map": 4100, "red": 4200}[family] + SEED)
    rnd = [draw_case(rng, family, OPS[k % 6], k) for k in range(N_RANDOM)]
    return directed_cases(family) + rnd


# ---- the route predictor ---------------------------------------------------------------
def route(fn, case, ptrs):
    """the launch route of fn on case, from the plan and the launchers' constants (no GPU).
    A plan of one operand passes it three times, of two (dot) passes c = a"""
    op, count, geo = case["op"], case["count"], case["geo"]
    used = {1: [geo[0]] * 3, 2: [geo[0], geo[0], geo[1]], 3: geo}[ARITY[fn]]   # c, a, b
    c, a, b = ((ptrs[g[0]] + base_off(ptrs, g), g[2]) for g in used)
    rc, p = ga_amd.patch_add_plan(op, a[0], a[1], b[0], b[1], c[0], c[1], count)
    assert rc == 0, (fn, case["name"], rc)
    W, rows, nvec = p["width"], p["rows"], p["nvec"]
    r = dict(W=W, LV=1 if p["levels"] <= 1 else 0, rows=rows, nvec=nvec)
    if fn in MAP_FNS:
        if all(g[1] == 0 and all(s % PAGE == 0 for s in g[2]) for g in used):
            block = 64 if W == 16 else 128          # "aligned"
        else:
            assert used[0][1] != 0, ("the generator draws two classes only", case["name"])
            block = 128                             # "unaligned"
        chunk = map_chunk(fn, W, block)
        r.update(block=block, chunk=chunk, launches=-(-rows // GRID_ROWS), full=nvec >= chunk, tail=nvec % chunk != 0)
    else:
        items = -(-nvec // DOT_BS) * rows
        nwg = -(-items // DOT_ITEMS)
        r.update(items=items, nwg=nwg, second_pass=nwg > FINAL_PASS, last_items=items - DOT_ITEMS * (nwg - 1))
    return r


def test_generator_reaches_every_route():
    """no GPU: what the GPU tests below are there to run is in their case lists, for every
    function, from the planner's own answer"""
    for fn in MAP_FNS:
        rs = [(c, route(fn, c, FAKE_PTRS)) for c in cases("map")]
        for op in OPS:
            for W in widths(op):
                for LV in (0, 1):
                    have = [r for c, r in rs if c["op"] == op and r["W"] == W and r["LV"] == LV]
                    what = (fn, ga_amd.OP_NAME[op], W, LV)
                    assert any(r["full"] for r in have), ("no row with a full chunk", what)
                    assert any(r["tail"] for r in have), ("no row with a tail", what)
                    assert any(r["full"] and r["tail"] for r in have), ("no full chunks followed by a tail", what)
        for LV in (0, 1):
            if fn != "fill":   # fill has one block size
                assert any(r["block"] == 64 and r["LV"] == LV for _, r in rs), (fn, "block 64", LV)
            assert any(r["launches"] >= 2 and r["LV"] == LV for _, r in rs), (fn, "two launches", LV)
            assert any(r["launches"] >= 3 and r["LV"] == LV for _, r in rs), (fn, "three launches", LV)
        if fn == "fill":
            for W in (4, 8, 16):
                assert {1023, 1024, 1025, 2049} <= {r["nvec"] for _, r in rs if r["W"] == W}, W
    for fn in ("dot", "select"):
        rs = [(c, route(fn, c, FAKE_PTRS)) for c in cases("red")]
        for op in OPS:
            for W in widths(op):
                for LV in (0, 1):
                    assert any(c["op"] == op and r["W"] == W and r["LV"] == LV for c, r in rs), (fn, op, W, LV)
        assert any(r["nvec"] % DOT_BS for _, r in rs)
        assert any(r["last_items"] < DOT_ITEMS for _, r in rs)
        assert any(r["second_pass"] for _, r in rs)
    # where the allocator puts the buffers does not change a route
    other = [p + 0x300 + 0x1000 * k for k, p in enumerate(FAKE_PTRS)]
    for c in cases("map"):
        assert route("add", c, other) == route("add", c, FAKE_PTRS), c["name"]


# ---- images and the comparison -----------------------------------------------------------
def prepare(case, ptrs, rng, small=None):
    """(element offsets of c, a, b in their buffers' images, {buffer: image}): the images hold
    valid elements at the patch's phase everywhere (K.make_buf)"""
    op, count = case["op"], case["count"]
    esz = DT[op].itemsize
    offs = [K.offsets(esz, base_off(ptrs, g), count, g[2]) for g in case["geo"]]
    nbytes = {}
    for g, o in zip(case["geo"], offs):
        nbytes[g[0]] = max(nbytes.get(g[0], 0), int(o.max()) + esz + TRAIL)
    first = {g[0]: base_off(ptrs, g) for g in reversed(case["geo"])}
    img = {b: K.make_buf(op, nb, first[b], rng, small) for b, nb in sorted(nbytes.items())}
    return offs, img


def compare(got, want):
    """None, or where two byte images differ"""
    if got.shape == want.shape and np.array_equal(got, want):
        return None
    if got.shape != want.shape:
        return f"{got.shape} against {want.shape}"
    d = np.flatnonzero(got != want)
    return f"{d.size} bytes differ, the first at {int(d[0])}, the last at {int(d[-1])}"


def model_fill(case, r, ptrs, img, fault=None):
    """what gaamd_patch_fill leaves in the output's image, launch by launch as go_map issues
    them; fault: a wrong kernel -- "row0" decodes blockIdx.y without row0, "tail" drops the
    chunk that is not full, "overrun" stores one whole vector past the row's end"""
    op = case["op"]
    esz = DT[op].itemsize
    W, rows, nvec = r["W"], r["rows"], r["nvec"]
    o = K.offsets(esz, base_off(ptrs, case["geo"][0]), case["count"], case["geo"][0][2]).reshape(rows, nvec * W // esz)
    val = K.ref_fill(op, 1, K.VALUE[op])[0]
    out = img.copy()
    for r0 in range(0, rows, GRID_ROWS):
        first = 0 if fault == "row0" else r0
        sel = o[first:first + min(GRID_ROWS, rows - r0)]
        if fault == "overrun":
            past = sel[:, -1:] + esz + np.arange(0, W, esz)
            K.put(out, past.reshape(-1), np.full(past.size, val))
        if fault == "tail":
            sel = sel[:, :nvec // FILL_CHUNK * FILL_CHUNK * W // esz]
        K.put(out, sel.reshape(-1), np.full(sel.size, val))
    return out


def test_checker_flags_wrong_kernels():
    """no GPU: the comparison of the GPU tests against numpy models of three wrong kernels, on
    the directed cases: every launch writing rows from 0, the tail chunk dropped, a whole vector
    stored past the row's end.  The model without a fault is what the tests expect"""
    rng = np.random.default_rng(1)
    seen = dict(row0=0, tail=0, overrun=0)
    for case in directed_cases("map"):
        r = route("fill", case, FAKE_PTRS)
        offs, img = prepare(case, FAKE_PTRS, rng)
        before = img[0]
        want = before.copy()
        K.put(want, offs[0], K.ref_fill(case["op"], offs[0].size, K.VALUE[case["op"]]))
        assert compare(model_fill(case, r, FAKE_PTRS, before), want) is None, case["name"]
        applies = dict(row0=r["launches"] >= 2, tail=r["tail"], overrun=True)
        for fault, on in applies.items():
            if on:
                assert compare(model_fill(case, r, FAKE_PTRS, before, fault), want), (fault, "went unnoticed", case["name"])
                seen[fault] += 1
    assert seen["row0"] >= 6 and seen["tail"] >= 8 and seen["overrun"] >= 8, seen


# ---- GPU -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bufs(gpu_lib):
    b = [ga_amd.DeviceBuffer(BUF) for _ in range(3)]
    for x in b:
        assert x.ptr % 256 == 0
    yield b
    for x in b:
        x.free()


def no_zero_divisor(op, x, bad):
    x = x.copy()
    x[bad] = complex(1, 1) if op in REAL else 1
    return x


def run_map(fn, case, devs, rng):
    """fn on one case: None, or what differs"""
    ptrs = [d.ptr for d in devs]
    op, count, geo = case["op"], case["count"], case["geo"]
    dt = DT[op]
    offs, img = prepare(case, ptrs, rng)
    (cb, _, cs), (ab, _, as_), (bb, _, bs) = geo
    pc, pa, pb = (ptrs[g[0]] + base_off(ptrs, g) for g in geo)
    n = offs[0].size
    if ARITY[fn] == 1:
        x = K.take(img[cb], offs[0], dt)
        if fn == "recip":
            bad = E.ref_elem1(op, E.RECIP, x)[1]
            if bad.any():   # zero divisors in the drawn data become 1 (1 + 1i)
                x = no_zero_divisor(op, x, bad)
                K.put(img[cb], offs[0], x)
        used = [cb]
        for b in used:
            devs[b].upload(img[b])
        if fn == "fill":
            rc, vals = ga_amd.patch_fill(op, K.VALUE[op], pc, cs, count), K.ref_fill(op, n, K.VALUE[op])
        elif fn == "scale":
            rc, vals = ga_amd.patch_scale(op, K.ALPHA[op], pc, cs, count), K.ref_scale(op, x, K.ALPHA[op])
        else:
            rc = ga_amd.patch_elem1(op, ELEM_FN[fn], pc, cs, count, scalar=E.CONST[op] if fn == "add_const" else None)
            vals, bad = E.ref_elem1(op, ELEM_FN[fn], x, E.CONST[op])
            assert not bad.any()
    else:
        a, b = K.take(img[ab], offs[1], dt), K.take(img[bb], offs[2], dt)
        if fn == "div":
            bad = E.ref_elem2(op, E.DIV, a, b)[1]
            if bad.any():
                K.put(img[bb], offs[2], no_zero_divisor(op, b, bad))
                a, b = K.take(img[ab], offs[1], dt), K.take(img[bb], offs[2], dt)   # a may be b
        used = sorted({cb, ab, bb})
        for k in used:
            devs[k].upload(img[k])
        if fn == "add":
            rc = ga_amd.patch_add(op, K.ALPHA[op], pa, as_, K.BETA[op], pb, bs, pc, cs, count)
            vals = K.ref_add(op, K.ALPHA[op], a, K.BETA[op], b)
        else:
            rc = ga_amd.patch_elem2(op, ELEM_FN[fn], pa, as_, pb, bs, pc, cs, count)
            vals, bad = E.ref_elem2(op, ELEM_FN[fn], a, b)
            assert not bad.any()
    if rc != 0:
        return f"returned {rc}"
    ga_amd.sync()
    want = img[cb].copy()
    K.put(want, offs[0], vals)
    err = compare(devs[cb].download(np.uint8, want.size), want)
    if err:
        return err
    for k in used:   # the inputs that are not the output are only read
        if k != cb and compare(devs[k].download(np.uint8, img[k].size), img[k]):
            return f"input buffer {k} changed"
    return None


def report(bad, total):
    assert not bad, "\n".join(f"{c['name']} {c['count']} {c['geo']} alias={c['alias']}: {e}" for c, e in bad[:5]) \
        + f"\n({len(bad)} of {total} cases differ)"


@pytest.mark.gpu
@pytest.mark.parametrize("fn", MAP_FNS)
def test_fuzz_map(gpu_lib, bufs, fn):
    """fill, scale, add and the element-wise functions on every directed and random case"""
    rng = np.random.default_rng(9100 + MAP_FNS.index(fn) + SEED)
    ptrs = [d.ptr for d in bufs]
    todo = cases("map")
    bad = []
    for case in todo:
        route(fn, case, ptrs)   # the plan accepts every generated case
        err = run_map(fn, case, bufs, rng)
        if err:
            bad.append((case, err))
    report(bad, len(todo))


def dot_small(op, n):
    """floats hold integers in [-s, s] with n * s^2 < 2^24 (f32) or 2^53 (f64) -- a complex
    element adds two products to each sum --, so every summation order gives the same bits"""
    if op in UNS:
        return None
    terms = n * (2 if op in REAL else 1)
    lim = (1 << 24) if op in (FLT, CPL) else (1 << 53)
    s = min(7, math.isqrt((lim - 1) // terms))
    assert s >= 1 and terms * s * s < lim
    return s


@pytest.mark.gpu
def test_fuzz_dot(gpu_lib, bufs):
    """exact sums (integers wrap; floats hold small integers) against numpy, each case twice"""
    rng = np.random.default_rng(9200 + SEED)
    ptrs = [d.ptr for d in bufs]
    todo = cases("red")
    bad = []
    for case in todo:
        route("dot", case, ptrs)
        op, count, geo = case["op"], case["count"], case["geo"]
        offs, img = prepare(case, ptrs, rng, dot_small(op, int(np.prod(count))))
        (ab, _, as_), (bb, _, bs) = geo[0], geo[1]
        for k in (ab, bb):
            bufs[k].upload(img[k])
        want = K.ref_dot_exact(op, K.take(img[ab], offs[0], DT[op]), K.take(img[bb], offs[1], DT[op]))
        for again in range(2):
            rc, got = ga_amd.patch_dot(op, ptrs[ab] + base_off(ptrs, geo[0]), as_, ptrs[bb] + base_off(ptrs, geo[1]), bs,
                                       count)
            if rc != 0 or got.tobytes() != want.tobytes():
                bad.append((case, f"run {again}: rc {rc}, got {got}, want {want}"))
        for k in (ab, bb):
            if compare(bufs[k].download(np.uint8, img[k].size), img[k]):
                bad.append((case, f"input buffer {k} changed"))
    report(bad, len(todo))


def select_plants(case, rng):
    """lists of element indices that get the extremum: the first and the last element, a drawn
    one; in the tall cases rows 65534, 65535 and 65536, each with a duplicate on the other
    side of row 65535 where there is one"""
    count = case["count"]
    n, rows = int(np.prod(count)), int(np.prod(count[1:]))
    out = [[0], [n - 1], [int(rng.integers(0, n))]]
    if rows >= GRID_ROWS:
        pairs = [(65534, 65535), (65535, 65534 + GRID_ROWS), (65536, 12)] if rows > GRID_ROWS else [(65534, 100)]
        for ra, rb in pairs:
            at = [r * count[0] + int(rng.integers(0, count[0])) for r in (ra, rb) if r < rows]
            out.append(sorted(set(at)))
    return out


@pytest.mark.gpu
def test_fuzz_select(gpu_lib, bufs):
    """distinct keys with the extremum planted: the index is numpy's first occurrence, the
    element has that occurrence's bits, the buffer is only read"""
    rng = np.random.default_rng(9300 + SEED)
    dev = bufs[0]
    ptrs = [d.ptr for d in bufs]
    todo = cases("red")
    bad = []
    for case in todo:
        route("select", case, ptrs)
        op, count, g = case["op"], case["count"], case["geo"][0]
        dt = DT[op]
        offs, img = prepare(case, ptrs, rng)
        o, im = offs[0], img[0]
        x = E.distinct(op, o.size, rng)
        K.put(im, o, x)
        dev.upload(im)
        base = ptrs[0] + base_off(ptrs, g)
        for want_max in (0, 1):
            for at in select_plants(case, rng):
                y = x.copy()
                for k, i in enumerate(at):
                    y[i] = E.extreme(op, want_max, k)
                    dev.upload(y[i:i + 1], offset=int(o[i]))
                i, val, key = E.ref_select(op, want_max, y)
                assert i == at[0]
                rc, gval, gkey, gi = ga_amd.patch_select(op, want_max, base, g[2], count)
                if (rc, gi, gval.tobytes(), gkey.tobytes()) != (0, i, val.tobytes(), key.tobytes()):
                    bad.append((case, f"{'max' if want_max else 'min'} planted at {at}: rc {rc}, index {gi}, {gval}"))
                for i in at:
                    dev.upload(x[i:i + 1], offset=int(o[i]))
        if compare(dev.download(np.uint8, im.size), im):
            bad.append((case, "the buffer changed"))
    report(bad, len(todo))


# ---- transposes: the layout of each side drawn on its own ---------------------------------
LAYOUT_PAIRS = [(a, b) for a in T.LAYOUTS for b in T.LAYOUTS]


def side_is_vector(mat):
    return mat.ptr % 16 == 0 and (mat.ld * 4 * mat.w) % 16 == 0


@pytest.mark.gpu
@pytest.mark.parametrize("op", [T.INT, T.DBL, T.DCP], ids=["4B", "8B", "16B"])
def test_fuzz_transpose(gpu_lib, bufs, op):
    """rows and cols from 1 to 3T + 3, all 16 pairs of source and destination layout"""
    rng = np.random.default_rng(9400 + op + SEED)
    t, w = T.tile(op), T.ESZ[op] // 4
    sides = set()
    for ls, ld in LAYOUT_PAIRS * TR_DRAWS:
        rows, cols = (int(v) for v in rng.integers(1, 3 * t + 4, 2))
        src = T.Mat(bufs[0], rows, cols, w, ls, lambda s: rng.integers(0, 1 << 32, s, dtype=np.uint32))
        dst = T.Mat(bufs[1], cols, rows, w, ld, T.sentinel)
        sides.add((side_is_vector(src), side_is_vector(dst)))
        src.upload()
        dst.upload()
        what = (op, rows, cols, ls, ld)
        assert ga_amd.transpose(op, rows, cols, src.ptr, src.ld, dst.ptr, dst.ld) == 0, what
        ga_amd.sync()
        got = T.unchanged_but(dst, dst.download())
        assert got.tobytes() == np.ascontiguousarray(src.view().transpose(1, 0, 2)).tobytes(), what
        assert src.download().tobytes() == src.img.tobytes(), ("the source changed", what)
    if w < 4:   # a 16-byte element is its own vector: one path
        assert sides == {(False, False), (False, True), (True, False), (True, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("op", [T.DBL, T.FLT], ids=["f64", "f32"])
def test_fuzz_transpose_acc(gpu_lib, bufs, op):
    """c = alpha * (c + b^T) with the layouts of b and c drawn on their own"""
    rng = np.random.default_rng(9500 + op + SEED)
    dt = ga_amd.OP_DTYPE[op]
    t, w = T.tile(op), dt.itemsize // 4
    sides = set()
    for lb, lc in LAYOUT_PAIRS * TR_DRAWS:
        m, n = (int(v) for v in rng.integers(1, 3 * t + 4, 2))
        alpha = float(rng.choice([0.5, -3.0]))
        cv = (rng.standard_normal((m, n)) * 10.0 ** rng.integers(-3, 4, (m, n))).astype(dt)
        bv = (rng.standard_normal((n, m)) * 10.0 ** rng.integers(-3, 4, (n, m))).astype(dt)
        b = T.Mat(bufs[0], n, m, w, lb, T.sentinel)
        c = T.Mat(bufs[1], m, n, w, lc, T.sentinel)
        b.view()[:] = T.words(bv)
        c.view()[:] = T.words(cv)
        sides.add((side_is_vector(b), side_is_vector(c)))
        b.upload()
        c.upload()
        what = (op, m, n, alpha, lb, lc)
        assert ga_amd.transpose_acc(op, m, n, alpha, b.ptr, b.ld, c.ptr, c.ld) == 0, what
        ga_amd.sync()
        got = T.unchanged_but(c, c.download())
        want = dt.type(alpha) * (cv + bv.T)   # stays in dt: one add, one multiply
        assert want.dtype == dt and got.tobytes() == T.words(want).tobytes(), what
        assert b.download().tobytes() == b.img.tobytes(), ("b changed", what)
    assert sides == {(False, False), (False, True), (True, False), (True, True)}
