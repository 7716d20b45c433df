"""Seeded cases for the differential fuzz of the GA caller layer (ga_amd/csrc/ga.cpp), and the
numpy model they are compared with.  No GPU: tests/test_ga_fuzz_cases.py checks the generator,
tests/ga_fuzz_worker.py runs the cases (test_gpu_ga_fuzz_mp.py starts 1 to 4 of it).

cases(seed, size) is a pure function: every rank calls it and gets the same list.  A case is a
plain dict (ints, strings, lists) that says everything: the call, the arrays with their type,
dims, data kind and block map, which array plays which role, the patches, the scalars.

What is drawn in two layers:
  logical  call, type, dims, patches, scalars, data seed -- from (seed) alone, so case i is the
           same computation on every rank count and its scalar results (dots, norms, selected
           element, icount) have to be the same bits on 1, 2, 3 and 4 ranks;
  maps     from (seed, size): NGA_Create with chunk None, NGA_Create with a drawn chunk, or
           NGA_Create_irreg with an explicit grid and strictly increasing starts.  A patch class
           that speaks of blocks (inside one block, crossing exactly one cut by one element,
           leaving a rank with nothing) is made true by drawing the irregular cuts around the
           patch, which is how the patch can stay the same on every rank count.
Coverage does not hang on luck: calls come from a fixed plan, and types, map kinds, operand
relations, patch classes, transposes and mask patterns from shuffled decks that are dealt out
before they are refilled.

The model restates nothing: it applies the restatements of test_gpu_ga_math (K), test_gpu_ga_elem
(E), test_gpu_matrix (M) and test_gpu_scan (S) to whole numpy arrays in C order.  gemm is the
int64 product of integer data in [-8, 8] with alpha 2 and beta -3, |c| <= 2 * 64 * k + 24 < 2^24
for k <= 40 (test_gpu_gemm.exact_case's argument), transpose is .T, symmetrize the expression
of ga.h.  Where a result depends on summation order the data are exactly summable and the model
asserts it (M.exactly_summable, S.exact_in_range, the bound above; the dots use K.gen's small
integers, |sum| <= 2 * 25 * 20000 < 2^24), so every comparison is bit for bit.
"""
import itertools

import numpy as np

import ga_amd
import test_gpu_ga_elem as E
import test_gpu_ga_math as K
import test_gpu_matrix as M
import test_gpu_scan as S
from ga_worker import C_DBL, C_DCPL, C_FLOAT, C_INT, C_LONG, C_SCPL, OP_OF, flat, sl

TYPES = [C_INT, C_LONG, C_FLOAT, C_DBL, C_SCPL, C_DCPL]
KINDS = ["regular", "chunk", "irreg"]
# operand relations of the calls with two or three arrays
RELATIONS = ["same", "shifted", "othermap", "c_is_a", "c_is_b", "self_shifted"]
# patch classes; the last three speak of blocks and force an irregular map on 2 ranks or more
PCLASSES = ["whole", "one", "rowcol", "last", "inside", "cross1", "norank"]
BLOCKY = ("inside", "cross1", "norank")
MAX_4D = 20000
GEMM_MAX = 40
TRANS = ["NN", "NT", "TN", "TT"]
MASK_PATTERNS = ["none", "all", "first", "last", "single", "half", "sparse"]

ELEM1 = {"GA_Abs_value": E.ABS, "GA_Add_constant": E.ADD_CONST, "GA_Recip": E.RECIP}
ELEM2 = {"GA_Elem_multiply": E.MUL, "GA_Elem_divide": E.DIV, "GA_Elem_maximum": E.MAX, "GA_Elem_minimum": E.MIN}
DIAG = ["GA_Shift_diagonal", "GA_Set_diagonal", "GA_Zero_diagonal", "GA_Add_diagonal", "GA_Get_diag"]

# (family, call, how often per round of the plan)
_PLAN = (
    [("math", c, 1) for c in ("GA_Fill", "GA_Scale", "GA_Zero", "NGA_Fill_patch", "NGA_Scale_patch", "NGA_Zero_patch")]
    + [("math", "GA_Add", 1), ("math", "NGA_Add_patch", 4), ("math", "GA_Copy", 1), ("math", "NGA_Copy_patch", 3),
       ("math", "GA_dot", 1), ("math", "NGA_dot_patch", 3)]
    + [("elem", c, 1) for c in ELEM1] + [("elem", c + "_patch", 1) for c in ELEM1]
    + [("elem", c, 1) for c in ELEM2] + [("elem", c + "_patch", 2) for c in ELEM2]
    + [("elem", "NGA_Select_elem", 2)]
    + [("gemm", "GA_Dgemm", 2), ("gemm", "GA_Sgemm", 2), ("gemm", "NGA_Matmul_patch", 4)]
    + [("trans", "GA_Transpose", 6), ("trans", "GA_Symmetrize", 2)]
    + [("matrix", c, 1) for c in DIAG]
    + [("matrix", "GA_Scale_rows", 2), ("matrix", "GA_Scale_cols", 2), ("matrix", "GA_Norm1", 2),
       ("matrix", "GA_Norm_infinity", 2)]
    + [("scan", "GA_Patch_enum", 2), ("scan", "GA_Scan_copy", 3), ("scan", "GA_Scan_add", 4), ("scan", "GA_Pack", 3),
       ("scan", "GA_Unpack", 3)]
)
ROUNDS = 2
PLAN = [(f, c, None) for _ in range(ROUNDS) for f, c, k in _PLAN for _ in range(k)]
# the relations the plan above does not draw: g_c of a matrix multiply in the array of an input
PLAN += [("gemm", "NGA_Matmul_patch", rel) for _ in range(ROUNDS) for rel in ("c_is_a", "c_is_b")]
CALLS = sorted({c for _, c, _ in _PLAN})
FAMILIES = ["math", "elem", "gemm", "trans", "matrix", "scan"]
FAMILY_TYPES = {"math": TYPES, "elem": TYPES, "gemm": [C_FLOAT, C_DBL], "trans": TYPES, "matrix": TYPES, "scan": TYPES}


def scan_tile():
    """the largest tile of the scan kernels over the type pairs (a host-side constant of the library)"""
    return max(ga_amd.scan_tile(op, mop) for op in K.OPS for mop in K.OPS)


class Deck:
    """values dealt out in shuffled order; refilled when empty, so each occurs once per len draws"""

    def __init__(self, values, rng):
        self.values, self.rng, self.left = list(values), rng, []

    def draw(self, ok=lambda v: True):
        for _ in range(2):
            for i, v in enumerate(self.left):
                if ok(v):
                    return self.left.pop(i)
            self.left += [self.values[i] for i in self.rng.permutation(len(self.values))]
        raise AssertionError("no value of the deck is admissible")


# ---- block maps ------------------------------------------------------------------------
def grids(dims, size):
    """every process grid with at most dims[d] blocks in dimension d and product <= size"""
    out = []
    for g in itertools.product(*[range(1, min(d, size) + 1) for d in dims]):
        if int(np.prod(g)) <= size:
            out.append(list(g))
    return out


def blocks(amap, dims, size):
    """[(lo, hi) or None] per rank for an irregular map, C subscripts inclusive: the rank is the
    row-major index of the block in the grid (the last C dimension fastest)"""
    grid, starts = amap["block"], amap["starts"]
    out = []
    for r in range(size):
        if r >= int(np.prod(grid)):
            out.append(None)
            continue
        idx = np.unravel_index(r, grid)
        lo = [starts[d][i] for d, i in enumerate(idx)]
        hi = [starts[d][i + 1] - 1 if i + 1 < grid[d] else dims[d] - 1 for d, i in enumerate(idx)]
        out.append((lo, hi))
    return out


def cut(box, lo, hi):
    """the part of the block `box` inside [lo, hi], or None"""
    if box is None:
        return None
    l = [max(a, b) for a, b in zip(box[0], lo)]
    h = [min(a, b) for a, b in zip(box[1], hi)]
    return (l, h) if all(a <= b for a, b in zip(l, h)) else None


def inside(box, lo, hi):
    return box is not None and all(b0 <= a and c <= b1 for a, c, b0, b1 in zip(lo, hi, box[0], box[1]))


class Gen:
    def __init__(self, seed, size):
        self.size = size
        self.lg = np.random.default_rng([seed, 1])          # the logical layer: the same on every rank count
        self.mg = np.random.default_rng([seed, 2, size])    # the maps
        self.T = scan_tile()
        lg, mg = self.lg, self.mg
        self.types = {f: Deck(FAMILY_TYPES[f], lg) for f in FAMILIES}
        self.mask_types = Deck(TYPES, lg)
        self.dot_types = Deck(TYPES, lg)
        self.two_cut = {nd: Deck([True, False, False], mg) for nd in (2, 3, 4)}   # two decomposed dimensions at once
        self.rel3 = {f: Deck(RELATIONS[:5] + (["self_shifted"] if f == "math" else []), lg) for f in ("math", "elem")}
        self.rel2 = Deck(["same", "shifted", "othermap", "c_is_a", "self_shifted"], lg)
        self.relw = Deck(["same", "othermap", "c_is_a", "c_is_b"], lg)
        self.pclass = {f: Deck(PCLASSES, lg) for f in ("math", "elem")}
        self.pclass["scan"] = Deck([p for p in PCLASSES if p != "rowcol"], lg)
        self.ndim = Deck([1, 2, 2, 3, 4], lg)
        self.trans = Deck(TRANS, lg)
        self.patterns = Deck(MASK_PATTERNS, lg)
        self.scan_len = Deck(["small", "small", "tile-1", "tile", "tile+1", "long"], lg)
        self.excl = Deck([0, 1], lg)
        self.selop = Deck(["min", "max"], lg)
        self.kinds = Deck(KINDS, mg)
        self.strategy = Deck(["independent", "aligned", "irregular"], mg)
        self.carry = Deck([True, False], lg)
        self.pack_how = Deck(["independent", "aligned", "irregular"], lg)
        self.one_extent = Deck([False, False, True], lg)

    # -- logical layer ---------------------------------------------------------------------
    def dims(self, nd, need=None):
        """extents 1-300 / 1-70 / 1-12 / 1-6 (4-D: at most MAX_4D elements); an extent of 1 every
        third draw; `need(dims)` is a condition the call puts on them"""
        top = {1: 300, 2: 70, 3: 12, 4: 6}[nd]
        one = self.one_extent.draw()
        for attempt in range(1000):
            d = [int(x) for x in self.lg.integers(1, top + 1, nd)]
            if one:
                d[int(self.lg.integers(0, nd))] = 1
            if int(np.prod(d)) <= MAX_4D and (need is None or need(d)):
                return d
            if attempt > 50:   # the condition does not go with an extent of 1
                one = False
        raise AssertionError("no admissible dims")

    def patch(self, dims, pclass):
        """(lo, hi) of the class, or None where the dims do not admit it"""
        lg, nd = self.lg, len(dims)
        if pclass == "whole":
            return [0] * nd, [d - 1 for d in dims]
        if pclass == "one":
            p = [int(lg.integers(0, d)) for d in dims]
            return p, list(p)
        if pclass == "rowcol":   # all of one dimension, one index in the others
            if nd < 2:
                return None
            k = int(lg.integers(0, nd))
            p = [int(lg.integers(0, d)) for d in dims]
            return [0 if d == k else p[d] for d in range(nd)], [dims[d] - 1 if d == k else p[d] for d in range(nd)]
        lo = [int(lg.integers(0, d)) for d in dims]
        hi = [int(lg.integers(l, d)) for l, d in zip(lo, dims)]
        if pclass == "last":
            return lo, [d - 1 for d in dims]
        # a box the cuts are drawn around: two elements or more in one dimension (cross1), and
        # room behind it in one dimension (norank)
        if pclass == "cross1" and not any(h > l for l, h in zip(lo, hi)):
            return None
        if pclass == "norank" and not any(h < d - 1 for h, d in zip(hi, dims)):
            return None
        if pclass == "inside" and all(l == 0 and h == d - 1 for l, h, d in zip(lo, hi, dims)):
            return None
        return lo, hi

    def shifted(self, dims, lo, hi, disjoint):
        """a patch of the same extents elsewhere (disjoint: sharing no element), or None"""
        lg = self.lg
        ext = [h - l + 1 for l, h in zip(lo, hi)]
        for _ in range(50):
            l2 = [int(lg.integers(0, d - e + 1)) for d, e in zip(dims, ext)]
            if l2 == lo:
                continue
            h2 = [l + e - 1 for l, e in zip(l2, ext)]
            meet = all(a <= d and c <= b for a, b, c, d in zip(lo, hi, l2, h2))
            if not (disjoint and meet):
                return l2, h2
        return None

    # -- maps ---------------------------------------------------------------------------------
    def starts_1d(self, n, nb, allowed, forced=()):
        """nb strictly increasing block starts from 0 over n elements: the forced ones, the rest
        drawn from `allowed`; fewer where there are not enough"""
        pool = sorted(set(allowed) - set(forced) - {0})
        k = max(0, min(nb - 1 - len(forced), len(pool)))
        extra = [pool[i] for i in self.mg.choice(len(pool), k, replace=False)] if k else []
        return sorted({0, *forced, *extra})

    def irreg(self, dims, pclass=None, lo=None, hi=None, tiles=False, most=False):
        """an irregular map; for a BLOCKY class its cuts make the class true of [lo, hi]"""
        mg, size, nd = self.mg, self.size, len(dims)
        forced = [[] for _ in dims]
        allowed = [list(range(1, d)) for d in dims]
        want2 = None
        if pclass in BLOCKY and size > 1:
            if pclass != "norank":   # no cut through the patch but the forced one
                for d in range(nd):
                    allowed[d] = [s for s in range(1, dims[d]) if s <= lo[d] or s > hi[d]]
            if pclass == "cross1":
                want2 = int(mg.choice([d for d in range(nd) if hi[d] > lo[d]]))
                forced[want2] = [hi[want2]]
            elif pclass == "norank":
                want2 = int(mg.choice([d for d in range(nd) if hi[d] < dims[d] - 1]))
                forced[want2] = [int(mg.integers(hi[want2] + 1, dims[want2]))]
        if tiles and nd == 1:   # rank boundaries on tile boundaries as well as inside tiles
            T = self.T
            near = [s for k in range(1, 4) for s in (k * T - 1, k * T, k * T + 1) if 0 < s < dims[0]]
            if near and mg.integers(0, 2):
                allowed[0] = [s for s in allowed[0] if s in near] or allowed[0]
        gs = [g for g in grids(dims, size) if want2 is None or g[want2] >= 2]
        full = [g for g in gs if int(np.prod(g)) == max(int(np.prod(h)) for h in gs)]
        pick = full if most or mg.integers(0, 3) else gs
        two = [g for g in gs if sum(b > 1 for b in g) == 2]
        if nd > 1 and two and not most and self.two_cut[nd].draw():
            pick = two
        grid = list(pick[int(mg.integers(0, len(pick)))])
        starts = [self.starts_1d(dims[d], grid[d], allowed[d], forced[d]) for d in range(nd)]
        return {"kind": "irreg", "block": [len(s) for s in starts], "starts": starts}

    def chunk(self, dims):
        """1 up to the extent, and 0 or -1 in some dimensions"""
        mg = self.mg
        out = []
        for d in dims:
            r = int(mg.integers(0, 6))
            out.append(0 if r == 0 else -1 if r == 1 else int(mg.integers(1, d + 1)))
        return {"kind": "chunk", "chunk": out}

    def amap(self, dims, pclass=None, lo=None, hi=None, kind=None, tiles=False):
        if pclass in BLOCKY and self.size > 1:
            kind = "irreg"
        kind = kind or self.kinds.draw()
        if kind == "regular":
            return {"kind": "regular"}
        if kind == "chunk":
            return self.chunk(dims)
        return self.irreg(dims, pclass, lo, hi, tiles)

    def other(self, dims, first, tiles=False):
        """a map that is not `first`"""
        for _ in range(20):
            m = self.amap(dims, tiles=tiles)
            if m != first:
                return m
        return {"kind": "regular"} if first["kind"] != "regular" else self.chunk(dims)

    # -- the calls --------------------------------------------------------------------------------
    def case(self, fam, call, rel=None):
        c = {"fam": fam, "call": call, "dseed": int(self.lg.integers(0, 2 ** 31)), "rel": rel, "pclass": None}
        getattr(self, "_" + fam)(c)
        return c

    def arr(self, t, dims, data, amap):
        return {"t": t, "dims": list(dims), "data": data, "map": amap}

    def _one_array(self, c, fam, t, data):
        """a call on one array: the whole-array form, or a patch of a drawn class"""
        patchy = c["call"].endswith("_patch")
        for _ in range(1000):
            dims = self.dims(self.ndim.draw())
            if not patchy:
                c["pclass"], p = "whole", None
                break
            c["pclass"] = self.pclass[fam].draw(lambda v: v != "rowcol" or len(dims) > 1)
            p = self.patch(dims, c["pclass"])
            if p:
                break
            self.pclass[fam].left.insert(0, c["pclass"])   # not this time: the class stays next in the deck
        lo, hi = p if p else (None, None)
        c["arrays"] = [self.arr(t, dims, data, self.amap(dims, c["pclass"], lo, hi))]
        c["args"] = {"a": 0}
        c["patch"] = {"a": [lo, hi]} if p else {}

    def _three(self, c, fam, t, data):
        """NGA_Add_patch's structure: a, b -> c (copy and dot: a, b), by operand relation"""
        patchy = c["call"].endswith("_patch")
        two = c["call"] in ("GA_Copy", "NGA_Copy_patch", "GA_dot", "NGA_dot_patch")
        copy = "Copy" in c["call"]
        if not patchy:
            rel = self.relw.draw(lambda v: not (two and v == "c_is_b") and not (copy and v == "c_is_a"))
        elif two:
            rel = self.rel2.draw(lambda v: not (copy and v == "c_is_a"))
        else:
            rel = self.rel3[fam].draw()
        c["rel"] = rel
        moved = rel in ("shifted", "self_shifted")
        for _ in range(1000):
            dims = self.dims(self.ndim.draw(), (lambda d: max(d) > 1) if moved else None)
            if not patchy:
                c["pclass"], p, q = "whole", None, None
                break
            c["pclass"] = self.pclass[fam].draw(lambda v: (v != "rowcol" or len(dims) > 1) and not (moved and v == "whole"))
            p = self.patch(dims, c["pclass"])
            q = self.shifted(dims, p[0], p[1], rel == "self_shifted") if p and moved else None
            if p and (q or not moved):
                break
            self.pclass[fam].left.insert(0, c["pclass"])
        lo, hi = p if p else (None, None)
        # a copy between equal maps and equal patches is copy_patch's `here`: explicit maps, so that
        # the CPU test can tell
        m = self.amap(dims, c["pclass"], lo, hi, kind="irreg" if copy and rel == "same" else None)
        # the patch class is that of the output's patch (g_c; g_b of copy; dot's temporary
        # duplicates g_a, whose patch is the moved one); the input a moves or changes its map
        elsewhere = self.other(dims, m) if rel == "othermap" else m
        if two:
            share = rel in ("c_is_a", "self_shifted")
            c["arrays"] = [self.arr(t, dims, data, elsewhere)] + ([] if share else [self.arr(t, dims, data, m)])
            c["args"] = {"a": 0, "b": 0 if share else 1}
        else:
            share = rel in ("c_is_a", "c_is_b", "self_shifted")
            c["arrays"] = [self.arr(t, dims, data, m), self.arr(t, dims, data, elsewhere)] \
                + ([] if share else [self.arr(t, dims, data, m)])
            c["args"] = {"a": 0, "b": 1, "c": 1 if rel == "c_is_b" else 0 if share else 2}
            if rel == "othermap" and self.mg.integers(0, 2):   # a on the other map, b on c's
                c["arrays"][0], c["arrays"][1] = c["arrays"][1], c["arrays"][0]
        c["patch"] = {}
        if patchy:
            c["patch"] = {r: [lo, hi] for r in c["args"]}
            if moved:
                c["patch"]["a"] = [q[0], q[1]]

    def _math(self, c):
        call = c["call"]
        t = self.dot_types.draw() if "dot" in call else self.types["math"].draw()
        c["t"] = t
        if "Add" in call:
            self._three(c, "math", t, "gen")
        elif "Copy" in call:
            self._three(c, "math", t, "gen")
        elif "dot" in call:
            self._three(c, "math", t, "small5")
        else:
            self._one_array(c, "math", t, "gen")

    def _elem(self, c):
        call = c["call"]
        t = self.types["elem"].draw()
        c["t"] = t
        base = call[:-6] if call.endswith("_patch") else call
        if base in ELEM1:
            self._one_array(c, "elem", t, "nonzero" if base == "GA_Recip" else "gen")
        elif base in ELEM2:
            self._three(c, "elem", t, "nonzero" if base == "GA_Elem_divide" else "gen")
        else:
            dims = self.dims(self.ndim.draw())
            c["arrays"], c["args"], c["patch"] = [self.arr(t, dims, "gen", self.amap(dims))], {"a": 0}, {}
            c["op"] = self.selop.draw()

    def _gemm(self, c):
        lg = self.lg
        t = {"GA_Dgemm": C_DBL, "GA_Sgemm": C_FLOAT}.get(c["call"]) or self.types["gemm"].draw()
        c["t"] = t
        ta, tb = self.trans.draw()
        shared = {"c_is_a": "a", "c_is_b": "b"}.get(c["rel"])   # g_c is an input's array
        # two patches side by side in one array of at most 70 columns: 30 + 5 of padding each
        m, n, k = (int(x) for x in lg.integers(1, (30 if shared else GEMM_MAX) + 1, 3))
        c.update(ta=ta, tb=tb, m=m, n=n, k=k)
        shapes = {"a": [k, m] if ta == "T" else [m, k], "b": [n, k] if tb == "T" else [k, n], "c": [m, n]}
        c["arrays"], c["args"], c["patch"] = [], {}, {}
        dims = {}
        for r in "abc":
            pad = [int(x) for x in lg.integers(0, 6, 2)]
            off = [int(lg.integers(0, p + 1)) for p in pad] if c["call"] == "NGA_Matmul_patch" else [0, 0]
            dims[r] = [s + p for s, p in zip(shapes[r], pad)]
            c["patch"][r] = [off, [o + s - 1 for o, s in zip(off, shapes[r])]]
        if shared:
            # the C patch to the right of the input's array, in the same rows or not: it never meets
            # the input patch, which the layer would reject
            lo, hi = c["patch"]["c"]
            c["patch"]["c"] = [[lo[0], lo[1] + dims[shared][1]], [hi[0], hi[1] + dims[shared][1]]]
            dims[shared] = [max(dims[shared][0], dims["c"][0]), dims[shared][1] + dims["c"][1]]
        for r in "abc":
            if r == "c" and shared:
                c["args"]["c"] = c["args"][shared]
                continue
            c["args"][r] = len(c["arrays"])
            c["arrays"].append(self.arr(t, dims[r], "gemm", self.amap(dims[r])))

    def _trans(self, c):
        lg = self.lg
        if c["call"] == "GA_Symmetrize":
            t = c["t"] = int(lg.choice([C_FLOAT, C_DBL]))
            n = int(lg.integers(1, 71))
            c["arrays"], c["args"], c["patch"] = [self.arr(t, [n, n], "gen", self.amap([n, n]))], {"a": 0}, {}
            return
        t = c["t"] = self.types["trans"].draw()
        dims = self.dims(2)
        how = self.strategy.draw()
        kind = "irreg" if how == "irregular" else None   # both maps explicit and unrelated
        ma = self.amap(dims, kind=kind)
        mb = self.amap(dims[::-1], kind=kind)
        if how == "aligned":
            # the mirror of every block of B in the same rank's block of A: A cut along one dimension
            # only (the rank numbering of a p x 1 grid survives the transposition), B its mirror
            ma = self.irreg(dims)
            k = int(np.argmax(ma["block"]))
            ma = {"kind": "irreg", "block": [b if d == k else 1 for d, b in enumerate(ma["block"])],
                  "starts": [s if d == k else [0] for d, s in enumerate(ma["starts"])]}
            mb = {"kind": "irreg", "block": ma["block"][::-1], "starts": ma["starts"][::-1]}
        c["arrays"] = [self.arr(t, dims, "gen", ma), self.arr(t, dims[::-1], "gen", mb)]
        c["args"], c["patch"] = {"a": 0, "b": 1}, {}

    def _matrix(self, c):
        call = c["call"]
        t = c["t"] = self.types["matrix"].draw()
        if "Norm" in call:
            dims = self.dims(int(self.lg.integers(1, 3)))
            data = "norm_exact" if call == "GA_Norm1" else "gen"
            c["arrays"], c["args"], c["patch"] = [self.arr(t, dims, data, self.amap(dims))], {"a": 0}, {}
            return
        dims = self.dims(2)
        n = {"GA_Scale_rows": dims[0], "GA_Scale_cols": dims[1]}.get(call, min(dims))
        how = self.strategy.draw()
        kind = "irreg" if how == "irregular" else None
        ma, mv = self.amap(dims, kind=kind), self.amap([n], kind=kind)
        if how == "aligned":
            # g_a cut along one dimension only and g_v by the same starts: every rank's range of g_v
            # lies in its own block of g_v
            k = 1 if call == "GA_Scale_cols" else 0
            mv = self.irreg([n])
            ma = {"kind": "irreg", "block": [mv["block"][0] if d == k else 1 for d in range(2)],
                  "starts": [mv["starts"][0] if d == k else [0] for d in range(2)]}
        c["arrays"] = [self.arr(t, dims, "gen", ma)]
        c["args"] = {"a": 0}
        if call not in ("GA_Shift_diagonal", "GA_Zero_diagonal"):
            c["arrays"].append(self.arr(t, [n], "gen", mv))   # g_v on its own map
            c["args"]["v"] = 1
        c["patch"] = {}

    def _scan(self, c):
        lg, T, call = self.lg, self.T, c["call"]
        t = c["t"] = self.types["scan"].draw()
        how = self.scan_len.draw()
        n = {"small": int(lg.integers(1, 301)), "tile-1": T - 1, "tile": T, "tile+1": T + 1,
             "long": int(lg.integers(2 * T, 3 * T + 18))}[how]
        # every other scan: the first element of the whole range set and nothing else, under an
        # irregular map of as many blocks as there are ranks -- the carry of the later ranks passes
        # over ranks that have a part and no set element
        carry = call in ("GA_Scan_copy", "GA_Scan_add") and self.carry.draw()
        # pack and unpack, one time in three each: the packed side under the mask's own irregular map
        # with the first element set (the first rank's place is the start of its own block: in
        # place); both sides under irregular maps that have nothing to do with each other (scratch)
        pack_how = self.pack_how.draw() if call in ("GA_Pack", "GA_Unpack") else None
        if carry or pack_how == "aligned":
            n = max(n, 8)
        fixed = carry or pack_how == "aligned"
        for _ in range(1000):
            c["pclass"] = self.pclass["scan"].draw((lambda v: v == "whole") if fixed else (lambda v: True))
            p = self.patch([n], c["pclass"])
            if p:
                break
            self.pclass["scan"].left.insert(0, c["pclass"])
            n = max(n, 3)
        lo, hi = p[0][0], p[1][0]
        c["lo"], c["hi"] = lo, hi
        if carry or pack_how in ("aligned", "irregular"):
            m = self.irreg([n], c["pclass"], [lo], [hi], tiles=True, most=True)
        else:
            m = self.amap([n], c["pclass"], [lo], [hi], tiles=True)
        c["patch"] = {}
        if call == "GA_Patch_enum":
            c["arrays"], c["args"] = [self.arr(t, [n], "gen", m)], {"a": 0}
            return
        mt = self.mask_types.draw()
        c["pattern"] = "first" if carry else str(self.lg.choice(["all", "first"])) if pack_how == "aligned" \
            else self.patterns.draw()
        c["mseed"] = int(lg.integers(0, 2 ** 31))
        msk = self.arr(mt, [n], "mask", m)
        if call in ("GA_Scan_copy", "GA_Scan_add"):
            c["excl"] = self.excl.draw() if call == "GA_Scan_add" else 0
            data = "scan_exact" if call == "GA_Scan_add" else "gen"
            c["arrays"] = [self.arr(t, [n], data, m), self.arr(t, [n], "gen", m), msk]
            c["args"] = {"src": 0, "dst": 1, "msk": 2}
            return
        # the packed side on its own map, long enough for the set elements of [lo, hi]
        cnt = int(mask_set(c, n)[lo:hi + 1].sum())
        np_ = int(lg.integers(max(cnt, 1), n + 1))
        if pack_how == "aligned":
            np_, mt_ = n, m
        elif pack_how == "irregular":
            mt_ = self.irreg([np_], tiles=True, most=True)
        else:
            mt_ = self.other([np_], m, tiles=True) if np_ == n else self.amap([np_], tiles=True)
        thin = self.arr(t, [np_], "gen", mt_)
        full = self.arr(t, [n], "gen", m)
        c["arrays"] = [full, thin, msk] if call == "GA_Pack" else [thin, full, msk]
        c["args"] = {"src": 0, "dst": 1, "msk": 2}


def mask_set(c, n):
    """which mask elements are set: the case's pattern over the n elements"""
    rng = np.random.default_rng(c["mseed"])
    idx = np.arange(n)
    lo, hi = c["lo"], c["hi"]
    p = c["pattern"]
    if p == "none":
        st = np.zeros(n, dtype=bool)
    elif p == "all":
        st = np.ones(n, dtype=bool)
    elif p == "first":
        st = idx == lo
    elif p == "last":
        st = idx == hi
    elif p == "single":
        st = idx == int(rng.integers(lo, hi + 1))
    else:
        st = rng.integers(0, 2 if p == "half" else 64, n) == 0
    if p in ("first", "last", "single", "sparse"):   # set elements outside [lo, hi] are ignored
        for i in (lo - 1, hi + 1):
            if 0 <= i < n:
                st = st | (idx == i)
    return st


def cases(seed, size):
    g = Gen(seed, size)
    out = []
    for i, (fam, call, rel) in enumerate(PLAN):
        c = g.case(fam, call, rel)
        c["index"] = i
        out.append(c)
    return out


# ---- data ----------------------------------------------------------------------------------------
GEMM_ALPHA, GEMM_BETA = 2.0, -3.0
ENUM_START, ENUM_INC = K.VALUE, K.ALPHA


def nonzero(op, x):
    """no zero divisor: no zero element, complex no zero part"""
    if op in K.REAL:
        re, im = x.real.copy(), x.imag.copy()
        re[re == 0] = 1
        im[im == 0] = 1
        return E.nonzero(op, K._cplx(op, re, im))
    x = x.copy()
    x[x == 0] = 1
    return E.nonzero(op, x)


def inputs(c):
    """the arrays' first contents, C order, from the case's data seed"""
    rng = np.random.default_rng(c["dseed"])
    out = []
    for a in c["arrays"]:
        op, n = OP_OF[a["t"]], int(np.prod(a["dims"]))
        kind = a["data"]
        if kind == "gen":
            x = K.gen(op, n, rng)
        elif kind == "small5":
            x = K.gen(op, n, rng, None if op in K.UNS else 5)
        elif kind == "nonzero":
            x = nonzero(op, K.gen(op, n, rng))
        elif kind == "norm_exact":
            x = M.gen_exact(op, n, rng)
            assert M.exactly_summable(op, x)
        elif kind == "scan_exact":
            x = S.gen_exact(op, n, rng)
            assert S.exact_in_range(op, x)
        elif kind == "gemm":
            x = rng.integers(-8, 9, n).astype(K.DT[op])
        else:
            x = S.make_mask(op, mask_set(c, n), rng)
        out.append(np.ascontiguousarray(x.reshape(a["dims"])))
    return out


def scalars(c):
    """the call's scalar arguments as one-element arrays of the type"""
    op = OP_OF[c["t"]]
    return {"value": K.scalar(op, K.VALUE[op]), "alpha": K.scalar(op, K.ALPHA[op]), "beta": K.scalar(op, K.BETA[op]),
            "const": K.scalar(op, E.CONST[op]), "shift": K.scalar(op, M.SHIFT_C[op]),
            "start": K.scalar(op, ENUM_START[op]), "inc": K.scalar(op, ENUM_INC[op])}


# ---- the model ---------------------------------------------------------------------------------------
def model(c, arrs):
    """(the arrays after the call, {name: bytes of a scalar result}); arrs is not changed"""
    arrs = [a.copy() for a in arrs]
    res = {}
    call, op, g, P = c["call"], OP_OF[c["t"]], c["args"], c["patch"]
    base = call[:-6] if call.endswith("_patch") else call

    def view(r):
        a = arrs[g[r]]
        return a[sl(*P[r])] if r in P else a[...]

    def store(r, vals):
        v = view(r)
        v[...] = np.asarray(vals).reshape(v.shape)

    if base in ("GA_Fill", "NGA_Fill"):
        store("a", K.ref_fill(op, view("a").size, K.VALUE[op]))
    elif base in ("GA_Zero", "NGA_Zero"):
        store("a", np.zeros(view("a").size, dtype=K.DT[op]))
    elif base in ("GA_Scale", "NGA_Scale"):
        store("a", K.ref_scale(op, flat(view("a")), K.ALPHA[op]))
    elif base in ("GA_Add", "NGA_Add"):
        store("c", K.ref_add(op, K.ALPHA[op], flat(view("a")), K.BETA[op], flat(view("b"))))
    elif base in ("GA_Copy", "NGA_Copy"):
        store("b", flat(view("a")).copy())
    elif base in ("GA_dot", "NGA_dot"):
        a, b = flat(view("a")), flat(view("b"))
        if op not in K.UNS:
            parts = 2 if op in K.REAL else 1
            assert 25.0 * 2 * parts * a.size < 2.0 ** 24   # every partial sum of the products is exact
        res["dot"] = K.ref_dot_exact(op, a, b).tobytes()
    elif base in ELEM1:
        vals, bad = E.ref_elem1(op, ELEM1[base], flat(view("a")), E.CONST[op])
        assert not bad.any()
        store("a", vals)
    elif base in ELEM2:
        vals, bad = E.ref_elem2(op, ELEM2[base], flat(view("a")), flat(view("b")))
        assert not bad.any()
        store("c", vals)
    elif call == "NGA_Select_elem":
        x = flat(arrs[g["a"]])
        i, elem, _ = E.ref_select(op, c["op"] == "max", x)
        res["val"] = elem.tobytes()
        res["index"] = np.array(np.unravel_index(i, arrs[g["a"]].shape), dtype=np.int32).tobytes()
    elif c["fam"] == "gemm":
        assert 2 * 64 * c["k"] + 3 * 8 < 2 ** 24
        a, b = view("a").astype(np.int64), view("b").astype(np.int64)
        prod = (a.T if c["ta"] == "T" else a) @ (b.T if c["tb"] == "T" else b)
        store("c", (2 * prod - 3 * view("c").astype(np.int64)).astype(K.DT[op]))
    elif call == "GA_Transpose":
        arrs[g["b"]] = np.ascontiguousarray(arrs[g["a"]].T)
    elif call == "GA_Symmetrize":
        a = arrs[g["a"]]
        arrs[g["a"]] = K.DT[op].type(0.5) * (a + a.T)
    elif call in DIAG:
        a = arrs[g["a"]]
        idx = np.arange(min(a.shape))
        if call == "GA_Shift_diagonal":
            a[idx, idx] = M.ref_diag_add(op, a[idx, idx], K.scalar(op, M.SHIFT_C[op]))
        elif call == "GA_Zero_diagonal":
            a[idx, idx] = 0
        elif call == "GA_Set_diagonal":
            a[idx, idx] = arrs[g["v"]]
        elif call == "GA_Add_diagonal":
            a[idx, idx] = M.ref_diag_add(op, a[idx, idx], arrs[g["v"]])
        else:
            arrs[g["v"]] = a[idx, idx].copy()
    elif call in ("GA_Scale_rows", "GA_Scale_cols"):
        arrs[g["a"]] = np.ascontiguousarray(M.ref_scale(op, arrs[g["a"]], arrs[g["v"]], call == "GA_Scale_rows"))
    elif call == "GA_Norm1":
        x = flat(arrs[g["a"]])
        assert M.exactly_summable(op, x)
        res["norm"] = np.float64(M.ref_norm1_exact(op, x)[0]).tobytes()
    elif call == "GA_Norm_infinity":
        res["norm"] = np.float64(M.ref_norm_inf(op, flat(arrs[g["a"]]))[0]).tobytes()
    elif call == "GA_Patch_enum":
        lo, hi = c["lo"], c["hi"]
        arrs[g["a"]][lo:hi + 1] = S.ref_enum(op, hi - lo + 1, 0, ENUM_START[op], ENUM_INC[op])
    else:
        lo, hi = c["lo"], c["hi"]
        st = mask_set(c, len(arrs[g["msk"]]))
        assert np.array_equal(S.ref_set(arrs[g["msk"]]), st)
        src, dst = arrs[g["src"]], arrs[g["dst"]]
        inside_ = np.zeros(len(st), dtype=bool)
        inside_[lo:hi + 1] = st[lo:hi + 1]
        if call in ("GA_Scan_copy", "GA_Scan_add"):
            fn = S.COPY if call == "GA_Scan_copy" else S.EXCL if c["excl"] else S.ADD
            if fn != S.COPY:
                assert S.exact_in_range(op, src)
            want, written = S.ref_scan(op, fn, src[lo:hi + 1], st[lo:hi + 1])
            part = dst[lo:hi + 1]
            part[written] = want[written]
        elif call == "GA_Pack":
            cnt = int(inside_.sum())
            assert cnt <= len(dst)
            dst[:cnt] = S.ref_pack(src, inside_)
            res["icount"] = np.int32(cnt).tobytes()
        else:
            cnt = int(inside_.sum())
            assert cnt <= len(src)
            arrs[g["dst"]] = S.ref_unpack(src, inside_, dst)
            res["icount"] = np.int32(cnt).tobytes()
    return arrs, res


def written(c):
    """indices of the arrays the call writes"""
    call, g = c["call"], c["args"]
    if c["fam"] == "scan" and call != "GA_Patch_enum":
        return [g["dst"]]
    if call == "GA_Get_diag":
        return [g["v"]]
    if call in ("NGA_Select_elem", "GA_Norm1", "GA_Norm_infinity") or "dot" in call:
        return []
    if "Copy" in call or call == "GA_Transpose":
        return [g["b"]]
    return [g["c"] if "c" in g else g["a"]]


# ---- the layer's host-side decisions, from map and patch (irregular maps only) -----------------------
def explicit(c):
    return all(a["map"]["kind"] == "irreg" for a in c["arrays"])


def case_blocks(c, size):
    return [blocks(a["map"], a["dims"], size) for a in c["arrays"]]


def copies(c, size):
    """{"here", "put"} over the ranks of every copy_patch the call runs (its own, or into the
    GA_Duplicate temporary of add_patch / elem2_patch / dot_patch)"""
    call, g, P = c["call"], c["args"], c["patch"]
    base = call[:-6] if call.endswith("_patch") else call
    if base not in ("GA_Add", "NGA_Add", "GA_Copy", "NGA_Copy", "GA_dot", "NGA_dot") and base not in ELEM2:
        return set()
    B = case_blocks(c, size)

    def box(r):
        a = c["arrays"][g[r]]
        return P[r] if r in P else [[0] * len(a["dims"]), [d - 1 for d in a["dims"]]]

    pairs = []   # (source role, destination role the temporary duplicates or the copy writes)
    if "Copy" in call:
        if not (g["a"] == g["b"] and box("a") == box("b")):
            pairs.append(("a", "b"))
    elif "dot" in call:
        if not (c["arrays"][g["a"]]["map"] == c["arrays"][g["b"]]["map"] and box("a") == box("b")):
            pairs.append(("b", "a"))
    else:
        for r in "ab":
            if not (c["arrays"][g[r]]["map"] == c["arrays"][g["c"]]["map"] and box(r) == box("c")):
                pairs.append((r, "c"))
    out = set()
    for s, d in pairs:
        same = c["arrays"][g[s]]["map"] == c["arrays"][g[d]]["map"]
        for q in range(size):
            if cut(B[g[s]][q], *box(s)):
                out.add("here" if same and box(s)[0] == box(d)[0] else "put")
    return out


def transposes(c, size):
    """{"own", "get_mirror"} over the ranks that own a block of B"""
    g = c["args"]
    A, B = (blocks(c["arrays"][g[r]]["map"], c["arrays"][g[r]]["dims"], size) for r in "ab")
    out = set()
    for q in range(size):
        if B[q]:
            lo, hi = B[q]
            out.add("own" if inside(A[q], lo[::-1], hi[::-1]) else "get_mirror")
    return out


def vec_parts(c, size):
    """{"in place", "scratch"} over the ranks: the Part of the matrix calls and of pack / unpack (room for n)"""
    call, g = c["call"], c["args"]
    out = set()
    if c["fam"] == "matrix" and "v" in g:
        A, V = (blocks(c["arrays"][g[r]]["map"], c["arrays"][g[r]]["dims"], size) for r in "av")
        for q in range(size):
            if not A[q]:
                continue
            (r0, c0), (r1, c1) = A[q]
            lo, hi = {"GA_Scale_rows": (r0, r1), "GA_Scale_cols": (c0, c1)}.get(call, (max(r0, c0), min(r1, c1)))
            if lo <= hi:
                out.add("in place" if inside(V[q], [lo], [hi]) else "scratch")
    elif call in ("GA_Pack", "GA_Unpack"):
        thin, full = (g["dst"], g["src"]) if call == "GA_Pack" else (g["src"], g["dst"])
        F = blocks(c["arrays"][full]["map"], c["arrays"][full]["dims"], size)
        Tn = blocks(c["arrays"][thin]["map"], c["arrays"][thin]["dims"], size)
        st = mask_set(c, c["arrays"][full]["dims"][0])
        place = 0
        for q in range(size):
            part = cut(F[q], [c["lo"]], [c["hi"]])
            if not part:
                continue
            n = part[1][0] - part[0][0] + 1
            cnt = int(st[part[0][0]:part[1][0] + 1].sum())
            if cnt:
                out.add("in place" if inside(Tn[q], [place], [place + n - 1]) else "scratch")
            place += cnt
    return out


def carry_skips(c, size):
    """True where a rank's carry passes over a rank that has a part of the range and no set element"""
    g = c["args"]
    n = c["arrays"][g["msk"]]["dims"][0]
    Bm = blocks(c["arrays"][g["msk"]]["map"], [n], size)
    st = mask_set(c, n)
    slots = []
    for q in range(size):
        part = cut(Bm[q], [c["lo"]], [c["hi"]])
        slots.append(None if not part else bool(st[part[0][0]:part[1][0] + 1].any()))
    for me in range(size):
        if slots[me] is None:
            continue
        frm = me - 1
        while frm >= 0 and not slots[frm]:
            frm -= 1
        if frm >= 0 and any(slots[r] is False for r in range(frm + 1, me)):
            return True
    return False


def patch_class_holds(c, size):
    """for a BLOCKY class under an irregular map on 2 ranks or more: is it true of the map?"""
    if c["fam"] == "scan":
        a, lo, hi = c["arrays"][c["args"].get("msk", 0)], [c["lo"]], [c["hi"]]
    else:
        r = "c" if "c" in c["patch"] else "b" if "b" in c["patch"] else "a"
        a, (lo, hi) = c["arrays"][c["args"][r]], c["patch"][r]
    B = blocks(a["map"], a["dims"], size)
    parts = [cut(b, lo, hi) for b in B]
    owners = [p for p in parts if p]
    if c["pclass"] == "inside":
        return len(owners) == 1
    if c["pclass"] == "norank":
        return any(b is not None and p is None for b, p in zip(B, parts))
    if len(owners) != 2:   # cross1: two owners, the second with the patch's last layer in one dimension
        return False
    differ = [d for d in range(len(lo)) if (owners[1][0][d], owners[1][1][d]) != (lo[d], hi[d])]
    return len(differ) == 1 and owners[1][0][differ[0]] == owners[1][1][differ[0]] == hi[differ[0]]
