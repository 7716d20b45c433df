"""No GPU: the case generator and the model of the GA-layer fuzz (tests/ga_fuzz_cases.py), for the
suite's seed -- 0, shifted by GAAMD_FUZZ_SEED as in the other fuzz tests -- and 1 to 4 ranks.

What the launch on the GPU relies on is asserted here: the list is a pure function of (seed,
size); every call, type, map kind, operand relation and patch class occurs; the host-side
decisions of ga.cpp that can be told from an explicit (irregular) map and the patch are each
taken both ways; and the model runs over every case with every exactness assertion holding, so
on the GPU no case is skipped and every comparison is bit for bit.

Where a condition cannot hold on one rank it is asserted from two ranks on: one rank owns
everything, so there is no cut to cross, no rank left with nothing, no mirror or vector range
outside its block.  Operand relations and patch classes are asserted for the families whose calls
take patches of several arrays (math, elem) and, for the range classes, the 1-D scan family."""
import ctypes
import json
import os

import numpy as np
import pytest

import ga_amd
import ga_fuzz_cases as F

SEED = int(os.environ.get("GAAMD_FUZZ_SEED", "0"))
SIZES = [1, 2, 3, 4]


@pytest.fixture(scope="module")
def lists():
    return {n: F.cases(SEED, n) for n in SIZES}


@pytest.mark.parametrize("n", SIZES)
def test_the_list_is_a_pure_function_of_seed_and_size(lists, n):
    again = F.cases(SEED, n)
    assert json.dumps(again) == json.dumps(lists[n])   # plain ints, strings and lists all the way down
    assert len(again) == len(F.PLAN) and [c["index"] for c in again] == list(range(len(F.PLAN)))
    assert json.dumps(F.cases(SEED + 1, n)) != json.dumps(lists[n])


def test_the_logical_layer_is_the_same_on_every_rank_count(lists):
    """case i is the same computation on 1, 2, 3 and 4 ranks: only the block maps differ, which
    is what lets the launcher ask for the same scalar results on every rank count"""
    def logical(c):
        d = {k: v for k, v in c.items() if k != "arrays"}
        d["arrays"] = [{k: v for k, v in a.items() if k != "map"} for a in c["arrays"]]
        return json.dumps(d)
    for n in SIZES[1:]:
        assert [logical(c) for c in lists[n]] == [logical(c) for c in lists[1]]


@pytest.mark.parametrize("n", SIZES)
def test_calls_types_maps_relations_and_patch_classes_all_occur(lists, n):
    cs = lists[n]
    assert {c["call"] for c in cs} == set(F.CALLS)
    for fam in F.FAMILIES:
        assert {c["t"] for c in cs if c["fam"] == fam} == set(F.FAMILY_TYPES[fam]), fam
    assert {c["t"] for c in cs if "dot" in c["call"]} == set(F.TYPES)   # the six GA_?dot and NGA_?dot_patch
    assert {c["arrays"][c["args"]["msk"]]["t"] for c in cs if "msk" in c["args"]} == set(F.TYPES)
    assert {a["map"]["kind"] for c in cs for a in c["arrays"]} == set(F.KINDS)
    chunks = [v for c in cs for a in c["arrays"] if a["map"]["kind"] == "chunk" for v in a["map"]["chunk"]]
    assert 0 in chunks and -1 in chunks and 1 in chunks and max(chunks) > 1
    assert {c["rel"] for c in cs if c["fam"] == "math"} - {None} == set(F.RELATIONS)
    assert {c["rel"] for c in cs if c["fam"] == "elem"} - {None} == set(F.RELATIONS[:5])
    for fam in ("math", "elem"):
        assert {c["pclass"] for c in cs if c["fam"] == fam} - {None} == set(F.PCLASSES), fam
    assert {c["pclass"] for c in cs if c["fam"] == "scan"} == set(F.PCLASSES) - {"rowcol"}
    assert {(c["ta"], c["tb"]) for c in cs if c["fam"] == "gemm"} == {tuple(t) for t in F.TRANS}
    assert {c["rel"] for c in cs if c["call"] == "NGA_Matmul_patch"} == {None, "c_is_a", "c_is_b"}
    assert {c["excl"] for c in cs if c["call"] == "GA_Scan_add"} == {0, 1}
    assert {c["op"] for c in cs if c["call"] == "NGA_Select_elem"} == {"min", "max"}
    assert {len(a["dims"]) for c in cs for a in c["arrays"]} == {1, 2, 3, 4}
    for fam in ("math", "elem"):   # the patch forms on arrays of rank 3 and 4, not on 2-D ones only
        assert {3, 4} <= {len(c["arrays"][0]["dims"]) for c in cs if c["fam"] == fam and c["patch"]}, fam
    assert any(1 in a["dims"] for c in cs for a in c["arrays"])           # NGA_Create's fdims[d] == 1
    T = F.scan_tile()
    lens = {c["arrays"][-1]["dims"][0] for c in cs if c["fam"] == "scan"}
    assert {T - 1, T, T + 1} <= lens and max(lens) <= 3 * T + 17 and max(lens) >= 2 * T


@pytest.mark.parametrize("n", SIZES)
def test_shapes_and_patches_are_legal(lists, n):
    """what the layer rejects by design never comes out of the generator"""
    for c in lists[n]:
        for a in c["arrays"]:
            d = a["dims"]
            assert 1 <= len(d) <= 4 and min(d) >= 1 and int(np.prod(d)) <= F.MAX_4D
            if c["fam"] != "scan":
                assert max(d) <= {1: 300, 2: 70, 3: 12, 4: 6}[len(d)]
            m = a["map"]
            if m["kind"] == "irreg":
                assert int(np.prod(m["block"])) <= n
                for s, nb, e in zip(m["starts"], m["block"], d):
                    assert len(s) == nb and s[0] == 0 and s[-1] < e and all(x < y for x, y in zip(s, s[1:]))
        for r, (lo, hi) in c["patch"].items():
            d = c["arrays"][c["args"][r]]["dims"]
            assert all(0 <= l <= h < e for l, h, e in zip(lo, hi, d)), c
        P, g = c["patch"], c["args"]
        roles = [r for r in "abc" if r in P]
        if c["fam"] in ("math", "elem"):
            ext = {tuple(h - l for l, h in zip(*P[r])) for r in roles}
            assert len(ext) <= 1, c                                        # no reshape
        for r in roles:                                                    # patches of one array: equal or disjoint
            for s in roles:
                if r < s and g[r] == g[s] and P[r] != P[s]:
                    assert not all(a <= d and c_ <= b for a, b, c_, d in zip(P[r][0], P[r][1], P[s][0], P[s][1])), c
        if c["fam"] == "gemm":   # g_c in an input's array: its patch does not meet the input's (checked above)
            assert max(c["m"], c["n"], c["k"]) <= F.GEMM_MAX and g["a"] != g["b"]
            assert len({g["a"], g["b"], g["c"]}) == (3 if c["rel"] is None else 2)
        if "src" in g:
            assert g["src"] != g["dst"]
        if c["call"] == "GA_Transpose":
            assert g["a"] != g["b"]


@pytest.mark.parametrize("n", SIZES)
def test_the_model_runs_over_every_case_and_stays_exact(lists, n):
    """no case is skipped and every exactness assertion of the restatements holds; what a call
    does not write is bit for bit what went in"""
    ran = 0
    for c in lists[n]:
        before = F.inputs(c)
        after, res = F.model(c, before)
        assert [a.tobytes() for a in before] == [a.tobytes() for a in F.inputs(c)]   # the model copies
        for i, (x, y) in enumerate(zip(before, after)):
            assert x.shape == y.shape and x.dtype == y.dtype
            if i not in F.written(c):
                assert x.tobytes() == y.tobytes(), c
        w = F.written(c)
        if c["patch"] and c["fam"] in ("math", "elem") and w:
            r = next(r for r in "cba" if r in c["patch"] and c["args"][r] == w[0])
            keep = np.ones(before[w[0]].shape, dtype=bool)
            keep[F.sl(*c["patch"][r])] = False
            assert before[w[0]][keep].tobytes() == after[w[0]][keep].tobytes(), c
        assert all(isinstance(v, bytes) for v in res.values())
        ran += 1
    assert ran == len(F.PLAN)


def test_the_process_grid_fits_the_ranks(lists):
    """gaamd_ga_proc_grid for every drawn regular shape, chunk or not: never more blocks than ranks"""
    L = ga_amd.lib()
    seen = 0
    for n in SIZES:
        for c in lists[n]:
            for a in c["arrays"]:
                if a["map"]["kind"] == "irreg":
                    continue
                nd = len(a["dims"])
                grid = (ctypes.c_int * nd)()
                chunk = ga_amd.int_array(a["map"]["chunk"]) if a["map"]["kind"] == "chunk" else None
                assert L.gaamd_ga_proc_grid(nd, ga_amd.int_array(a["dims"]), chunk, n, grid) == 0
                assert min(grid) >= 1 and int(np.prod(list(grid))) <= n, (a, list(grid))
                seen += 1
    assert seen > 100


def explicit(cs):
    return [c for c in cs if F.explicit(c)]


def test_four_ranks_decompose_two_dimensions_at_once(lists):
    grids = [tuple(a["map"]["block"]) for c in lists[4] if c["fam"] != "scan" for a in c["arrays"]
             if a["map"]["kind"] == "irreg"]
    assert (2, 2) in grids
    assert any(len(g) == 3 and sorted(g) == [1, 2, 2] for g in grids)
    assert any(len(g) == 4 and sum(b > 1 for b in g) == 2 for g in grids)


@pytest.mark.parametrize("n", SIZES[1:])
def test_host_side_decisions_are_taken_both_ways(lists, n):
    cs = explicit(lists[n])
    nothing = fewer = False
    for c in cs:
        for a, B in zip(c["arrays"], F.case_blocks(c, n)):
            fewer = fewer or None in B                       # fewer blocks than ranks
            nothing = nothing or None in B
    assert nothing and fewer
    assert any(any(h == l for l, h in zip(*b)) for c in cs for B in F.case_blocks(c, n) for b in B if b)   # one-element-wide blocks
    tr = set().union(*[F.transposes(c, n) for c in cs if c["call"] == "GA_Transpose"])
    assert tr == {"own", "get_mirror"}, tr
    vp = set().union(*[F.vec_parts(c, n) for c in cs if c["fam"] == "matrix"])
    assert vp == {"in place", "scratch"}, vp
    pk = set().union(*[F.vec_parts(c, n) for c in cs if c["call"] in ("GA_Pack", "GA_Unpack")])
    assert pk == {"in place", "scratch"}, pk
    cp = set().union(*[F.copies(c, n) for c in cs])
    assert cp == {"here", "put"}, cp


@pytest.mark.parametrize("n", SIZES)
def test_copy_patch_puts_on_every_rank_count(lists, n):
    """a shifted patch is a put even on one rank; the temporaries of the general path are taken"""
    cs = explicit(lists[n]) if n > 1 else lists[n]
    moved = [c for c in cs if c["rel"] in ("shifted", "self_shifted")]
    assert moved and all(c["patch"]["a"] != c["patch"].get("c", c["patch"]["b"]) for c in moved)


@pytest.mark.parametrize("n", [3, 4])
def test_a_scan_carry_passes_over_a_rank_without_a_set_element(lists, n):
    scans = [c for c in explicit(lists[n]) if c["call"] in ("GA_Scan_copy", "GA_Scan_add")]
    assert any(F.carry_skips(c, n) for c in scans)
    assert any(F.carry_skips(c, n) for c in scans if c["call"] == "GA_Scan_add")   # the tails between are added


@pytest.mark.parametrize("n", SIZES[1:])
def test_block_patch_classes_hold_of_the_drawn_map(lists, n):
    """inside one block, crossing exactly one cut by one element, leaving a rank with nothing:
    true of the irregular map that was drawn around the patch"""
    seen = set()
    for c in lists[n]:
        if c["pclass"] in F.BLOCKY:
            assert F.patch_class_holds(c, n), c
            seen.add((c["fam"], c["pclass"]))
    assert seen == {(f, p) for f in ("math", "elem", "scan") for p in F.BLOCKY}
