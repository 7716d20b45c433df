"""GPU, GA layer: a seeded differential fuzz of ga_amd/csrc/ga.cpp over block maps, rank counts
and patches, on 1, 2, 3 and 4 ranks sharing one GPU (tests/ga_fuzz_worker.py is one rank; the
cases and the numpy model of the whole global array are tests/ga_fuzz_cases.py, checked on the
CPU by tests/test_ga_fuzz_cases.py).  Seed 0, shifted by GAAMD_FUZZ_SEED.

Every computing call of include/ga.h, all six types, arrays of rank 1 to 4 under NGA_Create with
and without a chunk and under NGA_Create_irreg (2 x 2 and 2 x 1 x 2 grids on 4 ranks, grids of
fewer blocks than ranks, blocks of one element), every operand relation and patch class: each
rank compares every array involved with the model as raw bits, through NGA_Get and through its
own block, and the scalar results have to be the same bits on every rank and on every rank count.

Two launches per rank count, split by call family (PARTS below): each takes no longer than the GA
matrix launch on as many ranks (profiles/r14/ga_fuzz/times.txt).

Every rank process runs under its own time limit (a watcher thread each); once a launch ends in
anything but the outcome its test expects, the remaining tests of this file start nothing."""
import time

import pytest

import ga_fuzz_cases as F
import mp_launch

MP = mp_launch.Launcher("ga_fuzz_worker.py", "z", marker="FUZZ FAILURE")
# two launches per rank count, split by call family, so that each stays within the time of the
# GA matrix launch on as many ranks (profiles/r14/ga_fuzz/times.txt)
PARTS = {"math-elem-gemm": ("math", "elem", "gemm"), "trans-matrix-scan": ("trans", "matrix", "scan")}
assert sorted(f for p in PARTS.values() for f in p) == sorted(F.FAMILIES)
_results = {}   # (part, rank count) -> the RESULT lines of its ranks


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("part", list(PARTS))
def test_ga_fuzz_ranks(part, n):
    """every generated case runs -- none is skipped -- and agrees with the model bit for bit on every
    rank; the RESULT lines (dots, norms, the selected element and its subscripts, icount) are the
    same on every rank and on every rank count: exactly summable data and order-free results do
    not depend on how the arrays are cut"""
    generated = sum(entry[0] in PARTS[part] for entry in F.PLAN)   # the plan is the list: one case per entry
    t0 = time.perf_counter()
    outs = MP.launch_ok(None, n, extra_env={"GA_FUZZ_FAMILIES": ",".join(PARTS[part])})
    took = time.perf_counter() - t0
    ran = {int(ln.split()[1]) for out in outs for ln in out.splitlines() if ln.startswith("CASES ")}
    print(f"ga fuzz {part}: {n} ranks, {sorted(ran)} cases run of {generated} generated, {took:.2f} s")
    assert ran == {generated}
    for out in outs:
        assert f"CASES {generated} of {generated}" in out, out[-2000:]
    results = [[ln for ln in out.splitlines() if ln.startswith("RESULT ")] for out in outs]
    assert len(results[0]) > 10
    for s in results[1:]:
        assert s == results[0]
    _results[part, n] = results[0]
    for (p, m), other in _results.items():
        if p == part:
            assert other == results[0], f"the scalar results on {m} and on {n} ranks differ"
