"""GPU, GA layer: GA_Zgemm / GA_Cgemm / NGA_Matmul_patch on complex arrays, on 1, 2 and 3
ranks sharing one GPU (tests/ga_zgemm_worker.py is one rank).  Exact integer data is compared
as raw bits against the integer product; random data has to give the same bits on every rank
and on every rank count.  GA_Dgemm with trans 'C' still ends through GA_Error.

Every rank process runs under its own time limit (a watcher thread each); once a launch
ends in anything but what it was started for, the remaining tests of this file start nothing."""
import pytest

import mp_launch

MP = mp_launch.Launcher("ga_zgemm_worker.py", "z")
_gemm_lines = {}   # rank count -> the "ZGEMM ..." lines of its run


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_ga_zgemm_ranks(n):
    """exact products of both complex types on REGULAR maps (NN, TN, CN, NC; three panels of
    k), shifted patches on three differing irregular maps (a one-row block of C with 2 and 3
    ranks), no array left alive, the calls counted by GA_Print_stats under gemm; the sha256 of
    every random-data C (a second panel through beta = (1, 0)) is the same on every rank, and
    the same as on the rank counts run before this one"""
    outs = MP.launch_ok("all", n)
    for r, out in enumerate(outs):
        for section in ("exact", "maps", "bits"):
            assert f"SECTION {section} OK" in out, out[-2000:]
        stats = [ln for ln in out.splitlines() if f"[{r}] GA on-device calls: fill" in ln]
        assert len(stats) == 1, out[-2000:]
        calls = 8 + 2 + (1 if n == 2 else 0) + 6   # exact, maps (+ the one-row case), bits
        assert stats[0].endswith(f"gemm {calls}"), stats[0]
    lines = [[ln for ln in out.splitlines() if ln.startswith("ZGEMM ")] for out in outs]
    assert len(lines[0]) == 6, lines[0]
    for ln in lines[1:]:
        assert ln == lines[0], (ln, lines[0])
    _gemm_lines[n] = lines[0]
    for other, theirs in _gemm_lines.items():
        assert theirs == lines[0], f"{n} ranks and {other} ranks gave different bits:\n{lines[0]}\n{theirs}"


@pytest.mark.gpu
def test_ga_dgemm_still_refuses_conjugate_transpose():
    """the negative control: 'C' is for complex arrays only, GA_Dgemm answers as before --
    through GA_Error, with its message and a non-zero status, before any sync or launch"""
    MP.expect_abort("abort-dgemm-c", 1, ["GA_Dgemm: trans 'C' is not one of N n T t"])
