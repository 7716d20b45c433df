"""GPU, GA layer: GA_Shift_diagonal / GA_Set_diagonal / GA_Zero_diagonal / GA_Add_diagonal /
GA_Get_diag, GA_Scale_rows / GA_Scale_cols, GA_Norm1 / GA_Norm_infinity and the wrong-length
abort, on 1, 2 and 3 ranks sharing one GPU (tests/ga_matrix_worker.py is one rank).  Expected
values: the numpy restatement in test_gpu_matrix.py, compared as raw bits by every rank.

Every rank process runs under its own time limit (a watcher thread each); once a launch
ends in anything but the outcome its test expects, the remaining tests of this file start
nothing."""
import pytest

import mp_launch

MP = mp_launch.Launcher("ga_matrix_worker.py", "m")
_norms = {}   # rank count -> the NORM lines of its ranks


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_ga_matrix_ranks(n):
    """the nine calls on 37 x 53, 53 x 37 and 40 x 40 arrays in C_DBL, C_FLOAT, C_INT, C_LONG and
    C_DCPL, g_a and g_v each under a REGULAR and an irregular map (the vector's range in place and
    through scratch), both round trips, a 53 x 7 array of which a rank owns no diagonal element,
    a 2-element vector of which one of three ranks owns nothing, the norms equal to the
    restatement on every rank count -- the same NORM lines on every rank and on every count --
    no temporary left behind, and the new statistics line beside the existing ones"""
    outs = MP.launch_ok("all", n)
    for out in outs:
        for section in ("forms", "corners", "norms"):
            assert f"SECTION {section} OK" in out, out[-2000:]
        assert "GA on-device calls: fill" in out and "GA element-wise calls: abs" in out   # existing lines kept
        m = [ln for ln in out.splitlines() if "GA matrix calls: diagonal" in ln]
        assert len(m) == 1, out[-2000:]
        counts = dict(kv.rsplit(" ", 1) for kv in m[0].split("calls: ")[1].split(", "))
        assert int(counts["diagonal"]) > 0 and int(counts["scale_rows"]) == int(counts["scale_cols"]) > 0
        assert int(counts["norm1"]) > 0 and int(counts["norm_infinity"]) == 2 * int(counts["norm1"])
    norms = [[ln for ln in out.splitlines() if ln.startswith("NORM ")] for out in outs]
    assert len(norms[0]) > 50
    for s in norms[1:]:
        assert s == norms[0]
    _norms[n] = norms[0]
    for other in _norms.values():   # exactly summable data and maxima: the same bits on any rank count
        assert other == norms[0]


@pytest.mark.gpu
def test_ga_scale_rows_wrong_length_aborts():
    """GA_Scale_rows with a g_v one element too long on 2 ranks: every rank prints the message
    and ends through GA_Error with a non-zero status, before the first sync: none is killed at its
    time limit and none reaches the line after the call"""
    MP.expect_abort("abort-len", 2, ["21 elements, 20 are needed"])
