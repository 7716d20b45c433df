"""GPU, GA layer: GA_Transpose / GA_Symmetrize on 1, 2 and 3 ranks sharing one GPU
(tests/ga_transpose_worker.py is one rank).  Results are compared as raw bits against numpy's
transpose and 0.5 * (A + A.T); random data has to give the same bits on every rank and on
every rank count.  The aborts run one process each.

Every rank process runs under its own time limit (a watcher thread each); once a launch
ends in anything but what it was started for, the remaining tests of this file start
nothing."""
import pytest

import mp_launch

MP = mp_launch.Launcher("ga_transpose_worker.py", "t")
N_TRANSPOSE, N_SYMM = 7, 4   # the calls of the worker's mode "all"
_tr_lines = {}   # rank count -> the "TR ..." lines of its run


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_ga_transpose_ranks(n):
    """B = A.T for one type per element size on REGULAR maps; differing irregular maps with a
    one-row block of B and a one-column block of A, and the mirror patch in the rank's own
    block; GA_Symmetrize of f64 and f32 as bits and equal to its own transpose; no array left
    alive; the calls counted on the new line of GA_Print_stats and the old line still there
    once; the sha256 of every random-data result the same on every rank, and the same as on
    the rank counts run before this one"""
    outs = MP.launch_ok("all", n)
    for r, out in enumerate(outs):
        for section in ("transpose", "maps", "symm", "bits"):
            assert f"SECTION {section} OK" in out, out[-2000:]
        new = [ln for ln in out.splitlines() if f"[{r}] GA transposes:" in ln]
        assert new == [f"[{r}] GA transposes: transpose {N_TRANSPOSE}, symmetrize {N_SYMM}"], new
        old = [ln for ln in out.splitlines() if f"[{r}] GA on-device calls: fill" in ln]
        assert len(old) == 1 and old[0].endswith("gemm 0"), out[-2000:]
    lines = [[ln for ln in out.splitlines() if ln.startswith("TR ")] for out in outs]
    assert len(lines[0]) == 3, lines[0]
    for ln in lines[1:]:
        assert ln == lines[0], (ln, lines[0])
    _tr_lines[n] = lines[0]
    for other, theirs in _tr_lines.items():
        assert theirs == lines[0], f"{n} ranks and {other} ranks gave different bits:\n{lines[0]}\n{theirs}"


@pytest.mark.gpu
@pytest.mark.parametrize("mode,message,env", [
    ("abort-same", "GA_Transpose: the arrays have to be different", None),
    ("abort-3d", "GA_Transpose: arrays of rank other than 2", None),
    ("abort-type", "GA_Transpose: types of the arrays differ", None),
    ("abort-dims", "GA_Transpose: dims of the arrays do not agree", None),
    ("abort-square", "GA_Symmetrize: the array is not square", None),
    ("abort-int", "GA_Symmetrize: type 1001 is neither C_DBL nor C_FLOAT", None),
    ("abort-host", "host segment", {"COMEX_AMD_SEGMENT": "host"}),
], ids=["same-array", "3-d", "types", "dims", "not-square", "int", "host-segment"])
def test_ga_transpose_aborts(mode, message, env):
    """each wrong call ends the process through GA_Error: the message and a non-zero status
    (the checks come before the call's first sync or launch)"""
    MP.expect_abort(mode, 1, [message], extra_env=env)
