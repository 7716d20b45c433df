"""GPU, GA layer: GA_Abs_value / GA_Add_constant / GA_Recip / GA_Elem_multiply / _divide /
_maximum / _minimum, their patch forms, the general path, NGA_Select_elem and the
zero-divisor abort, on 1, 2 and 3 ranks sharing one GPU (tests/ga_elem_worker.py is one
rank).  Expected values: the numpy restatement in test_gpu_ga_elem.py, compared as raw bits.

Every rank process runs under its own time limit (a watcher thread each); once a launch
ends in anything but the outcome its test expects, the remaining tests of this file start
nothing."""
import pytest

import mp_launch

MP = mp_launch.Launcher("ga_elem_worker.py", "e")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_ga_elem_ranks(n):
    """whole-array and patch forms on a 37 x 53 and a 5 x 6 x 7 array, in place, the general
    path (another block map, shifted patches, temporaries destroyed), NGA_Select_elem min and
    max for the six types -- equal to numpy's first occurrence in C order (checked by every
    rank) and the same SEL line on every rank -- the tie whose lower index lives on the higher
    rank, and a 2-element array, of which one of three ranks owns nothing"""
    outs = MP.launch_ok("all", n)
    for out in outs:
        for section in ("forms", "general", "select"):
            assert f"SECTION {section} OK" in out, out[-2000:]
        assert "GA on-device calls: fill" in out          # the existing line's text is kept
        assert "GA element-wise calls: abs" in out and "select" in out   # GA_Print_stats counts the new calls
    sels = [[ln for ln in out.splitlines() if ln.startswith("SEL ")] for out in outs]
    assert len(sels[0]) == 48 + (6 if n > 1 else 0) + 16, (len(sels[0]), sels[0])
    for s in sels[1:]:
        assert s == sels[0], (s, sels[0])
    if n > 1:
        ties = [ln for ln in sels[0] if ln.startswith("SEL tie-")]
        assert len(ties) == 6 and all(ln.endswith("[0, 1]") for ln in ties), ties


@pytest.mark.gpu
def test_ga_elem_divide_zero_divisor_aborts():
    """GA_Elem_divide with a single zero in g_b on 2 ranks: every rank -- the one whose block
    holds the zero and the other -- prints the zero-divisor message and ends through
    GA_Error with a non-zero status.  The kernel has completed and the stream is synchronised
    before that, so no rank is left waiting in a barrier (none is killed at its time limit)"""
    MP.expect_abort("abort-zero", 2, ["zero divisor"])
