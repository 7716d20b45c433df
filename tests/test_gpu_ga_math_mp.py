"""GPU, GA layer: GA_Fill / GA_Scale / GA_Add / GA_Copy / GA_?dot, their patch forms,
the general path and the aborts, on 1, 2 and 3 ranks sharing one GPU
(tests/ga_math_worker.py is one rank).  Expected values: the numpy restatement in
test_gpu_ga_math.py, compared as raw bits.

Every rank process runs under its own time limit (a watcher thread each); once a
launch ends in anything but the outcome its test expects, the remaining tests of this
file start nothing."""
import pytest

import mp_launch

MP = mp_launch.Launcher("ga_math_worker.py", "m")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_ga_math_ranks(n):
    """whole-array calls, patch forms, the general path (another block map, shifted
    patches, temporaries destroyed) and the ordering against a pending NGA_NbAcc;
    every dot product is the same bits on every rank"""
    outs = MP.launch_ok("all", n)
    for out in outs:
        for section in ("whole", "patch", "general", "order"):
            assert f"SECTION {section} OK" in out, out[-2000:]
        assert "GA on-device calls: fill" in out   # GA_Print_stats counts the new calls
    dots = [[ln for ln in out.splitlines() if ln.startswith("DOT ")] for out in outs]
    assert len(dots[0]) == 13, dots[0]
    for d in dots[1:]:
        assert d == dots[0], (d, dots[0])


@pytest.mark.gpu
def test_ga_math_64bit_offsets():
    """a 1-D C_DBL array of 2**29 + 3 elements (byte offsets past 2**32): GA_Fill,
    GA_Ddot = 2**29 + 3 exactly, NGA_Get of the last three elements and of three
    straddling byte offset 2**32"""
    MP.launch_ok("big", 1)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2])
def test_ga_math_tall_arrays(n):
    """C_DBL and C_FLOAT arrays of [70001 * n + 1, 3]: NGA_Fill_patch, NGA_Scale_patch,
    NGA_Add_patch and the dot products on a patch of which every rank holds more than 65535
    rows of two elements (the worker asserts it), and GA_Fill on the whole array; the
    comparison covers the column outside the patch and the first and last rows"""
    outs = MP.launch_ok("tall", n)
    dots = [[ln for ln in out.splitlines() if ln.startswith("DOT ")] for out in outs]
    assert len(dots[0]) == 2, dots[0]
    for d in dots[1:]:
        assert d == dots[0], (d, dots[0])


@pytest.mark.gpu
@pytest.mark.parametrize("mode,message,env", [
    ("abort-type", "type mismatch", None),
    ("abort-trans", "transposed patches", None),
    ("abort-host", "host segment", {"COMEX_AMD_SEGMENT": "host"}),
], ids=["type", "transpose", "host-segment"])
def test_ga_math_aborts(mode, message, env):
    """GA_Ddot on a C_FLOAT array, a transposed NGA_Copy_patch and GA_Fill on an array in
    a host segment end every rank through GA_Error: the message and a non-zero status
    (the checks come before the call's first sync or launch)"""
    MP.expect_abort(mode, 2, [message], extra_env=env)
