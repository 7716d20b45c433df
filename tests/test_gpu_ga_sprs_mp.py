"""GPU, GA layer: the sparse arrays (NGA_Sprs_array_*) on 1, 2 and 3 ranks sharing one GPU
(tests/ga_sprs_worker.py is one rank), and two aborts on 2 ranks.  Expected values: the numpy
restatement in test_gpu_sprs.py of the whole matrix, compared as raw bits by every rank.

Every rank process runs under its own time limit (a watcher thread each); once a launch
ends in anything but the outcome its test expects, the remaining tests of this file start
nothing."""
import pytest

import mp_launch

MP = mp_launch.Launcher("ga_sprs_worker.py", "s", limit=120)
_digests = {}   # rank count -> the DIGEST lines of its ranks


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_ga_sprs_ranks(n):
    """assembly (elements dealt to the ranks by a seeded permutation, all added by rank 0, a rank adding
    none, 2 x 5 on 3 ranks, an empty row block, duplicates), the distributions, the block list and the
    block CSR read back through the access pointers; matvec with g_a / g_v under NGA_Create, a chunk and
    irregular maps, in place and through scratch; get_diag, shift_diag, scale, diag_left, diag_right,
    duplicate and destroy.  The same DIGEST lines on every rank AND on every rank count for inexact
    data; no global array left behind; the statistics line present once with every counter > 0"""
    outs = MP.launch_ok("all", n)
    for out in outs:
        for section in ("products", "others"):
            assert f"SECTION {section} OK" in out, out[-2000:]
        assert "GA on-device calls: fill" in out and "GA sparse calls: enum" in out   # existing lines kept
        m = [ln for ln in out.splitlines() if "GA sparse-array calls: assemble" in ln]
        assert len(m) == 1, out[-2000:]
        counts = dict(kv.rsplit(" ", 1) for kv in m[0].split("calls: ")[1].split(", "))
        assert set(counts) == {"assemble", "matvec", "get_diag", "shift_diag", "scale", "diag_left", "diag_right"}
        assert all(int(v) > 0 for v in counts.values()), counts
        assert int(counts["matvec"]) > int(counts["assemble"]) > int(counts["scale"])
        routes = [ln for ln in out.splitlines() if ln.startswith("ROUTES ")]
        assert len(routes) == 1
    for tag, least in (("DIGEST ", 150), ("DIGESTN ", 30)):
        digests = [[ln for ln in out.splitlines() if ln.startswith(tag)] for out in outs]
        assert len(digests[0]) > least, len(digests[0])
        for s in digests[1:]:
            assert s == digests[0]
        if tag == "DIGEST ":
            _digests[n] = digests[0]
    for other in _digests.values():   # inexact data: the same bits on any rank count (the order contract)
        assert other == _digests[n]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,message", [("abort-matvec", "has 4 elements, 6 are needed"),
                                          ("abort-add", "has been assembled already")])
def test_ga_sprs_aborts(mode, message):
    """on 2 ranks: every rank prints the message and ends through GA_Error with a non-zero status; none is
    killed at its time limit and none reaches the line after the call"""
    MP.expect_abort(mode, 2, [message])
