"""GPU, GA layer: GA_Patch_enum, GA_Scan_copy, GA_Scan_add, GA_Pack, GA_Unpack and the
too-short-destination abort, on 1, 2 and 3 ranks sharing one GPU (tests/ga_scan_worker.py is one
rank).  Expected values: the numpy restatement in test_gpu_scan.py, compared as raw bits by every
rank.

Every rank process runs under its own time limit (a watcher thread each); once a launch
ends in anything but the outcome its test expects, the remaining tests of this file start
nothing."""
import pytest

import mp_launch

MP = mp_launch.Launcher("ga_scan_worker.py", "s")
_digests = {}   # rank count -> the DIGEST lines of its ranks


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_ga_scan_ranks(n):
    """the ten (lo, hi, excl) cases of scan_addc.c and the cases of packc.c, unpackc.c and
    patch_enumc.c at 3001 elements, values in C_INT, C_LONG, C_FLOAT, C_DBL and C_DCPL under masks
    in C_INT, C_DBL and C_SCPL, REGULAR and irregular maps, set mask elements just outside the
    range; an array of 2 elements (on 3 ranks one owns nothing), a middle rank without a set
    element, a range that cuts inside blocks and excludes the last rank, a mask with none set,
    GA_Pack into another map of exactly icount elements and the round trip through GA_Unpack.
    The same DIGEST lines on every rank and on every rank count, no temporary left behind, and
    the new statistics line beside the existing ones"""
    outs = MP.launch_ok("all", n)
    for out in outs:
        for section in ("enums", "scans", "packs", "corners"):
            assert f"SECTION {section} OK" in out, out[-2000:]
        assert "GA on-device calls: fill" in out and "GA matrix calls: diagonal" in out   # existing lines kept
        m = [ln for ln in out.splitlines() if "GA sparse calls: enum" in ln]
        assert len(m) == 1, out[-2000:]
        counts = dict(kv.rsplit(" ", 1) for kv in m[0].split("calls: ")[1].split(", "))
        assert set(counts) == {"enum", "scan_copy", "scan_add", "pack", "unpack"}
        assert all(int(v) > 0 for v in counts.values()), counts
        assert int(counts["scan_add"]) > int(counts["scan_copy"]) and int(counts["pack"]) > int(counts["unpack"])
    digests = [[ln for ln in out.splitlines() if ln.startswith("DIGEST ")] for out in outs]
    assert len(digests[0]) > 500
    for s in digests[1:]:
        assert s == digests[0]
    _digests[n] = digests[0]
    for other in _digests.values():   # integers and exactly summable data: the same bits on any rank count
        assert other == digests[0]


@pytest.mark.gpu
def test_ga_pack_destination_too_short_aborts():
    """GA_Pack of 40 set elements into a g_dst of 39 on 2 ranks: every rank prints the message with
    both numbers and ends through GA_Error with a non-zero status: none is killed at its time limit
    and none reaches the line after the call"""
    MP.expect_abort("abort-short", 2, ["40 set elements", "of 39 elements"])
