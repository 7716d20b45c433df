"""GPU, GA layer: NGA_Sprs_array_matmat_multiply on 1, 2 and 3 ranks sharing one GPU (tests/ga_spgemm_worker.py is
one rank), the 2 x 5 times 5 x 3 product on 4 ranks, where two ranks own no row, and two aborts on 2 ranks.
Expected values: the numpy restatement of test_gpu_spgemm.py of the whole product, compared as raw bits by every
rank, through the add_element construction of its triples.

Every rank process runs under its own time limit (a watcher thread each); once a launch ends in anything but the
outcome its test expects, the remaining tests of this file start nothing."""
import pytest

import mp_launch

MP = mp_launch.Launcher("ga_spgemm_worker.py", "g", limit=120)
_digests = {}   # rank count -> the DIGEST lines of its ranks


def stats(out, title):
    m = [ln for ln in out.splitlines() if title in ln]
    assert len(m) == 1, out[-2000:]
    return dict(kv.rsplit(" ", 1) for kv in m[0].split("calls: ")[1].split(", "))


def check_stats(out, calls):
    assert stats(out, "GA sparse-sparse calls:") == {"matmat": str(calls)}
    assert set(stats(out, "GA sparse-product calls:")) == {"sprsdns", "from_dense", "from_sparse"}
    old = stats(out, "GA sparse-array calls:")
    assert set(old) == {"assemble", "matvec", "get_diag", "shift_diag", "scale", "diag_left", "diag_right"}
    return old


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_ga_spgemm_ranks(n):
    """a 37 x 53 A with an empty row block and duplicates times a 53 x 41 B with and without duplicates, A A for a
    40 x 40, the 2 x 5 times 5 x 3, a 3 x 40 times a 40 x 100 000 whose first row takes the kernels' fallback over
    several windows; f64, complex f32 and C_LONG.  C through access_col_block, col_block_list and the
    distributions equals the add_element construction of the model's triples; matvec on C; the dense identity; the
    route counters predicted; the operands and the live arrays unchanged; a second call the same bits; the new
    statistics line once with the old lines as they were, matmat not counted as an assemble; the same DIGEST lines
    on every rank and on every rank count"""
    outs = MP.launch_ok("all", n)
    for out in outs:
        assert "SECTION products OK" in out, out[-2000:]
        old = check_stats(out, 30)   # 3 types x 5 pairs x 2 calls
        # per pair: A, B (not for A A), the add_element construction of C; nothing else assembles
        assert int(old["assemble"]) == 3 * (3 + 3 + 2 + 3 + 3) and int(old["matvec"]) == 3 * 5 * 3
        assert len([ln for ln in out.splitlines() if ln.startswith("ROUTES ")]) == 1
    digests = [[ln for ln in out.splitlines() if ln.startswith("DIGEST ")] for out in outs]
    assert len(digests[0]) == 15, len(digests[0])
    for s in digests[1:]:
        assert s == digests[0]
    _digests[n] = digests[0]
    for other in _digests.values():   # inexact data: the same bits on any rank count (the order contract)
        assert other == _digests[n]


@pytest.mark.gpu
def test_ga_spgemm_ranks_without_rows():
    """4 ranks, 2 x 5 times 5 x 3: the ranks 1 and 3 own no row of A, launch nothing and take part in every sync;
    rank 2's part of B is empty"""
    outs = MP.launch_ok("four", 4)
    for out in outs:
        assert "SECTION four OK" in out
        check_stats(out, 6)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,message", [("abort-types", "the types of the two sparse arrays differ"),
                                          ("abort-dims", "A has 6 columns, B has 5 rows")])
def test_ga_spgemm_aborts(mode, message):
    """on 2 ranks: every rank prints the message and ends through GA_Error with a non-zero status; none is killed
    at its time limit and none reaches the line after the call"""
    MP.expect_abort(mode, 2, [message])
