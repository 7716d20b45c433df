"""GPU, GA layer: NGA_Sprs_array_sprsdns_multiply, _create_from_dense and _create_from_sparse on 1, 2 and
3 ranks sharing one GPU (tests/ga_spmm_worker.py is one rank), the 2 x 5 matrix on 4 ranks, where a
rank writes its rows through scratch, and two aborts on 2 ranks.  Expected values: the numpy
restatements of test_gpu_sprs.py / test_gpu_spmm.py of the whole matrix, compared as raw bits by
every rank.

Every rank process runs under its own time limit (a watcher thread each); once a launch ends in
anything but the outcome its test expects, the remaining tests of this file start nothing."""
import pytest

import mp_launch

MP = mp_launch.Launcher("ga_spmm_worker.py", "m", limit=120)
_digests = {}   # rank count -> the DIGEST lines of its ranks


def product_stats(out):
    m = [ln for ln in out.splitlines() if "GA sparse-product calls:" in ln]
    assert len(m) == 1, out[-2000:]
    return dict(kv.rsplit(" ", 1) for kv in m[0].split("calls: ")[1].split(", "))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_ga_spmm_ranks(n):
    """S B for a 37 x 53 matrix with an empty row block and duplicates, the 2 x 5 one and a block-diagonal one;
    f64, complex f32 and C_LONG; n = 1, 5, 70; B under NGA_Create, a chunk and the column cuts; the four
    route counters predicted from the block maps; C through NGA_Get and through each rank's own block; C on
    the row cuts; create_from_dense under three kinds of map against the add_element construction;
    create_from_sparse against the model; the round trip.  The same DIGEST lines on every rank AND on every
    rank count for inexact data; no global array left behind; the new statistics line once, the old one as
    it was"""
    outs = MP.launch_ok("all", n)
    for out in outs:
        for section in ("products", "conversions"):
            assert f"SECTION {section} OK" in out, out[-2000:]
        counts = product_stats(out)
        assert set(counts) == {"sprsdns", "from_dense", "from_sparse"}
        assert all(int(v) > 0 for v in counts.values()), counts
        old = [ln for ln in out.splitlines() if "GA sparse-array calls: assemble" in ln]
        assert len(old) == 1, out[-2000:]
        old = dict(kv.rsplit(" ", 1) for kv in old[0].split("calls: ")[1].split(", "))
        assert set(old) == {"assemble", "matvec", "get_diag", "shift_diag", "scale", "diag_left", "diag_right"}
        assert int(old["assemble"]) > 0 and int(old["matvec"]) == 0
        assert len([ln for ln in out.splitlines() if ln.startswith("ROUTES ")]) == 1
    for tag, least in (("DIGEST ", 60), ("DIGESTN ", 30)):
        digests = [[ln for ln in out.splitlines() if ln.startswith(tag)] for out in outs]
        assert len(digests[0]) >= least, len(digests[0])
        for s in digests[1:]:
            assert s == digests[0]
        if tag == "DIGEST ":
            _digests[n] = digests[0]
    for other in _digests.values():   # inexact data: the same bits on any rank count (the order contract)
        assert other == _digests[n]


@pytest.mark.gpu
def test_ga_spmm_rows_in_another_ranks_block():
    """4 ranks, 2 x 5: rank 2 owns row 1, which lies in rank 1's block of the product: through scratch and put"""
    outs = MP.launch_ok("four", 4)
    for out in outs:
        assert "SECTION four OK" in out
        assert int(product_stats(out)["sprsdns"]) == 6


@pytest.mark.gpu
@pytest.mark.parametrize("mode,message", [("abort-rows", "has 4 rows, 6 are needed"),
                                          ("abort-rank1", "has rank 1, a matrix of rank 2 is needed")])
def test_ga_spmm_aborts(mode, message):
    """on 2 ranks: every rank prints the message and ends through GA_Error with a non-zero status; none is
    killed at its time limit and none reaches the line after the call"""
    MP.expect_abort(mode, 2, [message])
