"""CPU: tests/mp_launch.py, the rank launcher of the multi-rank GA tests, with
tests/mp_stub_worker.py as the rank: the environment of a launch, the time limit per rank, the
abort rule, and that an instance starts nothing more once one of its launches went wrong."""
import glob
import time

import pytest

import mp_launch

Failed = pytest.fail.Exception
LIMIT = 2   # seconds: the stub's hang mode is killed at it


def stub(**kw):
    return mp_launch.Launcher("mp_stub_worker.py", "q", **kw)


def env_of(out):
    return dict(ln[4:].split("=", 1) for ln in out.splitlines() if ln.startswith("ENV "))


def test_ranks_in_order_sharing_port_and_job_id():
    res = stub().launch("ok", 3)
    envs = [env_of(out) for _, out in res]
    assert [rc for rc, _ in res] == [0, 0, 0]
    assert [e["RANK"] for e in envs] == ["0", "1", "2"] == [e["LOCAL_RANK"] for e in envs]
    for r, (_, out) in enumerate(res):
        assert f"RANK {r} OK" in out and "ARGS ['ok']" in out
    assert {e["WORLD_SIZE"] for e in envs} == {"3"} and {e["MASTER_ADDR"] for e in envs} == {"127.0.0.1"}
    assert {e["COMEX_AMD_STAGING_MB"] for e in envs} == {"16"}
    ports = {e["MASTER_PORT"] for e in envs}
    assert len(ports) == 1 and int(ports.pop()) > 0
    assert {e["COMEX_AMD_JOBID"] for e in envs} == {"q" + envs[0]["MASTER_PORT"]}


def test_stack_dump_time_is_the_limit_less_15_and_no_mode_is_no_argument():
    m = stub(limit=90)
    assert env_of(m.launch("ok", 1)[0][1])["TEST_STACK_DUMP_S"] == "75"
    (rc, out), = m.launch(None, 1, limit=60, extra_env={"STUB_SAY": "said"})
    assert rc == 0 and env_of(out)["TEST_STACK_DUMP_S"] == "45" and "ARGS []" in out and "said" in out
    assert [f"RANK {r} OK" in out for r, out in enumerate(m.launch_ok("ok", 2))] == [True, True]


def test_a_rank_past_its_limit_is_killed_and_the_others_are_returned():
    t0 = time.perf_counter()
    res = stub().launch("hang", 3, limit=LIMIT)
    assert time.perf_counter() - t0 < LIMIT + 5
    assert res[0][0] == 124 and res[0][1].endswith(f"\n[killed after {LIMIT} s]") and "RANK 0 OK" not in res[0][1]
    for r in (1, 2):
        assert res[r][0] == 0 and f"RANK {r} OK" in res[r][1]


def test_nothing_is_started_after_a_launch_went_wrong(tmp_path):
    m, other = stub(), stub()
    with pytest.raises(Failed, match="rank 0 rc=5"):
        m.launch_ok("fail", 2)
    started = str(tmp_path / "started")
    for call in (lambda: m.launch("ok", 2, extra_env={"STUB_STARTED": started}),
                 lambda: m.launch_ok("ok", 1, extra_env={"STUB_STARTED": started}),
                 lambda: m.expect_abort("abort", 1, [], extra_env={"STUB_STARTED": started})):
        with pytest.raises(Failed, match=r"not started: .*\(fail on 2 ranks: rank 0 status 5\)"):
            call()
    assert glob.glob(started + ".*") == []
    # the rule is per instance: a second one still launches
    assert [rc for rc, _ in other.launch("ok", 2, extra_env={"STUB_STARTED": started})] == [0, 0]
    assert sorted(glob.glob(started + ".*")) == [started + ".0", started + ".1"]


def test_launch_ok_needs_the_rank_line_as_well_as_status_0():
    m = stub()
    with pytest.raises(Failed, match="rank 1 rc=0"):
        m.launch_ok("ok", 2, extra_env={"RANK": "0"})      # status 0, but rank 1 says RANK 0 OK
    assert m.broken == ["ok on 2 ranks: rank 1 status 0"]


def test_expect_abort():
    res = stub().expect_abort("abort", 2, ["stub: the message", "the mess"])
    assert [rc for rc, _ in res] == [1, 1]
    for mode, n, messages, env, why in (
            ("ok", 1, [], None, "rank 0 rc=0"),                                   # ended well: status 0
            ("abort", 2, ["another message"], None, "rank 0 rc=1"),               # a message is missing
            ("abort", 1, [], {"STUB_SAY": "NOT REACHED"}, "rank 0 rc=1"),         # the call returned
            ("fail", 1, [], {"STUB_SAY": "ABORT EXPECTED"}, None),                # status 5 with the line: accepted
            ("hang", 1, [], {"STUB_SAY": "ABORT EXPECTED"}, "rank 0 rc=124")):    # killed at the limit
        m = stub()
        if why is None:
            m.expect_abort(mode, n, messages, limit=LIMIT, extra_env=env)
            assert m.broken == []
            continue
        with pytest.raises(Failed, match=why):
            m.expect_abort(mode, n, messages, limit=LIMIT, extra_env=env)
        assert len(m.broken) == 1 and m.broken[0].startswith(f"{mode}: rank 0 status")


def test_tails_marker_window():
    m = stub(marker="FUZZ FAILURE")
    long = "x" * 5000
    res = [(1, long + "FUZZ FAILURE here" + long), (0, long + "end")]
    t = m.tails(res)
    assert "--- rank 0: status 1 ---\nFUZZ FAILURE here" in t and "--- rank 1: status 0 ---\n" + "x" * 2497 + "end" in t
    assert len(t.split("--- rank 1")[0]) < 3100
    assert stub().tails(res).count("FUZZ FAILURE") == 0          # without a marker: the last 2500 characters
    assert stub().tails(res, marker="here").count("here" + "x" * 2996) == 1
