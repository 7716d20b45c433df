"""bench.py --dump-outputs: which elements it writes (CPU) and that a plain run's dump
is what the oracle computes from the same seeds for the last timed step (GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_patch_offsets_follow_the_descriptor():
    """3 levels, rows of 3 f64, strides that leave gaps: the order comex walks a
    strided descriptor (level 0 contiguous, then level 1, then level 2)."""
    count, strides = [24, 4, 2], [40, 400]
    want = [(k * 400 + j * 40) // 8 + i for k in range(2) for j in range(4) for i in range(3)]
    assert bench.patch_offsets(count, strides).tolist() == want
    assert bench.patch_offsets([64], []).tolist() == list(range(8))


def test_dump_indices_small_patch_is_whole():
    count, strides = [24, 4, 2], [40, 400]
    idx = bench.dump_indices(count, strides)
    span = bench.span_bytes(count, strides) // 8
    assert idx["patch"].tolist() == bench.patch_offsets(count, strides).tolist()
    assert sorted(idx["patch"].tolist() + idx["gap"].tolist()) == list(range(span))


@pytest.mark.parametrize("workload", sorted(bench.WORKLOADS))
def test_dump_indices_fixed_and_within_the_size_limit(workload):
    """Every workload: the same elements in every call, patch and gap disjoint and inside
    the span, and the two float64 arrays together under 64 MB."""
    _, count, sstr, dstr, _ = bench.WORKLOADS[workload]
    for strides in sorted({tuple(sstr), tuple(dstr)}):
        a = bench.dump_indices(count, strides)
        span = bench.span_bytes(count, strides) // 8
        if workload == "H":
            b = bench.dump_indices(count, strides)
            assert all(np.array_equal(a[k], b[k]) for k in ("patch", "gap"))
        assert a["patch"].size == min(bench.patch_bytes(count) // 8, bench.DUMP_PATCH_MAX)
        assert a["gap"].size == min(span - bench.patch_bytes(count) // 8, bench.DUMP_GAP_MAX)
        assert (a["patch"].size + a["gap"].size) * 8 <= 64e6
        both = np.concatenate([a["patch"], a["gap"]])
        assert both.min() >= 0 and both.max() < span
        in_patch = np.zeros(span, bool)
        in_patch[bench.patch_offsets(count, strides)] = True
        assert in_patch[a["patch"]].all() and not in_patch[a["gap"]].any()


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_destination(oracle, tmp_path):
    """A plain run (no --full) of the headline workload: --steps sets the timed steps, the
    line carries ms_per_step and nothing that takes a run of its own, and the dump is,
    bit for bit, the oracle's accumulate applied to the same seeded buffers as often as
    the timed steps visited the last step's buffer set."""
    steps, sets = 11, 8
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "3", "--warmup-ms", "0", "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["metric"] == bench.METRIC and line["unit"] == "GiB/s" and line["dtype"] == "f64"
    assert line["higher_is_better"] is True and line["full"] is False
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert "blocking_api" not in line and "host_inclusive" not in line
    assert sorted(os.listdir(tmp_path)) == ["gap.npy", "patch.npy"]

    op, count, sstr, dstr, _ = bench.WORKLOADS["H"]
    last = (steps - 1) % sets
    visits = len([i for i in range(steps) if i % sets == last])
    assert visits == 2
    src = oracle.fill(np.empty(bench.span_bytes(count, sstr) // 8), 0x5EED0000).view(np.uint8)
    dst = oracle.fill(np.empty(bench.span_bytes(count, dstr) // 8), 0x5EED0001 + 977 * last)
    untouched = dst.copy()
    for _ in range(visits):
        oracle.accs(op, bench.SCALE[op], src, 0, sstr, dst.view(np.uint8), 0, dstr, count, len(count) - 1)
    idx = bench.dump_indices(count, dstr)
    patch, gap = np.load(tmp_path / "patch.npy"), np.load(tmp_path / "gap.npy")
    assert patch.dtype == np.float64 and gap.dtype == np.float64
    assert np.array_equal(patch, dst[idx["patch"]])
    assert not np.array_equal(patch, untouched[idx["patch"]])
    assert np.array_equal(gap, untouched[idx["gap"]])
