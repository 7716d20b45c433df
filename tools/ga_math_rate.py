#!/usr/bin/env python3
"""Rates of gaamd_patch_fill / _scale / _add / _dot on the MI355X (needs the GPU; fails
without one).

Two geometries, f64: one contiguous run of 1 GiB, and the headline patch of bench.py
(2048 x 4096 doubles, leading dimension 8192: 64 MiB of payload in a 256 MiB span).
Every figure is one HIP-event pair around enough back-to-back calls to last >= 0.2 s,
after warm-up, on buffer sets that rotate call by call (>= 1 GiB in total, so the
Infinity Cache cannot hold them, as bench.py does).  On the headline patch the
gaamd_strided f64 accumulate -- the same bytes as gaamd_patch_add: two loads and one
store per element -- is measured in the same process, alternating with the add.

bytes moved per element: fill 8, scale 16, add 24, dot 16, accumulate 24.
gaamd_patch_dot returns its result, so each call ends in a stream synchronisation:
its figure is the rate of the call, launch and wait included.

Writes JSON (default profiles/r07/ga_math/rates.json): per figure the GB/s of every
round, their median, and the share of the 8 TB/s HBM peak.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import ga_amd  # noqa: E402

PEAK = 8.0e12
DBL = ga_amd.COMEX_ACC_DBL
BYTES_PER_ELEM = {"fill": 8, "scale": 16, "add": 24, "dot": 16, "acc": 24}


class Geometry:
    def __init__(self, name, count, stride, sets):
        self.name, self.count, self.stride = name, count, stride
        self.elems = int(np.prod(count))
        self.span = (count[0] * 8) if len(count) == 1 else stride[-1] * count[-1]
        self.sets = []
        L = ga_amd.lib()
        for s in range(sets):
            bufs = [ga_amd.DeviceBuffer(self.span) for _ in range(3)]
            for k, b in enumerate(bufs):
                assert L.gaamd_fill(ctypes.c_void_p(b.ptr), self.span // 8, 0, 1000 + 10 * s + k, None) == 0
            self.sets.append(bufs)
        ga_amd.sync()
        self.total_bytes = 3 * sets * self.span

    def free(self):
        for bufs in self.sets:
            for b in bufs:
                b.free()


def make_calls(g):
    L = ga_amd.lib()
    cnt, st = ga_amd.ll_array(g.count), ga_amd.ll_array(g.stride)
    one, half = np.array([1.0]), np.array([0.5])
    onep, halfp = one.ctypes.data_as(ctypes.c_void_p), half.ctypes.data_as(ctypes.c_void_p)
    res = np.zeros(2)
    resp = res.ctypes.data_as(ctypes.c_void_p)
    nd = len(g.count)
    # the accumulate's geometry: bytes in count[0], int strides
    icnt = ga_amd.int_array([g.count[0] * 8] + list(g.count[1:]))
    ist = ga_amd.int_array(g.stride)
    p = ctypes.c_void_p

    def fill(a, b, c):
        return L.gaamd_patch_fill(DBL, onep, p(c.ptr), st, cnt, nd, None)

    def scale(a, b, c):
        return L.gaamd_patch_scale(DBL, onep, p(c.ptr), st, cnt, nd, None)

    def add(a, b, c):
        return L.gaamd_patch_add(DBL, halfp, p(a.ptr), st, halfp, p(b.ptr), st, p(c.ptr), st, cnt, nd, None)

    def dot(a, b, c):
        return L.gaamd_patch_dot(DBL, p(a.ptr), st, p(b.ptr), st, cnt, nd, resp, None)

    def acc(a, b, c):
        return L.gaamd_strided(DBL, halfp, p(a.ptr), ist, p(c.ptr), ist, icnt, nd - 1, None)

    keep = (one, half, res, cnt, st, icnt, ist)
    return {"fill": fill, "scale": scale, "add": add, "dot": dot, "acc": acc}, keep


def timed(g, fn, reps):
    L = ga_amd.lib()
    e0, e1 = L.gaamd_event_create(), L.gaamd_event_create()
    ga_amd.sync()
    L.gaamd_event_record(e0, None)
    for i in range(reps):
        rc = fn(*g.sets[i % len(g.sets)])
        assert rc == 0, rc
    L.gaamd_event_record(e1, None)
    L.gaamd_event_sync(e1)
    ms = L.gaamd_event_elapsed_ms(e0, e1)
    L.gaamd_event_destroy(e0)
    L.gaamd_event_destroy(e1)
    return ms * 1e-3


def measure(g, name, fn, min_s, reps_known=None):
    if reps_known is None:
        timed(g, fn, 2 * len(g.sets))                       # warm-up: every set once or twice
        est = timed(g, fn, 4 * len(g.sets)) / (4 * len(g.sets))
        reps_known = max(8, int(1.25 * min_s / est) + 1)
    s = timed(g, fn, reps_known)
    gbs = g.elems * BYTES_PER_ELEM[name] * reps_known / s / 1e9
    return gbs, s, reps_known


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "ga_math", "rates.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    args = ap.parse_args()
    L = ga_amd.lib()
    if L.gaamd_device_count() < 1:
        sys.exit("ga_math_rate.py needs the MI355X: no HIP device is visible")
    assert ga_amd.comex_init() == 0
    out = {"peak_bytes_per_s": PEAK, "min_seconds_per_figure": args.min_seconds, "rounds": args.rounds,
           "bytes_per_element": BYTES_PER_ELEM, "geometries": {}}
    try:
        # one geometry at a time: its buffers are freed before the next is allocated
        for gname, count, stride, sets, names in (
                ("contiguous_1GiB_f64", [1 << 27], [], 2, ["fill", "scale", "add", "dot"]),
                ("headline_2048x4096_ld8192_f64", [2048, 4096], [8192 * 8], 4,
                 ["acc", "add", "fill", "scale", "dot"])):
            g = Geometry(gname, count, stride, sets)
            calls, keep = make_calls(g)
            figs = {n: {"gbs": [], "seconds": [], "reps": None} for n in names}
            for _ in range(args.rounds):        # the figures alternate within a round
                for n in names:
                    gbs, s, reps = measure(g, n, calls[n], args.min_seconds, figs[n]["reps"])
                    figs[n]["reps"] = reps
                    figs[n]["gbs"].append(round(gbs, 1))
                    figs[n]["seconds"].append(round(s, 4))
            for n in names:
                med = statistics.median(figs[n]["gbs"])
                figs[n]["median_gbs"] = med
                figs[n]["share_of_peak"] = round(med * 1e9 / PEAK, 4)
                print(f"{gname:32s} {n:6s} {med:8.1f} GB/s  {100 * med * 1e9 / PEAK:5.1f} % of peak  "
                      f"rounds {figs[n]['gbs']}", flush=True)
            if "acc" in figs:
                ratios = [round(a / b, 4) for a, b in zip(figs["add"]["gbs"], figs["acc"]["gbs"])]
                figs["add_over_acc"] = {"per_round": ratios, "median": statistics.median(ratios), "target": 0.95}
                print(f"{gname:32s} add / accumulate per round {ratios}", flush=True)
            out["geometries"][gname] = {"count_elements": count, "stride_bytes": stride, "buffer_sets": sets,
                                        "rotating_bytes": g.total_bytes, "figures": figs}
            g.free()
    finally:
        ga_amd.comex_finalize()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
