#!/usr/bin/env python3
"""Rates of gaamd_scale_rows / gaamd_scale_cols / gaamd_patch_norm on the MI355X, each beside
its yardstick in the same process (needs the GPU; fails without one).

Two f64 geometries: one contiguous run of 1 GiB (as a matrix: 32768 rows of 4096, lda 4096), and
the headline patch of bench.py (2048 rows of 4096 elements, leading dimension 8192).  Every
figure is one HIP-event pair around enough back-to-back calls to last >= 0.2 s, after warm-up,
on buffers that rotate call by call (as tools/ga_elem_rate.py does); the figures of a geometry
alternate within a round.

  scale_rows, scale_cols   against gaamd_patch_scale  (the same bytes: 2 elements moved per element)
  norm1, norm_inf          against gaamd_patch_dot    in bytes READ per second (1 against 2)

The norms and the dot product end in a stream synchronisation (they return a result): their
figures are the rate of the call, launch and wait included.  The multipliers are 1.0, so the
data do not drift call after call.  The ratios are written down as measured; there is no pass mark.

Then, on one rank, GA_Norm1 and GA_Scale_rows on a 2048 x 4096 C_DBL array against the route a
user has without them: NGA_Get to the host, numpy, NGA_Put back (wall clock).

Writes JSON (default profiles/r12/ga_matrix/rates.json).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import ga_amd  # noqa: E402

PEAK = 8.0e12
DBL = ga_amd.COMEX_ACC_DBL
ELEMS_MOVED = {"scale": 2, "scale_rows": 2, "scale_cols": 2, "dot": 2, "norm1": 1, "norm_inf": 1}
YARDSTICK = {"scale_rows": "scale", "scale_cols": "scale", "norm1": "dot", "norm_inf": "dot"}
NAMES = list(ELEMS_MOVED)


class Geometry:
    def __init__(self, name, rows, cols, ld, sets):
        self.name, self.rows, self.cols, self.ld = name, rows, cols, ld
        self.esz = 8
        self.elems = rows * cols
        self.span = rows * ld * self.esz
        L = ga_amd.lib()
        self.sets = []
        for s in range(sets):
            bufs = [ga_amd.DeviceBuffer(self.span) for _ in range(2)]
            for k, b in enumerate(bufs):
                assert L.gaamd_fill(ctypes.c_void_p(b.ptr), self.span // self.esz, 0, 1000 + 10 * s + k, None) == 0
            self.sets.append(bufs)
        self.ones = ga_amd.DeviceBuffer(max(rows, cols) * self.esz)
        self.ones.upload(np.ones(max(rows, cols)))
        ga_amd.sync()
        self.total_bytes = 2 * sets * self.span

    def free(self):
        for bufs in self.sets:
            for b in bufs:
                b.free()
        self.ones.free()


def make_calls(g):
    L = ga_amd.lib()
    p = ctypes.c_void_p
    if g.ld == g.cols:
        cnt, st = ga_amd.ll_array([g.elems]), ga_amd.ll_array([])
        nd = 1
    else:
        cnt, st = ga_amd.ll_array([g.cols, g.rows]), ga_amd.ll_array([g.ld * g.esz])
        nd = 2
    one = np.array([1.0])
    onep = one.ctypes.data_as(ctypes.c_void_p)
    res = np.zeros(2)
    resp = res.ctypes.data_as(ctypes.c_void_p)
    calls = {
        "scale": lambda a, b: L.gaamd_patch_scale(DBL, onep, p(a.ptr), st, cnt, nd, None),
        "scale_rows": lambda a, b: L.gaamd_scale_rows(DBL, g.rows, g.cols, p(a.ptr), g.ld, p(g.ones.ptr), None),
        "scale_cols": lambda a, b: L.gaamd_scale_cols(DBL, g.rows, g.cols, p(a.ptr), g.ld, p(g.ones.ptr), None),
        "dot": lambda a, b: L.gaamd_patch_dot(DBL, p(a.ptr), st, p(b.ptr), st, cnt, nd, resp, None),
        "norm1": lambda a, b: L.gaamd_patch_norm(DBL, ga_amd.GAAMD_NORM_ONE, p(a.ptr), st, cnt, nd, resp, None),
        "norm_inf": lambda a, b: L.gaamd_patch_norm(DBL, ga_amd.GAAMD_NORM_INF, p(a.ptr), st, cnt, nd, resp, None),
    }
    return calls, (one, res, cnt, st)


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
    gbs = g.elems * g.esz * ELEMS_MOVED[name] * reps_known / s / 1e9
    return gbs, s, reps_known


def ga_level(reps):
    """GA_Norm1 and GA_Scale_rows on one rank against get -> numpy (-> put)"""
    L = ga_amd.lib()
    ia = ga_amd.int_array
    dims = [2048, 4096]
    C_DBL = 1004
    g = L.NGA_Create(C_DBL, 2, ia(dims), b"a", None)
    gv = L.NGA_Create(C_DBL, 1, ia(dims[:1]), b"v", None)
    rng = np.random.default_rng(1)
    lo, hi, ld = ia([0, 0]), ia([d - 1 for d in dims]), ia(dims[1:])
    vlo, vhi = ia([0]), ia([dims[0] - 1])
    x = rng.uniform(1.0, 2.0, dims)
    v = np.ones(dims[0])
    L.NGA_Put(g, lo, hi, x.ctypes.data_as(ctypes.c_void_p), ld)
    L.NGA_Put(gv, vlo, vhi, v.ctypes.data_as(ctypes.c_void_p), ia([1]))
    L.GA_Sync()
    nm = ctypes.c_double(0)
    out = {"array": "2048 x 4096 C_DBL, one rank", "reps": reps}

    def wall(fn):
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return statistics.median(t)

    def host_norm1():
        a = np.empty(dims)
        L.NGA_Get(g, lo, hi, a.ctypes.data_as(ctypes.c_void_p), ld)
        return float(np.abs(a).sum())

    def host_scale_rows():
        a, w = np.empty(dims), np.empty(dims[0])
        L.NGA_Get(g, lo, hi, a.ctypes.data_as(ctypes.c_void_p), ld)
        L.NGA_Get(gv, vlo, vhi, w.ctypes.data_as(ctypes.c_void_p), ia([1]))
        a *= w[:, None]
        L.NGA_Put(g, lo, hi, a.ctypes.data_as(ctypes.c_void_p), ld)
        L.GA_Sync()

    dev_n = wall(lambda: L.GA_Norm1(g, ctypes.byref(nm)))
    host_n = wall(host_norm1)
    assert abs(nm.value - host_norm1()) <= 1e-9 * nm.value
    dev_s = wall(lambda: L.GA_Scale_rows(g, gv))
    host_s = wall(host_scale_rows)
    out["GA_Norm1"] = {"on_device_s": dev_n, "get_numpy_s": host_n, "ratio": round(host_n / dev_n, 1)}
    out["GA_Scale_rows"] = {"on_device_s": dev_s, "get_numpy_put_s": host_s, "ratio": round(host_s / dev_s, 1)}
    L.GA_Destroy(g)
    L.GA_Destroy(gv)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "ga_matrix", "rates.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    args = ap.parse_args()
    L = ga_amd.lib()
    if L.gaamd_device_count() < 1:
        sys.exit("ga_matrix_rate.py needs the MI355X: no HIP device is visible")
    assert L.GA_Initialize() == 0
    out = {"peak_bytes_per_s": PEAK, "min_seconds_per_figure": args.min_seconds, "rounds": args.rounds,
           "elements_moved_per_element": ELEMS_MOVED, "yardstick": YARDSTICK, "geometries": {}}
    try:
        # one geometry at a time: its buffers are freed before the next is allocated
        for gname, rows, cols, ld, sets in (("contiguous_1GiB_f64", 32768, 4096, 4096, 2),
                                            ("headline_2048x4096_ld8192_f64", 2048, 4096, 8192, 4)):
            g = Geometry(gname, rows, cols, ld, sets)
            calls, keep = make_calls(g)
            figs = {n: {"gbs": [], "seconds": [], "reps": None} for n in NAMES}
            for _ in range(args.rounds):        # the figures alternate within a round
                for n in NAMES:
                    gbs, s, reps = measure(g, n, calls[n], args.min_seconds, figs[n]["reps"])
                    figs[n]["reps"] = reps
                    figs[n]["gbs"].append(round(gbs, 1))
                    figs[n]["seconds"].append(round(s, 4))
            for n in NAMES:
                med = statistics.median(figs[n]["gbs"])
                figs[n]["median_gbs"] = med
                figs[n]["share_of_peak"] = round(med * 1e9 / PEAK, 4)
            ratios = {}
            for n, y in YARDSTICK.items():
                per = [round(a / b, 4) for a, b in zip(figs[n]["gbs"], figs[y]["gbs"])]
                ratios[f"{n}_over_{y}"] = {"per_round": per, "median": statistics.median(per)}
                print(f"{gname:32s} {n:10s} {figs[n]['median_gbs']:8.1f} GB/s  {y:5s} {figs[y]['median_gbs']:8.1f} GB/s"
                      f"  ratio per round {per}", flush=True)
            out["geometries"][gname] = {"rows": rows, "cols": cols, "ld_elements": ld, "buffer_sets": sets,
                                        "rotating_bytes": g.total_bytes, "figures": figs, "ratios": ratios}
            g.free()
        out["ga_level"] = ga_level(5)
        print(json.dumps(out["ga_level"]), flush=True)
    finally:
        L.GA_Terminate()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
