#!/usr/bin/env python3
"""Rates of gaamd_patch_elem1 / _elem2 / _select on the MI355X, each beside its yardstick
in the same process (needs the GPU; fails without one).

Two geometries, f64 and f32: one contiguous run of 1 GiB, and the headline patch of bench.py
(2048 x 4096 elements, leading dimension 8192).  Every figure is one HIP-event pair around
enough back-to-back calls to last >= 0.2 s, after warm-up, on buffer sets that rotate call by
call (as tools/ga_math_rate.py does); the figures of a geometry alternate within a round.

  elem2 MUL / MAX / DIV  against gaamd_patch_add    (3 elements moved per element)
  elem1 ABS / RECIP      against gaamd_patch_scale  (2)
  select                 against gaamd_patch_dot    in bytes READ per second (1 against 2)

RECIP, DIV, select and dot end in a stream synchronisation (they return a flag or a result):
their figures are the rate of the call, launch and wait included.  The data are uniform in
[-1, 1) (gaamd_fill); in f32 about one element in 2^24 is an exact zero, so a few calls of
RECIP and DIV meet zero divisors -- they are counted, and cost those lanes one store each.
The ratios are written down as measured; there is no pass mark.

Then, on one rank, GA_Elem_multiply and NGA_Select_elem on a 2048 x 4096 C_DBL array against
the route a user has without them: NGA_Get to the host, numpy, NGA_Put back (wall clock).

Writes JSON (default profiles/r10/ga_elem/rates.json).
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
DBL, FLT = ga_amd.COMEX_ACC_DBL, ga_amd.COMEX_ACC_FLT
FILL_TYPE = {DBL: 0, FLT: 1}
ELEMS_MOVED = {"add": 3, "mul": 3, "max": 3, "div": 3, "scale": 2, "abs": 2, "recip": 2, "dot": 2, "select": 1}
YARDSTICK = {"mul": "add", "max": "add", "div": "add", "abs": "scale", "recip": "scale", "select": "dot"}
NAMES = ["add", "mul", "max", "div", "scale", "abs", "recip", "dot", "select"]


class Geometry:
    def __init__(self, name, op, count, stride, sets):
        self.name, self.op, self.count, self.stride = name, op, count, stride
        self.esz = ga_amd.OP_DTYPE[op].itemsize
        self.elems = int(np.prod(count))
        self.span = (count[0] * self.esz) if len(count) == 1 else stride[-1] * count[-1]
        self.sets = []
        L = ga_amd.lib()
        for s in range(sets):
            bufs = [ga_amd.DeviceBuffer(self.span) for _ in range(3)]
            for k, b in enumerate(bufs):
                assert L.gaamd_fill(ctypes.c_void_p(b.ptr), self.span // self.esz, FILL_TYPE[op], 1000 + 10 * s + k,
                                    None) == 0
            self.sets.append(bufs)
        ga_amd.sync()
        self.total_bytes = 3 * sets * self.span

    def refill_c(self):
        """fresh values in [-1, 1) for the in-place operations: what the three-operand figures
        left in c (quotients, and zeros from them) would make RECIP meet zero divisors wholesale"""
        L = ga_amd.lib()
        for s, bufs in enumerate(self.sets):
            assert L.gaamd_fill(ctypes.c_void_p(bufs[2].ptr), self.span // self.esz, FILL_TYPE[self.op],
                                1000 + 10 * s + 2, None) == 0
        ga_amd.sync()

    def free(self):
        for bufs in self.sets:
            for b in bufs:
                b.free()


def make_calls(g):
    L = ga_amd.lib()
    op = g.op
    cnt, st = ga_amd.ll_array(g.count), ga_amd.ll_array(g.stride)
    half, one = np.array([0.5], dtype=ga_amd.OP_DTYPE[op]), np.array([1.0], dtype=ga_amd.OP_DTYPE[op])
    halfp, onep = half.ctypes.data_as(ctypes.c_void_p), one.ctypes.data_as(ctypes.c_void_p)
    res, idx = np.zeros(4), ctypes.c_longlong(0)
    resp = res.ctypes.data_as(ctypes.c_void_p)
    nd = len(g.count)
    p = ctypes.c_void_p
    zero_divisors = {"recip": 0, "div": 0}

    def e2(fn, name=None):
        def call(a, b, c):
            rc = L.gaamd_patch_elem2(op, fn, p(a.ptr), st, p(b.ptr), st, p(c.ptr), st, cnt, nd, None)
            if rc == ga_amd.GAAMD_ZERO_DIVISOR and name:
                zero_divisors[name] += 1
                return 0
            return rc
        return call

    def e1(fn, name=None):
        def call(a, b, c):
            rc = L.gaamd_patch_elem1(op, fn, None, p(c.ptr), st, cnt, nd, None)
            if rc == ga_amd.GAAMD_ZERO_DIVISOR and name:
                zero_divisors[name] += 1
                return 0
            return rc
        return call

    calls = {
        "add": lambda a, b, c: L.gaamd_patch_add(op, halfp, p(a.ptr), st, halfp, p(b.ptr), st, p(c.ptr), st, cnt, nd,
                                                 None),
        "mul": e2(ga_amd.GAAMD_ELEM_MUL), "max": e2(ga_amd.GAAMD_ELEM_MAX), "div": e2(ga_amd.GAAMD_ELEM_DIV, "div"),
        # alpha = 1: the same multiply, and c does not shrink towards zero call after call
        "scale": lambda a, b, c: L.gaamd_patch_scale(op, onep, p(c.ptr), st, cnt, nd, None),
        "abs": e1(ga_amd.GAAMD_ELEM_ABS), "recip": e1(ga_amd.GAAMD_ELEM_RECIP, "recip"),
        "dot": lambda a, b, c: L.gaamd_patch_dot(op, p(a.ptr), st, p(b.ptr), st, cnt, nd, resp, None),
        "select": lambda a, b, c: L.gaamd_patch_select(op, 1, p(a.ptr), st, cnt, nd, resp, None, ctypes.byref(idx),
                                                       None),
    }
    return calls, zero_divisors, (half, one, res, idx, cnt, st)


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
    if ELEMS_MOVED[name] == 2 and name != "dot":
        g.refill_c()
    if reps_known is None:
        timed(g, fn, 2 * len(g.sets))                       # warm-up: every set once or twice
        est = timed(g, fn, 4 * len(g.sets)) / (4 * len(g.sets))
        reps_known = max(8, int(1.25 * min_s / est) + 1)
    s = timed(g, fn, reps_known)
    gbs = g.elems * g.esz * ELEMS_MOVED[name] * reps_known / s / 1e9
    return gbs, s, reps_known


def ga_level(reps):
    """GA_Elem_multiply and NGA_Select_elem on one rank against get -> numpy -> put"""
    L = ga_amd.lib()
    ia = ga_amd.int_array
    dims = [2048, 4096]
    C_DBL = 1004
    g = [L.NGA_Create(C_DBL, 2, ia(dims), nm, None) for nm in (b"a", b"b", b"c")]
    rng = np.random.default_rng(1)
    lo, hi, ld = ia([0, 0]), ia([d - 1 for d in dims]), ia(dims[1:])
    host = [rng.uniform(1.0, 2.0, dims) for _ in range(3)]
    for h, x in zip(g, host):
        L.NGA_Put(h, lo, hi, x.ctypes.data_as(ctypes.c_void_p), ld)
    L.GA_Sync()
    val, idx = np.zeros(1), (ctypes.c_int * 2)()
    out = {"array": "2048 x 4096 C_DBL, one rank", "reps": reps}

    def wall(fn):
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return statistics.median(t)

    def host_multiply():
        a, b = np.empty(dims), np.empty(dims)
        L.NGA_Get(g[0], lo, hi, a.ctypes.data_as(ctypes.c_void_p), ld)
        L.NGA_Get(g[1], lo, hi, b.ctypes.data_as(ctypes.c_void_p), ld)
        c = a * b
        L.NGA_Put(g[2], lo, hi, c.ctypes.data_as(ctypes.c_void_p), ld)
        L.GA_Sync()

    def host_select():
        a = np.empty(dims)
        L.NGA_Get(g[0], lo, hi, a.ctypes.data_as(ctypes.c_void_p), ld)
        return np.unravel_index(int(np.argmax(a)), dims)

    dev_mul = wall(lambda: L.GA_Elem_multiply(g[0], g[1], g[2]))
    host_mul = wall(host_multiply)
    dev_sel = wall(lambda: L.NGA_Select_elem(g[0], b"max", val.ctypes.data_as(ctypes.c_void_p), idx))
    host_sel = wall(host_select)
    assert list(idx) == [int(v) for v in host_select()]
    out["GA_Elem_multiply"] = {"on_device_s": dev_mul, "get_numpy_put_s": host_mul, "ratio": round(host_mul / dev_mul, 1)}
    out["NGA_Select_elem"] = {"on_device_s": dev_sel, "get_numpy_s": host_sel, "ratio": round(host_sel / dev_sel, 1)}
    for h in g:
        L.GA_Destroy(h)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "ga_elem", "rates.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    args = ap.parse_args()
    L = ga_amd.lib()
    if L.gaamd_device_count() < 1:
        sys.exit("ga_elem_rate.py needs the MI355X: no HIP device is visible")
    assert L.GA_Initialize() == 0
    out = {"peak_bytes_per_s": PEAK, "min_seconds_per_figure": args.min_seconds, "rounds": args.rounds,
           "elements_moved_per_element": ELEMS_MOVED, "yardstick": YARDSTICK, "geometries": {}}
    try:
        # one geometry at a time: its buffers are freed before the next is allocated
        for op, tname in ((DBL, "f64"), (FLT, "f32")):
            esz = ga_amd.OP_DTYPE[op].itemsize
            for gname, count, stride, sets in (
                    (f"contiguous_1GiB_{tname}", [(1 << 30) // esz], [], 2),
                    (f"headline_2048x4096_ld8192_{tname}", [2048, 4096], [8192 * esz], 4)):
                g = Geometry(gname, op, count, stride, sets)
                calls, zero_divisors, keep = make_calls(g)
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
                    print(f"{gname:34s} {n:6s} {figs[n]['median_gbs']:8.1f} GB/s  {y:5s} {figs[y]['median_gbs']:8.1f} GB/s"
                          f"  ratio per round {per}", flush=True)
                out["geometries"][gname] = {"count_elements": count, "stride_bytes": stride, "buffer_sets": sets,
                                            "rotating_bytes": g.total_bytes, "figures": figs, "ratios": ratios,
                                            "calls_that_met_a_zero_divisor": zero_divisors}
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
