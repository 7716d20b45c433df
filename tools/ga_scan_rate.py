#!/usr/bin/env python3
"""Rates of gaamd_scan (ADD), gaamd_mask_pack, gaamd_mask_unpack, gaamd_enum and gaamd_scan_tail on
the MI355X, each beside its yardstick in the same process (needs the GPU; fails without one).

f64 values under a C_INT mask with about 1 element in 64 set, at two lengths: n = 2^27 (a 1 GiB
value array) and n = 8 Mi.  Every figure is one HIP-event pair around enough back-to-back calls
to last >= 0.2 s, after warm-up, on buffer sets that rotate call by call (as
tools/ga_matrix_rate.py does); the figures of a length alternate within a round.  A figure is
the bytes the call's kernels read and write, per second:

  scan_add     32 B an element: src and msk read twice (reduce, then scan), dst written
  pack, unpack 8 B an element for the mask, read by the count and by the move, plus 16 B for
               every set element (read and written)
  enum         8 B written                          beside gaamd_patch_fill (8 B)
  scan_tail    12 B read: src and msk once           beside gaamd_patch_dot (16 B read)
  scan_add, pack, unpack                             beside gaamd_patch_add (24 B: c = a + b)

scan_tail and the dot product end in a stream synchronisation (they return a result): their
figures are the rate of the call, launch and wait included.  The ratios are written down as
measured; there is no pass mark.

Then, on one rank, GA_Scan_add and GA_Pack of 8 Mi C_DBL elements against the route a user has
without them: NGA_Get of the arrays to the host, numpy, NGA_Put back (wall clock).

Writes JSON (default profiles/r13/ga_scan/rates.json).
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
DBL, INT = ga_amd.COMEX_ACC_DBL, ga_amd.COMEX_ACC_INT
ADD = ga_amd.GAAMD_SCAN_ADD
YARDSTICK = {"scan_add": "patch_add", "pack": "patch_add", "unpack": "patch_add", "enum": "patch_fill",
             "scan_tail": "patch_dot"}
NAMES = ["patch_add", "scan_add", "pack", "unpack", "patch_fill", "enum", "patch_dot", "scan_tail"]
PERIOD = 1 << 20   # the mask repeats a random pattern of this many elements


class Geometry:
    def __init__(self, name, n, sets):
        self.name, self.n = name, n
        L = ga_amd.lib()
        rng = np.random.default_rng(64)
        pat = (rng.integers(0, 64, PERIOD) == 0).astype(np.int32)
        mask = np.tile(pat, -(-n // PERIOD))[:n]
        self.count = int(mask.sum())
        self.sets = []
        for s in range(sets):
            b = {"src": ga_amd.DeviceBuffer(8 * n), "msk": ga_amd.DeviceBuffer(4 * n), "dst": ga_amd.DeviceBuffer(8 * n),
                 "packed": ga_amd.DeviceBuffer(8 * n)}
            for k, nm in enumerate(("src", "dst", "packed")):
                assert L.gaamd_fill(ctypes.c_void_p(b[nm].ptr), n, 0, 2000 + 10 * s + k, None) == 0
            b["msk"].upload(mask)
            self.sets.append(b)
        ga_amd.sync()
        self.total_bytes = sets * 28 * n
        d = self.count / n
        self.bytes_per_elem = {"patch_add": 24, "scan_add": 32, "pack": 8 + 16 * d, "unpack": 8 + 16 * d, "patch_fill": 8,
                               "enum": 8, "patch_dot": 16, "scan_tail": 12}

    def free(self):
        for b in self.sets:
            for x in b.values():
                x.free()


def make_calls(g):
    L = ga_amd.lib()
    p = ctypes.c_void_p
    cnt, st = ga_amd.ll_array([g.n]), ga_amd.ll_array([])
    one = np.array([1.0])
    onep = one.ctypes.data_as(ctypes.c_void_p)
    res = np.zeros(2)
    resp = res.ctypes.data_as(ctypes.c_void_p)
    flag = ctypes.c_int(0)
    n = g.n
    calls = {
        "patch_add": lambda b: L.gaamd_patch_add(DBL, onep, p(b["src"].ptr), st, onep, p(b["packed"].ptr), st,
                                                 p(b["dst"].ptr), st, cnt, 1, None),
        "scan_add": lambda b: L.gaamd_scan(DBL, ADD, INT, n, p(b["src"].ptr), p(b["msk"].ptr), p(b["dst"].ptr), 0, None,
                                           None),
        "pack": lambda b: L.gaamd_mask_pack(DBL, INT, n, p(b["src"].ptr), p(b["msk"].ptr), p(b["packed"].ptr), None),
        "unpack": lambda b: L.gaamd_mask_unpack(DBL, INT, n, p(b["packed"].ptr), p(b["msk"].ptr), p(b["dst"].ptr), None),
        "patch_fill": lambda b: L.gaamd_patch_fill(DBL, onep, p(b["dst"].ptr), st, cnt, 1, None),
        "enum": lambda b: L.gaamd_enum(DBL, n, 0, onep, onep, p(b["dst"].ptr), None),
        "patch_dot": lambda b: L.gaamd_patch_dot(DBL, p(b["src"].ptr), st, p(b["dst"].ptr), st, cnt, 1, resp, None),
        "scan_tail": lambda b: L.gaamd_scan_tail(DBL, ADD, INT, n, p(b["src"].ptr), p(b["msk"].ptr), ctypes.byref(flag),
                                                 resp, None),
    }
    return calls, (one, res, cnt, st, flag)


def timed(g, fn, reps):
    L = ga_amd.lib()
    e0, e1 = L.gaamd_event_create(), L.gaamd_event_create()
    ga_amd.sync()
    L.gaamd_event_record(e0, None)
    for i in range(reps):
        rc = fn(g.sets[i % len(g.sets)])
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
    gbs = g.n * g.bytes_per_elem[name] * reps_known / s / 1e9
    return gbs, s, reps_known


def ga_level(reps):
    """GA_Scan_add and GA_Pack on one rank against get -> numpy -> put"""
    L = ga_amd.lib()
    ia = ga_amd.int_array
    n = 8 << 20
    C_INT, C_DBL = 1001, 1004
    gs, gd, gm = (L.NGA_Create(t, 1, ia([n]), nm, None) for t, nm in ((C_DBL, b"src"), (C_DBL, b"dst"), (C_INT, b"msk")))
    rng = np.random.default_rng(1)
    lo, hi, ld = ia([0]), ia([n - 1]), ia([1])
    x = rng.integers(-100, 101, n).astype(np.float64)
    m = (rng.integers(0, 64, n) == 0).astype(np.int32)
    m[0] = 1
    L.NGA_Put(gs, lo, hi, x.ctypes.data_as(ctypes.c_void_p), ld)
    L.NGA_Put(gm, lo, hi, m.ctypes.data_as(ctypes.c_void_p), ld)
    L.GA_Sync()
    ic = ctypes.c_int(0)
    out = {"array": "8 Mi C_DBL under a C_INT mask, 1 in 64 set, one rank", "reps": reps}

    def wall(fn):
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return statistics.median(t)

    def fetch():
        a, w = np.empty(n), np.empty(n, dtype=np.int32)
        L.NGA_Get(gs, lo, hi, a.ctypes.data_as(ctypes.c_void_p), ld)
        L.NGA_Get(gm, lo, hi, w.ctypes.data_as(ctypes.c_void_p), ld)
        return a, w != 0

    def host_scan_add():
        a, st = fetch()
        c = np.cumsum(a)
        s = np.maximum.accumulate(np.where(st, np.arange(n), 0))
        r = c - (c[s] - a[s])   # exact here: the data are integer-valued
        L.NGA_Put(gd, lo, hi, r.ctypes.data_as(ctypes.c_void_p), ld)
        L.GA_Sync()
        return r

    def host_pack():
        a, st = fetch()
        r = a[st]
        L.NGA_Put(gd, lo, ia([len(r) - 1]), r.ctypes.data_as(ctypes.c_void_p), ld)
        L.GA_Sync()
        return r

    def got(k):
        r = np.empty(k)
        L.NGA_Get(gd, lo, ia([k - 1]), r.ctypes.data_as(ctypes.c_void_p), ld)
        return r

    dev_s = wall(lambda: L.GA_Scan_add(gs, gd, gm, 0, n - 1, 0))
    on_device = got(n)
    host_s = wall(host_scan_add)
    assert on_device.tobytes() == host_scan_add().tobytes()
    dev_p = wall(lambda: L.GA_Pack(gs, gd, gm, 0, n - 1, ctypes.byref(ic)))
    on_device = got(ic.value)
    host_p = wall(host_pack)
    assert on_device.tobytes() == host_pack().tobytes()
    out["GA_Scan_add"] = {"on_device_s": dev_s, "get_numpy_put_s": host_s, "ratio": round(host_s / dev_s, 1)}
    out["GA_Pack"] = {"on_device_s": dev_p, "get_numpy_put_s": host_p, "ratio": round(host_p / dev_p, 1),
                      "icount": ic.value}
    for g in (gs, gd, gm):
        L.GA_Destroy(g)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "ga_scan", "rates.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    args = ap.parse_args()
    L = ga_amd.lib()
    if L.gaamd_device_count() < 1:
        sys.exit("ga_scan_rate.py needs the MI355X: no HIP device is visible")
    assert L.GA_Initialize() == 0
    out = {"peak_bytes_per_s": PEAK, "min_seconds_per_figure": args.min_seconds, "rounds": args.rounds,
           "yardstick": YARDSTICK, "tile_elements": ga_amd.scan_tile(DBL, INT),
           "aggregate_scan_span_tiles": ga_amd.scan_agg_span(), "geometries": {}}
    try:
        # one length at a time: its buffers are freed before the next is allocated
        for gname, n, sets in (("f64_1GiB_2^27", 1 << 27, 2), ("f64_8Mi", 8 << 20, 4)):
            g = Geometry(gname, n, sets)
            calls, keep = make_calls(g)
            figs = {nm: {"gbs": [], "seconds": [], "reps": None} for nm in NAMES}
            for _ in range(args.rounds):        # the figures alternate within a round
                for nm in NAMES:
                    gbs, s, reps = measure(g, nm, calls[nm], args.min_seconds, figs[nm]["reps"])
                    figs[nm]["reps"] = reps
                    figs[nm]["gbs"].append(round(gbs, 1))
                    figs[nm]["seconds"].append(round(s, 4))
            for nm in NAMES:
                med = statistics.median(figs[nm]["gbs"])
                figs[nm]["median_gbs"] = med
                figs[nm]["share_of_peak"] = round(med * 1e9 / PEAK, 4)
                figs[nm]["bytes_per_element"] = round(g.bytes_per_elem[nm], 4)
                figs[nm]["median_us_per_call"] = round(statistics.median(figs[nm]["seconds"]) / figs[nm]["reps"] * 1e6, 1)
            ratios = {}
            for nm, y in YARDSTICK.items():
                per = [round(a / b, 4) for a, b in zip(figs[nm]["gbs"], figs[y]["gbs"])]
                ratios[f"{nm}_over_{y}"] = {"per_round": per, "median": statistics.median(per)}
                print(f"{gname:16s} {nm:10s} {figs[nm]['median_gbs']:8.1f} GB/s  {y:10s} {figs[y]['median_gbs']:8.1f} GB/s"
                      f"  ratio per round {per}", flush=True)
            out["geometries"][gname] = {"n": n, "set_elements": g.count, "buffer_sets": sets,
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
