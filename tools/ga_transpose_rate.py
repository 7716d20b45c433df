#!/usr/bin/env python3
"""Rates of gaamd_transpose / gaamd_transpose_acc and of GA_Transpose / GA_Symmetrize on the
MI355X, one rank (needs the GPU; fails without one).

  kernel   gaamd_transpose GB/s (bytes read + bytes written) at 4096 x 4096 and 8192 x 2048
           for 4-, 8- and 16-byte elements, and beside it gaamd_strided(GAAMD_OP_COPY) of the
           same 2-D shape and bytes: a copy is the ceiling of a transpose.  The two alternate
           in one run; a window is one HIP-event pair around `calls` back-to-back calls that
           rotate over three source / destination pairs, the figure the median of the windows
           after warm-up windows.
  acc      gaamd_transpose_acc f64 at 4096^2 against gaamd_patch_add (c = 1 * c + 1 * b in
           place) of the same bytes: two reads and one write per element.
  ga       GA_Transpose and GA_Symmetrize at 4096^2 f64 on one rank, wall clock around the
           call (its GA_Syncs, the get of the mirror patch and the stream syncs included),
           beside the bare kernel, and against the only route there was without them:
           NGA_Get to host memory, numpy .T (or 0.5 * (a + a.T)), NGA_Put.

Every part runs in a child process of its own under its own time limit; after a part that
does not end well nothing further is started.  Writes JSON (default
profiles/r09/ga_transpose/rates.json).
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import ga_amd  # noqa: E402

INT, DBL, DCP = ga_amd.COMEX_ACC_INT, ga_amd.COMEX_ACC_DBL, ga_amd.COMEX_ACC_DCP
C_DBL = 1004
SETS = 3
PART_LIMIT_S = {"kernel": 240, "acc": 120, "ga": 240}
ia = ga_amd.int_array


def windows(L, fn, calls, warmup, repeats):
    """milliseconds per call: an event pair around `calls` calls of fn(i), per window"""
    e0, e1 = L.gaamd_event_create(), L.gaamd_event_create()
    ms = []
    for w in range(warmup + repeats):
        L.gaamd_event_record(e0, None)
        for i in range(calls):
            fn(i)
        L.gaamd_event_record(e1, None)
        L.gaamd_event_sync(e1)
        if w >= warmup:
            ms.append(L.gaamd_event_elapsed_ms(e0, e1) / calls)
    L.gaamd_event_destroy(e0)
    L.gaamd_event_destroy(e1)
    return ms


def figure(ms, nbytes):
    med = statistics.median(ms)
    return {"ms_per_call": [round(x, 5) for x in ms], "median_ms": round(med, 5),
            "gbytes_per_s": round(nbytes / (med * 1e-3) / 1e9, 1)}


def filled(L, nbytes, seed):
    b = ga_amd.DeviceBuffer(nbytes)
    assert L.gaamd_fill(ctypes.c_void_p(b.ptr), nbytes // 8, 0, seed, None) == 0
    return b


def part_kernel(args):
    L = ga_amd.lib()
    out = {}
    for rows, cols in ((4096, 4096), (8192, 2048)):
        for op, esz in ((INT, 4), (DBL, 8), (DCP, 16)):
            nbytes = rows * cols * esz
            src = [filled(L, nbytes, 10 + i) for i in range(SETS)]
            dst = [filled(L, nbytes, 20 + i) for i in range(SETS)]
            ga_amd.sync()

            def tr(i):
                rc = ga_amd.transpose(op, rows, cols, src[i % SETS].ptr, cols, dst[i % SETS].ptr, rows)
                assert rc == 0, rc

            def cp(i):
                ga_amd.strided(ga_amd.GAAMD_OP_COPY, None, src[i % SETS].ptr, [cols * esz], dst[i % SETS].ptr,
                               [cols * esz], [cols * esz, rows], 1)

            # alternate the two, so that a drift of the machine meets both
            t_ms, c_ms = [], []
            for _ in range(args.rounds):
                t_ms += windows(L, tr, args.calls, 1, args.repeats)
                c_ms += windows(L, cp, args.calls, 1, args.repeats)
            ft, fc = figure(t_ms, 2 * nbytes), figure(c_ms, 2 * nbytes)
            key = f"{esz}B_{rows}x{cols}"
            out[key] = {"bytes_moved": 2 * nbytes, "transpose": ft, "strided_copy": fc,
                        "transpose_over_copy": round(ft["gbytes_per_s"] / fc["gbytes_per_s"], 3)}
            print(f"{key}: transpose {ft['gbytes_per_s']:8.1f} GB/s  copy {fc['gbytes_per_s']:8.1f} GB/s  "
                  f"ratio {out[key]['transpose_over_copy']}", flush=True)
            for b in src + dst:
                b.free()
    return out


def part_acc(args):
    L = ga_amd.lib()
    n, esz = 4096, 8
    nbytes = n * n * esz
    b = [filled(L, nbytes, 30 + i) for i in range(SETS)]
    c = [filled(L, nbytes, 40 + i) for i in range(SETS)]
    ga_amd.sync()

    def acc(i):
        rc = ga_amd.transpose_acc(DBL, n, n, 0.5, b[i % SETS].ptr, n, c[i % SETS].ptr, n)
        assert rc == 0, rc

    def add(i):   # c = 1 * c + 1 * b in place: the same two reads and one write
        rc = ga_amd.patch_add(DBL, 1.0, c[i % SETS].ptr, [n * esz], 1.0, b[i % SETS].ptr, [n * esz], c[i % SETS].ptr,
                              [n * esz], [n, n])
        assert rc == 0, rc

    a_ms, p_ms = [], []
    for _ in range(args.rounds):
        a_ms += windows(L, acc, args.calls, 1, args.repeats)
        p_ms += windows(L, add, args.calls, 1, args.repeats)
    fa, fp = figure(a_ms, 3 * nbytes), figure(p_ms, 3 * nbytes)
    out = {"bytes_moved": 3 * nbytes, "transpose_acc": fa, "patch_add": fp,
           "transpose_acc_over_patch_add": round(fa["gbytes_per_s"] / fp["gbytes_per_s"], 3)}
    print(f"f64 {n}^2: transpose_acc {fa['gbytes_per_s']} GB/s  patch_add {fp['gbytes_per_s']} GB/s", flush=True)
    return out


def ga_array(L, n, name, seed):
    g = L.NGA_Create(C_DBL, 2, ia([n, n]), name, None)
    assert g > 0
    p, ld = ctypes.c_void_p(), (ctypes.c_int * 1)()
    L.NGA_Access(g, ia([0, 0]), ia([n - 1, n - 1]), ctypes.byref(p), ld)
    assert L.gaamd_fill(p, n * n, 0, seed, None) == 0
    L.NGA_Release_update(g, ia([0, 0]), ia([n - 1, n - 1]))
    ga_amd.sync()
    L.GA_Sync()
    return g, p.value


def wall(fn, warmup, repeats):
    t = []
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            t.append(time.perf_counter() - t0)
    return t


def part_ga(args):
    L = ga_amd.lib()
    n, esz = 4096, 8
    nbytes = n * n * esz
    assert L.GA_Initialize() == 0
    try:
        a, pa = ga_array(L, n, b"a", 50)
        b, pb = ga_array(L, n, b"b", 51)
        lo, hi, ld = ia([0, 0]), ia([n - 1, n - 1]), ia([n])
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        h = np.empty((n, n))

        def host_transpose():
            L.GA_Sync()
            L.NGA_Get(a, lo, hi, vp(h), ld)
            ht = np.ascontiguousarray(h.T)
            L.NGA_Put(b, lo, hi, vp(ht), ld)
            L.GA_Sync()

        def host_symmetrize():
            L.GA_Sync()
            L.NGA_Get(a, lo, hi, vp(h), ld)
            hs = 0.5 * (h + h.T)
            L.NGA_Put(a, lo, hi, vp(hs), ld)
            L.GA_Sync()

        # the bare kernels on the same blocks, for the GA calls to stand beside
        k_tr = statistics.median(windows(L, lambda i: ga_amd.transpose(DBL, n, n, pa, n, pb, n), args.calls, 1,
                                         args.repeats))
        k_acc = statistics.median(windows(L, lambda i: ga_amd.transpose_acc(DBL, n, n, 0.5, pb, n, pa, n), args.calls,
                                          1, args.repeats))
        res = {}
        for name, ga_fn, host_fn, k_ms in (("transpose", lambda: L.GA_Transpose(a, b), host_transpose, k_tr),
                                           ("symmetrize", lambda: L.GA_Symmetrize(a), host_symmetrize, k_acc)):
            tg = wall(ga_fn, 2, 7)
            th = wall(host_fn, 1, 3)
            mg, mh = statistics.median(tg), statistics.median(th)
            res[name] = {"ga_call_s": [round(x, 6) for x in tg], "ga_call_median_s": round(mg, 6),
                         "bare_kernel_ms": round(k_ms, 5), "ga_call_over_bare_kernel": round(mg / (k_ms * 1e-3), 2),
                         "host_route_s": [round(x, 5) for x in th], "host_route_median_s": round(mh, 5),
                         "host_route_over_ga_call": round(mh / mg, 1)}
            print(f"GA {name} {n}^2 f64:", res[name], flush=True)
        res["size"], res["block_bytes"] = n, nbytes
        L.GA_Destroy(a)
        L.GA_Destroy(b)
    finally:
        L.GA_Terminate()
    return res


PARTS = {"kernel": part_kernel, "acc": part_acc, "ga": part_ga}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "ga_transpose", "rates.json"))
    ap.add_argument("--calls", type=int, default=200, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per round, after one warm-up window")
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the two kernels compared")
    ap.add_argument("--part", choices=sorted(PARTS), help="run one part in this process and print its JSON")
    args = ap.parse_args()
    if args.part:
        if ga_amd.lib().gaamd_device_count() < 1:
            sys.exit("ga_transpose_rate.py needs the MI355X: no HIP device is visible")
        if args.part == "ga":      # GA_Initialize / GA_Terminate are the part's own
            res = part_ga(args)
        else:
            assert ga_amd.comex_init() == 0
            try:
                res = PARTS[args.part](args)
            finally:
                ga_amd.comex_finalize()
        print("PART-JSON " + json.dumps(res), flush=True)
        return
    out = {"bytes": "read + written", "calls_per_window": args.calls, "windows": args.repeats * args.rounds,
           "buffer_sets": SETS}
    for part in ("kernel", "acc", "ga"):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--calls", str(args.calls), "--repeats",
               str(args.repeats), "--rounds", str(args.rounds)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=PART_LIMIT_S[part])
        except subprocess.TimeoutExpired:
            sys.exit(f"part {part} did not end within {PART_LIMIT_S[part]} s; nothing further started")
        sys.stdout.write(p.stdout)
        got = [ln for ln in p.stdout.splitlines() if ln.startswith("PART-JSON ")]
        if p.returncode != 0 or len(got) != 1:
            sys.stderr.write(p.stderr[-3000:])
            sys.exit(f"part {part} ended with status {p.returncode}; nothing further started")
        out[part] = json.loads(got[0][len("PART-JSON "):])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
