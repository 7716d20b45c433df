#!/usr/bin/env python3
"""Rates of gaamd_gemm and GA_Dgemm on the MI355X, one rank (needs the GPU; fails
without one).

  kernel   gaamd_gemm TFLOP/s (2 m n k flops), f64 and f32, NN and TN, at 1024^3, 2048^3
           and 4096^3: one HIP-event pair per call after warm-up calls, the median of the
           repeats.  The f32 figures stand beside the 122 TFLOP/s of an untuned LDS-tiled
           4096^3 GEMM on the f32 matrix-core instruction and its 155 TFLOP/s peak.
  ga       GA_Dgemm at 4096^3 on one rank, wall clock around the call (its two GA_Syncs,
           the panel gets and the stream syncs included), beside the bare kernel.
  host     the route a GA program had without GA_Dgemm, at 2048^3 f64: NGA_Get of A and B
           to host memory, numpy matmul on the host threads, NGA_Put of C -- against
           GA_Dgemm on the same arrays.

Writes JSON (default profiles/r08/ga_gemm/rates.json).
"""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "16")

import argparse  # noqa: E402
import ctypes  # noqa: E402
import json  # noqa: E402
import statistics  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import ga_amd  # noqa: E402

DBL, FLT = ga_amd.COMEX_ACC_DBL, ga_amd.COMEX_ACC_FLT
C_FLOAT, C_DBL = 1003, 1004
F32_UNTUNED_TF, F32_PEAK_TF = 122.0, 155.0
ia = ga_amd.int_array


def kernel_rates(sizes, warmup, repeats):
    L = ga_amd.lib()
    out = {}
    e0, e1 = L.gaamd_event_create(), L.gaamd_event_create()
    for op, name, esz, ftype in ((DBL, "f64", 8, 0), (FLT, "f32", 4, 1)):
        for s in sizes:
            bufs = [ga_amd.DeviceBuffer(s * s * esz) for _ in range(3)]
            for i, b in enumerate(bufs):
                assert L.gaamd_fill(ctypes.c_void_p(b.ptr), s * s, ftype, 77 + i, None) == 0
            ga_amd.sync()
            for ta, tb in (("N", "N"), ("T", "N")):
                ms = []
                for i in range(warmup + repeats):
                    L.gaamd_event_record(e0, None)
                    rc = ga_amd.gemm(op, ta, tb, s, s, s, 1.0, bufs[0].ptr, s, bufs[1].ptr, s, 0.5, bufs[2].ptr, s)
                    assert rc == 0, rc
                    L.gaamd_event_record(e1, None)
                    L.gaamd_event_sync(e1)
                    if i >= warmup:
                        ms.append(L.gaamd_event_elapsed_ms(e0, e1))
                med = statistics.median(ms)
                tf = 2.0 * s ** 3 / (med * 1e-3) / 1e12
                fig = {"ms": [round(x, 4) for x in ms], "median_ms": round(med, 4), "tflops": round(tf, 2)}
                if op == FLT:
                    fig["over_untuned_122"] = round(tf / F32_UNTUNED_TF, 3)
                    fig["over_peak_155"] = round(tf / F32_PEAK_TF, 3)
                out[f"{name}_{ta}{tb}_{s}"] = fig
                print(f"gaamd_gemm {name} {ta}{tb} {s}^3: {med:9.3f} ms  {tf:7.2f} TFLOP/s", flush=True)
            for b in bufs:
                b.free()
    L.gaamd_event_destroy(e0)
    L.gaamd_event_destroy(e1)
    return out


def ga_arrays(L, s):
    """three s x s C_DBL arrays, A and B filled on the device (one rank: the block is the array)"""
    gs = []
    for i, nm in enumerate((b"a", b"b", b"c")):
        g = L.NGA_Create(C_DBL, 2, ia([s, s]), nm, None)
        assert g > 0
        p, ld = ctypes.c_void_p(), (ctypes.c_int * 1)()
        L.NGA_Access(g, ia([0, 0]), ia([s - 1, s - 1]), ctypes.byref(p), ld)
        assert L.gaamd_fill(p, s * s, 0, 900 + i, None) == 0
        L.NGA_Release_update(g, ia([0, 0]), ia([s - 1, s - 1]))
        gs.append(g)
    ga_amd.sync()
    L.GA_Sync()
    return gs


def wall(fn, warmup, repeats):
    t = []
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            t.append(time.perf_counter() - t0)
    return t


def ga_rate(s, warmup, repeats):
    L = ga_amd.lib()
    a, b, c = ga_arrays(L, s)
    t = wall(lambda: L.GA_Dgemm(b"N", b"N", s, s, s, 1.0, a, b, 0.5, c), warmup, repeats)
    for g in (a, b, c):
        L.GA_Destroy(g)
    med = statistics.median(t)
    return {"seconds": [round(x, 5) for x in t], "median_s": round(med, 5),
            "tflops": round(2.0 * s ** 3 / med / 1e12, 2)}


def host_route(s, warmup, repeats):
    L = ga_amd.lib()
    a, b, c = ga_arrays(L, s)
    ha, hb = np.empty((s, s)), np.empty((s, s))
    lo, hi, ld = ia([0, 0]), ia([s - 1, s - 1]), ia([s])
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731

    def host():
        L.GA_Sync()
        L.NGA_Get(a, lo, hi, vp(ha), ld)
        L.NGA_Get(b, lo, hi, vp(hb), ld)
        hc = ha @ hb
        L.NGA_Put(c, lo, hi, vp(hc), ld)
        L.GA_Sync()

    th = wall(host, warmup, repeats)
    tg = wall(lambda: L.GA_Dgemm(b"N", b"N", s, s, s, 1.0, a, b, 0.0, c), warmup, repeats)
    for g in (a, b, c):
        L.GA_Destroy(g)
    mh, mg = statistics.median(th), statistics.median(tg)
    return {"size": s, "host_threads": os.environ.get("OMP_NUM_THREADS"),
            "host_route_s": [round(x, 5) for x in th], "host_route_median_s": round(mh, 5),
            "ga_dgemm_s": [round(x, 5) for x in tg], "ga_dgemm_median_s": round(mg, 5),
            "host_over_ga_dgemm": round(mh / mg, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "ga_gemm", "rates.json"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    L = ga_amd.lib()
    if L.gaamd_device_count() < 1:
        sys.exit("ga_gemm_rate.py needs the MI355X: no HIP device is visible")
    assert L.GA_Initialize() == 0
    out = {"flops": "2 m n k", "warmup": args.warmup, "repeats": args.repeats,
           "f32_reference_tflops": {"untuned_lds_tiled_4096": F32_UNTUNED_TF, "instruction_peak": F32_PEAK_TF}}
    try:
        out["gaamd_gemm"] = kernel_rates((1024, 2048, 4096), args.warmup, args.repeats)
        out["ga_dgemm_4096_one_rank"] = ga_rate(4096, 1, 3)
        k = out["gaamd_gemm"]["f64_NN_4096"]["median_ms"] * 1e-3
        out["ga_dgemm_4096_one_rank"]["over_bare_kernel"] = round(out["ga_dgemm_4096_one_rank"]["median_s"] / k, 3)
        print("GA_Dgemm 4096^3:", out["ga_dgemm_4096_one_rank"], flush=True)
        out["host_route_2048_f64"] = host_route(2048, 1, 3)
        print("host route 2048^3:", out["host_route_2048_f64"], flush=True)
    finally:
        L.GA_Terminate()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
