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

  --complex  gaamd_gemm_cplx instead (f64 and f32 complex, NN and CN, 8 m n k real flops),
           each beside gaamd_gemm of the same precision and shape in the same run: a complex
           element carries twice the flops per byte of a real one, so the complex TFLOP/s
           should not fall below the real kernel's.  The margin is the spread of the real
           kernel's own medians, taken three times over.  Then GA_Zgemm at 2048^3 on one
           rank against get -> host numpy matmul -> put.

Writes JSON (default profiles/r08/ga_gemm/rates.json; with --complex
profiles/r15/ga_zgemm/rates.json).
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
DCP, CPL = ga_amd.COMEX_ACC_DCP, ga_amd.COMEX_ACC_CPL
C_FLOAT, C_DBL, C_DCPL = 1003, 1004, 1007
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


def timed_ms(L, ev, call, warmup, repeats):
    """one HIP-event pair per call after the warm-up calls: the times of the repeats in ms"""
    ms = []
    for i in range(warmup + repeats):
        L.gaamd_event_record(ev[0], None)
        rc = call()
        assert rc == 0, rc
        L.gaamd_event_record(ev[1], None)
        L.gaamd_event_sync(ev[1])
        if i >= warmup:
            ms.append(L.gaamd_event_elapsed_ms(ev[0], ev[1]))
    return ms


def complex_kernel_rates(sizes, warmup, repeats):
    """gaamd_gemm_cplx NN and CN beside gaamd_gemm NN and TN of the same precision and shape"""
    L = ga_amd.lib()
    out = {}
    ev = (L.gaamd_event_create(), L.gaamd_event_create())
    for cop, rop, name, rsz, ftype in ((DCP, DBL, "f64", 8, 0), (CPL, FLT, "f32", 4, 1)):
        for s in sizes:
            bufs = [ga_amd.DeviceBuffer(2 * s * s * rsz) for _ in range(3)]   # complex; the real runs use half
            for i, b in enumerate(bufs):
                assert L.gaamd_fill(ctypes.c_void_p(b.ptr), 2 * s * s, ftype, 77 + i, None) == 0
            ga_amd.sync()
            pa, pb, pc = (b.ptr for b in bufs)
            for rt, ct in (("N", "N"), ("T", "C")):
                # the yardstick three times over: its medians' spread is the margin
                meds = []
                for _ in range(3):
                    ms = timed_ms(L, ev, lambda: ga_amd.gemm(rop, rt, "N", s, s, s, 1.0, pa, s, pb, s, 0.5, pc, s),
                                  warmup, repeats)
                    meds.append(statistics.median(ms))
                rmed = statistics.median(meds)
                rtf = 2.0 * s ** 3 / (rmed * 1e-3) / 1e12
                spread = (max(meds) - min(meds)) / rmed
                ms = timed_ms(L, ev, lambda: ga_amd.gemm_cplx(cop, ct, "N", s, s, s, 1 + 0.5j, pa, s, pb, s, 0.5 - 1j,
                                                              pc, s), warmup, repeats)
                cmed = statistics.median(ms)
                ctf = 8.0 * s ** 3 / (cmed * 1e-3) / 1e12
                out[f"{name}_{ct}N_{s}"] = {
                    "ms": [round(x, 4) for x in ms], "median_ms": round(cmed, 4), "tflops": round(ctf, 2),
                    "real_kernel": {"trans": rt + "N", "medians_ms": [round(x, 4) for x in meds],
                                    "median_ms": round(rmed, 4), "tflops": round(rtf, 2), "spread": round(spread, 4)},
                    "complex_over_real_tflops": round(ctf / rtf, 3),
                    "short_of_real_beyond_margin": bool(ctf < rtf * (1.0 - spread))}
                print(f"gaamd_gemm_cplx {name} {ct}N {s}^3: {cmed:9.3f} ms  {ctf:7.2f} TFLOP/s   "
                      f"gaamd_gemm {rt}N: {rmed:9.3f} ms  {rtf:7.2f} TFLOP/s (spread {spread:.3f})", flush=True)
            for b in bufs:
                b.free()
    L.gaamd_event_destroy(ev[0])
    L.gaamd_event_destroy(ev[1])
    return out


def ga_arrays(L, s, t=C_DBL):
    """three s x s arrays of type t (C_DBL or C_DCPL), A and B filled on the device (one rank:
    the block is the array)"""
    gs = []
    for i, nm in enumerate((b"a", b"b", b"c")):
        g = L.NGA_Create(t, 2, ia([s, s]), nm, None)
        assert g > 0
        p, ld = ctypes.c_void_p(), (ctypes.c_int * 1)()
        L.NGA_Access(g, ia([0, 0]), ia([s - 1, s - 1]), ctypes.byref(p), ld)
        assert L.gaamd_fill(p, s * s * (2 if t == C_DCPL else 1), 0, 900 + i, None) == 0
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


def host_route_complex(s, warmup, repeats):
    """GA_Zgemm against NGA_Get -> numpy complex128 matmul on the host threads -> NGA_Put"""
    from ga_amd._lib import DoubleComplex
    L = ga_amd.lib()
    a, b, c = ga_arrays(L, s, C_DCPL)
    ha, hb = np.empty((s, s), np.complex128), np.empty((s, s), np.complex128)
    lo, hi, ld = ia([0, 0]), ia([s - 1, s - 1]), ia([s])
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731

    def host():
        L.GA_Sync()
        L.NGA_Get(a, lo, hi, vp(ha), ld)
        L.NGA_Get(b, lo, hi, vp(hb), ld)
        hc = ha @ hb
        L.NGA_Put(c, lo, hi, vp(hc), ld)
        L.GA_Sync()

    one, zero = DoubleComplex(1.0, 0.0), DoubleComplex(0.0, 0.0)
    th = wall(host, warmup, repeats)
    tg = wall(lambda: L.GA_Zgemm(b"N", b"N", s, s, s, one, a, b, zero, c), warmup, repeats)
    for g in (a, b, c):
        L.GA_Destroy(g)
    mh, mg = statistics.median(th), statistics.median(tg)
    return {"size": s, "host_threads": os.environ.get("OMP_NUM_THREADS"),
            "host_route_s": [round(x, 5) for x in th], "host_route_median_s": round(mh, 5),
            "ga_zgemm_s": [round(x, 5) for x in tg], "ga_zgemm_median_s": round(mg, 5),
            "ga_zgemm_tflops": round(8.0 * s ** 3 / mg / 1e12, 2), "host_over_ga_zgemm": round(mh / mg, 2)}


def main_complex(args):
    L = ga_amd.lib()
    out = {"flops": "8 m n k (complex), 2 m n k (real)", "warmup": args.warmup, "repeats": args.repeats,
           "margin": "spread = (max - min) / median of three medians of gaamd_gemm, per shape"}
    try:
        out["gaamd_gemm_cplx"] = complex_kernel_rates((1024, 2048, 4096), args.warmup, args.repeats)
        out["host_route_2048_f64_complex"] = host_route_complex(2048, 1, 3)
        print("host route 2048^3 complex:", out["host_route_2048_f64_complex"], flush=True)
    finally:
        L.GA_Terminate()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--complex", action="store_true", help="gaamd_gemm_cplx / GA_Zgemm beside the real kernel")
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    L = ga_amd.lib()
    if L.gaamd_device_count() < 1:
        sys.exit("ga_gemm_rate.py needs the MI355X: no HIP device is visible")
    assert L.GA_Initialize() == 0
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", *(("r15", "ga_zgemm") if args.complex else ("r08", "ga_gemm")),
                                "rates.json")
    if args.complex:
        write(args.out, main_complex(args))
        return
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
    write(args.out, out)


def write(path, out):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
