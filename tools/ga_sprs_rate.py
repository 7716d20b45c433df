#!/usr/bin/env python3
"""Rates of gaamd_spmv and NGA_Sprs_array_matvec_multiply on the MI355X, one rank (needs the GPU;
fails without one).

  kernel   gaamd_spmv, f64 and f32, on two matrices of the same row lengths: a 27-point-stencil-like
           banded one over a 102^3 grid (1 061 208 rows, about 2^20; good locality of x) and one whose
           columns are uniformly random (the worst locality).  One HIP-event pair per call after
           warm-up calls, the median of the repeats.  Bytes moved count val + jdx + the offsets + y + x
           ONCE each: what the algorithm needs, not what the gather fetches.  The library's team
           (gaamd_spmv_team) and its neighbours are timed side by side.
  yardsticks, in the same run: gaamd_patch_dot (a streaming read reduction over two arrays) and
           gaamd_patch_add (two reads, one write), 2^26 elements each.
  ga       the banded f64 matrix through the GA layer: the add_element loop and
           NGA_Sprs_array_assemble (wall clock), NGA_Sprs_array_matvec_multiply per call (wall clock
           around the call, its two syncs included) beside the bare kernel, and the route a GA program
           had without it: NGA_Get of x -> numpy CSR product on the host -> NGA_Put of y.

Writes JSON (default profiles/r16/ga_sprs/rates.json).
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
C_DBL = 1004
ia = ga_amd.int_array


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def banded(side):
    """offsets (int32, n + 1) and columns (int32) of the 27-point stencil over a side^3 grid, taken on the
    linear index: row r holds r + dz * side^2 + dy * side + dx for d in {-1, 0, 1}^3 where that lies in
    [0, n); columns ascending within a row"""
    n = side ** 3
    d = np.array([dz * side * side + dy * side + dx for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)],
                 dtype=np.int64)
    cols = np.arange(n, dtype=np.int64)[:, None] + np.sort(d)[None, :]
    ok = (cols >= 0) & (cols < n)
    offs = np.zeros(n + 1, dtype=np.int32)
    offs[1:] = np.cumsum(ok.sum(axis=1))
    return n, offs, cols[ok].astype(np.int32)


def timed_ms(L, ev, call, warmup, repeats):
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


def fig(ms, nbytes):
    med = statistics.median(ms)
    return {"ms": [round(x, 4) for x in ms], "median_ms": round(med, 4), "bytes": int(nbytes),
            "gbytes_per_s": round(nbytes / (med * 1e-3) / 1e9, 1)}


def kernel_rates(L, ev, n, offs, jdx_band, warmup, repeats):
    out = {}
    nnz = int(offs[-1])
    rng = np.random.default_rng(1)
    jdx_rand = rng.integers(0, n, nnz, dtype=np.int32)
    start = np.zeros(1, dtype=np.int64)
    team = ga_amd.spmv_team(nnz, n)
    d_offs, d_start = ga_amd.DeviceBuffer(offs.nbytes), ga_amd.DeviceBuffer(8)
    d_offs.upload(offs)
    d_start.upload(start)
    d_jdx = {"banded": ga_amd.DeviceBuffer(4 * nnz), "random": ga_amd.DeviceBuffer(4 * nnz)}
    d_jdx["banded"].upload(jdx_band)
    d_jdx["random"].upload(jdx_rand)
    for op, name, dt in ((DBL, "f64", np.float64), (FLT, "f32", np.float32)):
        esz = np.dtype(dt).itemsize
        d_val, d_x, d_y = ga_amd.DeviceBuffer(esz * nnz), ga_amd.DeviceBuffer(esz * n), ga_amd.DeviceBuffer(esz * n)
        d_val.upload(rng.uniform(-1, 1, nnz).astype(dt))
        d_x.upload(rng.uniform(-1, 1, n).astype(dt))
        nbytes = nnz * (esz + 4) + 4 * (n + 1) + 2 * esz * n
        for kind in ("banded", "random"):
            for w in sorted({team, max(1, team // 2), max(1, team // 4), min(64, team * 2), min(64, team * 4)}):
                ms = timed_ms(L, ev, lambda: ga_amd.spmv(op, n, 1, d_offs.ptr, d_start.ptr, d_jdx[kind].ptr, d_val.ptr,
                                                         d_x.ptr, 0, d_y.ptr, w), warmup, repeats)
                f = fig(ms, nbytes)
                f["team"], f["library_team"] = w, w == team
                out[f"{name}_{kind}_team{w}"] = f
                print(f"gaamd_spmv {name} {kind:6s} team {w:2d}: {f['median_ms']:8.3f} ms  {f['gbytes_per_s']:8.1f} GB/s"
                      f"{'  <- gaamd_spmv_team' if w == team else ''}", flush=True)
        for b in (d_val, d_x, d_y):
            b.free()
    for b in (d_offs, d_start, *d_jdx.values()):
        b.free()
    out["rows"], out["entries"], out["library_team"] = n, nnz, team
    return out


def yardsticks(L, ev, warmup, repeats):
    out = {}
    n = 1 << 26
    for op, name, esz, ftype in ((DBL, "f64", 8, 0), (FLT, "f32", 4, 1)):
        bufs = [ga_amd.DeviceBuffer(n * esz) for _ in range(3)]
        for i, b in enumerate(bufs):
            assert L.gaamd_fill(ctypes.c_void_p(b.ptr), n, ftype, 11 + i, None) == 0
        ga_amd.sync()
        cnt = ga_amd.ll_array([n])
        res = np.zeros(2)
        ms = timed_ms(L, ev, lambda: L.gaamd_patch_dot(op, ctypes.c_void_p(bufs[0].ptr), None, ctypes.c_void_p(bufs[1].ptr),
                                                       None, cnt, 1, vp(res), None), warmup, repeats)
        out[f"patch_dot_{name}"] = fig(ms, 2 * n * esz)
        al, be = ga_amd.scale_buffer(op, 0.5)[0], ga_amd.scale_buffer(op, 0.25)[0]
        ms = timed_ms(L, ev, lambda: L.gaamd_patch_add(op, vp(al), ctypes.c_void_p(bufs[0].ptr), None, vp(be),
                                                       ctypes.c_void_p(bufs[1].ptr), None, ctypes.c_void_p(bufs[2].ptr), None,
                                                       cnt, 1, None), warmup, repeats)
        out[f"patch_add_{name}"] = fig(ms, 3 * n * esz)
        for k in (f"patch_dot_{name}", f"patch_add_{name}"):
            print(f"{k}: {out[k]['median_ms']:8.3f} ms  {out[k]['gbytes_per_s']:8.1f} GB/s", flush=True)
        for b in bufs:
            b.free()
    return out


def wall(fn, warmup, repeats):
    t = []
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            t.append(time.perf_counter() - t0)
    return t


def ga_route(L, n, offs, jdx, kernel_ms):
    rng = np.random.default_rng(2)
    nnz = int(offs[-1])
    val = rng.uniform(-1, 1, nnz)
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(offs))
    s = L.NGA_Sprs_array_create(n, n, C_DBL)
    add = L.NGA_Sprs_array_add_element
    base, il, jl = val.ctypes.data, rows.tolist(), jdx.tolist()
    t0 = time.perf_counter()
    for k in range(nnz):
        add(s, il[k], jl[k], base + 8 * k)
    t_add = time.perf_counter() - t0
    t0 = time.perf_counter()
    assert L.NGA_Sprs_array_assemble(s) == 1
    t_asm = time.perf_counter() - t0
    gx, gy = (L.NGA_Create(C_DBL, 1, ia([n]), nm, None) for nm in (b"x", b"y"))
    x = rng.uniform(-1, 1, n)
    lo, hi, ld = ia([0]), ia([n - 1]), ia([])
    L.NGA_Put(gx, lo, hi, vp(x), ld)
    L.GA_Sync()
    tm = wall(lambda: L.NGA_Sprs_array_matvec_multiply(s, gx, gy), 2, 7)
    y_dev = np.empty(n)
    L.NGA_Get(gy, lo, hi, vp(y_dev), ld)
    hx, first = np.empty(n), offs[:-1].astype(np.int64)
    assert (np.diff(offs) > 0).all()

    def host():
        L.GA_Sync()
        L.NGA_Get(gx, lo, hi, vp(hx), ld)
        hy = np.add.reduceat(val * hx[jdx], first)
        L.NGA_Put(gy, lo, hi, vp(hy), ld)
        L.GA_Sync()
        return hy

    th = wall(host, 1, 3)
    hy = host()
    err = float(np.abs(hy - y_dev).max())
    L.NGA_Sprs_array_destroy(s)
    L.GA_Destroy(gx)
    L.GA_Destroy(gy)
    mm, mh = statistics.median(tm), statistics.median(th)
    return {"rows": n, "entries": nnz, "add_element_loop_s": round(t_add, 3), "assemble_s": round(t_asm, 3),
            "matvec_s": [round(v, 6) for v in tm], "matvec_median_s": round(mm, 6),
            "bare_kernel_ms": kernel_ms, "matvec_over_bare_kernel": round(mm / (kernel_ms * 1e-3), 2),
            "host_route_s": [round(v, 5) for v in th], "host_route_median_s": round(mh, 5),
            "host_threads": os.environ.get("OMP_NUM_THREADS"), "host_over_matvec": round(mh / mm, 1),
            "max_abs_difference_host_vs_device": err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "ga_sprs", "rates.json"))
    ap.add_argument("--side", type=int, default=102, help="the grid is side^3 rows")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--no-ga", action="store_true", help="kernels and yardsticks only")
    args = ap.parse_args()
    L = ga_amd.lib()
    if L.gaamd_device_count() < 1:
        sys.exit("ga_sprs_rate.py needs the MI355X: no HIP device is visible")
    assert L.GA_Initialize() == 0
    out = {"bytes": "val + jdx + offsets + y + x, each once", "warmup": args.warmup, "repeats": args.repeats}
    try:
        ev = (L.gaamd_event_create(), L.gaamd_event_create())
        n, offs, jdx = banded(args.side)
        out["gaamd_spmv"] = kernel_rates(L, ev, n, offs, jdx, args.warmup, args.repeats)
        out["yardsticks"] = yardsticks(L, ev, args.warmup, args.repeats)
        team = out["gaamd_spmv"]["library_team"]
        for name in ("f64", "f32"):
            for kind in ("banded", "random"):
                r = out["gaamd_spmv"][f"{name}_{kind}_team{team}"]["gbytes_per_s"]
                out[f"{name}_{kind}_over_patch_dot"] = round(r / out["yardsticks"][f"patch_dot_{name}"]["gbytes_per_s"], 3)
                out[f"{name}_{kind}_over_patch_add"] = round(r / out["yardsticks"][f"patch_add_{name}"]["gbytes_per_s"], 3)
        if not args.no_ga:
            out["ga_banded_f64_one_rank"] = ga_route(L, n, offs, jdx, out["gaamd_spmv"][f"f64_banded_team{team}"]["median_ms"])
            print("GA layer:", out["ga_banded_f64_one_rank"], flush=True)
        L.gaamd_event_destroy(ev[0])
        L.gaamd_event_destroy(ev[1])
    finally:
        L.GA_Terminate()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
