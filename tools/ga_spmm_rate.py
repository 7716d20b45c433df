#!/usr/bin/env python3
"""Rates of gaamd_spmm, NGA_Sprs_array_sprsdns_multiply and NGA_Sprs_array_create_from_dense on the
MI355X, one rank (needs the GPU; fails without one).

  kernel   gaamd_spmm, f64 and f32, n = 1, 8, 32, 128, on the two matrices of tools/ga_sprs_rate.py: the
           27-point-stencil-like banded one over a 102^3 grid (1 061 208 rows, 28.5 M entries) and one of
           the same row lengths whose columns are uniformly random.  One HIP-event pair per product after
           warm-up calls, the median of the repeats.  Bytes count val + jdx + the offsets, the rows of B
           the entries name and C ONCE each: what the algorithm needs, not what the gathers fetch.
           GFLOP/s counts one product and one add per entry and column.
           Beside every point, in the same run: n calls of gaamd_spmv with the team the GA layer picks
           (one event pair around the n calls; the copies of the columns out of and into a 2-D array,
           which a caller without gaamd_spmm also pays, are NOT counted), and gaamd_patch_add on 2^26
           elements as the streaming yardstick.
  ga       the banded f64 matrix through the GA layer at n = 32: NGA_Sprs_array_sprsdns_multiply per call
           (wall clock around the call, its syncs, the allocation of g_c and its destruction included)
           beside the bare kernel.
  dense    NGA_Sprs_array_create_from_dense of a 16384 x 16384 f64 array with 1 element in 64 kept (wall
           clock), beside the route without it: NGA_Get of the array -> numpy filter on the host ->
           the add_element loop -> assemble.

Writes JSON (default profiles/r17/ga_spmm/rates.json).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ga_sprs_rate as R  # noqa: E402  (sets the host thread count, puts the repository on the path)

import argparse  # noqa: E402
import ctypes  # noqa: E402
import json  # noqa: E402
import statistics  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

import ga_amd  # noqa: E402

DBL, FLT, C_DBL = R.DBL, R.FLT, R.C_DBL
ia, vp = R.ia, R.vp
WIDTHS = (1, 8, 32, 128)


def kernel_rates(L, ev, rows, offs, jdx_band, add_gbs, warmup, repeats):
    out = {}
    nnz = int(offs[-1])
    rng = np.random.default_rng(1)
    jdx = {"banded": jdx_band, "random": rng.integers(0, rows, nnz, dtype=np.int32)}
    named = {k: int(len(np.unique(v))) for k, v in jdx.items()}
    team = ga_amd.spmv_team(nnz, rows)
    d_offs, d_start = ga_amd.DeviceBuffer(offs.nbytes), ga_amd.DeviceBuffer(8)
    d_offs.upload(offs)
    d_start.upload(np.zeros(1, dtype=np.int64))
    d_jdx = {k: ga_amd.DeviceBuffer(4 * nnz) for k in jdx}
    for k in jdx:
        d_jdx[k].upload(jdx[k])
    nmax = max(WIDTHS)
    for op, name, dt, ftype in ((DBL, "f64", np.float64, 0), (FLT, "f32", np.float32, 1)):
        esz = np.dtype(dt).itemsize
        d_val, d_b, d_c = (ga_amd.DeviceBuffer(esz * k) for k in (nnz, rows * nmax, rows * nmax))
        d_val.upload(rng.uniform(-1, 1, nnz).astype(dt))
        assert L.gaamd_fill(ctypes.c_void_p(d_b.ptr), rows * nmax, ftype, 5, None) == 0
        ga_amd.sync()
        for kind in jdx:
            one = statistics.median(R.timed_ms(L, ev, lambda: ga_amd.spmv(op, rows, 1, d_offs.ptr, d_start.ptr, d_jdx[kind].ptr,
                                                                          d_val.ptr, d_b.ptr, 0, d_c.ptr, team), warmup, repeats))
            for n in WIDTHS:
                ms = R.timed_ms(L, ev, lambda: ga_amd.spmm(op, rows, 1, d_offs.ptr, d_start.ptr, d_jdx[kind].ptr, d_val.ptr,
                                                           d_b.ptr, n, 0, n, d_c.ptr, n), warmup, repeats)
                f = R.fig(ms, nnz * (esz + 4) + 4 * (rows + 1) + (named[kind] + rows) * n * esz)
                f["gflop_per_s"] = round(2.0 * nnz * n / (f["median_ms"] * 1e-3) / 1e9, 1)

                def matvecs():
                    rc = 0
                    for k in range(n):   # column k as a vector: the same traffic as a copied-out column
                        rc |= ga_amd.spmv(op, rows, 1, d_offs.ptr, d_start.ptr, d_jdx[kind].ptr, d_val.ptr,
                                          d_b.ptr + k * rows * esz, 0, d_c.ptr + k * rows * esz, team)
                    return rc

                mv = statistics.median(R.timed_ms(L, ev, matvecs, 1, max(3, repeats // 3)))
                f["n_spmv_calls_ms"] = round(mv, 4)
                f["n_spmv_over_spmm"] = round(mv / f["median_ms"], 2)
                f["over_patch_add_rate"] = round(f["gbytes_per_s"] / add_gbs[name], 3)
                out[f"{name}_{kind}_n{n}"] = f
                print(f"gaamd_spmm {name} {kind:6s} n {n:3d}: {f['median_ms']:8.3f} ms {f['gbytes_per_s']:8.1f} GB/s "
                      f"{f['gflop_per_s']:8.1f} GFLOP/s; {n} spmv {mv:8.3f} ms = {f['n_spmv_over_spmm']:.2f} x; "
                      f"{f['over_patch_add_rate']:.3f} of patch_add", flush=True)
            out[f"{name}_{kind}_one_spmv_ms"] = round(one, 4)
        for b in (d_val, d_b, d_c):
            b.free()
    for b in (d_offs, d_start, *d_jdx.values()):
        b.free()
    out.update(rows=rows, entries=nnz, spmv_team=team, named_rows=named)
    return out


def ga_product(L, rows, offs, jdx, n, kernel_ms):
    rng = np.random.default_rng(2)
    nnz = int(offs[-1])
    val = rng.uniform(-1, 1, nnz)
    ri = np.repeat(np.arange(rows, dtype=np.int32), np.diff(offs))
    s = L.NGA_Sprs_array_create(rows, rows, C_DBL)
    add, base, il, jl = L.NGA_Sprs_array_add_element, val.ctypes.data, ri.tolist(), jdx.tolist()
    for k in range(nnz):
        add(s, il[k], jl[k], base + 8 * k)
    assert L.NGA_Sprs_array_assemble(s) == 1
    gb = L.NGA_Create(C_DBL, 2, ia([rows, n]), b"b", None)
    p, ld = ctypes.c_void_p(), (ctypes.c_int * 1)()
    L.NGA_Access(gb, ia([0, 0]), ia([rows - 1, n - 1]), ctypes.byref(p), ld)
    assert L.gaamd_fill(p, rows * n, 0, 7, None) == 0
    L.NGA_Release_update(gb, ia([0, 0]), ia([rows - 1, n - 1]))
    ga_amd.sync()

    def call():
        g = L.NGA_Sprs_array_sprsdns_multiply(s, gb)
        L.GA_Destroy(g)

    t = R.wall(call, 2, 7)
    L.NGA_Sprs_array_destroy(s)
    L.GA_Destroy(gb)
    med = statistics.median(t)
    return {"rows": rows, "entries": nnz, "n": n, "sprsdns_s": [round(v, 6) for v in t], "sprsdns_median_s": round(med, 6),
            "bare_kernel_ms": kernel_ms, "sprsdns_over_bare_kernel": round(med / (kernel_ms * 1e-3), 2)}


def dense_conversion(L, side):
    a = np.zeros((side, side))
    rng = np.random.default_rng(3)
    for res in range(64):   # row r keeps the columns c with c % 64 == r % 64: 1 in 64, the diagonal among them
        a[res::64, res::64] = rng.uniform(0.5, 1.5, a[res::64, res::64].shape)
    g = L.NGA_Create(C_DBL, 2, ia([side, side]), b"a", None)
    p, ld = ctypes.c_void_p(), (ctypes.c_int * 1)()
    L.NGA_Access(g, ia([0, 0]), ia([side - 1, side - 1]), ctypes.byref(p), ld)
    assert L.gaamd_memcpy(p, vp(a), a.nbytes) == 0
    L.NGA_Release_update(g, ia([0, 0]), ia([side - 1, side - 1]))
    L.GA_Sync()
    t_dev = []
    for _ in range(3):
        t0 = time.perf_counter()
        s = L.NGA_Sprs_array_create_from_dense(g)
        t_dev.append(time.perf_counter() - t0)
        L.NGA_Sprs_array_destroy(s)
    host = np.empty_like(a)
    t0 = time.perf_counter()
    L.NGA_Get(g, ia([0, 0]), ia([side - 1, side - 1]), vp(host), ia([side]))
    t_get = time.perf_counter() - t0
    i, j = np.nonzero((host != 0) | np.eye(side, dtype=bool))
    v = np.ascontiguousarray(host[i, j])
    t_filter = time.perf_counter() - t0 - t_get
    s = L.NGA_Sprs_array_create(side, side, C_DBL)
    add, base, il, jl = L.NGA_Sprs_array_add_element, v.ctypes.data, i.tolist(), j.tolist()
    for k in range(len(il)):
        add(s, il[k], jl[k], base + 8 * k)
    assert L.NGA_Sprs_array_assemble(s) == 1
    t_host = time.perf_counter() - t0
    L.NGA_Sprs_array_destroy(s)
    L.GA_Destroy(g)
    med = statistics.median(t_dev)
    return {"side": side, "kept": int(len(il)), "create_from_dense_s": [round(x, 4) for x in t_dev],
            "create_from_dense_median_s": round(med, 4), "host_route_s": round(t_host, 3), "host_get_s": round(t_get, 3),
            "host_filter_s": round(t_filter, 3), "host_over_create_from_dense": round(t_host / med, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R.ROOT, "profiles", "r17", "ga_spmm", "rates.json"))
    ap.add_argument("--side", type=int, default=102, help="the grid is side^3 rows")
    ap.add_argument("--dense-side", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--no-ga", action="store_true", help="kernels and the yardstick only")
    args = ap.parse_args()
    L = ga_amd.lib()
    if L.gaamd_device_count() < 1:
        sys.exit("ga_spmm_rate.py needs the MI355X: no HIP device is visible")
    assert L.GA_Initialize() == 0
    out = {"bytes": "val + jdx + offsets + the named rows of B + C, each once", "flops": "2 per entry and column",
           "warmup": args.warmup, "repeats": args.repeats}
    try:
        ev = (L.gaamd_event_create(), L.gaamd_event_create())
        out["yardsticks"] = R.yardsticks(L, ev, args.warmup, args.repeats)
        add_gbs = {k: out["yardsticks"][f"patch_add_{k}"]["gbytes_per_s"] for k in ("f64", "f32")}
        rows, offs, jdx = R.banded(args.side)
        out["gaamd_spmm"] = kernel_rates(L, ev, rows, offs, jdx, add_gbs, args.warmup, args.repeats)
        low = [k for k, f in out["gaamd_spmm"].items() if isinstance(f, dict) and "n_spmv_over_spmm" in f
               and int(k.rsplit("_n", 1)[1]) >= 8 and f["n_spmv_over_spmm"] <= 1]
        out["points_at_n_ge_8_not_faster_than_n_spmv"] = low
        if not args.no_ga:
            out["ga_banded_f64_n32_one_rank"] = ga_product(L, rows, offs, jdx, 32, out["gaamd_spmm"]["f64_banded_n32"]["median_ms"])
            print("GA layer:", out["ga_banded_f64_n32_one_rank"], flush=True)
            out["create_from_dense_f64"] = dense_conversion(L, args.dense_side)
            print("create_from_dense:", out["create_from_dense_f64"], flush=True)
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
