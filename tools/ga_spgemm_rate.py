#!/usr/bin/env python3
"""Rates of gaamd_spgemm_count / gaamd_spgemm_fill and NGA_Sprs_array_matmat_multiply on the MI355X, one rank
(needs the GPU; fails without one).  Every matrix is SQUARED: C = A A.

  kernel   f64 and f32 on the two matrices of tools/ga_sprs_rate.py -- the 27-point-stencil-like banded one over
           a 102^3 grid (1 061 208 rows, 28.5 M entries) and one of the same row lengths whose columns are
           uniformly random -- and on a banded 16384 x 16384 one (27 diagonals).  One HIP-event pair per kernel
           after warm-up calls, the median of the repeats: count and fill apart (the prefix sums between them
           are formed on the host and not timed here), products/s over count + fill, and the distinct / product
           ratio (entries of C over the sum of U).
  ga       NGA_Sprs_array_matmat_multiply(s, s) per call, f64 (wall clock around the call, its syncs, the
           flattening and publishing of B, the offsets through the host and the destruction of C included),
           beside the bare kernels.
  dense    at 16384 x 16384, the route without the call inside the library: create_from_sparse(B) ->
           sprsdns_multiply -> create_from_dense (wall clock, the two dense arrays destroyed).
  host     the route outside the library: download the blocks -> scipy.sparse CSR product on the host (a numpy
           product, at the small size only, where scipy cannot be imported) -> the add_element loop -> assemble.
           At sizes above --host-entries entries of C only the download and the host product are run; the rest is
           EXTRAPOLATED from the cost per entry measured at the small size in the same run, and labelled so.

Writes JSON (default profiles/r19/ga_spgemm/rates.json).
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


def band(n, half=13):
    """offsets and columns of the n x n matrix with the diagonals -half .. half"""
    cols = np.arange(n, dtype=np.int64)[:, None] + np.arange(-half, half + 1, dtype=np.int64)[None, :]
    ok = (cols >= 0) & (cols < n)
    offs = np.zeros(n + 1, dtype=np.int32)
    offs[1:] = np.cumsum(ok.sum(axis=1))
    return n, offs, cols[ok].astype(np.int32)


def up(a):
    b = ga_amd.DeviceBuffer(max(16, a.nbytes))
    b.upload(np.ascontiguousarray(a))
    return b


def kernel_rates(L, ev, rows, offs, jdx, warmup, repeats):
    """A A at kernel level, one column block: {f64, f32: figures}"""
    out = {}
    nnz = int(offs[-1])
    rng = np.random.default_rng(1)
    d_offs, d_start, d_roffs, d_jdx = up(offs), up(np.zeros(1, dtype=np.int64)), up(offs.astype(np.int64)), up(jdx)
    d_counts, d_bound = ga_amd.DeviceBuffer(4 * rows), ga_amd.DeviceBuffer(8 * rows)
    count = lambda: ga_amd.spgemm_count(rows, 1, d_offs.ptr, d_start.ptr, d_jdx.ptr, 0, rows, d_roffs.ptr, d_jdx.ptr,  # noqa: E731
                                        rows, 1, d_counts.ptr, d_bound.ptr)
    ms_count = R.timed_ms(L, ev, count, warmup, repeats)
    counts, bound = d_counts.download(np.int32, rows), d_bound.download(np.int64, rows)
    coffs = np.zeros(rows + 1, dtype=np.int64)
    coffs[1:] = np.cumsum(counts)
    entries, products = int(coffs[-1]), int(bound.sum())
    assert entries < 2 ** 31
    d_coffs = up(coffs.astype(np.int32))
    d_cjdx = ga_amd.DeviceBuffer(max(16, 4 * entries))
    for op, name, dt in ((DBL, "f64", np.float64), (FLT, "f32", np.float32)):
        esz = np.dtype(dt).itemsize
        d_val, d_cval = up(rng.uniform(-1, 1, nnz).astype(dt)), ga_amd.DeviceBuffer(max(16, esz * entries))
        fill = lambda: ga_amd.spgemm_fill(op, rows, 1, d_offs.ptr, d_start.ptr, d_jdx.ptr, d_val.ptr, 0, rows, d_roffs.ptr,  # noqa: E731
                                          d_jdx.ptr, d_val.ptr, rows, 1, d_coffs.ptr, d_start.ptr, d_cjdx.ptr, d_cval.ptr)
        ms_fill = R.timed_ms(L, ev, fill, warmup, repeats)
        c, f = statistics.median(ms_count), statistics.median(ms_fill)
        out[name] = {"fill_ms": [round(x, 3) for x in ms_fill], "fill_median_ms": round(f, 3),
                     "products_per_s": round(products / ((c + f) * 1e-3), 0)}
        print(f"  {name}: count {c:9.3f} ms, fill {f:9.3f} ms, {out[name]['products_per_s'] / 1e9:7.3f} G products/s", flush=True)
        d_val.free()
        d_cval.free()
    for b in (d_offs, d_start, d_roffs, d_jdx, d_counts, d_bound, d_coffs, d_cjdx):
        b.free()
    out.update(count_note="the count kernel reads no values: timed once per matrix, used for both types",
               count_ms=[round(x, 3) for x in ms_count], count_median_ms=round(statistics.median(ms_count), 3),
               rows=rows, entries_of_a=nnz, products=products, entries_of_c=entries,
               distinct_per_product=round(entries / max(products, 1), 4),
               rows_on_the_fallback=int((bound > ga_amd.spgemm_lds_cap()).sum()))
    return out


def assemble(L, rows, offs, jdx, val):
    ri = np.repeat(np.arange(rows, dtype=np.int32), np.diff(offs))
    s = L.NGA_Sprs_array_create(rows, rows, C_DBL)
    add, base, il, jl = L.NGA_Sprs_array_add_element, val.ctypes.data, ri.tolist(), jdx.tolist()
    for k in range(len(il)):
        add(s, il[k], jl[k], base + 8 * k)
    assert L.NGA_Sprs_array_assemble(s) == 1
    return s


def download(L, s, rows):
    """(offs, jdx, val) of the one column block of a one-rank f64 array"""
    idx, jdx, val = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    L.NGA_Sprs_array_access_col_block(s, 0, ctypes.byref(idx), ctypes.byref(jdx), ctypes.byref(val))
    offs = np.empty(rows + 1, dtype=np.int32)
    assert L.gaamd_memcpy(vp(offs), idx, offs.nbytes) == 0
    j, v = np.empty(int(offs[-1]), dtype=np.int32), np.empty(int(offs[-1]))
    assert L.gaamd_memcpy(vp(j), jdx, j.nbytes) == 0 and L.gaamd_memcpy(vp(v), val, v.nbytes) == 0
    return offs, j, v


def numpy_product(rows, offs, jdx, val):
    """A A on the host without scipy: per row the products in order, summed per column (np.add.at keeps the order)"""
    oo, jj, vv = [0], [], []
    for r in range(rows):
        ks = np.arange(offs[r], offs[r + 1])
        if len(ks):
            span = np.concatenate([np.arange(offs[k], offs[k + 1]) for k in jdx[ks]])
            a = np.repeat(val[ks], offs[jdx[ks] + 1] - offs[jdx[ks]])
            cols, inv = np.unique(jdx[span], return_inverse=True)
            acc = np.zeros(len(cols))
            np.add.at(acc, inv, a * val[span])
            jj.append(cols.astype(np.int32))
            vv.append(acc)
            oo.append(oo[-1] + len(cols))
        else:
            oo.append(oo[-1])
    return np.array(oo, dtype=np.int32), np.concatenate(jj), np.concatenate(vv)


def ga_rates(L, rows, offs, jdx, kernel, dense, host_entries, numpy_rows, add_us_per_entry=None):
    out = {"rows": rows}
    val = np.random.default_rng(2).uniform(-1, 1, int(offs[-1]))
    s = assemble(L, rows, offs, jdx, val)

    def call():
        c = L.NGA_Sprs_array_matmat_multiply(s, s)
        assert c > 0
        L.NGA_Sprs_array_destroy(c)

    t = R.wall(call, 1, 5)
    med = statistics.median(t)
    bare = (kernel["count_median_ms"] + kernel["f64"]["fill_median_ms"]) * 1e-3
    out.update(matmat_s=[round(x, 5) for x in t], matmat_median_s=round(med, 5), bare_kernels_s=round(bare, 5),
               matmat_over_bare_kernels=round(med / bare, 2))
    if dense:
        def route():
            g_b = L.NGA_Sprs_array_create_from_sparse(s)
            g_c = L.NGA_Sprs_array_sprsdns_multiply(s, g_b)
            c = L.NGA_Sprs_array_create_from_dense(g_c)
            L.NGA_Sprs_array_destroy(c)
            L.GA_Destroy(g_c)
            L.GA_Destroy(g_b)

        td = statistics.median(R.wall(route, 1, 3))
        out.update(dense_route_median_s=round(td, 4), dense_route_over_matmat=round(td / med, 1))
    try:
        import scipy.sparse as sp
    except ImportError:
        sp = None
    if sp is None and rows > numpy_rows:
        out.update(host_route_s=None, host_route_note="scipy.sparse is not importable and the numpy product is run at the small size only")
    else:
        t0 = time.perf_counter()
        o, j, v = download(L, s, rows)
        t_down = time.perf_counter() - t0
        if sp is not None:
            c = sp.csr_matrix((v, j, o), shape=(rows, rows))
            c = c @ c
            c.sort_indices()
            c_offs, c_jdx, c_val, how = c.indptr.astype(np.int32), c.indices.astype(np.int32), np.ascontiguousarray(c.data), "scipy.sparse"
        else:
            c_offs, c_jdx, c_val = numpy_product(rows, o, j, v)
            how = "numpy"
        t_prod = time.perf_counter() - t0 - t_down
        out.update(host_product=how, host_download_s=round(t_down, 4), host_product_s=round(t_prod, 4), host_entries_of_c=int(len(c_jdx)))
        if len(c_jdx) <= host_entries:
            t1 = time.perf_counter()
            s_c = assemble(L, rows, c_offs, c_jdx, c_val)
            t_add = time.perf_counter() - t1
            L.NGA_Sprs_array_destroy(s_c)
            t_host = t_down + t_prod + t_add
            out.update(host_add_and_assemble_s=round(t_add, 4), host_add_and_assemble_us_per_entry=round(t_add / len(c_jdx) * 1e6, 4),
                       host_route_s=round(t_host, 3), host_route_over_matmat=round(t_host / med, 1))
        else:   # not run: the per-entry cost measured at the small size in this run, times the entries
            est = t_down + t_prod + len(c_jdx) * add_us_per_entry * 1e-6 if add_us_per_entry else None
            out.update(host_route_s=None, host_download_and_product_over_matmat=round((t_down + t_prod) / med, 1),
                       host_route_extrapolated_s=None if est is None else round(est, 1),
                       host_route_extrapolated_over_matmat=None if est is None else round(est / med, 0),
                       host_route_note="add_element and assemble NOT RUN at this size; the extrapolated figure adds the entries of C "
                                       "times the cost per entry of that loop and the assembly measured at the small size in this run")
    L.NGA_Sprs_array_destroy(s)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R.ROOT, "profiles", "r19", "ga_spgemm", "rates.json"))
    ap.add_argument("--side", type=int, default=102, help="the grid is side^3 rows")
    ap.add_argument("--small", type=int, default=16384, help="rows of the small banded matrix")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-entries", type=int, default=4000000, help="the most entries of C the host route adds one by one")
    ap.add_argument("--no-ga", action="store_true", help="kernels only")
    ap.add_argument("--no-large-ga", action="store_true", help="the GA layer at the small size only")
    args = ap.parse_args()
    L = ga_amd.lib()
    if L.gaamd_device_count() < 1:
        sys.exit("ga_spgemm_rate.py needs the MI355X: no HIP device is visible")
    assert L.GA_Initialize() == 0
    out = {"products": "the sum over the rows of U, one multiply and one add each", "warmup": args.warmup,
           "repeats": args.repeats, "lds_cap": ga_amd.spgemm_lds_cap()}
    try:
        ev = (L.gaamd_event_create(), L.gaamd_event_create())
        rows, offs, jdx = R.banded(args.side)
        # uniformly random columns, ascending within a row as the assembly leaves them
        rowid = np.repeat(np.arange(rows, dtype=np.int64), np.diff(offs))
        key = np.sort(rowid * rows + np.random.default_rng(1).integers(0, rows, int(offs[-1])))
        small = band(args.small)
        cases = (("banded", rows, offs, jdx), ("random", rows, offs, (key % rows).astype(np.int32)), ("band_small",) + small)
        out["kernels"] = {}
        for name, n, o, j in cases:
            print(f"{name}: {n} rows, {int(o[-1])} entries", flush=True)
            out["kernels"][name] = kernel_rates(L, ev, n, o, j, args.warmup, args.repeats)
        if not args.no_ga:
            out["ga_band_small_f64"] = ga_rates(L, small[0], small[1], small[2], out["kernels"]["band_small"], True, args.host_entries,
                                                small[0])
            print("GA layer, small:", out["ga_band_small_f64"], flush=True)
            if not args.no_large_ga:
                out["ga_banded_f64"] = ga_rates(L, rows, offs, jdx, out["kernels"]["banded"], False, args.host_entries, small[0],
                                                out["ga_band_small_f64"].get("host_add_and_assemble_us_per_entry"))
                print("GA layer, banded:", out["ga_banded_f64"], flush=True)
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
