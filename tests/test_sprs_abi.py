"""CPU: the sparse-array names are exported where they belong, gaamd_ga_sprs_range and gaamd_spmv_team
follow their rules, the kernel entry points return their codes before any launch, the numpy
restatement used by the GPU tests (tests/test_gpu_sprs.py) agrees with plain Python loops written
from the contract in include/ga_amd.h and include/ga.h, and the host part of the assembly
(ga_amd/csrc/sprs_build.hpp), built as a stand-alone program under the address and
undefined-behaviour sanitizers, produces the restatement's block CSR.  No device is needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ga_amd
import test_gpu_sprs as S
from ga_amd._lib import GA_LIB_PATH, LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = S.K
OPS, DT, UNS, REAL = S.OPS, S.DT, S.UNS, S.REAL
NEW_GA = ["NGA_Sprs_array_" + n for n in (
    "create", "add_element", "assemble", "destroy", "duplicate", "row_distribution", "column_distribution",
    "col_block_list", "access_col_block", "matvec_multiply", "get_diag", "shift_diag", "scale", "diag_left_multiply",
    "diag_right_multiply")] + ["gaamd_ga_sprs_range", "gaamd_ga_sprs_route_counts"]
NEW_CORE = ["gaamd_spmv", "gaamd_spmv_team", "gaamd_sprs_diag", "gaamd_sprs_scale_left", "gaamd_sprs_scale_right"]
opid = dict(ids=lambda o: ga_amd.OP_NAME[o])


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3}


def test_exported_names():
    core, ga = exported(LIB_PATH), exported(GA_LIB_PATH)
    assert not [n for n in NEW_GA if n not in ga]
    assert not [n for n in NEW_GA if n in core]
    assert not [n for n in core if n.startswith(("GA_", "NGA_", "gaamd_ga_"))]
    assert not [n for n in NEW_CORE if n not in core]
    assert not [n for n in NEW_CORE if n in ga]


@pytest.mark.parametrize("dim", [1, 2, 7, 1000, 1024, 2 ** 31 - 1])
def test_sprs_range_is_the_owner_formula(dim):
    for nproc in (1, 2, 3, 5, 8):
        ranges = [ga_amd.sprs_range(dim, nproc, p) for p in range(nproc)]
        assert ranges == [S.own_range(dim, nproc, p) for p in range(nproc)]
        nxt = 0
        for p, (lo, hi) in enumerate(ranges):   # ascending, every index exactly once
            assert lo == nxt and hi >= lo - 1
            nxt = hi + 1
            if hi >= lo:   # the ends belong to p, their outer neighbours do not
                assert S.owner(lo, dim, nproc) == p == S.owner(hi, dim, nproc)
                assert lo == 0 or S.owner(lo - 1, dim, nproc) < p
                assert hi == dim - 1 or S.owner(hi + 1, dim, nproc) > p
        assert nxt == dim
        if dim <= 1024:   # brute force
            own = S.owner(np.arange(dim), dim, nproc)
            for p, (lo, hi) in enumerate(ranges):
                assert np.array_equal(np.flatnonzero(own == p), np.arange(lo, hi + 1))
    assert ga_amd.sprs_range(0, 2, 0) == (0, -1) and ga_amd.sprs_range(10, 2, 2) == (0, -1)   # not a case: empty


def test_spmv_team_rule():
    teams = set()
    for rows in (1, 3, 1000, 3001, 1 << 20, 1 << 40):
        last = 1
        for avg16 in range(0, 16 * 300, 7):   # nnz / rows from 0 to 300 in sixteenths
            nnz = rows * avg16 // 16
            w = ga_amd.spmv_team(nnz, rows)
            assert w in (1, 2, 4, 8, 16, 32, 64) and w >= last   # grows with nnz
            assert w == 64 or 2 * w * rows >= nnz
            assert w == 1 or 2 * (w // 2) * rows < nnz            # the smallest such power of two
            last = w
            teams.add(w)
    assert teams == set(S.TEAMS)
    for nnz in (10, 40000, 1 << 30):   # shrinks with rows
        ws = [ga_amd.spmv_team(nnz, rows) for rows in (1, 10, 1000, 100000, 1 << 31)]
        assert ws == sorted(ws, reverse=True)
    assert ga_amd.spmv_team(0, 10) == ga_amd.spmv_team(10, 0) == ga_amd.spmv_team(-1, -1) == 1
    assert ga_amd.spmv_team(40000, 3001) == 8 and ga_amd.spmv_team(27 << 20, 1 << 20) == 16


# ---- the codes of the kernel entry points -------------------------------------------------
A = 0x7F0000000000   # address-shaped numbers; never read


def test_kernel_entry_point_codes():
    E_COUNT, E_OP, E_SCALAR, E_RANGE, E_ALIGN = -3, -4, -5, -7, -8
    op = S.DBL
    spmv = lambda **k: ga_amd.spmv(**{**dict(op=op, nrows=5, nblk=1, offs=A, start=A, jdx=A, val=A, x=A, x_first=0, y=A,  # noqa: E731
                                             team=8), **k})
    assert spmv(nrows=-1) == E_COUNT == spmv(nblk=-1)
    assert spmv(op=36) == E_OP == spmv(team=3) == spmv(team=0) == spmv(team=128)
    assert spmv(nrows=0) == 0 == spmv(nrows=0, y=0)          # nothing to do comes before the pointers
    assert spmv(op=36, nrows=-1) == E_COUNT
    for miss in ("offs", "start", "jdx", "val", "x", "y"):
        assert spmv(**{miss: 0}) == E_SCALAR, miss
    assert spmv(nrows=(1 << 40) + 1) == E_RANGE
    assert spmv(y=A + 4) == E_ALIGN == spmv(start=A + 4) == spmv(jdx=A + 2) == spmv(op=S.DCP, x=A + 8)
    diag = lambda **k: ga_amd.sprs_diag(**{**dict(op=op, fn=S.GET, nrows=5, offs=A, jdx=A, val=A, diag_first=0, out=A,  # noqa: E731
                                                  team=8), **k})
    assert diag(nrows=-1) == E_COUNT and diag(fn=2) == E_OP == diag(team=5) == diag(op=0)
    assert diag(nrows=0) == 0 and diag(out=0) == E_SCALAR == diag(fn=S.SHIFT) == diag(val=0)
    assert diag(out=A + 4) == E_ALIGN
    left = lambda **k: ga_amd.sprs_scale_left(**{**dict(op=op, nrows=5, offs=A, val=A, d=A, team=8), **k})  # noqa: E731
    assert left(nrows=-1) == E_COUNT and left(team=6) == E_OP and left(nrows=0) == 0 and left(d=0) == E_SCALAR
    right = lambda **k: ga_amd.sprs_scale_right(**{**dict(op=op, n=5, jdx=A, val=A, d=A, d_first=0), **k})  # noqa: E731
    assert right(n=-1) == E_COUNT and right(op=1) == E_OP and right(n=0) == 0 and right(jdx=0) == E_SCALAR
    assert right(n=1 << 39) == E_RANGE and right(val=A + 4) == E_ALIGN


# ---- the restatement against loops written from the contract -------------------------------
def loop_mul(op, a, x):
    """one product: Python ints modulo 2^bits; the floating-point types through numpy scalars, one rounding
    per operation"""
    if op in UNS:
        bits = 8 * DT[op].itemsize
        return (int(a) % (1 << bits)) * (int(x) % (1 << bits)) % (1 << bits)
    if op in REAL:
        r = REAL[op].type
        ar, ai, xr, xi = r(a.real), r(a.imag), r(x.real), r(x.imag)
        p1, p2, p3, p4 = r(ar * xr), r(ai * xi), r(ar * xi), r(ai * xr)
        return (r(p1 - p2), r(p3 + p4))
    return DT[op].type(a * x)


def loop_add(op, a, b):
    if op in UNS:
        return (a + b) % (1 << (8 * DT[op].itemsize))
    if op in REAL:
        r = REAL[op].type
        return (r(a[0] + b[0]), r(a[1] + b[1]))
    return DT[op].type(a + b)


def loop_spmv(op, csr, x, W):
    zero = 0 if op in UNS else (REAL[op].type(0), REAL[op].type(0)) if op in REAL else DT[op].type(0)
    out = []
    for r in range(csr["nrows"]):
        lst = []   # the row's list over the blocks in ascending order
        for b in range(len(csr["blocks"])):
            s, o = int(csr["start"][b]), csr["offs"][b]
            lst += list(range(s + o[r], s + o[r + 1]))
        part = []
        for lane in range(W):
            acc = zero
            for k in lst[lane::W]:
                acc = loop_add(op, acc, loop_mul(op, csr["val"][k], x[csr["jdx"][k]]))
            part.append(acc)
        s = 1
        while s < W:
            part = [loop_add(op, part[l], part[l ^ s]) for l in range(W)]
            s *= 2
        out.append(part[0])
    if op in UNS:
        return np.array(out, dtype=UNS[op]).view(DT[op])
    if op in REAL:
        return K._cplx(op, np.array([p[0] for p in out]), np.array([p[1] for p in out]))
    return np.array(out, dtype=DT[op])


@pytest.mark.parametrize("W", [1, 2, 8, 64])
@pytest.mark.parametrize("op", OPS, **opid)
def test_restatement_matches_loops(op, W):
    """rows of 0, 1, W-1, W, W+1 and 3W+5 entries (duplicates among them) over 3 column blocks"""
    rng = np.random.default_rng(op * 10 + W)
    jdim, counts = 400, [0, 1, max(W - 1, 0), W, W + 1, 3 * W + 5, 0]
    ii, jj = [], []
    for r, c in enumerate(counts):
        ii += [r] * c
        jj += rng.choice(jdim, c, replace=False).tolist()
    ii += [4, 4]
    jj += [jj[ii.index(4)]] * 2   # one (i, j) of row 4 three times
    perm = rng.permutation(len(ii))
    i, j = np.array(ii)[perm], np.array(jj)[perm]
    v, x = K.gen(op, len(i), rng), K.gen(op, jdim, rng)
    csr = S.build_csr(i, j, v, 0, len(counts), jdim, 3)
    # the assembly's order: blocks ascending, rows ascending, columns ascending, duplicates in input order
    for b, blk in enumerate(csr["blocks"]):
        s, o = int(csr["start"][b]), csr["offs"][b]
        for r in range(len(counts)):
            cols = csr["jdx"][s + o[r]:s + o[r + 1]]
            assert (np.diff(cols) >= 0).all() and (S.owner(cols.astype(np.int64), jdim, 3) == blk).all()
    dup = np.flatnonzero((csr["jdx"] == jj[ii.index(4)]) & (S.entry_rows(csr) == 4))
    want_order = [k for k in range(len(i)) if i[k] == 4 and j[k] == jj[ii.index(4)]]
    assert len(dup) == 3 and [csr["val"][k].tobytes() for k in dup] == [v[k].tobytes() for k in want_order]
    got = S.ref_spmv(op, csr, x, 0, W)
    want = loop_spmv(op, csr, x, W)
    assert got.tobytes() == want.tobytes(), (np.flatnonzero(got != want), got, want)


def test_ref_assemble_orders_by_source_rank():
    """two ranks add the same (i, j): the lower rank's copy comes first, whatever the global order was"""
    i, j = np.array([3, 3, 3, 0]), np.array([2, 2, 2, 1])
    v = np.array([10.0, 20.0, 30.0, 40.0])
    src = np.array([1, 0, 1, 0])
    for rank in (0, 1):
        csr = S.ref_assemble(S.ga_parts(i, j, v, src, 2), 4, 4, 2, rank)
        assert csr["val"].tolist() == ([40.0] if rank == 0 else [20.0, 10.0, 30.0])


# ---- the host part of the assembly under the sanitizers ------------------------------------------
@pytest.fixture(scope="module")
def sprs_build_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sprs") / "sprs_build_main"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "sprs_build_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.mark.parametrize("name", ["ladder", "tiny", "gap", "dups", "idle"])
def test_assembly_host_code_under_sanitizers(sprs_build_exe, name):
    for size in (1, 2, 3):
        idim, jdim, i, j, src = S.ga_matrix(name, size)
        v = np.arange(len(i), dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        parts = S.ga_parts(i, j, v, src, size)
        lines = [f"{idim} {jdim} {size} {len(i)}"]
        for pi, pj, pv in parts:   # the order the owners receive them in
            lines += [f"{a} {b} {c}" for a, b, c in zip(pi.tolist(), pj.tolist(), pv.tolist())]
        r = subprocess.run([sprs_build_exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
        want = []
        for p in range(size):
            c = S.ref_assemble(parts, idim, jdim, size, p)
            lo, hi = S.own_range(idim, size, p)
            row = lambda tag, a: " ".join([tag] + [str(int(t)) for t in np.asarray(a).reshape(-1)])  # noqa: E731
            want += [f"rank {p} rows {lo} {hi}", row("blocks", c["blocks"]), row("start", c["start"]), row("offs", c["offs"]),
                     row("jdx", c["jdx"]), row("val", c["val"])]
        assert r.stdout.splitlines() == want, (name, size)
