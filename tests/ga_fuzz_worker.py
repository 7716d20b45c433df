"""One rank of the GA-layer fuzz (test_gpu_ga_fuzz_mp.py starts 1, 2, 3 or 4 of these on one GPU).

Runs every case of ga_fuzz_cases.cases(seed, size) -- seed 0, shifted by GAAMD_FUZZ_SEED -- whose
call family is named in GA_FUZZ_FAMILIES (a comma-separated list; all families when it is not
set) or, with GA_FUZZ_ONLY=<index>, that one case alone.

Per array, right after creation: the blocks NGA_Distribution reports tile the array exactly,
GA_Get_proc_grid agrees with them, and after rank 0's NGA_Put every rank reads its own block
through NGA_Access and gaamd_memcpy and compares it with the model's slice -- a placement check
that does not go back through the path the put took.
Per case: the call; then every array involved, by NGA_Get of the whole array on every rank,
against the numpy model as raw bits (inputs unchanged, nothing changed outside the patch), the
own-block read of every array the call wrote, the scalar results equal to the model's, and
gaamd_ga_live_arrays unchanged by the call.

Prints "RESULT <index>:<call>:<name> <hex>" for every scalar result (the launcher wants the
same lines from every rank and on every rank count), "CASES <run> of <generated>" and
"RANK <r> OK".  A failure names the seed, the case index and the whole case; the ranks agree on
it after the case's last collective call, so all of them end there and none waits in a barrier.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import ga_amd  # noqa: E402
import ga_fuzz_cases as F  # noqa: E402
from ga_worker import DOT_OF, C_DBL, blocks_of, ia, sl, vp  # noqa: E402

SEED = int(os.environ.get("GAAMD_FUZZ_SEED", "0"))


class Arr:
    """a global array of a case: its handle, its blocks and the model's contents"""

    def __init__(self, L, spec, name, rank, size):
        self.L, self.dims, self.nd = L, spec["dims"], len(spec["dims"])
        self.dt = ga_amd.OP_DTYPE[F.OP_OF[spec["t"]]]
        m = spec["map"]
        if m["kind"] == "irreg":
            self.g = L.NGA_Create_irreg(spec["t"], self.nd, ia(self.dims), name, ia(m["block"]),
                                        ia([s for d in m["starts"] for s in d]))
        else:
            self.g = L.NGA_Create(spec["t"], self.nd, ia(self.dims), name, ia(m["chunk"]) if m["kind"] == "chunk" else None)
        assert self.g > 0
        self.blocks = blocks_of(L, self.g, self.nd, size)
        self.mine = self.blocks[rank] if all(h >= l for l, h in zip(*self.blocks[rank])) else None

    def check_distribution(self, m, size):
        """disjoint and covering; the process grid is the number of distinct block starts"""
        cover = np.zeros(self.dims, dtype=np.int32)
        owners = [(lo, hi) for lo, hi in self.blocks if all(h >= l for l, h in zip(lo, hi))]
        for lo, hi in owners:
            assert all(0 <= l and h < d for l, h, d in zip(lo, hi, self.dims)), (lo, hi)
            cover[sl(lo, hi)] += 1
        assert (cover == 1).all(), f"the blocks do not tile the array: {self.blocks}"
        grid = (ctypes.c_int * self.nd)()
        self.L.GA_Get_proc_grid(self.g, grid)
        assert [len({lo[d] for lo, _ in owners}) for d in range(self.nd)] == list(grid), (list(grid), self.blocks)
        assert int(np.prod(list(grid))) == len(owners) <= size
        assert owners == self.blocks[:len(owners)]   # the ranks beyond the grid own nothing
        if m["kind"] == "irreg":
            assert list(grid) == m["block"] and owners == [b for b in F.blocks(m, self.dims, size) if b], self.blocks

    def put(self, vals, rank):
        """rank 0 writes the whole array (the array is new: nobody reads it yet; the caller syncs)"""
        if rank == 0:
            self.L.NGA_Put(self.g, ia([0] * self.nd), ia([d - 1 for d in self.dims]), vp(vals), ia(self.dims[1:]))

    def own_block(self, model, what):
        """this rank's block through NGA_Access and a plain device-to-host copy"""
        if self.mine is None:
            return
        lo, hi = self.mine
        ext = [h - l + 1 for l, h in zip(lo, hi)]
        ptr, ld = ctypes.c_void_p(), (ctypes.c_int * max(1, self.nd - 1))()
        self.L.NGA_Access(self.g, ia(lo), ia(hi), ctypes.byref(ptr), ld)
        assert list(ld)[:self.nd - 1] == ext[1:], (list(ld), ext)
        got = np.empty(ext, dtype=self.dt)
        assert self.L.gaamd_memcpy(vp(got), ptr, got.nbytes) == 0
        self.L.NGA_Release(self.g, ia(lo), ia(hi))
        want = np.ascontiguousarray(model[sl(lo, hi)])
        assert got.tobytes() == want.tobytes(), \
            f"{what}: own block {lo}..{hi}: {np.count_nonzero(got.view(np.uint8) != want.view(np.uint8))} bytes differ"

    def check(self, model, what):
        got = np.empty(self.dims, dtype=self.dt)
        self.L.NGA_Get(self.g, ia([0] * self.nd), ia([d - 1 for d in self.dims]), vp(got), ia(self.dims[1:]))
        if got.tobytes() != model.tobytes():
            bad = np.argwhere((got.view(np.uint8).reshape(*self.dims, -1) != model.view(np.uint8).reshape(*self.dims, -1)).any(-1))
            raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ, the first at {bad[0].tolist()}")


def call(L, c, A):
    """the GA call of the case on the arrays A; {name: bytes} of its scalar results"""
    name, g, P, t = c["call"], {r: A[i].g for r, i in c["args"].items()}, c["patch"], c["t"]
    sc = F.scalars(c)
    res = {}
    lohi = {r: (ia(P[r][0]), ia(P[r][1])) for r in P}
    base = name[:-6] if name.endswith("_patch") else name
    if name in ("GA_Fill", "GA_Scale"):
        getattr(L, name)(g["a"], vp(sc["value" if name == "GA_Fill" else "alpha"]))
    elif name == "GA_Zero":
        L.GA_Zero(g["a"])
    elif name == "NGA_Fill_patch":
        L.NGA_Fill_patch(g["a"], *lohi["a"], vp(sc["value"]))
    elif name == "NGA_Scale_patch":
        L.NGA_Scale_patch(g["a"], *lohi["a"], vp(sc["alpha"]))
    elif name == "NGA_Zero_patch":
        L.NGA_Zero_patch(g["a"], *lohi["a"])
    elif name == "GA_Add":
        L.GA_Add(vp(sc["alpha"]), g["a"], vp(sc["beta"]), g["b"], g["c"])
    elif name == "NGA_Add_patch":
        L.NGA_Add_patch(vp(sc["alpha"]), g["a"], *lohi["a"], vp(sc["beta"]), g["b"], *lohi["b"], g["c"], *lohi["c"])
    elif name == "GA_Copy":
        L.GA_Copy(g["a"], g["b"])
    elif name == "NGA_Copy_patch":
        L.NGA_Copy_patch(b"N", g["a"], *lohi["a"], g["b"], *lohi["b"])
    elif base in ("GA_dot", "NGA_dot"):
        if name == "GA_dot":
            v = getattr(L, f"GA_{DOT_OF[t]}dot")(g["a"], g["b"])
        else:
            v = getattr(L, f"NGA_{DOT_OF[t]}dot_patch")(g["a"], b"N", *lohi["a"], g["b"], b"N", *lohi["b"])
        dt = ga_amd.OP_DTYPE[F.OP_OF[t]]
        res["dot"] = np.array([complex(v.real, v.imag) if dt.kind == "c" else v], dtype=dt).tobytes()
    elif base in F.ELEM1:
        args = [g["a"]] + (list(lohi["a"]) if P else []) + ([vp(sc["const"])] if base == "GA_Add_constant" else [])
        getattr(L, name)(*args)
    elif base in F.ELEM2:
        if P:
            getattr(L, name)(g["a"], *lohi["a"], g["b"], *lohi["b"], g["c"], *lohi["c"])
        else:
            getattr(L, name)(g["a"], g["b"], g["c"])
    elif name == "NGA_Select_elem":
        a = A[c["args"]["a"]]
        val, index = np.zeros(1, dtype=a.dt), (ctypes.c_int * a.nd)(*([-1] * a.nd))
        L.NGA_Select_elem(g["a"], c["op"].encode(), vp(val), index)
        res["val"], res["index"] = val.tobytes(), np.array(list(index), dtype=np.int32).tobytes()
    elif name in ("GA_Dgemm", "GA_Sgemm"):
        getattr(L, name)(c["ta"].encode(), c["tb"].encode(), c["m"], c["n"], c["k"], F.GEMM_ALPHA, g["a"], g["b"],
                         F.GEMM_BETA, g["c"])
    elif name == "NGA_Matmul_patch":
        dt = np.float64 if t == C_DBL else np.float32
        al, be = np.array([F.GEMM_ALPHA], dtype=dt), np.array([F.GEMM_BETA], dtype=dt)
        L.NGA_Matmul_patch(c["ta"].encode(), c["tb"].encode(), vp(al), vp(be), g["a"], *lohi["a"], g["b"], *lohi["b"],
                           g["c"], *lohi["c"])
    elif name == "GA_Transpose":
        L.GA_Transpose(g["a"], g["b"])
    elif name in ("GA_Symmetrize", "GA_Zero_diagonal"):
        getattr(L, name)(g["a"])
    elif name == "GA_Shift_diagonal":
        L.GA_Shift_diagonal(g["a"], vp(sc["shift"]))
    elif name in ("GA_Set_diagonal", "GA_Add_diagonal", "GA_Get_diag", "GA_Scale_rows", "GA_Scale_cols"):
        getattr(L, name)(g["a"], g["v"])
    elif name in ("GA_Norm1", "GA_Norm_infinity"):
        nm = ctypes.c_double(-1.0)
        getattr(L, name)(g["a"], ctypes.byref(nm))
        res["norm"] = np.float64(nm.value).tobytes()
    elif name == "GA_Patch_enum":
        L.GA_Patch_enum(g["a"], c["lo"], c["hi"], vp(sc["start"]), vp(sc["inc"]))
    elif name == "GA_Scan_copy":
        L.GA_Scan_copy(g["src"], g["dst"], g["msk"], c["lo"], c["hi"])
    elif name == "GA_Scan_add":
        L.GA_Scan_add(g["src"], g["dst"], g["msk"], c["lo"], c["hi"], c["excl"])
    elif name in ("GA_Pack", "GA_Unpack"):
        ic = ctypes.c_int(-1)
        getattr(L, name)(g["src"], g["dst"], g["msk"], c["lo"], c["hi"], ctypes.byref(ic))
        res["icount"] = np.int32(ic.value).tobytes()
    else:
        raise AssertionError(f"no such call: {name}")
    return res


class Checks:
    """the checks of one case: the first failure is kept and the collectives of the case go on, so
    that the ranks can agree on the outcome instead of one leaving the others in a barrier"""

    def __init__(self):
        self.failure = None

    def run(self, fn, *args):
        if self.failure is None:
            try:
                fn(*args)
            except AssertionError as e:
                self.failure = str(e) or repr(e)


def same(a, b, what):
    assert a == b, f"{what}: {a!r} != {b!r}"


def run_case(L, rank, size, c):
    """None, or what went wrong on this rank"""
    ok = Checks()
    live0 = L.gaamd_ga_live_arrays()
    before = F.inputs(c)
    after, want = F.model(c, before)
    A = []
    for i, (spec, x) in enumerate(zip(c["arrays"], before)):
        a = Arr(L, spec, f"fuzz{c['index']}.{i}".encode(), rank, size)
        A.append(a)
        ok.run(a.check_distribution, spec["map"], size)
        a.put(x, rank)
    L.GA_Sync()   # rank 0's puts are complete at their owners
    for i, (a, x) in enumerate(zip(A, before)):
        ok.run(a.own_block, x, f"array {i} after NGA_Put")
    live = L.gaamd_ga_live_arrays()
    ok.run(same, live, live0 + len(A), "live arrays after creation")
    got = call(L, c, A)
    ok.run(same, L.gaamd_ga_live_arrays(), live, "live arrays after the call (a temporary is left)")
    ok.run(same, sorted(got), sorted(want), "names of the scalar results")
    for k in sorted(got):
        print(f"RESULT {c['index']}:{c['call']}:{k} {got[k].hex()}", flush=True)
        ok.run(same, got[k].hex(), want.get(k, b"").hex(), f"scalar result {k} against the model")
    for i, a in enumerate(A):
        ok.run(a.check, after[i], f"array {i} after the call ({'written' if i in F.written(c) else 'an input'})")
        if i in F.written(c):
            ok.run(a.own_block, after[i], f"array {i} after the call")
    L.GA_Sync()   # no rank destroys what another still reads
    for a in A:
        L.GA_Destroy(a.g)
    ok.run(same, L.gaamd_ga_live_arrays(), live0, "live arrays after GA_Destroy")
    return ok.failure


def main():
    import faulthandler
    faulthandler.dump_traceback_later(int(os.environ.get("TEST_STACK_DUMP_S", "600")), exit=False)
    rank, size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    L = ga_amd.lib()
    assert L.GA_Initialize() == 0
    cs = F.cases(SEED, size)
    only = os.environ.get("GA_FUZZ_ONLY")
    fams = os.environ.get("GA_FUZZ_FAMILIES", ",".join(F.FAMILIES)).split(",")
    assert set(fams) <= set(F.FAMILIES), fams
    todo = [c for c in cs if c["fam"] in fams] if only is None else [cs[int(only)]]
    ran = 0
    for c in todo:
        failure = run_case(L, rank, size, c)
        flag = ctypes.c_int(1 if failure else 0)
        L.armci_msg_igop(ctypes.byref(flag), 1, b"max")   # every rank learns of a failure on any rank
        if flag.value:
            print(f"FUZZ FAILURE seed {SEED} ranks {size} case {c['index']} (rerun it alone with GA_FUZZ_ONLY={c['index']}): "
                  f"{failure or 'on another rank'}\n{json.dumps(c)}", flush=True)
            L.GA_Terminate()
            sys.exit(1)
        ran += 1
    L.GA_Sync()
    print(f"CASES {ran} of {len(todo)}", flush=True)
    L.GA_Terminate()
    print(f"RANK {rank} OK", flush=True)


if __name__ == "__main__":
    main()
