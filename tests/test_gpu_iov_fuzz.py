"""Seeded io-vector fuzz over the routing thresholds of comex_accv / putv / getv
(ga_amd/csrc/iov.cpp, gaamd_iov.hip), bit-exact against the oracle's pair-by-pair loop
(ora_accv / ora_copyv: comex.c:7327-7400, one _acc or memcpy per pair, in order).

What a scatter-accumulate computes depends on a chain of size thresholds (2048 pairs:
GPU ordering without a host check; 1024: one workgroup or partitions; 1024 entries a
partition bucket; 65536: windows or deferral to the masked radix pass; 131072 and every
64 Ki: host passes over the pool; 2^19 and 8192 conflicts: the hashed path's hand-overs;
n = 129 * 2^lg: the partition count; 2^22: radix only).  tests/test_gpu_fuzz.py draws n
log-uniformly to 150 000, which almost never lands on one of them.  Here

  * every seed runs a FIXED schedule of size classes either side of each threshold;
  * a small predictor (`predict`, restating iov.cpp's classification and the partition
    hash of gaamd_iov.hip) says which path counters (ga_amd.iov_path_counts) a call must
    move, and every case asserts those deltas exactly as well as the bytes: a seed
    provably reached the route it was meant to reach;
  * destination mode (f) loads ONE partition with exactly 1023 / 1024 / 1025 / 1500
    entries, the point where k_iov_keyof's overflow flag, k_iov_part's early return and
    k_iov_keys_partmask's mask have to agree;
  * both sides' bases get offsets below the natural alignment, so that the launcher's
    vector width W = lowbit(addresses | row | 16) is not always the widest (W < esz -> esz
    for a double at 4 bytes; 16-byte float pairs at base + 4 -> W = 4);
  * every acc / put case of up to 2^19 + 1 pairs runs again with tuning iov_lds=0 (the
    hashed path, which getv from a peer GPU still uses, and its hand-over to radix);
  * every case that defers partitions runs a second time (the partition counters must be
    back at zero, or the second result differs).

No tolerance anywhere; NaNs match any NaN (helpers.same_bits_nan_aware).
Destination spans of 8 to 16 GiB and the limit on `units` (every GPU-ordered route takes
units < 0xffffffff, the classification and the launchers alike; from there up the
host-checked kernels): tests/test_gpu_far_offsets.py.
"""
import ctypes
import os

import numpy as np
import pytest

import cases as C
import ga_amd
from helpers import _giov, first_mismatch, phased_fill, random_alpha, same_bits_nan_aware

pytestmark = pytest.mark.gpu

OPS = (C.INT, C.DBL, C.FLT, C.CPL, C.DCP, C.LNG)
# GAAMD_FUZZ_SEED shifts every seed, as in test_gpu_fuzz.py; 0 is the suite's
SEED = int(os.environ.get("GAAMD_FUZZ_SEED", "0")) * 100003

PATHS = ("hashed", "hashed_then_radix", "radix", "lds")
# the thresholds restated (iov.cpp, gaamd_kernels.h, gaamd_iov.hip)
RUNS_MIN, RUNS_MAX_BYTES = 2048, 256
LDS_ROUTE, PART_CAP, PART_WINDOW_MAX, PART_MAX = 1024, 1024, 1 << 16, 1 << 22
PART_MEAN, PART_GMAX = 128, 8192
HASH_MAX_PAIRS, HASH_CAP = 1 << 19, 8192
HOST_POOL_MIN = 131072

BIG = (PART_MAX - 1, PART_MAX, PART_MAX + 1, PART_MAX + 1024)
N_MAX = PART_MAX + 1024
PAIR_BUDGET = 8 << 20          # pairs a seed schedules in all (the 2^22-class id included)
MAX_REGION = 640 << 20         # destination region bytes of one case
MAX_SRC = 256 << 20            # source bytes of one case
SERIAL_MAX = 65537             # cases the one-lane serial kernel may get stay this small


# ---------------------------------------------------------------------------------------
# the predictor
def part_lg(n):
    """iov_part_lg: log2 of the partitions for n pairs"""
    lg = 0
    while (n >> lg) > PART_MEAN and (1 << lg) < PART_GMAX:
        lg += 1
    return lg


def part_of(keys_u32, lg):
    """iov_part_of: the 0x9E3779B1 multiply in uint32, then the top lg bits"""
    keys = np.asarray(keys_u32, dtype=np.uint32)
    if lg == 0:
        return np.zeros(keys.shape, dtype=np.uint32)
    return (keys * np.uint32(0x9E3779B1)) >> np.uint32(32 - lg)


def predict(n, nbytes, dst_offsets, iov_lds):
    """Expected deltas of ga_amd.iov_path_counts() for one local accv / putv (or getv into
    device memory) of n pairs of nbytes at the byte offsets dst_offsets: iov.cpp's
    classification of the destinations, then the route of the GPU-ordered calls."""
    out = dict.fromkeys(PATHS, 0)
    d = np.asarray(dst_offsets, dtype=np.uint64)
    if np.array_equal(d, d[0] + np.arange(n, dtype=np.uint64) * np.uint64(nbytes)):
        return out                                # one contiguous vector in pair order
    if nbytes > RUNS_MAX_BYTES:
        return out                                # host-checked: plain or serial kernel
    rel = d - d.min()
    if np.any(rel % np.uint64(nbytes)):
        return out                                # partial overlaps possible: host-checked
    keys = rel // np.uint64(nbytes)
    assert int(keys.max()) < (1 << 31), "destination span far below 2^32 units"
    if n < RUNS_MIN and np.unique(keys).size == n:
        return out                                # the host hash check finds no repeat
    if iov_lds:
        if n <= PART_MAX:
            out["lds"] = 1
            if n > PART_WINDOW_MAX:
                lg = part_lg(n)
                counts = np.bincount(part_of(keys.astype(np.uint32), lg), minlength=1 << lg)
                if counts.max() > PART_CAP:
                    out["radix"] = 1              # deferred partitions: the masked radix pass
        else:
            out["radix"] = 1
    elif n <= HASH_MAX_PAIRS:
        _, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
        conflicts = int((cnt[inv] > 1).sum())     # pairs whose destination repeats
        out["hashed" if conflicts <= HASH_CAP else "hashed_then_radix"] = 1
    else:
        out["radix"] = 1
    return out


def launcher_width(op, nbytes, addr_or):
    """(W, widest): the vector width the launchers take for elements of `op` in pairs of
    nbytes whose listed addresses OR to addr_or (W = lowbit(addresses | row | 16), at most
    16, raised to esz when below it), and the widest the pair size alone allows"""
    esz = C.ESZ[op]
    row = (nbytes // esz) * esz
    lowbit = lambda x: x & -x
    widest = min(16, lowbit(row | 16))
    W = min(16, lowbit(int(addr_or) | row | 16))
    return W, widest


# ---------------------------------------------------------------------------------------
# case construction
def big_fill(op, nbytes, off, seed):
    """phased_fill for any size: above 4 MiB one generated MiB of elements repeated"""
    if nbytes <= (4 << 20):
        return phased_fill(op, nbytes, off, seed)
    ph = off % C.ESZ[op]
    out = np.zeros(nbytes, dtype=np.uint8)
    out[ph:] = np.resize(C.fill_bytes(op, 1 << 20, seed), nbytes - ph)
    return out


def loaded_partition(rng, n, k, repeated):
    """(keys, slots): n destination keys of which exactly k hash to one partition p under
    part_of(., part_lg(n)) -- k distinct keys, or one key k times -- and no other does; at
    random positions.  Key 0 is always present (the library's keys are relative to the
    lowest destination): it lies in partition 0, so p > 0 unless k == n."""
    lg = part_lg(n)
    G = 1 << lg
    slots = max(2 * n, 2048 * G)
    if k < n:
        assert G > 1
        p = int(rng.integers(1, G))
    else:
        p = 0
    while True:
        universe = np.arange(slots, dtype=np.uint32)
        in_p = universe[part_of(universe, lg) == p]
        if in_p.size > k:
            break
        slots *= 2
    if p == 0:        # every pair in partition 0: key 0 among them
        hot = np.concatenate([[0], rng.choice(in_p[1:], k - 1, replace=False)]) if not repeated else np.zeros(k)
    elif repeated:
        hot = np.full(k, rng.choice(in_p))
    else:
        hot = rng.choice(in_p, k, replace=False)
    rest = rng.integers(0, slots, n - k).astype(np.uint32)
    bad = np.nonzero(part_of(rest, lg) == p)[0]
    while bad.size:
        rest[bad] = rng.integers(0, slots, bad.size).astype(np.uint32)
        bad = bad[part_of(rest[bad], lg) == p]
    if rest.size:
        rest[0] = 0
    keys = np.concatenate([hot.astype(np.uint32), rest])[rng.permutation(n)]
    assert int(keys.min()) == 0 and int(np.count_nonzero(part_of(keys, lg) == p)) == k
    return keys.astype(np.uint64), slots


def mode_slots(mode, n):
    """destination slots a mode may span at n pairs (for the size caps)"""
    if mode == "a":
        return n
    if mode == "d":
        return max(1, n // 4)
    if mode == "e":
        return 64
    if mode == "f":
        return 2 * max(2 * n, 2048 << part_lg(n))
    return 8 * n + 16


def destinations(rng, mode, n, nbytes, esz, variant=None):
    """(byte offsets from the destination base, region bytes) of one mode:
    a contiguous in pair order; b all distinct, scattered over 8n slots; c sparse random
    in 8n + 16 slots (a few repeats); d dense random in n / 4 slots; e a hot set of 1-64
    slots; f one loaded partition (variant = (k, repeated)); g partial overlaps (a grid of
    single elements under multi-element pairs)"""
    B = np.uint64(nbytes)
    if mode == "a":
        return np.arange(n, dtype=np.uint64) * B, n * nbytes
    if mode == "b":
        keys = rng.permutation(n).astype(np.uint64) * np.uint64(8) + rng.integers(0, 8, n).astype(np.uint64)
        return keys * B, 8 * n * nbytes
    if mode == "f":
        keys, slots = loaded_partition(rng, n, *variant)
        return keys * B, slots * nbytes
    slots = {"c": 8 * n + 16, "d": max(1, n // 4), "e": int(rng.integers(1, 65)),
             "g": (8 * n + 16, max(1, n // 4), int(rng.integers(1, 65)))[int(rng.integers(0, 3))]}[mode]
    step = esz if mode == "g" else nbytes
    return rng.integers(0, slots, n).astype(np.uint64) * np.uint64(step), slots * step + nbytes


def sources(rng, n, nbytes):
    """one vector in pair order (GA's `v`), a permutation, or random repeats"""
    k = int(rng.integers(0, 3))
    if k == 0:
        return np.arange(n, dtype=np.uint64) * np.uint64(nbytes)
    if k == 1:
        return rng.permutation(n).astype(np.uint64) * np.uint64(nbytes)
    return rng.integers(0, n, n).astype(np.uint64) * np.uint64(nbytes)


def pick_pair_size(rng, kind, n, mode, op=None, want_even=False):
    """(op, nbytes) within the size caps: acc esz x {1,1,1,2,3,8}, put/get that of a double
    or 1-40 arbitrary bytes; mode g needs pairs of several elements; want_even: a row that
    is a multiple of 8 bytes (so that a base offset of 4 lowers W)"""
    slots = mode_slots(mode, n)
    fits = lambda b: slots * b <= MAX_REGION and n * b <= MAX_SRC
    if kind == "acc":
        nels = (2, 3, 8) if mode == "g" else (1, 1, 1, 2, 3, 8)
        ok = {o: [e for e in nels if fits(C.ESZ[o] * e) and not (want_even and (C.ESZ[o] * e) % 8)]
              for o in ((op,) if op is not None else OPS)}
        ok = {o: v for o, v in ok.items() if v}
        op = sorted(ok)[int(rng.integers(0, len(ok)))]
        return op, C.ESZ[op] * int(rng.choice(ok[op]))
    nels = [e for e in ((2, 3, 8) if mode == "g" else (1, 1, 1, 2, 3, 8)) if fits(8 * e)]
    whole = 8 * int(rng.choice(nels)) if nels else 8
    odd = 1 + int(rng.integers(1 if mode == "g" else 0, 40))
    return C.DBL, (whole if rng.random() < 0.5 or not fits(odd) else odd)


class Seed:
    """one seed's draws and what its cases covered"""

    def __init__(self, rng):
        self.rng = rng
        self.k = 0                 # cases made (the kind rotation)
        self.acc = 0               # acc cases made
        self.acc_reduced = 0       # of them: W < esz or W below the pair's widest
        self.seen = set()
        self.log = []

    def make(self, n, kind=None, mode=None, nbytes=None, op=None, host_src=None, host_dst=None):
        """the cases of one draw at n pairs (mode f gives two: k distinct keys, and one key
        k times); anything not given is drawn"""
        rng = self.rng
        kind = kind or ("acc", "acc", "put", "get")[self.k % 4]
        self.k += 1
        if mode is None:
            mode = "abcdefg"[int(rng.integers(0, 7))]
        if mode == "f" and n < LDS_ROUTE:
            mode = "e"
        if mode == "g" and n > SERIAL_MAX:
            mode = "d"
        # whenever fewer than a third of the seed's acc cases so far ran below the widest
        # vector, the next is made to: base + 4 on the destination side and a row of a
        # multiple of 8 bytes (W = 4)
        force = kind == "acc" and 3 * self.acc_reduced <= self.acc and (nbytes is None or nbytes % 8 == 0)
        if nbytes is None:
            op, nbytes = pick_pair_size(rng, kind, n, mode, op, want_even=force)
        elif op is None:
            op = C.DBL
        esz = C.ESZ[op] if kind == "acc" else 1
        if mode == "g" and nbytes <= esz:
            mode = "d"
        if host_src is None:
            host_src = kind != "get" and rng.random() < 0.3
        if host_dst is None:
            host_dst = kind == "get" and rng.random() < 0.5
        if kind == "acc":
            # offsets the library accepts: multiples of 4 (below that is its -8 refusal)
            offs = [0, C.ESZ[op], 4, 8, 16, 32, 48]
            s_off, d_off = int(rng.choice(offs)), int(rng.choice(offs))
            if force:
                d_off = 4
        else:
            s_off, d_off = int(rng.integers(0, 16)), int(rng.integers(0, 16))
        alpha = random_alpha(rng, op) if kind == "acc" else None
        so = sources(rng, n, nbytes)
        variants = [None]
        if mode == "f":
            k = min(n, int(rng.choice([1023, 1024, 1025, 1500])))
            variants = [(k, False), (k, True)]
        out = []
        for v in variants:
            do, d_bytes = destinations(rng, mode, n, nbytes, esz, v)
            out.append(dict(kind=kind, op=op, n=n, nbytes=nbytes, mode=mode, variant=v, so=so + np.uint64(s_off),
                            do=do + np.uint64(d_off), s_off=s_off, d_off=d_off, d_bytes=d_bytes + d_off,
                            host_src=host_src, host_dst=host_dst, alpha=alpha, fill=len(self.log) + len(out)))
        return out


def describe(c):
    return dict(kind=c["kind"], op=C.NAMES[c["op"]], n=c["n"], nbytes=c["nbytes"], mode=c["mode"], variant=c["variant"],
                s_off=c["s_off"], d_off=c["d_off"], host_src=c["host_src"], host_dst=c["host_dst"], alpha=c["alpha"])


def same(got, want, c):
    if c["kind"] != "acc":
        return np.array_equal(got, want)
    ph = c["d_off"] % np.dtype(C.REAL[c["op"]]).itemsize   # compare from the elements' phase: NaNs seen whole
    return np.array_equal(got[:ph], want[:ph]) and same_bits_nan_aware(got[ph:], want[ph:], c["op"])


def mismatch(got, want, c):
    if c["kind"] != "acc":
        bad = np.nonzero(got != want)[0]
        return f"{bad.size} bytes differ, first at {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"
    ph = c["d_off"] % np.dtype(C.REAL[c["op"]]).itemsize
    return first_mismatch(got[ph:], want[ph:], c["op"])


def run_case(L, oracle, c, seed=None, twice=False):
    """One case through the library: the bytes against the oracle and the path counters
    against predict(), with the default tuning; once more after a deferral, or when
    `twice` (the oracle applied twice); and, for acc / put of up to 2^19 + 1 pairs, again
    with iov_lds=0."""
    kind, op, n, nbytes = c["kind"], c["op"], c["n"], c["nbytes"]
    so, do, d_bytes = c["so"], c["do"], c["d_bytes"]
    s_bytes = int(so.max()) + nbytes
    src_h = big_fill(op, s_bytes, c["s_off"], 50 + c["fill"])
    dst_h = big_fill(op, d_bytes, c["d_off"], 60 + c["fill"])
    sb = None if c["host_src"] else ga_amd.DeviceBuffer(s_bytes)
    db = None if c["host_dst"] else ga_amd.DeviceBuffer(d_bytes)
    dst_g = dst_h.copy() if c["host_dst"] else None     # what the library writes when host_dst
    what = describe(c)
    try:
        if sb:
            sb.upload(src_h)
        s_base = sb.ptr if sb else src_h.ctypes.data
        d_base = db.ptr if db else dst_g.ctypes.data
        if kind == "acc":
            keep, sp = ga_amd.scale_buffer(op, c["alpha"])
            # W the launcher's way, from the listed device addresses (a property of the draw)
            addr_or = np.bitwise_or.reduce(do + np.uint64(d_base))
            if sb:
                addr_or |= np.bitwise_or.reduce(so + np.uint64(s_base))
            W, widest = launcher_width(op, nbytes, addr_or)
            assert W >= 4, what                          # never the library's -8 refusal
            c["reduced"] = W < C.ESZ[op] or W < widest

        def call():
            g = _giov(so + np.uint64(s_base), do + np.uint64(d_base), nbytes)
            p0 = ga_amd.iov_path_counts()
            if kind == "acc":
                rc = L.comex_accv(op, sp, ctypes.byref(g), 1, 0, 0)
            elif kind == "put":
                rc = L.comex_putv(ctypes.byref(g), 1, 0, 0)
            else:
                rc = L.comex_getv(ctypes.byref(g), 1, 0, 0)
            assert rc == 0, what
            ga_amd.comex_fence_all()
            p1 = ga_amd.iov_path_counts()
            return {k: int(p1[k] - p0[k]) for k in PATHS}

        def apply_oracle(want):
            sa, da = so + np.uint64(src_h.ctypes.data), do + np.uint64(want.ctypes.data)
            if kind == "acc":
                oracle.accv(op, c["alpha"], sa, da, nbytes)
            else:
                oracle.copyv(sa, da, nbytes)

        zero = dict.fromkeys(PATHS, 0)
        expect = zero if c["host_dst"] else predict(n, nbytes, do, 1)
        if db:
            db.upload(dst_h)
        delta = call()
        got = dst_g if c["host_dst"] else db.download(np.uint8, d_bytes)
        want = dst_h.copy()
        apply_oracle(want)
        assert delta == expect, (what, "path counters", delta, expect)
        assert same(got, want, c), (what, mismatch(got, want, c))
        c["delta"] = delta
        if twice or (expect["lds"] and expect["radix"]):
            # after a deferral the same call again: the partition counters were left at zero
            delta2 = call()
            got2 = db.download(np.uint8, d_bytes)
            apply_oracle(want)
            assert delta2 == expect, (what, "path counters, second call", delta2, expect)
            assert same(got2, want, c), (what, "second call", mismatch(got2, want, c))
        c["delta0"] = None
        if kind != "get" and n <= HASH_MAX_PAIRS + 1:
            expect0 = predict(n, nbytes, do, 0)
            want0 = dst_h.copy()
            apply_oracle(want0)
            db.upload(dst_h)
            old = ga_amd.set_tuning("iov_lds", 0)
            try:
                delta0 = call()
            finally:
                ga_amd.set_tuning("iov_lds", old)
            got0 = db.download(np.uint8, d_bytes)
            assert delta0 == expect0, (what, "path counters, iov_lds=0", delta0, expect0)
            assert same(got0, want0, c), (what, "iov_lds=0", mismatch(got0, want0, c))
            assert same(got0, got, c), (what, "iov_lds=0 against iov_lds=1", mismatch(got0, got, c))
            c["delta0"] = delta0
    finally:
        if sb:
            sb.free()
        if db:
            db.free()
    if seed is not None:
        seed.log.append(what)
        if kind == "acc":
            seed.acc += 1
            seed.acc_reduced += bool(c["reduced"])
        seed.seen |= coverage(c)


def coverage(c):
    """which of the per-seed guarantees a finished case provides"""
    tags, d, d0, n = set(), c["delta"], c["delta0"], c["n"]
    only = lambda dd, *keys: all(dd[k] == (1 if k in keys else 0) for k in PATHS)
    if only(d, "lds"):
        tags.add("lds alone below 1024" if n < LDS_ROUTE else "lds alone from 1024")
    if only(d, "lds", "radix"):
        tags.add("lds+radix")
    if only(d, "radix") and n > PART_MAX:
        tags.add("radix alone above 2^22")
    if d0 and only(d0, "hashed"):
        tags.add("hashed")
    if d0 and only(d0, "hashed_then_radix"):
        tags.add("hashed_then_radix")
    if c["host_src"] and n >= HOST_POOL_MIN:
        tags.add("host source of at least 131072 pairs")
    if only(d) and not c["host_dst"]:
        tags.add("no counter")
    return tags


# a fixed case for each guarantee the draws of a seed may miss
FIXED = {
    "lds alone below 1024": dict(n=500, kind="acc", mode="e", op=C.DBL, nbytes=8, host_src=False),
    "lds alone from 1024": dict(n=5000, kind="acc", mode="d", op=C.FLT, nbytes=4, host_src=False),
    "lds+radix": dict(n=100001, kind="acc", mode="e", op=C.DBL, nbytes=8, host_src=False),
    "radix alone above 2^22": dict(n=PART_MAX + 1, kind="acc", mode="d", op=C.DBL, nbytes=8, host_src=False),
    "hashed": dict(n=5000, kind="put", mode="c", nbytes=8, host_src=False),
    "hashed_then_radix": dict(n=20000, kind="acc", mode="e", op=C.DCP, nbytes=16, host_src=False),
    "host source of at least 131072 pairs": dict(n=HOST_POOL_MIN, kind="put", mode="d", nbytes=8, host_src=True),
    "no counter": dict(n=3000, kind="acc", mode="a", op=C.DBL, nbytes=24, host_src=False),
}


def guarantee(L, oracle, S, wanted):
    for tag in wanted:
        if tag not in S.seen:
            for c in S.make(**FIXED[tag]):
                run_case(L, oracle, c, S)
    missing = [t for t in wanted if t not in S.seen]
    assert not missing, (missing, S.log)


def schedule_sizes(seed):
    """the sizes of one seed: (those of the thresholds id, the 2^22-class size); one rng
    for both ids so that the seed's pair budget covers them together"""
    rng = np.random.default_rng(6100 + seed + SEED)
    classes = [(1, 2, 63, 64, 65), (1023, 1024, 1025), (2047, 2048, 2049), (16383, 16384, 16385),
               (65535, 65536, 65537), (131071, 131072, 131073), (524287, 524288, 524289), (528383, 528384)]
    sizes = [int(rng.choice(cl)) for cl in classes]
    big = int(rng.choice(BIG))
    total = sum(sizes) + big
    for _ in range(4):
        n = max(1, int(np.exp(rng.uniform(0, np.log(N_MAX)))))
        while total + n > PAIR_BUDGET:      # redrawn until the seed fits its budget
            n = max(1, int(np.exp(rng.uniform(0, np.log(N_MAX)))))
        sizes.append(n)
        total += n
    assert total <= PAIR_BUDGET
    return [sizes[i] for i in rng.permutation(len(sizes))], big


@pytest.fixture
def lds_default():
    """the default route (iov_lds=1) whatever an earlier test left, restored afterwards"""
    old = ga_amd.set_tuning("iov_lds", 1)
    yield
    ga_amd.set_tuning("iov_lds", old)


# ---------------------------------------------------------------------------------------
# fixed boundary cases
BOUNDARY_OPS = ((C.DBL, 8, 0), (C.DCP, 48, 0), (C.FLT, 16, 4))   # (op, pair bytes, base offset of both sides)


def boundary_case(rng, op, nbytes, off, n, k, repeated, fill):
    keys, slots = loaded_partition(rng, n, k, repeated)
    return dict(kind="acc", op=op, n=n, nbytes=nbytes, mode="f", variant=(k, repeated),
                so=rng.permutation(n).astype(np.uint64) * np.uint64(nbytes) + np.uint64(off),
                do=keys * np.uint64(nbytes) + np.uint64(off), s_off=off, d_off=off, d_bytes=slots * nbytes + off,
                host_src=False, host_dst=False, alpha=C.SCALE[op], fill=fill)


@pytest.mark.parametrize("n,k", [(n, k) for n in (65536, 65537) for k in (1023, 1024, 1025)] + [(4096, 4096)])
def test_partition_bucket_boundary(gpu_lib, oracle, lds_default, n, k):
    """One partition of exactly k = 1023 / 1024 / 1025 entries (k distinct keys, and one
    key k times), every other pair in partitions far below their bucket, at 65536 pairs
    (an overflowed partition is applied in input windows, silently) and 65537 (it is
    deferred to the masked radix pass: `radix` moves, only for k = 1025): DBL 8-byte
    pairs, DCP 48-byte pairs, FLT 16-byte pairs at base + 4 (W = 4).  Every call is made a
    second time and compared with the oracle applied twice (a partition counter not back
    at zero shows there).  n = k = 4096: every pair in one partition, the windowed branch
    with windows that match fully."""
    rng = np.random.default_rng(4100 + n + k)
    fill = 0
    for op, nbytes, off in BOUNDARY_OPS:
        for repeated in ((False,) if k == n else (False, True)):
            c = boundary_case(rng, op, nbytes, off, n, k, repeated, fill)
            fill += 1
            lg = part_lg(n)
            counts = np.bincount(part_of((c["do"] // np.uint64(nbytes)).astype(np.uint32), lg), minlength=1 << lg)
            assert counts.max() == k and np.count_nonzero(counts > 512) == 1, "the case is the one it claims to be"
            run_case(gpu_lib, oracle, c, twice=True)
            defers = n == 65537 and k == 1025
            assert c["delta"] == dict(hashed=0, hashed_then_radix=0, radix=int(defers), lds=1), (n, k, c["delta"])
            if op == C.FLT:
                assert c["reduced"], "16-byte float pairs at base + 4: W = 4"


@pytest.mark.parametrize("op", [C.DBL, C.CPL], ids=lambda o: C.NAMES[o])
def test_hashed_conflict_boundary(gpu_lib, oracle, lds_default, op):
    """The hashed path (iov_lds=0) at its conflict list's capacity, 20000 pairs of 8
    bytes: 4096 destinations named twice each at random positions are exactly 8192
    conflicting pairs, ordered in LDS (`hashed`); one more pair on one of them, 8193, and
    the list overflows into the masked radix pass (`hashed_then_radix`)."""
    n, nbytes = 20000, 8
    rng = np.random.default_rng(4200 + op)
    distinct = rng.permutation(8 * n)[: n - 4096].astype(np.uint64)
    keys = np.concatenate([distinct[:4096], distinct])[rng.permutation(n)]
    single = np.nonzero(np.isin(keys, distinct[4096:]))[0]
    for extra, path in ((0, "hashed"), (1, "hashed_then_radix")):
        if extra:
            keys = keys.copy()
            keys[single[0]] = distinct[7]           # a pair into a triple
        c = dict(kind="acc", op=op, n=n, nbytes=nbytes, mode="hash", variant=extra,
                 so=rng.permutation(n).astype(np.uint64) * np.uint64(nbytes), do=keys * np.uint64(nbytes), s_off=0,
                 d_off=0, d_bytes=8 * n * nbytes, host_src=False, host_dst=False, alpha=C.SCALE[op], fill=extra)
        run_case(gpu_lib, oracle, c)
        assert c["delta0"] == {**dict.fromkeys(PATHS, 0), path: 1}, (extra, c["delta0"])


# ---------------------------------------------------------------------------------------
# the seeded fuzz
@pytest.mark.parametrize("seed", range(6))
def test_random_io_vectors_thresholds(gpu_lib, oracle, lds_default, seed):
    """A fixed schedule of size classes either side of every routing threshold (see the
    module docstring), the value within a class, the kind (acc, acc, put, get), op, alpha,
    pair size, destination mode (a-g), source side and both base offsets drawn by the
    seed; one case at 256 bytes and one at 257-320 (kIovRunsMaxBytes).  Every case: bytes
    and exact counter deltas (run_case).  Afterwards the seed asserts the routes it
    covered (a fixed case is appended for any its draws missed) and that at least a fifth
    of its acc cases ran below the widest vector.  The seed's 2^22-class size is
    test_random_io_vectors_4mi's."""
    sizes, _ = schedule_sizes(seed)
    S = Seed(np.random.default_rng(6300 + seed + SEED))
    for n in sizes:
        for c in S.make(n):
            run_case(gpu_lib, oracle, c, S)
    # the edges of kIovRunsMaxBytes: 256 bytes is ordered on the GPU, 257-320 host-checked
    rng = S.rng
    wide = 8 * int(rng.integers(33, 41)) if seed % 2 else 257 + int(rng.integers(0, 64))
    for nbytes, kind in ((256, ("acc", "put")[seed % 2]), (wide, ("put", "acc")[seed % 2])):
        n = int(np.exp(rng.uniform(np.log(64), np.log(4096))))
        for c in S.make(n, kind=kind, mode="d", nbytes=nbytes, op=C.DBL):
            run_case(gpu_lib, oracle, c, S)
    guarantee(gpu_lib, oracle, S, [t for t in FIXED if t != "radix alone above 2^22"])
    assert 5 * S.acc_reduced >= S.acc, (S.acc_reduced, S.acc)


@pytest.mark.parametrize("seed", range(6))
def test_random_io_vectors_4mi(gpu_lib, oracle, lds_default, seed):
    """The seed's 2^22-class case (2^22 - 1, 2^22, 2^22 + 1 or 2^22 + 1024 pairs: the last
    size of the partitioned path and the first of radix only), an id of its own for its
    run time; the seed's guarantee of `radix` alone above 2^22 pairs is asserted here."""
    _, big = schedule_sizes(seed)
    S = Seed(np.random.default_rng(6400 + seed + SEED))
    S.k = int(S.rng.integers(0, 4))
    for c in S.make(big):
        run_case(gpu_lib, oracle, c, S)
    guarantee(gpu_lib, oracle, S, ["radix alone above 2^22"])
    assert 5 * S.acc_reduced >= S.acc, (S.acc_reduced, S.acc)


# ---------------------------------------------------------------------------------------
# getv into repeated pageable host destinations
def numbered_pairs(n, nbytes):
    """n pairs of nbytes whose bytes encode the pair's index"""
    w = nbytes // 8
    i = np.arange(n, dtype=np.uint64)
    out = np.empty((n, w), dtype=np.uint64)
    for j in range(w):
        out[:, j] = i ^ np.uint64(j * 0x0101010101010101)
    return out.reshape(-1).view(np.uint8)


def repeated_slots(layout, n):
    """mirror: n / 2 slots, slot s named by pair s and by pair n - 1 - s, so each slot's
    last writer sits at the mirrored position of its first (around the middle of the list
    the first is at the END of one range of a split scatter and the last at the START of
    the next); hot: slot i mod 64"""
    i = np.arange(n, dtype=np.uint64)
    if layout == "mirror":
        return np.where(i < n // 2, i, np.uint64(n - 1) - i), n // 2
    return i % np.uint64(64), 64


@pytest.mark.parametrize("nbytes", [8, 24])
@pytest.mark.parametrize("n", [131072, 1 << 20, 1 << 22])
def test_getv_repeated_host_destinations(gpu_lib, oracle, lds_default, n, nbytes):
    """comex_getv from HBM into ONE pageable host buffer whose slots are each named by
    several pairs, at sizes where the host passes run on the pool (two threads from
    131072 pairs): every slot must hold its highest-indexed pair's bytes, the outcome of
    the reference's pair-by-pair loop (comex.c:7327-7400), whatever the threads' timing.
    A scatter split over threads by ranges of the list gets the slots around the middle
    of the mirror layout wrong.  Then the mirror image, comex_putv from pageable host
    sources into repeated device destinations (ordered on the GPU).
    iov.cpp scatters on the pool only when the destinations are one contiguous vector in
    pair order, else on one thread; with the scatter of any list split over the pool all
    six ids failed on the mirror layout (27341 of 65536 slots at 131072 pairs of 8 bytes,
    1075264 of 2097152 at 2^22 pairs: the earlier pair's bytes)."""
    src = numbered_pairs(n, nbytes)
    so = np.arange(n, dtype=np.uint64) * np.uint64(nbytes)
    zero = dict.fromkeys(PATHS, 0)
    sb = ga_amd.DeviceBuffer(src.size)
    try:
        sb.upload(src)
        for layout in ("mirror", "hot"):
            slot, slots = repeated_slots(layout, n)
            do = slot * np.uint64(nbytes)
            host = np.zeros(slots * nbytes, dtype=np.uint8)
            g = _giov(so + np.uint64(sb.ptr), do + np.uint64(host.ctypes.data), nbytes)
            p0 = ga_amd.iov_path_counts()
            assert gpu_lib.comex_getv(ctypes.byref(g), 1, 0, 0) == 0
            ga_amd.comex_fence_all()
            p1 = ga_amd.iov_path_counts()
            want = np.zeros_like(host)
            oracle.copyv(so + np.uint64(src.ctypes.data), do + np.uint64(want.ctypes.data), nbytes)
            last = n - 1 - np.arange(slots) if layout == "mirror" else n - 64 + np.arange(slots)
            assert np.array_equal(want.view(np.uint64)[:: nbytes // 8], last.astype(np.uint64)), "the oracle: last pair wins"
            bad = np.nonzero((host != want).reshape(slots, nbytes).any(axis=1))[0]
            assert bad.size == 0, (layout, f"{bad.size} of {slots} slots differ, first slot {bad[0]}: holds pair "
                                   f"{host.view(np.uint64)[bad[0] * (nbytes // 8)]}, want pair {last[bad[0]]}")
            assert {k: int(p1[k] - p0[k]) for k in PATHS} == zero, layout
            # the mirror image: host sources into repeated device destinations
            db = ga_amd.DeviceBuffer(slots * nbytes)
            try:
                db.upload(np.zeros(slots * nbytes, dtype=np.uint8))
                g = _giov(so + np.uint64(src.ctypes.data), do + np.uint64(db.ptr), nbytes)
                p0 = ga_amd.iov_path_counts()
                assert gpu_lib.comex_putv(ctypes.byref(g), 1, 0, 0) == 0
                ga_amd.comex_fence_all()
                p1 = ga_amd.iov_path_counts()
                assert np.array_equal(db.download(np.uint8, slots * nbytes), want), ("putv", layout)
                assert {k: int(p1[k] - p0[k]) for k in PATHS} == predict(n, nbytes, do, 1), ("putv", layout)
            finally:
                db.free()
    finally:
        sb.free()
