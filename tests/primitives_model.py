"""Exact host models of the two device primitives -- exclusive_scan_u32 (device_scan.hip) and radix_sort_u64 (device_sort.hip) --
and the case tables that tests/test_gpu_primitives.py runs through SharkHip.debug_scan_u32 / debug_sort_u64.
tests/test_primitives_cpu.py proves the models against plain loops and shows that the tables are sharp (regimes, mutants).

Everything is integer arithmetic: every comparison is exact equality.

How the tables were thinned
---------------------------
Scan.  The full product sizes x values x placements has 14 * 8 * 20 + 5 * 8 * 3 = 2 360 cases; the table keeps 400:
  * sizes up to 2T + 1 (14 of them): every size at every one of the 20 placements (16 out of place, 4 in place), one value kind
    each, value = SCAN_VALUES[(3 * size index + placement index) % 8].  20 placements walk through all 8 kinds at every size and,
    3 being coprime to 8, 14 sizes walk through all 8 kinds at every placement: every (size, value) pair occurs at two or three
    placements and every (placement, value) pair at one or two sizes.  280 cases.
  * the 5 larger sizes: all 8 value kinds at the three placements the issue names (aligned in place, aligned out of place, in 0 /
    out 1).  120 cases.
Sort.  The full product 16 * 11 * 10 has 1 760 cases; the table keeps about 900: at every (size, end_bit) the three kinds that carry
a property of their own -- `random` (all 64 bits), `serial` (stability) and `zero` (padding lanes; only where n is not a multiple
of 64, `equal` covers the rest) -- and of the other seven those with (size index + end_bit index + kind index) % 3 == 0, which puts
every one of them at every size and at every end_bit.
"""
import functools
from collections import namedtuple

import numpy as np

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1

# ---- the kernels' constants (device_scan.hpp, device_scan.hip, device_sort.hpp) ----
SCAN_TILE = 4096
SCAN_ITEMS = 16
SCAN_OFFS_THREADS = 1024
RS_TILE = 4096
RS_THREADS = 256

T = SCAN_TILE
R = RS_TILE


# =====================================================================================================================
# scan
# =====================================================================================================================
def scan_model(a):
    """(out, total): out[i] = sum of a[:i] modulo 2^32, total = the exact sum (a Python int).  Exact while n * 2^32 < 2^64"""
    a = np.asarray(a, dtype=np.uint32)
    if len(a) == 0:
        return np.zeros(0, dtype=np.uint32), 0
    c = np.cumsum(a.astype(np.uint64), dtype=np.uint64)
    return ((c - a) & np.uint64(M32)).astype(np.uint32), int(c[-1])


def scan_loop(a):
    """the same with a plain loop over Python ints"""
    out, run = [], 0
    for v in a.tolist():
        out.append(run & M32)
        run += v
    return np.array(out, dtype=np.uint32), run


def scan_per(n):
    """tiles per thread of scan_tile_offsets_kernel, computed the way the kernel computes it"""
    ntiles = (n + SCAN_TILE - 1) // SCAN_TILE
    return (ntiles + SCAN_OFFS_THREADS - 1) // SCAN_OFFS_THREADS


def scan_vec(case):
    """whether exclusive_scan_u32 takes the vector kernels: in and out both 16-byte aligned"""
    return case.in_off == 0 and case.out_off == 0


SCAN_SIZES_SMALL = (0, 1, 15, 16, 17, 1023, 1024, 1025, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1)
SCAN_SIZES_LARGE = (1023 * T + 5, 1024 * T, 1024 * T + 1, 2048 * T, 2048 * T + 17)
SCAN_VALUES = ("zeros", "ones", "max", "random", "flags", "depth", "straddle", "ramp")
# (in_off, out_off, in_place): the 16 out-of-place pairs, then the 4 in-place ones
SCAN_PLACEMENTS = tuple((i, o, False) for i in range(4) for o in range(4)) + tuple((i, i, True) for i in range(4))
SCAN_PLACEMENTS_LARGE = ((0, 0, True), (0, 0, False), (0, 1, False))

ScanCase = namedtuple("ScanCase", "n values in_off out_off in_place")


def scan_case_name(c):
    return "scan[n=%d %s in+%d %s]" % (c.n, c.values, c.in_off, "in place" if c.in_place else "out+%d" % c.out_off)


def _seed(*parts):
    s = 0x5EED
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % (1 << 31)
    return s


@functools.lru_cache(maxsize=8)
def scan_values(n, kind):
    """the n input words of a value kind (read-only)"""
    rng = np.random.default_rng(_seed("scan", n, kind))
    if kind == "zeros":
        a = np.zeros(n, dtype=np.uint32)
    elif kind == "ones":
        a = np.ones(n, dtype=np.uint32)
    elif kind == "max":                 # outputs wrap in every tile, total = n * (2^32 - 1)
        a = np.full(n, M32, dtype=np.uint32)
    elif kind == "random":
        a = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    elif kind == "flags":               # 0/1 at density 1/7
        a = (rng.integers(0, 7, size=n) == 0).astype(np.uint32)
    elif kind == "depth":
        # a difference array as depth mode builds it: +1 where an interval opens, 2^32 - 1 (that is -1) where it closes, every closing
        # behind its opening, so the running sum never goes below zero.  Interval j opens at a random position and closes at a later one
        a = np.zeros(n, dtype=np.uint32)
        if n >= 2:
            m = max(1, n // 5)
            lo = rng.integers(0, n - 1, size=m)
            hi = lo + 1 + rng.integers(0, 64, size=m)
            hi = np.minimum(hi, n - 1)
            d = np.bincount(lo, minlength=n) - np.bincount(hi, minlength=n)      # openings minus closings per position
            a = (d & M32).astype(np.uint32)                                       # (modulo 2^32: k closings are -k)
    elif kind == "straddle":            # one 0xFFFFFFFF as the last item of a tile, one as the first of the next, the rest 0
        a = np.zeros(n, dtype=np.uint32)
        # the last tile boundary inside the array; arrays of less than a tile plus one item: the boundary between two threads' runs,
        # or the array's two last items
        b = ((n - 1) // SCAN_TILE) * SCAN_TILE if n > SCAN_TILE else ((n - 1) // SCAN_ITEMS) * SCAN_ITEMS if n > SCAN_ITEMS else n - 1
        if n >= 2:
            a[b - 1] = a[b] = M32
        elif n == 1:
            a[0] = M32
    elif kind == "ramp":
        a = (np.arange(n, dtype=np.uint64) % 251).astype(np.uint32)
    else:
        raise KeyError(kind)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=8)
def scan_expected(n, kind):
    """(in, out, total) of a (size, value kind): computed once, shared by every placement, read-only"""
    a = scan_values(n, kind)
    out, total = scan_model(a)
    out.setflags(write=False)
    return a, out, total


def _scan_cases():
    cases = []
    for si, n in enumerate(SCAN_SIZES_SMALL):
        for pi, (io, oo, ip) in enumerate(SCAN_PLACEMENTS):
            cases.append(ScanCase(n, SCAN_VALUES[(3 * si + pi) % len(SCAN_VALUES)], io, oo, ip))
    for n in SCAN_SIZES_LARGE:
        for (io, oo, ip) in SCAN_PLACEMENTS_LARGE:
            for kind in SCAN_VALUES:
                cases.append(ScanCase(n, kind, io, oo, ip))
    return tuple(cases)


SCAN_CASES = _scan_cases()


def scan_groups():
    """the GPU test's parameters: (size class, in_off, out_off, in_place) -> the cases of that group.  Size class 0 = the sizes up
    to 2T + 1 together (one value kind each), every larger size a class of its own (all value kinds)"""
    groups = {}
    for c in SCAN_CASES:
        groups.setdefault((c.n if c.n > 2 * T + 1 else 0, c.in_off, c.out_off, c.in_place), []).append(c)
    return groups


def scan_where(i):
    """where item i of a scan lies: tile, the thread whose 16-item run holds it, that thread's wave and lane, the item within the run"""
    t = (i % SCAN_TILE) // SCAN_ITEMS
    return "tile %d thread-run %d (wave %d lane %d) item %d" % (i // SCAN_TILE, t, t // 64, t % 64, i % SCAN_ITEMS)


def first_diff(expected, actual):
    """index of the first differing element, None when the arrays are equal"""
    if len(expected) != len(actual):
        return min(len(expected), len(actual))
    d = np.flatnonzero(expected != actual)
    return int(d[0]) if len(d) else None


def scan_mismatch(case, what, expected, actual):
    """None when equal, else the message: case, first differing index, where it lies, expected and actual there"""
    i = first_diff(expected, actual)
    if i is None:
        return None
    return "%s: %s differs first at %d of %d (%s): expected 0x%08x, got 0x%08x; %d words differ" % (
        scan_case_name(case), what, i, len(expected), scan_where(i), int(expected[i]), int(actual[i]), int(np.count_nonzero(expected != actual)))


# =====================================================================================================================
# sort
# =====================================================================================================================
def sort_passes(end_bit):
    """passes of the loop `for (shift = 0; shift < end_bit; shift += 8)`"""
    return (end_bit + 7) // 8


def sort_mask(end_bit):
    return (1 << (8 * sort_passes(end_bit))) - 1


def sort_model(keys, end_bit):
    """(ordered keys, buffer): the keys ordered stably by their low 8 * ceil(end_bit / 8) bits; buffer 0 (a) after an even number
    of passes, 1 (b) after an odd one; n == 0 returns a without a pass"""
    keys = np.asarray(keys, dtype=np.uint64)
    if len(keys) == 0:
        return keys.copy(), 0
    order = np.argsort(keys & np.uint64(sort_mask(end_bit)), kind="stable")
    return keys[order], sort_passes(end_bit) & 1


def sort_loop(keys, end_bit):
    """the same as plain loops over Python ints: one stable bucket pass per digit"""
    cur = [int(k) for k in keys]
    if not cur:
        return np.zeros(0, dtype=np.uint64), 0
    buf = 0
    shift = 0
    while shift < end_bit:
        buckets = [[] for _ in range(256)]
        for k in cur:
            buckets[(k >> shift) & 255].append(k)
        cur = [k for b in buckets for k in b]
        buf ^= 1
        shift += 8
    return np.array(cur, dtype=np.uint64), buf


SORT_SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, R - 1, R, R + 1, 2 * R + 1, 3 * R + 100, 17 * R + 1, 300 * R + 77)
SORT_END_BITS = (1, 8, 9, 16, 17, 18, 33, 40, 48, 63, 64)
SORT_KEYS_ALWAYS = ("random", "serial", "zero")
SORT_KEYS_ROTATING = ("equal", "alternating", "ascending", "descending", "lanes", "threads", "index")
SORT_KEYS = SORT_KEYS_ALWAYS + SORT_KEYS_ROTATING

SortCase = namedtuple("SortCase", "n end_bit keys")


def sort_case_name(c):
    return "sort[n=%d end_bit=%d %s]" % (c.n, c.end_bit, c.keys)


_REP = 0x0101010101010101      # a digit in every byte


@functools.lru_cache(maxsize=16)
def sort_keys(n, kind, width):
    """the n keys of a kind for a sort over the low `width` bits (width = 8 * passes; read-only).  Kinds whose point is stability
    carry a running serial number in the bits above `width` (none at width 64): the model leaves those bits in input order"""
    rng = np.random.default_rng(_seed("sort", n, kind, width))
    i = np.arange(n, dtype=np.uint64)
    mask = np.uint64((1 << width) - 1)
    serial = (i << np.uint64(width)) if width < 64 else np.zeros(n, dtype=np.uint64)
    if kind == "equal":                 # every lane of every wave is a peer, one digit takes the whole tile
        k = np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)
    elif kind == "zero":                # the padding lanes hold key 0 as well and must not count as peers
        k = np.zeros(n, dtype=np.uint64)
    elif kind == "alternating":
        k = np.where(i % np.uint64(2) == 0, np.uint64(0xFEDCBA9876543210), np.uint64(0x0000000100000100))
    elif kind == "ascending":
        k = i * np.uint64(2654435761)                  # (below 2^64 for every size of the table)
    elif kind == "descending":
        k = (i * np.uint64(2654435761))[::-1].copy()
    elif kind == "random":
        k = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    elif kind == "serial":              # stability across waves, rows and workgroups
        k = (rng.integers(0, 1 << 17, size=n, dtype=np.uint64) & mask) | serial
    elif kind == "lanes":               # lane l of every wave holds digit l in every pass: 64 distinct digits per wave, no peers
        k = (((i % np.uint64(64)) * np.uint64(_REP)) & mask) | serial
    elif kind == "threads":             # thread t holds digit t in every pass: every digit once per row
        k = (((i % np.uint64(RS_THREADS)) * np.uint64(_REP)) & mask) | serial
    elif kind == "index":               # the index build's keys: rank << 16 | gene, sentinels n_set << 16 single and in one run
        n_set = max(1, n // 3)
        k = (rng.integers(0, n_set, size=n, dtype=np.uint64) << np.uint64(16)) | rng.integers(0, 1 << 16, size=n, dtype=np.uint64)
        sent = rng.integers(0, 9, size=n) == 0
        if n >= 4:
            lo = int(rng.integers(0, n - n // 4))
            sent[lo:lo + n // 4] = True
        k[sent] = np.uint64(n_set << 16)
    else:
        raise KeyError(kind)
    k = np.ascontiguousarray(k, dtype=np.uint64)
    k.setflags(write=False)
    return k


def sort_case_keys(c):
    return sort_keys(c.n, c.keys, 8 * sort_passes(c.end_bit))


def _sort_cases():
    cases = []
    for ei, e in enumerate(SORT_END_BITS):
        for si, n in enumerate(SORT_SIZES):
            for kind in SORT_KEYS_ALWAYS:
                if kind == "zero" and n % 64 == 0:
                    continue
                cases.append(SortCase(n, e, kind))
            for ki, kind in enumerate(SORT_KEYS_ROTATING):
                if (si + ei + ki) % 3 == 0:
                    cases.append(SortCase(n, e, kind))
    return tuple(cases)


SORT_CASES = _sort_cases()


def sort_groups():
    """the GPU test's parameters: end_bit -> its cases"""
    groups = {}
    for c in SORT_CASES:
        groups.setdefault(c.end_bit, []).append(c)
    return groups


def sort_where(i):
    """where position i of a key array lies when a workgroup reads it: tile, row of the tile, wave of the row, lane"""
    r = i % RS_TILE
    return "tile %d row %d wave %d lane %d" % (i // RS_TILE, r // RS_THREADS, (r % RS_THREADS) // 64, r % 64)


def sort_mismatch(case, expected, actual):
    i = first_diff(expected, actual)
    if i is None:
        return None
    return "%s: output differs first at %d of %d (%s): expected 0x%016x, got 0x%016x; %d keys differ" % (
        sort_case_name(case), i, len(expected), sort_where(i), int(expected[i]), int(actual[i]), int(np.count_nonzero(expected != actual)))
