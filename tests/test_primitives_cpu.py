"""CPU proof of tests/primitives_model.py: the models against plain loops, the regimes the case tables were built to reach, and a
fixed list of wrong implementations ("mutants", numpy at the level of results) each of which some case of the table must tell
from the model.  A mutant that no case kills means the table has a hole: the case is added, the mutant stays."""
import numpy as np
import pytest

from tests import primitives_model as pm

T, R = pm.T, pm.R
SMALL = 2 * T + 1


def _scan_pairs():
    """the (size, value kind) pairs of the scan table in table order, each once"""
    seen = []
    for c in pm.SCAN_CASES:
        if (c.n, c.values) not in seen:
            seen.append((c.n, c.values))
    return seen


def test_entry_points_are_exported_and_stay_out_of_the_public_interface():
    import ctypes
    import os
    import subprocess
    import shark_amd
    from shark_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(capi.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(root, "shark_amd", "csrc"), "-j4", "all"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(capi.LIB_PATH)
    header = open(os.path.join(root, "include", "shark_hip.h")).read()
    for name in ("shk_debug_scan_u32", "shk_debug_sort_u64"):
        assert hasattr(lib, name), "libsharkhip.so does not export %s" % name
        assert name not in shark_amd.EXPORTS and name not in header


# ---- models against loops ------------------------------------------------------------------------------------------
def test_scan_model_equals_loop_on_every_small_case():
    checked = 0
    for n, kind in _scan_pairs():
        if n > SMALL:
            continue
        a, out, total = pm.scan_expected(n, kind)
        lout, ltotal = pm.scan_loop(a)
        assert total == ltotal and np.array_equal(out, lout), "scan model differs from the loop at n=%d %s" % (n, kind)
        assert out.dtype == np.uint32 and len(out) == n
        checked += 1
    assert checked == len(pm.SCAN_SIZES_SMALL) * len(pm.SCAN_VALUES)      # the thinning kept every (size, value) pair


def test_sort_model_equals_loop_on_every_small_case():
    loops = {}
    checked = 0
    for c in pm.SORT_CASES:
        if c.n > SMALL:
            continue
        keys = pm.sort_case_keys(c)
        got, buf = pm.sort_model(keys, c.end_bit)
        at = (c.n, c.keys, pm.sort_passes(c.end_bit))      # (keys and passes are all the loop depends on)
        if at not in loops:
            loops[at] = pm.sort_loop(keys, c.end_bit)
        lgot, lbuf = loops[at]
        assert buf == lbuf and np.array_equal(got, lgot), "sort model differs from the loop at %s" % pm.sort_case_name(c)
        checked += 1
    assert checked > 500


def test_depth_values_never_go_negative():
    for n in pm.SCAN_SIZES_SMALL:
        a = pm.scan_values(n, "depth").astype(np.int32).astype(np.int64)      # 2^32 - 1 read as -1
        assert (np.cumsum(a) >= 0).all() and (n < 2 or (a < 0).any())


# ---- the tables ----------------------------------------------------------------------------------------------------
def test_tables_are_complete_and_of_modest_size():
    assert 200 <= len(pm.SCAN_CASES) <= 500
    assert {c.n for c in pm.SCAN_CASES} == set(pm.SCAN_SIZES_SMALL) | set(pm.SCAN_SIZES_LARGE)
    for n in pm.SCAN_SIZES_SMALL:
        assert {(c.in_off, c.out_off, c.in_place) for c in pm.SCAN_CASES if c.n == n} == set(pm.SCAN_PLACEMENTS)
        assert {c.values for c in pm.SCAN_CASES if c.n == n} == set(pm.SCAN_VALUES)
    for p in pm.SCAN_PLACEMENTS:
        assert {c.values for c in pm.SCAN_CASES if (c.in_off, c.out_off, c.in_place) == p and c.n <= SMALL} == set(pm.SCAN_VALUES)
    for n in pm.SCAN_SIZES_LARGE:
        assert {(c.in_off, c.out_off, c.in_place, c.values) for c in pm.SCAN_CASES if c.n == n} == {
            p + (v,) for p in pm.SCAN_PLACEMENTS_LARGE for v in pm.SCAN_VALUES}
    assert len(set(pm.SCAN_CASES)) == len(pm.SCAN_CASES) and len(set(pm.SORT_CASES)) == len(pm.SORT_CASES)
    for e in pm.SORT_END_BITS:
        assert {c.keys for c in pm.SORT_CASES if c.end_bit == e} == set(pm.SORT_KEYS)
        assert {c.n for c in pm.SORT_CASES if c.end_bit == e} == set(pm.SORT_SIZES)
    for n in pm.SORT_SIZES:
        want = set(pm.SORT_KEYS) - ({"zero"} if n % 64 == 0 else set())
        assert {c.keys for c in pm.SORT_CASES if c.n == n} == want
    assert max(pm.SORT_SIZES) < 1 << 32


def test_regimes_reached():
    # the tile-offset kernel's tiles per thread
    assert {pm.scan_per(c.n) for c in pm.SCAN_CASES if c.n} == {1, 2, 3}
    assert pm.scan_per(1024 * T) == 1 and pm.scan_per(1024 * T + 1) == 2 and pm.scan_per(2048 * T) == 2 and pm.scan_per(2048 * T + 17) == 3
    # both kernel paths, out of place and in place, at sizes with whole 16-item runs and a ragged one (n >= 17) and in every `per`
    for vec in (True, False):
        for in_place in (True, False):
            hit = [c for c in pm.SCAN_CASES if pm.scan_vec(c) == vec and c.in_place == in_place and c.n >= 17]
            assert {pm.scan_per(c.n) for c in hit} == ({1, 2, 3} if vec or not in_place else {1}), (vec, in_place)
    assert any(not pm.scan_vec(c) and pm.scan_per(c.n) == 3 for c in pm.SCAN_CASES)
    # a total above 2^32 (already at a small size), and outputs that wrap
    assert pm.scan_expected(15, "max")[2] == 15 * pm.M32 > 1 << 32
    assert any(c.values == "max" and c.n >= 2 for c in pm.SCAN_CASES)
    # both parities of the pass count
    assert {pm.sort_passes(e) & 1 for e in pm.SORT_END_BITS} == {0, 1}
    assert [pm.sort_passes(e) for e in pm.SORT_END_BITS] == [1, 1, 2, 2, 3, 3, 5, 5, 6, 8, 8]
    # a last row with fewer than 64 valid lanes that contains key 0 (the padding lanes beside it hold 0 as well)
    ragged = [c for c in pm.SORT_CASES if 0 < c.n % pm.RS_THREADS < 64 and (pm.sort_case_keys(c)[c.n - c.n % pm.RS_THREADS:] == 0).any()]
    assert ragged and {c.end_bit for c in ragged} == set(pm.SORT_END_BITS)
    assert any(c.n > R for c in ragged)      # ... and one behind full tiles
    # a histogram whose scan has more than one tile
    assert any(256 * -(-c.n // R) > pm.SCAN_TILE for c in pm.SORT_CASES)


def test_mismatch_messages_name_the_place():
    c = pm.ScanCase(2 * T + 1, "ramp", 0, 1, False)
    a, out, _ = pm.scan_expected(c.n, c.values)
    assert pm.scan_mismatch(c, "out", out, out.copy()) is None
    bad = out.copy()
    bad[T + 16 * 65 + 3] ^= 1
    msg = pm.scan_mismatch(c, "out", out, bad)
    assert "n=8193 ramp in+0 out+1" in msg and "at 5139 " in msg and "tile 1 thread-run 65 (wave 1 lane 1) item 3" in msg and "1 words differ" in msg
    s = pm.SortCase(R + 1, 9, "random")
    keys, _ = pm.sort_model(pm.sort_case_keys(s), s.end_bit)
    bad = keys.copy()
    bad[256 * 3 + 64 * 2 + 5] ^= np.uint64(1 << 40)
    msg = pm.sort_mismatch(s, keys, bad)
    assert "n=4097 end_bit=9 random" in msg and "tile 0 row 3 wave 2 lane 5" in msg


# ---- mutants -------------------------------------------------------------------------------------------------------
def _scan_drop_carry(a):
    """tile offsets that drop the carry into tiles numbered 1024 and above"""
    out, total = pm.scan_model(a)
    cut = 1024 * T
    if len(a) > cut:
        out = out.copy()
        out[cut:] = pm.scan_model(a[cut:])[0]
    return out, total


def _scan_total32(a):
    out, total = pm.scan_model(a)
    return out, total & pm.M32


def _scan_saturate(a):
    out, total = pm.scan_model(a)
    if len(a):
        c = np.cumsum(a.astype(np.uint64), dtype=np.uint64) - a
        out = np.minimum(c, np.uint64(pm.M32)).astype(np.uint32)
    return out, total


def _scan_pad_ones(a):
    """items behind n in the last 16-item run taken as 1: they follow every real item, so only the total sees them"""
    out, total = pm.scan_model(a)
    return out, total + (-len(a)) % pm.SCAN_ITEMS


def _scan_inclusive(a):
    out, total = pm.scan_model(a)
    return (out + np.asarray(a, dtype=np.uint32)).astype(np.uint32), total


def _scan_whole_runs_only(a):
    """right only when n is a multiple of 16: the ragged last run is neither read nor written (its outputs stay 0)"""
    whole = len(a) - len(a) % pm.SCAN_ITEMS
    out, total = pm.scan_model(a[:whole])
    return np.concatenate([out, np.zeros(len(a) - whole, dtype=np.uint32)]), total


SCAN_MUTANTS = {
    "carry dropped from tile 1024 on": _scan_drop_carry,
    "32-bit total": _scan_total32,
    "saturating outputs": _scan_saturate,
    "padding items taken as 1": _scan_pad_ones,
    "inclusive scan": _scan_inclusive,
    "right for multiples of 16 only": _scan_whole_runs_only,
}


@pytest.mark.parametrize("name", list(SCAN_MUTANTS))
def test_scan_mutant_is_killed(name):
    mutant = SCAN_MUTANTS[name]
    killer = None
    for n, kind in _scan_pairs():
        a, out, total = pm.scan_expected(n, kind)
        mout, mtotal = mutant(a)
        if mtotal != total or not np.array_equal(mout, out):
            killer = "n=%d %s" % (n, kind)
            break
    assert killer is not None, "no case of the scan table tells the mutant '%s' from the model" % name
    print("scan mutant '%s' killed by %s" % (name, killer))


def emulate_sort(keys, passes, lanes_rev=False, waves_rev=False, rows_rev=False):
    """the pass structure of rs_scatter_kernel at the level of results: per pass the keys go out by (digit, tile, row, wave, lane)
    of their present position; a flag reverses one level among equal digits"""
    cur = np.asarray(keys, dtype=np.uint64)
    i = np.arange(len(cur), dtype=np.int64)
    tile, row, wave, lane = i // R, (i % R) // pm.RS_THREADS, (i % pm.RS_THREADS) // 64, i % 64
    for p in range(passes):
        digit = ((cur >> np.uint64(8 * p)) & np.uint64(255)).astype(np.int64)
        order = np.lexsort((-lane if lanes_rev else lane, -wave if waves_rev else wave, -row if rows_rev else row, tile, digit))
        cur = cur[order]
    return cur, passes & 1


def _sort_pad_peers(keys, end_bit):
    """padding lanes counted as peers of digit 0: the last wave's padding takes part as keys of value 0"""
    pad = (-len(keys)) % 64
    got, buf = pm.sort_model(np.concatenate([keys, np.zeros(pad, dtype=np.uint64)]), end_bit)
    return got[:len(keys)], buf if len(keys) else 0


def _sort_floor_passes(keys, end_bit):
    return emulate_sort(keys, end_bit // 8) if len(keys) else pm.sort_model(keys, end_bit)


def _sort_wrong_buffer(keys, end_bit):
    """after an odd number of passes the result is taken from a, which holds what the pass before left"""
    p = pm.sort_passes(end_bit)
    if len(keys) == 0 or p % 2 == 0:
        return pm.sort_model(keys, end_bit)
    return emulate_sort(keys, p - 1)[0], 0


def _sort_whole_key(keys, end_bit):
    return np.sort(keys, kind="stable"), pm.sort_model(keys, end_bit)[1]


SORT_MUTANTS = {
    "padding lanes are peers of digit 0": _sort_pad_peers,
    "lanes of a wave reversed": lambda k, e: emulate_sort(k, pm.sort_passes(e), lanes_rev=True) if len(k) else pm.sort_model(k, e),
    "waves of a row reversed": lambda k, e: emulate_sort(k, pm.sort_passes(e), waves_rev=True) if len(k) else pm.sort_model(k, e),
    "rows of a tile reversed": lambda k, e: emulate_sort(k, pm.sort_passes(e), rows_rev=True) if len(k) else pm.sort_model(k, e),
    "floor(end_bit / 8) passes": _sort_floor_passes,
    "wrong buffer after an odd number of passes": _sort_wrong_buffer,
    "ordered by the whole key": _sort_whole_key,
}


def test_sort_emulation_without_a_mutation_is_the_model():
    for c in pm.SORT_CASES:
        if c.n > SMALL:
            continue
        keys = pm.sort_case_keys(c)
        got, buf = emulate_sort(keys, pm.sort_passes(c.end_bit)) if c.n else (keys, 0)
        want, wbuf = pm.sort_model(keys, c.end_bit)
        assert buf == wbuf and np.array_equal(got, want), pm.sort_case_name(c)


@pytest.mark.parametrize("name", list(SORT_MUTANTS))
def test_sort_mutant_is_killed(name):
    """the KEYS must differ: a mutant that only names the other buffer would be told apart by any case"""
    mutant = SORT_MUTANTS[name]
    killer = None
    for c in sorted(pm.SORT_CASES, key=lambda c: c.n):
        keys = pm.sort_case_keys(c)
        want, _ = pm.sort_model(keys, c.end_bit)
        got, _ = mutant(keys, c.end_bit)
        if not np.array_equal(got, want):
            killer = pm.sort_case_name(c)
            break
    assert killer is not None, "no case of the sort table tells the mutant '%s' from the model" % name
    print("sort mutant '%s' killed by %s" % (name, killer))


def test_wrong_buffer_is_also_told_by_the_buffer_index():
    for e in pm.SORT_END_BITS:
        keys = pm.sort_keys(65, "random", 8 * pm.sort_passes(e))
        assert (_sort_wrong_buffer(keys, e)[1] != pm.sort_model(keys, e)[1]) == bool(pm.sort_passes(e) & 1)
