"""Entry-by-entry audit of the k-mer keyed, minimiser-bucketed table (DeviceIndex::ktab) against a model of its own.

Three pieces, numpy only, no GPU:

`ktab_home_model` restates ktab_home (shark_amd/csrc/kmer_device.hpp): where a canonical k-mer lives and the word its slot is
compared with; `slot_key` is its inverse, (a slot's high word, the bucket it sits in) -> the key.  tests/test_ktab_audit.py pins the
model to the header through bin/shark-ktab-check.

`build_image` is the builder of ktab_build_kernel (index_build.hip) done serially, for an insertion order of the caller's choice:
the images it makes are what the auditor is tried on, whole and with single corruptions.

`audit_ktab` takes the array and the scalars as shk_debug_index_array("ktab" / "ktmeta") returns them and the expected key set --
every canonical k-mer whose filter bit is set, from the oracle's filter words (pyoracle.filter_sweep), with the low word each must
carry (index_audit.expected_low) -- and returns (violations, statistics).  A violation is a string "ktab[slot]: ..." in
index_audit's style.  Exact where the content is determined (which keys, their low words, the marks), invariants where the order of
the build's atomic operations is free (which slot of its path a key sits in)."""
import numpy as np

from tests.index_audit import TAB_OVERFLOW, _report
from tests.repeat_refs import KTAB_C1

KTAB_C2 = 0x85EBCA6B
KTAB_PATH = 64               # buckets on a key's path: home, home + one line, ..., home + 63 lines
_U = np.uint64


def revcompl(x, k):
    """so_revcompl (kmer_utils.hpp:47-55) for an array of k-mers"""
    x = ~np.asarray(x, dtype=np.uint64)
    rc = np.zeros(len(x), dtype=np.uint64)
    for _ in range(k):
        rc = (rc << _U(2)) | (x & _U(3))
        x = x >> _U(2)
    return rc


def wmer_hashes(kmers, k, w):
    """per k-mer the hashes of its k - w + 1 canonical w-mers (repeat_refs.wmer_hash of each), one column per w-mer"""
    fwd = np.asarray(kmers, dtype=np.uint64)
    rc = revcompl(fwd, k)
    wmask = _U((1 << (2 * w)) - 1)
    nw = k - w
    cols = []
    for i in range(nw + 1):
        a = (fwd >> _U(2 * (nw - i))) & wmask        # w-mer i from the left of fwd ...
        b = (rc >> _U(2 * i)) & wmask                # ... and its reverse complement, w-mer i from the right of rc
        cols.append((np.minimum(a, b) * _U(KTAB_C1)) & _U(0xFFFFFFFF))
    return np.stack(cols, axis=1)


def _image(key, k):
    """the bijection of ktab_home on a key's low 32 bits: the top three bases xored into the last three, then the upper of those
    six bits into the lower"""
    lo = (key & _U(0xFFFFFFFF)) ^ ((key >> _U(2 * k - 6)) & _U(63))
    return lo ^ ((lo >> _U(3)) & _U(7))


def ktab_home_model(keys, k, w, line_lg):
    """(bucket, want) of ktab_home for an array of k-mers (either strand: the canonical form is the key), 6 <= k <= 17, w <= 15,
    k - w <= 3"""
    assert 6 <= k <= 17 and 1 <= w <= min(k, 15) and k - w <= 3 and 1 <= line_lg <= 28
    fwd = np.asarray(keys, dtype=np.uint64)
    key = np.minimum(fwd, revcompl(fwd, k))
    mh = wmer_hashes(fwd, k, w).min(axis=1)
    line = ((mh * _U(KTAB_C2)) & _U(0xFFFFFFFF)) >> _U(32 - line_lg)
    lo = _image(key, k)
    bucket = (line << _U(3)) | (lo & _U(7))
    want = (((((key >> _U(32)) << _U(29)) | (lo >> _U(3))) << _U(1)) | _U(1)) & _U(0xFFFFFFFF)
    return bucket.astype(np.int64), want.astype(np.int64)


def slot_key(hi, bucket, k):
    """the inverse: the key a slot with high word `hi` in bucket `bucket` stands for (any value; it need not be a k-mer)"""
    hi = np.asarray(hi, dtype=np.uint64)
    lo = (((hi >> _U(1)) & _U(0x1FFFFFFF)) << _U(3)) | (np.asarray(bucket, dtype=np.uint64) & _U(7))
    lo = lo ^ ((lo >> _U(3)) & _U(7))                          # (bits 3-5 are their own: the step is its own inverse)
    pre = (((hi >> _U(30)) & _U(3)) << _U(32)) | lo            # the key but for its last three bases
    return pre ^ ((pre >> _U(2 * k - 6)) & _U(63))             # (2k - 6 >= 6: the top three bases are already the key's)


def line_lg_rule(n_set, bf_bits, k, load=0.09):
    """the builder's sizing (index_build.hip): the smallest table of at least 2^6 lines that holds the expected keys -- the set
    bits' own k-mers and the filter's false positives among the other canonical k-mers -- at `load`"""
    est = n_set + 0.5 * 4.0 ** k * (n_set / bf_bits)
    line_lg = 6
    while line_lg < 28 and (16 << line_lg) * load < est:
        line_lg += 1
    return line_lg


def build_image(keys, low, k, w, line_lg, order=None):
    """ktab_build_kernel done serially: the keys (canonical k-mers) go in one after the other, in `order` (indices into keys;
    default: as given), each into the first free slot of home, home + one line, ... (at most 63 steps, wrapping behind the last
    line); a key placed behind its home marks slot 0 of the home.  -> (ktab as allocated: 16 spare slots at the end, ktmeta)"""
    keys = np.asarray(keys, dtype=np.uint64)
    low = np.asarray(low, dtype=np.uint64)
    bucket, want = ktab_home_model(keys, k, w, line_lg)
    nb = 8 << line_lg
    slots = [0] * (2 * nb + 16)
    entry = ((want.astype(np.uint64) << _U(32)) | (low & _U(0xFFFFFFFF) & ~_U(TAB_OVERFLOW))).tolist()
    home = bucket.tolist()
    for i in (range(len(keys)) if order is None else np.asarray(order).tolist()):
        b = home[i]
        for d in range(KTAB_PATH):
            s = 2 * b if slots[2 * b] == 0 else (2 * b + 1 if slots[2 * b + 1] == 0 else -1)
            if s >= 0:
                slots[s] = entry[i]
                if d:
                    slots[2 * home[i]] |= TAB_OVERFLOW
                break
            b = (b + 8) & (nb - 1)
        else:
            raise AssertionError("build_image: key %d finds no place on its path" % int(keys[i]))
    return np.array(slots, dtype=np.uint64), {"ktab_lg": line_lg + 3, "ktab_w": w, "ktab_keys": len(keys)}


def stored_keys(ktab, ktmeta, k):
    """the keys of the occupied slots (taken bit set), decoded: (slot indices, keys)"""
    nb = 1 << ktmeta["ktab_lg"]
    hi = ktab[:2 * nb] >> _U(32)
    idx = np.flatnonzero((hi & _U(1)) != 0)
    return idx, slot_key(hi[idx], idx >> 1, k)


def audit_ktab(ktab, ktmeta, k, keys, low, complete, must=None):
    """ktab / ktmeta: the array and the scalars (ktab_lg, ktab_w, ktab_keys) as read back.  keys: the expected keys, canonical
    k-mers in ascending order, each once; low: the low word each must carry (overflow mark aside); complete: the x-ranges
    [(lo, hi), ...] over which `keys` holds EVERY key there is; must: optionally a flag per key -- it must be stored wherever it
    lies (the reference's own k-mers).  Every stored key has to be in `keys` in any case.  -> (violations, statistics)"""
    out = []
    ktab = np.asarray(ktab, dtype=np.uint64)
    keys = np.asarray(keys, dtype=np.uint64)
    low = np.asarray(low, dtype=np.int64)
    lg, w, n_keys = ktmeta["ktab_lg"], ktmeta["ktab_w"], ktmeta["ktab_keys"]
    stats = {"keys": 0, "displaced": 0, "longest_path": 0, "wrapped": 0, "palindromic": 0, "above_2_32": 0}
    if lg < 4 or not (6 <= k <= 17 and 1 <= w <= min(k, 15) and k - w <= 3):
        return ["ktab[0]: no table to audit (ktab_lg %d, w %d, k %d)" % (lg, w, k)], stats
    line_lg = lg - 3
    n_lines, nb = 1 << line_lg, 8 << line_lg
    if len(ktab) != (16 << line_lg) + 16:
        return ["ktab[0]: %d slots for ktab_lg %d, expected %d" % (len(ktab), lg, (16 << line_lg) + 16)], stats
    if len(keys) > 1 and not (keys[1:] > keys[:-1]).all():
        raise ValueError("audit_ktab: the expected keys are not ascending and distinct")
    body = ktab[:2 * nb]
    _report(out, "ktab", ktab[2 * nb:] != 0, lambda i: "spare bucket holds %#x" % int(ktab[2 * nb + i]), np.arange(2 * nb, 2 * nb + 16))
    hi = (body >> _U(32)).astype(np.int64)
    lo = (body & _U(0xFFFFFFFF)).astype(np.int64)
    taken = (hi & 1) != 0
    _report(out, "ktab", ~taken & (body != 0), lambda i: "%#x in a slot without the taken bit" % int(body[i]))
    # ---- slot decoding ----
    idx = np.flatnonzero(taken)
    bkt = idx >> 1
    key = slot_key(hi[idx], bkt, k)
    rc = revcompl(key, k)
    is_kmer = key < _U(1 << (2 * k))
    canon = is_kmer & (key <= rc)
    _report(out, "ktab", ~is_kmer, lambda i: "key %#x is no %d-mer" % (int(key[i]), k), idx)
    _report(out, "ktab", is_kmer & ~canon, lambda i: "key %d is not canonical (its reverse complement %d is)" % (int(key[i]), int(rc[i])), idx)
    ok = np.flatnonzero(canon)                                  # what follows is said of the slots that decode to a canonical k-mer
    idx, bkt, key = idx[ok], bkt[ok], key[ok]
    home, want = ktab_home_model(key, k, w, line_lg)
    _report(out, "ktab", want != hi[idx], lambda i: "high word %#x, key %d has %#x" % (hi[idx[i]], int(key[i]), want[i]), idx)
    _report(out, "ktab", (home & 7) != (bkt & 7), lambda i: "key %d belongs in bucket %d of a line, not %d" % (int(key[i]), home[i] & 7, bkt[i] & 7), idx)
    d = ((bkt >> 3) - (home >> 3)) & (n_lines - 1)
    _report(out, "ktab", d >= KTAB_PATH, lambda i: "key %d sits %d lines behind its home line %d" % (int(key[i]), d[i], home[i] >> 3), idx)
    # ---- no key twice; as many as the builder counted ----
    order = np.argsort(key, kind="stable")
    ks = key[order]
    dup = np.flatnonzero(ks[1:] == ks[:-1]) + 1
    _report(out, "ktab", dup, lambda i: "key %d is stored more than once" % int(ks[i]), idx[order])
    if int(taken.sum()) != n_keys:
        out.append("ktab[0]: %d occupied slots, ktab_keys says %d" % (int(taken.sum()), n_keys))
    # ---- soundness: every stored key is an expected one, with its low word ----
    r = np.searchsorted(keys, key)
    known = (r < len(keys)) & (keys[np.minimum(r, max(len(keys) - 1, 0))] == key) if len(keys) else np.zeros(len(key), bool)
    _report(out, "ktab", ~known, lambda i: "key %d is not a canonical k-mer whose filter bit is set" % int(key[i]), idx)
    got, exp = lo[idx[known]] & ~TAB_OVERFLOW, low[r[known]]
    _report(out, "ktab", got != exp, lambda i: "low word %#x, expected %#x (key %d)" % (got[i], exp[i], int(key[known][i])), idx[known])
    # ---- completeness: inside the ranges known exhaustively, and the flagged keys wherever they lie ----
    have = np.zeros(len(keys), dtype=bool)
    have[r[known]] = True
    need = np.zeros(len(keys), dtype=bool) if must is None else np.asarray(must, dtype=bool).copy()
    whole = False
    for x_lo, x_hi in complete:
        need |= (keys >= _U(x_lo)) & (keys < _U(min(x_hi, 1 << (2 * k))))
        whole |= x_lo == 0 and x_hi >= 1 << (2 * k)
    if len(keys):
        khome, _ = ktab_home_model(keys, k, w, line_lg)
        _report(out, "ktab", need & ~have, lambda i: "key %d (home bucket %d) is not stored" % (int(keys[i]), khome[i]), 2 * khome)
    if whole and n_keys != len(keys):
        out.append("ktab[0]: ktab_keys %d, the filter has %d canonical k-mers" % (n_keys, len(keys)))
    # ---- path: a displaced key passed only buckets without a free slot (a free slot ends every search) ----
    full = (hi[0::2] != 0) & (hi[1::2] != 0)
    dd = np.minimum(d, KTAB_PATH - 1)
    bad = np.zeros(len(key), dtype=bool)
    for j in range(int(dd.max()) if len(dd) else 0):
        on = dd > j
        bad[on] |= ~full[(home[on] + 8 * j) & (nb - 1)]
    _report(out, "ktab", bad, lambda i: "key %d, displaced by %d lines, passed a bucket with a free slot (home bucket %d)" % (int(key[i]), d[i], home[i]), idx)
    # ---- marks: slot 0 of exactly the buckets that are the home of a displaced key ----
    wantm = np.zeros(nb, dtype=bool)
    wantm[home[(d > 0) & (d < KTAB_PATH)]] = True
    gotm = (lo[0::2] & TAB_OVERFLOW) != 0
    _report(out, "ktab", wantm & ~gotm, "overflow mark missing (a key of this home bucket sits further down)", np.arange(nb) * 2)
    _report(out, "ktab", gotm & ~wantm, "overflow mark without a displaced key of this home bucket", np.arange(nb) * 2)
    _report(out, "ktab", (lo[1::2] & TAB_OVERFLOW) != 0, "overflow mark in slot 1", np.arange(nb) * 2 + 1)
    _report(out, "ktab", (hi == 0) & ((lo & TAB_OVERFLOW) != 0), "overflow mark in a slot whose high word is zero")
    stats.update(keys=int(taken.sum()), displaced=int((d > 0).sum()), longest_path=int(d.max()) if len(d) else 0,
                 wrapped=int(((home >> 3) + d >= n_lines).sum()), palindromic=int((key == revcompl(key, k)).sum()),
                 above_2_32=int((key >= _U(1 << 32)).sum()))
    return out, stats
