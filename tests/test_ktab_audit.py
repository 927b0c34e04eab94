"""The auditor of the minimiser-bucketed table (tests/ktab_audit.py), tried without a GPU: images made by the serial builder pass
for every insertion order, each of fourteen single corruptions is reported with the slot or the key it concerns, one k = 15 case
runs the whole pipeline (oracle-built filter, so_filter_sweep, the builder's own sizing rule, the audit), and the Python model of
ktab_home is pinned to kmer_device.hpp through bin/shark-ktab-check.  k = 9 with 64 or 128 lines for the small cases: paths wrap
behind the last line by themselves."""
import os
import subprocess

import numpy as np
import pytest

from tests import index_audit, ktab_audit, repeat_refs, synth
from tests.ktab_audit import TAB_OVERFLOW, audit_ktab, build_image, ktab_home_model, revcompl, slot_key, stored_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "shark_amd", "bin", "shark-ktab-check")
K = 9
WHOLE = [(0, 1 << (2 * K))]


def _threads():
    return max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "16") or 16)))


def _canonical(k):
    x = np.arange(1 << (2 * k), dtype=np.uint64)
    return x[x <= revcompl(x, k)]


def _filter(seed, n, k=K):
    """a random subset of the canonical k-mers and a low word for each (30 payload bits, the multi flag at random)"""
    rng = np.random.default_rng(seed)
    keys = np.sort(rng.choice(_canonical(k), size=n, replace=False))
    low = rng.integers(0, 1 << 30, size=n, dtype=np.int64) | (rng.integers(0, 2, size=n, dtype=np.int64) << 31)
    return rng, keys, low


def _orders(rng, n):
    return {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "shuffled": rng.permutation(n)}


@pytest.mark.parametrize("w", [9, 8, 6])
@pytest.mark.parametrize("line_lg", [6, 7])
def test_serial_builder_passes_in_every_order(w, line_lg):
    """ascending, descending, shuffled: three different images of the same key set, none with a violation; the statistics agree
    with what the builder was given, and every configuration displaces keys (load 0.4 in 16-slot lines)"""
    rng, keys, low = _filter(100 * w + line_lg, (16 << line_lg) * 2 // 5)
    images = []
    for name, order in _orders(rng, len(keys)).items():
        img, meta = build_image(keys, low, K, w, line_lg, order)
        viol, st = audit_ktab(img, meta, K, keys, low, WHOLE)
        assert viol == [], (name, viol)
        assert st["keys"] == len(keys) and st["displaced"] > 0 and st["longest_path"] >= 1, (name, st)
        assert st["palindromic"] == 0 and st["above_2_32"] == 0          # (k odd; 18-bit keys)
        idx, got = stored_keys(img, meta, K)
        assert np.array_equal(np.sort(got), keys)
        images.append(img)
    assert not np.array_equal(images[0], images[1]) and not np.array_equal(images[0], images[2])


def test_paths_wrap_behind_the_last_line():
    """some configuration of the above has keys whose path runs from the last lines into line 0 (the probe's `& kmask`), and the
    audit follows them there"""
    wrapped = {}
    for w in (9, 8, 6):
        for line_lg in (6, 7):
            rng, keys, low = _filter(100 * w + line_lg, (16 << line_lg) * 2 // 5)
            img, meta = build_image(keys, low, K, w, line_lg, rng.permutation(len(keys)))
            viol, st = audit_ktab(img, meta, K, keys, low, WHOLE)
            assert viol == []
            wrapped[w, line_lg] = st["wrapped"]
    assert max(wrapped.values()) >= 1, wrapped
    assert wrapped[6, 6] >= 1, wrapped          # (1 + 4 + ... few distinct minimisers, 64 lines: crowded lines everywhere, the last included)


def test_sliced_and_flagged_expectations():
    """what the k = 17 cases rely on: with `complete` a part of the range, a missing key is reported inside it and for a flagged key
    outside it, not for an unflagged key outside it"""
    rng, keys, low = _filter(5, 400)
    img, meta = build_image(keys, low, K, 8, 6)
    half = 1 << (2 * K - 1)
    inside, outside = int(np.flatnonzero(keys < half)[3]), int(np.flatnonzero(keys >= half)[3])
    idx, got = stored_keys(img, meta, K)
    for which, flagged, reported in ((inside, False, True), (outside, False, False), (outside, True, True)):
        bad = img.copy()
        s = int(idx[np.flatnonzero(got == keys[which])[0]])
        bad[s] = 0
        m2 = dict(meta, ktab_keys=meta["ktab_keys"] - 1)
        must = np.zeros(len(keys), bool)
        must[which] = flagged
        viol, _ = audit_ktab(bad, m2, K, keys, low, [(0, half)], must)
        said = any("key %d " % int(keys[which]) in v and "is not stored" in v for v in viol)
        assert said == reported, (which, flagged, viol)


# ---- fourteen single corruptions --------------------------------------------------------------------------------------------
class _Img:
    """an image that passes, decoded: what the corruptions pick their victims from"""

    def __init__(self, seed=11, w=8, line_lg=6, n=420):
        rng, self.keys, self.low = _filter(seed, n)
        self.w, self.line_lg, self.nb = w, line_lg, 8 << line_lg
        self.img, self.meta = build_image(self.keys, self.low, K, w, line_lg, rng.permutation(n))
        assert audit_ktab(self.img, self.meta, K, self.keys, self.low, WHOLE)[0] == []
        self.slot, self.key = stored_keys(self.img, self.meta, K)
        self.home, self.want = ktab_home_model(self.key, K, w, line_lg)
        self.d = (((self.slot >> 1) >> 3) - (self.home >> 3)) & ((1 << line_lg) - 1)
        self.rng = rng

    def free(self, b):
        """a free slot of bucket b, or -1"""
        return 2 * b if self.img[2 * b] == 0 else (2 * b + 1 if self.img[2 * b + 1] == 0 else -1)

    def marked(self, b):
        return bool(self.img[2 * b] & np.uint64(TAB_OVERFLOW))

    def pick(self, cond):
        for i in range(len(self.key)):
            if cond(i):
                return i
        raise AssertionError("no slot of this image suits the corruption: choose another seed")


@pytest.fixture(scope="module")
def base():
    return _Img()


def _cleared_path_end(c):
    i = c.pick(lambda i: c.d[i] > 0)
    img = c.img.copy()
    img[c.slot[i]] = 0
    return img, c.meta, ["key %d " % c.key[i], "is not stored"]


def _cleared_mid_path(c):
    i = c.pick(lambda i: c.d[i] > 0)                     # slot 1 of its home bucket lies on its path
    img = c.img.copy()
    img[2 * c.home[i] + 1] = 0
    return img, c.meta, ["key %d," % c.key[i], "passed a bucket with a free slot"]


def _payload_bit(c):
    s = int(c.slot[len(c.slot) // 2])
    img = c.img.copy()
    img[s] ^= np.uint64(1 << 7)
    return img, c.meta, ["ktab[%d]:" % s, "low word"]


def _key_bit(c):
    i = len(c.slot) // 3
    img = c.img.copy()
    img[c.slot[i]] ^= np.uint64(1 << (32 + 5))
    return img, c.meta, ["key %d " % c.key[i], "is not stored"]


def _moved_within_line(c):
    def other(i):
        b = int(c.slot[i]) >> 1
        return next((f for f in (c.free((b & ~7) | j) for j in range(8) if j != (b & 7)) if f >= 0), -1)
    i = c.pick(lambda i: c.d[i] == 0 and other(i) >= 0)
    img = c.img.copy()
    img[other(i)] = img[c.slot[i]] & ~np.uint64(TAB_OVERFLOW)
    img[c.slot[i]] = 0
    return img, c.meta, ["key %d " % c.key[i], "is not stored"]


def _moved_behind_a_free_slot(c):
    # a key from slot 1 of its home to the same bucket of the next line, the home marked as the builder would: all that is
    # wrong is that the search for it ends at the slot it left
    i = c.pick(lambda i: c.d[i] == 0 and c.slot[i] % 2 == 1 and c.free((int(c.home[i]) + 8) & (c.nb - 1)) >= 0)
    img = c.img.copy()
    img[c.free((int(c.home[i]) + 8) & (c.nb - 1))] = img[c.slot[i]]
    img[c.slot[i]] = 0
    img[2 * c.home[i]] |= np.uint64(TAB_OVERFLOW)
    return img, c.meta, ["key %d," % c.key[i], "passed a bucket with a free slot"]


def _mark_removed(c):
    i = c.pick(lambda i: c.d[i] > 0)
    img = c.img.copy()
    img[2 * c.home[i]] &= ~np.uint64(TAB_OVERFLOW)
    return img, c.meta, ["ktab[%d]:" % (2 * c.home[i]), "overflow mark missing"]


def _mark_added(c):
    i = c.pick(lambda i: c.slot[i] % 2 == 0 and not c.marked(int(c.slot[i]) >> 1))
    img = c.img.copy()
    img[c.slot[i]] |= np.uint64(TAB_OVERFLOW)
    return img, c.meta, ["ktab[%d]:" % c.slot[i], "without a displaced key"]


def _mark_in_slot_1(c):
    i = c.pick(lambda i: c.slot[i] % 2 == 1)
    img = c.img.copy()
    img[c.slot[i]] |= np.uint64(TAB_OVERFLOW)
    return img, c.meta, ["ktab[%d]:" % c.slot[i], "overflow mark in slot 1"]


def _duplicated(c):
    def further(i):
        b = int(c.slot[i]) >> 1
        for _ in range(int(c.d[i]) + 1, 64):
            b = (b + 8) & (c.nb - 1)
            if c.free(b) >= 0:
                return c.free(b)
        return -1
    i = c.pick(lambda i: further(i) >= 0)
    img = c.img.copy()
    img[further(i)] = img[c.slot[i]] & ~np.uint64(TAB_OVERFLOW)
    return img, c.meta, ["key %d " % c.key[i], "more than once"]


def _taken_bit(c):
    s = int(c.slot[len(c.slot) // 5])
    img = c.img.copy()
    img[s] &= ~np.uint64(1 << 32)
    return img, c.meta, ["ktab[%d]:" % s, "without the taken bit"]


def _spare_written(c):
    img = c.img.copy()
    img[2 * c.nb + 3] = 5
    return img, c.meta, ["ktab[%d]:" % (2 * c.nb + 3), "spare bucket"]


def _count_off(c):
    return c.img, dict(c.meta, ktab_keys=c.meta["ktab_keys"] + 1), ["ktab[0]:", "ktab_keys"]


def _non_key_inserted(c):
    # at its rightful place: home bucket, right high word, a payload, the count raised -- all that is wrong is that the filter
    # does not hold it
    cand = np.setdiff1d(_canonical(K)[::37], c.keys)
    home, want = ktab_home_model(cand, K, c.w, c.line_lg)
    j = next(j for j in range(len(cand)) if c.free(int(home[j])) >= 0)
    img = c.img.copy()
    img[c.free(int(home[j]))] = (np.uint64(want[j]) << np.uint64(32)) | np.uint64(77)
    return img, dict(c.meta, ktab_keys=c.meta["ktab_keys"] + 1), ["key %d " % cand[j], "is not a canonical k-mer whose filter bit is set"]


def _stored_reverse_complemented(c):
    # the reverse complement has the key's minimiser, hence its line; bucket and high word are its own
    rc = revcompl(c.key, K)
    lo = ktab_audit._image(rc, K)
    bkt = ((c.home >> 3) << 3) | (lo & np.uint64(7)).astype(np.int64)
    i = c.pick(lambda i: c.d[i] == 0 and not (c.slot[i] % 2 == 0 and c.marked(int(c.home[i]))) and bkt[i] != c.home[i] and c.free(int(bkt[i])) >= 0)
    assert int(slot_key(((lo[i] >> np.uint64(3)) << np.uint64(1)) | np.uint64(1), bkt[i], K)) == int(rc[i]) != int(c.key[i])
    img = c.img.copy()
    img[c.free(int(bkt[i]))] = ((((lo[i] >> np.uint64(3)) << np.uint64(1)) | np.uint64(1)) << np.uint64(32)) | (img[c.slot[i]] & np.uint64(0xFFFFFFFF))
    img[c.slot[i]] = 0
    return img, c.meta, ["key %d " % rc[i], "is not canonical"]


CORRUPTIONS = [_cleared_path_end, _cleared_mid_path, _payload_bit, _key_bit, _moved_within_line, _moved_behind_a_free_slot, _mark_removed,
               _mark_added, _mark_in_slot_1, _duplicated, _taken_bit, _spare_written, _count_off, _non_key_inserted, _stored_reverse_complemented]


@pytest.mark.parametrize("corrupt", CORRUPTIONS, ids=lambda f: f.__name__.strip("_"))
def test_single_corruption_is_reported(base, corrupt):
    """one thing wrong in an image that passed: at least one violation, and one of them says what and names the slot or the key"""
    img, meta, needles = corrupt(base)
    viol, _ = audit_ktab(img, meta, K, base.keys, base.low, WHOLE)
    assert viol, corrupt.__name__
    assert all(v.startswith("ktab[") for v in viol), viol
    assert any(all(n in v for n in needles) for v in viol), (needles, viol)


def test_base_image_is_left_alone(base):
    """(the corruptions work on copies: the shared image still passes)"""
    assert audit_ktab(base.img, base.meta, K, base.keys, base.low, WHOLE)[0] == []


# ---- the real pipeline on the CPU ---------------------------------------------------------------------------------------------
def test_pipeline_k15(oracle):
    """k = 15, 40 genes, 2^26 bits: the oracle's filter, every canonical 15-mer asked (so_filter_sweep over all 4^15 values), low
    words from index_audit.Model, the serial builder at the device builder's sizing rule, the audit -- and the sweep's keys are
    the reference's own k-mers plus false positives, about as many as the filter's density predicts"""
    k, bf_bits = 15, 1 << 26
    rng = np.random.default_rng(15)
    genes = [bytes(g) for g in synth.make_genes(rng, 40, 300, 2000, share_every=3)]
    o = oracle.Shark(k=k, c=0.0, bf_bits=bf_bits)
    o.build(genes)
    m = index_audit.Model(oracle, o, genes, k, bf_bits)
    n, keys = oracle.filter_sweep(k, o.bf_words(), bf_bits, 0, 1 << (2 * k), nthreads=_threads())
    assert n == len(keys) and (keys[1:] > keys[:-1]).all()
    pos = oracle.get_hash_many(keys) % np.uint64(bf_bits)
    rk = np.searchsorted(m.setbits, pos)
    assert np.array_equal(m.setbits[rk], pos)                       # every key's bit is a set bit
    ref = np.unique(m.canon[m.vx])
    assert np.isin(ref, keys).all()                                 # the reference's own k-mers are among them
    expect_fp = (4 ** k / 2 - len(ref)) * m.n_set / bf_bits
    assert abs((len(keys) - len(ref)) - expect_fp) < 6 * expect_fp ** 0.5 + 10, (len(keys), len(ref), expect_fp)
    low = index_audit.expected_low(m, rk)
    line_lg = ktab_audit.line_lg_rule(m.n_set, bf_bits, k)
    img, meta = build_image(keys, low, k, 15, line_lg)
    assert len(img) == (16 << line_lg) + 16
    viol, st = audit_ktab(img, meta, k, keys, low, [(0, 1 << (2 * k))], np.isin(keys, ref))
    assert viol == [], viol
    assert st["keys"] == len(keys) and st["displaced"] > 0, st
    o.close()


# ---- the model against the header ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    if not os.path.exists(TOOL):
        env = dict(os.environ)
        env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.run(["make", "-C", os.path.join(ROOT, "shark_amd", "csrc"), "../bin/shark-ktab-check"], check=True, stdout=subprocess.DEVNULL, env=env)
    return TOOL


def _tool_says(tool, k, w, line_lg, kmers):
    text = "%d %d %d\n" % (k, w, line_lg) + "\n".join(str(int(x)) for x in kmers) + "\n"
    r = subprocess.run([tool], input=text, capture_output=True, text=True, check=True)
    a = np.array(r.stdout.split(), dtype=np.int64).reshape(-1, 2)
    assert len(a) == len(kmers)
    return a[:, 0], a[:, 1]


@pytest.mark.parametrize("k,w,line_lg", [(15, 15, 12), (16, 15, 17), (17, 15, 20), (17, 14, 28), (9, 6, 6)])
def test_model_equals_ktab_home(tool, k, w, line_lg):
    """ktab_home itself (kmer_device.hpp, compiled for the host) on 10^5 random k-mers of either strand, the extremes and, for
    k = 16, every palindrome: the same bucket and the same compare word as the model; the inverse gives the canonical key back; the
    model's minimiser hash is repeat_refs.wmer_hash's"""
    rng = np.random.default_rng(k * 100 + w)
    x = rng.integers(0, 1 << (2 * k), size=100000, dtype=np.uint64)
    x = np.concatenate([x, np.array([0, 1, (1 << (2 * k)) - 1, (1 << (2 * k)) - 2, 1 << 32 if k > 16 else 5, (1 << 32) - 1 if k >= 16 else 6], dtype=np.uint64)])
    if k == 16:
        h = np.arange(1 << 16, dtype=np.uint64)                     # a palindrome is its first half followed by that half's reverse complement
        pal = (h << np.uint64(16)) | revcompl(h, 8)
        assert np.array_equal(pal, revcompl(pal, 16))
        x = np.concatenate([x, pal])
    bucket, want = ktab_home_model(x, k, w, line_lg)
    tb, tw = _tool_says(tool, k, w, line_lg, x)
    assert np.array_equal(bucket, tb) and np.array_equal(want, tw)
    canon = np.minimum(x, revcompl(x, k))
    assert np.array_equal(slot_key(want, bucket, k), canon)
    b2, w2 = ktab_home_model(revcompl(x, k), k, w, line_lg)          # the other strand: the same place
    assert np.array_equal(b2, bucket) and np.array_equal(w2, want)
    hs = ktab_audit.wmer_hashes(x[:50], k, w)
    for i in range(50):
        s = repeat_refs._unpack(int(x[i]), k)
        assert [repeat_refs.wmer_hash(s[j:j + w]) for j in range(k - w + 1)] == [int(v) for v in hs[i]]
