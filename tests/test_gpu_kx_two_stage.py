"""The two-stage compare of the k-mer keyed exact table (kmer_table.hpp: kxtab_candidate, then kxtab_confirm behind a ballot) under
probes that pass the first stage and must fail the second.  From the exported image, its multipliers and the key list the two Feistel
steps are inverted to canonical k-mers that are NOT keys and yet agree with the probed slot in the tag's low 16 bits:
  (N1) the slot of a stored key, its low 16 tag bits, bit 16 or 17 different;
  (N2) tag low half 0, high bits not 0, on an empty slot that exists;
  (N3) tag exactly 0, on an empty slot;
  (N4) a ring slot at or above KXTAB_SLOTS, the tag's low 16 bits equal to the two image bytes found there (T2's or D's).
A kernel that stopped at the 16-bit compare would count every one of them as a hit.  They are planted in reads at every slot of
both mates (even and odd prefix slots, tile slots, slots behind the first stop), at all tile slots of a pair at once, beside N, and
where one false hit lifts a pair from the gene over its threshold; the results must be the oracle's, on every route a one-gene index
takes, and equal to the same library's with SHK_NO_KMER_TABLE=1.  The stages themselves are restated here and asserted for every
planted k-mer: candidate yes, lookup no.

Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import torch  # noqa: F401  (torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both)

from tests import synth
from tests.placement_audit import kmer_bytes

pytestmark = pytest.mark.gpu

U64 = np.uint64
SWITCHES = ("SHK_PROBE", "SHK_NO_LDS_TABLE", "SHK_FORCE_GENERIC", "SHK_KTAB", "SHK_NO_LDS_SUMMARY", "SHK_NO_SUMMARY", "SHK_TILE_FIRST", "SHK_NO_TRI",
            "SHK_NO_TRO", "SHK_CLS_MIN_FILL", "SHK_NO_SPARSE", "SHK_FORCE_TRO", "SHK_NO_KMER_TABLE")

# kmer_table.hpp
SLOTS, RING, T2_OFF, D_OFF, GROUPS = 57344, 65536, 114688, 129024, 8192
L, C = 150, 0.6
THR = 180          # ceil(C * 2 L)
CLASSES = ("N1", "N2", "N3", "N4")


# ---------------------------------------------------------------------------
# the lookup rule in two stages, and its inverse
# ---------------------------------------------------------------------------
def kx_mix(m1, m2, c):
    """kxtab_mix: (tag, slot before the displacement, low 16 bits)"""
    c = np.asarray(c, dtype=U64)
    m32 = U64(0xFFFFFFFF)
    lo = c & m32
    a = lo & U64(0xFFFF)
    tag = (c >> U64(16)) ^ ((((a * U64(m1) + U64(m1)) & m32) >> U64(6)) & U64(0x3FFFF))
    base = (lo ^ (((tag * U64(m2)) & m32) >> U64(16))) & U64(0xFFFF)
    return tag, base


def kx_unmix(m1, m2, tag, base):
    """the key with this tag and this slot before the displacement: the two Feistel steps backwards"""
    tag, base = np.asarray(tag, dtype=U64), np.asarray(base, dtype=U64)
    m32 = U64(0xFFFFFFFF)
    a = (base ^ (((tag * U64(m2)) & m32) >> U64(16))) & U64(0xFFFF)
    b = tag ^ (((((a + U64(1)) * U64(m1)) & m32) >> U64(6)) & U64(0x3FFFF))
    return (b << U64(16)) | a


def kx_candidate(img, m1, m2, c):
    """stage 1 (kxtab_candidate): mixing, D, slot, T16, the tag's low 16 bits compared -> (candidate, tag, twice the slot)"""
    tag, base = kx_mix(m1, m2, c)
    d = img[D_OFF:D_OFF + 2 * GROUPS].view(np.uint16)[(tag & U64(GROUPS - 1)).astype(np.int64)].astype(U64)
    s2 = (((base + d) << U64(1)) & U64(2 * RING - 2)).astype(np.int64)
    t16 = img[:2 * RING].view(np.uint16)[s2 >> 1].astype(U64)
    return t16 == (tag & U64(0xFFFF)), tag, s2


def kx_confirm(img, tag, s2):
    """stage 2 (kxtab_confirm): T2's two bits, the slot exists, the tag is not the empty entry's"""
    t2 = img[T2_OFF + (s2 >> 3)].astype(U64)
    return (s2 < 2 * SLOTS) & (((t2 >> (s2 & 6).astype(U64)) & U64(3)) == (tag >> U64(16))) & (tag != U64(0))


def kx_lookup(img, m1, m2, c):
    cand, tag, s2 = kx_candidate(img, m1, m2, c)
    return cand & kx_confirm(img, tag, s2)


def revcomp_of(v, k):
    v = np.asarray(v, dtype=U64)
    rc = np.zeros(len(v), dtype=U64)
    for j in range(k):
        rc |= (U64(3) - ((v >> U64(2 * j)) & U64(3))) << U64(2 * (k - 1 - j))
    return rc


def near_misses(img, m1, m2, keys, k):
    """per class: the canonical k-mers (sorted, distinct) that are no keys and pass the 16-bit stage the way the class says"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    slot = np.arange(RING, dtype=np.int64)
    word = img[:2 * RING].view(np.uint16).astype(U64)                                # the two bytes a probe of ring slot s compares
    t2 = (img[T2_OFF + (slot[:SLOTS] >> 2)].astype(U64) >> (2 * (slot[:SLOTS] & 3)).astype(U64)) & U64(3)
    entry = word[:SLOTS] | (t2 << U64(16))
    D = img[D_OFF:D_OFF + 2 * GROUPS].view(np.uint16).astype(np.int64)
    used, empty = slot[:SLOTS][entry != 0], slot[:SLOTS][entry == 0]
    beyond = slot[SLOTS:]
    raw = {c: [] for c in CLASSES}
    for h in range(4):
        hi = U64(h << 16)
        if h:
            raw["N1"].append((entry[used] ^ hi, used))
            raw["N2"].append((np.full(len(empty), hi, dtype=U64), empty))
        else:
            raw["N3"].append((np.zeros(len(empty), dtype=U64), empty))
        raw["N4"].append((word[beyond] | hi, beyond))
    out = {}
    for cls, parts in raw.items():
        tag = np.concatenate([t for t, _ in parts])
        s = np.concatenate([x for _, x in parts])
        c = kx_unmix(m1, m2, tag, (s - D[(tag & U64(GROUPS - 1)).astype(np.int64)]) & (RING - 1))
        c = c[c < U64(4 ** k)]
        c = np.unique(c[c <= revcomp_of(c, k)])
        out[cls] = c[~np.isin(c, keys)]
    return out


def check_construction(img, m1, m2, keys, k, nm):
    """the CPU part: every planted k-mer is a candidate and not in the table -- by the class's own reason"""
    assert kx_lookup(img, m1, m2, keys).all()
    for cls in CLASSES:
        c = nm[cls]
        assert len(c) >= 32, (k, cls, len(c))
        cand, tag, s2 = kx_candidate(img, m1, m2, c)
        assert cand.all(), (k, cls)
        assert not kx_lookup(img, m1, m2, c).any(), (k, cls)
        assert not np.isin(c, keys).any() and (c <= revcomp_of(c, k)).all() and (c < U64(4 ** k)).all()
        t2 = (img[T2_OFF + (s2 >> 3)].astype(U64) >> (s2 & 6).astype(U64)) & U64(3)
        if cls == "N1":
            assert (s2 < 2 * SLOTS).all() and (tag != 0).all() and (t2 != (tag >> U64(16))).all()
            assert (((t2 << U64(16)) | (tag & U64(0xFFFF))) != 0).all()                        # (the slot is a stored key's)
        elif cls == "N2":
            assert (s2 < 2 * SLOTS).all() and ((tag & U64(0xFFFF)) == 0).all() and (tag != 0).all() and (t2 == 0).all()
        elif cls == "N3":
            assert (s2 < 2 * SLOTS).all() and (tag == 0).all() and (t2 == 0).all()             # (all 18 bits agree: only tag != 0 rejects)
        else:
            assert (s2 >= 2 * SLOTS).all()
    # (and the classes are told apart by the guards: N3 and part of N4 pass the T2 compare as well)
    cand, tag, s2 = kx_candidate(img, m1, m2, nm["N4"])
    t2 = (img[T2_OFF + (s2 >> 3)].astype(U64) >> (s2 & 6).astype(U64)) & U64(3)
    assert np.any((t2 == (tag >> U64(16))) & (tag != 0)), "no N4 k-mer that only `slot < KXTAB_SLOTS` rejects"


# ---------------------------------------------------------------------------
# indices, reads
# ---------------------------------------------------------------------------
INDICES = {13: (8000, 1 << 24), 17: (20000, 1 << 33)}
_cases = {}


def gene_of(k):
    return synth.random_seq(np.random.default_rng(4000 + k), INDICES[k][0])


def build(monkeypatch, k, env=None, expect_kx=True):
    from shark_amd import SharkHip
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for name, val in (env or {}).items():
        monkeypatch.setenv(name, val)
    h = SharkHip(k=k, c=C, bf_bits=INDICES[k][1])
    h.build([bytes(gene_of(k))])
    assert h.probe_mode() == "lds-table", h.probe_mode()
    meta = dict(h.debug_index_meta(), **h.debug_kx_meta())
    assert meta["kx_in_use"] == (1 if expect_kx else 0), meta
    return h, meta


def kmer_seq(rng, v, k):
    s = np.frombuffer(kmer_bytes(v, k), dtype=np.uint8)
    return synth.revcomp(s) if rng.integers(0, 2) else s.copy()


def make_pairs(rng, gene, k, nm, keys):
    """(mate 1 list, mate 2 list, kind per pair); 2 x 150 bp"""
    m1, m2, kind = [], [], []
    turn = [0]

    def nm_seq(cls=None):
        cls = cls or CLASSES[turn[0] % 4]
        turn[0] += 1
        pool = nm[cls]
        return kmer_seq(rng, pool[int(rng.integers(0, len(pool)))], k)

    def add(a, b, what):
        assert len(a) == L and len(b) == L
        m1.append(a)
        m2.append(b)
        kind.append(what)

    nk = L - k + 1
    # pairs from elsewhere, one near-miss at slot p of mate 1 / mate 2: every p -- even and odd prefix slots, tile slots, slots
    # behind the first stop
    for mate in (0, 1):
        for p in range(nk):
            r = [synth.random_seq(rng, L), synth.random_seq(rng, L)]
            r[mate][p:p + k] = nm_seq()
            add(r[0], r[1], "elsewhere")
    # ... near-misses at ALL tile slots (0, k, 2k, ...) of both mates, one class and mixed; and the same shifted by 1, 2 (prefix slots)
    for shift in (0, 0, 0, 0, 0, 1, 2):
        cls = CLASSES[len(m1) % 4] if shift == 0 and len(m1) % 5 else None
        r = [synth.random_seq(rng, L), synth.random_seq(rng, L)]
        for mate in (0, 1):
            for p in range(shift, nk, k):
                r[mate][p:p + k] = nm_seq(cls)
        add(r[0], r[1], "elsewhere-tiles")
    # ... with N beside the planted k-mer (in front of it, behind it), and inside a second one
    for i in range(36):
        r = [synth.random_seq(rng, L), synth.random_seq(rng, L)]
        mate, p = i & 1, 1 + (i * 7) % (nk - 2)
        r[mate][p:p + k] = nm_seq()
        if i % 3 != 1:
            r[mate][p - 1] = ord("N")
        if i % 3 != 0 and p + k < L:
            r[mate][p + k] = ord("N")
        if i % 4 == 3:
            q = (p + 2 * k) % (nk - 1)
            r[1 - mate][q:q + k] = nm_seq()
            r[1 - mate][q + k // 2] = ord("N")
        add(r[0], r[1], "elsewhere-N")
    # pairs from the gene whose true coverage is short of the threshold by less than one k-mer: one mate is 150 bases of the gene, the
    # other starts with G >= k bases of it (150 + G < 180), then a planted k-mer, then random bases.  Planted: a near-miss (a false hit
    # would give 150 + G + k >= 180) -- and the same pair with a key in its place, which is over the threshold
    # -- every class with the short mate as mate 2 and as mate 1 (different slots of the packed pair, hence different rounds), in
    # both orientations of the gene's bases; every fourth with N right behind the planted k-mer
    n_short = 0
    for G in range(max(k, THR - L - k), THR - L):
        for cls in CLASSES:
            for first in (False, True):
                n_short += 1
                a = int(rng.integers(0, len(gene) - 400))
                whole = gene[a:a + L].copy()
                tail = synth.random_seq(rng, L - G - k)
                if n_short % 4 == 0:
                    tail[0] = ord("N")
                near = nm_seq(cls)
                key = kmer_seq(rng, keys[int(rng.integers(0, len(keys)))], k)
                for planted, what in ((near, "gene-short"), (key, "gene-over")):
                    part = np.concatenate([synth.revcomp(gene[a + 200:a + 200 + G]) if (n_short >> 1) & 1 else gene[a + 200:a + 200 + G], planted, tail])
                    if first:
                        add(part, synth.revcomp(whole), what)
                    else:
                        add(whole.copy(), part, what)
    # pairs from the gene with six to nine of their sixteen tiles broken by one substitution each: the tiles' round does not settle
    # them (11 tiles are needed), the rounds behind it do
    for i in range(60):
        a = int(rng.integers(0, len(gene) - 400))
        r = [gene[a:a + L].copy(), synth.revcomp(gene[a + 200:a + 200 + L])]
        for t in rng.choice(16, size=6 + i % 4, replace=False):
            mate, p = int(t) >> 3, (int(t) & 7) * k + (k - 1 if i % 2 else int(rng.integers(0, k)))
            if p < L:
                r[mate][p] = synth.ACGT[(int(np.searchsorted(synth.ACGT, r[mate][p])) + 1 + int(rng.integers(0, 3))) & 3]
        add(r[0], r[1], "gene-broken-tiles")
    order = rng.permutation(len(m1))
    return [m1[i] for i in order], [m2[i] for i in order], np.array(kind)[order]


def args(b):
    return b["seq1"], b["off1"], b["seq2"], b["off2"]


def head(batch, want, n, first=0):
    """pairs [first, first + n) of a batch, and the oracle's answer for them (a pair's answer does not depend on its batch)"""
    o1, o2 = batch["off1"].astype(np.int64), batch["off2"].astype(np.int64)
    sub = (batch["seq1"][o1[first]:o1[first + n]], (o1[first:first + n + 1] - o1[first]).astype(np.uint64),
           batch["seq2"][o2[first]:o2[first + n]], (o2[first:first + n + 1] - o2[first]).astype(np.uint64))
    goff = want[0].astype(np.int64)
    return sub, ((goff[first:first + n + 1] - goff[first]).astype(want[0].dtype), want[1][goff[first]:goff[first + n]])


def case_for(oracle, monkeypatch, k):
    """per index, made once: the image's near-misses (construction checked), the batches (2 x 150 bp: 3 m + 1 pairs; trimmed: the
    same pairs with both mates cut to 120 .. 150 bases) and the oracle's answers"""
    if k not in _cases:
        gene = gene_of(k)
        h, meta = build(monkeypatch, k)
        img, keys = h.debug_index_array("kxtab"), h.debug_index_array("kxkeys")
        h.close()
        m1, m2 = meta["kx_m1"], meta["kx_m2"]
        nm = near_misses(img, m1, m2, keys, k)
        check_construction(img, m1, m2, keys, k, nm)
        rng = np.random.default_rng(k)
        a, b, kind = make_pairs(rng, gene, k, nm, keys)
        n = (len(a) - 1) // 3 * 3 + 1
        a, b, kind = a[:n], b[:n], kind[:n]
        o = oracle.Shark(k=k, c=C, bf_bits=INDICES[k][1])
        o.build([bytes(gene)])
        batches = {}
        for name in ("uniform", "trimmed"):
            if name == "trimmed":
                a = [x[:int(rng.integers(120, L + 1))] for x in a]
                b = [x[:int(rng.integers(120, L + 1))] for x in b]
            bt = synth.batch_from_lists(a, b)
            batches[name] = (bt, o.classify(*args(bt), nthreads=4))
        assigned = np.diff(batches["uniform"][1][0].astype(np.int64)) > 0
        # the construction does what it says -- by the oracle: no pair from elsewhere is assigned whatever is planted in it; a false
        # hit would decide the pairs from the gene that are short of the threshold (nearly all: a chance hit in the random tail is
        # rare), the same pairs with a key are over it; most of the pairs with broken tiles are the gene's
        for what in ("elsewhere", "elsewhere-tiles", "elsewhere-N"):
            assert not assigned[kind == what].any(), what
        short, over = assigned[kind == "gene-short"], assigned[kind == "gene-over"]
        assert len(short) >= 40 and short.mean() < 0.2 and over.mean() > 0.9, (k, len(short), short.mean(), over.mean())
        assert assigned[kind == "gene-broken-tiles"].mean() > 0.5
        _cases[k] = (batches, n, {c: len(v) for c, v in nm.items()})
    return _cases[k]


ROUTES = [
    ("uniform+tiles", "uniform", {"SHK_TILE_FIRST": "1"}, ("+three-pairs", "+tiles-first")),
    ("uniform", "uniform", {"SHK_TILE_FIRST": "0"}, ("+three-pairs",)),
    ("uniform-one-pair", "uniform", {"SHK_NO_TRI": "1"}, (", 21, true>",)),
    ("offsets+tiles", "trimmed", {"SHK_TILE_FIRST": "1"}, ("offsets", "+tiles-first")),
    ("offsets", "trimmed", {"SHK_TILE_FIRST": "0"}, ("offsets",)),
    ("class-by-class", "trimmed", {"SHK_CLS_MIN_FILL": "1", "SHK_NO_TRO": "1"}, ("verdict=classes",)),
    ("ragged", "trimmed", {"SHK_CLS_MIN_FILL": "0", "SHK_NO_TRO": "1"}, (", 21, false>",)),
]


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "gene_off differs at read %d" % int(np.argmax(got[0][:len(want[0])] != want[0])))
    assert np.array_equal(got[1], want[1]), what


@pytest.mark.parametrize("k", sorted(INDICES))
def test_near_misses_pass_the_first_stage_only(oracle, monkeypatch, k):
    """the construction alone: at least 32 k-mers of each class per index, each one a candidate and none in the table"""
    _, n, counts = case_for(oracle, monkeypatch, k)
    print("k = %d: %d pairs, near-misses per class %s" % (k, n, counts))
    assert n % 3 == 1 and min(counts.values()) >= 32


@pytest.mark.parametrize("k", sorted(INDICES))
@pytest.mark.parametrize("name,kind,env,says", ROUTES, ids=[r[0] for r in ROUTES])
def test_planted_near_misses_on_every_route(oracle, monkeypatch, name, kind, env, says, k):
    batches, n, _ = case_for(oracle, monkeypatch, k)
    batch, want = batches[kind]
    h, _ = build(monkeypatch, k, env=env)
    same(h.classify(*args(batch)), want, (name, "3 m + 1"))
    lk = h.last_kernel()
    for s in says:
        assert s in lk, (name, s, lk)
    sub, w = head(batch, want, n - 2)
    same(h.classify(*sub), w, (name, "3 m - 1"))
    for cnt in range(1, 9):
        sub, w = head(batch, want, cnt, first=11 * cnt)
        same(h.classify(*sub), w, (name, cnt))
    same(h.classify(*args(batch)), want, (name, "again"))          # (the stream's history picks the tiles' round by itself now)
    h.close()
    h2, _ = build(monkeypatch, k, env=dict(env, SHK_NO_KMER_TABLE="1"), expect_kx=False)
    same(h2.classify(*args(batch)), want, (name, "SHK_NO_KMER_TABLE=1"))
    h2.close()
