"""The k-mer keyed exact table of a one-gene index on the GPU (kmer_table.hpp; kmer_enum_kernel in index_build.hip; the KX
instantiations of classify_uni_kernel): the key set the device enumerates against a brute force over all canonical k-mers, the image
it builds under a Python restatement of the lookup rule, both sides of the capacity, colliding k-mers that decide a verdict, every
route a one-gene index can take, and where a read sits in its batch.  Every case asserts through the index's read-out (`kxmeta`) that the table
is in use -- or, in the stated fall-back cases, that it is not -- so none passes by silently probing the hashed table.

Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import torch  # noqa: F401  (torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both)

from tests import synth
from tests.placement_audit import canonical_kmers, kmer_bytes, xxh64_u64

pytestmark = pytest.mark.gpu

U64 = np.uint64
SWITCHES = ("SHK_PROBE", "SHK_NO_LDS_TABLE", "SHK_FORCE_GENERIC", "SHK_KTAB", "SHK_NO_LDS_SUMMARY", "SHK_NO_SUMMARY", "SHK_TILE_FIRST", "SHK_NO_TRI",
            "SHK_NO_TRO", "SHK_CLS_MIN_FILL", "SHK_NO_SPARSE", "SHK_FORCE_TRO", "SHK_NO_KMER_TABLE")

# kmer_table.hpp
SLOTS, T2_OFF, D_OFF, KX_BYTES, MAX_KEYS = 57344, 114688, 129024, 145408, 44000


def kx_lookup(img, m1, m2, c):
    """kxtab_lookup restated: img = the exported image (uint8), c = uint64 values below 2^34"""
    c = np.asarray(c, dtype=U64)
    m32 = U64(0xFFFFFFFF)
    lo = c & m32
    a = lo & U64(0xFFFF)
    tag = (c >> U64(16)) ^ ((((a * U64(m1) + U64(m1)) & m32) >> U64(6)) & U64(0x3FFFF))
    base = lo ^ (((tag * U64(m2)) & m32) >> U64(16))
    d = img[D_OFF:D_OFF + 16384].view(np.uint16)[(tag & U64(0x1FFF)).astype(np.int64)].astype(U64)
    s2 = (((base + d) << U64(1)) & U64(0x1FFFE)).astype(np.int64)
    t16 = img[:131072].view(np.uint16)[s2 >> 1].astype(U64)
    t2 = img[T2_OFF + (s2 >> 3)].astype(U64)
    e = t16 | (((t2 >> (s2 & 6).astype(U64)) & U64(3)) << U64(16))
    return (s2 < 2 * SLOTS) & (e == tag) & (tag != U64(0))


def revcomp_of(v, k):
    v = np.asarray(v, dtype=U64)
    rc = np.zeros(len(v), dtype=U64)
    for j in range(k):
        rc |= (U64(3) - ((v >> U64(2 * j)) & U64(3))) << U64(2 * (k - 1 - j))
    return rc


def brute_force_keys(k, lgb, filters):
    """per filter (bool array of 2^lgb bits): every canonical k-mer whose XXH64 position is a set bit, sorted -- one pass over all 4^k
    k-mers (less the ones whose first base is above the complement of their last: never canonical)"""
    out = [[] for _ in filters]
    mask = U64((1 << lgb) - 1)
    step = 1 << 22
    for first in range(0, 4 ** k, step):
        v = np.arange(first, min(first + step, 4 ** k), dtype=U64)
        v = v[(v >> U64(2 * k - 2)) + (v & U64(3)) <= U64(3)]
        pos = (xxh64_u64(v) & mask).astype(np.int64)
        for f, o in zip(filters, out):
            hit = v[f[pos]]
            o.append(hit[hit <= revcomp_of(hit, k)])
    return [np.sort(np.concatenate(o)) for o in out]


def filter_bits(h):
    return np.unpackbits(h.copy_bf().view(np.uint8), bitorder="little").astype(bool)


def gene_of(seed, n):
    return synth.random_seq(np.random.default_rng(seed), n)


def build(monkeypatch, gene, k, bf_bits, c=0.6, env=None, expect_kx=True, modes=("lds-table",)):
    from shark_amd import SharkHip
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for name, val in (env or {}).items():
        monkeypatch.setenv(name, val)
    h = SharkHip(k=k, c=c, bf_bits=bf_bits)
    h.build([bytes(gene)])
    assert h.probe_mode() in modes, h.probe_mode()
    meta = dict(h.debug_index_meta(), **h.debug_kx_meta())
    assert meta["kx_in_use"] == (1 if expect_kx else 0), meta
    assert len(h.debug_index_array("kxtab")) == (147456 if expect_kx else 0)
    return h, meta


_oracles = {}


def oracle_for(oracle, gene, k, bf_bits, c=0.6):
    key = (bytes(gene), k, bf_bits, c)
    if key not in _oracles:
        o = oracle.Shark(k=k, c=c, bf_bits=bf_bits)
        o.build([bytes(gene)])
        _oracles[key] = o
    return _oracles[key]


def args(b):
    return b["seq1"], b["off1"], b["seq2"], b["off2"]


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "gene_off differs at read %d" % int(np.argmax(got[0][:len(want[0])] != want[0])))
    assert np.array_equal(got[1], want[1]), what


# ---------------------------------------------------------------------------
# 1. the key set and the image
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [11, 12, 13])
def test_key_set_and_image_against_brute_force(monkeypatch, k):
    """(k, 2^24 bits), genes of 3 000 and 8 000 bases: the exported sorted key list IS the set of canonical k-mers whose XXH64 position
    is a set bit (k = 12: k-mers that are their own reverse complement are enumerated once; k = 13: the colliding k-mers are twice
    the gene's own, the headline's regime), and the exported image answers exactly that set"""
    lgb = 24
    genes = [gene_of(100 * k + n, n) for n in (3000, 8000)]
    if k == 12:
        for g in genes:
            g[1000:1012] = np.frombuffer(b"ACGTACGTACGT", dtype=np.uint8)      # its own reverse complement: in the list once
    built = [build(monkeypatch, g, k, 1 << lgb) for g in genes]
    want = brute_force_keys(k, lgb, [filter_bits(h) for h, _ in built])
    rng = np.random.default_rng(k)
    for (h, meta), keys_want, n in zip(built, want, (3000, 8000)):
        keys = h.debug_index_array("kxkeys")
        assert meta["kx_keys"] == len(keys) == len(keys_want), (k, n, meta["kx_keys"], len(keys_want))
        assert np.array_equal(keys, keys_want), (k, n)
        expected = meta["n_set"] * (1 + 4 ** k / 2 / 2 ** lgb)
        assert 0.9 * expected < len(keys) < 1.1 * expected, (k, n, len(keys), expected)
        if k == 12:
            assert int(np.sum(keys == revcomp_of(keys, k))) >= 1
        img = h.debug_index_array("kxtab")
        assert not img[KX_BYTES:].any()
        m1, m2 = meta["kx_m1"], meta["kx_m2"]
        assert kx_lookup(img, m1, m2, keys).all(), (k, n)
        probes = [rng.integers(0, 1 << 34, size=2000000, dtype=np.uint64)]
        probes += [keys ^ U64(1 << b) for b in range(34)]
        if k == 11:
            probes.append(np.arange(4 ** k, dtype=U64))          # every 11-mer, canonical or not
        for p in probes:
            assert np.array_equal(kx_lookup(img, m1, m2, p), np.isin(p, keys)), (k, n)
        h.close()


# ---------------------------------------------------------------------------
# 2. both sides of the capacity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,lgb,n_bases,in_use", [(13, 24, 8000, True), (13, 24, 16000, False), (17, 33, 21500, True), (17, 33, 23000, False)])
def test_both_sides_of_the_capacity(oracle, monkeypatch, k, lgb, n_bases, in_use):
    """(13, 2^24): a gene of 8 000 bases has about 24 000 keys -- the table is built; one of 16 000 bases about 48 000 -- it is not (nor
    does the hashed exact table hold 16 000 positions of a 2^24-bit filter: the LDS summary's chain serves).  (17, 2^33): 21 500 bases,
    about 43 000 keys, built; 23 000 bases, about 46 000, not built, the hashed exact table serves.  All give the oracle's associations"""
    gene = gene_of(7 + n_bases, n_bases)
    h, meta = build(monkeypatch, gene, k, 1 << lgb, expect_kx=in_use, modes=("lds-table",) if lgb == 33 else ("lds-table", "lds-summary+table"))
    expected = meta["n_set"] * (1 + 4 ** k / 2 / 2 ** lgb)
    assert (expected <= MAX_KEYS) == in_use, meta
    if in_use:
        assert 0.97 * expected < meta["kx_keys"] < 1.03 * expected, meta
    o = oracle_for(oracle, gene, k, 1 << lgb)
    batch = synth.make_reads(np.random.default_rng(5), [gene], 3000, read_len=150, on_target=0.5)
    want = o.classify(*args(batch), nthreads=2)
    assert 1000 < int(want[0][-1]) < 2000
    same(h.classify(*args(batch)), want, n_bases)
    assert (", 21, " in h.last_kernel()) == (h.probe_mode() == "lds-table"), h.last_kernel()
    h.close()


# ---------------------------------------------------------------------------
# 3. colliding k-mers decide a verdict
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,bf_bits,n_bases", [(13, 1 << 24, 8000), (17, 1 << 33, 20000)])
def test_colliding_kmers_decide_a_verdict(oracle, monkeypatch, k, bf_bits, n_bases):
    """2 x 150 bp, c = 0.6: the threshold is 180 bases.  Mate 1 is 150 bases of the gene, mate 2 starts with G bases of the gene, then a
    k-mer from the exported list that is NOT the gene's (it collides with one in the filter), or a random k-mer in its place, then
    random bases (the same ones for both) -- for G from below 30 - k to above 30, so that pairs pass only because of the colliding k-mer, pairs pass without
    it, and pairs fail with it"""
    L, c = 150, 0.6
    gene = gene_of(31 * k, n_bases)
    h, meta = build(monkeypatch, gene, k, bf_bits, c=c)
    keys = h.debug_index_array("kxkeys")
    codes = (np.searchsorted(synth.ACGT, gene)).astype(np.uint8)
    fw, rc = canonical_kmers(codes, k)
    own = np.unique(np.minimum(fw, rc)[:len(gene) - k + 1])
    colliders = np.setdiff1d(keys, own)
    assert meta["n_set"] <= len(own) <= 1.01 * meta["n_set"]
    assert 0.8 * len(own) * 4 ** k / 2 / bf_bits < len(colliders) < 1.2 * len(own) * 4 ** k / 2 / bf_bits, (len(own), len(colliders))
    rng = np.random.default_rng(k)
    m1, m2, with_collider = [], [], []
    for G in range(30 - k - 2, 33):
        for rep in range(8):
            a = int(rng.integers(0, len(gene) - 400))
            tail = synth.random_seq(rng, L - G - k)
            for use in (True, False):
                kmer = np.frombuffer(kmer_bytes(colliders[int(rng.integers(0, len(colliders)))], k), dtype=np.uint8) if use else synth.random_seq(rng, k)
                if use and rep % 2:
                    kmer = synth.revcomp(kmer)
                m1.append(gene[a:a + L].copy())
                m2.append(np.concatenate([gene[a + 200:a + 200 + G], kmer, tail]))
                with_collider.append(use)
    batch = synth.batch_from_lists(m1, m2)
    n = len(m1)
    assert 200 <= n <= 700
    o = oracle_for(oracle, gene, k, bf_bits, c)
    want = o.classify(*args(batch), nthreads=2)
    assigned = np.diff(want[0].astype(np.int64)) > 0
    use = np.array(with_collider)
    # the construction does what it says: in pairs that differ only in the k-mer behind the gene's bases, the colliding one decides
    flips = int(np.sum(assigned[0::2] & ~assigned[1::2]))
    assert flips >= 20, flips
    assert np.any(~assigned[use]) and np.any(assigned[~use])
    same(h.classify(*args(batch)), want, "k-mer table")
    assert "+three-pairs" in h.last_kernel()
    h.close()
    h2, _ = build(monkeypatch, gene, k, bf_bits, c=c, env={"SHK_NO_KMER_TABLE": "1"}, expect_kx=False)
    same(h2.classify(*args(batch)), want, "SHK_NO_KMER_TABLE=1")
    h2.close()


# ---------------------------------------------------------------------------
# 4. every route of a one-gene index, and where a read sits in its batch
# ---------------------------------------------------------------------------
GENE17 = gene_of(1717, 20000)
_batches = {}


def batches17(oracle):
    """20 000 pairs, 50 % on-target, 1 % substitutions and N: 2 x 150 bp, and the same stream at mixed lengths; with the oracle's answers"""
    if not _batches:
        o = oracle_for(oracle, GENE17, 17, 1 << 33)
        for name, var in (("uniform", False), ("trimmed", True)):
            b = synth.make_reads(np.random.default_rng(17), [GENE17], 20000, read_len=150, on_target=0.5, sub_rate=0.01, n_rate=0.002, var_len=var)
            want = o.classify(*args(b), nthreads=4)
            assert 5000 < int(want[0][-1]) < 11000
            _batches[name] = (b, want)
    return _batches


ROUTES = [
    ("uniform+tiles", "uniform", {"SHK_TILE_FIRST": "1"}, ("+three-pairs", "+tiles-first")),
    ("uniform", "uniform", {"SHK_TILE_FIRST": "0"}, ("+three-pairs",)),
    ("uniform-one-pair", "uniform", {"SHK_NO_TRI": "1"}, (", 21, true>",)),
    ("offsets+tiles", "trimmed", {"SHK_TILE_FIRST": "1"}, ("offsets", "+tiles-first")),
    ("offsets", "trimmed", {"SHK_TILE_FIRST": "0"}, ("offsets",)),
    ("class-by-class", "trimmed", {"SHK_CLS_MIN_FILL": "1", "SHK_NO_TRO": "1"}, ("verdict=classes",)),
    ("ragged", "trimmed", {"SHK_CLS_MIN_FILL": "0", "SHK_NO_TRO": "1"}, (", 21, false>",)),
]


@pytest.mark.parametrize("name,kind,env,says", ROUTES, ids=[r[0] for r in ROUTES])
def test_routes_of_a_one_gene_index(oracle, monkeypatch, name, kind, env, says):
    batch, want = batches17(oracle)[kind]
    h, meta = build(monkeypatch, GENE17, 17, 1 << 33, env=env)
    assert 38000 < meta["kx_keys"] < 42000, meta
    same(h.classify(*args(batch)), want, name)
    lk = h.last_kernel()
    for s in says:
        assert s in lk, (name, s, lk)
    same(h.classify(*args(batch)), want, (name, "second batch"))      # (the stream's history picks the tiles' round by itself now)
    h.close()
    h2, _ = build(monkeypatch, GENE17, 17, 1 << 33, env=dict(env, SHK_NO_KMER_TABLE="1"), expect_kx=False)
    same(h2.classify(*args(batch)), want, (name, "switch off"))
    for s in says:
        assert s in h2.last_kernel(), (name, s, h2.last_kernel())
    h2.close()


def test_where_a_read_sits_in_its_batch(oracle, monkeypatch):
    """single-end; pair counts that are no multiple of the three pairs a staging pass takes; batches of 1, 2, 3 and 4"""
    batch, want = batches17(oracle)["uniform"]
    o = oracle_for(oracle, GENE17, 17, 1 << 33)
    h, _ = build(monkeypatch, GENE17, 17, 1 << 33)
    off1, off2 = batch["off1"].astype(np.int64), batch["off2"].astype(np.int64)

    def head(first, n, paired=True):
        s1 = batch["seq1"][off1[first]:off1[first + n]]
        o1 = (off1[first:first + n + 1] - off1[first]).astype(np.uint64)
        if not paired:
            return s1, o1, None, None
        return s1, o1, batch["seq2"][off2[first]:off2[first + n]], (off2[first:first + n + 1] - off2[first]).astype(np.uint64)

    for first, n in ((0, 1), (1, 2), (3, 3), (6, 4), (100, 1000), (2000, 1001), (4000, 1003 + 1)):
        sub = head(first, n)
        same(h.classify(*sub), o.classify(*sub, nthreads=2), (first, n))
    for first, n in ((0, 1), (5, 2), (7, 4), (3000, 2000)):
        sub = head(first, n, paired=False)
        w = o.classify(*sub, nthreads=2)
        same(h.classify(*sub), w, ("single-end", first, n))
        if n == 2000:
            assert 300 < int(w[0][-1]) < 1100 and ", 21, " in h.last_kernel(), h.last_kernel()
    h.close()
