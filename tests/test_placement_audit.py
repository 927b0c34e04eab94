"""The placement table's auditor (tests/placement_audit.py) without a GPU: its numpy model against the pure-Python definition
(tests/placement_model.py) pair by pair, its hash port against the oracle's XXH64, the seeded collision search, and seeded defects
over the model's own arrays -- each must produce a finding, the clean arrays none."""
import numpy as np
import pytest

from tests import placement_audit as pa
from tests.placement_model import PlacementModel

SMALL = [pytest.param(c, id=c["id"]) for c in pa.CASES if c["small"]]


@pytest.mark.parametrize("c", SMALL)
def test_the_two_models_agree_pair_by_pair(c, oracle, example_dir):
    recs = c["ref"](c["k"], example_dir)
    m = pa.TableModel(recs, c["k"])
    assert pa.declared(m, c["needs"]) == []
    if c["check"]:
        c["check"](m, c["k"])
    pm = PlacementModel(recs, c["k"])
    want = {}
    for g in pm.records:
        for canon, occ in pm.kmer_map(g).items():
            want[(g, canon)] = (len(occ),) + (occ[0] if len(occ) == 1 else ())
    got = {}
    for g, canon, cnt, z in zip(m.gene.tolist(), m.canon.tolist(), m.count.tolist(), m.z.tolist()):
        assert (g, canon) not in got
        got[(g, canon)] = (cnt,) + ((z & 0x7FFFFFFF, z >> 31) if cnt == 1 else ())
        assert (z == pa.AMBIGUOUS) == (cnt > 1)
    assert got == want
    # gene_start: the records' lengths under the ids gene_records gives them, an id without a record has length 0
    lens = np.diff(m.gene_start.astype(np.int64))
    assert len(lens) == m.nidx and {g: int(n) for g, n in enumerate(lens) if n} == {g: len(r) for g, r in pm.records.items()}
    assert m.ids_without_record == m.nidx - len(pm.records)
    # the table's order and the directory, restated entry by entry
    key = list(zip(m.hash.tolist(), m.first.tolist()))
    assert key == sorted(key) and len(set(key)) == m.n
    assert m.lg >= 6 and (1 << m.lg) >= 2 * m.n and (m.lg == 6 or (1 << (m.lg - 1)) < 2 * m.n)
    bucket = [h >> (32 - m.lg) for h in m.hash.tolist()]
    for b in (0, 1, (1 << m.lg) // 3, (1 << m.lg) - 1, 1 << m.lg):
        assert m.pdir[b] == sum(x < b for x in bucket)
    assert m.pdir[(1 << m.lg) + 1] == 0 and len(m.pdir) == (1 << m.lg) + 2


def test_the_first_position_is_the_smallest_global_one(oracle):
    #        0         1         2
    #        0123456789012345678901234
    r2 = b"ACGTTGCATGGACCTAACGTTGAGC"         # k = 5: ACGTT at 0 and 16 and as AACGT at 15, CGTTG at 1 and 17
    m = pa.TableModel([b"GGG", r2, b"NNNNNNN", r2[:8]], 5)
    assert m.nidx == 3 and m.gene_start.tolist() == [0, 0, 25, 33] and m.ids_without_record == 1
    acgtt = int("".join(str("ACGT".index(c)) for c in "AACGT"), 4)
    e = m.entry_of([1, 2, 0, 1], [acgtt, acgtt, acgtt, 0])
    assert e[2] == -1 and e[3] == -1
    assert (m.count[e[0]], m.z[e[0]], m.first[e[0]]) == (3, pa.AMBIGUOUS, 3)
    assert (m.count[e[1]], m.z[e[1]], m.first[e[1]]) == (1, 0, 3 + 25 + 7)          # ACGTT is not the canonical form: orientation 0, x = 0


def test_hash_port_equals_the_oracles_xxh64(oracle):
    L = oracle.lib()
    rng = np.random.default_rng(5)
    canon = np.concatenate([rng.integers(0, 1 << 62, size=300, dtype=np.uint64), np.array([0, 1, (1 << 62) - 1], dtype=np.uint64)])
    gene = np.concatenate([rng.integers(0, 65536, size=300), [0, 65535, 7]])
    word = pa.combined_word(gene, canon)
    assert int(word[0]) == int(canon[0]) ^ (((int(gene[0]) + 1) * 0x9E3779B185EBCA87) & (2 ** 64 - 1))
    want = [L.so_get_hash(int(w)) for w in word]
    assert pa.xxh64_u64(word).tolist() == want
    assert pa.pl_hash32(gene, canon).tolist() == [w >> 32 for w in want]


@pytest.mark.parametrize("k", pa.COLLISION_KS)
def test_collision_search_is_deterministic_and_finds_a_pair(oracle, k):
    L = oracle.lib()
    found = pa.find_collision(k)
    assert found is not None and found == pa.find_collision(k)
    a, b = found
    assert a != b and max(a, b) < 4 ** k
    for v in (a, b):                                                                     # canonical, not palindromic
        assert v < L.so_revcompl(v, k)
    h = [L.so_get_hash(int(pa.combined_word(0, v))) >> 32 for v in (a, b)]
    assert h[0] == h[1]
    across = pa.find_collision(k, 0, 1)
    assert across is not None and across == pa.find_collision(k, 0, 1)
    ha = L.so_get_hash(int(pa.combined_word(0, across[0]))) >> 32
    hb = L.so_get_hash(int(pa.combined_word(1, across[1]))) >> 32
    assert ha == hb


# ---------------------------------------------------------------------------
# seeded defects
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean(oracle):
    """a reference with every structure the defects need: the interleaved collision, repeats, records without an id"""
    k = 17
    recs = pa.ref_collision_interleaved(k) + pa.ref_short_records(k) + pa.ref_repeats(k)[:8] + pa.ref_both_strands(k)
    m = pa.TableModel(recs, k)
    assert m.n_ambiguous > 0 and m.n_hash_groups > 0 and m.ids_without_record > 0
    return m


def _arrays(m, ent=None, lg=None, pdir=None):
    """read-back arrays for these entries ((n, 4) words); the directory is the one pl_dir_kernel would write for them"""
    ent = m.ptab if ent is None else ent
    lg = m.lg if lg is None else lg
    if pdir is None:
        pdir = pa.make_pdir(pa.pl_hash32(ent[:, 3], ent[:, 0].astype(np.uint64) | (ent[:, 1].astype(np.uint64) << np.uint64(32))), lg)
    spare = np.full(4, 0xDEADBEEF, dtype=np.uint32)                                      # (the spare entry is never written)
    return {"ptab": np.concatenate([ent.ravel(), spare]), "pdir": pdir}, {"ptab_lg": lg, "ptab_n": len(ent)}


def _audit(m, ent=None, lg=None, pdir=None, gene_start=None):
    arrays, pmeta = _arrays(m, ent, lg, pdir)
    return pa.audit(arrays, pmeta, m.gene_start if gene_start is None else gene_start, m)


def _has(findings, *words):
    return any(all(w in f for w in words) for f in findings)


def test_clean_arrays_give_no_finding(clean):
    assert _audit(clean) == []
    assert np.array_equal(_arrays(clean)[0]["pdir"], clean.pdir)


def test_an_entry_dropped(clean):
    m = clean
    for j in (0, m.n // 2, m.n - 1):
        f = _audit(m, np.delete(m.ptab, j, axis=0))
        assert _has(f, "ptab[%d]:" % j, "is missing") and _has(f, "ptab_n") and _has(f, "lookup", "not found"), f


def test_an_entry_duplicated(clean):
    m = clean
    j = m.n // 3
    f = _audit(m, np.insert(m.ptab, j, m.ptab[j], axis=0))
    assert _has(f, "appears 2 times") and _has(f, "lookup", "found 2 times") and _has(f, "out of order"), f


def test_unique_and_ambiguous_flipped(clean):
    m = clean
    u, a = np.flatnonzero(m.count == 1)[5], np.flatnonzero(m.count > 1)[2]
    ent = m.ptab.copy()
    ent[u, 2] = pa.AMBIGUOUS
    f = _audit(m, ent)
    assert _has(f, "ptab[%d]:" % u, "z word ambiguous, expected x=") and _has(f, "lookup", "answers ambiguous"), f
    ent = m.ptab.copy()
    ent[a, 2] = int(m.first[a])                                                          # (as if the first window were the only one)
    f = _audit(m, ent)
    assert _has(f, "ptab[%d]:" % a, "expected ambiguous") and _has(f, "lookup", "expected ambiguous"), f


def test_orientation_and_x(clean):
    m = clean
    u = np.flatnonzero(m.count == 1)
    for j, delta in ((u[0], 1 << 31), (u[-1], 1 << 31), (u[7], 1), (u[len(u) // 2], -1 & 0xFFFFFFFF)):
        ent = m.ptab.copy()
        ent[j, 2] = (int(ent[j, 2]) ^ delta) if delta == 1 << 31 else (int(ent[j, 2]) + delta) & 0xFFFFFFFF
        if ent[j, 2] == m.ptab[j, 2]:
            continue
        f = _audit(m, ent)
        assert _has(f, "ptab[%d]:" % j, "z word x=") and _has(f, "lookup", "answers"), f


def test_gene_word_wrong(clean):
    m = clean
    j = m.n // 5
    ent = m.ptab.copy()
    ent[j, 3] += 1
    f = _audit(m, ent, pdir=m.pdir)                                                      # (the directory as the right entries give it)
    assert _has(f, "ptab[%d]: gene %d, expected %d" % (j, m.gene[j] + 1, m.gene[j])) and _has(f, "is missing") and _has(f, "lookup", "not found"), f


def test_entries_swapped(clean):
    m = clean
    same = np.flatnonzero(m.hash[1:] == m.hash[:-1])
    assert len(same)
    j = same[0]                                                                          # two entries of one hash group
    ent = m.ptab.copy()
    ent[[j, j + 1]] = ent[[j + 1, j]]
    f = _audit(m, ent)
    assert f and all("out of order" in x for x in f) and _has(f, "ptab[%d]:" % (j + 1)), f   # (the lookup still finds both)
    bucket = m.hash >> (32 - m.lg)
    two = np.flatnonzero((bucket[1:] == bucket[:-1]) & (m.hash[1:] != m.hash[:-1]))
    assert len(two)
    j = two[0]                                                                           # one bucket, different hashes
    ent = m.ptab.copy()
    ent[[j, j + 1]] = ent[[j + 1, j]]
    f = _audit(m, ent)
    assert f and all("out of order" in x for x in f) and _has(f, "ptab[%d]:" % (j + 1)), f


def test_directory_defects(clean):
    m = clean
    nb = 1 << m.lg
    b = int(m.hash[m.n // 2] >> (32 - m.lg))                                             # a bucket that holds an entry
    pdir = m.pdir.copy()
    pdir[b] += 1
    f = _audit(m, pdir=pdir)
    assert _has(f, "pdir[%d]: %d, expected %d" % (b, pdir[b], m.pdir[b])) and _has(f, "lookup", "not found"), f
    pdir = m.pdir.copy()
    pdir[b + 1] = int(pdir[b + 1]) - 1
    assert _has(_audit(m, pdir=pdir), "pdir[%d]:" % (b + 1))
    empty = int(np.flatnonzero(np.diff(m.pdir[:nb + 1].astype(np.int64)) == 0)[0])       # an empty bucket whose words only the comparison sees
    for at, d in ((nb, -1), (nb, 1), (nb + 1, 1), (0, 1), (empty, 1)):
        pdir = m.pdir.copy()
        pdir[at] = int(pdir[at]) + d
        assert _has(_audit(m, pdir=pdir), "pdir[%d]:" % at), (at, d)


def test_bucket_count_defects(clean):
    m = clean
    assert m.lg > pa.MIN_LG
    f = _audit(m, lg=m.lg - 1)                                                           # a directory that is right for one bit fewer
    assert f == ["pmeta[0]: ptab_lg %d (%d buckets), expected %d" % (m.lg - 1, 1 << (m.lg - 1), m.lg)], f
    assert _has(_audit(m, lg=m.lg + 1), "ptab_lg")
    arrays, pmeta = _arrays(m)
    pmeta["ptab_lg"] -= 1                                                                # ... and one that is not
    assert _has(pa.audit(arrays, pmeta, m.gene_start, m), "pdir[0]:", "words for ptab_lg")
    arrays, pmeta = _arrays(m)
    pmeta["ptab_n"] -= 1
    assert _has(pa.audit(arrays, pmeta, m.gene_start, m), "ptab[0]:", "words for ptab_n")


def test_gene_start_defects(clean):
    m = clean
    gs = m.gene_start.copy()
    gs[3] += 1
    assert _audit(m, gene_start=gs) == ["gene_start[3]: %d, expected %d" % (gs[3], m.gene_start[3])]
    gs = m.gene_start.copy()
    gs[2:] += 5                                                                          # a record's length under the id in front of its own
    f = _audit(m, gene_start=gs)
    assert _has(f, "gene_start[2]:") and _has(f, "gene_start[...]"), f
    assert _has(_audit(m, gene_start=m.gene_start[:-1]), "gene_start[0]:", "entries")


def test_a_foreign_pair_is_found_by_the_absent_sample(clean):
    """an entry the reference does not have, under a gene id the sample asks for: the k-mer of another entry under nidx"""
    m = clean
    ent = np.vstack([m.ptab, m.ptab[:40]])
    ent[m.n:, 3] = m.nidx
    h = pa.pl_hash32(ent[:, 3], ent[:, 0].astype(np.uint64) | (ent[:, 1].astype(np.uint64) << np.uint64(32)))
    ent = ent[np.argsort(h, kind="stable")]
    arrays, pmeta = _arrays(m, ent)
    f = pa.audit(arrays, pmeta, m.gene_start, m, n_absent=40 * m.n)
    assert _has(f, "is not in the reference") and _has(f, "lookup", "is not in the reference and is found"), f
