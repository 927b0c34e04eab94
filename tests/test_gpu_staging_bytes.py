"""Staging (stage_bases.hpp: ASCII bases -> two streams of 2-bit codes + validity bits) on every kernel that stages, byte value by byte
value: a byte taken for a base that is none, or for none that is one, must change a result.

One gene of 6 000 bases, k = 17, c = 0.6, 2^33 bits.  A batch of a shape (L1, L2) holds, per pair compared with the oracle:
  * knife-edge pairs: gene bases in one run per mate, x bases in all, between bases that differ from the gene's; inside mate 1's run
    one byte is replaced by the value v at a place where the gene's base has v's 2-bit code.  v one of ACGTacgt: the base itself,
    perhaps in the other case -- the pair covers x of len = L1 + L2.  Any other v: the run falls apart into two pieces that cover
    x - 1 of len - 1.  x is chosen so that the coverage is exactly ceil(c * len), and one below it: for EVERY one of the 256 values
    both outcomes occur (the oracle's analyze() confirms coverage and len of each such pair; no value is left out -- the oracle's
    batch interface takes every byte).  An invalid v taken for valid bridges the two pieces (its code is the gene's base's): the
    pair one below passes.  A valid v taken for invalid breaks the run: the pair on the threshold fails.
  * ordinary pairs from the gene and from elsewhere with one byte replaced by each of the 256 values at a random place;
  * whole reads, whole mates and single bases in lower case;
  * the one-bit neighbours of ACGT and acgt, 0x00, 0x7F, 0x80 | base and 0xFF scattered several to a pair.
Routes: 2 x 150 through the three-pairs kernel on the k-mer keyed table (with the tiles' round and without) and on its hashed twin
(SHK_NO_KMER_TABLE=1); 2 x 100 (the one-pair kernel, 8 bases per lane); single-end 150; three
genes; mixed lengths through the offsets form; min_quality = 20 with qualities (knife-edge pairs on the quality character as well:
masked iff it is below 53 as a signed char); a table-mode index of 300 genes (SHK_NO_LDS_TABLE=1) run twice, anchor_verdict_kernel in
front; SHK_FORCE_GENERIC=1 (process_read).  Every route runs its batch with the buffers at byte shifts 0 .. 3; last_kernel() is
asserted per run.

Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import torch  # noqa: F401  (torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both)

from tests import synth, views

pytestmark = pytest.mark.gpu

SWITCHES = ("SHK_PROBE", "SHK_NO_LDS_TABLE", "SHK_FORCE_GENERIC", "SHK_KTAB", "SHK_NO_LDS_SUMMARY", "SHK_NO_SUMMARY", "SHK_TILE_FIRST", "SHK_NO_TRI",
            "SHK_NO_TRO", "SHK_CLS_MIN_FILL", "SHK_NO_SPARSE", "SHK_FORCE_TRO", "SHK_NO_KMER_TABLE", "SHK_ANCHOR_ALWAYS", "SHK_NO_ANCHOR",
            "SHK_NO_PRE_VERDICT", "SHK_NO_REFEXT")
K, C, BF = 17, 0.6, 1 << 33
BASES = b"ACGTacgt"
# the one-bit neighbours of the eight bases, 0x00, 0x7F, 0x80 | base, 0xFF
NEAR = sorted({b ^ (1 << i) for b in BASES for i in range(8)} | {0x00, 0x7F, 0xFF} | {0x80 | b for b in BASES})
MQ = 20 + 33                                              # a quality character below it, as a signed char, masks its base
QCHARS = (MQ - 1, MQ, 33, 0x7F, 0x80, 0xFF, 0x00, MQ + 1, 0xB5)


def thr_of(length):
    """the smallest integer t with (double)t >= c * (double)len (ReadAnalyzer.hpp:104)"""
    x = C * float(length)
    t = int(x)
    return t if float(t) >= x else t + 1


def code_of(v):
    t = v & 0xDF
    return ((t >> 1) ^ (t >> 2)) & 3


def is_base(v):
    return v in BASES


def masked(q):
    return (q - 256 if q >= 128 else q) < MQ


def reference(n_genes):
    """gene 0: 6 000 bases; the others 1 to 3 kb"""
    rng = np.random.default_rng(4242)
    first = synth.random_seq(rng, 6000)
    return [first] + [synth.random_seq(rng, int(rng.integers(1000, 3000))) for _ in range(n_genes - 1)]


# ---------------------------------------------------------------------------
# pairs
# ---------------------------------------------------------------------------
def knife_pair(rng, genes, L1, L2, v, below, by_quality=False):
    """(m1, m2 or None, q1, q2, len, coverage) -- see the module's text.  by_quality: the byte stays the gene's base and v is the
    quality character at its place (qualities are phred 40 elsewhere)"""
    total = L1 + L2
    breaks = masked(v) if by_quality else not is_base(v)
    length = total - (1 if breaks else 0)
    target = thr_of(length) - below
    x = target + (1 if breaks else 0)
    for _ in range(200):
        if L2:
            lo, hi = max(2 * K + 1, x - (L2 - 2)), min(L1 - 2, x - K)
            assert lo <= hi, (L1, L2, x)
            xa = int(rng.integers(lo, hi + 1))
            runs = [(0, "mid", xa), (1, "mid", x - xa)]
        else:
            xa = x
            runs = [(0, "mid", xa)]
        m1, m2, info, _ = views._pair(rng, genes, K, L1, L2 if L2 else 1, runs, gene=0)
        _, p, _, _, _ = info[0]
        # places inside mate 1's run with k bases of it on either side at least
        cand = [j for j in range(p + K, p + xa - K) if by_quality or code_of(int(m1[j])) == code_of(v)]
        if is_base(v) and not by_quality:
            cand = [j for j in cand if (int(m1[j]) & 0xDF) == (v & 0xDF)]
        if not cand:
            continue
        j = cand[int(rng.integers(0, len(cand)))]
        q1 = q2 = None
        if by_quality:
            q1, q2 = np.full(L1, views.HI_Q, np.uint8), (np.full(L2, views.HI_Q, np.uint8) if L2 else None)
            q1[j] = v
        else:
            m1[j] = v
        return m1, (m2 if L2 else None), q1, q2, length, target
    raise AssertionError("no place for the byte %#x" % v)


def plain_pair(rng, gene, L1, L2, from_gene):
    if from_gene:
        a = int(rng.integers(0, len(gene) - L1 - L2 - 60))
        m1 = gene[a:a + L1].copy()
        m2 = synth.revcomp(gene[a + L1 + 50:a + L1 + 50 + L2]) if L2 else None
        if L2 == L1 and rng.integers(0, 2):
            m1, m2 = m2, m1
    else:
        m1, m2 = synth.random_seq(rng, L1), (synth.random_seq(rng, L2) if L2 else None)
    return m1, m2


def put(rng, m1, m2, v):
    m = m2 if (m2 is not None and rng.integers(0, 2)) else m1
    m[int(rng.integers(0, len(m)))] = v


def build_case(oracle, key, n_genes, shape, q=0, trim=False):
    """(batch, the oracle's answer, the knife-edge pairs' [(index, value, assigned)])"""
    L1, L2 = shape
    genes = reference(n_genes)
    rng = np.random.default_rng([L1, L2, n_genes, q, int(trim)])
    o = oracle.Shark(k=K, c=C, bf_bits=BF, min_quality=q)
    o.build([bytes(g) for g in genes])
    reads, knife = [], []

    def add(m1, m2, q1=None, q2=None, noisy=True):
        if q and q1 is None:
            q1 = np.full(len(m1), views.HI_Q, np.uint8)
            q2 = np.full(len(m2), views.HI_Q, np.uint8) if m2 is not None else None
            for qq in (q1, q2):          # a few masked bases anywhere, and quality characters of both signs
                if noisy and qq is not None and rng.integers(0, 2):
                    qq[rng.integers(0, len(qq), size=3)] = [QCHARS[int(i)] for i in rng.integers(0, len(QCHARS), size=3)]
        reads.append((m1, m2, q1, q2))

    def lengths():
        """(trimmed batches) a pair's own lengths"""
        if not trim:
            return L1, L2
        return int(rng.integers(L1 - 30, L1 + 1)), int(rng.integers(L2 - 30, L2 + 1))

    def knife_of(v, below, by_quality=False):
        l1, l2 = lengths()
        m1, m2, q1, q2, length, target = knife_pair(rng, genes, l1, l2, v, below, by_quality)
        joined = m1.copy()
        if by_quality:
            joined[np.array([masked(int(c)) for c in q1], bool)] = ord("N")
        read = bytes(joined) + (b"N" + bytes(m2) if m2 is not None else b"")
        got, mx, _, ln = o.analyze(read)
        assert ln == length and mx == target, (hex(v), below, by_quality, mx, target, ln, length)
        assert (0 in got) == (below == 0), (hex(v), below, got)
        knife.append((len(reads), v, below == 0, by_quality))
        add(m1, m2, q1, q2, noisy=False)

    for v in range(256):
        for below in (0, 1):
            knife_of(v, below)
    if q:
        for v in QCHARS:
            for below in (0, 1):
                knife_of(v, below, by_quality=True)
    for v in range(256):                                   # one byte replaced, anywhere
        l1, l2 = lengths()
        m1, m2 = plain_pair(rng, genes[0], l1, l2, from_gene=bool(v & 1) ^ bool(v & 2))
        put(rng, m1, m2, v)
        add(m1, m2)
    for i in range(48):                                    # lower case: whole reads, whole mates, single bases, one base in twenty
        l1, l2 = lengths()
        m1, m2 = plain_pair(rng, genes[0], l1, l2, from_gene=i % 3 != 0)
        kind = i % 4
        for j, m in enumerate((m1, m2)):
            if m is None:
                continue
            if kind == 0 or (kind == 1 and j == i // 4 % 2):
                m |= 0x20
            elif kind == 2:
                m[int(rng.integers(0, len(m)))] |= 0x20
            elif kind == 3:
                m[rng.random(len(m)) < 0.05] |= 0x20
        add(m1, m2)
    for i in range(96):                                    # the near misses, several to a pair
        l1, l2 = lengths()
        m1, m2 = plain_pair(rng, genes[0], l1, l2, from_gene=i % 3 != 0)
        for _ in range(1 + i % 5):
            put(rng, m1, m2, NEAR[int(rng.integers(0, len(NEAR)))])
        add(m1, m2)
    if n_genes > 1:                                        # the other genes' reads
        for i in range(64):
            g = genes[1 + i % (n_genes - 1)]
            l1, l2 = lengths()
            a = int(rng.integers(0, len(g) - l1 - l2))
            m1, m2 = g[a:a + l1].copy(), (synth.revcomp(g[a + l1:a + l1 + l2]) if L2 else None)
            put(rng, m1, m2, NEAR[i % len(NEAR)])
            add(m1, m2)
    # (the knife-edge pairs stay where they are: the first; the rest is shuffled among itself, so that triples mix kinds)
    nk = len(knife)
    order = list(range(nk)) + [nk + int(j) for j in rng.permutation(len(reads) - nk)]
    reads = [reads[j] for j in order]
    batch = views.batch_of(reads)
    ans = o.classify(batch["seq1"], batch["off1"], batch["seq2"], batch["off2"], batch["qual1"], batch["qual2"], nthreads=4)
    o.close()
    assigned = np.diff(ans[0].astype(np.int64)) > 0
    # every value, both outcomes -- in the batch's own answer too
    seen = {}
    for i, v, want, byq in knife:
        assert bool(assigned[i]) == want, (key, i, hex(v), want, byq)
        seen.setdefault((v, byq), set()).add(want)
    assert all(s == {True, False} for s in seen.values()) and {v for v, byq in seen if not byq} == set(range(256))
    if q:
        assert {v for v, byq in seen if byq} == set(QCHARS)
    assert 0.2 < assigned.mean() < 0.8, assigned.mean()
    return batch, ans, knife


_made = {}
TABLE_MODES = ("table", "summary+table", "minimiser-table")       # no table and no summary in LDS: anchor_verdict_kernel applies


def case(oracle, key, *a, **kw):
    if key not in _made:
        _made[key] = build_case(oracle, key, *a, **kw)
    return _made[key]


# ---------------------------------------------------------------------------
# running
# ---------------------------------------------------------------------------
def make_handle(monkeypatch, n_genes, env=None, q=0, mode=("lds-table",), kx=None):
    from shark_amd import SharkHip
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for name, val in (env or {}).items():
        monkeypatch.setenv(name, val)
    h = SharkHip(k=K, c=C, bf_bits=BF, min_quality=q)
    h.build([bytes(g) for g in reference(n_genes)])
    assert h.probe_mode() in mode, h.probe_mode()
    if kx is not None:
        assert h.debug_kx_meta()["kx_in_use"] == kx
    return h


def max_len(batch):
    m = int(np.diff(batch["off1"].astype(np.int64)).max())
    return max(m, int(np.diff(batch["off2"].astype(np.int64)).max())) if batch["off2"] is not None else m


def resident(h, batch, shifts):
    """classify_device on the batch's arrays at these byte displacements inside larger ones -> (gene_off, gene_ids)"""
    from shark_amd import capi
    e = views.embed(batch, shifts)
    keep, p = views.to_device(e)
    r = h.classify_device(e["n"], p["seq1"], p["off1"], p["seq2"], p["off2"], p["qual1"], p["qual2"], max_read_len=max_len(batch))
    n, tot = int(r.n), int(r.n_assoc)
    goff, gids = np.zeros(n + 1, np.uint32), np.zeros(tot, np.uint16)
    capi.hip_memcpy_dtoh(goff, r.gene_off, goff.nbytes)
    if tot:
        capi.hip_memcpy_dtoh(gids, r.gene_ids, gids.nbytes)
    del keep
    return goff, gids


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "gene_off differs at read %d" % int(np.argmax(got[0][:len(want[0])] != want[0])))
    assert np.array_equal(got[1], want[1]), what


# (seq1, seq2) shifts, the qualities at other ones; last the aligned control
SHIFTS = [views.shifts_of(s1, s2, (s1 + 1) % 4, (s2 + 2) % 4) for s1, s2 in ((1, 3), (2, 1), (3, 2), (0, 0))]


def run(h, batch, want, what, says=(), says_not=(), shifts=SHIFTS):
    for sh in shifts:
        same(resident(h, batch, sh), want, (what, sh["seq1"] - views.PAD, sh["seq2"] - views.PAD))
        lk = h.last_kernel()
        for s in says:
            assert s in lk, (what, s, lk)
        for s in says_not:
            assert s not in lk, (what, s, lk)


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
ONE_GENE = [
    ("kx-tiles", {"SHK_TILE_FIRST": "1"}, 1, ("classify_uni_kernel<5, ", "+three-pairs", "+tiles-first", "verdict=uniform"), ()),
    ("kx", {"SHK_TILE_FIRST": "0"}, 1, ("classify_uni_kernel<5, ", "+three-pairs", "verdict=uniform"), ("+tiles-first",)),
    ("hashed-tiles", {"SHK_TILE_FIRST": "1", "SHK_NO_KMER_TABLE": "1"}, 0, ("classify_uni_kernel<5, ", "+three-pairs", "+tiles-first"), ()),
    ("hashed", {"SHK_TILE_FIRST": "0", "SHK_NO_KMER_TABLE": "1"}, 0, ("classify_uni_kernel<5, ", "+three-pairs"), ("+tiles-first",)),
]


@pytest.mark.parametrize("name,env,kx,says,says_not", ONE_GENE, ids=[r[0] for r in ONE_GENE])
def test_three_pairs_2x150_at_every_byte_shift(oracle, monkeypatch, name, env, kx, says, says_not):
    """sixteen bases per lane (stage16): the k-mer keyed kernel and its hashed twin, with the tiles' round and without"""
    batch, want, _ = case(oracle, "2x150", 1, (150, 150))
    h = make_handle(monkeypatch, 1, env=env, kx=kx)
    run(h, batch, want, name, says, says_not)
    h.close()


@pytest.mark.parametrize("shape,u", [((100, 100), 3), ((150, 0), 3)], ids=["2x100", "single-150"])
def test_other_shapes(oracle, monkeypatch, shape, u):
    """2 x 100: three pairs do not share a staging pass, the one-pair kernel stages eight bases per lane (stage8); single-end 150 bp:
    the three-pairs kernel at U = 3"""
    batch, want, _ = case(oracle, "%dx%d" % shape, 1, shape)
    h = make_handle(monkeypatch, 1, kx=1)
    run(h, batch, want, shape, ("classify_uni_kernel<%d, " % u, "verdict=uniform"))
    h.close()


def test_three_genes(oracle, monkeypatch):
    """the several-genes form (LXM)"""
    batch, want, _ = case(oracle, "three-genes", 3, (150, 150))
    assert len(set(want[1].tolist())) == 3
    h = make_handle(monkeypatch, 3, kx=0)
    run(h, batch, want, "three genes", ("classify_uni_kernel<5, ", "+three-pairs", "+sparse-first-rounds"))
    h.close()


def test_mixed_lengths_through_the_offsets_form(oracle, monkeypatch):
    batch, want, _ = case(oracle, "trimmed", 1, (150, 150), trim=True)
    h = make_handle(monkeypatch, 1, env={"SHK_TILE_FIRST": "1"}, kx=1)
    run(h, batch, want, "trimmed", ("offsets", "+three-pairs"))
    h.close()


def test_qualities(oracle, monkeypatch):
    """min_quality = 20: the one-pair kernel with qualities -- the mask of a lane's eight quality characters goes through gather8"""
    batch, want, _ = case(oracle, "q20", 1, (150, 150), q=20)
    h = make_handle(monkeypatch, 1, q=20)
    run(h, batch, want, "q20", ("classify_uni_kernel<", ", true, 21, "), ("+three-pairs",))
    h.close()


def test_table_mode_with_the_anchor_verdict_in_front(oracle, monkeypatch):
    """300 genes, no table in LDS: anchor_verdict_kernel (32 bases per lane) in front of the table kernel, for the second batch too --
    the first one's share of assigned reads keeps it on"""
    batch, want, _ = case(oracle, "table", 300, (150, 150))
    h = make_handle(monkeypatch, 300, env={"SHK_NO_LDS_TABLE": "1"}, mode=TABLE_MODES)
    for turn in (0, 1):
        run(h, batch, want, ("table", turn), ("classify_uni_kernel<", "+anchored-extension", "+pre-verdict"))
    h.close()


def test_table_mode_with_qualities(oracle, monkeypatch):
    """the same with min_quality = 20: anchor_verdict_kernel's quality mask (qmask_of)"""
    batch, want, _ = case(oracle, "table-q", 300, (150, 150), q=20)
    h = make_handle(monkeypatch, 300, env={"SHK_NO_LDS_TABLE": "1"}, q=20, mode=TABLE_MODES)
    for turn in (0, 1):
        run(h, batch, want, ("table-q", turn), ("classify_uni_kernel<", "+pre-verdict"))
    h.close()


@pytest.mark.parametrize("key,shape,q", [("2x150", (150, 150), 0), ("q20", (150, 150), 20)], ids=["plain", "q20"])
def test_the_generic_path(oracle, monkeypatch, key, shape, q):
    """SHK_FORCE_GENERIC=1: process_read (classify.hip) stages the batch"""
    batch, want, _ = case(oracle, key, 1, shape, q=q)
    h = make_handle(monkeypatch, 1, env={"SHK_FORCE_GENERIC": "1"}, q=q)
    run(h, batch, want, ("generic", key), ("classify_fast_kernel<",), ("classify_uni_kernel",))
    h.close()
