"""The threshold of a pair with invalid characters in the three-pairs kernel (classify_uni.hpp, THRTAB): a uniform batch's pair reads
ceil(c * (L1 + L2 - n)) from a table the wave fills once, n being the popcount of the pair's share of a ballot over the 16-base chunks
that hold an invalid character -- exact when no chunk holds two; a pair with two in one chunk takes the reduction over the validity
bytes and cov_threshold as before.  No result may depend on which way was taken.

The batches are built so that the reference alone decides:
  * pairs from the gene and from elsewhere with n = 0, 1, 2, 3, 5, 13, 14, 20 invalid characters, each in a chunk of its own (the table)
    and with two of them in one chunk (the reduction), both kinds in one triple;
  * the layout's edges: N at the first and the last base of a chunk and of either mate, in mate 2's last chunk (six bases of the read
    and ten positions behind its end that must not be counted), lower-case bases, non-ACGT bytes other than N;
  * pairs whose coverage is exactly ceil(0.6 * (300 - n)) and one below it, by substitutions -- where a wrong table entry shows; the
    oracle's analyze() confirms coverage and len of every such pair on the CPU, and both sides of the threshold occur;
  * pairs from elsewhere with 13 and 14 invalid characters (the bound cut's spUb < thr_r flips between them at 2 x 150 bp), one pair
    from the gene per triple;
  * the hashed twin, an index of three genes, single-end 150 bp, 2 x 100 bp (which the three-pairs kernel leaves to the one-pair
    kernel, see test_other_lengths), 2 x 96 bp and 2 x 120 bp, an incomplete last triple, and a batch of mixed lengths through the
    offsets form (which keeps its own thresholds) as a control.
Every pair is compared with the oracle.

Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import torch  # noqa: F401  (torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both)

from tests import synth

pytestmark = pytest.mark.gpu

SWITCHES = ("SHK_PROBE", "SHK_NO_LDS_TABLE", "SHK_FORCE_GENERIC", "SHK_KTAB", "SHK_NO_LDS_SUMMARY", "SHK_NO_SUMMARY", "SHK_TILE_FIRST", "SHK_NO_TRI",
            "SHK_NO_TRO", "SHK_CLS_MIN_FILL", "SHK_NO_SPARSE", "SHK_FORCE_TRO", "SHK_NO_KMER_TABLE")
K, C, BF = 17, 0.6, 1 << 33
COUNTS = (0, 1, 2, 3, 5, 13, 14, 20)
OTHER = np.frombuffer(b"RYKMSWBDHVX.-*n@", dtype=np.uint8)      # not ACGT, not N


def thr_of(n, total=300):
    """ceil(0.6 * (total - n)) the way the reference compares: the smallest integer t with (double)t >= c * (double)len"""
    x = C * float(total - n)
    t = int(x)
    return t if float(t) >= x else t + 1


def genes_of(n_genes):
    rng = np.random.default_rng(9100 + n_genes)
    return [synth.random_seq(rng, 6000 if n_genes == 1 else 3000) for _ in range(n_genes)]


# ---------------------------------------------------------------------------
# where the invalid characters go: (mate, position) lists
# ---------------------------------------------------------------------------
def chunks_of(L1, L2):
    """the 16-base chunks of a pair as (mate, first base, bases of the read in it)"""
    out = []
    for mate, Lm in ((0, L1), (1, L2)):
        for b in range(0, Lm, 16):
            out.append((mate, b, min(16, Lm - b)))
    return out


def spots(rng, n, L1, L2, two_in_one, edge=False):
    """n places, one per chunk -- or, two_in_one, n - 1 chunks with two places in one of them.  edge: at a chunk's first or last base"""
    ch = chunks_of(L1, L2)
    two_in_one = two_in_one and n >= 2
    need = n - 1 if two_in_one else n
    assert need <= len(ch)
    out = []
    for i, j in enumerate(rng.permutation(len(ch))[:need]):
        mate, b, nb = ch[j]
        o = (0 if rng.integers(0, 2) else nb - 1) if edge else int(rng.integers(0, nb))
        out.append((mate, b + o))
        if two_in_one and i == 0:
            o2 = (nb - 1 - o) if edge else (o + 1 + int(rng.integers(0, nb - 1))) % nb
            out.append((mate, b + o2))
    assert len(set(out)) == n
    return out


def put(mates, places, byte=ord("N")):
    for mate, p in places:
        mates[mate][p] = byte


def gene_pair(rng, gene, L1, L2):
    a = int(rng.integers(0, len(gene) - 2 * max(L1, L2) - 60))
    m1 = gene[a:a + L1].copy()
    m2 = synth.revcomp(gene[a + L1 + 50:a + L1 + 50 + L2]) if L2 else None
    if rng.integers(0, 2) and L2 == L1:
        m1, m2 = m2, m1
    return [m1, m2] if L2 else [m1]


def elsewhere_pair(rng, L1, L2):
    return [synth.random_seq(rng, L1), synth.random_seq(rng, L2)] if L2 else [synth.random_seq(rng, L1)]


def substitute(m, p):
    m[p] = synth.ACGT[(int(np.searchsorted(synth.ACGT, m[p])) + 1) & 3]


# ---------------------------------------------------------------------------
# a pair from the gene whose coverage is exactly `target`
# ---------------------------------------------------------------------------
BOUNDARY = [(m, p) for p2 in ((15, 16), (47, 48), (79, 80), (111, 112), (143, 144)) for m in (0, 1) for p in p2]   # 20 places, 20 chunks


def on_threshold_pair(rng, gene, n, target, two_in_one):
    """2 x 150 bp of the gene, n invalid characters at chunk boundaries (two_in_one: one of them moved next to another, into its chunk),
    then substitutions that leave runs of intact bases of target bases in all (a run shorter than k covers nothing)"""
    mates = gene_pair(rng, gene, 150, 150)
    places = list(BOUNDARY[:n])
    if two_in_one and n >= 2:
        m, p = places[0]
        places[-1] = (m, p - 1)                  # 14 beside 15: the same chunk
    put(mates, places)
    broken = [np.zeros(150, bool), np.zeros(150, bool)]
    for m, p in places:
        broken[m][p] = True

    def runs():
        out = []
        for m in (0, 1):
            s = 0
            for p in range(151):
                if p == 150 or broken[m][p]:
                    if p - s >= K:
                        out.append((m, s, p - s))
                    s = p + 1
        return out

    def sub(m, p):
        substitute(mates[m], p)
        broken[m][p] = True

    D = sum(r[2] for r in runs()) - target
    assert D >= 0
    for m, s, ln in reversed(runs()):
        if D == 0:
            break
        if D >= ln:
            # the whole run: a substitution every k bases from its (k - 1)-th leaves pieces of k - 1 at most
            for p in range(s + K - 1, s + ln, K):
                sub(m, p)
            D -= ln
        else:
            # its first ln - cut bases stay (k at least), what is behind them goes the same way
            cut = min(D, ln - K)
            if cut == 0:
                continue
            keep = ln - cut
            sub(m, s + keep)
            for p in range(s + keep + K, s + ln, K):
                sub(m, p)
            D -= cut
    assert D == 0 and sum(r[2] for r in runs()) == target, (n, target, D)
    return mates


# ---------------------------------------------------------------------------
# the batches
# ---------------------------------------------------------------------------
def counts_batch(rng, genes, L1, L2, reps, counts=COUNTS):
    """triples of (table, reduction, table / reduction by turns) pairs for every count, from the genes and from elsewhere by turns"""
    m1, m2 = [], []
    nch = len(chunks_of(L1, L2))
    i = 0
    for rep in range(reps):
        for n in counts:
            if n > nch:
                continue
            for slot in range(3):
                two = slot == 1 or (slot == 2 and (i & 1))
                src = (i // 3 + slot) % 3          # two pairs in three from a gene
                mates = gene_pair(rng, genes[i % len(genes)], L1, L2) if src else elsewhere_pair(rng, L1, L2)
                if src == 2:                       # some errors: not every pair ends in the tiles' round
                    for mt in mates:
                        for p in rng.choice(len(mt), size=int(rng.integers(1, 7)), replace=False):
                            substitute(mt, int(p))
                put(mates, spots(rng, n, L1, L2, two, edge=bool(rep & 1)))
                m1.append(mates[0])
                m2.append(mates[1] if L2 else None)
                i += 1
    return m1, m2


def edges_batch(rng, gene):
    m1, m2 = [], []

    def add(mates):
        m1.append(mates[0])
        m2.append(mates[1])

    fixed = [[(0, 0)], [(0, 149)], [(1, 0)], [(1, 149)], [(0, 0), (0, 149), (1, 0), (1, 149)],
             [(1, 144)], [(1, 149), (1, 144)], [(1, 145), (1, 148)], [(1, 143), (1, 144)], [(0, 144), (0, 149), (1, 146)],
             [(0, 16)], [(0, 15)], [(0, 15), (0, 16)], [(0, 16), (0, 31)], [(1, 127), (1, 128), (1, 143)],
             [(m, p) for m in (0, 1) for p in range(144, 150)]]
    for places in fixed:
        for byte in (ord("N"), None):
            for src in (0, 1):
                mates = gene_pair(rng, gene, 150, 150) if src else elsewhere_pair(rng, 150, 150)
                for j, pl in enumerate(places):
                    put(mates, [pl], byte if byte is not None else int(OTHER[(j + len(m1)) % len(OTHER)]))
                add(mates)
    # lower-case bases: alone, and beside invalid characters of both kinds
    for i in range(48):
        mates = gene_pair(rng, gene, 150, 150) if i % 3 else elsewhere_pair(rng, 150, 150)
        for mt in mates:
            lo = rng.random(150) < (0.05 if i & 1 else 0.5)
            mt[lo] |= 0x20
        if i % 4:
            put(mates, spots(rng, i % 7, 150, 150, bool(i & 8)), ord("N") if i & 2 else int(OTHER[i % len(OTHER)]))
        add(mates)
    return m1, m2


def threshold_batch(rng, gene):
    """(mates 1, mates 2, per pair (n, target coverage))"""
    m1, m2, want = [], [], []
    for rep in range(3):
        for n in COUNTS:
            for two in (False, True):
                if two and n < 2:
                    continue
                for below in (0, 1):
                    mates = on_threshold_pair(rng, gene, n, thr_of(n) - below, two)
                    m1.append(mates[0])
                    m2.append(mates[1])
                    want.append((n, thr_of(n) - below))
    return m1, m2, want


def bound_cut_batch(rng, gene):
    m1, m2 = [], []
    for i in range(96):
        for slot in range(3):
            if slot == i % 3:
                mates = gene_pair(rng, gene, 150, 150)
                put(mates, spots(rng, int(rng.integers(0, 3)), 150, 150, False))
            else:
                mates = elsewhere_pair(rng, 150, 150)
                put(mates, spots(rng, 13 + ((i + slot) & 1), 150, 150, bool(i & 2)))
            m1.append(mates[0])
            m2.append(mates[1])
    return m1, m2


_made = {}


def one_gene_case(oracle):
    """made once: the 2 x 150 bp batch of all four parts on the one-gene index, and the oracle's answer"""
    if "one" not in _made:
        gene = genes_of(1)[0]
        rng = np.random.default_rng(77)
        o = oracle.Shark(k=K, c=C, bf_bits=BF)
        o.build([bytes(gene)])
        a1, a2 = counts_batch(rng, [gene], 150, 150, reps=60)
        b1, b2 = edges_batch(rng, gene)
        c1, c2, want = threshold_batch(rng, gene)
        d1, d2 = bound_cut_batch(rng, gene)
        # the threshold pairs, by the oracle alone: len = 300 - n, coverage = the target, assigned iff the target is the threshold
        sides = set()
        for x, y, (n, target) in zip(c1, c2, want):
            genes, mx, _, ln = o.analyze(bytes(x) + b"N" + bytes(y))
            assert ln == 300 - n and mx == target, (n, target, mx, ln)
            assert (len(genes) == 1) == (target == thr_of(n)), (n, target, genes)
            sides.add((n, target == thr_of(n)))
        assert sides == {(n, s) for n in COUNTS for s in (False, True)}
        assert [thr_of(n) for n in COUNTS] == [180, 180, 179, 179, 177, 173, 172, 168]
        m1, m2 = a1 + d1 + b1 + c1, a2 + d2 + b2 + c2          # (the first two are made of triples: they start at a multiple of 3)
        assert len(a1) % 3 == 0 and len(d1) % 3 == 0
        batch = synth.batch_from_lists(m1, m2)
        ans = o.classify(*args(batch), nthreads=4)
        o.close()
        assigned = np.diff(ans[0].astype(np.int64)) > 0
        assert 0.2 < assigned.mean() < 0.8, assigned.mean()
        first = len(a1) + len(d1) + len(b1)
        thr_assigned = assigned[first:first + len(c1)]
        assert np.array_equal(thr_assigned, np.array([t == thr_of(n) for n, t in want]))
        _made["one"] = (batch, ans, len(m1))
    return _made["one"]


def args(b):
    return b["seq1"], b["off1"], b["seq2"], b["off2"]


def head(batch, want, n):
    """the first n reads of a batch and the oracle's answer for them (a read's answer does not depend on its batch)"""
    o1 = batch["off1"].astype(np.int64)
    sub = dict(batch, seq1=batch["seq1"][:o1[n]], off1=batch["off1"][:n + 1].copy())
    if batch["seq2"] is not None:
        o2 = batch["off2"].astype(np.int64)
        sub.update(seq2=batch["seq2"][:o2[n]], off2=batch["off2"][:n + 1].copy())
    goff = want[0].astype(np.int64)
    return sub, (want[0][:n + 1].copy(), want[1][:goff[n]])


def make_handle(monkeypatch, genes, env=None, kmer_table=True):
    from shark_amd import SharkHip
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for name, val in (env or {}).items():
        monkeypatch.setenv(name, val)
    h = SharkHip(k=K, c=C, bf_bits=BF)
    if not kmer_table:
        h.kmer_table(False)
    h.build([bytes(g) for g in genes])
    assert h.probe_mode() == "lds-table", h.probe_mode()
    assert h.debug_kx_meta()["kx_in_use"] == (1 if kmer_table and len(genes) == 1 else 0)
    return h


def on_device(h, batch, max_read_len):
    """the batch through classify_device (device pointers, the bound on a mate's length given) -> (gene_off, gene_ids) on the host"""
    from shark_amd.capi import hip_memcpy_dtoh
    dev = torch.device("cuda:0")
    t = {name: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev) for name, v in batch.items() if v is not None}
    torch.cuda.synchronize()
    g = lambda name: t[name].data_ptr() if name in t else 0  # noqa: E731
    n = len(batch["off1"]) - 1
    r = h.classify_device(n, g("seq1"), g("off1"), g("seq2"), g("off2"), max_read_len=max_read_len)
    tot = int(r.n_assoc)
    goff, gids = np.zeros(n + 1, np.uint32), np.zeros(tot, np.uint16)
    hip_memcpy_dtoh(goff, r.gene_off, goff.nbytes)
    if tot:
        hip_memcpy_dtoh(gids, r.gene_ids, gids.nbytes)
    del t
    return goff, gids


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "gene_off differs at read %d" % int(np.argmax(got[0][:len(want[0])] != want[0])))
    assert np.array_equal(got[1], want[1]), what


def three_pairs_ran(h, also=()):
    lk = h.last_kernel()
    assert "classify_uni_kernel<" in lk and "+three-pairs" in lk and "verdict=uniform" in lk, lk
    for s in also:
        assert s in lk, (s, lk)
    return lk


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
ROUTES = [
    ("tiles", {"SHK_TILE_FIRST": "1"}, True, (" +tiles-first",)),
    ("no-tiles", {"SHK_TILE_FIRST": "0"}, True, ()),
    ("hashed-tiles", {"SHK_TILE_FIRST": "1"}, False, (" +tiles-first",)),
    ("hashed-no-tiles", {"SHK_TILE_FIRST": "0"}, False, ()),
]


@pytest.mark.parametrize("name,env,kmer_table,says", ROUTES, ids=[r[0] for r in ROUTES])
def test_counts_edges_thresholds_and_the_bound_cut(oracle, monkeypatch, name, env, kmer_table, says):
    """the one-gene index, 2 x 150 bp: the k-mer keyed kernel and its hashed twin, with the tiles' round and without; the whole batch
    and the same less one and less two pairs, so that the last triple is complete once and incomplete twice"""
    batch, want, n = one_gene_case(oracle)
    h = make_handle(monkeypatch, genes_of(1), env=env, kmer_table=kmer_table)
    same(on_device(h, batch, 150), want, (name, n))
    lk = three_pairs_ran(h, says)
    assert ("+tiles-first" in lk) == bool(says), lk
    for cut in (2, 1):
        sub, w = head(batch, want, n - cut)
        same(on_device(h, sub, 150), w, (name, n - cut))
        three_pairs_ran(h, says)
    h.close()


def other_case(oracle, key, genes, L1, L2, reps, trim=False):
    if key not in _made:
        rng = np.random.default_rng(len(key) + L1 + 3 * L2)
        counts = tuple(c for c in COUNTS if c <= len(chunks_of(L1, L2)))
        m1, m2 = counts_batch(rng, genes, L1, L2, reps, counts)
        m1, m2 = m1[:len(m1) // 3 * 3 - 1], m2[:len(m1) // 3 * 3 - 1]        # (an incomplete last triple here too)
        if trim:
            m1 = [x[:int(rng.integers(L1 - 30, L1 + 1))] for x in m1]
            m2 = [x[:int(rng.integers(L2 - 30, L2 + 1))] for x in m2]
            m1[0], m2[0] = m1[0][:L1 - 30], m2[0][:L2 - 30]
        batch = synth.batch_from_lists(m1, m2 if L2 else None)
        o = oracle.Shark(k=K, c=C, bf_bits=BF)
        o.build([bytes(g) for g in genes])
        ans = o.classify(*args(batch), nthreads=4)
        o.close()
        assigned = np.diff(ans[0].astype(np.int64)) > 0
        assert 0.1 < assigned.mean() < 0.9, (key, assigned.mean())
        _made[key] = (batch, ans)
    return _made[key]


@pytest.mark.parametrize("tiles", ["1", "0"])
def test_three_genes(oracle, monkeypatch, tiles):
    """the several-genes form (LXM) of the three-pairs kernel"""
    genes = genes_of(3)
    batch, want = other_case(oracle, "three-genes", genes, 150, 150, reps=3)
    assert len(set(want[1].tolist())) == 3
    h = make_handle(monkeypatch, genes, env={"SHK_TILE_FIRST": tiles})
    same(on_device(h, batch, 150), want, "three genes")
    three_pairs_ran(h, (" +sparse-first-rounds",))
    h.close()


def tri_fits(L1, L2, U):
    """tri_applies (classify_uni.hpp): three pairs of these lengths share a staging pass of the kernel with U rounds"""
    c1, c2 = (L1 + 15) >> 4, (L2 + 15) >> 4
    nk1, nk2 = max(L1 - K + 1, 0), max(L2 - K + 1, 0)
    return L1 != 0 and c1 + c2 <= 21 and ((c1 << 4) + nk2 if nk2 else nk1) <= 64 * U


LENGTHS = [(150, 0, 3), (100, 100, 3), (96, 96, 3), (120, 120, 4)]


@pytest.mark.parametrize("tiles", ["1", "0"])
@pytest.mark.parametrize("L1,L2,U", LENGTHS, ids=["single-150", "2x100", "2x96", "2x120"])
def test_other_lengths(oracle, monkeypatch, L1, L2, U, tiles):
    """other layouts, other instantiations, the same table: single-end 150 bp and 2 x 96 bp (U = 3), 2 x 120 bp (U = 4).  2 x 100 bp is
    another U than the headline's as well, 3 -- but in sixteen-base chunks its 196 slots do not fit 3 rounds, so that batch is a uniform
    one the three-pairs kernel leaves to the one-pair kernel: compared with the oracle all the same"""
    from shark_amd import SharkHip
    batch, want = other_case(oracle, "len-%d-%d" % (L1, L2), genes_of(1), L1, L2, reps=4)
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("SHK_TILE_FIRST", tiles)
    h = SharkHip(k=K, c=C, bf_bits=BF)
    h.build([bytes(g) for g in genes_of(1)])
    assert h.probe_mode() == "lds-table" and h.debug_kx_meta()["kx_in_use"] == 1
    same(on_device(h, batch, L1), want, (L1, L2))
    lk = three_pairs_ran(h, ("classify_uni_kernel<%d," % U,))
    assert tri_fits(L1, L2, U) == ((L1, L2) != (100, 100)), lk
    h.close()


def test_mixed_lengths_take_the_offsets_form(oracle, monkeypatch):
    """the control: mates of 120 .. 150 bases go through the offsets form, which keeps a threshold per pair of its own"""
    batch, want = other_case(oracle, "trimmed", genes_of(1), 150, 150, reps=4, trim=True)
    h = make_handle(monkeypatch, genes_of(1), env={"SHK_TILE_FIRST": "1"})
    same(on_device(h, batch, 150), want, "trimmed")
    lk = h.last_kernel()
    assert "offsets" in lk and "+three-pairs" in lk, lk
    h.close()
