"""The three results of the tiles' round of the three-pairs kernel (classify_uni_tiles.inc), written by lanes 0, 1, 2 under one ballot
with one store for the three counts and one for the three inline entries -- and, around them, a triple's loads at the ends of a batch,
at every alignment and beyond 4 GiB (classify_uni_loads.inc: tri_issue), which the same batches exercise.  No result may change:
every pair of every batch here is compared with the oracle -- its count, its ids -- and the device's per-gene counters, reset before
the batch, with the histogram of the oracle's ids.

One gene of 6 000 bases, c = 0.6, 2^33 bits; k = 17 (the k-mer keyed table) and k = 19 (its hashed twin).
  * ends of a batch: n = 1 ... 8 and 3 m + {0, 1, 2} pairs.  The mates' buffers are exact-size views at byte shifts 0 ... 3 inside larger
    arrays.  The last pair's gene bases end flush with both mates -- on the threshold, so that a dword left out of a guarded load takes
    the pair away, or one base under it with the gene continuing behind the view, so that a byte too many could bring it in; the
    first pair the same way at its beginning.  (A fetch behind the view cannot show in a result and nothing here waits for a fault.)
  * every hit pattern of a triple: the eight combinations of "ends in the tiles' round" / "does not" over p = 0, 1, 2 in the first, a
    middle and the last triple.  A pair that does not is a pair from elsewhere (its count stays 0) or one from the gene with a
    substitution in the middle of six tiles (ten matching tiles: the later rounds assign it).
  * the threshold's edge: pairs whose matching tiles are exactly the number that passes and one fewer (11 and 10 of 16 at 2 x 150,
    k = 17: 11 x 17 = 187 >= 180 > 170), errors planted tile by tile -- the other tiles broken at both ends and in the middle, so that
    the pair's coverage is k times its matching tiles and the oracle takes the one and not the other --, alone and mixed in a triple,
    and the same with an N in the middle of one tile.
  * lengths (150, 150), (151, 149), (149, 151), (160, 140): between them read r's first byte meets every alignment in either mate;
    tri_guard = ceil(19 / min(L1, L2)) = 1 for each.
  * the hashed twin, and mixed lengths through the offsets form with short pairs at p = 0, 1, 2 on both sides of their own thresholds.
  * mate buffers beyond 4 GiB, made on the device.

Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import torch  # noqa: F401  (torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both)

from tests import synth, views

pytestmark = pytest.mark.gpu

SWITCHES = ("SHK_PROBE", "SHK_NO_LDS_TABLE", "SHK_FORCE_GENERIC", "SHK_KTAB", "SHK_NO_LDS_SUMMARY", "SHK_NO_SUMMARY", "SHK_TILE_FIRST", "SHK_NO_TRI",
            "SHK_NO_TRO", "SHK_CLS_MIN_FILL", "SHK_NO_SPARSE", "SHK_FORCE_TRO", "SHK_NO_KMER_TABLE")
C, BF = 0.6, 1 << 33
SHAPES = [(150, 150), (151, 149), (149, 151), (160, 140)]
SHIFTS = [(0, 0), (1, 3), (2, 1), (3, 2)]                      # (seq1, seq2) byte shifts of the views
EXT = 25                                                      # gene bases that continue behind / before an edge pair's view


def thr_of(length):
    """the smallest integer t with (double)t >= c * (double)len (ReadAnalyzer.hpp:104)"""
    x = C * float(length)
    t = int(x)
    return t if float(t) >= x else t + 1


_gene = []


def the_gene():
    if not _gene:
        _gene.append(synth.random_seq(np.random.default_rng(6100), 6000))
    return _gene[0]


# ---------------------------------------------------------------------------
# pairs: a read is (m1, m2, None, None) as in tests/views.py
# ---------------------------------------------------------------------------
def gene_pair(rng, L1, L2):
    g = the_gene()
    a = int(rng.integers(0, len(g) - L1 - L2 - 60))
    return g[a:a + L1].copy(), synth.revcomp(g[a + L1 + 50:a + L1 + 50 + L2])


def elsewhere_pair(rng, L1, L2):
    return synth.random_seq(rng, L1), synth.random_seq(rng, L2)


def substitute(m, p):
    m[p] = synth.ACGT[(int(np.searchsorted(synth.ACGT, m[p])) + 1) & 3]


def tiles_of(L, k):
    """the disjoint k-mers of a mate that the tiles' round probes: slots 0, k, 2 k, ... -- eight at most"""
    nk = L - k + 1
    return min((nk - 1) // k + 1, 8) if nk > 0 else 0


def tiled_pair(rng, L1, L2, k, n_match, sharp, with_n=False):
    """a pair from the gene of which exactly n_match tiles match.  sharp: the others are broken at both ends and in the middle, and so is
    what lies behind a mate's last tile -- the pair covers k * n_match bases and nothing else; else one substitution in the middle of
    each.  with_n: one of the broken tiles has an N in its middle instead (len drops by one).  Returns (m1, m2, coverage or None)"""
    m = list(gene_pair(rng, L1, L2))
    T = [(t, j) for t in (0, 1) for j in range(tiles_of((L1, L2)[t], k))]
    order = [T[int(i)] for i in rng.permutation(len(T))]
    broken = order[n_match:]
    assert broken or not with_n
    for i, (t, j) in enumerate(broken):
        if sharp:
            substitute(m[t], k * j)
            substitute(m[t], k * j + k - 1)
        if with_n and i == 0:
            m[t][k * j + k // 2] = ord("N")
        else:
            substitute(m[t], k * j + k // 2)
    if sharp:
        for t in (0, 1):
            for p in range(k * tiles_of((L1, L2)[t], k), (L1, L2)[t], k - 1):
                substitute(m[t], p)
    return m[0], m[1], (k * n_match if sharp else None)


def need_tiles(L1, L2, k):
    return -(-thr_of(L1 + L2) // k)


def runs_pair(rng, L1, L2, runs, ext=0):
    """two mates of random bases with runs of gene bases: runs = [(mate, position, x)], each a window of the gene on a strand drawn per
    run; the mate's bases beside a run differ from the gene's own neighbours of the window, so a run of x bases covers exactly x.
    Returns (m1, m2, [(the ext gene bases before the window, the ext behind it)] per run, in the mate's orientation)"""
    m = [synth.random_seq(rng, L1), synth.random_seq(rng, L2)]
    info = []
    for t, p, x in runs:
        g = the_gene() if rng.random() < 0.5 else synth.revcomp(the_gene())
        s = int(rng.integers(ext + 1, len(g) - x - ext - 1))
        m[t][p:p + x] = g[s:s + x]
        for q, gq in ((p - 1, s - 1), (p + x, s + x)):
            if 0 <= q < len(m[t]):
                m[t][q] = g[gq]
                substitute(m[t], q)
        info.append((g[s - ext:s].copy(), g[s + x:s + x + ext].copy()))
    return m[0], m[1], info


def edge_pair(rng, L1, L2, k, side, under):
    """gene bases flush with both mates' ends (side 'right') or beginnings ('left'), thr - under of them in all; with the bytes of the gene
    that continue behind (before) them: ((m1, m2), [bytes for seq1, bytes for seq2])"""
    x = thr_of(L1 + L2) - under
    a = min(L1 - 20, x - 3 * k)
    at = (0, 0) if side == "left" else (L1 - a, L2 - (x - a))
    m1, m2, info = runs_pair(rng, L1, L2, [(0, at[0], a), (1, at[1], x - a)], ext=EXT)
    return (m1, m2), [info[0][1 if side == "right" else 0], info[1][1 if side == "right" else 0]]


# ---------------------------------------------------------------------------
# the oracle's answers, per read
# ---------------------------------------------------------------------------
class Answers:
    """a pool of pairs with the oracle's answer for each (a read's answer does not depend on its batch)"""

    def __init__(self, oracle, k):
        self.o = oracle.Shark(k=k, c=C, bf_bits=BF)
        self.o.build([bytes(the_gene())])
        self.k = k
        self.pairs, self.ids = [], []

    def add(self, pairs):
        """-> the indices of these pairs in the pool"""
        first = len(self.pairs)
        b = synth.batch_from_lists([p[0] for p in pairs], [p[1] for p in pairs])
        goff, gids = self.o.classify(b["seq1"], b["off1"], b["seq2"], b["off2"], nthreads=4)
        goff = goff.astype(np.int64)
        for i, p in enumerate(pairs):
            self.pairs.append((p[0], p[1]))
            self.ids.append(gids[goff[i]:goff[i + 1]].copy())
        return list(range(first, len(self.pairs)))

    def analyze(self, pair):
        genes, mx, _, ln = self.o.analyze(bytes(pair[0]) + b"N" + bytes(pair[1]))
        return genes, mx, ln

    def assigned(self, i):
        return len(self.ids[i]) > 0

    def batch(self, idx):
        """(the SoA batch of these pairs, the expected (gene_off, gene_ids))"""
        b = synth.batch_from_lists([self.pairs[i][0] for i in idx], [self.pairs[i][1] for i in idx])
        cnt = np.array([len(self.ids[i]) for i in idx], np.int64)
        goff = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
        gids = np.concatenate([self.ids[i] for i in idx]).astype(np.uint16) if len(idx) else np.zeros(0, np.uint16)
        return b, (goff, gids)

    def close(self):
        self.o.close()


_answers = {}


def answers(oracle, k):
    """one pool per k (an oracle of 2^33 bits holds a GiB)"""
    if k not in _answers:
        _answers[k] = Answers(oracle, k)
    return _answers[k]


N_COUNTERS = 4


def same(got, want, what):
    """count per pair, the ids, and the device's per-gene counters (got[2]: read after the batch, reset before it) against the
    histogram of the oracle's ids"""
    assert len(got[0]) == len(want[0]), what
    gc, wc = np.diff(got[0].astype(np.int64)), np.diff(want[0].astype(np.int64))
    assert np.array_equal(gc, wc), (what, "count differs at pair %d: %d for %d" % (int(np.argmax(gc != wc)), int(gc[np.argmax(gc != wc)]), int(wc[np.argmax(gc != wc)])))
    assert np.array_equal(got[1], want[1]), (what, "ids differ")
    hist = np.bincount(want[1], minlength=N_COUNTERS).astype(np.uint64)
    assert np.array_equal(got[2], hist), (what, "per-gene counters differ from the oracle's histogram", got[2].tolist(), hist.tolist())


# ---------------------------------------------------------------------------
# running
# ---------------------------------------------------------------------------
def make_handle(monkeypatch, k, env=None):
    from shark_amd import SharkHip
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for name, val in (env or {}).items():
        monkeypatch.setenv(name, val)
    h = SharkHip(k=k, c=C, bf_bits=BF)
    h.build([bytes(the_gene())])
    assert h.probe_mode() == "lds-table", h.probe_mode()
    assert h.debug_kx_meta()["kx_in_use"] == (1 if k <= 17 else 0)
    return h


def fetch(r):
    from shark_amd import capi
    n, tot = int(r.n), int(r.n_assoc)
    goff, gids = np.zeros(n + 1, np.uint32), np.zeros(tot, np.uint16)
    capi.hip_memcpy_dtoh(goff, r.gene_off, goff.nbytes)
    if tot:
        capi.hip_memcpy_dtoh(gids, r.gene_ids, gids.nbytes)
    return goff, gids


def resident(h, batch, shift, max_read_len, lead=None, trail=None):
    """classify_device on exact-size views of the batch's arrays at these byte shifts inside larger ones"""
    e = views.embed(batch, views.shifts_of(shift[0], shift[1]), lead=lead, trail=trail)
    keep, p = views.to_device(e)
    h.gene_counts_reset()
    r = h.classify_device(e["n"], p["seq1"], p["off1"], p["seq2"], p["off2"], max_read_len=max_read_len)
    out = fetch(r) + (h.gene_counts(N_COUNTERS),)
    del keep
    return out


_prime = {}


def prime(h, L1, L2):
    """a batch of which every pair is assigned: the next batch of the handle gets the tiles' round (a quarter would do)"""
    if (L1, L2) not in _prime:
        rng = np.random.default_rng([L1, L2])
        pr = [gene_pair(rng, L1, L2) for _ in range(24)]
        _prime[(L1, L2)] = synth.batch_from_lists([p[0] for p in pr], [p[1] for p in pr])
    goff, _, counters = resident(h, _prime[(L1, L2)], (0, 0), max(L1, L2))
    assert int(goff[-1]) == 24 == int(counters[0])


def ran(h, tiles, offsets=False, u=5):
    lk = h.last_kernel()
    assert "classify_uni_kernel<%d, " % u in lk and "+three-pairs" in lk, lk
    assert ("offsets" in lk) if offsets else ("verdict=uniform" in lk), lk
    assert ("+tiles-first" in lk) == tiles, lk
    return lk


def run(h, batch, want, what, L1, L2, shift=(0, 0), tiles=True, offsets=False, lead=None, trail=None):
    if tiles:
        prime(h, L1, L2)
    same(resident(h, batch, shift, max(L1, L2), lead, trail), want, what)
    ran(h, tiles, offsets)


# ---------------------------------------------------------------------------
# the pools (made once)
# ---------------------------------------------------------------------------
_made = {}


def mixed_pool(oracle, k, L1, L2, n):
    """n pairs: from the gene (a few substitutions in some), from elsewhere, ten-tile pairs, by turns"""
    key = ("mixed", k, L1, L2, n)
    if key not in _made:
        rng = np.random.default_rng([k, L1, L2, n])
        A = answers(oracle, k)
        pairs = []
        for i in range(n):
            kind = int(rng.integers(0, 4))
            if kind == 0:
                pairs.append(elsewhere_pair(rng, L1, L2))
            elif kind == 1:
                pairs.append(tiled_pair(rng, L1, L2, k, need_tiles(L1, L2, k) - 1, sharp=bool(i & 1))[:2])
            else:
                m1, m2 = gene_pair(rng, L1, L2)
                for m in (m1, m2):
                    for p in rng.choice(len(m), size=int(rng.integers(0, 4)), replace=False):
                        substitute(m, int(p))
                pairs.append((m1, m2))
        idx = A.add(pairs)
        edges = {}
        for side in ("left", "right"):
            for under in (0, 1):
                pr, by = edge_pair(rng, L1, L2, k, side, under)
                genes, mx, ln = A.analyze(pr)
                assert ln == L1 + L2 and mx == thr_of(L1 + L2) - under and (len(genes) == 1) == (under == 0), (side, under, mx, ln)
                edges[(side, under)] = (A.add([pr])[0], by)
        frac = np.mean([A.assigned(i) for i in idx])
        assert 0.3 < frac < 0.8, frac
        _made[key] = (A, idx, edges)
    return _made[key]


def with_edges(pool, n, under):
    """n pairs of the pool: the first begins flush, the last ends flush (n = 1: the last alone) -> (batch, want, lead, trail)"""
    A, idx, edges = pool
    last, trail = edges[("right", under)]
    if n == 1:
        b, want = A.batch([last])
        return b, want, None, trail
    first, lead = edges[("left", under)]
    b, want = A.batch([first] + idx[:n - 2] + [last])
    return b, want, lead, trail


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
M = 2000
ENDS = list(range(1, 9)) + [3 * M, 3 * M + 1, 3 * M + 2]


@pytest.mark.parametrize("tiles", [True, False], ids=["tiles", "no-tiles"])
def test_ends_of_a_batch(oracle, monkeypatch, tiles):
    """a partial last triple, a last triple on another wave than the one before it, guarded loads for the last reads -- at every byte shift"""
    pool = mixed_pool(oracle, 17, 150, 150, 3 * M + 2)
    h = make_handle(monkeypatch, 17, env=None if tiles else {"SHK_TILE_FIRST": "0"})
    for j, n in enumerate(ENDS):
        for under in (0, 1):
            b, want, lead, trail = with_edges(pool, n, under)
            assert len(b["off1"]) - 1 == n and (int(np.diff(want[0].astype(np.int64))[-1]) == 1) == (under == 0)
            for shift in (SHIFTS if n <= 8 or under == 0 else SHIFTS[j % 4:j % 4 + 1]):
                run(h, b, want, ("ends", n, under, shift), 150, 150, shift, tiles=tiles, lead=lead, trail=trail)
    h.close()


def pattern_case(oracle):
    if "pattern" not in _made:
        rng = np.random.default_rng(31)
        A = answers(oracle, 17)
        n_tri = 23
        hit = A.add([gene_pair(rng, 150, 150) for _ in range(3 * n_tri)])
        miss = A.add([elsewhere_pair(rng, 150, 150) if i & 1 else tiled_pair(rng, 150, 150, 17, 10, sharp=False)[:2] for i in range(3 * n_tri)])
        assert all(A.assigned(i) for i in hit)
        assert all(A.assigned(i) == (not (j & 1)) for j, i in enumerate(miss)), "ten tiles with one substitution each are assigned by the later rounds"
        _made["pattern"] = (A, hit, miss, n_tri)
    return _made["pattern"]


@pytest.mark.parametrize("combo", range(8))
def test_every_hit_pattern_of_a_triple(oracle, monkeypatch, combo):
    """bit p of combo: pair p of the first, the middle and the last triple ends in the tiles' round; the other triples take the other
    seven patterns by turns.  What does not end there goes through the later rounds, and its count and ids are its own"""
    A, hit, miss, n_tri = pattern_case(oracle)
    idx = []
    for t in range(n_tri):
        c = combo if t in (0, n_tri // 2, n_tri - 1) else (combo + t) & 7
        idx += [(hit if (c >> p) & 1 else miss)[3 * t + p] for p in range(3)]
    b, want = A.batch(idx)
    h = make_handle(monkeypatch, 17)
    for shift in SHIFTS[:2]:
        run(h, b, want, ("pattern", combo, shift), 150, 150, shift)
    h.close()


def edge_case(oracle, k, L1, L2):
    """triples over (on the threshold, one tile fewer, from elsewhere)^3, in three forms: sharp, sharp with an N in a tile, one
    substitution per broken tile"""
    key = ("edge", k, L1, L2)
    if key not in _made:
        rng = np.random.default_rng([k, L1, L2, 5])
        A = answers(oracle, k)
        need = need_tiles(L1, L2, k)
        pairs, sides = [], set()
        for form in range(3):
            for combo in range(27):
                for p in range(3):
                    kind = (combo // 3 ** p) % 3
                    if kind == 2:
                        pairs.append(elsewhere_pair(rng, L1, L2))
                        continue
                    m1, m2, cov = tiled_pair(rng, L1, L2, k, need - kind, sharp=form < 2, with_n=form == 1)
                    if cov is not None:
                        genes, mx, ln = A.analyze((m1, m2))
                        assert mx == cov and ln == L1 + L2 - (form == 1), (form, kind, mx, cov, ln)
                        assert (len(genes) == 1) == (kind == 0) == (cov >= thr_of(ln)), (form, kind, genes)
                        sides.add((form, kind))
                    pairs.append((m1, m2))
        assert sides == {(f, s) for f in (0, 1) for s in (0, 1)}
        idx = A.add(pairs)
        _made[key] = (A, idx)
    return _made[key]


def test_the_thresholds_edge(oracle, monkeypatch):
    """11 matching tiles of 16 pass the tiles' round, 10 do not (and, the other tiles broken for good, nothing else assigns the pair);
    alone and mixed in one triple; with an N inside a tile"""
    assert need_tiles(150, 150, 17) == 11 and tiles_of(150, 17) == 8
    A, idx = edge_case(oracle, 17, 150, 150)
    b, want = A.batch(idx)
    h = make_handle(monkeypatch, 17)
    for shift in SHIFTS:
        run(h, b, want, ("edge", shift), 150, 150, shift)
    h.close()


def tri_fits(L1, L2, k, U):
    """tri_applies (classify_uni.hpp): three pairs of these lengths share a staging pass of the kernel with U rounds"""
    c1, c2 = (L1 + 15) >> 4, (L2 + 15) >> 4
    nk1, nk2 = max(L1 - k + 1, 0), max(L2 - k + 1, 0)
    return L1 != 0 and c1 + c2 <= 21 and ((c1 << 4) + nk2 if nk2 else nk1) <= 64 * U


def shape_batch(oracle, k, L1, L2, extra):
    """a few hundred mixed pairs and the threshold's edge at these lengths, between an edge pair at either end; 3 m + extra pairs"""
    pool = mixed_pool(oracle, k, L1, L2, 240)
    A, idx, edges = pool
    key = ("shape-edge", k, L1, L2)
    if key not in _made:
        rng = np.random.default_rng([k, L1, L2, 9])
        need = need_tiles(L1, L2, k)
        pairs = []
        for i in range(36):
            m1, m2, cov = tiled_pair(rng, L1, L2, k, need - (i & 1), sharp=True, with_n=bool(i & 2))
            genes, mx, ln = A.analyze((m1, m2))
            assert mx == cov and ln == L1 + L2 - bool(i & 2) and (len(genes) == 1) == (not i & 1), (i, mx, cov, ln, genes)
            pairs.append((m1, m2))
        _made[key] = A.add(pairs)
    mid = idx + _made[key]
    n = len(mid) // 3 * 3 + extra - 2
    first, lead = edges[("left", 1)]
    last, trail = edges[("right", 0)]
    b, want = A.batch([first] + mid[:n] + [last])
    assert (len(b["off1"]) - 1) % 3 == extra
    return b, want, lead, trail


@pytest.mark.parametrize("L1,L2", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_lengths_and_alignment(oracle, monkeypatch, L1, L2):
    """read r of a mate starts at r L: with these lengths at every byte alignment, in either mate, at every shift of the views"""
    assert tri_fits(L1, L2, 17, 5) and -(-19 // min(L1, L2)) == 1                   # (tri_guard: the batch's last read alone is guarded)
    for mate in (0, 1):
        assert {(r * s[mate]) % 4 for s in SHAPES for r in range(4)} == {0, 1, 2, 3}
    assert need_tiles(L1, L2, 17) == 11 and tiles_of(L1, 17) == tiles_of(L2, 17) == 8
    b, want, lead, trail = shape_batch(oracle, 17, L1, L2, extra=SHAPES.index((L1, L2)) % 3)
    h = make_handle(monkeypatch, 17)
    for shift in SHIFTS:
        run(h, b, want, ("lengths", L1, L2, shift), L1, L2, shift, lead=lead, trail=trail)
    h.close()


def test_the_hashed_twin(oracle, monkeypatch):
    """k = 19: no k-mer keyed table, the hashed instantiation; seven tiles a mate, ten of fourteen pass (190 >= 180 > 171)"""
    assert tiles_of(150, 19) == 7 and need_tiles(150, 150, 19) == 10
    b, want, lead, trail = shape_batch(oracle, 19, 150, 150, extra=2)
    h = make_handle(monkeypatch, 19)
    for shift in SHIFTS[:2]:
        run(h, b, want, ("hashed", shift), 150, 150, shift, lead=lead, trail=trail)
    h.close()


def trimmed_case(oracle):
    """2 x 150 bp with short pairs at p = 0, 1, 2 of their triples -- one, two or all three of a triple --: pairs of 118 ... 149 bases a
    mate whose coverage is ceil(c (l1 + l2)) of their OWN lengths and one below it, and trimmed pairs from the gene that pass the
    tiles' round on the tiles they have"""
    if "trimmed" not in _made:
        rng = np.random.default_rng(53)
        A = answers(oracle, 17)
        pairs, sides = [], set()
        for i in range(72):
            short = {i % 3} if i % 4 else ({0, 1, 2} if i % 8 else {i % 3, (i + 1) % 3})
            for p in range(3):
                if p not in short:
                    pairs.append(gene_pair(rng, 150, 150) if (i + p) % 3 else elsewhere_pair(rng, 150, 150))
                    continue
                l1, l2 = int(rng.integers(118, 150)), int(rng.integers(118, 150))
                if (i + p) % 4 == 3:
                    pairs.append(gene_pair(rng, l1, l2))
                    continue
                under = (i >> 1) & 1
                x = thr_of(l1 + l2) - under
                xa = x // 2
                m1, m2, _ = runs_pair(rng, l1, l2, [(0, int(rng.integers(1, l1 - xa)), xa), (1, int(rng.integers(1, l2 - (x - xa))), x - xa)])
                genes, mx, ln = A.analyze((m1, m2))
                assert mx == x and ln == l1 + l2 and (len(genes) == 1) == (under == 0), (l1, l2, mx, x, ln)
                sides.add((p, under))
                pairs.append((m1, m2))
        assert sides == {(p, u) for p in range(3) for u in (0, 1)}
        idx = A.add(pairs)
        _made["trimmed"] = (A, idx)
    return _made["trimmed"]


def test_mixed_lengths_through_the_offsets_form(oracle, monkeypatch):
    """the offsets form: the tiles' round compares a pair's own threshold, lane p's"""
    A, idx = trimmed_case(oracle)
    h = make_handle(monkeypatch, 17)
    for cut, shift in zip((0, 1, 2), SHIFTS[1:]):
        b, want = A.batch(idx[:len(idx) - cut])
        run(h, b, want, ("trimmed", cut, shift), 150, 150, shift, offsets=True)
    h.close()


BIG_L1, BIG_L2 = 151, 149


def test_mates_beyond_4_gib(oracle, monkeypatch):
    """a read's place in its mate's buffer is a 64-bit product: 28.9 M pairs of 151 + 149 bases made on the device, either buffer just
    over 4 GiB.  Pairs from the gene in the triples on both sides of the 2^32-byte boundary of each mate and in the first and the last
    triple; those, and a fixed sample of the others, against the oracle; the per-gene counts against the sum of the counts"""
    dev = torch.device("cuda:0")
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 16 << 30:
        pytest.skip("needs 16 GiB of free device memory for two mate buffers over 4 GiB, %.1f GiB free" % (free / 2 ** 30))
    L1, L2 = BIG_L1, BIG_L2
    n = (1 << 32) // L2 + 70_001                       # 3 m + 1 pairs: a partial last triple
    assert n % 3 == 1 and n * L2 > 1 << 32 and n * L1 > 1 << 32
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    seq = []
    for L in (L1, L2):
        s = torch.empty(n * L, dtype=torch.uint8, device=dev)
        step = 1 << 28
        for a in range(0, n * L, step):
            c = torch.randint(0, 4, (min(step, n * L - a),), dtype=torch.uint8, device=dev, generator=g)
            s[a:a + len(c)] = c * 2 + 65 + (c >> 1) * 2 + (c == 3).to(torch.uint8) * 11      # A C G T, in uint8 throughout
            del c
        seq.append(s)
    rng = np.random.default_rng(88)
    planted = {0, 1, 2, n - 1}
    for L in (L1, L2):
        t = ((1 << 32) // L) // 3                      # the triple that holds the boundary's read
        planted |= {3 * tt + p for tt in (t - 1, t, t + 1) for p in range(3)}
    planted = sorted(planted)
    assert planted[-1] == n - 1
    for i in planted:
        m1, m2 = gene_pair(rng, L1, L2)
        if i % 2:
            m1, m2, _ = tiled_pair(rng, L1, L2, 17, 10, sharp=False)
        seq[0][i * L1:(i + 1) * L1] = torch.from_numpy(m1).to(dev)
        seq[1][i * L2:(i + 1) * L2] = torch.from_numpy(m2).to(dev)
    off1 = torch.arange(0, (n + 1) * L1, L1, dtype=torch.int64, device=dev)
    off2 = torch.arange(0, (n + 1) * L2, L2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    h = make_handle(monkeypatch, 17)
    prime(h, L1, L2)
    h.gene_counts_reset()
    r = h.classify_device(n, seq[0].data_ptr(), off1.data_ptr(), seq[1].data_ptr(), off2.data_ptr(), max_read_len=max(L1, L2))
    goff, gids = fetch(r)
    counters = h.gene_counts(N_COUNTERS)
    ran(h, True)
    h.close()
    count = np.diff(goff.astype(np.int64))
    # the device's per-gene counters: their total is the sum of the counts, and all of it is the one gene's
    assert int(counters.sum()) == int(count.sum()) == len(gids) and int(counters[0]) == int(count.sum()), (counters.tolist(), int(count.sum()))
    sample = sorted(set(planted) | {int(i) for i in np.random.default_rng(7).integers(0, n, size=300)})
    A = answers(oracle, 17)
    at = torch.tensor(sample, dtype=torch.int64, device=dev)
    h1 = seq[0][(at[:, None] * L1 + torch.arange(L1, device=dev)[None, :]).reshape(-1)].cpu().numpy().reshape(len(sample), L1)
    h2 = seq[1][(at[:, None] * L2 + torch.arange(L2, device=dev)[None, :]).reshape(-1)].cpu().numpy().reshape(len(sample), L2)
    idx = A.add([(h1[j].copy(), h2[j].copy()) for j in range(len(sample))])
    for j, i in enumerate(sample):
        assert int(count[i]) == len(A.ids[idx[j]]), ("pair %d" % i, int(count[i]), A.ids[idx[j]])
        assert np.array_equal(gids[goff[i]:goff[i + 1]], A.ids[idx[j]]), i
    assert all(A.assigned(idx[sample.index(i)]) for i in planted)
    assert int(count.sum()) == len(planted) == int(counters[0]), "a pair of random bases that the gene takes"
