"""The miss path of the sparse first rounds of a one-gene index (classify_uni.hpp, per_pair: round A's candidate stage and one ballot;
no candidate: round B's and one ballot; none again and the slots left cover less than the threshold: the pair is through) and the
hand-over to the general code (sparse_first) of every pair with a candidate in A or B.  No result may change: every pair of every
batch is held against the oracle -- its count, its ids -- and the device's per-gene counters, reset before the batch, against the
histogram of the oracle's ids; last_kernel() is asserted per run, the tiles' round comes from a primed handle.

One gene of 6 000 bases, c = 0.6, 2^33 bits; k = 17 (the k-mer keyed table) and k = 19 (its hashed twin).  The plan of a pair of
L1 + L2 bases (classify_uni_plan.inc, plan_sparse; restated in plan_of): T tiles, the prefix [0, 128 - T) -- even slots and the tiles
in round A, the rest of the prefix in round B, the T slots in front of slot 128 displaced --, spUb bases behind the prefix.  At the
shapes here T = 7, the prefix is mate 1's slots 0 .. 120, spUb = L1 + L2 - 121.

Kinds of pairs (kinds()), each of them as the OPEN pair of every open / settled pattern of a triple in the first, a middle and the last
triple of a batch (a settled pair is one from the gene: the tiles' round takes it, or round A where that round is off):
  elsewhere     random bases: the miss path
  only-A        random bases and ONE k-mer of the gene, in an even slot of the prefix: a candidate in A alone
  only-B        the same in an odd slot: B alone
  only-F        the same in a displaced slot: neither round sees it, and the bound cut must still be right
  only-tile     the same in a tile slot of mate 2 (a lane of round A behind the even slots)
  by-A          a pair from the gene, six of mate 1's eight tiles broken by one substitution each: ten matching tiles fail the tiles'
                round (eleven are needed; k = 19: five broken, nine of fourteen), round A's coverage settles it
  by-A-runs     gene bases [0, thr - T k) of mate 1 and the last T k of mate 2: fewer than the tiles needed, coverage exactly thr in A
  by-prefix     the same with mate 1's run at [1, ...): A's even slots cover two bases fewer, the whole prefix behind B covers thr
  under         one base fewer: the whole prefix covers thr - 1, the pair goes on and stays without a gene
  tag-A/B/AB    random bases with a k-mer that is NOT in the table and passes the 16-bit candidate stage (the constructions of
                tests/test_gpu_kx_two_stage.py) in an even slot, an odd slot, both; and `under` with one in A, where a false hit
                would lift it over the threshold  (k = 17 only: the hashed twin has one stage)
  N             random bases with one N; with one N in every chunk of 16 bases; with two N in one chunk (the threshold by the
                reduction, not the table); with so many that spUb >= the pair's own threshold -- the pair must NOT be cut behind B.
                analyze() gives each pair's len; the counts lie on both sides of the inequality.  (2 x 150 bp has 20 chunks; the
                shape 145 + 161 has 21, the most the three-pairs kernel takes, with the sparse order on: T = 5.)

Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import torch  # noqa: F401  (torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both)

from tests import synth
from tests import test_gpu_triple_loads_results as base
from tests import test_gpu_kx_two_stage as two_stage

pytestmark = pytest.mark.gpu

SHAPES, SHIFTS = base.SHAPES, base.SHIFTS
thr_of = base.thr_of


# ---------------------------------------------------------------------------
# the plan (classify_uni_plan.inc: bases_behind, slot_for_ub, plan_sparse) for the three-pairs layout
# ---------------------------------------------------------------------------
def bases_behind(s, L1, L2, k):
    nk1, nk2, P2 = max(L1 - k + 1, 0), max(L2 - k + 1, 0), 16 * ((L1 + 15) // 16)
    u = L1 - s if s < nk1 else 0
    s2 = max(s - P2, 0)
    return u + (L2 - s2 if s2 < nk2 else 0)


def plan_of(L1, L2, k, thr=None):
    """(T, spUb, mate 2's position of tile 0) -- T = 0: no sparse order"""
    thr = thr_of(L1 + L2) if thr is None else thr
    nk1, nk2, P2 = L1 - k + 1, L2 - k + 1, 16 * ((L1 + 15) // 16)
    sp_last = P2 + nk2 - 1
    B = thr - 1
    assert L1 + L2 > B and L1 + L2 - B < nk1, "the first slot with at most thr - 1 bases behind it lies in mate 1 at these shapes"
    X = L1 + L2 - B
    T = min(16, (nk2 - 1) // k + 1, (sp_last - 127) // (k - 1), 128 - X)
    assert T > 0 and bases_behind(128 - T, L1, L2, k) < thr
    return T, bases_behind(128 - T, L1, L2, k), nk2 - 1


def tiles_matching(runs, L1, L2, k):
    """tiles of the tiles' round (slots 0, k, 2 k, ... of either mate, eight at most) that lie inside a run"""
    n = 0
    for t, L in ((0, L1), (1, L2)):
        for j in range(base.tiles_of(L, k)):
            n += any(rt == t and p <= j * k and j * k + k <= p + x for rt, p, x in runs)
    return n


# ---------------------------------------------------------------------------
# the kinds
# ---------------------------------------------------------------------------
def one_kmer(rng, L1, L2, k, mate, pos):
    return base.runs_pair(rng, L1, L2, [(mate, pos, k)])[:2]


def runs_kind(rng, A, L1, L2, k, start, under):
    """gene bases [start, start + thr - T k - under) of mate 1 and the last T k of mate 2 -> (pair, its coverage)"""
    T, _, _ = plan_of(L1, L2, k)
    thr = thr_of(L1 + L2)
    x1 = thr - T * k - under
    runs = [(0, start, x1), (1, L2 - T * k, T * k)]
    assert x1 >= k and start + x1 - k < 128 - T, "mate 1's run lies in the prefix"
    assert tiles_matching(runs, L1, L2, k) < base.need_tiles(L1, L2, k), "the tiles' round does not take the pair"
    m1, m2, _ = base.runs_pair(rng, L1, L2, runs)
    genes, mx, ln = A.analyze((m1, m2))
    assert mx == thr - under and ln == L1 + L2 and (len(genes) == 1) == (under == 0), (mx, thr, under, ln, genes)
    return m1, m2


def by_a_pair(rng, L1, L2, k):
    """a pair from the gene with just enough of mate 1's tiles broken in the middle that one tile fewer matches than the tiles' round
    needs (2 x 150 bp, k = 17: six of eight broken, ten of sixteen match)"""
    m1, m2 = base.gene_pair(rng, L1, L2)
    n_break = base.tiles_of(L1, k) + base.tiles_of(L2, k) - (base.need_tiles(L1, L2, k) - 1)
    assert 0 < n_break <= base.tiles_of(L1, k)
    for j in rng.permutation(base.tiles_of(L1, k))[:n_break]:
        base.substitute(m1, int(j) * k + k // 2)
    return m1, m2


def with_n(rng, L1, L2, where):
    """random bases with N at these (mate, position)"""
    m = [synth.random_seq(rng, L1), synth.random_seq(rng, L2)]
    for t, p in where:
        m[t][p] = ord("N")
    return m[0], m[1]


def n_kinds(rng, A, L1, L2, k):
    """-> {name: pair}; asserts the sides of spUb < thr(len) with the oracle's len"""
    T, sp_ub, _ = plan_of(L1, L2, k)
    chunks = [(t, 16 * c) for t, L in ((0, L1), (1, L2)) for c in range((L + 15) // 16)]
    many = int(np.ceil(L1 + L2 - sp_ub / base.C)) + 4                    # enough N that c (L1 + L2 - n) <= spUb, and four more
    spread = [(t, int(p)) for t, L in ((0, L1), (1, L2)) for p in rng.choice(L, size=(many + 1) // 2, replace=False)]
    out = {"N-one": with_n(rng, L1, L2, [(0, L1 // 3)]),
           "N-per-chunk": with_n(rng, L1, L2, [(t, p + int(rng.integers(0, min(16, (L1, L2)[t] - p)))) for t, p in chunks]),
           "N-two-in-a-chunk": with_n(rng, L1, L2, [(1, 35), (1, 44)]),
           "N-many": with_n(rng, L1, L2, spread)}
    want_len = {"N-one": L1 + L2 - 1, "N-per-chunk": L1 + L2 - len(chunks), "N-two-in-a-chunk": L1 + L2 - 2, "N-many": L1 + L2 - len(spread)}
    sides = set()
    for name, pr in out.items():
        genes, mx, ln = A.analyze(pr)
        assert ln == want_len[name] and not genes, (name, ln, want_len[name], genes)
        sides.add(sp_ub < thr_of(ln))
    # (a pair without N is cut; at 2 x 150 bp one with a single N still is, two N already reach spUb = 179; at 145 + 161 one N does)
    assert sp_ub < thr_of(L1 + L2) and sp_ub >= thr_of(want_len["N-many"])
    assert (sp_ub < thr_of(want_len["N-one"])) == (L1 + L2 == 300) and (sides == {True, False} or L1 + L2 != 300)
    return out


_nm = {}


def near_miss_kmers(monkeypatch, k):
    """k-mers that pass the candidate stage of this gene's table and are not in it (tests/test_gpu_kx_two_stage.py)"""
    if k not in _nm:
        h = base.make_handle(monkeypatch, k)
        img, keys, meta = h.debug_index_array("kxtab"), h.debug_index_array("kxkeys"), h.debug_kx_meta()
        h.close()
        nm = two_stage.near_misses(img, meta["kx_m1"], meta["kx_m2"], keys, k)
        two_stage.check_construction(img, meta["kx_m1"], meta["kx_m2"], keys, k, nm)
        _nm[k] = nm
    return _nm[k]


def planted(rng, nm, pair, k, slots):
    m1 = pair[0].copy()
    for i, s in enumerate(slots):
        cls = two_stage.CLASSES[(i + int(rng.integers(0, 4))) % 4]
        m1[s:s + k] = two_stage.kmer_seq(rng, nm[cls][int(rng.integers(0, len(nm[cls])))], k)
    return m1, pair[1].copy()


_kinds = {}
PER_KIND = 9


def kinds(oracle, monkeypatch, k, L1, L2):
    """{kind: indices of PER_KIND pairs in the pool}, the pool, the indices of settled (gene) pairs"""
    key = (k, L1, L2)
    if key not in _kinds:
        rng = np.random.default_rng([k, L1, L2, 77])
        A = base.answers(oracle, k)
        T, sp_ub, tile0 = plan_of(L1, L2, k)
        assert T == 7 and 128 - T < L1 - k + 1
        even = lambda: 2 * int(rng.integers(0, (128 - T + 1) // 2))                        # slots 0, 2, ... of round A
        odd = lambda: int(rng.choice([2 * int(rng.integers(0, 55)) + 1, int(rng.integers(113, 128 - T))]))   # 2 ln + 1 and lanes nA - 1 ...: round B
        made = {"elsewhere": [base.elsewhere_pair(rng, L1, L2) for _ in range(PER_KIND)],
                "only-A": [one_kmer(rng, L1, L2, k, 0, even()) for _ in range(PER_KIND)],
                "only-B": [one_kmer(rng, L1, L2, k, 0, odd()) for _ in range(PER_KIND)],
                "only-F": [one_kmer(rng, L1, L2, k, 0, 128 - T + i % T) for i in range(PER_KIND)],
                "only-tile": [one_kmer(rng, L1, L2, k, 1, tile0 - (i % T) * k) for i in range(PER_KIND)],
                "by-A": [by_a_pair(rng, L1, L2, k) for _ in range(PER_KIND)],
                "by-A-runs": [runs_kind(rng, A, L1, L2, k, 0, 0) for _ in range(PER_KIND)],
                "by-prefix": [runs_kind(rng, A, L1, L2, k, 1, 0) for _ in range(PER_KIND)],
                "under": [runs_kind(rng, A, L1, L2, k, 2 * (i % 3), 1) for i in range(PER_KIND)]}
        for name, pr in n_kinds(rng, A, L1, L2, k).items():
            made[name] = [pr] + [with_n(rng, L1, L2, [(t, int(p)) for t in (0, 1) for p in np.flatnonzero((pr[t] == ord("N")))]) for _ in range(PER_KIND - 1)]
        if k <= 17:
            nm = near_miss_kmers(monkeypatch, k)
            made["tag-A"] = [planted(rng, nm, base.elsewhere_pair(rng, L1, L2), k, [even()]) for _ in range(PER_KIND)]
            made["tag-B"] = [planted(rng, nm, base.elsewhere_pair(rng, L1, L2), k, [odd()]) for _ in range(PER_KIND)]
            made["tag-AB"] = [planted(rng, nm, base.elsewhere_pair(rng, L1, L2), k, [2 * i, 61 + 2 * i]) for i in range(PER_KIND)]
            # (`under` covers mate 1's [0, 60): the planted k-mer behind it, in an even slot, would add k bases)
            made["tag-under"] = [planted(rng, nm, runs_kind(rng, A, L1, L2, k, 0, 1), k, [80 + 2 * i]) for i in range(PER_KIND)]
        idx = {name: A.add(prs) for name, prs in made.items()}
        settled = A.add([base.gene_pair(rng, L1, L2) for _ in range(3 * len(idx) + 6)])
        assert all(A.assigned(i) for i in settled)
        for name, ii in idx.items():
            want = name in ("by-A", "by-A-runs", "by-prefix")
            assert all(A.assigned(i) == want for i in ii), (name, [A.assigned(i) for i in ii])
        _kinds[key] = (A, idx, settled)
    return _kinds[key]


def pattern_batch(case, combo, first):
    """one triple per kind, the kinds in turn from `first`: bit p of combo = pair p is a settled one, else the kind's"""
    A, idx, settled = case
    names = sorted(idx)
    names = names[first % len(names):] + names[:first % len(names)]
    out = []
    for t, name in enumerate(names):
        out += [settled[3 * t + p] if (combo >> p) & 1 else idx[name][(3 * combo + p) % PER_KIND] for p in range(3)]
    return A.batch(out)


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", [True, False], ids=["tiles", "no-tiles"])
@pytest.mark.parametrize("combo", range(8))
def test_every_kind_in_every_pattern_of_a_triple(oracle, monkeypatch, combo, tiles):
    """every kind as the open pair(s) of this pattern; turn by turn each kind's triple is the batch's first, a middle and its last"""
    case = kinds(oracle, monkeypatch, 17, 150, 150)
    h = base.make_handle(monkeypatch, 17, env=None if tiles else {"SHK_TILE_FIRST": "0"})
    n_kinds_ = len(case[1])
    for first in range(n_kinds_):
        b, want = pattern_batch(case, combo, first)
        base.run(h, b, want, ("pattern", combo, first, tiles), 150, 150, SHIFTS[first % 4], tiles=tiles)
    h.close()


M = 2000
ENDS = list(range(1, 9)) + [3 * M, 3 * M + 1, 3 * M + 2]


def long_batch(case, n, start):
    """n pairs: the kinds and the settled pairs by turns, from kind `start`"""
    A, idx, settled = case
    names = sorted(idx)
    out = []
    for i in range(n):
        j = i + start
        out.append(settled[j % len(settled)] if j % 4 == 3 else idx[names[(j // 4 * 3 + j % 4) % len(names)]][(j // 7) % PER_KIND])
    return A.batch(out)


@pytest.mark.parametrize("tiles", [True, False], ids=["tiles", "no-tiles"])
def test_ends_of_a_batch(oracle, monkeypatch, tiles):
    """1 ... 8 and 3 m + {0, 1, 2} pairs as exact-size views at byte shifts 0 ... 3: a partial last triple, whichever kind ends the batch"""
    case = kinds(oracle, monkeypatch, 17, 150, 150)
    h = base.make_handle(monkeypatch, 17, env=None if tiles else {"SHK_TILE_FIRST": "0"})
    for j, n in enumerate(ENDS):
        for s, shift in enumerate(SHIFTS):
            b, want = long_batch(case, n, 5 * j + s)
            assert len(b["off1"]) - 1 == n
            base.run(h, b, want, ("ends", n, shift, tiles), 150, 150, shift, tiles=tiles)
    h.close()


@pytest.mark.parametrize("L1,L2", SHAPES[1:], ids=["%dx%d" % s for s in SHAPES[1:]])
def test_the_other_lengths(oracle, monkeypatch, L1, L2):
    case = kinds(oracle, monkeypatch, 17, L1, L2)
    h = base.make_handle(monkeypatch, 17)
    for combo, shift in zip((0, 3, 5, 6), SHIFTS):
        b, want = pattern_batch(case, combo, combo)
        base.run(h, b, want, ("lengths", L1, L2, combo, shift), L1, L2, shift)
    b, want = long_batch(case, 601, 2)
    base.run(h, b, want, ("lengths", L1, L2, "long"), L1, L2, SHIFTS[1])
    h.close()


@pytest.mark.parametrize("tiles", [True, False], ids=["tiles", "no-tiles"])
def test_the_hashed_twin(oracle, monkeypatch, tiles):
    """k = 19: XXH64 probes, one stage; the same path"""
    case = kinds(oracle, monkeypatch, 19, 150, 150)
    assert "tag-A" not in case[1]
    h = base.make_handle(monkeypatch, 19, env=None if tiles else {"SHK_TILE_FIRST": "0"})
    for combo, shift in zip((0, 1, 2, 4, 7), SHIFTS + SHIFTS[:1]):
        b, want = pattern_batch(case, combo, combo)
        base.run(h, b, want, ("hashed", combo, shift, tiles), 150, 150, shift, tiles=tiles)
    for n in (7, 6001):
        b, want = long_batch(case, n, 1)
        base.run(h, b, want, ("hashed", n, tiles), 150, 150, SHIFTS[2], tiles=tiles)
    h.close()


def test_twenty_one_chunks(oracle, monkeypatch):
    """145 + 161 bases: 10 + 11 chunks of 16 bases, the most a pair of the three-pairs kernel has, and the sparse order on with T = 5;
    an N in every one of the 21 chunks (the threshold table's last entry in use), and the other N counts"""
    L1, L2, k = 145, 161, 17
    assert base.tri_fits(L1, L2, k, 5) and (L1 + 15) // 16 + (L2 + 15) // 16 == 21
    T, sp_ub, _ = plan_of(L1, L2, k)
    assert T == 5 and sp_ub == 183 < thr_of(L1 + L2) == 184
    rng = np.random.default_rng(2121)
    A = base.answers(oracle, k)
    nk = n_kinds(rng, A, L1, L2, k)
    prs = []
    for i in range(20):
        prs += [nk[name] for name in sorted(nk)] + [base.elsewhere_pair(rng, L1, L2), base.gene_pair(rng, L1, L2), one_kmer(rng, L1, L2, k, 0, 2 * i), one_kmer(rng, L1, L2, k, 0, 2 * i + 1)]
    idx = A.add(prs)
    for tiles in (True, False):
        h = base.make_handle(monkeypatch, k, env=None if tiles else {"SHK_TILE_FIRST": "0"})
        for cut, shift in zip((0, 1, 2), SHIFTS):
            b, want = A.batch(idx[:len(idx) - cut])
            base.run(h, b, want, ("21 chunks", cut, shift, tiles), L1, L2, shift, tiles=tiles)
        h.close()


def test_short_pairs_through_the_offsets_form(oracle, monkeypatch):
    """mixed lengths: a short pair's spUb and threshold are its own.  The trimmed batch of tests/test_gpu_triple_loads_results.py (short
    pairs at p = 0, 1, 2 on both sides of their own thresholds) with, in between, short pairs from elsewhere -- plain, with one k-mer of
    the gene in A, in B, and with enough N that the pair's own spUb reaches its own threshold: not cut behind B"""
    A, idx = base.trimmed_case(oracle)
    k = 17
    rng = np.random.default_rng(909)
    prs, sides = [], set()
    for i in range(48):
        l1, l2 = int(rng.integers(122, 150)), int(rng.integers(118, 150))
        kind = i % 4
        if kind == 0:
            pr = base.elsewhere_pair(rng, l1, l2)
        elif kind == 1:
            pr = one_kmer(rng, l1, l2, k, 0, 2 * int(rng.integers(0, 50)))
        elif kind == 2:
            pr = one_kmer(rng, l1, l2, k, 0, 2 * int(rng.integers(0, 50)) + 1)
        else:
            pr = with_n(rng, l1, l2, [(0, int(p)) for p in rng.choice(100, size=60 + i % 7, replace=False)])
        genes, mx, ln = A.analyze(pr)
        ub = bases_behind(121, l1, l2, k)                                   # (the layout's prefix: T = 7 at 2 x 150)
        sides.add((i % 3, ub < thr_of(ln)))
        assert not genes and (ub < thr_of(ln)) == (kind != 3), (l1, l2, ln, ub)
        prs.append(pr)
    assert sides == {(p, s) for p in range(3) for s in (True, False)}
    extra = A.add(prs)
    mixed = []
    for t in range(len(extra)):
        mixed += idx[3 * t:3 * t + 3]
        mixed.insert(len(mixed) - t % 3, extra[t])                          # the short pair at p = 2, 1, 0 of its triple by turns ...
    mixed = mixed[:len(mixed) // 3 * 3]
    for tiles in (True, False):
        h = base.make_handle(monkeypatch, k, env=None if tiles else {"SHK_TILE_FIRST": "0"})
        for cut, shift in zip((0, 1, 2), SHIFTS[1:]):
            b, want = A.batch(mixed[:len(mixed) - cut])
            base.run(h, b, want, ("short pairs", cut, shift, tiles), 150, 150, shift, tiles=tiles, offsets=True)
        h.close()
