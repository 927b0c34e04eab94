"""The candidate stages of the rounds A and B of a pair's miss path issued as ONE block (classify_uni.hpp, per_pair, SP_JOINT:
classify_uni_tiles.inc lx_candidates2) on the k-mer keyed LDS table: both rounds' windows, both D reads, both T16 reads, two ballots,
the bound cut -- and B's answer handed to sparse_first whatever A's was.  The same slots are probed with the same rule as before;
only the order of issue changes, and B's stage now also runs for a pair that A alone settles.  No result may change: every pair of
every batch is held against the oracle -- its count, its ids --, the device's per-gene counters, reset before the batch, against
the histogram of the oracle's ids, and last_kernel() is asserted per run (the helpers of tests/test_gpu_triple_loads_results.py and
tests/test_gpu_sparse_miss_path.py; the tiles' round comes from a primed handle, its twin from SHK_TILE_FIRST=0).

One gene of 6 000 bases, c = 0.6, 2^33 bits, k = 17; 2 x 150 bp (T = 7 tiles) and 145 + 161 bp (21 chunks, T = 5).
  * cross-talk between the pairs of a triple: every triple over {elsewhere, only-A, only-B, by-A, N with spUb >= thr} in all three
    positions, 125 triples in one batch, through the headline kernel (by-A pairs fail the tiles' round, pairs from the gene would be
    settled by it) and through the twin
  * A and B at once within one pair: a true k-mer in an even AND in an odd slot; false 16-bit candidates in both rounds (tag-AB); a
    pair that A's coverage settles at exactly the threshold with a false candidate in B; and `under` (coverage thr - 1) with a false
    candidate in B, which must not lift it -- the B stage that now always runs changes no verdict of A's
  * `under` beside pairs at exactly the threshold, in one triple
  * the batch's end: n = 1 ... 8 and 3 m + 1, 3 m + 2 pairs, the last triple's open pair(s) in position 0 and 1, views at byte shifts 0 ... 3
  * pairs whose threshold needs the wave reduction (two N in one chunk) in triples whose other pairs do not
  * one control at k = 19, the hashed twin: it KEEPS the serial order of the two rounds (no registers for two XXH64 states; SP_JOINT is
    a form of the k-mer keyed instantiations only), and nothing moved there

Run on the GPU box with `pytest -m gpu`."""
import itertools

import numpy as np
import pytest

import torch  # noqa: F401  (torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both)

from tests import test_gpu_sparse_miss_path as sp
from tests import test_gpu_triple_loads_results as base

pytestmark = pytest.mark.gpu

SHIFTS = base.SHIFTS
FIVE = ("elsewhere", "only-A", "only-B", "by-A", "N-many")
TWIN = {"SHK_TILE_FIRST": "0"}


def both_ways(monkeypatch, k, L1, L2, runs):
    """runs = [(batch, want, what, shift)]: each through the headline kernel (primed handle) and through the twin"""
    for tiles in (True, False):
        h = base.make_handle(monkeypatch, k, env=None if tiles else TWIN)
        for b, want, what, shift in runs:
            base.run(h, b, want, (what, "tiles" if tiles else "twin"), L1, L2, shift, tiles=tiles)
        h.close()


def triples_over(A, pools, names):
    """every triple over `names` in all three positions, one batch; pools[name]: indices into A's pool, taken in turn"""
    at = dict.fromkeys(names, 0)
    out = []
    for combo in itertools.product(names, repeat=3):
        for name in combo:
            out.append(pools[name][at[name] % len(pools[name])])
            at[name] += 1
    return A.batch(out)


def test_cross_talk_between_the_pairs_of_a_triple(oracle, monkeypatch):
    A, idx, _ = sp.kinds(oracle, monkeypatch, 17, 150, 150)
    T, sp_ub, _ = sp.plan_of(150, 150, 17)
    assert T == 7 and sp_ub == 179
    b, want = triples_over(A, idx, FIVE)
    assert len(b["off1"]) - 1 == 375
    both_ways(monkeypatch, 17, 150, 150, [(b, want, "cross-talk", SHIFTS[1])])


_wide = {}


def wide_case(oracle):
    """the five kinds at 145 + 161 bases (T = 5): made here, the pools of tests/test_gpu_sparse_miss_path.py are 2 x 150 bp's"""
    if not _wide:
        L1, L2, k = 145, 161, 17
        T, sp_ub, _ = sp.plan_of(L1, L2, k)
        assert T == 5 and sp_ub == 183 < base.thr_of(L1 + L2)
        rng = np.random.default_rng([L1, L2, 4242])
        A = base.answers(oracle, k)
        n_many = sp.n_kinds(rng, A, L1, L2, k)["N-many"]
        where = [(t, int(p)) for t in (0, 1) for p in np.flatnonzero(n_many[t] == ord("N"))]
        made = {"elsewhere": [base.elsewhere_pair(rng, L1, L2) for _ in range(6)],
                "only-A": [sp.one_kmer(rng, L1, L2, k, 0, 2 * int(rng.integers(0, (128 - T + 1) // 2))) for _ in range(6)],   # even slots of the prefix
                "only-B": [sp.one_kmer(rng, L1, L2, k, 0, 2 * int(rng.integers(0, 55)) + 1) for _ in range(6)],              # odd slots
                "by-A": [sp.by_a_pair(rng, L1, L2, k) for _ in range(6)],
                "N-many": [n_many] + [sp.with_n(rng, L1, L2, where) for _ in range(5)]}
        idx = {name: A.add(prs) for name, prs in made.items()}
        for name, ii in idx.items():
            assert all(A.assigned(i) == (name == "by-A") for i in ii), name
        _wide["case"] = (A, idx)
    return _wide["case"]


def test_cross_talk_at_twenty_one_chunks(oracle, monkeypatch):
    A, idx = wide_case(oracle)
    b, want = triples_over(A, idx, FIVE)
    both_ways(monkeypatch, 17, 145, 161, [(b, want, "cross-talk 145+161", SHIFTS[2])])


_both = {}


def both_rounds_case(oracle, monkeypatch):
    """pairs with something in round A AND in round B"""
    if not _both:
        L1 = L2 = 150
        k = 17
        A, idx, _ = sp.kinds(oracle, monkeypatch, k, L1, L2)
        nm = sp.near_miss_kmers(monkeypatch, k)
        rng = np.random.default_rng(1717)
        thr = base.thr_of(L1 + L2)
        # true k-mers of the gene in an even slot (round A, lane s / 2) and an odd one (round B), apart: each covers k bases, no gene
        true_ab = [base.runs_pair(rng, L1, L2, [(0, 2 * i, k), (0, 2 * i + 41, k)])[:2] for i in range(0, 30, 5)]
        # by-A-runs covers mate 1's [0, 61) and the tiles: exactly thr in A.  A false candidate in an odd slot behind the run
        exact_tag_b = [sp.planted(rng, nm, sp.runs_kind(rng, A, L1, L2, k, 0, 0), k, [81 + 2 * i]) for i in range(6)]
        # the same one base short (thr - 1 over the whole prefix): a false hit in B would lift it over the threshold
        under_tag_b = [sp.planted(rng, nm, sp.runs_kind(rng, A, L1, L2, k, 0, 1), k, [81 + 2 * i]) for i in range(6)]
        made = {"true-AB": A.add(true_ab), "exact-tag-B": A.add(exact_tag_b), "under-tag-B": A.add(under_tag_b)}
        for pr in exact_tag_b:
            genes, mx, ln = A.analyze(pr)
            assert mx == thr and len(genes) == 1, (mx, thr, genes)
        for pr in under_tag_b:
            genes, mx, ln = A.analyze(pr)
            assert mx == thr - 1 and not genes, (mx, thr, genes)
        assert not any(A.assigned(i) for i in made["true-AB"] + made["under-tag-B"]) and all(A.assigned(i) for i in made["exact-tag-B"])
        made["tag-AB"] = idx["tag-AB"]
        made["elsewhere"] = idx["elsewhere"]
        _both["case"] = (A, made)
    return _both["case"]


def test_a_and_b_at_once_within_one_pair(oracle, monkeypatch):
    A, made = both_rounds_case(oracle, monkeypatch)
    names = ("true-AB", "tag-AB", "exact-tag-B", "under-tag-B")
    alone = [i for name in names for i in made[name][:3]]                  # each kind filling its triple
    b1, w1 = A.batch(alone)
    b2, w2 = triples_over(A, made, names + ("elsewhere",))
    both_ways(monkeypatch, 17, 150, 150, [(b1, w1, "A and B, alone", SHIFTS[0]), (b2, w2, "A and B, mixed", SHIFTS[3])])


def test_under_beside_the_threshold(oracle, monkeypatch):
    """coverage thr - 1 (`under`) beside coverage exactly thr, by round A (`by-A-runs`) and by the whole prefix (`by-prefix`)"""
    A, idx, _ = sp.kinds(oracle, monkeypatch, 17, 150, 150)
    b, want = triples_over(A, idx, ("under", "by-A-runs", "by-prefix"))
    both_ways(monkeypatch, 17, 150, 150, [(b, want, "under", SHIFTS[1])])


M = 300
ENDS = list(range(1, 9)) + [3 * M + 1, 3 * M + 2]
OPEN = ("elsewhere", "only-B", "only-A", "tag-AB", "N-one")


def test_the_batchs_end(oracle, monkeypatch):
    """n pairs, the kinds and settled pairs by turns; the last triple's pairs -- one at 3 m + 1, two at 3 m + 2 -- are open ones"""
    A, idx, settled = sp.kinds(oracle, monkeypatch, 17, 150, 150)
    names = sorted(idx)
    runs = []
    for j, n in enumerate(ENDS):
        out = []
        for i in range(n):
            q = i + 3 * j
            out.append(settled[q % len(settled)] if q % 4 == 3 else idx[names[q % len(names)]][(q // 5) % sp.PER_KIND])
        for p in range(min(n, n % 3 if n % 3 else 3)):
            out[n - 1 - p] = idx[OPEN[(j + p) % len(OPEN)]][(j + p) % sp.PER_KIND]
        b, want = A.batch(out)
        assert len(b["off1"]) - 1 == n
        runs += [(b, want, ("end", n, shift), shift) for shift in SHIFTS]
    both_ways(monkeypatch, 17, 150, 150, runs)


def test_pairs_whose_threshold_takes_the_reduction(oracle, monkeypatch):
    """two N in one chunk: the pair's threshold is the wave reduction's, not the table's; beside pairs of the table's"""
    A, idx, _ = sp.kinds(oracle, monkeypatch, 17, 150, 150)
    b, want = triples_over(A, idx, ("N-two-in-a-chunk", "elsewhere", "only-B", "N-one"))
    both_ways(monkeypatch, 17, 150, 150, [(b, want, "reduction", SHIFTS[2])])


def test_the_hashed_twin_keeps_the_serial_order(oracle, monkeypatch):
    """k = 19: XXH64 probes.  That instantiation kept round B behind round A's ballot; its results are what they were"""
    A, idx, _ = sp.kinds(oracle, monkeypatch, 19, 150, 150)
    b, want = triples_over(A, idx, FIVE)
    h = base.make_handle(monkeypatch, 19)
    assert h.debug_kx_meta()["kx_in_use"] == 0
    base.run(h, b, want, "hashed control", 150, 150, SHIFTS[1])
    h.close()
