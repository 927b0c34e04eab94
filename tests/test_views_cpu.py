"""tests/views.py against the CPU oracle: the generators' reads sit where they were designed to sit -- on the steps around the
threshold, one leaked base away from passing -- and embed places the views where it was asked to.  Without these conditions
tests/test_gpu_views.py could pass on kernels that leak."""
from fractions import Fraction

import numpy as np
import pytest

from tests import evidence_model, synth, views

def _oracle(oracle, genes, k, c, bf_bits=1 << 30, q=0):
    o = oracle.Shark(k=k, c=c, bf_bits=bf_bits, min_quality=q)
    o.build([bytes(g) for g in genes])
    return o


def _assoc(o, batch):
    return synth.assoc_lists(*o.classify(batch["seq1"], batch["off1"], batch["seq2"], batch["off2"], batch["qual1"], batch["qual2"]))


@pytest.mark.parametrize("c,length", views.THRESHOLD_PAIRS)
def test_threshold_pairs_sit_on_an_integer(oracle, c, length):
    """the exact product c * len is an integer N; fp64 puts it above N, below it ((0.57, 300)) or on it ((0.5, 252)); the oracle
    accepts coverage N accordingly, rejects N - 1 (N where fp64 is above) and accepts the step above"""
    exact = Fraction(int(round(c * 100)), 100) * length
    assert exact.denominator == 1
    N = int(exact)
    prod = float(c) * float(length)
    want = {(0.57, 300): "below", (0.5, 252): "exact"}.get((c, length), "above")
    assert ("above" if prod > N else "below" if prod < N else "exact") == want
    thr = views.threshold(c, length)
    assert thr == (N + 1 if want == "above" else N)
    genes = views.reference(1)
    batch, design = views.ladder_case(genes, 17, c, length)
    o = _oracle(oracle, genes, 17, c)
    ev = evidence_model.expected_evidence(o, batch)
    got = _assoc(o, batch)
    seen = set()
    for i, (cov, ln, step, form) in enumerate(design):
        assert int(ev[i][0]) == cov and ev[i][2] == ln == length and ev[i][1] > 0, (i, form, ev[i], cov)
        assert (len(got[i]) > 0) == (cov >= thr), (i, cov, thr)
        seen.add(cov)
    assert {N - 1, N, N + 1} <= seen          # the oracle was asked about N itself, and about both its neighbours
    assert np.array_equal(evidence_model.passes(ev, c), np.array([d[0] >= thr for d in design]))


_oracles = {}


def _route_oracle(oracle, n_genes, bf_bits, q, k, c):
    key = (n_genes, bf_bits, q, k, c)
    if key not in _oracles:
        _oracles[key] = _oracle(oracle, views.reference(n_genes), k, c, bf_bits, q)
    return _oracles[key]


@pytest.mark.parametrize("n_genes,bf_bits,q,k,c,length,invalid,ragged", views.all_ladder_cases())
def test_ladder_reads_cover_what_they_were_designed_to(oracle, n_genes, bf_bits, q, k, c, length, invalid, ragged):
    """every ladder batch the GPU file runs, on its route's reference, filter and -q: max == the designed coverage, len == the designed
    length, nk > 0; associations exactly from the threshold up; per placement form at least PER_STEP reads at thr - 1 and at thr.
    The one thing that takes a read off its design is a false positive of the Bloom filter under one of its random k-mers (it adds
    up to k to a gene's coverage): with s set bits in a filter of b bits a read of 300 bases meets one with probability 300 s / b --
    6 . 10^-4 on one gene in 2^30 bits, 5 % and 7 % on the six genes of the table routes in 2^26 and 3 . 2^24 bits.  So at most one read
    per batch may miss on the large filters and one in ten on the small ones, and the counts per form are taken over the reads that
    sit on their design."""
    genes = views.reference(n_genes)
    batch, design = views.ladder_case(genes, k, c, length, qual=q > 0, invalid=invalid, ragged=ragged)
    o = _route_oracle(oracle, n_genes, bf_bits, q, k, c)
    ev = evidence_model.expected_evidence(o, batch)
    got = _assoc(o, batch)
    at, off_design = {}, 0
    for i, (cov, ln, step, form) in enumerate(design):
        assert cov - views.threshold(c, ln) == step
        assert int(ev[i][2]) == ln and ev[i][1] > 0 and int(ev[i][0]) >= cov, (i, form, step, ev[i], cov, ln)
        if int(ev[i][0]) != cov:
            off_design += 1
            continue
        assert (len(got[i]) > 0) == (step >= 0), (i, form, step)
        at[(form, step)] = at.get((form, step), 0) + 1
    assert off_design <= (1 if bf_bits >= 1 << 30 else len(design) // 10), (off_design, len(design))
    forms = {f for f, _ in at}
    assert "split" in forms or length == 150
    assert any(f.startswith("two-runs") for f in forms)
    if invalid and not ragged:
        assert {d[1] for d in design} >= {length - 1, length - 2, length - 3}
    for f in forms:
        for step in (-1, 0):
            assert at.get((f, step), 0) >= views.PER_STEP, (f, step)


def _one(o, m1, m2):
    joined = bytes(m1) + (b"N" + bytes(m2) if m2 is not None else b"")
    genes, mx, _, ln = o.analyze(joined)
    return tuple(genes), mx, ln


def _hostile_check(o, k, c, L2, batch, marked, lead, trail, trimmed):
    reads = views.reads_of(batch)
    assert len(lead[0]) >= k and len(trail[0]) >= k
    good, kinds, short = 0, set(), 0
    for mark in marked:
        i, t, end = mark
        m = [reads[i][0], reads[i][1]]
        assert reads[i][2] is None or ((reads[i][2] == views.HI_Q).all() and (reads[i][3] is None or (reads[i][3] == views.HI_Q).all()))
        plain = _one(o, m[0], m[1])
        b = np.array([views.neighbour_byte(batch, mark, lead, trail)], np.uint8)
        m[t] = np.concatenate([m[t], b]) if end == "end" else np.concatenate([b, m[t]])
        leaked = _one(o, m[0], m[1])
        ok = len(plain[0]) == 0 and len(leaked[0]) > 0 and plain[1] == views.threshold(c, plain[2]) - 1
        good += ok
        if ok:
            kinds.add((t, end))
            short += len(reads[i][t]) == k - 1
    assert good >= 0.9 * len(marked), (good, len(marked))
    assert kinds == {(t, e) for t in ((0, 1) if L2 else (0,)) for e in ("end", "begin")}
    assert marked[0][0] == 0 and marked[-1][0] == len(reads) - 1          # the batch's edges are hostile to the lead and the trail
    assert (short > 0) == trimmed
    assert 300 <= len(reads) <= 700


@pytest.mark.parametrize("n_genes,bf_bits,q,L1,L2,trimmed,seed", views.all_mixed_cases())
def test_hostile_reads_flip_under_one_leaked_byte(oracle, n_genes, bf_bits, q, L1, L2, trimmed, seed):
    """every mixed batch the GPU file runs: each hostile read (qualities of phred 40 throughout, so -q masks none of its bases) is
    rejected as it is and accepted once the one byte of the buffer behind (before) the marked mate is let in -- at least 90 % of
    them (a chance match elsewhere spoils one now and then); both mates, both ends, the batch's own first and last read against
    the lead and the trail; in trimmed batches mates of k - 1 bases too"""
    genes = views.reference(n_genes)
    o = _route_oracle(oracle, n_genes, bf_bits, q, views.K, views.C)
    batch, marked, lead, trail = views.mixed_case(genes, views.K, views.C, L1, L2, qual=q > 0, trimmed=trimmed, seed=seed)
    _hostile_check(o, views.K, views.C, L2, batch, marked, lead, trail, trimmed)


@pytest.mark.parametrize("k,L1,L2,c", [(31, 150, 150, 0.56), (17, 100, 100, 0.55), (17, 150, 0, 0.68), (16, 300, 300, 0.56)])
def test_hostile_reads_at_other_k_and_lengths(oracle, k, L1, L2, c):
    """the generator beyond the GPU file's own batches: k = 31 and 16, 2 x 100, single-end"""
    genes = views.reference(3)
    batch, marked, lead, trail = views.mixed_case(genes, k, c, L1, L2)
    _hostile_check(_oracle(oracle, genes, k, c), k, c, L2, batch, marked, lead, trail, False)


def test_embed_places_every_view_where_it_was_asked_to(oracle):
    genes = views.reference(3)
    batch, marked, lead, trail = views.mixed_case(genes, 17, 0.56, 151, 101, qual=True)
    for s in range(4):
        for o1, o2 in ((0, 8), (8, 0), (8, 8), (0, 0)):
            sh = views.shifts_of(s, (s + 2) % 4, (s + 1) % 4, (s + 3) % 4, o1, o2)
            e = views.embed(batch, sh, lead, trail)
            for name in views.BYTE_ARRAYS + views.OFF_ARRAYS:
                big, d = e["arrays"][name], e["disp"][name]
                assert big.ctypes.data % 16 == 0                       # (the device allocation is aligned at least as well)
                v = views.view_of(e, name, len(batch[name]))
                assert v.ctypes.data == big.ctypes.data + d and np.array_equal(v, batch[name])
                if name in views.OFF_ARRAYS:
                    assert v.ctypes.data % 16 == sh[name] and d == sh[name]
                    assert (big[:d // 8] == views.POISON).all() and (big[d // 8 + len(v):] == views.POISON).all() and len(big) > d // 8 + len(v)
                else:
                    assert v.ctypes.data % 4 == sh[name] % 4 and d >= 16 and len(big) >= d + len(v) + 16
            for t, name in ((0, "seq1"), (1, "seq2")):
                big, d, n = e["arrays"][name], e["disp"][name], len(batch[name])
                assert np.array_equal(big[d - len(lead[t]):d], lead[t]) and np.array_equal(big[d + n:d + n + len(trail[t])], trail[t])
            for name in ("qual1", "qual2"):
                big, d, n = e["arrays"][name], e["disp"][name], len(batch[name])
                assert (big[:d] == views.HI_Q).all() and (big[d + n:] == views.HI_Q).all()


def test_with_first_offset_keeps_the_reads(oracle):
    genes = views.reference(1)
    batch, marked, lead, trail = views.mixed_case(genes, 17, 0.56, 150, 150, qual=True)
    for o1, o2 in ((1, 0), (0, 5), (8, 8), (150, 150), (150, 0)):
        b = views.with_first_offset(batch, o1, o2, lead)
        assert int(b["off1"][0]) == o1 and int(b["off2"][0]) == o2
        assert all(all(np.array_equal(x, y) for x, y in zip(r, s)) for r, s in zip(views.reads_of(b), views.reads_of(batch)))
        if o1:
            assert np.array_equal(b["seq1"][max(0, o1 - len(lead[0])):o1], lead[0][-o1:]) and len(b["qual1"]) == len(b["seq1"])
