"""CPU tests (no GPU) of tests/repeat_refs.py: the generator is deterministic, and the oracle's index of each builder's reference
has the property the builder is for -- so the GPU tests on these references (tests/test_gpu_repeats.py) cannot be vacuous.
Also the replay of tests/golden/ref_repeat_cases.npz (the reference program's recorded answers on one case per builder)
through oracle_cli and the oracle's batch API."""
import os

import numpy as np
import pytest

from tests import ref_cases as rc
from tests import repeat_refs as rr
from tests import synth

K = 17
BITS = 1 << 30          # sparse: no two reference k-mers share a filter bit (checked where a test relies on it)


def _index(oracle, genes, k=K, bf_bits=BITS):
    o = oracle.Shark(k=k, c=0.0, bf_bits=bf_bits)
    o.build([bytes(g) for g in genes])
    return o


def _lists(o):
    """the oracle's gene lists, one per set bit in bit order: runs of ascending ids in index_kmer (no wrap: ids ascend inside a
    list and a new list starts where they do not) -- only used where the set bits are also counted another way"""
    ids = o.index_kmer().astype(np.int64)
    cut = np.flatnonzero(np.diff(ids) <= 0) + 1
    return np.split(ids, cut)


def _canon_kmers(g, k=K):
    """the distinct canonical k-mers of one record (ACGT in either case; anything else cuts), as byte strings"""
    s = bytes(g).upper()
    out = set()
    for i in range(len(s) - k + 1):
        w = s[i:i + k]
        if set(w) <= set(b"ACGT"):
            out.add(min(w, rc.revcomp(w)))
    return out


def _list_of(o, kmer):
    """the gene list the oracle keeps for one k-mer, through a read that is that k-mer (c = 0: every gene of the list ties)"""
    b = synth.batch_from_lists([bytes(kmer)])
    goff, gids = o.classify(b["seq1"], b["off1"])
    return [int(x) for x in gids]


def test_same_seed_same_bytes():
    def everything(seed):
        rng = np.random.default_rng(seed)
        genes, marks = rr.compose(rr.families(rng, 2, 4, 500, 0.95), rr.interspersed(rng, [], 120, 30, 0.1), rr.low_complexity(rng, [], K),
                                  rr.tandem(rng, 80, 6, True), rr.saturated_neighbourhood(rng, K, 15), rr.shared_motif(rng, 50), rr.mixed_reference(rng))
        pairs = rr.boundary_sweeps(genes, marks, 100, step=7) + rr.pure(100) + rr.polya_tail(rng, 100)
        b = rr.batch(rr.dress(rng, pairs, 0.01, 0.002, 0.2), ragged_rng=rng, qual_rng=rng)
        return b"".join(bytes(g) for g in genes) + repr(marks).encode() + b"".join(bytes(v) for v in b.values() if v is not None)
    assert everything(5) == everything(5)
    assert everything(5) != everything(6)


def test_families(oracle):
    rng = np.random.default_rng(1)
    genes, marks = rr.families(rng, 3, 8, 1200, 0.97)
    assert len(genes) == 3 * 8 + 2
    o = _index(oracle, genes)
    # members of a family share most of their k-mers with some sibling, families share none
    k0 = _canon_kmers(genes[0])
    assert len(k0 & set().union(*[_canon_kmers(g) for g in genes[1:8]])) > 0.4 * len(k0)
    assert not (k0 & _canon_kmers(genes[8]))
    # identical lists for a gene, its duplicate and its reverse complement: every k-mer of gene 0 names all three
    dup, rev = 24, 25
    assert bytes(genes[dup]) == bytes(genes[0]) and bytes(genes[rev]) == rc.revcomp(bytes(genes[0]))
    for i in range(0, len(genes[0]) - K + 1, 37):
        got = _list_of(o, genes[0][i:i + K])
        assert {0, dup, rev} <= set(got) and got == sorted(got)
    assert o.num_kmer() == len(set().union(*[_canon_kmers(g) for g in genes]))
    longest = max(len(x) for x in _lists(o))
    assert longest >= 8                               # some k-mer survives in five paralogs or more (+ duplicate + reverse complement)
    o.close()


@pytest.mark.parametrize("n_carriers", [50, 1000])
def test_interspersed(oracle, n_carriers):
    rng = np.random.default_rng(2)
    base, _ = rr.plain(rng, 20, 300, 800)
    genes, marks = rr.interspersed(rng, base, 200, n_carriers, 0.15)
    assert len(marks) == n_carriers and len(genes) == max(20, n_carriers)
    assert any(m["rev"] for m in marks) and not all(m["rev"] for m in marks)
    o = _index(oracle, genes)
    longest = max(len(x) for x in _lists(o))
    exact = sum(m["rate"] == 0.0 for m in marks)
    assert exact >= n_carriers // 2
    assert n_carriers >= longest >= exact             # the conserved k-mers' lists: every exact copy, and more where a diverged copy keeps the k-mer
    m = marks[0]
    el = genes[m["gene"]][m["start"]:m["end"]]
    assert len(_list_of(o, el[50:50 + K])) >= exact
    assert any(len(x) == 1 for x in _lists(o))        # private lists: the carriers' own sequence and the diverged k-mers
    o.close()


@pytest.mark.parametrize("k", [11, 16, 17, 21, 31])
def test_low_complexity(oracle, k):
    rng = np.random.default_rng(3)
    genes, marks = rr.low_complexity(rng, [], k)
    kinds = [m["kind"] for m in marks]
    assert kinds.count("homopolymer") == 10 and {"homopolymer-complement", "period2-AC", "period2-AT", "period3", "period-k-1", "run-with-N",
                                                 "run-lower-case", "run-at-start", "run-at-end", "run-only"} <= set(kinds)
    runs = sorted(m["n"] for m in marks if m["kind"] == "homopolymer")
    assert runs == sorted([k - 1, k, k + 1, 100, 253, 254, 255, 256, 300, 1000])
    for m in marks:                                   # the run is where the mark says, and the flanks do not prolong it
        g = genes[m["gene"]]
        if m["kind"] == "homopolymer":
            assert bytes(g[m["start"]:m["end"]]) == b"A" * m["n"]
            assert m["start"] == 0 or g[m["start"] - 1] != ord("A")
            assert m["end"] == len(g) or g[m["end"]] != ord("A")
    only = next(m for m in marks if m["kind"] == "run-only")
    assert bytes(genes[only["gene"]]) == b"T" * 200
    assert next(m for m in marks if m["kind"] == "run-at-start")["start"] == 0
    e = next(m for m in marks if m["kind"] == "run-at-end")
    assert e["end"] == len(genes[e["gene"]])
    # a homopolymer run of length n >= k contributes exactly one set bit: a record that is nothing but the run has one k-mer, and the
    # whole reference has as many set bits as distinct canonical k-mers (the filter is sparse enough for that to be checkable)
    o1 = _index(oracle, [genes[only["gene"]]], k=k)
    assert o1.num_kmer() == 1 and len(o1.index_kmer()) == 1
    o1.close()
    o = _index(oracle, genes, k=k)
    distinct = set().union(*[_canon_kmers(g, k) for g in genes])
    assert o.num_kmer() == len(distinct)
    # poly-A / poly-T: ONE canonical k-mer, listed for every gene with an A or T run of k bases or more (9 A runs, the T run of 300, the record of T)
    got = _list_of(o, b"A" * k)
    want = sorted(m["gene"] for m in marks if m["kind"] in ("homopolymer", "homopolymer-complement", "run-only") and m["n"] >= k)
    assert got == want and len(got) == 11
    assert _list_of(o, b"T" * k) == got
    # (AT)n: for even k both windows, ATAT..AT and TATA..TA, are their own reverse complement (two canonical k-mers, each a
    # palindrome); for odd k one window is the other's reverse complement (one canonical k-mer)
    at = next(m for m in marks if m["kind"] == "period2-AT")
    assert len(_canon_kmers(genes[at["gene"]][at["start"]:at["end"]], k)) == (2 if k % 2 == 0 else 1)
    # the run broken by N: two runs of 60 and 59 -> still that one k-mer; the lower-case stretch does not cut
    for kind in ("run-with-N", "run-lower-case"):
        m = next(x for x in marks if x["kind"] == kind)
        assert len(_canon_kmers(genes[m["gene"]][m["start"]:m["end"]], k)) == 1
    o.close()


@pytest.mark.parametrize("unit_len,copies,drift", [(40, 30, False), (400, 2, False), (150, 12, True)])
def test_tandem(oracle, unit_len, copies, drift):
    rng = np.random.default_rng(4)
    genes, marks = rr.tandem(rng, unit_len, copies, drift)
    assert len(genes) == 1 and len(genes[0]) == 120 + unit_len * copies + 150 and len(marks) == copies
    g = genes[0]
    if not drift:
        assert all(bytes(g[m["start"]:m["end"]]) == bytes(g[marks[0]["start"]:marks[0]["end"]]) for m in marks)
    else:
        d = [int((g[a["start"]:a["end"]] != g[b["start"]:b["end"]]).sum()) for a, b in zip(marks, marks[1:])]
        assert d == [1] * (copies - 1)
    o = _index(oracle, genes)
    # the tandem gene's k-mer count: every k-mer window, less the windows that repeat an earlier one
    assert o.num_kmer() == len(_canon_kmers(g)) == len(o.index_kmer())
    if not drift:
        # exact copies: a window that lies inside the array and starts a period or more behind its first base repeats the window one
        # period earlier -- unit_len * (copies - 1) - k + 1 of them; every other window is a k-mer of its own
        assert o.num_kmer() == (len(g) - K + 1) - (unit_len * (copies - 1) - K + 1)
    o.close()


def test_saturated_neighbourhood(oracle):
    rng = np.random.default_rng(5)
    m, h = rr.smallest_hash_wmer(15)
    assert rr.wmer_hash(m) == h < 64
    genes, marks = rr.saturated_neighbourhood(rng, K, 15)
    assert len(genes) == 3 and len(marks) == 48
    kms = set()
    for x in marks:
        km = genes[x["gene"]][x["start"]:x["end"]]
        assert bytes(m) in bytes(km)
        # the fixed w-mer is the minimiser of every one of them: no other w-mer of the k-mer hashes lower
        assert min(rr.wmer_hash(km[i:i + 15]) for i in range(3)) == h
        kms.add(min(bytes(km), rc.revcomp(bytes(km))))
    assert len(kms) == 48                              # 48 keys for one line of 16 slots
    o = _index(oracle, genes)
    assert o.num_kmer() == len(set().union(*[_canon_kmers(g) for g in genes]))
    o.close()


@pytest.mark.parametrize("n_genes", [300, 5000])
def test_shared_motif(oracle, n_genes):
    rng = np.random.default_rng(6)
    genes, marks = rr.shared_motif(rng, n_genes)
    assert len(genes) == n_genes and all(len(g) == 100 for g in genes)
    o = _index(oracle, genes)
    lens = np.array([len(x) for x in _lists(o)])
    assert lens.max() == n_genes and (lens == n_genes).sum() == 40 - K + 1
    motif = genes[0][30:70]
    b = synth.batch_from_lists([bytes(motif), bytes(genes[7][:80])])
    goff, gids = o.classify(b["seq1"], b["off1"])
    assert list(gids[:goff[1]]) == list(range(n_genes))      # every gene ties on the motif, ascending
    assert list(gids[goff[1]:]) == [7]
    o.close()


def test_read_sweeps():
    rng = np.random.default_rng(7)
    genes, marks = rr.tandem(rng, 60, 5, False)
    L = 50
    m = marks[2]
    sw = rr.sweep(genes, 0, m["start"], L)
    assert len(sw) == L                                # every offset b - L + 1 ... b
    for i, (a, b) in enumerate(sw):
        s = m["start"] - L + 1 + i
        frag = genes[0][s:s + L + 40]
        if s & 1:
            frag = synth.revcomp(frag)
        assert bytes(a) == bytes(frag[:L]) and bytes(b) == bytes(synth.revcomp(frag)[:L])
    ins = rr.inside(genes, 0, m["start"], m["end"], L)
    assert len(ins) == 60 - L + 1 and all(len(a) == L for a, _ in ins)
    assert bytes(rr.pure(6)[2][0]) == b"ACACAC"
    tails = rr.polya_tail(rng, 80)
    assert [bytes(a).endswith(b"A" * t) for (a, _), t in zip(tails, (10, 20, 30, 40, 50, 60))] == [True] * 6
    rag = rr.batch(sw, ragged_rng=rng)
    l1 = np.diff(rag["off1"].astype(np.int64))
    assert l1.min() >= L // 2 and l1.max() <= L and len(set(l1)) > 1
    uni = rr.batch(rr.pad_uniform(sw, L, rng))
    assert set(np.diff(uni["off1"].astype(np.int64))) == {L} == set(np.diff(uni["off2"].astype(np.int64)))


# ---------------------------------------------------------------------------
# the reference program's recorded answers on one case per builder (tests/golden/gen_ref_repeat_cases.py)
# ---------------------------------------------------------------------------
REPEAT_NPZ = os.path.join(rc.GOLD, "ref_repeat_cases.npz")
REPEAT_CASES = rc.load(REPEAT_NPZ)


def test_recording_is_what_the_generator_builds():
    """the stored inputs are today's builders' output (a generator that drifts from its recording fails here), and the recorded
    answers hold the ties the cases are for"""
    assert [cs["name"] for cs in REPEAT_CASES] == list(rr.BUILDER_CASES)
    for cs in REPEAT_CASES:
        fresh = rr.program_case(cs["name"])
        assert all(fresh[key] == cs[key] for key in fresh), cs["name"]
    widest = {cs["name"]: max(len(a) for a in rc.associations(cs)) for cs in REPEAT_CASES}
    assert widest["shared_motif"] == 300 and widest["interspersed"] >= 25 and widest["low_complexity"] >= 11 and widest["families"] >= 3, widest
    assert os.path.getsize(REPEAT_NPZ) < os.path.getsize(rc.CASES_NPZ)


@pytest.mark.parametrize("cs", REPEAT_CASES, ids=[cs["name"] for cs in REPEAT_CASES])
def test_oracle_reproduces_recorded_repeat_case(oracle, cs, tmp_path):
    """oracle_cli byte for byte, and the batch API the GPU tests compare against read by read"""
    assert rc.run_case(oracle.CLI_PATH, cs, str(tmp_path), bits_flag="--bf-bits") == (cs["ssv"], cs["out1"], cs["out2"])
    o = oracle.Shark(k=cs["k"], c=float(cs["c"]), bf_bits=cs["bf_bits"], min_quality=cs["q"], single=cs["single"])
    o.build([s for _, s in rc.parse_fasta(cs["fasta"])])
    b = rc.batch(cs)
    goff, gids = o.classify(b["seq1"], b["off1"], b["seq2"], b["off2"], b["qual1"], b["qual2"], nthreads=2)
    o.close()
    assert [list(map(int, gids[goff[i]:goff[i + 1]])) for i in range(len(goff) - 1)] == rc.associations(cs)
