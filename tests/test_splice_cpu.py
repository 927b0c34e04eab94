"""Spliced ends without a GPU: the model (tests/splice_model.py) on placements worked out by hand, its ranged candidate search against
the naive restatement that tries every site of the gene, the junction-file conversion, the example's figures, and the boundary
(header, binding, library symbols, the command's flag rejections)."""
import os
import re

import numpy as np
import pytest

from shark_amd import capi
from tests import synth
from tests.align_model import cigar, sam_lines, to_record, verify_sam_line
from tests.segments_model import SegmentsModel, expected_segments
from tests.splice_cases import ONE_JUNCTION, cut, example_spliced, junction_gene
from tests.splice_model import (DEFAULTS, check_sites, expected_alignments_spliced, mate_alignment_spliced, naive_candidates, ranged_candidates,
                                sites_from_junction_lines, splice_end)
from tests.test_align_cpu import EMPTY, _other, _raw_mates, _rc, _row0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "shark_amd", "libsharkhip.so")
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example")
K = 5

# the example at the command's defaults (3, 2, 2), sites from its own junction table: mates that gain a block
EXAMPLE_MATES_THAT_GAIN_A_BLOCK = 614


def _sub(seq, *at):
    s = bytearray(seq)
    for i in at:
        s[i:i + 1] = _other(s[i:i + 1])
    return bytes(s)


def _rows_for(pieces, L, strand=0):
    """the rows of a mate cut from one diagonal piece (a, b) placed at read base q: [(a, b, q)] -> segment rows at K"""
    rows = [_row0(a - q, q, q + (b - a)) for a, b, q in pieces]
    if strand:
        rows = [(1, pos, sup, L - K - last, L - K - first) for _, pos, sup, first, last in rows]
    return rows + [EMPTY] * (4 - len(rows))


def _al(mate, rows, rec, sites, params=DEFAULTS, P=0, B=0, stats=None):
    return mate_alignment_spliced(bytes(mate), rows, K, 1, bytes(rec), sorted(sites), params, P, B, stats)


# ---------------------------------------------------------------------------
# placements by hand
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("strand", [0, 1])
def test_one_junction_by_hand_on_both_strands(strand):
    rng = np.random.default_rng(5)
    plain, micro = junction_gene(rng, 0), junction_gene(rng, 3)
    turn = (lambda m: _rc(m)) if strand else (lambda m: bytes(m))
    for name, pieces, want, want_tie in ONE_JUNCTION:
        voting = max(pieces, key=lambda p: p[1] - p[0])
        q = 0 if voting == pieces[0] else pieces[0][1] - pieces[0][0]
        L = sum(b - a for a, b in pieces)
        rows = _rows_for([(voting[0], voting[1], q)], L, strand)
        for s in (plain, micro):
            mate = turn(cut(s, pieces))
            before = _al(mate, rows, s, [])
            assert before[0] == 1 and before[4] == [(voting[0], q, voting[1] - voting[0])]
            st = {}
            al = _al(mate, rows, s, [(80, 140)], stats=st)
            assert al == (2, strand, L, 0, want), (name, al)
            assert st[name + "_placed"] == 1 and st["mates_gained"] == 1
            assert cigar(to_record(al), L)[0] == "%dM60N%dM" % (want[0][2], want[1][2])
            # min_overhang above the overhang of 10, and off
            assert _al(mate, rows, s, [(80, 140)], (11, 2, 2)) == before and _al(mate, rows, s, [(80, 140)], (0, 2, 2)) == before
        # the microhomology of 3: both descriptions of the one placement listed -- they do not compete, the largest donor wins
        st = {}
        al = _al(turn(cut(micro, pieces)), rows, micro, [(80, 140), (83, 143)], stats=st)
        assert al == (2, strand, L, 0, want_tie), (name, al)
        # on the gene without it, (83, 143) alone costs its three bases: too costly at max_cost 2, placed at 3
        mate = turn(cut(plain, pieces))
        assert _al(mate, rows, plain, [(83, 143)], (3, 2, 2))[0] == 1
        assert _al(mate, rows, plain, [(83, 143)], (3, 3, 2))[4] == want_tie


def test_ambiguity_cost_and_the_null_candidate():
    rng = np.random.default_rng(6)
    e1, i1, e2, i2, e3 = (synth.random_seq(rng, n) for n in (60, 40, 40, 40, 60))
    # exon skipping: exon 3 starts with exon 2's first four bases and differs at its fifth and sixth
    e3[:4] = e2[:4]
    e3[4], e3[5] = (ord(_other(bytes([e2[4]]))), ord(_other(bytes([e2[5]]))))
    i1[:6] = [ord(_other(bytes([e2[t]]), bytes([e3[t]]))) for t in range(6)]          # (the null candidate matches nothing)
    s = np.concatenate([e1, i1, e2, i2, e3])
    sites = [(60, 100), (60, 180)]
    rows = _rows_for([(10, 60, 0)], 54)
    # h = 4: both acceptors cost 0: their shifts differ, cost2 - cost = 0 < 2: a clip
    st = {}
    al = _al(cut(s, ((10, 60), (100, 104))), rows, s, sites, stats=st)
    assert al[0] == 1 and st == {"right_attempted": 1, "right_ambiguous": 1}
    # two bases longer the skipping acceptor costs 2: placed on exon 2; min_gap 3 asks for more; min_gap 0 at h = 4 decides by the tie
    # rule (the largest acceptor)
    m6 = cut(s, ((10, 60), (100, 106)))
    rows6 = _rows_for([(10, 60, 0)], 56)
    assert _al(m6, rows6, s, sites)[4] == [(10, 0, 50), (100, 50, 6)]
    assert _al(m6, rows6, s, sites, (3, 2, 3))[0] == 1
    assert _al(cut(s, ((10, 60), (100, 104))), rows, s, sites, (3, 2, 0))[4] == [(10, 0, 50), (180, 50, 4)]
    # substitutions in the overhang: 1 and 2 are placed (cost <= max_cost, the others far worse), 3 is too costly
    base = cut(s, ((10, 60), (100, 120)))
    rows20 = _rows_for([(10, 60, 0)], 70)
    for n, blocks in ((1, 2), (2, 2), (3, 1)):
        st = {}
        al = _al(_sub(bytes(base), *[52 + 3 * t for t in range(n)]), rows20, s, [(60, 100)], stats=st)
        assert al[0] == blocks and al[3] == (n if blocks == 2 else 0), (n, al)
        assert ("right_too_costly" in st) == (blocks == 1)
    # an N in the overhang, and a record N under it, cost like a substitution but count as neither
    with_n = bytearray(base)
    with_n[55:56] = b"N"
    al = _al(bytes(with_n), rows20, s, [(60, 100)])
    assert al[0] == 2 and al[2:4] == (69, 0)
    s_n = s.copy()
    s_n[105] = ord("N")
    al = _al(bytes(base), rows20, s_n, [(60, 100)], (3, 0, 2))
    assert al[0] == 1                                            # (max_cost 0: the record's N is not a match)
    # an intron that begins like the next exon: the null candidate ties, the end stays a clip
    twin = s.copy()
    twin[60:66] = twin[100:106]
    st = {}
    assert _al(m6, rows6, twin, [(60, 100)], stats=st)[0] == 1 and st.get("right_ambiguous") == 1
    assert _al(m6, rows6, twin, [(60, 100)], (3, 2, 0))[0] == 2


def test_bounds_of_the_overhang_the_candidate_range_and_the_record():
    rng = np.random.default_rng(8)
    s = junction_gene(rng, 0, 120, 60, 120)                     # exon [0, 120), intron [120, 180), exon [180, 300)
    for h, placed in ((1, False), (2, False), (3, True), (48, True), (49, False)):
        mate = cut(s, ((60, 120), (180, 180 + h)))
        al = _al(mate, _rows_for([(60, 120, 0)], 60 + h), s, [(120, 180)], (3, 2, 2) if h != 1 else (2, 2, 2))
        assert (al[0] == 2) == placed, (h, al)
        if placed:
            assert al[4] == [(60, 0, 60), (180, 60, h)]
    assert _al(cut(s, ((60, 120), (180, 181))), _rows_for([(60, 120, 0)], 61), s, [(120, 180)], (1, 0, 1))[0] == 2
    # the donor's range [xe - B, xe + h - 1] around a block that ends at xe = 110 short of the junction, h = 20 (B = 16)
    mate = cut(s, ((60, 120), (180, 190)))                       # the block is given as [60, 110): 10 of its bases and 10 past the junction wait
    rows = _rows_for([(60, 110, 0)], 70)
    assert _al(mate, rows, s, [(120, 180)])[4] == [(60, 0, 60), (180, 60, 10)]      # (the block grows by d - xe = 10)
    for d, a, cand in ((94, 154, True), (93, 153, False), (129, 189, True), (130, 190, False)):
        assert ((d, a) in ranged_candidates("right", [(d, a)], 60, 0, 50, 70, 300)) == cand, (d, a)
    # a block of 10 bases: B = 9
    assert ranged_candidates("right", [(50, 100), (51, 100)], 50, 0, 10, 30, 300) == [(51, 100)]
    # the far side ends exactly at len_g, and one base past it
    assert ranged_candidates("right", [(120, 280)], 60, 0, 60, 80, 300) == [(120, 280)]
    assert ranged_candidates("right", [(120, 281)], 60, 0, 60, 80, 300) == []
    # the left end's mirror: a in [x0 - h + 1, x0 + B], the new block inside the record
    for d, a, cand in ((100, 161, True), (100, 160, False), (100, 196, True), (100, 197, False)):
        assert ((d, a) in ranged_candidates("left", [(d, a)], 180, 20, 60, 80, 300)) == cand, (d, a)
    assert ranged_candidates("left", [(20, 180)], 180, 20, 60, 80, 300) == [(20, 180)]
    assert ranged_candidates("left", [(19, 180)], 180, 20, 60, 80, 300) == []


def test_the_block_budget():
    rng = np.random.default_rng(9)
    ex = [synth.random_seq(rng, n) for n in (80, 40, 80, 60, 60)]
    introns = [synth.random_seq(rng, 50) for _ in range(4)]
    s = np.concatenate([ex[0], introns[0], ex[1], introns[1], ex[2], introns[2], ex[3], introns[3], ex[4]])
    # exons at [0, 80), [130, 170), [220, 300), [350, 410), [460, 520)
    sites = [(80, 130), (170, 220), (300, 350), (410, 460)]
    # 10 bases of exon 1, the whole exon 2, 10 of exon 3: one block becomes three
    mate = cut(s, ((70, 80), (130, 170), (220, 230)))
    st = {}
    al = _al(mate, _rows_for([(130, 170, 10)], 60), s, sites, stats=st)
    assert al[4] == [(70, 0, 10), (130, 10, 40), (220, 50, 10)] and st["left_placed"] == st["right_placed"] == 1
    # three blocks and two placeable ends: only the left is placed
    mate = cut(s, ((70, 80), (130, 170), (220, 300), (350, 410), (460, 470)))
    rows = _rows_for([(130, 170, 10), (220, 300, 50), (350, 410, 130)], 200)
    al = _al(mate, rows, s, sites)
    assert al[0] == 4 and al[4][0] == (70, 0, 10) and al[4][-1] == (350, 130, 60)
    # four blocks: untouched
    mate = cut(s, ((70, 80), (130, 170), (220, 300), (350, 410), (460, 520)))
    rows = _rows_for([(130, 170, 10), (220, 300, 50), (350, 410, 130), (460, 520, 190)], 250)
    assert _al(mate, rows, s, sites) == _al(mate, rows, s, [])


def test_then_step_3a_extends_only_the_unplaced_end():
    rng = np.random.default_rng(10)
    s = junction_gene(rng, 0)
    mate = bytearray(cut(s, ((20, 80), (140, 150))))
    mate[2:3] = _other(mate[2:3])                                # a substitution near the left end: the block starts at read base 3
    rows = _rows_for([(23, 80, 3)], 70)
    assert _al(bytes(mate), rows, s, [(80, 140)])[4] == [(23, 3, 57), (140, 60, 10)]
    al = _al(bytes(mate), rows, s, [(80, 140)], DEFAULTS, 4, 5)
    assert al == (2, 0, 69, 1, [(20, 0, 60), (140, 60, 10)])


def test_the_left_end_is_priced_on_block_0_as_gap_closure_left_it():
    """exon A [0, 40), exon 1 [80, 92), exon 2 [140, 200); the mate is s[35:40] + s[80:92], two bases that fit neither side, s[142:180].
    Closure gives both to block 0 (every split costs 2: the largest s), so step 3b sees {80, 5, 14}: B = 13, the two bases are
    evaluated and are not a match -- at max_cost 0 the end stays a clip, though the 12-base span alone would have cost nothing"""
    rng = np.random.default_rng(12)
    s = bytearray(synth.random_seq(rng, 200))
    for t in range(4):
        s[79 - t:80 - t] = _other(s[39 - t:40 - t])
    gap = b"".join(_other(s[92 + t:93 + t], s[140 + t:141 + t]) for t in range(2))
    s = bytes(s)
    mate = s[35:40] + s[80:92] + gap + s[142:180]
    rows = _rows_for([(80, 92, 5), (142, 180, 19)], len(mate))
    plain = _al(mate, rows, s, [])
    assert plain[4] == [(80, 5, 14), (142, 19, 38)]
    st = {}
    assert _al(mate, rows, s, [(40, 80)], (3, 0, 1), stats=st) == plain and st == {"left_attempted": 1, "left_too_costly": 1}
    assert _al(mate, rows, s, [(40, 80)], (3, 2, 2))[4] == [(35, 0, 5), (80, 5, 14), (142, 19, 38)]
    assert ranged_candidates("left", [(53, 93)], 80, 5, 14, len(mate), 200) == [(53, 93)]
    assert ranged_candidates("left", [(54, 94)], 80, 5, 14, len(mate), 200) == []


# ---------------------------------------------------------------------------
# the ranged search against the naive restatement
# ---------------------------------------------------------------------------
def test_the_ranged_search_is_the_naive_restatement_on_random_ends():
    rng = np.random.default_rng(11)
    placed = 0
    for _ in range(600):
        len_g = int(rng.integers(120, 400))
        rec = synth.random_seq(rng, len_g)
        L = int(rng.integers(30, 120))
        ln = int(rng.integers(1, L))
        q = int(rng.integers(0, L - ln + 1))
        x = int(rng.integers(q, max(q + 1, len_g - (L - q))))
        n = int(rng.integers(0, 40))
        sites = set()
        for _ in range(n):
            d = int(rng.integers(1, len_g - 2))
            sites.add((d, int(rng.integers(d + 1, len_g))))
        sites = sorted(sites)
        for side in ("left", "right"):
            a = ranged_candidates(side, sites, x, q, ln, L, len_g)
            b = naive_candidates(side, sites, x, q, ln, L, len_g)
            assert a == b, (side, x, q, ln, L, len_g, sites)
            placed += bool(a)
    assert placed > 100


def test_the_model_with_either_search_on_synthetic_spliced_batches(oracle):
    from tests.spliced_model import expected_junction_table, table_rows
    from tests.spliced_synth import spliced_gene, spliced_reads
    rng = np.random.default_rng(81)
    genes = [spliced_gene(rng, 1 + i, 17) for i in range(3)]
    records = [bytes(g) for g, _ in genes]
    sm = SegmentsModel(records, 17)
    o = oracle.Shark(k=17, c=0.0, bf_bits=1 << 26)
    nidx = o.build(records)
    batch = spliced_reads(rng, genes, 300, paired=True, sub=0.01)
    goff, gids = o.classify(batch["seq1"], batch["off1"], batch.get("seq2"), batch.get("off2"), None, None)
    rows = expected_segments(sm, batch, goff, gids, 4)[1]
    table = expected_junction_table(batch, goff, gids, rows, 17, 8)
    sites = check_sites(sorted({(g, d, d + i) for g, d, a, i, n in table_rows(table)}), [len(r) for r in records])
    assert len(sites) >= 3
    st, st2 = {}, {}
    recs = expected_alignments_spliced(sm, batch, goff, gids, rows, 8, sites, DEFAULTS, 4, 5, stats=st)
    naive = expected_alignments_spliced(sm, batch, goff, gids, rows, 8, sites, DEFAULTS, 4, 5, stats=st2, candidates=naive_candidates)
    assert recs.tobytes() == naive.tobytes() and st == st2
    plain = expected_alignments_spliced(sm, batch, goff, gids, rows, 8, sites, (0, 0, 0), 4, 5)
    assert st["mates_gained"] >= 10 and st.get("left_placed", 0) >= 3 and st.get("right_placed", 0) >= 3, st
    assert (recs["n_blocks"] >= plain["n_blocks"]).all() and int((recs["n_blocks"] > plain["n_blocks"]).sum()) == st["mates_gained"]
    raw = _raw_mates(batch)
    legend = ["g%d" % g for g in range(nidx)]
    lines = sam_lines(["r%d" % i for i in range(300)], raw, None, goff, gids, recs, legend, True)
    fasta = {legend[g]: records[g] for g in range(nidx)}
    assert len(lines) > 100 and all(verify_sam_line(ln, fasta) >= 0 for ln in lines)


# ---------------------------------------------------------------------------
# the command's conversion
# ---------------------------------------------------------------------------
def test_junction_lines_become_sites():
    legend, lengths = ["gA", "gB"], [300, 200]
    lines = ["gB 50 98 50 3", "gA 80 137 60 1", "gA 80 140 60 7", "", "gA 20 60 40"]
    # (donor, donor + intron), not the acceptor column; duplicates after the conversion merge; sorted by (gene, donor, acceptor)
    assert sites_from_junction_lines(lines, legend, lengths) == [(0, 20, 60), (0, 80, 140), (1, 50, 100)]
    assert sites_from_junction_lines(lines, legend, lengths, 2) == [(0, 80, 140), (1, 50, 100)]
    assert sites_from_junction_lines(lines, legend, lengths, 8) == []
    for bad, what in (("gC 1 2 3 4", "line 2: unknown gene"), ("gA 1 2", "line 2: malformed"), ("gA 1 x 3 4", "line 2: malformed"), ("gA +1 2 3 4", "line 2: malformed"),
                      ("gA 1_0 20 3 4", "line 2: malformed"), ("gA 1 2 3 -4", "line 2: malformed"), ("gA 1 2 3 12345678901", "line 2: malformed"), ("gA 1 2 3 4 5", "line 2: malformed"),
                      ("gA 0 5 5 1", "line 2: the site lies outside"), ("gA 250 299 50 1", "line 2: the site lies outside"), ("gA 5 5 0 1", "line 2: the site lies outside")):
        with pytest.raises(ValueError, match=what):
            sites_from_junction_lines(["gA 80 140 60 7", bad], legend, lengths)
    assert sites_from_junction_lines(["gA 249 299 50 1"], legend, lengths) == [(0, 249, 299)]
    with pytest.raises(ValueError):
        check_sites([(0, 80, 140), (0, 80, 140)], lengths)
    with pytest.raises(ValueError):
        check_sites([(0, 80, 300)], lengths)


# ---------------------------------------------------------------------------
# the example
# ---------------------------------------------------------------------------
def test_the_example_figures(oracle):
    fa = synth.read_fasta(os.path.join(EXAMPLE, "ENSG00000277117.fa"))
    sm, batch, goff, gids, lines, sites, plain, recs, st = example_spliced(oracle, fa)
    gained = int((recs["n_blocks"] > plain["n_blocks"]).sum())
    print("example: junction lines", len(lines), "sites", len(sites), "mates with a block", int((recs["n_blocks"] > 0).sum()), "gain a block", gained, st)
    assert len(sites) > 0 and gained > 0 and gained == st["mates_gained"]
    assert gained == EXAMPLE_MATES_THAT_GAIN_A_BLOCK
    # the sample has no errors: every placed base agrees with the record
    assert int(recs["mismatches"].sum()) == int(plain["mismatches"].sum()) and int(recs["matches"].sum()) > int(plain["matches"].sum())
    legend = [n.decode() for n, _ in fa]
    fasta = {legend[g]: bytes(sm.records.get(g, b"")) for g in range(len(fa))}
    r1 = synth.read_fastq(os.path.join(EXAMPLE, "sample_1.fq"))
    ids = [i.decode() if isinstance(i, bytes) else str(i) for i, _, _ in r1]
    out = sam_lines(ids, _raw_mates(batch), None, goff, gids, recs, legend, True)
    assert len(out) == int((recs["n_blocks"] > 0).sum()) and all(verify_sam_line(ln, fasta) == 0 for ln in out)


# ---------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------
NEW = ("shk_splice_sites_set", "shk_alignments_splice")


def test_header_declares_and_library_exports_the_new_calls_with_their_argument_errors():
    text = open(os.path.join(ROOT, "include", "shark_hip.h")).read()
    assert "3b. SPLICED ENDS" in text and "SHK_SPLICE_MAX_OVERHANG 48" in text and "SHK_SPLICE_BACK         16" in text
    for phrase in ("an overhang that itself holds a second junction", "sites learned within the run", "a mate with no block"):
        assert phrase in text, phrase
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    assert re.search(r"typedef struct shk_splice_site \{ uint32_t gene, donor, acceptor; \} shk_splice_site;", hdr)
    from shark_amd import EXPORTS, SharkHip
    assert set(NEW) <= set(EXPORTS) and capi.SPLICE_SITE_DTYPE.itemsize == 12
    assert (capi.SHK_SPLICE_MAX_OVERHANG, capi.SHK_SPLICE_BACK) == (48, 16)
    for name in ("splice_sites_set", "alignments_splice"):
        assert callable(getattr(SharkHip, name))
    assert os.path.exists(LIB), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    lib = capi.load()
    for s in NEW:
        assert hasattr(lib, s), s
    ERR_ARG = -1
    assert lib.shk_splice_sites_set(None, None, 0) == ERR_ARG and lib.shk_alignments_splice(None, 3, 2, 2) == ERR_ARG


def test_cli_flags():
    import subprocess
    cli = os.path.join(ROOT, "shark_amd", "bin", "shark")
    assert os.path.exists(cli), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    run = lambda *a: subprocess.run([cli, "-r", "x.fa", "-1", "y.fq"] + list(a), capture_output=True, text=True)  # noqa: E731
    r = run("--splice-junctions", "j")
    assert r.returncode == 1 and "--splice-junctions needs --sam FILE or --pileup-aligned" in r.stderr
    for flag in ("--splice-min-mates", "--splice-min-overhang", "--splice-max-cost", "--splice-min-gap"):
        r = run("--sam", "s", flag, "3")
        assert r.returncode == 1 and "need --splice-junctions FILE" in r.stderr, (flag, r.stderr)
    for flag, bad in (("--splice-min-overhang", "0"), ("--splice-min-overhang", "49"), ("--splice-max-cost", "65"), ("--splice-min-gap", "65")):
        r = run("--sam", "s", "--splice-junctions", "j", flag, bad)
        assert r.returncode == 1 and "must be" in r.stderr, (flag, bad, r.stderr)
    r = subprocess.run([cli, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and all(s in r.stderr for s in ("--splice-junctions FILE", "--splice-min-mates N", "--splice-min-overhang N", "--splice-max-cost N",
                                                             "--splice-min-gap N"))
