"""End extension and aligned pileup without a GPU: the model (tests/extend_model.py) on records worked out by hand, its two scorers
against each other, the tiling claim, the example's figures, and the boundary (header, binding, library symbols, the text form of
extended records)."""
import os
import re

import numpy as np

from shark_amd import capi
from tests import synth
from tests.align_model import cigar, mate_alignment, sam_lines, to_record, verify_sam_line
from tests.extend_cases import example_alignments, tiling_case
from tests.extend_model import best_extension, expected_aligned_pileup, expected_alignments_extended, mate_alignment_extended, naive_extension
from tests.pileup_model import expected_pileup
from tests.segments_model import SegmentsModel, expected_segments
from tests.test_align_cpu import EMPTY, _lib_cigar, _other, _raw_mates, _rc, _record, _row0
from tests.variants_model import expected_variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "shark_amd", "libsharkhip.so")
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example")
K = 5


def _sub(seq, *at):
    s = bytearray(seq)
    for i in at:
        s[i:i + 1] = _other(s[i:i + 1])
    return bytes(s)


# ---------------------------------------------------------------------------
# the scorer by hand
# ---------------------------------------------------------------------------
def test_the_scorer_on_strings_worked_out_by_hand():
    # an isolated mismatch next to the block, the rest matching to the mate's end: h - 1 - P + B > 0 decides
    assert best_extension("X===", True, 4, 5) == 4            # 3 - 4 + 5 = 4
    assert best_extension("X===", True, 4, 0) == 0            # 3 - 4 = -1
    assert best_extension("X====", True, 4, 0) == 0           # 4 - 4 = 0: a tie with e = 0 goes to the smallest e
    assert best_extension("X=====", True, 4, 0) == 6          # 5 - 4 = 1
    assert best_extension("X", True, 4, 5) == 1 and best_extension("X", True, 5, 5) == 0 and best_extension("X", False, 4, 5) == 0
    # at distance d: the whole overhang must beat its first d bases
    assert best_extension("==X==", True, 4, 5) == 5           # 4 - 4 + 5 = 5 > 2
    assert best_extension("==X==", True, 4, 0) == 2           # 0 < 2
    assert best_extension("==X==", False, 4, 5) == 2          # the record ends, not the mate: no bonus
    # two mismatches: the near one is extended through, the far one cuts (and the other way round with a bonus that carries both)
    assert best_extension("=X" + "=" * 10 + "X=", True, 4, 0) == 12
    assert best_extension("=X" + "=" * 10 + "X=", True, 4, 5) == 14
    assert best_extension("=X=X" + "=" * 3, True, 1, 0) == 7 and best_extension("=X=X" + "=" * 3, True, 15, 0) == 1
    # neithers score nothing: trailing ones are not taken unless the bonus carries the extension to the end
    assert best_extension("==..", True, 4, 0) == 2 and best_extension("==..", True, 4, 1) == 4 and best_extension("==..", False, 4, 1) == 2
    assert best_extension("....", True, 4, 0) == 0 and best_extension("....", True, 4, 1) == 4
    assert best_extension(".=", True, 4, 0) == 2
    # unrelated sequence keeps its matching prefix
    assert best_extension("===XXX=X", False, 4, 5) == 3
    assert best_extension("", True, 4, 5) == 0


def test_the_two_scorers_agree_on_random_overhangs():
    rng = np.random.default_rng(7)
    n = 0
    for _ in range(3000):
        H = int(rng.integers(0, 140))
        p_match = float(rng.choice([0.25, 0.7, 0.9, 0.97]))
        u = rng.random(H)
        kinds = "".join("=" if v < p_match else ("." if v > 0.98 else "X") for v in u)
        P, B, to_end = int(rng.integers(1, 16)), int(rng.integers(0, 16)), bool(rng.integers(0, 2))
        e = best_extension(kinds, to_end, P, B)
        assert e == naive_extension(kinds, to_end, P, B), (kinds, to_end, P, B)
        n += 0 < e < H
    assert n > 300


# ---------------------------------------------------------------------------
# records by hand
# ---------------------------------------------------------------------------
def test_one_block_both_ends_on_both_strands():
    """record of 200; the mate is record[50:110] with bases 2 and 57 substituted; windows of 5 vote over [3, 57): block {53, 3, 54}"""
    rec = _record(11, 200)
    mate = _sub(rec[50:110], 2, 57)
    rows = [_row0(50, 3, 57), EMPTY, EMPTY, EMPTY]
    assert mate_alignment(mate, rows, K, 1, rec) == (1, 0, 54, 0, [(53, 3, 54)])
    assert mate_alignment_extended(mate, rows, K, 1, rec, 0, 5) == (1, 0, 54, 0, [(53, 3, 54)])
    # left overhang X== (h = 3), right X== (h = 3): 2 - 4 + 5 = 3 > 0 both
    st = {}
    al = mate_alignment_extended(mate, rows, K, 1, rec, 4, 5, st)
    assert al == (1, 0, 58, 2, [(50, 0, 60)]) and st == {"left": 1, "right": 1, "gained": 1, "bases": 6}
    assert cigar(to_record(al), 60) == ("60M", 2)
    # without a bonus neither end pays: 2 - 4 < 0
    assert mate_alignment_extended(mate, rows, K, 1, rec, 4, 0) == (1, 0, 54, 0, [(53, 3, 54)])
    assert mate_alignment_extended(mate, rows, K, 1, rec, 1, 0) == (1, 0, 58, 2, [(50, 0, 60)])
    assert mate_alignment_extended(mate, rows, K, 1, rec, 2, 0) == (1, 0, 54, 0, [(53, 3, 54)])      # 2 - 2 = 0: the tie stays at e = 0
    # strand 1: the reverse complement with the rows turned gives the same record
    rows1 = [(1, 50, rows[0][2], 60 - K - rows[0][4], 60 - K - rows[0][3]), EMPTY, EMPTY, EMPTY]
    assert mate_alignment_extended(_rc(mate), rows1, K, 1, rec, 4, 5) == (1, 1, 58, 2, [(50, 0, 60)])


def test_the_record_ends_cut_the_overhang_and_earn_no_bonus():
    rec = _record(12, 100)
    # the mate hangs 4 bases over the record's first base and 3 over its last: its bases 4 .. 4 + 100 are the record
    mate = b"ACGT" + rec + b"TTT"
    rows = [_row0(-4, 10, 90), EMPTY, EMPTY, EMPTY]
    assert mate_alignment(mate, rows, K, 1, rec) == (1, 0, 80, 0, [(6, 10, 80)])
    al = mate_alignment_extended(mate, rows, K, 1, rec, 4, 5)
    assert al == (1, 0, 100, 0, [(0, 4, 100)]) and cigar(to_record(al), 107) == ("4S100M3S", 0)
    # a substitution at the record's first base: X at the end of the left overhang, no bonus behind it: the clip grows by one
    al = mate_alignment_extended(_sub(mate, 4), rows, K, 1, rec, 4, 15)
    assert al == (1, 0, 99, 0, [(1, 5, 99)]) and cigar(to_record(al), 107) == ("5S99M3S", 0)


def test_a_junction_overhang_keeps_its_matching_prefix():
    """exon1 + intron + exon2; the mate is the last 40 bases of exon 1 and 10 bases of exon 2: only the first diagonal votes"""
    rng = np.random.default_rng(13)
    e1, e2 = bytes(synth.random_seq(rng, 60)), bytes(synth.random_seq(rng, 60))
    for same, want in ((0, 0), (3, 3)):
        intron = bytearray(synth.random_seq(rng, 50))
        for t in range(4):
            intron[t:t + 1] = e2[t:t + 1] if t < same else _other(e2[t:t + 1])
        rec = e1 + bytes(intron) + e2
        mate = e1[20:] + e2[:10]
        rows = [_row0(20, 0, 40), EMPTY, EMPTY, EMPTY]
        al = mate_alignment_extended(mate, rows, K, 1, rec, 4, 5)
        assert al == (1, 0, 40 + want, 0, [(20, 0, 40 + want)]), (same, al)


def test_two_blocks_only_the_outer_ends_move():
    rec = _record(14, 300)
    mate = _sub(rec[10:50] + rec[200:240], 1, 78)
    rows = [_row0(10, 2, 40), _row0(160, 40, 77), EMPTY, EMPTY]
    before = mate_alignment(mate, rows, K, 1, rec)
    assert before == (2, 0, 75, 0, [(12, 2, 38), (200, 40, 37)])
    al = mate_alignment_extended(mate, rows, K, 1, rec, 4, 5)
    assert al == (2, 0, 78, 2, [(10, 0, 40), (200, 40, 40)]) and cigar(to_record(al), 80) == ("40M150N40M", 2)


def test_non_bases_and_masked_bytes_are_neither():
    rec = _record(15, 120)
    mate = bytearray(rec[30:90])
    mate[1:2] = b"N"
    mate[58:60] = b"NN"
    rows = [_row0(30, 3, 57), EMPTY, EMPTY, EMPTY]
    # left: = N = : all taken (2 matches, then the bonus); right: = N N: one match, the trailing neithers only with a bonus
    assert mate_alignment_extended(bytes(mate), rows, K, 1, rec, 4, 0) == (1, 0, 57, 0, [(30, 0, 58)])
    assert mate_alignment_extended(bytes(mate), rows, K, 1, rec, 4, 1) == (1, 0, 57, 0, [(30, 0, 60)])
    # a record non-base: the same
    rec2 = bytearray(rec)
    rec2[31:32] = b"N"
    assert mate_alignment_extended(bytes(rec[30:90]), rows, K, 1, bytes(rec2), 4, 0) == (1, 0, 59, 0, [(30, 0, 60)])


def test_extended_records_keep_their_text_form(oracle):
    """random mates over spliced genes with substitutions: shk_alignment_cigar accepts every extended record, gives the model's text,
    and every line passes the verifier"""
    from tests.spliced_synth import spliced_gene, spliced_reads
    rng = np.random.default_rng(80)
    genes = [spliced_gene(rng, 1 + i, 17) for i in range(3)]
    records = [bytes(g) for g, _ in genes]
    sm = SegmentsModel(records, 17)
    o = oracle.Shark(k=17, c=0.0, bf_bits=1 << 26)
    nidx = o.build(records)
    batch = spliced_reads(rng, genes, 200, paired=True, sub=0.03)
    goff, gids = o.classify(batch["seq1"], batch["off1"], batch.get("seq2"), batch.get("off2"), None, None)
    rows = expected_segments(sm, batch, goff, gids, 4)[1]
    st = {}
    recs = expected_alignments_extended(sm, batch, goff, gids, rows, 8, 4, 5, stats=st)
    plain = expected_alignments_extended(sm, batch, goff, gids, rows, 8, 0, 0)
    assert st["gained"] >= 20 and recs.tobytes() != plain.tobytes()
    assert (recs["n_blocks"] == plain["n_blocks"]).all() and (recs["block"][..., 2].sum(-1) >= plain["block"][..., 2].sum(-1)).all()
    raw = _raw_mates(batch)
    for i in range(200):
        for j in range(int(goff[i]), int(goff[i + 1])):
            for t in range(2):
                assert _lib_cigar(recs[j, t], len(raw[i][t]), 20) == (0,) + cigar(recs[j, t], len(raw[i][t]), 20)
    legend = ["g%d" % g for g in range(nidx)]
    lines = sam_lines(["r%d" % i for i in range(200)], raw, None, goff, gids, recs, legend, True)
    fasta = {legend[g]: records[g] for g in range(nidx)}
    assert len(lines) > 100 and all(verify_sam_line(ln, fasta) >= 0 for ln in lines)
    # aligned pileup from the records: one observation per base-bearing block base, a mate per record with a block
    counts, mates, bearing = expected_aligned_pileup(sm, batch, goff, gids, recs)
    assert int(counts.sum()) == bearing and mates == int((recs["n_blocks"] > 0).sum())


# ---------------------------------------------------------------------------
# the tiling claim
# ---------------------------------------------------------------------------
def tiling_counts(oracle, P, B, L=100, k=17, s_min=8):
    rec, site, reads = tiling_case(L, k)
    sm = SegmentsModel([rec], k)
    o = oracle.Shark(k=k, c=0.0, bf_bits=1 << 26)
    o.build([rec])
    batch = synth.batch_from_lists([np.frombuffer(r, np.uint8) for r in reads])
    goff, gids = o.classify(batch["seq1"], batch["off1"], None, None, None, None)
    assert int(goff[-1]) == 2 * L
    rows = expected_segments(sm, batch, goff, gids, 4)[1]
    owned = expected_pileup(sm, batch, goff, gids, rows, s_min)[0]
    recs = expected_alignments_extended(sm, batch, goff, gids, rows, s_min, P, B)
    aligned = expected_aligned_pileup(sm, batch, goff, gids, recs)[0]
    return rec, site, owned, aligned


def test_tiling_every_read_offset_shows_both_alleles_only_with_extension(oracle):
    """owned pileup: the record's base from all L mates, the other base from the L - 2k whose substitution has windows on both sides;
    aligned pileup at (4, 5): L against L, and the site is a variant at frac 1/2 only then"""
    rec, site, owned, aligned = tiling_counts(oracle, 4, 5)
    r = b"ACGT".index(rec[site:site + 1])
    a = b"ACGT".index(_other(rec[site:site + 1]))
    assert int(owned[site, r]) == 100 and int(owned[site, a]) == 66 and int(owned[site].sum()) == 166
    assert int(aligned[site, r]) == 100 and int(aligned[site, a]) == 100 and int(aligned[site].sum()) == 200
    prm = (8, 3, 1, 2)
    assert site not in expected_variants(owned, [rec], np.array([0, len(rec)]), prm)["x"].tolist()
    assert expected_variants(aligned, [rec], np.array([0, len(rec)]), prm)["x"].tolist() == [site]
    # aligned pileup without extension is owned pileup on these single-block mates
    _, _, owned0, aligned0 = tiling_counts(oracle, 0, 0)
    assert np.array_equal(owned0, aligned0)


# ---------------------------------------------------------------------------
# the example's figures
# ---------------------------------------------------------------------------
# found with the model (k = 17, c = 0.6, s_min = 8, P = 4, B = 5): of the example's 3 858 aligned mates this many gain at least one base
# on the unmutated record (the sample has no errors: what they gain are clean overhangs of fewer than k bases past a junction's other
# side or at an end the windows left out); on the record with twelve substituted bases, the sites of aligned pileup with extension
# at the command's thresholds (depth 8, alt 3, frac 1/5)
EXAMPLE_MATES_THAT_GAIN = 97
EXAMPLE_MISMATCHES_FROM_THE_BONUS = 54
MUTATED_EXAMPLE_SITES_EXTENDED = [150, 5544, 5600, 5734, 9660, 9700, 12345, 14100]


def test_the_example_figures(oracle):
    from tests.depth_model import model_layout
    from tests.test_variants_cpu import EXAMPLE_SITES, SUBSTITUTED, mutated_example_records
    fa = synth.read_fasta(os.path.join(EXAMPLE, "ENSG00000277117.fa"))
    sm, batch, goff, gids, recs, st = example_alignments(oracle, fa, 4, 5)
    print("example: mates", int((recs["n_blocks"] > 0).sum()), st)
    assert int((recs["n_blocks"] > 0).sum()) == 3858
    assert st["gained"] == EXAMPLE_MATES_THAT_GAIN
    # the sample has no errors, so a mismatch in an extended block is an overhang of a few bases past a junction that the end bonus carried
    # into the intron (h - 1 - P + B > d holds for h = 2 already at P = 4, B = 5): the price of the bonus, on 3 858 mates
    assert int(recs["mismatches"].sum()) == EXAMPLE_MISMATCHES_FROM_THE_BONUS
    fa2 = mutated_example_records()
    sm, batch, goff, gids, recs, st = example_alignments(oracle, fa2, 4, 5)
    counts = expected_aligned_pileup(sm, batch, goff, gids, recs)[0]
    sites = expected_variants(counts, [s for _, s in fa2], model_layout(sm, len(fa2)))["x"].tolist()
    print("mutated example: sites", sites, "depth at the substituted bases", [int(counts[x].sum()) for x in SUBSTITUTED], st)
    assert sites == MUTATED_EXAMPLE_SITES_EXTENDED
    # the seven of owned pileup stay; base 16 gets its 7 mates back, all showing the original base -- one short of the command's depth
    # floor of 8, so it is observed and still not called; 5734 is no substituted base: the bonus's price above, enough of it in one place
    assert [x for x in sites if x in SUBSTITUTED] == [150, 5544, 5600, 9660, 9700, 12345, 14100] and len(sites) - 1 == EXAMPLE_SITES
    assert int(counts[16].sum()) == 7 and int(counts[16].max()) == 7
    assert 16 in expected_variants(counts, [s for _, s in fa2], model_layout(sm, len(fa2)), (7, 3, 1, 5))["x"].tolist()


# ---------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------
NEW = ("shk_alignments_extend", "shk_pileup_enable_aligned")


def test_header_declares_and_library_exports_the_new_calls_with_their_argument_errors():
    text = open(os.path.join(ROOT, "include", "shark_hip.h")).read()
    assert "3a. END EXTENSION" in text and "ALIGNED PILEUP" in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    from shark_amd import EXPORTS, SharkHip
    assert set(NEW) <= set(EXPORTS)
    for name in ("alignments_extend", "pileup_enable_aligned"):
        assert callable(getattr(SharkHip, name))
    assert os.path.exists(LIB), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    lib = capi.load()
    for s in NEW:
        assert hasattr(lib, s), s
    ERR_ARG = -1
    # (no context: an argument error, not a crash; the bounds with a context are the GPU suite's)
    assert lib.shk_alignments_extend(None, 4, 5) == ERR_ARG and lib.shk_pileup_enable_aligned(None, 8) == ERR_ARG


def test_cli_flags():
    import subprocess
    cli = os.path.join(ROOT, "shark_amd", "bin", "shark")
    assert os.path.exists(cli), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    run = lambda *a: subprocess.run([cli, "-r", "x.fa", "-1", "y.fq"] + list(a), capture_output=True, text=True)  # noqa: E731
    r = run("--pileup-aligned")
    assert r.returncode == 1 and "--pileup-aligned needs --pileup FILE or --variants FILE" in r.stderr
    r = run("--extend-ends")
    assert r.returncode == 1 and "--extend-ends needs --sam FILE or --pileup-aligned" in r.stderr
    for flag in ("--extend-penalty", "--extend-bonus"):
        r = run("--sam", "s", flag, "3")
        assert r.returncode == 1 and "need --extend-ends" in r.stderr
    for flag, bad in (("--extend-penalty", "0"), ("--extend-penalty", "16"), ("--extend-bonus", "16")):
        r = run("--sam", "s", "--extend-ends", flag, bad)
        assert r.returncode == 1 and "must be in the range" in r.stderr, (flag, bad, r.stderr)
    r = subprocess.run([cli, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and all(s in r.stderr for s in ("--extend-ends", "--extend-penalty N", "--extend-bonus N", "--pileup-aligned"))
