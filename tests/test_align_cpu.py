"""Alignments mode without a GPU: the model (tests/align_model.py) on mates worked out by hand, rule by rule; shk_alignment_cigar -- a
pure host function of the library -- through ctypes against the model's letter-by-letter walk; a verifier that needs nothing but a
SAM line and the FASTA over the model's lines; the model's figures on the bundled example and on its mutated record; and the
boundary -- the new symbols in the header, the binding and the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from shark_amd import capi
from tests import synth
from tests.align_model import (cigar, expected_alignments, mate_alignment, sam_header, sam_lines, sam_seq, to_record, verify_sam_line)
from tests.segments_model import SegmentsModel, expected_segments
from tests.spliced_synth import spliced_gene, spliced_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "shark_amd", "libsharkhip.so")
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example")
K = 5
EMPTY = (0, 0, 0, 0, 0)


def _rc(b):
    return bytes(synth.revcomp(np.frombuffer(bytes(b), np.uint8)))


def _other(base, *more):
    """a base that differs from every given one"""
    return next(bytes([c]) for c in b"ACGT" if bytes([c]) not in [bytes(base[:1]).upper()] + [bytes(m[:1]).upper() for m in more])


def _record(seed, n):
    return bytes(synth.random_seq(np.random.default_rng(seed), n))


def _row0(pos, q_lo, q_hi, k=K):
    """the strand 0 segment whose span is the read bases [q_lo, q_hi) on diagonal pos: record [pos + q_lo, pos + q_hi)"""
    return (0, pos, q_hi - k - q_lo + 1, q_lo, q_hi - k)


def _both_strands(mate, rows, L, record, s_min=1, k=K):
    """the alignment of the mate by strand 0 rows, checked to be the same from the reverse-complemented mate with the rows turned
    onto strand 1 (first and last mirror: slot p of the mate is slot L - k - p of its reverse complement)"""
    fwd = mate_alignment(bytes(mate), rows, k, s_min, record)
    rows1 = [(1, pos, sup, L - k - last, L - k - first) if sup else EMPTY for _, pos, sup, first, last in rows]
    rev = mate_alignment(_rc(mate), rows1, k, s_min, record)
    assert rev[0] == fwd[0] and rev[2:] == fwd[2:] and (rev[1] == 1 or rev[0] == 0)
    return fwd


# ---------------------------------------------------------------------------
# the model on mates worked out by hand, rule by rule
# ---------------------------------------------------------------------------
def test_the_worked_example_of_the_header():
    """L = 100, k = 17, strand 1, spans [9653, 9727) at pos 9653 and [10912, 10943) at pos 10843: blocks {9653, 0, 74} and, trimmed by
    the overlap of 5, {10917, 74, 26}; nothing clipped, 1190 record bases between them"""
    rec = _record(5, 20000)
    rows = [(1, 9653, 58, 26, 83), (1, 10843, 15, 0, 14), EMPTY, EMPTY]
    assert [sp[:2] for sp in capi.kept_spans(rows, 100, 17, 8)] == [(9653, 9727), (10912, 10943)]
    mate = _rc(rec[9653:9727] + rec[10917:10943])                # the read the two blocks spell, as the sequencer gave it
    stats = {}
    al = mate_alignment(mate, rows, 17, 8, rec, stats)
    assert al == (2, 1, 100, 0, [(9653, 0, 74), (10917, 74, 26)]) and stats == {"trimmed": 1}
    assert cigar(to_record(al), 100, 20) == ("74M1190N26M", 0) and cigar(to_record(al), 100, 1190) == ("74M1190N26M", 0)
    assert cigar(to_record(al), 100, 1191) == ("74M1190D26M", 1190)
    # a floor above the second diagonal's support keeps the first block alone: the rest of the mate is clipped
    al = mate_alignment(mate, rows, 17, 16, rec)
    assert al == (1, 1, 74, 0, [(9653, 0, 74)]) and cigar(to_record(al), 100) == ("74M26S", 0)
    # and above the first one's nothing is left
    assert mate_alignment(mate, rows, 17, 59, rec) == (0, 0, 0, 0, [])
    assert cigar(to_record(mate_alignment(mate, rows, 17, 59, rec)), 100) == ("*", 0)


def test_trimming_that_empties_a_block_and_a_block_out_of_read_order():
    rec = _record(1, 200)
    mate = bytearray(rec[0:50] + rec[80:110])                                     # read [0, 50) on pos 0, [50, 80) on pos 30
    a, c = _row0(0, 0, 50), _row0(30, 50, 80)
    # read bases [40, 50) once more on diagonal 20 (record [60, 70)): all of them are taken, the piece yields nothing
    emptied = _row0(20, 40, 50)
    stats = {}
    al = mate_alignment(bytes(mate), [a, c, emptied, EMPTY], K, 1, rec, stats)
    assert al == (2, 0, 80, 0, [(0, 0, 50), (80, 50, 30)]) and stats == {"dropped": 1}
    assert _both_strands(mate, [a, c, emptied, EMPTY], 80, rec) == al
    # read bases [5, 15) on diagonal 55 (record [60, 70)): reached behind read base 49, out of read order
    disorder = _row0(55, 5, 15)
    assert _both_strands(mate, [a, c, disorder, EMPTY], 80, rec) == al
    # trimmed, not emptied: read bases [45, 60) on diagonal 30 (record [75, 90)) keep [50, 60)
    partial = _row0(30, 45, 60)
    stats = {}
    al = mate_alignment(bytes(mate), [a, partial, EMPTY, EMPTY], K, 1, rec, stats)
    assert al == (2, 0, 60, 0, [(0, 0, 50), (80, 50, 10)]) and stats == {"trimmed": 1}
    assert cigar(to_record(al), 80) == ("50M30N10M20S", 0)


def _gap_case(R, G, junk, seed=2, left=30, right=30):
    """exon of `left` bases, R junk bases, exon of `right` bases against a record with G bases between the exons: (mate, rows, record)"""
    rec = _record(seed, left + G + right + 10)
    mate = rec[:left] + bytes(junk) + rec[left + G:left + G + right]
    assert len(junk) == R
    rows = [_row0(0, 0, left), _row0(G - R, left + R, left + R + right), EMPTY, EMPTY]
    return mate, rows, rec


def test_closure_at_one_base_goes_where_it_matches_and_a_tie_goes_left():
    for want_s in (0, 1, "tie", "neither"):
        mate, rows, rec = _gap_case(1, 11, b"A")
        rec = bytearray(rec)                                                      # bases 30 and 40: under the junk base on A's and on B's diagonal
        if want_s == 0:
            rec[30:31], rec[40:41] = _other(b"A"), b"A"
        elif want_s == 1:
            rec[30:31], rec[40:41] = b"A", _other(b"A")
        elif want_s == "tie":
            rec[30:31], rec[40:41] = b"A", b"A"
        else:
            rec[30:31], rec[40:41] = _other(b"A"), _other(b"A")
        stats = {}
        al = mate_alignment(mate, rows, K, 1, bytes(rec), stats)
        assert stats == {"closed": 1}
        if want_s == 0:
            assert al == (2, 0, 61, 0, [(0, 0, 30), (40, 30, 31)])
        elif want_s in (1, "tie"):
            assert al == (2, 0, 61, 0, [(0, 0, 31), (41, 31, 30)])                # the largest s
        else:
            assert al == (2, 0, 60, 1, [(0, 0, 31), (41, 31, 30)])                # cost 1 either way: the largest s, one mismatch
        assert _both_strands(mate, rows, 61, bytes(rec)) == al
        assert cigar(to_record(al), 61, 5) == ("31M10N30M" if want_s != 0 else "30M10N31M", 1 if want_s == "neither" else 0)


def test_the_best_split_in_the_middle_and_ties_between_splits():
    # four junk bases: the first two match A's diagonal only, the last two B's only: s = 2 costs nothing, every other split does
    mate, rows, rec = _gap_case(4, 20, b"ACGT")
    rec = bytearray(rec)
    rec[30:34] = b"AC" + _other(b"G") + _other(b"T")
    rec[46:50] = _other(b"A") + _other(b"C") + b"GT"
    al = _both_strands(mate, rows, 64, bytes(rec))
    assert al == (2, 0, 64, 0, [(0, 0, 32), (48, 32, 32)])
    # every junk base matches both diagonals: every split costs 0, the largest wins
    rec[30:34] = b"ACGT"
    rec[46:50] = b"ACGT"
    assert _both_strands(mate, rows, 64, bytes(rec)) == (2, 0, 64, 0, [(0, 0, 34), (50, 34, 30)])
    # s = 1 and s = 3 both cost 1 (s = 0, 2, 4 cost 2): the larger
    rec[30:34] = b"A" + _other(b"C") + b"G" + _other(b"T")
    rec[46:50] = _other(b"A") + b"C" + _other(b"G") + b"T"
    assert _both_strands(mate, rows, 64, bytes(rec)) == (2, 0, 63, 1, [(0, 0, 33), (49, 33, 31)])


def test_an_insertion_and_a_gap_wider_than_a_wavefront_stay_open():
    # G < R: ten read bases against five record bases
    mate, rows, rec = _gap_case(10, 5, b"ACGTACGTAC")
    stats = {}
    al = mate_alignment(mate, rows, K, 1, rec, stats)
    assert al == (2, 0, 60, 0, [(0, 0, 30), (35, 40, 30)]) and stats == {"open_insertion": 1}
    assert cigar(to_record(al), 70, 20) == ("30M10I5D30M", 15) and cigar(to_record(al), 70, 5) == ("30M10I5N30M", 10)
    # G == R closes, G == R - 1 does not
    for G, closed in ((10, True), (9, False)):
        mate, rows, rec = _gap_case(10, G, b"N" * 10)
        stats = {}
        al = mate_alignment(mate, rows, K, 1, rec, stats)
        assert (stats == {"closed": 1}) == closed and (stats == {"open_insertion": 1}) != closed
        assert al[4] == ([(0, 0, 40), (40, 40, 30)] if closed else [(0, 0, 30), (39, 40, 30)])
    # R = 64 closes, R = 65 stays open
    for R, closed in ((64, True), (65, False)):
        mate, rows, rec = _gap_case(R, 100, b"N" * R)
        stats = {}
        al = _both_strands(mate, rows, 60 + R, rec)
        mate_alignment(mate, rows, K, 1, rec, stats)
        assert stats == ({"closed": 1} if closed else {"open_wide": 1})
        assert al == (2, 0, 60, 0, [(0, 0, 30 + R), (130, 30 + R, 30)] if closed else [(0, 0, 30), (130, 30 + R, 30)])
        assert cigar(to_record(al), 60 + R, 20) == (("94M36N30M", 0) if closed else ("30M65I100N30M", 65))


def test_a_non_base_and_a_masked_byte_inside_a_closure():
    """both count as not a match for a split's cost and as neither a match nor a mismatch in the totals"""
    mate, rows, rec = _gap_case(3, 20, b"ANA")
    rec = bytearray(rec)
    rec[30:33] = b"A" + b"C" + _other(b"A")      # A's diagonal: match, N (not a match), mismatch
    rec[47:50] = _other(b"A") + b"C" + b"A"      # B's diagonal: mismatch, N, match
    # cost: s = 0: 1 + 1 + 0 = 2; s = 1: 0 + 1 + 0 = 1; s = 2: 0 + 1 + 0 = 1; s = 3: 0 + 1 + 1 = 2 -> s = 2
    al = _both_strands(mate, rows, 63, bytes(rec))
    assert al == (2, 0, 62, 0, [(0, 0, 32), (49, 32, 31)])
    # the same byte masked by -q instead (the classifier's mask: the byte minus 64 is no base)
    masked = bytearray(mate)
    masked[31] = (ord("C") - 64) & 0xFF
    assert _both_strands(masked, rows, 63, bytes(rec)) == al
    # a record byte that is no base: neither, and not a match for the cost
    rec2 = bytearray(rec)
    rec2[10] = ord("N")
    rec2[30] = ord("n")
    al2 = mate_alignment(mate, rows, K, 1, bytes(rec2))
    assert al2[2] == al[2] - 2 and al2[3] == 0 and al2[0] == 2


def test_clipping_at_the_record_ends_and_lower_case():
    rec = _record(3, 60)
    mate = bytearray(b"ACGTA" + rec[0:40])                                        # five bases hang over the record's start
    mate[20] |= 0x20
    al = _both_strands(mate, [_row0(-5, 0, 45), EMPTY, EMPTY, EMPTY], 45, rec)
    assert al == (1, 0, 40, 0, [(0, 5, 40)]) and cigar(to_record(al), 45) == ("5S40M", 0)
    mate = bytearray(rec[30:60] + b"ACGTACG")                                     # seven over its end
    al = _both_strands(mate, [_row0(30, 0, 37), EMPTY, EMPTY, EMPTY], 37, rec)
    assert al == (1, 0, 30, 0, [(30, 0, 30)]) and cigar(to_record(al), 37) == ("30M7S", 0)
    # a span wholly outside the record leaves nothing
    assert mate_alignment(bytes(mate), [_row0(60, 0, 37), EMPTY, EMPTY, EMPTY], K, 1, rec) == (0, 0, 0, 0, [])


def test_sam_seq_turns_the_raw_bytes_onto_the_record_strand():
    assert sam_seq(b"ACGTacgtNn-x", 0) == "ACGTacgtNn-x"
    assert sam_seq(b"ACGTacgtNn-x", 1) == "NNNNacgtACGT"
    assert sam_seq(b"AAcG", 1) == "CgTT"


# ---------------------------------------------------------------------------
# shk_alignment_cigar through ctypes
# ---------------------------------------------------------------------------
def _rec(blocks, mismatches=0, strand=0, matches=0):
    return to_record((len(blocks), strand, matches, mismatches, blocks))


def _lib_cigar(rec, L, min_intron, cap=256):
    lib = capi.load()
    one = np.zeros(1, dtype=capi.ALIGNMENT_DTYPE)
    one[0] = rec
    buf = C.create_string_buffer(b"\xff" * cap, cap)
    nm = C.c_uint32(12345)
    rc = lib.shk_alignment_cigar(one.ctypes.data_as(C.c_void_p), L, min_intron, buf, cap, C.byref(nm))
    return rc, (buf.value.decode() if rc == 0 else None), nm.value


def test_cigar_of_the_library_is_the_models_on_the_hand_worked_cases():
    assert os.path.exists(LIB), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    cases = [(_rec([(9653, 0, 74), (10917, 74, 26)]), 100), (_rec([(0, 0, 30), (35, 40, 30)], 2), 70), (_rec([(0, 5, 40)], 1, 1), 45),
             (_rec([(30, 0, 30)]), 37), (_rec([(0, 0, 30), (130, 95, 30)], 3), 125), (_rec([]), 50),
             (_rec([(10, 3, 20), (40, 23, 10), (50, 40, 5), (1000, 45, 7)], 4), 60)]
    for rec, L in cases:
        for mi in (0, 1, 5, 6, 20, 1190, 1191, 0xFFFFFFFF):
            assert _lib_cigar(rec, L, mi) == (0,) + cigar(rec, L, mi), (rec, L, mi)
            assert capi.cigar(rec, L, mi) == cigar(rec, L, mi)
    assert capi.cigar(cases[0][0], 100) == ("74M1190N26M", 0)                      # (the binding's default min_intron is the command's)


def test_cigar_merges_adjacent_equal_operations_and_the_min_intron_edge():
    # two blocks that touch in the read and in the record: one M
    assert _lib_cigar(_rec([(10, 0, 20), (30, 20, 15)]), 40, 20) == (0, "35M5S", 0) == (0,) + cigar(_rec([(10, 0, 20), (30, 20, 15)]), 40, 20)
    # an insertion with no record base between the blocks: I and nothing else
    assert _lib_cigar(_rec([(10, 0, 20), (30, 24, 10)], 1), 34, 20) == (0, "20M4I10M", 5)
    # G = min_intron - 1 is a deletion and counts in NM, G = min_intron is an intron and does not
    r = _rec([(0, 0, 10), (29, 10, 10)], 2)
    assert _lib_cigar(r, 20, 20) == (0, "10M19D10M", 21) and _lib_cigar(r, 20, 19) == (0, "10M19N10M", 2)
    r = _rec([(0, 0, 10), (30, 10, 10)], 2)
    assert _lib_cigar(r, 20, 20) == (0, "10M20N10M", 2) and _lib_cigar(r, 20, 21) == (0, "10M20D10M", 22)
    # min_intron 0: a gap of no record bases writes nothing
    assert _lib_cigar(_rec([(0, 0, 10), (10, 13, 7)]), 20, 0) == (0, "10M3I7M", 3)


def test_cigar_on_random_valid_records():
    rng = np.random.default_rng(99)
    for _ in range(300):
        n = int(rng.integers(1, 5))
        x = q = 0
        blocks = []
        q = int(rng.integers(0, 4)) * int(rng.integers(0, 2))
        x = int(rng.integers(0, 1 << 20))
        for _r in range(n):
            ln = int(rng.integers(1, 200))
            blocks.append((x, q, ln))
            q += ln + int(rng.integers(0, 70)) * int(rng.integers(0, 2))
            x += ln + int(rng.choice([0, 1, 19, 20, 21, 5000])) * int(rng.integers(0, 2))
        L = blocks[-1][1] + blocks[-1][2] + int(rng.integers(0, 3))
        rec = _rec(blocks, int(rng.integers(0, 9)), int(rng.integers(0, 2)))
        for mi in (1, 20, 21):
            assert _lib_cigar(rec, L, mi) == (0,) + cigar(rec, L, mi), (blocks, L, mi)


def test_cigar_refuses_small_buffers_and_inconsistent_records():
    ERR_ARG = -1
    r = _rec([(9653, 0, 74), (10917, 74, 26)])
    assert _lib_cigar(r, 100, 20, cap=12)[:2] == (0, "74M1190N26M")                # 11 characters and the NUL
    assert _lib_cigar(r, 100, 20, cap=11)[0] == ERR_ARG and _lib_cigar(r, 100, 20, cap=1)[0] == ERR_ARG
    assert _lib_cigar(_rec([]), 100, 20, cap=2)[:2] == (0, "*") and _lib_cigar(_rec([]), 100, 20, cap=1)[0] == ERR_ARG
    assert _lib_cigar(r, 99, 20)[0] == ERR_ARG                                     # a block past L
    assert _lib_cigar(_rec([(10, 0, 20), (29, 20, 5)]), 40, 20)[0] == ERR_ARG      # record intervals overlap
    assert _lib_cigar(_rec([(10, 0, 20), (40, 19, 5)]), 40, 20)[0] == ERR_ARG      # read intervals overlap
    assert _lib_cigar(_rec([(10, 0, 20), (40, 20, 0)]), 40, 20)[0] == ERR_ARG      # an empty block
    five = _rec([(0, 0, 1), (2, 1, 1), (4, 2, 1), (6, 3, 1)])
    five["n_blocks"] = 5
    assert _lib_cigar(five, 40, 20)[0] == ERR_ARG
    lib = capi.load()
    assert lib.shk_alignment_cigar(None, 10, 20, C.create_string_buffer(8), 8, None) == ERR_ARG
    with pytest.raises(ValueError):
        capi.cigar(r, 99)


# ---------------------------------------------------------------------------
# the verifier over the model's lines; the example's figures
# ---------------------------------------------------------------------------
def _raw_mates(batch):
    off1, off2 = batch["off1"], batch.get("off2")
    out = []
    for i in range(len(off1) - 1):
        m1 = bytes(batch["seq1"][int(off1[i]):int(off1[i + 1])])
        m2 = bytes(batch["seq2"][int(off2[i]):int(off2[i + 1])]) if batch.get("seq2") is not None else None
        out.append((m1, m2))
    return out


@pytest.mark.parametrize("paired", [True, False])
def test_every_line_of_synthetic_spliced_batches_passes_the_verifier(oracle, paired):
    rng = np.random.default_rng(78 + paired)
    genes = [spliced_gene(rng, 1 + i, 17) for i in range(3)]
    records = [bytes(g) for g, _ in genes]
    sm = SegmentsModel(records, 17)
    o = oracle.Shark(k=17, c=0.0, bf_bits=1 << 26)
    nidx = o.build(records)
    batch = spliced_reads(rng, genes, 300, paired=paired, sub=0.03)
    goff, gids = o.classify(batch["seq1"], batch["off1"], batch.get("seq2"), batch.get("off2"), None, None)
    rows = expected_segments(sm, batch, goff, gids, 4)[1]
    stats = {}
    recs = expected_alignments(sm, batch, goff, gids, rows, 8, stats=stats)
    legend = ["g%d" % g for g in range(nidx)]
    lines = sam_lines(["r%d" % i for i in range(300)], _raw_mates(batch), None, goff, gids, recs, legend, paired)
    fasta = {legend[g]: records[g] for g in range(nidx)}
    print("lines", len(lines), stats)
    assert len(lines) == int((recs["n_blocks"] > 0).sum()) > 100
    assert stats.get("trimmed", 0) >= 1 and stats.get("closed", 0) >= 1
    nms = [verify_sam_line(ln, fasta) for ln in lines]
    assert sum(nm > 0 for nm in nms) >= 20
    assert sam_header(legend, sm, nidx)[:2] == ["@HD\tVN:1.6\tSO:unsorted", "@SQ\tSN:g0\tLN:%d" % len(records[0])]
    flags = {int(ln.split("\t")[1]) for ln in lines}
    assert all(bool(f & 0x1) == paired and bool(f & 0xC0) == paired for f in flags)
    assert any(f & 0x100 for f in flags) == any(goff[i + 1] - goff[i] > 1 for i in range(300))


def _example_alignments(oracle, fa):
    r1 = synth.read_fastq(os.path.join(EXAMPLE, "sample_1.fq"))
    r2 = synth.read_fastq(os.path.join(EXAMPLE, "sample_2.fq"))
    o = oracle.Shark(k=17, c=0.6, bf_bits=1 << 33)
    nidx = o.build([s for _, s in fa])
    batch = synth.batch_from_lists([s for _, s, _ in r1], [s for _, s, _ in r2])
    goff, gids = o.classify(batch["seq1"], batch["off1"], batch["seq2"], batch["off2"], None, None)
    sm = SegmentsModel([s for _, s in fa], 17)
    rows = expected_segments(sm, batch, goff, gids, 4)[1]
    stats = {}
    recs = expected_alignments(sm, batch, goff, gids, rows, 8, stats=stats)
    legend = [n.decode() for n, _ in fa]
    ids = [i.decode() if isinstance(i, bytes) else str(i) for i, _, _ in r1]
    quals = [(bytes(a[2]), bytes(b[2])) for a, b in zip(r1, r2)]
    lines = sam_lines(ids, _raw_mates(batch), quals, goff, gids, recs, legend, True)
    return recs, lines, {legend[g]: bytes(sm.records.get(g, b"")) for g in range(nidx)}, stats


# the model's figures (k = 17, c = 0.6, s_min = 8): the aligned mates are test_spliced_cpu.py's and test_pileup_cpu.py's 3 858 counted
# mates, and the sample, simulated from the record without errors, shows no edit anywhere; against test_variants_cpu.py's record with
# twelve substituted bases the lines with NM > 0 are the mates with a block over one of them (found with the model)
EXAMPLE_MATES = 3858
MUTATED_EXAMPLE_LINES_WITH_EDITS = 1029


def test_the_example_aligns_every_counted_mate_without_an_edit(oracle):
    fa = synth.read_fasta(os.path.join(EXAMPLE, "ENSG00000277117.fa"))
    recs, lines, fasta, stats = _example_alignments(oracle, fa)
    print("example:", len(lines), "lines,", stats, "blocks per mate", np.bincount(recs["n_blocks"].ravel()).tolist())
    assert int((recs["n_blocks"] > 0).sum()) == EXAMPLE_MATES == len(lines)
    assert all(verify_sam_line(ln, fasta) == 0 for ln in lines)
    assert int(recs["mismatches"].sum()) == 0 and (recs["n_blocks"] >= 2).any()


def test_the_mutated_example_shows_its_substitutions_as_edits(oracle):
    from tests.test_variants_cpu import SUBSTITUTED, mutated_example_records
    recs, lines, fasta, stats = _example_alignments(oracle, mutated_example_records())
    nms = [verify_sam_line(ln, fasta) for ln in lines]
    with_edits = sum(nm > 0 for nm in nms)
    print("mutated example:", len(lines), "lines,", with_edits, "with NM > 0,", stats)
    assert with_edits == MUTATED_EXAMPLE_LINES_WITH_EDITS
    # every edit is one of the substituted bases under a block of its line
    for ln, nm in zip(lines, nms):
        if nm:
            f = ln.split("\t")
            x0 = int(f[3]) - 1
            span = sum(int(n) for n, o in re.findall(r"(\d+)([MDN])", f[5]))
            assert any(x0 <= x < x0 + span for x in SUBSTITUTED), ln


# ---------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------
NEW = ("shk_alignments_enable", "shk_alignments_last", "shk_alignment_cigar")


def test_header_declares_and_binding_binds_the_new_calls():
    text = open(os.path.join(ROOT, "include", "shark_hip.h")).read()
    assert "/* ---- alignments:" in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    for s in ("shk_mate_alignment", "shk_alignments"):
        assert re.search(r"\}\s*%s\s*;" % s, hdr), s
    from shark_amd import EXPORTS, SharkHip
    assert set(NEW) <= set(EXPORTS)
    for name in ("alignments_enable", "alignments_last"):
        assert callable(getattr(SharkHip, name))
    assert callable(capi.alignments_from_raw) and callable(capi.alignments_from_device) and callable(capi.cigar)
    assert capi.ALIGNMENT_DTYPE.itemsize == 64
    assert os.path.exists(LIB), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    lib = C.CDLL(LIB)
    for s in NEW:
        assert hasattr(lib, s), s


def test_cli_flags():
    import subprocess
    cli = os.path.join(ROOT, "shark_amd", "bin", "shark")
    assert os.path.exists(cli), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    run = lambda *a: subprocess.run([cli, "-r", "x.fa", "-1", "y.fq"] + list(a), capture_output=True, text=True)  # noqa: E731
    r = run("--sam", "s", "--sam-min-support", "0")
    assert r.returncode == 1 and "--sam-min-support must be at least 1" in r.stderr
    for flag in ("--sam-min-support", "--sam-min-intron"):
        r = run(flag, "8")
        assert r.returncode == 1 and "need --sam FILE" in r.stderr
    r = run("--sam")
    assert r.returncode == 1 and "unknown argument" in r.stderr           # (a missing FILE)
    r = subprocess.run([cli, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and all(s in r.stderr for s in ("--sam FILE", "--sam-min-support N", "--sam-min-intron N"))
