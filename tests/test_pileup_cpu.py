"""Pileup mode without a GPU: the model (tests/pileup_model.py) on mates worked out by hand, its identity with spliced depth's model
on the bundled example and on synthetic spliced batches, the `--pileup` line format, and the boundary -- the five new symbols in the
header and the binding, the new flags of the command."""
import os
import re
import subprocess

import numpy as np
import pytest

from shark_amd import capi
from tests import synth
from tests.depth_model import model_layout
from tests.pileup_model import add_mate, expected_pileup, mate_alleles, pileup_lines
from tests.segments_model import SegmentsModel, expected_segments
from tests.spliced_model import expected_spliced_depth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "shark_amd", "libsharkhip.so")
CLI = os.path.join(ROOT, "shark_amd", "bin", "shark")
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example")

# test_segments_cpu.py's record: 60 bases, 56 windows of 5 with 56 different canonical 5-mers; G[14:17] == G[30:33]
#        0         1         2         3         4         5
#        012345678901234567890123456789012345678901234567890123456789
G = b"ATCCGAGTTCGGTCGCCGGAGACATGCTGAGCCTTGCATACACAGATAAGATCGTGCTCT"
K = 5
CODE = {c: i for i, c in enumerate(b"ACGT")}


def _rc(b):
    return bytes(synth.revcomp(np.frombuffer(bytes(b), np.uint8)))


def _pile(oracle, reads, s_min=5, record=G):
    """(counts, lost, mates) of single-end reads, each associated with gene 0 of the one-record reference"""
    oracle.lib()
    m = SegmentsModel([record], K)
    batch = synth.batch_from_lists([np.frombuffer(bytes(r), np.uint8) for r in reads])
    goff, gids = np.arange(len(reads) + 1), [0] * len(reads)
    rows = expected_segments(m, batch, goff, gids, 4)[1]
    return expected_pileup(m, batch, goff, gids, rows, s_min)


def _reference_counts(lo, hi, record=G):
    want = np.zeros((len(record), 4), dtype=np.uint32)
    for x in range(lo, hi):
        want[x, CODE[record[x]]] += 1
    return want


def test_a_substitution_shows_at_its_base_on_either_strand(oracle):
    mate = bytearray(G[10:40])
    assert mate[15] == ord("G")
    mate[15] = ord("T")                                      # record base 25: windows 11 .. 15 fall silent, the diagonal's span does not
    want = _reference_counts(10, 40)
    want[25] = (0, 0, 0, 1)
    for read in (bytes(mate), _rc(mate)):
        counts, lost, mates = _pile(oracle, [read])
        assert np.array_equal(counts, want) and not lost.any() and mates == 1
    counts, _, mates = _pile(oracle, [bytes(mate), _rc(mate), G[10:40]])
    want = 3 * _reference_counts(10, 40)
    want[25] = (0, 0, 1, 2)
    assert np.array_equal(counts, want) and mates == 3


def test_the_worked_example_of_the_header():
    """spans [9653, 9727) and [10912, 10943) on strand 1: 74 + 31 observations, none between"""
    rng = np.random.default_rng(5)
    mate = bytes(synth.random_seq(rng, 100))
    rows = [(1, 9653, 58, 26, 83), (1, 10843, 15, 0, 14), (0, 0, 0, 0, 0), (0, 0, 0, 0, 0)]
    seen = mate_alleles(mate, rows, 17, 8, 20000)
    own = np.nonzero(seen >= 0)[0]
    assert own.tolist() == list(range(9653, 9727)) + list(range(10912, 10943)) and len(own) == 74 + 31 and (seen[own] < 4).all()
    # strand 1: record base x reads mate byte pos + L - 1 - x, complemented
    assert seen[9653] == 3 - CODE[mate[99]] and seen[9726] == 3 - CODE[mate[26]]
    assert seen[10912] == 3 - CODE[mate[30]] and seen[10942] == 3 - CODE[mate[0]]
    counts, lost = np.zeros((20000, 4), np.uint32), np.zeros(20000, np.uint32)
    assert add_mate(counts, lost, 0, seen) and int(counts.sum()) == 105 and not counts[9727:10912].any()
    # a floor above the second diagonal's support keeps the first span alone
    assert int((mate_alleles(mate, rows, 17, 16, 20000) >= 0).sum()) == 74


def test_overlapping_spans_count_a_base_once_from_the_earlier_span(oracle):
    """six bases repeated: the mate's diagonals (pos 4, pos -2) span [4, 24) and [18, 40); [18, 24) belongs to the first.  The first
    copy of record base 18 is substituted (window 15 still votes, so the first span keeps its end): the substitute is what counts"""
    mate = bytearray(G[4:24] + G[18:40])
    assert mate[14] == ord("G") and mate[20] == ord("G")     # the two copies of record base 18
    mate[14] = ord("C")
    oracle.lib()
    m = SegmentsModel([G], K)
    batch = synth.batch_from_lists([np.frombuffer(bytes(mate), np.uint8)])
    rows = expected_segments(m, batch, [0, 1], [0], 4)[1]
    assert [sp[:2] for sp in capi.kept_spans(rows[0, 0], len(mate), K, 5)] == [(4, 24), (18, 40)]
    counts, lost, mates = expected_pileup(m, batch, [0, 1], [0], rows, 5)
    want = _reference_counts(4, 40)
    want[18] = (0, 1, 0, 0)
    assert np.array_equal(counts, want) and int(counts.sum()) == 36 and mates == 1
    for read in (bytes(mate), _rc(mate)):                    # (either strand)
        assert np.array_equal(_pile(oracle, [read])[0], want)


def test_a_non_base_makes_no_observation_and_lower_case_counts(oracle):
    mate = bytearray(G[10:40])
    mate[15] = ord("N")
    mate[20] = mate[20] | 0x20
    assert chr(mate[20]) == "g"
    want = _reference_counts(10, 40)
    want[25] = 0
    for read in (bytes(mate), _rc(mate)):
        counts, lost, mates = _pile(oracle, [read])
        assert np.array_equal(counts, want) and mates == 1
        assert lost[25] == 1 and int(lost.sum()) == 1
    # a mate that owns bases but shows none is a pileup mate all the same (the header's rule is ownership)
    rows = [(0, 10, 6, 0, 5), (0, 0, 0, 0, 0)]
    seen = mate_alleles(b"N" * 10, rows, K, 5, 60)
    assert (seen[10:20] == 4).all() and (seen[:10] == -1).all() and (seen[20:] == -1).all()


def test_spans_are_clipped_at_the_record_ends():
    mate = b"ACGTACGTACGTACGTACGT"
    seen = mate_alleles(mate, [(0, 50, 6, 0, 15)], K, 5, 60)                   # span [50, 70) of a record of 60
    assert np.nonzero(seen >= 0)[0].tolist() == list(range(50, 60)) and seen[50:60].tolist() == [CODE[c] for c in mate[:10]]
    seen = mate_alleles(mate, [(0, -3, 6, 0, 15)], K, 5, 60)                   # span [-3, 17)
    assert np.nonzero(seen >= 0)[0].tolist() == list(range(0, 17)) and seen[:17].tolist() == [CODE[c] for c in mate[3:20]]
    seen = mate_alleles(mate, [(1, 50, 6, 0, 15)], K, 5, 60)                   # strand 1: span [50, 70), byte 50 + 19 - x
    assert seen[50:60].tolist() == [3 - CODE[c] for c in mate[::-1][:10]]
    assert not (mate_alleles(mate, [(0, 60, 6, 0, 15)], K, 5, 60) >= 0).any()


# ---------------------------------------------------------------------------
# the identity with spliced depth's model
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def example(oracle):
    fa = synth.read_fasta(os.path.join(EXAMPLE, "ENSG00000277117.fa"))
    r1 = synth.read_fastq(os.path.join(EXAMPLE, "sample_1.fq"))
    r2 = synth.read_fastq(os.path.join(EXAMPLE, "sample_2.fq"))
    o = oracle.Shark(k=17, c=0.6, bf_bits=1 << 33)
    o.build([s for _, s in fa])
    batch = synth.batch_from_lists([s for _, s, _ in r1], [s for _, s, _ in r2])
    goff, gids = o.classify(batch["seq1"], batch["off1"], batch["seq2"], batch["off2"], None, None)
    sm = SegmentsModel([s for _, s in fa], 17)
    rows = expected_segments(sm, batch, goff, gids, 4)[1]
    return fa, batch, goff, gids, sm, rows


# the model's figures on the example (k = 17, c = 0.6, s_min = 8): test_spliced_cpu.py's 378 301 union bases and 3 858 mates, of which
# every one is an observation (the sample's reads hold no N); record bases where two or more alleles were each seen at least twice
# (none: the sample was simulated without variants), and record bases where a second allele was seen at all
EXAMPLE_UNION_BASES = 378301
EXAMPLE_MATES = 3858
EXAMPLE_OBSERVATIONS = 378301
EXAMPLE_MULTI_ALLELE_POSITIONS = 0
EXAMPLE_SECOND_ALLELE_POSITIONS = 0


def test_the_example_sums_to_spliced_depth(example):
    fa, batch, goff, gids, sm, rows = example
    counts, lost, mates = expected_pileup(sm, batch, goff, gids, rows, 8)
    depth, depth_mates = expected_spliced_depth(sm, batch, goff, gids, rows, 8)
    assert np.array_equal(counts.sum(axis=1, dtype=np.uint64) + lost, depth) and mates == depth_mates
    multi = int(((counts >= 2).sum(axis=1) >= 2).sum())
    print("example: observations", int(counts.sum()), "lost", int(lost.sum()), "mates", mates, "positions with two alleles seen twice", multi)
    assert (int(depth.sum()), mates) == (EXAMPLE_UNION_BASES, EXAMPLE_MATES)
    assert int(counts.sum()) == EXAMPLE_OBSERVATIONS and int(counts.sum()) + int(lost.sum()) == EXAMPLE_UNION_BASES
    second = int(((counts >= 1).sum(axis=1) >= 2).sum())
    print("example: positions with a second allele", second)
    assert multi == EXAMPLE_MULTI_ALLELE_POSITIONS and second == EXAMPLE_SECOND_ALLELE_POSITIONS
    # nothing compares the reads with the record on the device, but the pileup must look like it: where ten mates or more show a
    # base, the base most of them show is the record's nearly everywhere
    rec = np.frombuffer(bytes(fa[0][1]).upper(), np.uint8)
    deep = np.nonzero(counts.sum(axis=1) >= 10)[0]
    assert len(deep) > 1000 and (synth.ACGT[counts[deep].argmax(axis=1)] == rec[deep]).mean() > 0.99


@pytest.mark.parametrize("masked", [False, True])
def test_synthetic_spliced_batches_sum_to_spliced_depth(oracle, masked):
    from tests.test_gpu_spliced_depth import spliced_gene, spliced_reads
    oracle.lib()
    rng = np.random.default_rng(77 + masked)
    genes = [spliced_gene(rng, 1 + i, 17) for i in range(3)]
    sm = SegmentsModel([bytes(g) for g, _ in genes], 17)
    q = 20 if masked else 0
    o = oracle.Shark(k=17, c=0.0, bf_bits=1 << 26, min_quality=q)
    o.build([bytes(g) for g, _ in genes])
    batch = spliced_reads(rng, genes, 300, sub=0.03, qual=masked, lower=0.2 if masked else 0.0)
    goff, gids = o.classify(batch["seq1"], batch["off1"], batch["seq2"], batch["off2"], batch.get("qual1"), batch.get("qual2"))
    rows = expected_segments(sm, batch, goff, gids, 4, q)[1]
    counts, lost, mates = expected_pileup(sm, batch, goff, gids, rows, 8, q)
    depth, depth_mates = expected_spliced_depth(sm, batch, goff, gids, rows, 8)
    total = counts.sum(axis=1, dtype=np.uint64)
    assert np.array_equal(total + lost, depth) and mates == depth_mates and mates > 100
    assert (total <= depth).all() and (lost.any() == masked)
    # sub = 0.03: alternative alleles exist (behind the mask few mates keep a diagonal of 8 windows of 17: not asked there)
    assert masked or int((np.sort(counts, axis=1)[:, :3].sum(axis=1) > 0).sum()) >= 20


def test_pileup_lines_by_hand():
    counts = np.array([[0, 0, 0, 0], [3, 0, 1, 0], [0, 0, 0, 12], [0, 2, 0, 0]], dtype=np.uint32)
    assert pileup_lines(counts, [0, 3, 3, 4], ["g one", "empty", "g2"]) == ["g one 1 3 0 1 0", "g one 2 0 0 0 12", "g2 0 0 2 0 0"]
    assert pileup_lines(counts[:1], [0, 1], ["g"]) == []


# ---------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------
NEW = ("shk_pileup_enable", "shk_pileup_get", "shk_pileup_get_all", "shk_pileup_mates", "shk_pileup_reset")


def test_header_declares_and_binding_binds_the_new_calls():
    text = open(os.path.join(ROOT, "include", "shark_hip.h")).read()
    assert "/* ---- pileup:" in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    from shark_amd import EXPORTS, SharkHip
    assert set(NEW) <= set(EXPORTS)
    for name in ("pileup_enable", "pileup", "pileup_all", "pileup_mates", "pileup_reset"):
        assert callable(getattr(SharkHip, name))
    assert os.path.exists(LIB), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    import ctypes as C
    lib = C.CDLL(LIB)
    for s in NEW:
        assert hasattr(lib, s), s


def test_cli_flags():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.join(ROOT, "shark_amd", "csrc"), "-j4", "all"], check=True, stdout=subprocess.DEVNULL)
    run = lambda *a: subprocess.run([CLI, "-r", "x.fa", "-1", "y.fq"] + list(a), capture_output=True, text=True)  # noqa: E731
    r = run("--pileup", "p", "--pileup-min-support", "0")
    assert r.returncode == 1 and "--pileup-min-support must be at least 1" in r.stderr
    r = run("--pileup-min-support", "8")
    assert r.returncode == 1 and "--pileup-min-support needs --pileup FILE" in r.stderr
    r = run("--pileup")
    assert r.returncode == 1 and "unknown argument" in r.stderr           # (a missing FILE)
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--pileup FILE" in r.stderr and "--pileup-min-support N" in r.stderr
