"""Segments mode without a GPU: the model (tests/segments_model.py) against placement's on every association, spliced reads worked
out by hand, the junction function (the model's and the binding's), the bundled example, and the boundary -- the two new symbols in
the header and the binding, `--segments` / `--junctions` in the command."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import synth
from tests.placement_model import PlacementModel, expected_placements
from tests.segments_model import SegmentsModel, expected_segments, junction_lines, junctions, mate_lengths, segment_lines, span

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "shark_amd", "libsharkhip.so")
CLI = os.path.join(ROOT, "shark_amd", "bin", "shark")
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example")

# test_placement_cpu.py's record: 26 bases, 22 windows of 5 with 22 different canonical 5-mers
R = b"CACGTTAGTCCTGGGGTTAAGTAGTT"
# 60 bases, 56 windows of 5 with 56 different canonical 5-mers; G[14:17] == G[30:33] (a 3-base microhomology between a donor at 14
# and an acceptor at 30) with G[13] != G[29] and G[17] != G[33]; the "exons" of the cases below are G[4:14], G[24:33], G[30:40],
# G[36:46] and G[44:54]
#        0         1         2         3         4         5
#        012345678901234567890123456789012345678901234567890123456789
G = b"ATCCGAGTTCGGTCGCCGGAGACATGCTGAGCCTTGCATACACAGATAAGATCGTGCTCT"
K = 5


def _rc(b):
    return bytes(synth.revcomp(np.frombuffer(bytes(b), np.uint8)))


@pytest.fixture(scope="module")
def oracle_lib(oracle):
    return oracle.lib()


def test_the_record_is_what_the_cases_assume(oracle_lib):
    from tests.placement_model import windows
    w = windows(G, K)
    assert len(G) == 60 and [p for p, _, _ in w] == list(range(56)) and len({c for _, c, _ in w}) == 56
    assert G[14:17] == G[30:33] and G[13] != G[29] and G[17] != G[33]


# ---------------------------------------------------------------------------
# spliced reads, by hand.  A row is (strand, pos, support, first, last); a junction (donor, acceptor, intron, overlap)
# ---------------------------------------------------------------------------
def test_one_intron_on_each_strand(oracle_lib):
    m = SegmentsModel([G], K)
    read = G[4:14] + G[36:46]              # 20 bases, 16 slots
    # slots 0 .. 5 lie in the first part: window x = 4 + p, pos 4; slots 10 .. 15 in the second: x = 36 + p - 10, pos 26; slots 6 .. 9
    # straddle the junction and match nothing.  Six votes each: the smaller pos is rank 0
    assert m.mate_segments(0, read, 4) == (2, [(0, 4, 6, 0, 5), (0, 26, 6, 10, 15), (0, 0, 0, 0, 0), (0, 0, 0, 0, 0)])
    assert span((0, 4, 6, 0, 5), 20, K) == (4, 14) and span((0, 26, 6, 10, 15), 20, K) == (36, 46)
    assert junctions(m.mate_segments(0, read, 4)[1], 20, K, 6) == [(14, 36, 22, 0)]
    # reversed: slot p is slot 15 - p of the read above; pos = x + p + k - L is the same record coordinate
    assert m.mate_segments(0, _rc(read), 4) == (2, [(1, 4, 6, 10, 15), (1, 26, 6, 0, 5), (0, 0, 0, 0, 0), (0, 0, 0, 0, 0)])
    assert span((1, 4, 6, 10, 15), 20, K) == (4, 14) and span((1, 26, 6, 0, 5), 20, K) == (36, 46)
    assert junctions(m.mate_segments(0, _rc(read), 4)[1], 20, K, 6) == [(14, 36, 22, 0)]
    assert junctions(m.mate_segments(0, read, 4)[1], 20, K, 7) == []          # neither side reaches 7


def test_two_introns_in_one_mate_and_more_keys_than_entries(oracle_lib):
    m = SegmentsModel([G], K)
    read = G[4:14] + G[24:33] + G[44:54]   # 10 + 9 + 10 bases: the parts start at read offsets 0, 10 and 19
    # slots 0 .. 5: pos 4; slots 10 .. 14: x = 24 + p - 10, pos 14; slots 19 .. 24: x = 44 + p - 19, pos 25
    full = [(0, 4, 6, 0, 5), (0, 25, 6, 19, 24), (0, 14, 5, 10, 14)]
    assert m.mate_keys(0, read) == full
    assert m.mate_segments(0, read, 4) == (3, full + [(0, 0, 0, 0, 0)])
    assert junctions(full, 29, K, 5) == [(14, 24, 10, 0), (33, 44, 11, 0)]
    # with the middle exon below the floor the outer two are consecutive: one junction over both introns
    assert junctions(full, 29, K, 6) == [(14, 44, 21, -9)]
    # n_keys > m: the reported entries are the top m
    assert m.mate_segments(0, read, 2) == (3, full[:2])
    assert m.mate_segments(0, read, 1) == (3, full[:1])
    assert junctions(full[:1], 29, K, 5) == []


def test_microhomology_and_substitution_at_the_junction(oracle_lib):
    m = SegmentsModel([G], K)
    # G[14:17] == G[30:33]: the read's bases 10 .. 12 continue the first diagonal as well, slots 6 .. 8 vote for pos 4 (x = 10 .. 12)
    read = G[4:14] + G[30:40]
    rows = m.mate_segments(0, read, 4)[1]
    assert rows[:2] == [(0, 4, 9, 0, 8), (0, 20, 6, 10, 15)]
    assert junctions(rows, 20, K, 6) == [(17, 30, 16, 3)]
    # a substitution at read offset 8 silences slots 4 .. 8: the first part's last voting slot is 3, hi = 4 + 3 + 5 = 12
    read = bytearray(G[4:14] + G[36:46])
    read[8] = ord("A") if read[8] != ord("A") else ord("C")
    rows = m.mate_segments(0, bytes(read), 4)[1]
    assert rows[:2] == [(0, 26, 6, 10, 15), (0, 4, 4, 0, 3)]
    assert junctions(rows, 20, K, 4) == [(12, 36, 22, -2)]


def test_tie_order_between_strands(oracle_lib):
    m = SegmentsModel([R], K)
    # (test_placement_cpu.py::test_ties) R[2:10] and the reverse complement of R[10:18]: four votes each, strand 0 first
    assert m.mate_segments(0, R[2:10] + _rc(R[10:18]), 2) == (2, [(0, 2, 4, 0, 3), (1, 10, 4, 8, 11)])
    assert m.mate_segments(0, R[2:10] + _rc(R[10:19]), 2)[1] == [(1, 10, 5, 8, 12), (0, 2, 4, 0, 3)]          # (a window over the joint votes as well)
    # the other strand is never a junction partner
    assert junctions(m.mate_segments(0, R[2:10] + _rc(R[10:18]), 2)[1], 16, K, 1) == []
    # one inserted base: two diagonals one base apart, pos_B < pos_A in record order -- an insertion in the read, not a junction
    rows = m.mate_segments(0, R[2:10] + b"A" + R[10:18], 2)[1]
    assert rows == [(0, 1, 4, 9, 12), (0, 2, 4, 0, 3)] and junctions(rows, 17, K, 1) == []


def test_short_mate_and_single_end_batch(oracle_lib):
    m = SegmentsModel([G], K)
    assert m.mate_segments(0, G[:4], 3) == (0, [(0, 0, 0, 0, 0)] * 3)
    assert junctions(m.mate_segments(0, G[:4], 3)[1], 4, K, 1) == []
    batch = synth.batch_from_lists([G[4:14] + G[36:46], G[:4]])
    keys, rows = expected_segments(m, batch, [0, 1, 2], [0, 0], 2)
    assert keys.tolist() == [[2, 0], [0, 0]]
    assert rows[0].tolist() == [[[0, 4, 6, 0, 5], [0, 26, 6, 10, 15]], [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]] and not rows[1].any()
    assert mate_lengths(batch).tolist() == [[20, 0], [4, 0]]


def test_the_worked_example_of_the_header(oracle_lib):
    rows = [(1, 9653, 58, 26, 83), (1, 10843, 15, 0, 14)]
    assert span(rows[0], 100, 17) == (9653, 9727) and span(rows[1], 100, 17) == (10912, 10943)
    assert junctions(rows, 100, 17, 8) == [(9727, 10912, 1190, 5)]
    assert junctions(rows, 100, 17, 16) == []
    assert junctions(rows[::-1], 100, 17, 8) == [(9727, 10912, 1190, 5)]          # (record order, not rank order, decides)


def test_the_binding_computes_the_same_junctions(oracle_lib):
    from shark_amd import capi
    m = SegmentsModel([G], K)
    reads = [G[4:14] + G[36:46], G[4:14] + G[24:33] + G[44:54], G[4:14] + G[30:40], _rc(G[4:14] + G[36:46]), G[:4], G[4:30]]
    some = 0
    for rd in reads:
        for mm in (1, 2, 4):
            for s_min in (1, 5, 6, 8):
                rows = m.mate_segments(0, rd, mm)[1]
                assert capi.junctions(rows, len(rd), K, s_min) == junctions(rows, len(rd), K, s_min)
                some += len(junctions(rows, len(rd), K, s_min))
    assert some > 10
    assert capi.junctions([(1, 9653, 58, 26, 83), (1, 10843, 15, 0, 14)], 100, 17) == [(9727, 10912, 1190, 5)]
    assert capi.segment_span((1, 10843, 15, 0, 14), 100, 17) == (10912, 10943)
    raw = np.array([[[[0xFFFFFFFE, 7, 1, 2, 9]]]], dtype=np.uint32)          # {pos = -2, support, strand, first, last}
    assert capi.segments_from_raw(raw).tolist() == [[[[1, -2, 7, 2, 9]]]]


def test_lines(oracle_lib):
    keys = np.array([[2, 1], [0, 3]], dtype=np.uint32)
    rows = np.zeros((2, 2, 2, 5), dtype=np.int64)
    rows[0, 0] = [[0, 4, 6, 0, 5], [0, 26, 6, 10, 15]]
    rows[0, 1, 0] = [1, -3, 2, 1, 2]
    rows[1, 1, 0] = [0, 9, 7, 3, 9]
    assert segment_lines(["r0", "r1", "r2"], [0, 1, 1, 2], [1, 0], keys, rows, ["gA", "gB"], True) == [
        "r0 gB 2 0 4 6 0 5 0 26 6 10 15 1 1 -3 2 1 2 0 0 0 0 0", "r2 gA 0 0 0 0 0 0 0 0 0 0 0 3 0 9 7 3 9 0 0 0 0 0"]
    assert segment_lines(["r0"], [0, 1], [1], keys, rows, ["gA", "gB"], False) == ["r0 gB 2 0 4 6 0 5 0 26 6 10 15"]
    # two reads with the same junction in gene 1, one in gene 0: sorted by gene index, donor, acceptor
    rows = np.zeros((3, 2, 2, 5), dtype=np.int64)
    rows[0, 0] = rows[1, 1] = [[0, 4, 6, 0, 5], [0, 26, 6, 10, 15]]
    rows[2, 0] = [[0, 4, 6, 0, 5], [0, 26, 6, 10, 15]]
    lengths = np.full((3, 2), 20)
    assert junction_lines([0, 1, 2, 3], [1, 1, 0], rows, lengths, K, ["gA", "gB"], 6) == ["gA 14 36 22 1", "gB 14 36 22 2"]
    assert junction_lines([0, 1, 2, 3], [1, 1, 0], rows, lengths, K, ["gA", "gB"], 7) == []
    # two mates with one (gene, donor, acceptor) and different introns -- a base inserted in the second read just behind the junction
    # moves its second diagonal by one while the spans stay [4, 14) and [36, 46): one line, two mates, the smaller intron
    rows = np.zeros((2, 2, 2, 5), dtype=np.int64)
    rows[0, 0] = [[0, 4, 6, 0, 5], [0, 26, 6, 10, 15]]
    rows[1, 0] = [[0, 4, 6, 0, 5], [0, 25, 6, 11, 16]]
    assert junction_lines([0, 1, 2], [0, 0], rows, np.array([[20, 0], [21, 0]]), K, ["gA"], 6) == ["gA 14 36 21 2"]
    assert junction_lines([0, 1, 2], [0, 0], rows[::-1], np.array([[21, 0], [20, 0]]), K, ["gA"], 6) == ["gA 14 36 21 2"]


# ---------------------------------------------------------------------------
# rank 0 is the placement, association for association
# ---------------------------------------------------------------------------
def _rank0(rows):
    return rows[:, :, 0, :3]


def test_rank_0_is_the_placement_on_synthetic_batches(oracle_lib):
    """test_placement_cpu.py's hand-made mates and the reads of its yardstick check (same generator, both strands), and mates cut from
    two places of a gene"""
    pm, sm = PlacementModel([R], K), SegmentsModel([R], K)
    hand = [R[3:15], _rc(R[3:15]), b"GGGG" + R[:8], R[-8:] + b"GGGG", R[2:10] + b"A" + R[10:18], R[2:10] + _rc(R[10:18]), R[2:10] + _rc(R[10:19]), b"CACG",
            R[3:9] + b"N" + R[10:15]]
    for rd in hand:
        n_keys, rows = sm.mate_segments(0, rd, 4)
        assert rows[0][:3] == pm.place_mate(0, rd) and n_keys == len(sm.mate_keys(0, rd))
    rng = np.random.default_rng(3)
    genes = synth.make_genes(rng, 100, 600, 1400)
    pm, sm = PlacementModel([bytes(g) for g in genes], 17), SegmentsModel([bytes(g) for g in genes], 17)
    m1, m2, gids = [], [], []
    for _ in range(150):
        gi = int(rng.integers(0, len(genes)))
        g = genes[gi]
        a, b = int(rng.integers(0, len(g) - 100)), int(rng.integers(0, len(g) - 100))
        m1.append(g[a:a + 100])
        m2.append(synth.revcomp(np.concatenate([g[a:a + 60], g[b:b + 40]])))
        gids.append(gi)
    batch = synth.batch_from_lists(m1, m2)
    goff = np.arange(len(gids) + 1)
    keys, rows = expected_segments(sm, batch, goff, gids, 4)
    assert np.array_equal(_rank0(rows), expected_placements(pm, batch, goff, gids))
    assert int((keys[:, 1] >= 2).sum()) > 100 and int((rows[:, 0, 0, 2] == 84).sum()) > 140          # (not vacuous)


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
    keys, rows = expected_segments(sm, batch, goff, gids, 4)
    return fa, batch, goff, gids, keys, rows


def test_the_example_rank_0_and_junctions(example):
    """on the bundled example rank 0 is the placement of every association, and both mate files show junctions at s_min = 8 (the
    counts are DESIGN.md 11's)"""
    fa, batch, goff, gids, keys, rows = example
    pm = PlacementModel([s for _, s in fa], 17)
    assert int(goff[-1]) == 1929
    assert np.array_equal(_rank0(rows), expected_placements(pm, batch, goff, gids))
    lengths = mate_lengths(batch)
    read_of = np.repeat(np.arange(len(goff) - 1), np.diff(goff))
    n_junc = [0, 0]
    multi = [0, 0]
    for j in range(int(goff[-1])):
        for t in range(2):
            n_junc[t] += len(junctions(rows[j, t], int(lengths[read_of[j], t]), 17, 8))
            multi[t] += int((rows[j, t, :, 2] >= 8).sum() >= 2)
    print("example: mates with two or more diagonals of at least 8 votes", multi, "junctions", n_junc)
    assert n_junc[0] >= 1 and n_junc[1] >= 1
    assert (multi, n_junc) == (EXAMPLE_MULTI, EXAMPLE_JUNCTIONS)
    lines = junction_lines(goff, gids, rows, lengths, 17, [n.decode() for n, _ in fa], 8)
    assert len(lines) == EXAMPLE_DISTINCT and sum(int(ln.split(" ")[4]) for ln in lines) == sum(n_junc)


# the model's figures on the example (k = 17, c = 0.6, m = 4, s_min = 8), as DESIGN.md 11 quotes them
EXAMPLE_MULTI = [417, 477]
EXAMPLE_JUNCTIONS = [468, 535]
EXAMPLE_DISTINCT = 9


# ---------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------
NEW = ("shk_segments_enable", "shk_segments_last")


def test_header_declares_and_binding_binds_the_new_calls():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "shark_hip.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    assert "typedef struct shk_segment { int32_t pos; uint32_t support, strand, first, last; } shk_segment;" in hdr
    assert re.search(r"#define\s+SHK_MAX_SEGMENTS\s+4\b", hdr)
    from shark_amd import EXPORTS, SharkHip, capi
    assert set(NEW) <= set(EXPORTS) and capi.SHK_MAX_SEGMENTS == 4
    for name in ("segments_enable", "segments_last"):
        assert callable(getattr(SharkHip, name))
    assert os.path.exists(LIB), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    import ctypes as C
    lib = C.CDLL(LIB)
    for s in NEW:
        assert hasattr(lib, s), s


def test_cli_flags():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.join(ROOT, "shark_amd", "csrc"), "-j4", "all"], check=True, stdout=subprocess.DEVNULL)
    for flag in ("--segments", "--junctions", "--segments-max", "--junctions-min-support"):
        r = subprocess.run([CLI, "-r", "x.fa", "-1", "y.fq", flag], capture_output=True, text=True)
        assert r.returncode == 1 and flag[2:] in r.stderr
    r = subprocess.run([CLI, "-r", "x.fa", "-1", "y.fq", "--segments-max", "5"], capture_output=True, text=True)
    assert r.returncode == 1 and "--segments-max must be in the range [1, 4]" in r.stderr
    r = subprocess.run([CLI, "-r", "x.fa", "-1", "y.fq", "--junctions-min-support", "0"], capture_output=True, text=True)
    assert r.returncode == 1 and "--junctions-min-support must be at least 1" in r.stderr
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--segments FILE" in r.stderr and "--junctions FILE" in r.stderr
