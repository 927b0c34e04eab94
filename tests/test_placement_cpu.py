"""Placement mode without a GPU: the model (tests/placement_model.py) on cases worked out by hand, a guard against a vacuous
yardstick, and the boundary -- the three new symbols in the header and the binding, `--placements` in the command."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import synth
from tests.placement_model import PlacementModel, expected_placements, gene_records, masked_mates, placement_lines, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "shark_amd", "libsharkhip.so")
CLI = os.path.join(ROOT, "shark_amd", "bin", "shark")

# 26 bases whose 22 windows of 5 have 22 different canonical 5-mers (k odd: no window is its own reverse complement)
#        0         1         2
#        01234567890123456789012345
R = b"CACGTTAGTCCTGGGGTTAAGTAGTT"


def _rc(b):
    return bytes(synth.revcomp(np.frombuffer(bytes(b), np.uint8)))


@pytest.fixture(scope="module")
def oracle_lib(oracle):
    return oracle.lib()


def test_the_record_is_what_the_cases_assume(oracle_lib):
    w = windows(R, 5)
    assert [p for p, _, _ in w] == list(range(22)) and len({c for _, c, _ in w}) == 22


def test_forward_reverse_and_overhangs(oracle_lib):
    m = PlacementModel([R], 5)
    read = R[3:15]                                        # 12 bases, 8 slots, slot p is window x = 3 + p
    assert m.place_mate(0, read) == (0, 3, 8)
    assert m.place_mate(0, _rc(read)) == (1, 3, 8)       # slot p is window x = 10 - p reversed: 10 - p + p + 5 - 12 = 3
    # four foreign bases in front of R[0:8]: slots 4 .. 7 are windows 0 .. 3, pos = x - p = -4; the slots that touch the foreign bases match nothing
    assert m.place_mate(0, b"GGGG" + R[:8]) == (0, -4, 4)
    # R[18:26] and four foreign bases: slots 0 .. 3 are windows 18 .. 21; pos + L = 30 passes the record's end (26)
    assert m.place_mate(0, R[-8:] + b"GGGG") == (0, 18, 4)


def test_ties(oracle_lib):
    m = PlacementModel([R], 5)
    # one inserted base: slots 0 .. 3 lie on x - p = 2, slots 9 .. 12 (windows 10 .. 13) on x - p = 1; four votes each: the smaller pos
    assert m.place_mate(0, R[2:10] + b"A" + R[10:18]) == (0, 1, 4)
    # R[2:10] and the reverse complement of R[10:18], 16 bases: slots 0 .. 3 vote (0, 2); slot 8 + j is window 13 - j reversed,
    # pos = 13 - j + 8 + j + 5 - 16 = 10, four votes for (1, 10): strand 0 first
    assert m.place_mate(0, R[2:10] + _rc(R[10:18])) == (0, 2, 4)
    # ... and with one more base of the second part strand 1 has five votes and wins
    assert m.place_mate(0, R[2:10] + _rc(R[10:19])) == (1, 10, 5)


def test_a_kmer_twice_in_the_gene_does_not_vote(oracle_lib):
    #       0         1         2
    #       0123456789012345678901234
    r2 = b"ACGTTGCATGGACCTAACGTTGAGC"     # ACGTT at 0 and 16 (and its reverse complement AACGT at 15), CGTTG at 1 and 17
    m = PlacementModel([r2], 5)
    assert m.place_mate(0, r2[:10]) == (0, 0, 4)          # six slots, the first two are ambiguous
    assert m.place_mate(0, r2[:6]) == (0, 0, 0)           # only ambiguous slots: no vote at all


def test_even_k_palindromic_window(oracle_lib):
    rec = b"TTACGTGGCA"                   # k = 4: ACGT at 2 is its own reverse complement
    m = PlacementModel([rec], 4)
    assert m.place_mate(0, rec) == (0, 0, 6)              # seven slots, six votes
    assert m.place_mate(0, b"ACGT") == (0, 0, 0)
    assert m.place_mate(0, _rc(rec)) == (1, 0, 6)


def test_n_quality_mask_and_short_mate(oracle_lib):
    m = PlacementModel([R], 5)
    read = bytearray(R[3:15])
    read[6] = ord("N")                                    # slots 2 .. 6 hold it: 0, 1 and 7 vote
    assert m.place_mate(0, bytes(read)) == (0, 3, 3)
    assert m.place_mate(0, b"CACG") == (0, 0, 0)          # shorter than k
    # the same through a batch with -q 20: the base at 6 has quality 5, the pair's second mate is R[0:12] reversed, untouched
    q1 = bytearray(b"I" * 12)
    q1[6] = 33 + 5
    batch = synth.batch_from_lists([R[3:15]], [_rc(R[:12])], [bytes(q1)], [b"I" * 12])
    mates = list(masked_mates(batch, 20))
    assert mates[0][0][6] == R[9] - 64 and mates[0][1] == _rc(R[:12])
    got = expected_placements(m, batch, [0, 1], [0], 20)
    assert got.tolist() == [[[0, 3, 3], [1, 0, 8]]]
    assert expected_placements(m, synth.batch_from_lists([R[3:15]]), [0, 1], [0]).tolist() == [[[0, 3, 8], [0, 0, 0]]]   # single-end: mate 2 empty


def test_record_numbering_quirk(oracle_lib):
    r2 = b"ACGTTGCATGGACCTAACGTTGAGC"
    fasta = [b"NNNNNNNN", R, b"ACG", r2]                  # all-N (>= k, no k-mer): the counter stays; shorter than k: it advances
    assert gene_records(fasta, 5) == {0: R, 2: r2}
    m = PlacementModel(fasta, 5)
    assert m.place_mate(0, R[3:15]) == (0, 3, 8) and m.place_mate(2, r2[2:12]) == (0, 2, 6)
    assert m.place_mate(1, R[3:15]) == (0, 0, 0) and m.place_mate(2, b"GGGGGGGG") == (0, 0, 0)   # (id 1 has no record; r2 has no GGGGG / CCCCC)


def test_lines(oracle_lib):
    pl = np.array([[[0, 3, 8], [1, -2, 5]], [[0, 0, 0], [0, 7, 1]]], dtype=np.int64)
    assert placement_lines(["r0", "r1", "r2"], [0, 1, 1, 2], [1, 0], pl, ["gA", "gB"], True) == ["r0 gB 0 3 8 1 -2 5", "r2 gA 0 0 0 0 7 1"]
    assert placement_lines(["r0"], [0, 1], [1], pl, ["gA", "gB"], False) == ["r0 gB 0 3 8"]


def test_the_yardstick_is_not_vacuous(oracle_lib):
    """on the plain synthetic reference of the GPU tests, error-free reads drawn from a gene are placed on their true diagonal
    with support >= 1 for at least 95 % of the mates"""
    rng = np.random.default_rng(3)
    genes = synth.make_genes(rng, 100, 600, 1400)
    m = PlacementModel([bytes(g) for g in genes], 17)
    ok = total = 0
    for _ in range(400):
        gi = int(rng.integers(0, len(genes)))
        g = genes[gi]
        a = int(rng.integers(0, len(g) - 100))
        mate = bytes(g[a:a + 100])
        for rd, strand in ((mate, 0), (_rc(mate), 1)):
            s, pos, sup = m.place_mate(gi, rd)
            ok += int((s, pos) == (strand, a) and sup >= 1)
            total += 1
    assert total == 800 and ok >= 0.95 * total, (ok, total)


# ---------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------
NEW = ("shk_ref_keep_positions", "shk_placement_enable", "shk_placement_last")


def test_header_declares_and_binding_binds_the_new_calls():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "shark_hip.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    assert "typedef struct shk_mate_placement { int32_t pos; uint32_t support; uint32_t strand; } shk_mate_placement;" in hdr
    from shark_amd import EXPORTS, SharkHip
    assert set(NEW) <= set(EXPORTS)
    for name in ("keep_positions", "placement_enable", "placement_last"):
        assert callable(getattr(SharkHip, name))
    assert os.path.exists(LIB), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    import ctypes as C
    lib = C.CDLL(LIB)
    for s in NEW:
        assert hasattr(lib, s), s


def test_cli_placements_needs_a_value():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.join(ROOT, "shark_amd", "csrc"), "-j4", "all"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([CLI, "-r", "x.fa", "-1", "y.fq", "--placements"], capture_output=True, text=True)
    assert r.returncode == 1 and "placements" in r.stderr
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--placements FILE" in r.stderr
