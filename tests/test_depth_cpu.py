"""Depth mode without a GPU: the model (tests/depth_model.py) on cases worked out by hand over one 60-base gene with k = 5, the
lines of `shark --depth`, and the boundary -- the seven new symbols in the header and the binding, `--depth` in the command."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import synth
from tests.depth_model import depth_lines, depth_summary, expected_depth, model_layout
from tests.placement_model import PlacementModel, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "shark_amd", "libsharkhip.so")
CLI = os.path.join(ROOT, "shark_amd", "bin", "shark")

# 60 bases whose 56 windows of 5 have 56 different canonical 5-mers (k odd: no window is its own reverse complement)
#        0         1         2         3         4         5
#        012345678901234567890123456789012345678901234567890123456789
G = b"TCCGCGTCCCTGCTCCTTGAGCTGGGCCGCTTCGAGAAAATATAGTAACCCAAGAACAAA"


def _rc(b):
    return bytes(synth.revcomp(np.frombuffer(bytes(b), np.uint8)))


@pytest.fixture(scope="module")
def model(oracle):
    oracle.lib()
    return PlacementModel([G], 5)


def _one(model, m1, m2=None, min_support=1):
    """depth (as a list) and counted mates of one read (pair) associated with gene 0"""
    batch = synth.batch_from_lists([m1], [m2] if m2 is not None else None)
    d, mates = expected_depth(model, batch, [0, 1], [0], min_support)
    return d.tolist(), mates


def test_the_record_is_what_the_cases_assume(model):
    w = windows(G, 5)
    assert len(G) == 60 and [p for p, _, _ in w] == list(range(56)) and len({c for _, c, _ in w}) == 56
    assert model_layout(model).tolist() == [0, 60]


def test_a_mate_inside_the_gene(model):
    assert model.place_mate(0, G[10:30]) == (0, 10, 16)
    assert _one(model, G[10:30]) == ([0] * 10 + [1] * 20 + [0] * 30, 1)


def test_a_mate_overhanging_the_start(model):
    # four foreign bases in front of G[0:12]: pos = -4, L = 16, [-4, 12) clips to [0, 12)
    assert model.place_mate(0, b"AAAA" + G[:12]) == (0, -4, 8)
    assert _one(model, b"AAAA" + G[:12]) == ([1] * 12 + [0] * 48, 1)


def test_a_mate_overhanging_the_end(model):
    # G[50:60] and four foreign bases: pos = 50, L = 14, [50, 64) clips to [50, 60)
    assert model.place_mate(0, G[50:] + b"CCCC") == (0, 50, 6)
    assert _one(model, G[50:] + b"CCCC") == ([0] * 50 + [1] * 10, 1)


def test_a_reverse_strand_mate(model):
    # pos is the leftmost record base on either strand: the interval is the forward mate's
    assert model.place_mate(0, _rc(G[20:40])) == (1, 20, 16)
    assert _one(model, _rc(G[20:40])) == ([0] * 20 + [1] * 20 + [0] * 20, 1)


def test_a_pair_whose_mates_overlap_counts_two_on_the_overlap(model):
    assert _one(model, G[5:25], _rc(G[15:35])) == ([0] * 5 + [1] * 10 + [2] * 10 + [1] * 10 + [0] * 25, 2)


def test_a_mate_below_min_support_does_not_count(model):
    assert model.place_mate(0, G[10:17]) == (0, 10, 3)              # 7 bases: three slots
    assert _one(model, G[10:17], min_support=3) == ([0] * 10 + [1] * 7 + [0] * 43, 1)
    assert _one(model, G[10:17], min_support=4) == ([0] * 60, 0)
    # of a pair only the mate that reaches it: mate 1 has 16 votes, mate 2 three
    assert _one(model, G[30:50], G[10:17], min_support=4) == ([0] * 30 + [1] * 20 + [0] * 10, 1)
    # a mate shorter than k and a mate without a hit have support 0
    assert _one(model, b"TCCG", b"AAAAAAAAAAAA") == ([0] * 60, 0)
    with pytest.raises(ValueError):
        _one(model, G[10:30], min_support=0)


def test_a_tied_read_counts_in_each_gene_and_an_id_without_a_record_has_length_zero(oracle):
    oracle.lib()
    m = PlacementModel([b"NNNNNNNN", G, b"ACG", G], 5)     # all-N: the counter stays; shorter than k: id 1, no record
    assert sorted(m.records) == [0, 2] and model_layout(m).tolist() == [0, 60, 60, 120] and model_layout(m, 3).tolist() == [0, 60, 60, 120]
    batch = synth.batch_from_lists([G[10:30]])
    d, mates = expected_depth(m, batch, [0, 3], [0, 1, 2], 1)
    assert d.tolist() == ([0] * 10 + [1] * 20 + [0] * 30) * 2 and mates == 2
    assert depth_summary(d, model_layout(m)) == [(60, 20, 1, 20), (0, 0, 0, 0), (60, 20, 1, 20)]


def test_summary_and_run_length_lines_with_a_zero_gap():
    depth = np.array([0, 0, 1, 1, 2, 2, 2, 1, 0, 0, 0, 3, 3, 0] + [5, 5, 5] + [0, 0], dtype=np.uint32)
    gene_start = [0, 14, 14, 17, 19]
    assert depth_summary(depth, gene_start) == [(14, 8, 3, 15), (0, 0, 0, 0), (3, 3, 5, 15), (2, 0, 0, 0)]
    assert depth_lines(depth, gene_start, ["gA", "gB", "gC", "gD"]) == ["gA 2 4 1", "gA 4 7 2", "gA 7 8 1", "gA 11 13 3", "gC 0 3 5"]


# ---------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------
NEW = ("shk_depth_enable", "shk_depth_layout", "shk_depth_get", "shk_depth_get_all", "shk_depth_summary", "shk_depth_mates", "shk_depth_reset")


def test_header_declares_and_binding_binds_the_new_calls():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "shark_hip.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    assert hdr.index("shk_placement_last") < hdr.index("shk_depth_enable") < hdr.index("shk_gene_counts")
    from shark_amd import EXPORTS, SharkHip
    from shark_amd.capi import GENE_DEPTH_DTYPE
    assert set(NEW) <= set(EXPORTS)
    assert GENE_DEPTH_DTYPE.itemsize == 24 and GENE_DEPTH_DTYPE.fields["sum"][1] == 16
    for name in ("depth_enable", "depth_layout", "depth", "depth_all", "depth_summary", "depth_mates", "depth_reset"):
        assert callable(getattr(SharkHip, name))
    assert os.path.exists(LIB), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    import ctypes as C
    lib = C.CDLL(LIB)
    for s in NEW:
        assert hasattr(lib, s), s


def test_cli_depth_is_parsed_and_refused(tmp_path):
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.join(ROOT, "shark_amd", "csrc"), "-j4", "all"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([CLI, "-r", "x.fa", "-1", "y.fq", "--depth"], capture_output=True, text=True)
    assert r.returncode == 1 and "depth" in r.stderr
    r = subprocess.run([CLI, "-r", "x.fa", "-1", "y.fq", "--depth", "d.txt", "--depth-min-support", "0"], capture_output=True, text=True)
    assert r.returncode == 1 and "shark: --depth-min-support must be at least 1." in r.stderr
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--depth FILE" in r.stderr and "--depth-min-support N" in r.stderr
    # the samples are there, the depth file cannot be opened: a message and exit code 1 before any work is done
    fq = tmp_path / "a.fq"
    fq.write_text("@r\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n")
    fa = tmp_path / "g.fa"
    fa.write_text(">g\nACGTACGTACGTACGTACGTACGT\n")
    r = subprocess.run([CLI, "-r", str(fa), "-1", str(fq), "-o", str(tmp_path / "o"), "--depth", str(tmp_path / "no" / "such" / "d.txt")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "cannot open the depth file" in r.stderr
