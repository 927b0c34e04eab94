"""Spliced depth and the junction table without a GPU: the pure functions of the binding (kept_spans, span_union) and the model
(tests/spliced_model.py) on cases worked out by hand, the bundled example, and the boundary -- the four new symbols in the header and
the binding, the new flags of the command."""
import os
import re
import subprocess

import numpy as np
import pytest

from shark_amd import capi
from tests import synth
from tests.segments_model import SegmentsModel, expected_segments, junction_lines, mate_lengths
from tests.spliced_model import expected_junction_table, expected_spliced_depth, junction_table_lines, mate_mask, table_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "shark_amd", "libsharkhip.so")
CLI = os.path.join(ROOT, "shark_amd", "bin", "shark")
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example")

# test_segments_cpu.py's record: 60 bases, 56 windows of 5 with 56 different canonical 5-mers; G[14:17] == G[30:33]
#        0         1         2         3         4         5
#        012345678901234567890123456789012345678901234567890123456789
G = b"ATCCGAGTTCGGTCGCCGGAGACATGCTGAGCCTTGCATACACAGATAAGATCGTGCTCT"
K = 5


def _rc(b):
    return bytes(synth.revcomp(np.frombuffer(bytes(b), np.uint8)))


def _mask_runs(mask):
    """[(lo, hi)] of the runs of True"""
    d = np.diff(np.concatenate([[0], np.asarray(mask, dtype=np.int8), [0]]))
    return list(zip(np.nonzero(d == 1)[0].tolist(), np.nonzero(d == -1)[0].tolist()))


def _both(rows, L, k, s_min, len_g):
    """the union of a mate's kept spans, from the binding and from the model's mask: they must agree"""
    u = capi.span_union(capi.kept_spans(rows, L, k, s_min), len_g)
    assert u == _mask_runs(mate_mask(rows, L, k, s_min, len_g))
    return u


def test_the_worked_example_of_the_header():
    rows = [(1, 9653, 58, 26, 83), (1, 10843, 15, 0, 14)]
    assert capi.kept_spans(rows, 100, 17, 8) == [(9653, 9727, 9653), (10912, 10943, 10843)]
    assert capi.kept_spans(rows[::-1], 100, 17, 8) == [(9653, 9727, 9653), (10912, 10943, 10843)]
    assert _both(rows, 100, 17, 8, 20000) == [(9653, 9727), (10912, 10943)]          # 74 + 31 bases, none of the 1185 in between
    assert capi.kept_spans(rows, 100, 17, 16) == [(9653, 9727, 9653)]
    assert capi.junctions(rows, 100, 17, 8) == [(9727, 10912, 1190, 5)]
    # plain depth paints [9653, 9753) along rank 0 alone: 26 bases of intron


def test_unions_by_hand():
    # disjoint, touching, overlapping, one span inside another; clipped at both ends of the record
    assert capi.span_union([(4, 14), (36, 46)], 60) == [(4, 14), (36, 46)]
    assert capi.span_union([(4, 14), (14, 20)], 60) == [(4, 20)]
    assert capi.span_union([(4, 14), (10, 20)], 60) == [(4, 20)]
    assert capi.span_union([(4, 30), (10, 20)], 60) == [(4, 30)]
    assert capi.span_union([(4, 30), (10, 20), (25, 40), (50, 70)], 60) == [(4, 40), (50, 60)]
    assert capi.span_union([(-3, 5, 99), (2, 4, 7)], 60) == [(0, 5)]              # (rows may carry their pos behind lo, hi)
    assert capi.span_union([(60, 70)], 60) == [] and capi.span_union([], 60) == []
    # the same four shapes as segments of a mate of 20 bytes on strand 0 (lo = pos + first, hi = pos + last + 5)
    for L, rows, want in ((20, [(0, 4, 6, 0, 5), (0, 26, 6, 10, 15)], [(4, 14), (36, 46)]),
                          (20, [(0, 4, 6, 0, 5), (0, 4, 6, 10, 11)], [(4, 20)]),
                          (20, [(0, 4, 6, 0, 5), (0, 3, 6, 7, 12)], [(4, 20)]),
                          (30, [(0, 4, 22, 0, 21), (0, 3, 6, 7, 12)], [(4, 30)])):
        assert _both(rows, L, K, 6, 60) == want
        d = mate_mask(rows, L, K, 6, 60)
        assert int(d.sum()) == sum(hi - lo for lo, hi in want)               # every base once


def test_kept_span_edge_cases():
    spliced = [(0, 4, 6, 0, 5), (0, 26, 6, 10, 15), (0, 0, 0, 0, 0), (0, 0, 0, 0, 0)]
    assert capi.kept_spans(spliced, 20, K, 6) == [(4, 14, 4), (36, 46, 26)]
    # rank 0 below s_min gives nothing (ranks descend in support)
    assert capi.kept_spans(spliced, 20, K, 7) == [] and _both(spliced, 20, K, 7, 60) == []
    assert capi.kept_spans([(0, 0, 0, 0, 0)] * 4, 20, K, 1) == []
    # a lower rank on the other strand is dropped
    rows = [(1, 10, 5, 8, 12), (0, 2, 4, 0, 3)]
    assert capi.kept_spans(rows, 17, K, 1) == [(10, 19, 10)] and _both(rows, 17, K, 1, 26) == [(10, 19)]
    # a fifth diagonal is ignored: the kept spans are defined on the first four ranks
    five = [(0, 0, 9, 0, 8), (0, 100, 8, 20, 27), (0, 200, 7, 40, 46), (0, 300, 6, 60, 65), (0, 400, 6, 80, 85)]
    assert [sp[2] for sp in capi.kept_spans(five, 100, K, 1)] == [0, 100, 200, 300]
    assert _both(five, 100, K, 1, 1000) == [(0, 13), (120, 132), (240, 251), (360, 370)]
    # sorted by (lo, hi), whatever the ranks say
    assert capi.kept_spans([(0, 26, 7, 10, 15), (0, 4, 6, 0, 5)], 20, K, 6) == [(4, 14, 4), (36, 46, 26)]


def test_the_model_on_spliced_reads_by_hand(oracle):
    oracle.lib()
    m = SegmentsModel([G], K)
    # one intron on either strand; microhomology (G[14:17] == G[30:33]: the first span runs on to 17); two introns
    reads = [G[4:14] + G[36:46], _rc(G[4:14] + G[36:46]), G[4:14] + G[30:40], G[4:14] + G[24:33] + G[44:54], G[:4]]
    batch = synth.batch_from_lists(reads)
    goff, gids = np.arange(len(reads) + 1), [0] * len(reads)
    _, rows = expected_segments(m, batch, goff, gids, 4)
    depth, mates = expected_spliced_depth(m, batch, goff, gids, rows, 5)
    want = np.zeros(60, dtype=np.uint32)
    for lo, hi in ((4, 14), (36, 46), (4, 14), (36, 46), (4, 17), (30, 40), (4, 14), (24, 33), (44, 54)):
        want[lo:hi] += 1
    assert depth.tolist() == want.tolist() and mates == 4
    assert table_rows(expected_junction_table(batch, goff, gids, rows, K, 5)) == [(0, 14, 24, 10, 1), (0, 14, 36, 22, 2), (0, 17, 30, 16, 1), (0, 33, 44, 11, 1)]
    # a floor of 6 drops the middle exon of the fourth read: its outer two are consecutive
    depth6, mates6 = expected_spliced_depth(m, batch, goff, gids, rows, 6)
    want[24:33] -= 1
    assert depth6.tolist() == want.tolist() and mates6 == 4
    assert table_rows(expected_junction_table(batch, goff, gids, rows, K, 6)) == [(0, 14, 36, 22, 2), (0, 14, 44, 21, 1), (0, 17, 30, 16, 1)]
    assert expected_spliced_depth(m, batch, goff, gids, rows, 10)[1] == 0


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
    return fa, batch, goff, gids, sm, rows


# the model's figures on the example (k = 17, c = 0.6, s_min = 8): test_segments_cpu.py's 9 keys and 468 + 535 observations; the total
# length of the counted mates' span unions, and the mates counted
EXAMPLE_DISTINCT = 9
EXAMPLE_OBSERVATIONS = 468 + 535
EXAMPLE_UNION_BASES = 378301
EXAMPLE_MATES = 3858


def test_the_example_table_and_depth(example):
    fa, batch, goff, gids, sm, rows = example
    legend = [n.decode() for n, _ in fa]
    table = expected_junction_table(batch, goff, gids, rows, 17, 8)
    assert len(table) == EXAMPLE_DISTINCT and sum(e[1] for e in table.values()) == EXAMPLE_OBSERVATIONS
    assert junction_table_lines(table, legend) == junction_lines(goff, gids, rows, mate_lengths(batch), 17, legend, 8)
    depth, mates = expected_spliced_depth(sm, batch, goff, gids, rows, 8)
    # the per-gene sum is the total length of the mates' span unions (the binding's functions, interval arithmetic)
    lengths = mate_lengths(batch)
    read_of = np.repeat(np.arange(len(goff) - 1), np.diff(goff))
    per_gene, counted = {}, 0
    for j in range(int(goff[-1])):
        g = int(gids[j])
        for t in range(2):
            u = capi.span_union(capi.kept_spans(rows[j, t], int(lengths[read_of[j], t]), 17, 8), len(sm.records.get(g, b"")))
            per_gene[g] = per_gene.get(g, 0) + sum(hi - lo for lo, hi in u)
            counted += bool(u)
    from tests.depth_model import depth_summary, model_layout
    summary = depth_summary(depth, model_layout(sm))
    assert [s[3] for s in summary] == [per_gene.get(g, 0) for g in range(len(summary))]
    print("example: union bases", int(depth.sum()), "mates", mates)
    assert (int(depth.sum()), mates) == (EXAMPLE_UNION_BASES, EXAMPLE_MATES) and counted == mates


# ---------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------
NEW = ("shk_depth_enable_spliced", "shk_junctions_enable", "shk_junctions_get", "shk_junctions_reset")


def test_header_declares_and_binding_binds_the_new_calls():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "shark_hip.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    assert "typedef struct shk_junction { uint32_t gene, donor, acceptor, intron; uint64_t mates; } shk_junction;" in hdr
    from shark_amd import EXPORTS, SharkHip
    assert set(NEW) <= set(EXPORTS) and capi.JUNCTION_DTYPE.itemsize == 24
    for name in ("depth_enable_spliced", "junctions_enable", "junctions_get", "junctions_reset"):
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
    r = run("--depth-spliced")
    assert r.returncode == 1 and "--depth-spliced needs --depth FILE" in r.stderr
    r = run("--junctions-device")
    assert r.returncode == 1 and "--junctions-device needs --junctions FILE" in r.stderr
    r = run("--junctions", "j", "--junctions-capacity", "64")
    assert r.returncode == 1 and "--junctions-capacity needs --junctions-device" in r.stderr
    r = run("--junctions", "j", "--junctions-device", "--junctions-capacity", "0")
    assert r.returncode == 1 and "--junctions-capacity must be in the range" in r.stderr
    for m in ("1", "3"):
        r = run("--junctions", "j", "--junctions-device", "--segments-max", m)
        assert r.returncode == 1 and "--junctions-device needs --segments-max 4" in r.stderr
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--depth-spliced" in r.stderr and "--junctions-device" in r.stderr and "--junctions-capacity N" in r.stderr
