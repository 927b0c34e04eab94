"""Cases that the CPU and the GPU tests of spliced ends share (tests/test_splice_cpu.py, tests/test_gpu_splice.py): the genes of one
junction with their hand-worked mates, and the bundled example with the sites of its own junction table.

Test infrastructure only."""
import os

import numpy as np

from tests import synth
from tests.segments_model import SegmentsModel, expected_segments
from tests.splice_model import DEFAULTS, expected_alignments_spliced, sites_from_junction_lines
from tests.spliced_model import expected_junction_table, junction_table_lines

EXAMPLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "example")


def differs(*bases):
    return next(c for c in synth.ACGT if all(c != b for b in bases))


def junction_gene(rng, same, e1=80, intron=60, e2=80):
    """exon, intron, exon as one uint8 record: the intron's first `same` bases equal exon 2's, the next up to base 3 differ from them;
    its last four bases differ from exon 1's last four (so no base of a mate that crosses the junction matches by construction next
    to it on the wrong side)"""
    a, i, b = synth.random_seq(rng, e1), synth.random_seq(rng, intron), synth.random_seq(rng, e2)
    for t in range(4):
        i[t] = b[t] if t < same else differs(b[t])
        i[intron - 1 - t] = differs(a[e1 - 1 - t])
    return np.concatenate([a, i, b])


# the hand-worked mates of one junction gene s (exon [0, 80), intron [80, 140), exon [140, 220)) as (name, slice pairs, blocks with the
# site (80, 140) listed); on the gene with same = 3 and BOTH (80, 140) and (83, 143) listed the tie goes to the largest donor
ONE_JUNCTION = (
    ("right", ((20, 80), (140, 150)), [(20, 0, 60), (140, 60, 10)], [(20, 0, 63), (143, 63, 7)]),
    ("left", ((70, 80), (140, 200)), [(70, 0, 10), (140, 10, 60)], [(70, 0, 13), (143, 13, 57)]),
)


def cut(s, pieces):
    return np.concatenate([s[a:b] for a, b in pieces])


def example_spliced(oracle, fa, params=DEFAULTS, P=0, B=0, min_mates=1):
    """(model, batch, gene_off, gene_ids, sites, records without the step, records with it, stats): the bundled sample against the
    records `fa` at k = 17, c = 0.6, s_min = 8, with the sites of the sample's own junction table (the model's `shark --junctions`
    lines at floor 8, through the command's conversion)"""
    r1 = synth.read_fastq(os.path.join(EXAMPLE, "sample_1.fq"))
    r2 = synth.read_fastq(os.path.join(EXAMPLE, "sample_2.fq"))
    o = oracle.Shark(k=17, c=0.6, bf_bits=1 << 33)
    o.build([s for _, s in fa])
    batch = synth.batch_from_lists([s for _, s, _ in r1], [s for _, s, _ in r2])
    goff, gids = o.classify(batch["seq1"], batch["off1"], batch["seq2"], batch["off2"], None, None)
    sm = SegmentsModel([s for _, s in fa], 17)
    rows = expected_segments(sm, batch, goff, gids, 4)[1]
    legend = [n.decode() for n, _ in fa]
    lines = junction_table_lines(expected_junction_table(batch, goff, gids, rows, 17, 8), legend)
    sites = sites_from_junction_lines(lines, legend, [len(s) for _, s in fa], min_mates)
    st = {}
    plain = expected_alignments_spliced(sm, batch, goff, gids, rows, 8, [], (0, 0, 0), P, B)
    recs = expected_alignments_spliced(sm, batch, goff, gids, rows, 8, sites, params, P, B, stats=st)
    return sm, batch, goff, gids, lines, sites, plain, recs, st
