"""Cases that the CPU and the GPU tests of end extension and aligned pileup share (tests/test_extend_cpu.py, tests/test_gpu_extend.py).

Test infrastructure only."""
import os

import numpy as np

from tests import synth
from tests.extend_model import expected_alignments_extended
from tests.segments_model import SegmentsModel, expected_segments

EXAMPLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "example")


def substituted(seq, *at):
    """seq (bytes) with the bases at the given indices replaced by the first of A, C, G, T that differs"""
    s = bytearray(seq)
    for i in at:
        s[i] = next(c for c in b"ACGT" if c != s[i])
    return bytes(s)


def tiling_case(L=100, k=17, seed=21):
    """(record, site, reads): one gene, a site in its interior, and for every read offset 0 .. L - 1 of the site one mate with the
    record's base there and one with a substituted base"""
    rec = bytes(synth.random_seq(np.random.default_rng(seed), 400))
    site = 200
    reads = []
    for i in range(L):
        m = rec[site - i:site - i + L]
        reads += [m, substituted(m, i)]
    return rec, site, reads


def example_alignments(oracle, fa, P, B):
    """(model, batch, gene_off, gene_ids, records, stats): the bundled sample against the records `fa` ([(name, bytes)]) by the oracle and
    the model at k = 17, c = 0.6, s_min = 8 and extension (P, B)"""
    r1 = synth.read_fastq(os.path.join(EXAMPLE, "sample_1.fq"))
    r2 = synth.read_fastq(os.path.join(EXAMPLE, "sample_2.fq"))
    o = oracle.Shark(k=17, c=0.6, bf_bits=1 << 33)
    o.build([s for _, s in fa])
    batch = synth.batch_from_lists([s for _, s, _ in r1], [s for _, s, _ in r2])
    goff, gids = o.classify(batch["seq1"], batch["off1"], batch["seq2"], batch["off2"], None, None)
    sm = SegmentsModel([s for _, s in fa], 17)
    rows = expected_segments(sm, batch, goff, gids, 4)[1]
    st = {}
    recs = expected_alignments_extended(sm, batch, goff, gids, rows, 8, P, B, stats=st)
    return sm, batch, goff, gids, recs, st


