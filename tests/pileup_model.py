"""The yardstick for pileup mode (shk_pileup_enable / shk_pileup_get_all / `shark --pileup`) -- include/shark_hip.h "pileup".

Written from the header's text on top of tests/segments_model.py's rows (m = 4) and the masked mates of tests/placement_model.py:

  per mate     an int8 array over its gene's record, -1 everywhere.  The kept spans are visited in sorted order and a span writes
               only coordinates that still hold -1: ownership by FIRST WRITER.  What it writes is the base the mate shows there on
               the record's strand (0 .. 3), or 4 where the mate's byte is no base (an N, a byte masked by -q).
  counts       the mates' arrays added up: counts[x][b] += 1 where the array holds b < 4; lost[x] += 1 where it holds 4
  pileup mate  a mate whose array holds anything but -1

No running reach, no clipping arithmetic on pieces, no per-lane passes: it shares no idea with the kernel.

Test infrastructure only."""
import numpy as np

from shark_amd import capi
from tests.depth_model import model_layout
from tests.placement_model import _to_int, masked_mates


def mate_alleles(mate, rows, k, s_min, len_g):
    """int8[len_g] of one masked mate (bytes) with its segment rows (strand, pos, support, first, last): -1 not owned, 0 .. 3 the
    base it shows on the record's strand, 4 owned by a byte that is no base"""
    to_int = np.asarray(_to_int(), dtype=np.int8)
    L = len(mate)
    seen = np.full(len_g, -1, dtype=np.int8)
    spans = capi.kept_spans(rows, L, k, s_min)
    if not spans:
        return seen
    strand = int(rows[0][0])                                    # (rank 0's: every kept span lies on it)
    codes = to_int[np.frombuffer(bytes(mate), dtype=np.uint8)]  # 0: no base; 1 .. 4: A, C, G, T
    for lo, hi, pos in spans:
        xs = np.arange(max(lo, 0), max(min(hi, len_g), 0))
        xs = xs[seen[xs] == -1]                                 # (first writer: what an earlier span holds stays)
        i = xs - pos if strand == 0 else pos + L - 1 - xs
        assert ((0 <= i) & (i < L)).all(), (lo, hi, pos, L, strand)   # (the header: a span lies inside [pos, pos + L))
        c = codes[i]
        seen[xs] = np.where(c == 0, 4, c - 1 if strand == 0 else 3 - (c - 1))
    return seen


def add_mate(counts, lost, a, seen):
    """adds one mate's array to counts[(n_bases, 4)] / lost[n_bases] at base offset a; True iff the mate owned a base"""
    xs = np.nonzero(seen >= 0)[0]
    obs = xs[seen[xs] < 4]
    counts[a + obs, seen[obs]] += 1                             # (one entry per x: no index repeats)
    lost[a + xs[seen[xs] == 4]] += 1
    return len(xs) > 0


def expected_pileup(model, batch, gene_off, gene_ids, rows, s_min, min_quality=0):
    """(counts, lost, mates) of one batch: uint32 (n_bases, 4) observations and uint32 (n_bases,) owned bytes that are no base, in
    model_layout(model)'s order, and the pileup mates.  rows: expected_segments(model, batch, gene_off, gene_ids, 4, min_quality)[1]"""
    if s_min < 1:
        raise ValueError("min_support must be at least 1")
    gs = model_layout(model)
    counts = np.zeros((int(gs[-1]), 4), dtype=np.uint32)
    lost = np.zeros(int(gs[-1]), dtype=np.uint32)
    gene_off = np.asarray(gene_off)
    mates = 0
    for i, pair in enumerate(masked_mates(batch, min_quality)):
        for j in range(int(gene_off[i]), int(gene_off[i + 1])):
            g = int(gene_ids[j])
            len_g = len(model.records.get(g, b""))
            for t, mate in enumerate(pair):
                if mate is None:
                    continue
                mates += add_mate(counts, lost, int(gs[g]), mate_alleles(mate, rows[j, t], model.k, s_min, len_g))
    return counts, lost, mates


def pileup_lines(counts, gene_start, legend):
    """the lines of `shark --pileup`: <gene> <x> <A> <C> <G> <T> per record base with at least one observation, x 0-based, genes in
    id order, x ascending"""
    lines = []
    for g in range(len(gene_start) - 1):
        a = int(gene_start[g])
        for x in range(int(gene_start[g + 1]) - a):
            c = [int(v) for v in counts[a + x]]
            if any(c):
                lines.append("%s %d %d %d %d %d" % (legend[g], x, c[0], c[1], c[2], c[3]))
    return lines
