"""The yardstick for spliced depth (shk_depth_enable_spliced) and the device junction table (shk_junctions_enable /
shk_junctions_get) -- include/shark_hip.h "spliced depth and the junction table".

Written from the header's text on top of tests/segments_model.py's rows (m = 4):

  kept spans of a mate   its first four ranked segments with support >= s_min on rank 0's strand, as record spans [lo, hi)
  spliced depth          per counted mate a BOOLEAN MASK over its gene's record, set on every kept span and clipped by the record's
                         ends; the masks are added.  A base counts once per mate however many spans hold it; a mate counts iff its
                         mask has a base.  No difference array, no sorting, no running reach: it shares no idea with the kernel.
  junction table         a dict (gene, donor, acceptor) -> [smallest intron, mates] from shark_amd.capi.junctions at m = 4

Test infrastructure only."""
import numpy as np

from shark_amd import capi
from tests.depth_model import model_layout
from tests.segments_model import mate_lengths, span


def mate_mask(rows, L, k, s_min, len_g):
    """the bases of a record of len_g bytes that one mate of L bytes covers: bool[len_g]"""
    mask = np.zeros(len_g, dtype=bool)
    rows = [tuple(int(v) for v in r) for r in rows][:4]
    if not rows or rows[0][2] < max(1, s_min):
        return mask
    for r in rows:
        if r[2] >= s_min and r[2] >= 1 and r[0] == rows[0][0]:
            lo, hi = span(r, L, k)
            mask[max(lo, 0):max(min(hi, len_g), 0)] = True
    return mask


def expected_spliced_depth(model, batch, gene_off, gene_ids, rows, s_min):
    """(depth, mates) of one batch: the uint32 depth of every base in model_layout(model)'s order and the number of mates that
    covered at least one base.  rows: expected_segments(model, batch, gene_off, gene_ids, 4)[1]"""
    if s_min < 1:
        raise ValueError("min_support must be at least 1")
    gs = model_layout(model)
    depth = np.zeros(int(gs[-1]), dtype=np.uint32)
    lengths = mate_lengths(batch)
    gene_off = np.asarray(gene_off)
    mates = 0
    for i in range(len(gene_off) - 1):
        for j in range(int(gene_off[i]), int(gene_off[i + 1])):
            g = int(gene_ids[j])
            len_g = len(model.records.get(g, b""))
            for t in range(2):
                mask = mate_mask(rows[j, t], int(lengths[i, t]), model.k, s_min, len_g)
                if mask.any():
                    a = int(gs[g])
                    depth[a:a + len_g] += mask
                    mates += 1
    return depth, mates


def expected_junction_table(batch, gene_off, gene_ids, rows, k, s_min):
    """{(gene, donor, acceptor): [intron, mates]} of one batch; rows as above"""
    table = {}
    add_to_table(table, batch, gene_off, gene_ids, rows, k, s_min)
    return table


def add_to_table(table, batch, gene_off, gene_ids, rows, k, s_min):
    lengths = mate_lengths(batch)
    gene_off = np.asarray(gene_off)
    for i in range(len(gene_off) - 1):
        for j in range(int(gene_off[i]), int(gene_off[i + 1])):
            for t in range(2):
                for donor, acceptor, intron, _ in capi.junctions(rows[j, t], int(lengths[i, t]), k, s_min):
                    e = table.setdefault((int(gene_ids[j]), donor, acceptor), [intron, 0])
                    e[0] = min(e[0], intron)
                    e[1] += 1
    return table


def table_rows(table):
    """the dict as SharkHip.junctions_get hands the table out: rows (gene, donor, acceptor, intron, mates) sorted by key"""
    return [(g, d, a, table[(g, d, a)][0], table[(g, d, a)][1]) for g, d, a in sorted(table)]


def junction_table_lines(table, legend):
    """the lines of `shark --junctions`"""
    return ["%s %d %d %d %d" % (legend[g], d, a, i, n) for g, d, a, i, n in table_rows(table)]
