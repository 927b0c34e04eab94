"""The yardstick for depth mode (shk_depth_enable / shk_depth_get_all / shk_depth_summary / `shark --depth`): per-base read depth
along each gene, include/shark_hip.h "depth".

Written from the semantics on top of tests/placement_model.py: for every association and mate whose placement has
support >= min_support, every base of [pos, pos + L) that lies inside the gene's record is incremented -- one association and one
mate at a time, over plain numpy slices.  No difference array and no prefix sum: it shares no idea with the kernels.

  layout   gene g at [gene_start[g], gene_start[g + 1]) of one array over all genes; an id without a record (main.cpp:160-187's
           numbering quirk) has length 0

Test infrastructure only."""
import numpy as np

from tests.placement_model import expected_placements, masked_mates


def model_layout(model, nidx=None):
    """gene_start (uint64, nidx + 1 entries) from the model's records; nidx defaults to the last id with a record, plus one"""
    n = (max(model.records) + 1 if model.records else 0) if nidx is None else int(nidx)
    gs = np.zeros(n + 1, dtype=np.uint64)
    for g in range(n):
        gs[g + 1] = gs[g] + np.uint64(len(model.records.get(g, b"")))
    return gs


def expected_depth(model, batch, gene_off, gene_ids, min_support, q=0):
    """(depth, mates): the uint32 depth of every base in model_layout(model)'s order after this one batch, and the number of
    (association, mate) intervals that were counted"""
    if min_support < 1:
        raise ValueError("min_support must be at least 1")
    gs = model_layout(model)
    depth = np.zeros(int(gs[-1]), dtype=np.uint32)
    placements = expected_placements(model, batch, gene_off, gene_ids, q)
    gene_off = np.asarray(gene_off)
    mates = 0
    for i, pair in enumerate(masked_mates(batch, q)):
        for j in range(int(gene_off[i]), int(gene_off[i + 1])):
            g = int(gene_ids[j])
            len_g = len(model.records.get(g, b""))
            for m, mate in enumerate(pair):
                if mate is None:
                    continue
                _, pos, support = (int(v) for v in placements[j, m])
                if support < min_support:
                    continue
                lo, hi = max(pos, 0), min(pos + len(mate), len_g)
                if hi <= lo:
                    continue
                a = int(gs[g])
                depth[a + lo:a + hi] += 1
                mates += 1
    return depth, mates


def depth_summary(depth, gene_start):
    """[(len, covered, max, sum)] per gene -- what SharkHip.depth_summary reports in its fields of those names"""
    out = []
    for g in range(len(gene_start) - 1):
        d = np.asarray(depth[int(gene_start[g]):int(gene_start[g + 1])], dtype=np.uint64)
        out.append((len(d), int((d > 0).sum()), int(d.max()) if len(d) else 0, int(d.sum())))
    return out


def depth_lines(depth, gene_start, legend):
    """the lines of `shark --depth`: <gene> <start> <end> <depth> per maximal run of equal depth >= 1, 0-based half-open, genes in
    id order, runs in coordinate order"""
    lines = []
    for g in range(len(gene_start) - 1):
        d = [int(v) for v in depth[int(gene_start[g]):int(gene_start[g + 1])]]
        x = 0
        while x < len(d):
            e = x
            while e < len(d) and d[e] == d[x]:
                e += 1
            if d[x] >= 1:
                lines.append("%s %d %d %d" % (legend[g], x, e, d[x]))
            x = e
    return lines
