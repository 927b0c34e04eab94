"""The yardstick for variants mode (shk_ref_keep_bases / shk_variants_get / shk_variants_summary / `shark --variants`) --
include/shark_hip.h "variants".

Written from the header's text: one Python loop over the record positions, one position at a time, in Python integers (nothing can
overflow).  Inputs are the pileup counts in pileup_all()'s layout, the records by gene id, gene_start and the four parameters.  No
tiles, no ballots, no scan: it shares no idea with the kernels.

Test infrastructure only."""
import numpy as np

from shark_amd import capi
from tests.placement_model import _to_int

DEFAULTS = (8, 3, 1, 5)     # min_depth, min_alt, frac_num, frac_den: the command's


def _records(records):
    """{gene id: bytes} from a dict of that shape or from a list indexed by gene id"""
    if isinstance(records, dict):
        return {int(g): bytes(r) for g, r in records.items()}
    return {g: bytes(r) for g, r in enumerate(records)}


def check_params(params):
    min_depth, min_alt, num, den = (int(v) for v in params)
    if min_depth < 1 or min_alt < 1 or not 1 <= den <= 65535 or not 0 <= num <= den:
        raise ValueError("parameters outside min_depth >= 1, min_alt >= 1, 1 <= frac_den <= 65535, frac_num <= frac_den")
    return min_depth, min_alt, num, den


def expected_recbase(records):
    """uint8, one entry per record base, genes in id order (an id without a record has no base): to_int[byte] - 1 for a base, 4 otherwise"""
    to_int = _to_int()
    recs = _records(records)
    out = []
    for g in sorted(recs):
        out.extend(to_int[c] - 1 if to_int[c] else 4 for c in recs[g])
    return np.asarray(out, dtype=np.uint8)


def position(n, r, params):
    """one position by the header's rule: (alt, T, site) for counts n[0 .. 4) and record base r < 4"""
    min_depth, min_alt, num, den = params
    n = [int(v) for v in n]
    T = sum(n)
    alt = None
    for b in range(4):
        if b != r and (alt is None or n[b] > n[alt]):     # (strictly larger: ties stay with the smaller b)
            alt = b
    site = T >= min_depth and n[alt] >= min_alt and n[alt] * den >= num * T
    return alt, T, site


def _walk(counts, records, gene_start, params):
    """(g, x, r, n, alt, T, site) for every record position with r < 4, genes in id order, x ascending"""
    params = check_params(params)
    to_int = _to_int()
    recs = _records(records)
    counts = np.asarray(counts).reshape(-1, 4)
    for g in range(len(gene_start) - 1):
        a, len_g = int(gene_start[g]), int(gene_start[g + 1]) - int(gene_start[g])
        rec = recs.get(g, b"")
        assert len(rec) == len_g, (g, len(rec), len_g)
        for x in range(len_g):
            c = to_int[rec[x]]
            if c == 0:
                continue                                   # (r == 4: no part in anything)
            n = [int(v) for v in counts[a + x]]
            alt, T, site = position(n, c - 1, params)
            yield g, x, c - 1, n, alt, T, site


def expected_variants(counts, records, gene_start, params=DEFAULTS):
    """the sites as shk_variants_get hands them out: a structured array (capi.VARIANT_DTYPE) sorted by (gene, x)"""
    rows = [(g, x, r, alt, n) for g, x, r, n, alt, T, site in _walk(counts, records, gene_start, params) if site]
    out = np.zeros(len(rows), dtype=capi.VARIANT_DTYPE)
    for i, (g, x, r, alt, n) in enumerate(rows):
        out[i] = (g, x, r, alt, n)
    return out


def expected_summary(counts, records, gene_start, params=DEFAULTS):
    """per gene (observed, mismatches, covered, sites): a structured array (capi.GENE_VARIANTS_DTYPE) of len(gene_start) - 1 records"""
    min_depth = check_params(params)[0]
    acc = [[0, 0, 0, 0] for _ in range(len(gene_start) - 1)]
    for g, x, r, n, alt, T, site in _walk(counts, records, gene_start, params):
        acc[g][0] += T
        acc[g][1] += T - n[r]
        acc[g][2] += T >= min_depth
        acc[g][3] += bool(site)
    out = np.zeros(len(acc), dtype=capi.GENE_VARIANTS_DTYPE)
    for g, (obs, mis, cov, sites) in enumerate(acc):
        out[g] = (obs % (1 << 64), mis % (1 << 64), cov, sites)
    return out


def variant_lines(variants, legend):
    """the lines of `shark --variants`: <gene> <x> <ref> <alt> <A> <C> <G> <T> per site in the order given, ref and alt as letters"""
    return ["%s %d %s %s %d %d %d %d" % (legend[int(v["gene"])], int(v["x"]), "ACGT"[int(v["ref"])], "ACGT"[int(v["alt"])],
                                         int(v["n"][0]), int(v["n"][1]), int(v["n"][2]), int(v["n"][3])) for v in variants]
