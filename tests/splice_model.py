"""The yardstick for spliced ends (shk_splice_sites_set / shk_alignments_splice / `shark --splice-junctions`) -- include/shark_hip.h,
"alignments" step 3b.

Written from the header's text on top of tests/align_model.py (the record after step 3, the oriented read, the record's codes, step 4's
kinds) and tests/extend_model.py (step 3a, which runs afterwards):

  placement  a candidate is a LIST of record coordinates, one per evaluated read base, written out in full; its cost is the number of
             list entries whose base is not a match (a coordinate outside the record is not a match).  The null candidate is the list
             on the block's own diagonal.
  range      the candidates of an end come from two bisections of the gene's sorted sites (`ranged_candidates`);
             `naive_candidates` tries every site of the gene and keeps those whose resulting blocks are legal.  The CPU tests hold the
             two against each other.
  choice     all candidates are sorted by (cost, -d, -a); cost2 is a minimum over a filtered list.
  counting   the blocks' matches and mismatches counted anew over the final blocks.

No lanes, no ballots, no running best and second best: it shares no idea with the kernel.

Test infrastructure only."""
import bisect

import numpy as np

from shark_amd import capi
from tests.align_model import _kind, mate_alignment, oriented_codes, record_codes, to_record
from tests.extend_model import best_extension, check_params, extend_alignment
from tests.placement_model import masked_mates

MAX_OVERHANG = 48
BACK = 16
DEFAULTS = (3, 2, 2)                                            # the command's min_overhang, max_cost, min_gap


def check_splice(min_overhang, max_cost, min_gap):
    if not (0 <= min_overhang <= MAX_OVERHANG and 0 <= max_cost <= 64 and 0 <= min_gap <= 64):
        raise ValueError("min_overhang lies in 0 .. 48, max_cost and min_gap in 0 .. 64")


def check_sites(sites, lengths):
    """shk_splice_sites_set's SHK_ERR_ARG rules: sites is a list of (gene, donor, acceptor), lengths[g] = len_g"""
    sites = [tuple(int(v) for v in s) for s in sites]
    for i, (g, d, a) in enumerate(sites):
        if not (0 <= g < len(lengths) and 1 <= d < a <= lengths[g] - 1):
            raise ValueError("site %d lies outside its record" % i)
        if i and sites[i - 1] >= (g, d, a):
            raise ValueError("site %d does not ascend" % i)
    return sites


def sites_by_gene(sites):
    """{gene: [(d, a)] sorted}"""
    out = {}
    for g, d, a in sites:
        out.setdefault(int(g), []).append((int(d), int(a)))
    return {g: sorted(v) for g, v in out.items()}


def _cost(read, rec, ps, xs):
    return sum(1 for p, x in zip(ps, xs) if not (0 <= x < len(rec)) or _kind(int(read[p]), int(rec[x])) != "=")


def ranged_candidates(side, sites, x, q, ln, L, len_g):
    """the header's candidate rules by two bisections of the sorted sites; (x, q, ln): the last block (side 'right') or block 0"""
    B = min(BACK, ln - 1)
    if side == "right":
        xe, h = x + ln, L - (q + ln)
        lo = bisect.bisect_left(sites, (xe - B, -1))
        hi = bisect.bisect_right(sites, (xe + h - 1, 1 << 62))
        return [(d, a) for d, a in sites[lo:hi] if a + (xe + h - d) <= len_g]
    h = q
    by_a = sorted((a, d) for d, a in sites)
    lo = bisect.bisect_left(by_a, (x - h + 1, -1))
    hi = bisect.bisect_right(by_a, (x + B, 1 << 62))
    return sorted((d, a) for a, d in by_a[lo:hi] if d - (q - x + a) >= 0)


def naive_candidates(side, sites, x, q, ln, L, len_g):
    """every site of the gene is tried: it is a candidate iff the two blocks its placement gives are legal -- the near block is cut back
    by at most B bases, the far block holds at least one read base and lies inside the record"""
    B = min(BACK, ln - 1)
    out = []
    for d, a in sites:
        if side == "right":
            near = (x, q, ln + (d - (x + ln)))
            far = (a, q + near[2], L - (q + near[2]))
            ok = ln - B <= near[2] and far[2] >= 1 and far[0] + far[2] <= len_g
        else:
            n = q - x + a
            far = (d - n, 0, n)
            near = (a, n, ln - (a - x))
            ok = ln - B <= near[2] and far[2] >= 1 and far[0] >= 0
        if ok:
            out.append((d, a))
    return sorted(out)


def splice_end(side, read, rec, sites, block, L, params, stats=None, candidates=ranged_candidates):
    """one end of step 3b: None (the end stays as it is) or (near block, far block) as the header places them"""
    min_overhang, max_cost, min_gap = params
    x, q, ln = block
    len_g = len(rec)
    B = min(BACK, ln - 1)
    h = L - (q + ln) if side == "right" else q
    if not (min_overhang <= h <= MAX_OVERHANG):
        return None

    def bump(key):
        if stats is not None:
            stats[side + "_" + key] = stats.get(side + "_" + key, 0) + 1

    bump("attempted")
    if side == "right":
        ps = list(range(q + ln - B, L))
    else:
        ps = list(range(0, q + B))
    diag = [x + (p - q) for p in ps]
    priced = []
    for d, a in candidates(side, sites, x, q, ln, L, len_g):
        if side == "right":
            xs = [c if c < d else c + (a - d) for c in diag]
        else:
            xs = [c if c >= a else c - (a - d) for c in diag]
        priced.append((_cost(read, rec, ps, xs), -d, -a))
    if not priced:
        bump("no_candidate")
        return None
    priced.sort()
    cost, d, a = priced[0][0], -priced[0][1], -priced[0][2]
    cost2 = min([_cost(read, rec, ps, diag)] + [c for c, nd, na in priced if (-na) - (-nd) != a - d])
    if cost > max_cost:
        bump("too_costly")
        return None
    if cost2 - cost < min_gap:
        bump("ambiguous")
        return None
    bump("placed")
    if side == "right":
        xe, qe = x + ln, q + ln
        if d < xe:
            bump("shortened")
        return (x, q, ln + (d - xe)), (a, qe + (d - xe), h - (d - xe))
    if a > x:
        bump("shortened")
    n = q - x + a
    return (a, n, ln - (a - x)), (d - n, 0, n)


def splice_alignment(al, mate, record, sites, params, stats=None, candidates=ranged_candidates):
    """mate_alignment's tuple after step 3b (counts are those of the new blocks); sites: the gene's sorted [(d, a)]"""
    n, strand, _, _, blocks = al
    if n == 0 or params[0] == 0 or not sites:
        return al
    read, rec = oriented_codes(mate, strand), record_codes(record)
    L = len(read)
    blocks = [tuple(b) for b in blocks]
    gained = 0
    if len(blocks) <= 3:
        got = splice_end("left", read, rec, sites, blocks[0], L, params, stats, candidates)
        if got:
            blocks[0:1] = [got[1], got[0]]
            gained += 1
    if len(blocks) <= 3:
        got = splice_end("right", read, rec, sites, blocks[-1], L, params, stats, candidates)
        if got:
            blocks[-1:] = [got[0], got[1]]
            gained += 1
    if stats is not None and gained:
        stats["mates_gained"] = stats.get("mates_gained", 0) + 1
    matches = mismatches = 0
    for x, q, ln in blocks:
        assert ln >= 1 and 0 <= x and x + ln <= len(rec) and 0 <= q and q + ln <= L, (blocks, al)
        for t in range(ln):
            kind = _kind(int(read[q + t]), int(rec[x + t]))
            matches += kind == "="
            mismatches += kind == "X"
    for (xa, qa, la), (xb, qb, _) in zip(blocks, blocks[1:]):
        assert xa + la <= xb and qa + la <= qb
    return (len(blocks), strand, matches, mismatches, blocks)


def mate_alignment_spliced(mate, rows, k, s_min, record, sites, params, P, B, stats=None, ext_stats=None, candidates=ranged_candidates,
                           scorer=best_extension, align_stats=None, gaps=None):
    """steps 1 .. 3, 3b, 3a, 4 of one mate; params = (min_overhang, max_cost, min_gap), min_overhang == 0: step 3b is off.  stats are
    step 3b's counters, ext_stats step 3a's, align_stats and gaps align_model.mate_alignment's"""
    check_params(P, B)
    check_splice(*params)
    al = mate_alignment(mate, rows, k, s_min, record, align_stats, gaps)
    al = splice_alignment(al, mate, record, sites, params, stats, candidates)
    return al if P == 0 else extend_alignment(al, mate, record, P, B, ext_stats, scorer)


def expected_alignments_spliced(model, batch, gene_off, gene_ids, rows, s_min, sites, params, P=0, B=0, min_quality=0, stats=None,
                                candidates=ranged_candidates, scorer=best_extension, ext_stats=None, align_stats=None, gaps=None):
    """extend_model.expected_alignments_extended with step 3b in front of 3a: (n_assoc, 2) records of capi.ALIGNMENT_DTYPE.
    sites: a checked list of (gene, donor, acceptor); ext_stats, align_stats, gaps: mate_alignment_spliced's"""
    if s_min < 1:
        raise ValueError("min_support must be at least 1")
    per_gene = sites_by_gene(sites)
    gene_off = np.asarray(gene_off)
    out = np.zeros((int(gene_off[-1]) if len(gene_off) else 0, 2), dtype=capi.ALIGNMENT_DTYPE)
    for i, pair in enumerate(masked_mates(batch, min_quality)):
        for j in range(int(gene_off[i]), int(gene_off[i + 1])):
            g = int(gene_ids[j])
            record = model.records.get(g, b"")
            for t, mate in enumerate(pair):
                if mate is not None:
                    out[j, t] = to_record(mate_alignment_spliced(mate, rows[j, t], model.k, s_min, record, per_gene.get(g, []), params, P, B,
                                                                 stats, ext_stats, candidates, scorer, align_stats, gaps))
    return out


# ---------------------------------------------------------------------------
# the command: `shark --junctions` lines -> sites
# ---------------------------------------------------------------------------
def sites_from_junction_lines(lines, legend, lengths, min_mates=1):
    """`<gene> <donor> <acceptor> <intron> [<mates>]` per line -> the sorted, merged list of (gene, donor, donor + intron).  The site is
    the intron interval of the alignment blocks (the left block keeps the microhomology), not the file's acceptor column, which is the
    right span's lo and includes the overlap.  ValueError names the line that is malformed, names an unknown gene or lies outside its
    record"""
    index = {}
    for g, name in enumerate(legend):
        index.setdefault(name, g)                                # (a name given twice: the first record)
    out = set()
    for n, line in enumerate(lines, 1):
        f = line.split()
        if not f:
            continue
        try:
            if len(f) not in (4, 5):
                raise ValueError
            if not all(v.isascii() and v.isdigit() and len(v) <= 10 for v in f[1:]):    # (the command's rule: unsigned digit strings)
                raise ValueError
            d, a, intron = (int(v) for v in f[1:4])
            mates = int(f[4]) if len(f) == 5 else 1
        except ValueError:
            raise ValueError("line %d: malformed" % n)
        if f[0] not in index:
            raise ValueError("line %d: unknown gene" % n)
        g = index[f[0]]
        if not (1 <= d < d + intron <= lengths[g] - 1):
            raise ValueError("line %d: the site lies outside its record" % n)
        if mates >= min_mates:
            out.add((g, d, d + intron))
    return sorted(out)
